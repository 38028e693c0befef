"""The cases behind tests/golden/conv3d_routes.json (tools/gen_conv3d_routes.py records them, tests/test_conv3d_route_cpu.py and
tests/test_gpu_conv3d_route.py read them back, tools/ab_routes.py compares two builds' bits on them).

(a) forward cases: the `label|kernel` list of bench.profiled_forward for a formula-weights network.
(b) single-layer cases: the smallest shapes at which each kernel family's geometry can go wrong, each under the epilogues the
    layer has in a forward -- statistics (a contract block's conv before its InstanceNorm), LeakyReLU + hash dropout (MC-dropout),
    activation only (dropout off), LeakyReLU + mask dropout (injected masks)."""
import ctypes as C

GOLDEN = "conv3d_routes.json"

# ---- (a) ---------------------------------------------------------------------------------------------------------------------
# (id, volume shape, network kwargs, vx_config fields); F = 8 and T = 2 unless the id says otherwise.  (16, 16, 64) is the smallest
# shape whose level 1 reaches the 16-channel z-column kernel and whose level 2 reaches the deep kernel.
_VARIANTS = [("default", {}, {}), ("nodrop", dict(do_dropout=False), {}), ("nonorm", dict(do_instancenorm=False), {}),
             ("cls5", dict(num_classes=5), {}),
             ("skip_raw0", {}, dict(s16_skip_raw=0)), ("no_prenorm", {}, dict(s16_no_prenorm=1)), ("no_xp8", {}, dict(s16_no_xp8=1)),
             ("no_upfuse", {}, dict(s16_no_upfuse=1)), ("no_head_fusion", {}, dict(no_head_fusion=1)),
             ("no_poolfuse", {}, dict(s16_no_poolfuse=1)), ("no_deep", {}, dict(s16_no_deep=1)), ("no_l1dma", {}, dict(s16_no_l1dma=1)),
             ("no_zc16", {}, dict(s16_no_zc16=1)), ("no_halves", {}, dict(s16_no_halves=1)), ("fp32", {}, dict(conv_fp32=1)),
             ("storage16_1", {}, dict(storage16=1)), ("storage16_2", {}, dict(storage16=2))]
FORWARD_T, FORWARD_SEED = 2, 4242
FORWARD_CASES = [(f"{n}@{'x'.join(map(str, s))}", s, kw, cfg) for s in ((32, 32, 32), (16, 16, 64)) for n, kw, cfg in _VARIANTS]
FORWARD_CASES += [(f"F{f}@32x32x32", (32, 32, 32), dict(initial_filter_size=f), {}) for f in (16, 32)]


def forward_model(kw):
    """values_amd.UNet3D with the formula weights (tests/test_gpu_unet3d.py make_model, any class count / width)"""
    import torch
    from tests.formula import formula_unet3d_state_dict
    from values_amd import UNet3D
    kw = dict(dict(num_classes=2, do_dropout=True), **kw)
    sd = formula_unet3d_state_dict(seed_tag=0, num_classes=kw["num_classes"], f=kw.get("initial_filter_size", 8))
    m = UNet3D(**kw)
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in sd.items()}, strict=True)
    return m.cuda()


def forward_input(shape):
    import torch
    from tests.formula import formula_volume
    return torch.from_numpy(formula_volume((1, 1) + tuple(shape), tag=11)).float().cuda()


def forward_rows(model, x):
    import bench
    return [f"{lab}|{name}" for lab, name, _ in bench.profiled_forward(model, x, FORWARD_T, FORWARD_SEED)]


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
EPILOGUES = ("stats", "lrelu_hash", "lrelu", "lrelu_mask")
LAYER_N = 2
_FAMILIES = [
    ("xp8w", {}, [(8, 8, 32), (12, 16, 64)], [(8, 8), (16, 8)]),
    ("zc16", {}, [(4, 8, 32), (6, 16, 64)], [(8, 16), (16, 16)]),
    # (6, 8, 8): three tiles that do not divide the four-entry statistics buffer -- the statistics launch must fall through
    ("deep", {}, [(4, 4, 16), (8, 8, 8), (16, 16, 16), (32, 32, 32), (6, 8, 8)], [(16, 32), (32, 32), (64, 64)]),
    ("s16", {}, [(5, 7, 9), (16, 16, 16), (32, 32, 32)], [(32, 16), (8, 32), (24, 8)]),
    ("fp32", dict(conv_fp32=1), [(5, 7, 9), (8, 8, 16)], [(16, 8), (24, 8), (16, 16)]),
]
LAYER_CASES = [dict(id=f"{fam}:{'x'.join(map(str, s))}:{ci}->{co}:{e}", cfg=cfg, shape=s, cin=ci, cout=co, epilogue=e)
               for fam, cfg, shapes, layers in _FAMILIES for s in shapes for ci, co in layers for e in EPILOGUES]


def layer_args(lib, case, ptr):
    """vx_conv3d_args of a single-layer case: a dense launch, N = LAYER_N.  ptr(name) gives the address of a buffer (a real tensor
    for a launch, any 16-byte aligned non-null number for the dry run); the weights' family is asked of `lib`, under the
    configuration that is set NOW."""
    from values_amd import _lib
    D, H, W = case["shape"]
    a = _lib.ConvArgs()
    a.in_, a.w_packed, a.bias, a.out = ptr("in"), ptr("w_packed"), ptr("bias"), ptr("out")
    a.in_pitch, a.out_pitch, a.out_coff = case["cin"], case["cout"], 0
    a.N, a.D, a.H, a.W, a.Cin, a.Cout = LAYER_N, D, H, W, case["cin"], case["cout"]
    a.w_family = lib.vx_conv3d_k3_family(case["cin"], case["cout"])
    a.range_flag = ptr("range_flag")
    e = case["epilogue"]
    if e == "stats":
        a.stats_partial = ptr("stats")
    else:
        a.act = _lib.VX_ACT_LRELU
        if e == "lrelu_hash":
            a.drop_mode, a.drop_seed, a.drop_layer = _lib.VX_DROP_HASH, 77, 3
        elif e == "lrelu_mask":
            a.drop_mode, a.drop_mask = _lib.VX_DROP_MASK, ptr("mask")
    return a


def dummy_ptr(name):
    return 0x10000 * (1 + sorted(("in", "w_packed", "bias", "out", "range_flag", "stats", "mask")).index(name))


def dry_run(lib, a):
    """(return code, kernel name) of vx_conv3d_k3_route"""
    buf = C.create_string_buffer(128)
    rc = lib.vx_conv3d_k3_route(C.byref(a), buf, len(buf))
    return rc, buf.value.decode()


class LayerBuffers:
    """device buffers of a single-layer case (inputs a pure function of the case); launch() leaves the outputs in .out / .stats /
    .range_flag"""

    def __init__(self, lib, case):
        import torch
        from values_amd import _lib
        D, H, W = case["shape"]
        ci, co, N = case["cin"], case["cout"], LAYER_N
        g = torch.Generator(device="cpu").manual_seed(1 + ci * 7 + co * 3 + D + 2 * H + 5 * W)
        dev = torch.device("cuda", 0)
        self.x = torch.randn((N, D, H, W, ci), generator=g).to(dev)
        self.w = (torch.randn((co, ci, 3, 3, 3), generator=g) * (1.0 / (27 * ci) ** 0.5)).to(dev)
        self.b = (torch.randn(co, generator=g) * 0.1).to(dev)
        self.mask = (torch.rand((N, D, H, W, co), generator=g) > 0.5).to(torch.uint8).to(dev)
        self.wp = torch.zeros(lib.vx_conv3d_k3_packed_floats(ci, co), dtype=torch.float32, device=dev)
        rc = lib.vx_pack_conv3d_k3(_lib.ptr(self.w), _lib.ptr(self.wp), ci, co, _lib.stream_ptr())
        assert rc == 0, lib.vx_last_error_string()
        self.out = torch.zeros((N, D, H, W, co), device=dev)
        self.stats = torch.zeros((N, lib.vx_conv3d_k3_tiles(D, H, W), co, 2), device=dev)
        self.range_flag = torch.zeros(4, dtype=torch.int32, device=dev)
        self.lib, self.case = lib, case

    def ptr(self, name):
        t = {"in": self.x, "w_packed": self.wp, "bias": self.b, "out": self.out, "range_flag": self.range_flag, "stats": self.stats,
             "mask": self.mask}[name]
        return t.data_ptr()

    def launch(self):
        """-> the kernel name after the real launch"""
        import torch
        from values_amd import _lib
        self.out.zero_(); self.stats.zero_(); self.range_flag.zero_()
        a = layer_args(self.lib, self.case, self.ptr)
        rc = self.lib.vx_conv3d_k3(C.byref(a), _lib.stream_ptr())
        assert rc == 0, (self.case["id"], rc, self.lib.vx_last_error_string())
        torch.cuda.synchronize()
        return self.lib.vx_last_kernel_name().decode()
