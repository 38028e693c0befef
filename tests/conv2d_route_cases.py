"""The cases behind tests/golden/conv2d_routes.json (tools/gen_conv2d_routes.py records them, tests/test_conv2d_route_cpu.py and
tests/test_gpu_conv2d_route.py read them back, tools/ab_routes2d.py compares two builds' bits on them).

(a) forward cases: the ordered kernel-name list of one HighResolutionNet forward (the `small` layout, formula weights, 2 x 3 x 64 x 96),
    taken from the hook profile_forward reads (HighResolutionNet._prof), in training mode and in eval mode (eval reaches the
    output-epilogue instances), under each configuration switch that moves a 2D launch.
(b) single-layer cases: the smallest shapes at which the tile and chunk geometry can go wrong (the shapes of test_gpu_ops2d.py's
    PROLOGUE_CASES), crossed with row tiles 1 / 2 / 3 / 5, octets 1 / 3, wide sub-blocks 2 / 3, several chunks, the output epilogue
    and the configuration switches."""
import ctypes as C
import functools
import os

GOLDEN = "conv2d_routes.json"

# ---- (a) ---------------------------------------------------------------------------------------------------------------------
CONFIGS = [("default", {}), ("no_wide", dict(c2s_no_wide=1)), ("no_oct", dict(c2s_no_oct=1)), ("fp32", dict(conv_fp32=1))]
FORWARD_SHAPE = (2, 3, 64, 96)
FORWARD_CASES = [(f"{mode}:{n}", mode, cfg) for mode in ("train", "eval") for n, cfg in CONFIGS]


def forward_model(mode):
    """values_amd.HighResolutionNet, the small layout with formula weights (tests/test_gpu_hrnet.py make); eval: running statistics
    at their initial values"""
    import torch
    from tests.formula import HRNET_SMALL_EXTRA, formula_state_dict_from_shapes
    from values_amd.hrnet import HighResolutionNet
    extra = dict(HRNET_SMALL_EXTRA, DROPOUT_FINAL=False)
    m = HighResolutionNet({"MODEL": {"EXTRA": extra, "ALIGN_CORNERS": False, "INPUT_CHANNELS": 3, "PRETRAINED": False},
                           "DATASET": {"NUM_CLASSES": 4}})
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in formula_state_dict_from_shapes(shapes).items()}, strict=False)
    m = m.cuda()
    return m.eval() if mode == "eval" else m


def forward_input():
    import torch
    from tests.formula import formula_tensor
    return torch.from_numpy(formula_tensor(FORWARD_SHAPE, 21)).float().cuda()


def forward_run(model, x):
    """-> (kernel names of the forward's vx_conv2d launches in launch order, logits)"""
    import torch
    old = os.environ.get("VX_HRNET_SINGLE_STREAM")
    os.environ["VX_HRNET_SINGLE_STREAM"] = "1"           # (as profile_forward: the branches in one order on one stream)
    try:
        model._prof = []
        y = model.forward_samples(x, 1)
        torch.cuda.synchronize()
        rows, model._prof = model._prof, None
    finally:
        model._prof = None
        if old is None:
            os.environ.pop("VX_HRNET_SINGLE_STREAM", None)
        else:
            os.environ["VX_HRNET_SINGLE_STREAM"] = old
    return [r[0] for r in rows], y


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
LAYER_N = 2
CINS = (3, 8, 18, 32, 48, 64, 80)          # REAL input channels: octets 1 and 3, wide 2 and 3 sub-blocks, 4 and 5 chunks
COUTS = (16, 32, 48, 72)                   # row tiles 1, 2, 3 -- and 5 on 1x1
# (KS, S, H, W, real Cin values): a tile smaller than the tile; one past a tile edge; odd sizes on parity planes; 1x1 with four and
# twelve chunks (weights resident / re-staged)
_GEOMS = [(3, 1, 5, 7, CINS), (3, 1, 17, 21, CINS), (3, 1, 20, 33, CINS), (3, 2, 17, 31, CINS), (3, 2, 33, 19, CINS),
          (1, 1, 5, 7, CINS), (1, 1, 20, 33, CINS), (1, 1, 9, 21, (256, 720))]


def _cases():
    out = []
    for cname, cfg in CONFIGS:
        for ks, s, h, w, cins in _GEOMS:
            for ci in cins:
                for co in COUTS:
                    for epi in (0, 1):
                        if cfg.get("conv_fp32") and (epi or co == 72):      # (the fp32 kernels carry no epilogue)
                            continue
                        out.append(dict(id=f"{cname}:k{ks}s{s}:{h}x{w}:{ci}->{co}:{'epi' if epi else 'stats'}", cfg=cfg, ks=ks, s=s, h=h,
                                        w=w, cin=ci, cout=co, epi=epi))
    return out


LAYER_CASES = _cases()


def r4(c):
    return (c + 3) // 4 * 4


def r16(c):
    return (c + 15) // 16 * 16


def out_hw(case):
    ks, s = case["ks"], case["s"]
    return (case["h"] + 2 * (ks // 2) - ks) // s + 1, (case["w"] + 2 * (ks // 2) - ks) // s + 1


def layer_args(lib, case, ptr):
    """vx_conv2d_args of a single-layer case as HighResolutionNet launches it: the input at pitch round4(Cin), N = LAYER_N, a bias;
    statistics partials, or (epi) the output epilogue with residual and ReLU.  ptr(name) gives the address of a buffer (a real
    tensor for a launch, any 16-byte aligned non-null number for the dry run); the weights' family is asked of `lib` under the
    configuration that is set NOW."""
    from values_amd import _lib
    a = _lib.Conv2dArgs()
    ci, co = case["cin"], case["cout"]
    a.w_family = lib.vx_conv2d_family(ci, co, case["ks"])
    a.in_, a.in_pitch, a.w_packed, a.bias = ptr("in"), r4(ci), ptr("w_packed"), ptr("bias")
    a.out, a.out_pitch, a.out_coff = ptr("out"), r4(co), 0
    a.N, a.H, a.W, a.Cin, a.Cout, a.KS, a.S = LAYER_N, case["h"], case["w"], r16(ci), co, case["ks"], case["s"]
    if case["epi"]:
        a.out_scale, a.out_shift, a.out_add, a.out_add_pitch, a.out_act = ptr("scale"), ptr("shift"), ptr("add"), r4(co), _lib.VX_ACT_RELU
    else:
        a.stats_partial = ptr("stats")
    return a


_NAMES = ("in", "w_packed", "bias", "out", "stats", "scale", "shift", "add")


def dummy_ptr(name):
    return 0x10000 * (1 + _NAMES.index(name))


def dry_run(lib, a):
    """(return code, kernel name, (nchunks, w_all, grid_x, grid_y), lds_bytes) of vx_conv2d_route"""
    from values_amd import _lib
    buf, info = C.create_string_buffer(128), _lib.Conv2dRouteInfo()
    rc = lib.vx_conv2d_route(C.byref(a), buf, len(buf), C.byref(info))
    return rc, buf.value.decode(), (info.nchunks, info.w_all, info.grid_x, info.grid_y), info.lds_bytes


@functools.lru_cache(maxsize=None)
def _host(shape, tag, scale=1.0):
    import torch
    from tests.formula import formula_tensor
    return torch.from_numpy(formula_tensor(shape, tag, scale)).float()


class LayerBuffers:
    """device buffers of a single-layer case (inputs a pure function of the case's shape); launch() leaves the outputs in .out /
    .stats"""

    def __init__(self, lib, case):
        import torch
        from values_amd import _lib
        ci, co, ks, n, h, w = case["cin"], case["cout"], case["ks"], LAYER_N, case["h"], case["w"]
        oh, ow = out_hw(case)
        dev = torch.device("cuda", 0)
        x = torch.zeros((n, h, w, r4(ci)))
        x[..., :ci] = _host((n, h, w, ci), 31)
        self.x = x.to(dev)
        self.w = _host((co, ci, ks, ks), 32, (1.0 / (ks * ks * ci)) ** 0.5).to(dev)
        self.b = torch.zeros(r16(co))
        self.b[:co] = _host((co,), 33, 0.1)
        self.b = self.b.to(dev)
        self.scale, self.shift = (_host((co,), 34) * 0.3 + 1.0).to(dev), _host((co,), 35, 0.3).to(dev)
        self.add = _host((n, oh, ow, r4(co)), 36).to(dev)
        self.wp = torch.zeros(lib.vx_conv2d_packed_floats(ci, co, ks), dtype=torch.float32, device=dev)
        rc = lib.vx_pack_conv2d(_lib.ptr(self.w), _lib.ptr(self.wp), ci, co, ks, _lib.stream_ptr())
        assert rc == 0, lib.vx_last_error_string()
        self.out = torch.zeros((n, oh, ow, r4(co)), device=dev)
        self.stats = torch.zeros((n * lib.vx_conv2d_tiles(h, w, ks, case["s"]), co, 2), device=dev)
        self.lib, self.case = lib, case

    def ptr(self, name):
        t = {"in": self.x, "w_packed": self.wp, "bias": self.b, "out": self.out, "stats": self.stats, "scale": self.scale,
             "shift": self.shift, "add": self.add}[name]
        return t.data_ptr()

    def launch(self):
        """-> the kernel name after the real launch"""
        import torch
        from values_amd import _lib
        self.out.zero_(); self.stats.zero_()
        a = layer_args(self.lib, self.case, self.ptr)
        rc = self.lib.vx_conv2d(C.byref(a), _lib.stream_ptr())
        assert rc == 0, (self.case["id"], rc, self.lib.vx_last_error_string())
        torch.cuda.synchronize()
        return self.lib.vx_last_kernel_name().decode()
