"""The cases behind tests/golden/convT_routes.json (tools/gen_convT_routes.py records them, tests/test_convT_route_cpu.py and
tests/test_gpu_convT_route.py read them back, tools/ab_routesT.py compares two builds' bits on them): single vx_convT_k2s2
launches at the smallest shapes at which each rule of values_amd/csrc/convT_route.h can go wrong.

  chan     the channel rule under the default configuration, at 2x4x4x4 and at 1x3x5x7 (105 voxels: the last column tile is partial)
  fp32     the channel rule under conv_fp32 = 1
  epi      every epilogue the kernels branch on, for one case of each of the four kernels
  decode   N = D = H = 1: W = 65535 stays on the matrix kernel, W = 65536 (nvox x dmax = 2^32) moves to the row-streaming kernel
  generic  channel counts no other kernel takes; 24 output channels fail the rows kernel's lane rule, but the matrix kernel takes
           16 -> 24 first at a small size, so it is recorded at W = 65536 as well
  stride   the grid-stride loops of the tile kernels with a second column tile per wave and a partial last tile: the split-fp16 kernel
           from ncoltiles > 4 ceil(512 / grid_y) (64 -> 32: 524 tiles for 512 waves; 128 -> 64: 130 for 128), the fp32 matrix kernel from
           524288 voxels (16 -> 8 at 2x64x64x65: 33280 tiles for 32768 waves); plain, and ReLU + hash dropout into half 1 of an
           xblk = 2 concat buffer
  bound    both sides of the decode bound nvox x dmax < 2^32 with all three magics live: 2x2x2x23170 (4 294 791 200) stays on the
           matrix kernel, 2x2x2x23171 (4 295 161 928) moves to the row-streaming kernel
  rowsnd   the row-streaming kernel with n, z, y > 0 at 2x2x2x23171: every epilogue the shape admits (2 W % 4 = 2: xblk 1 and 2),
           16 -> 16 (1 482 944 pieces for 4096 x 256 threads: its grid stride) and 32 -> 16

The generic kernel's own grid stride starts above 8192 x 256 = 2 M voxels, a 0.5 GB output at the smallest layer: left out.

The decode bound cannot be crossed below 65536 voxels, whose output is 16.8 MB at 8 channels: the rows kernel's epilogue cases
with a wide pitch or a concat buffer (25 / 34 MB) and 16 -> 24 at that size (50 MB), the bound / rowsnd cases (47 .. 95 MB) and
stride's 16 -> 8 (136 MB plain, 273 MB as a concat buffer: the one large buffer) are the only buffers above 20 MB.

tests/test_gpu_convT_matrix.py compares the output of every case with tests/convT_ref.py."""
import ctypes as C
import functools

GOLDEN = "convT_routes.json"

ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2
DROP_NONE, DROP_HASH, DROP_MASK = 0, 1, 2
SMALL, ODD, LINE = (2, 4, 4, 4), (1, 3, 5, 7), (1, 1, 1, 65536)
BELOW, ABOVE = (2, 2, 2, 23170), (2, 2, 2, 23171)
DROP_SEED, DROP_LAYER = 77, 3

# the epilogue variants: (tag, fields of the case)
_EPI = [("none", {}), ("relu", dict(act=ACT_RELU)), ("lrelu", dict(act=ACT_LRELU)),
        ("hash", dict(act=ACT_RELU, drop=DROP_HASH)), ("mask", dict(act=ACT_RELU, drop=DROP_MASK)),
        ("coff", dict(out_coff=4, out_extra=4)), ("inpitch", dict(in_extra=4))]
_EPI += [(f"xblk{xb}h{half}", dict(xblk=xb, half=half)) for xb in (1, 2, 4) for half in (0, 1)]
# one case of each kernel: (Cin, Cout, volume)
_EPI_BASES = [(16, 8, (2, 3, 5, 6)), (64, 32, (2, 3, 5, 6)), (16, 8, LINE), (8, 8, (2, 2, 2, 2))]


def _case(group, cin, cout, vol, cfg=None, tag="", **fields):
    c = dict(cfg=cfg or {}, cin=cin, cout=cout, vol=vol, act=ACT_NONE, drop=DROP_NONE, xblk=0, half=0, out_coff=0, out_extra=0, in_extra=0)
    c.update(fields)
    c["id"] = f"{group}:{cin}->{cout}:{'x'.join(str(v) for v in vol)}" + (f":{tag}" if tag else "")
    return c


def _cases():
    out = []
    for vol in (SMALL, ODD):
        out += [_case("chan", ci, co, vol) for ci, co in ((16, 8), (16, 16), (32, 8), (32, 16), (64, 32), (64, 8), (128, 64), (128, 8))]
    out += [_case("fp32", ci, co, ODD, cfg=dict(conv_fp32=1)) for ci, co in ((64, 32), (64, 8), (128, 64), (16, 8))]
    for ci, co, vol in _EPI_BASES:
        out += [_case("epi", ci, co, vol, tag=tag, **f) for tag, f in _EPI]
    for ci, co in ((16, 8), (32, 16)):
        out += [_case("decode", ci, co, (1, 1, 1, w)) for w in (65535, 65536)]
    out += [_case("generic", ci, co, (2, 2, 2, 2)) for ci, co in ((8, 8), (24, 16), (16, 24))] + [_case("generic", 16, 24, LINE)]
    for ci, co, vol in ((64, 32, (2, 5, 27, 31)), (128, 64, (3, 3, 7, 33)), (16, 8, (2, 64, 64, 65))):
        out += [_case("stride", ci, co, vol), _case("stride", ci, co, vol, tag="hashx2h1", act=ACT_RELU, drop=DROP_HASH, xblk=2, half=1)]
    out += [_case("bound", 16, 8, vol) for vol in (BELOW, ABOVE)]
    out += [_case("rowsnd", 16, 8, ABOVE, tag=tag, **f) for tag, f in _EPI if (2 * ABOVE[3]) % (f.get("xblk") or 1) == 0]
    out += [_case("rowsnd", 16, 16, ABOVE), _case("rowsnd", 32, 16, ABOVE)]
    return out


LAYER_CASES = _cases()
GROUPS = sorted({c["id"].split(":")[0] for c in LAYER_CASES})


def matrix_params():
    """[(case, conv_fp32)] of the value matrix (tests/test_convT_ref_cpu.py, tests/test_gpu_convT_matrix.py): every case under its own
    configuration, and those with 64 / 128 input channels -- the only ones whose route depends on the conv mode (convT_tile_rule) --
    under the other mode as well; a launch that two groups share is listed once"""
    out, seen = [], set()
    for c in LAYER_CASES:
        own = c["cfg"].get("conv_fp32", 0)
        for mode in ((own, 1 - own) if c["cin"] in (64, 128) else (own,)):
            key = (mode,) + tuple((k, v) for k, v in sorted(c.items()) if k not in ("id", "cfg"))
            if key not in seen:
                seen.add(key)
                out.append((c, mode))
    return out


def layer_args(case, ptr, drop_seed=DROP_SEED, seed_dev=False):
    """vx_convT_args of a case.  ptr(name) gives the address of a buffer: a real tensor for a launch, any non-null number for the
    dry run.  seed_dev: pass the device seed word ptr("seed")"""
    from values_amd import _lib
    a = _lib.ConvTArgs()
    ci, co = case["cin"], case["cout"]
    a.in_, a.in_pitch, a.w_packed, a.bias = ptr("in"), ci + case["in_extra"], ptr("w_packed"), ptr("bias")
    a.out, a.out_pitch, a.out_coff = ptr("out"), co + case["out_extra"], case["out_coff"]
    a.N, a.D, a.H, a.W = case["vol"]
    a.Cin, a.Cout, a.act, a.drop_mode, a.drop_seed, a.drop_layer = ci, co, case["act"], case["drop"], drop_seed, DROP_LAYER
    if case["drop"] == DROP_MASK:
        a.drop_mask = ptr("mask")
    a.out_xblk, a.out_half, a.range_flag = case["xblk"], case["half"], ptr("range")
    if seed_dev:
        a.seed_dev = ptr("seed")
    return a


_NAMES = ("in", "w_packed", "bias", "out", "mask", "range", "seed")


def dummy_ptr(name):
    return 0x10000 * (1 + _NAMES.index(name))


def dry_run(lib, a):
    """(return code, kernel name, grid_x, grid_y) of vx_convT_k2s2_route"""
    from values_amd import _lib
    buf, info = C.create_string_buffer(128), _lib.ConvTRouteInfo()
    rc = lib.vx_convT_k2s2_route(C.byref(a), buf, len(buf), C.byref(info))
    return rc, buf.value.decode(), info.grid_x, info.grid_y


@functools.lru_cache(maxsize=None)
def _host(shape, tag, scale=1.0):
    import torch
    from tests.formula import formula_tensor
    return torch.from_numpy(formula_tensor(shape, tag, scale)).float()


def host_inputs(case, scale=1.0):
    """(x [N][D][H][W][Cin], w (Cin, Cout, 2, 2, 2), b (Cout), mask [N][2D][2H][2W][Cout] uint8 or None): float32 CPU tensors, all in
    [-1, 1) x scale"""
    import torch
    ci, co, (n, d, h, w) = case["cin"], case["cout"], case["vol"]
    mask = (_host((n, 2 * d, 2 * h, 2 * w, co), 44) > 0).to(torch.uint8) if case["drop"] == DROP_MASK else None
    return _host((n, d, h, w, ci), 41, scale), _host((ci, co, 2, 2, 2), 42, (1.0 / ci) ** 0.5), _host((co,), 43, 0.1), mask


class LayerBuffers:
    """device buffers of a case (inputs a pure function of the case's shape); launch() leaves the output in .out.
    guard = True (tests/test_gpu_convT_matrix.py): the output is prefilled with SENTINEL, not zeros, and lies between two guard
    regions of one output row each (.whole = guard | out | guard), and the in_extra columns of the input hold NaN, not zeros.
    scale multiplies the input."""
    SENTINEL = -77.0

    def __init__(self, lib, case, guard=False, scale=1.0):
        import torch
        from values_amd import _lib
        ci, co, (n, d, h, w) = case["cin"], case["cout"], case["vol"]
        dev = torch.device("cuda", 0)
        x = torch.full((n, d, h, w, ci + case["in_extra"]), float("nan") if guard else 0.0)
        hx, hw, hb, hmask = host_inputs(case, scale)
        x[..., :ci] = hx
        self.x, self.w, self.b = x.to(dev), hw.to(dev), hb.to(dev)
        self.wp = torch.zeros(lib.vx_convT_k2s2_packed_floats(ci, co), dtype=torch.float32, device=dev)
        rc = lib.vx_pack_convT_k2s2(_lib.ptr(self.w), _lib.ptr(self.wp), ci, co, _lib.stream_ptr())
        assert rc == 0, lib.vx_last_error_string()
        # plain: [N][2D][2H][2W][pitch]; concat buffer: [N][2D][2H][2W / xb][2][xb][Cout]
        shape = (n, 2 * d, 2 * h, 2 * w, 2 * co if case["xblk"] else co + case["out_extra"])
        self.guard = 2 * w * shape[-1] if guard else 0          # floats: one output row (a multiple of 4, so .out stays 16-byte aligned)
        body = n * 8 * d * h * w * shape[-1]
        self.whole = torch.zeros(body + 2 * self.guard, device=dev)
        self.out = self.whole[self.guard:self.guard + body].view(shape)
        self.mask = hmask.to(dev) if hmask is not None else None
        self.range = torch.zeros(1, dtype=torch.int32, device=dev)
        self.seed = torch.zeros(1, dtype=torch.int32, device=dev)
        self.lib, self.case = lib, case

    def ptr(self, name):
        t = {"in": self.x, "w_packed": self.wp, "bias": self.b, "out": self.out, "mask": self.mask, "range": self.range, "seed": self.seed}[name]
        return t.data_ptr()

    def launch(self, drop_seed=DROP_SEED, seed_dev=None, range_init=0):
        """-> the kernel name after the real launch.  seed_dev: the value of the device seed word, None: no such word"""
        import torch
        from values_amd import _lib
        self.whole.fill_(self.SENTINEL if self.guard else 0.0)
        self.range.fill_(range_init)
        if seed_dev is not None:
            self.seed.copy_(torch.tensor([seed_dev], dtype=torch.int64).to(torch.int32))      # the word's 32 bits
        a = layer_args(self.case, self.ptr, drop_seed, seed_dev is not None)
        rc = self.lib.vx_convT_k2s2(C.byref(a), _lib.stream_ptr())
        assert rc == 0, (self.case["id"], rc, self.lib.vx_last_error_string())
        torch.cuda.synchronize()
        return self.lib.vx_last_kernel_name().decode()
