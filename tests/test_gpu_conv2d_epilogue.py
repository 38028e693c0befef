"""GPU, kernel level: vx_bn_running_affine (BatchNorm with running statistics as scale / shift rows) and the output epilogue
of vx_conv2d (vx_conv2d_args.out_scale / out_shift / out_add / out_act).

The epilogue is stated as: bit-identical to vx_conv2d without it followed by vx_affine_gather(scale, shift, add, act) -- so
the comparison has no tolerance.  Every instance family vx_conv2d_family can return is covered (sub-block 3x3 at stride 1 and
2, whole-Cin items, 1x1 with 1 .. 5 row tiles, both octet-granular families), at two spatial sizes that leave partial tiles
in x and y."""
import ctypes as C

import numpy as np
import pytest
import torch

from values_amd import _lib
from tests.formula import formula_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"


def r4(c):
    return (c + 3) // 4 * 4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


# ---------------------------------------------------------------------------------------------- vx_bn_running_affine
def test_bn_running_affine_three_layers_one_launch():
    lib = _lib.load()
    layers = [(16, 16), (18, 32), (270, 272)]       # (C, cpitch)
    eps = 1e-5
    items = (_lib.BnAffineItem * len(layers))()
    keep, host = [], []
    for k, (c, cp) in enumerate(layers):
        gamma = 1.0 + formula_tensor((c,), 700 + k, scale=0.3)
        beta = formula_tensor((c,), 710 + k, scale=0.2)
        mean = formula_tensor((c,), 720 + k, scale=2.0)
        var = 0.05 + np.abs(formula_tensor((c,), 730 + k, scale=4.0))
        t = [dev(v) for v in (gamma, beta, mean, var)]
        sc = torch.full((cp,), -77.0, dtype=torch.float32, device=DEV)
        sh = torch.full((cp,), -77.0, dtype=torch.float32, device=DEV)
        keep += t + [sc, sh]
        it = items[k]
        it.gamma, it.beta, it.running_mean, it.running_var = (v.data_ptr() for v in t)
        it.scale, it.shift, it.C, it.cpitch = sc.data_ptr(), sh.data_ptr(), c, cp
        host.append(tuple(v.cpu().numpy().astype(np.float64) for v in t) + (sc, sh))
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(DEV)
    _lib.check(lib.vx_bn_running_affine(_lib.ptr(table), len(layers), eps, _lib.stream_ptr()), "vx_bn_running_affine")
    torch.cuda.synchronize()
    for (c, cp), (g, b, mu, var, sc, sh) in zip(layers, host):
        want_sc = g / np.sqrt(var + np.float64(np.float32(eps)))
        want_sh = b - mu * want_sc
        got_sc, got_sh = sc.cpu().numpy(), sh.cpu().numpy()
        # within 1 float32 ulp of the float64 formula (the kernel rounds its float64 result once)
        for got, want in ((got_sc, want_sc), (got_sh, want_sh)):
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(got[:c].astype(np.float64) - want) <= ulp), (c, np.abs(got[:c] - want).max())
        assert np.all(got_sc[c:] == 0) and np.all(got_sh[c:] == 0)        # rows [C, cpitch): exactly 0


def test_bn_running_affine_refuses_bad_arguments():
    lib = _lib.load()
    assert lib.vx_bn_running_affine(None, 1, 1e-5, _lib.stream_ptr()) == -1
    t = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert lib.vx_bn_running_affine(_lib.ptr(t), 0, 1e-5, _lib.stream_ptr()) == -2
    assert b"n_items" in lib.vx_last_error_string()


# ---------------------------------------------------------------------------------------------- the conv epilogue
class Layer:
    """One conv layer on the device: input at pitch round4(cin), packed weights, and what every variant shares."""

    def __init__(self, cin, cout, ks, s, n, h, w, bias=False):
        lib = _lib.load()
        self.cin, self.cout, self.ks, self.s, self.n, self.h, self.w = cin, cout, ks, s, n, h, w
        self.oh = (h + 2 * (ks // 2) - ks) // s + 1
        self.ow = (w + 2 * (ks // 2) - ks) // s + 1
        self.in_pitch = r4(cin)
        x = torch.zeros((n, h, w, self.in_pitch), dtype=torch.float32, device=DEV)
        x[..., :cin] = dev(formula_tensor((n, h, w, cin), 801))
        wt = dev(formula_tensor((cout, cin, ks, ks), 802, scale=(3.0 / (ks * ks * cin)) ** 0.5))
        self.wp = torch.empty(lib.vx_conv2d_packed_floats(cin, cout, ks), dtype=torch.float32, device=DEV)
        _lib.check(lib.vx_pack_conv2d(_lib.ptr(wt), _lib.ptr(self.wp), cin, cout, ks, _lib.stream_ptr()), "vx_pack_conv2d")
        self.family = lib.vx_conv2d_family(cin, cout, ks)
        self.x = x
        self.bias = None
        if bias:
            self.bias = torch.zeros((cout + 15) // 16 * 16, dtype=torch.float32, device=DEV)
            self.bias[:cout] = dev(formula_tensor((cout,), 803, scale=0.5))
        cp = r4(cout)
        # scale in [0.5, 1.5]; shift and residual signed, so ReLU clips about half of the values; tails zero
        self.scale = torch.zeros(cp, dtype=torch.float32, device=DEV)
        self.shift = torch.zeros(cp, dtype=torch.float32, device=DEV)
        self.scale[:cout] = dev(1.0 + formula_tensor((cout,), 804, scale=0.5))
        self.shift[:cout] = dev(formula_tensor((cout,), 805, scale=0.6))
        self.add = torch.zeros((n, self.oh, self.ow, cp), dtype=torch.float32, device=DEV)
        self.add[..., :cout] = dev(formula_tensor((n, self.oh, self.ow, cout), 806, scale=1.0))

    def args(self, out, out_pitch, out_coff=0):
        a = _lib.Conv2dArgs()
        a.w_family = self.family
        a.in_ = self.x.data_ptr(); a.in_pitch = self.in_pitch; a.w_packed = self.wp.data_ptr()
        a.bias = self.bias.data_ptr() if self.bias is not None else None
        a.out = out.data_ptr(); a.out_pitch = out_pitch; a.out_coff = out_coff
        a.N, a.H, a.W, a.Cin, a.Cout, a.KS, a.S = self.n, self.h, self.w, (self.cin + 15) // 16 * 16, self.cout, self.ks, self.s
        return a

    def fused(self, add, relu, out_pitch=None, out_coff=0, sentinel=None):
        cp = r4(self.cout)
        out_pitch = out_pitch or cp
        out = torch.full((self.n, self.oh, self.ow, out_pitch), 0.0 if sentinel is None else sentinel, dtype=torch.float32, device=DEV)
        a = self.args(out, out_pitch, out_coff)
        a.out_scale, a.out_shift = self.scale.data_ptr(), self.shift.data_ptr()
        a.out_act = _lib.VX_ACT_RELU if relu else _lib.VX_ACT_NONE
        if add:
            a.out_add, a.out_add_pitch = self.add.data_ptr(), cp
        _lib.check(_lib.load().vx_conv2d(C.byref(a), _lib.stream_ptr()), "vx_conv2d (epilogue)")
        self.kernel = _lib.load().vx_last_kernel_name().decode()
        return out

    def unfused(self, add, relu, out_pitch=None, out_coff=0, sentinel=None):
        cp = r4(self.cout)
        raw = torch.zeros((self.n, self.oh, self.ow, cp), dtype=torch.float32, device=DEV)
        _lib.check(_lib.load().vx_conv2d(C.byref(self.args(raw, cp)), _lib.stream_ptr()), "vx_conv2d (raw)")
        out_pitch = out_pitch or cp
        out = torch.full((self.n, self.oh, self.ow, out_pitch), 0.0 if sentinel is None else sentinel, dtype=torch.float32, device=DEV)
        g = _lib.AffineArgs()
        g.x = raw.data_ptr(); g.x_pitch = cp
        g.scale, g.shift = self.scale.data_ptr(), self.shift.data_ptr()
        if add:
            g.add, g.add_pitch = self.add.data_ptr(), cp
        g.out = out.data_ptr(); g.out_pitch = out_pitch; g.out_coff = out_coff
        g.N, g.H, g.W, g.C, g.OH, g.OW = self.n, self.oh, self.ow, cp, self.oh, self.ow
        g.act = _lib.VX_ACT_RELU if relu else _lib.VX_ACT_NONE
        _lib.check(_lib.load().vx_affine_gather(C.byref(g), _lib.stream_ptr()), "vx_affine_gather")
        return out


LAYERS = [(16, 16, 3, 1), (32, 48, 3, 2), (64, 18, 1, 1), (18, 36, 3, 2), (3, 64, 3, 2), (48, 48, 3, 1)]
SIZES = [(21, 19), (33, 40)]


@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("cin,cout,ks,s", LAYERS, ids=lambda v: str(v))
def test_epilogue_is_raw_conv_then_affine_gather_bit_for_bit(cin, cout, ks, s, hw):
    L = Layer(cin, cout, ks, s, 2, hw[0], hw[1])
    cp = r4(cout)
    for add, relu in ((False, False), (False, True), (True, False), (True, True)):
        got, want = L.fused(add, relu), L.unfused(add, relu)
        torch.cuda.synchronize()
        assert L.kernel.startswith("conv2d_s16_kernel<") and L.kernel.endswith(",1>"), L.kernel
        assert torch.equal(got, want), (add, relu, (got - want).abs().max().item())
        if relu:      # the variant does something: ReLU clips a good part of the values, not all of them
            frac = (got[..., :cout] == 0).float().mean().item()
            assert 0.2 < frac < 0.8, frac
        if cout % 4:  # the padded output channels are exactly 0
            assert cp > cout and bool((got[..., cout:] == 0).all())
    # out_coff into a wider concat buffer whose other channels keep a sentinel
    pitch, coff = cp + 24, 8
    got, want = L.fused(True, True, pitch, coff, sentinel=-77.0), L.unfused(True, True, pitch, coff, sentinel=-77.0)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert bool((got[..., :coff] == -77.0).all()) and bool((got[..., coff + cp:] == -77.0).all())
    assert bool((got[..., coff:coff + cout] != -77.0).all())


@pytest.mark.parametrize("cin,cout", [(64, 80), (270, 270)], ids=["5tiles", "head270"])
def test_epilogue_wide_1x1_row_tile_families(cin, cout):
    """the 1x1 families of five row tiles (one register set in the epilogue) and of the W18 head conv (4 groups of 5, a
    partial last quad), residual + ReLU"""
    L = Layer(cin, cout, 1, 1, 2, 21, 19, bias=True)
    got, want = L.fused(True, True), L.unfused(True, True)
    torch.cuda.synchronize()
    assert ",5,4,16,0,1>" in L.kernel, L.kernel
    assert torch.equal(got, want)
    if cout % 4:
        assert bool((got[..., cout:] == 0).all())


@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_epilogue_with_conv_bias(hw):
    L = Layer(16, 16, 3, 1, 2, hw[0], hw[1], bias=True)
    for add, relu in ((False, False), (True, True)):
        got, want = L.fused(add, relu), L.unfused(add, relu)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (add, relu)
    L0 = Layer(16, 16, 3, 1, 2, hw[0], hw[1], bias=False)
    assert not torch.equal(L0.fused(False, False), L.fused(False, False))      # the bias is in the result


# ---------------------------------------------------------------------------------------------- refusals (argument checks)
def _refused(a, code, word):
    lib = _lib.load()
    rc = lib.vx_conv2d(C.byref(a), _lib.stream_ptr())
    msg = lib.vx_last_error_string().decode()
    assert rc == code, (rc, msg)
    assert word in msg, msg


def test_epilogue_refusals_return_before_any_launch(vxcfg):
    vxcfg.set(conv_fp32=0)
    L = Layer(16, 16, 3, 1, 1, 8, 8)
    out = torch.zeros((1, 8, 8, 16), dtype=torch.float32, device=DEV)
    part = torch.zeros((_lib.load().vx_conv2d_tiles(8, 8, 3, 1), 16, 2), dtype=torch.float32, device=DEV)
    a = L.args(out, 16)
    a.out_scale, a.out_shift = L.scale.data_ptr(), L.shift.data_ptr()
    a.stats_partial = part.data_ptr()
    _refused(a, -3, "stats_partial")
    a = L.args(out, 16)
    a.out_add, a.out_add_pitch = L.add.data_ptr(), 16
    _refused(a, -1, "out_add")
    a = L.args(out, 16)
    a.out_act = _lib.VX_ACT_RELU
    _refused(a, -3, "out_act")
    a = L.args(out, 16)
    a.out_scale = L.scale.data_ptr()
    _refused(a, -1, "out_shift")
    torch.cuda.synchronize()
    assert bool((out == 0).all())       # nothing ran


def test_epilogue_is_refused_by_the_native_fp32_family(vxcfg):
    vxcfg.setenv("VX_CONV_FP32", "1")
    L = Layer(16, 16, 3, 1, 1, 8, 8)          # packed for the native-fp32 family
    out = torch.zeros((1, 8, 8, 16), dtype=torch.float32, device=DEV)
    a = L.args(out, 16)
    a.out_scale, a.out_shift = L.scale.data_ptr(), L.shift.data_ptr()
    _refused(a, -3, "conv_fp32")
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    _lib.check(_lib.load().vx_conv2d(C.byref(L.args(out, 16)), _lib.stream_ptr()), "vx_conv2d (fp32, raw)")   # the raw conv runs
