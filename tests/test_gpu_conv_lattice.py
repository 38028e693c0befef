"""GPU: the conv kernels on inputs whose right answer is exactly representable (tests/conv_lattice.py; the conditions are proven on the
CPU by tests/test_conv_lattice_cpu.py).  A correct kernel is exact on them for any summation order, tile shape and arrangement of
accumulators; a wrong or missing 16-byte piece moves some output by thousands of tolerances.

  hi-lattice        torch.equal with the float64 expectation, every family, both conv modes; the statistics partials, added in float64
                    over tiles, equal sum E (and sum E^2 where sum E^2 < 2^20) exactly; pitch padding / the other concat half untouched
  lattice with lo   |got - E| <= 3 * 2^-24 (|M| + |X| / 2048 + |b|) per element (split-fp16 kernels)
  impulses          forms (a) and (b) on the split-fp16 kernels, form (a) on the fp32 kernels: tol 2^-23 |E|
  epilogues         ReLU, hash dropout (x 2), mask dropout where the family takes a mask, on one case per family.  The column and deep
                    kernels apply hash dropout only behind a LeakyReLU: exact where the pre-activation is >= 0, which is what is
                    compared bit for bit; LeakyReLU's negative side and the normalise-on-load prologues stay with the dense tests.
  composed launches the zc16 planar hand-over and the fused up-convolutions of xp8w and zc16 on the hi-lattice, where the intermediate tensor
                    is fp16-exact and the whole launch exact (conv_lattice.HI_ONLY_BOUND)
Every launch asserts vx_last_kernel_name(): the intended family and instance ran.  The launch helpers are those of
tests/test_gpu_kernels.py and tests/test_gpu_kernels2d.py."""
import ctypes as C

import pytest
import torch

from tests import conv_lattice as L
from tests import test_gpu_kernels as K
from tests import test_gpu_kernels2d as K2
from values_amd import _lib

pytestmark = pytest.mark.gpu

conv_mode = K.conv_mode      # the fixture of tests/test_gpu_kernels.py: the split-fp16 schedule and conv_fp32 = 1
_ALL3D = L.CONV3D_CASES + L.CONV3D_FP32_CASES
_BY_ID = {c[0]: c for c in _ALL3D}


def _kn():
    return _lib.load().vx_last_kernel_name().decode()


def _pack3d(wt, cin, cout):
    lib = _lib.load()
    wd = wt.float().contiguous().to(K.dev())
    wp = torch.empty(lib.vx_conv3d_k3_packed_floats(cin, cout), dtype=torch.float32, device=K.dev())
    _lib.check(lib.vx_pack_conv3d_k3(_lib.ptr(wd), _lib.ptr(wp), cin, cout, _lib.stream_ptr()), "pack")
    return wp


def _launch3d(row, c, *, act=0, drop=0, mask=None, seed=0, layer=0, stats=False, padded=False):
    """one vx_conv3d_k3 launch of a matrix row through its family's helper -> (out NCDHW cpu float32, statistics (N, tiles, Cout, 2)
    cpu or None, kernel name).  padded: into a wider output (pitch padding / the other half of an x-blocked buffer must stay -77)."""
    _, fam, _, cin, cout, (n, d, h, w), kw, _, _ = row
    xb = kw.get("xblk", 0)
    x = c.x.float()
    if fam in ("s16", "fp32"):
        pk = dict(out_pitch=cout + 16, out_coff=8) if padded else {}
        got, st, (lo, hi) = K.run_conv(c.x, c.w, c.b, act=act, drop_mode=drop, mask=mask, seed=seed, layer=layer, stats=stats, **kw, **pk)
        kn = _kn()
        assert (lo == -77.0).all() and (hi == -77.0).all()
        return got, st, kn
    assert mask is None
    xd = (K.to_xblk(x[:, :cin // 2], x[:, cin // 2:], xb) if xb else K.cl(x)).to(K.dev())
    if fam == "xp8w":
        got, st, _, flag = K._xp8_conv(xd, cin, c.w, c.b, n, d, h, w, act=act, drop=drop, seed=seed, layer=layer, stats=stats, xblk=xb,
                                       out_xblk=4 if padded else 0)         # (the helper asserts the other half untouched)
        assert flag == 0.0
        return got, st, _kn()
    wp, bd = _pack3d(c.w, cin, cout), c.b.float().contiguous().to(K.dev())
    if fam == "zc16":
        out, st, _, kn = K._zc16_launch(xd, cin, wp, bd, n, d, h, w, act=act, drop=drop, seed=seed, layer=layer, stats=stats,
                                        out_xblk=4 if padded else 0)
        if padded:
            blk = out.view(n, d, h, w // 4, 2, 4, 16)
            assert (blk[:, :, :, :, 0] == -77.0).all()
            out = blk[:, :, :, :, 1].reshape(n, d, h, w, 16)
    else:
        pk = dict(out_pitch=cout + 8, out_coff=4) if padded else {}
        out, st, kn = K._deep_launch(xd, cin, cout, wp, bd, n, d, h, w, act=act, drop=drop, seed=seed, layer=layer, stats=stats,
                                     in_xblk=xb, **pk)
        if padded:
            assert (out[..., :4] == -77.0).all() and (out[..., 4 + cout:] == -77.0).all()
            out = out[..., 4:4 + cout]
    return K.ncdhw(out).cpu(), (st.cpu() if st is not None else None), kn


def _check_stats(st, E, red_tiles, red_E):
    """the partials, added in float64, are the exact sums wherever every fp32 partial is exact (conv_lattice.stats_exact)"""
    s = st.double().sum(red_tiles)
    sum_ok = bool((E.abs().sum(red_E) < 2.0 ** 22).all())
    sq_ok = bool(((E * E).sum(red_E) < 2.0 ** 20).all())
    assert sum_ok
    want = E.sum(red_E)
    assert torch.equal(s[..., 0], want), ("sum column", (s[..., 0] - want).abs().max().item(), (s[..., 0] != want).nonzero()[:6].tolist())
    if sq_ok:
        want2 = (E * E).sum(red_E)
        assert torch.equal(s[..., 1], want2), ("sum-of-squares column", (s[..., 1] - want2).abs().max().item(),
                                               (s[..., 1] != want2).nonzero()[:6].tolist())


def _case3d(row, flavour):
    return L.make_case("conv3d", row[3], row[4], tuple(row[5]), flavour, 3, 1)


_LATTICE_PARAMS = [(r[0], f) for r in L.CONV3D_CASES for f in ("hi", "lo")] + [(r[0], "hi") for r in L.CONV3D_FP32_CASES]


@pytest.mark.parametrize("cid,flavour", _LATTICE_PARAMS, ids=["%s-%s" % p for p in _LATTICE_PARAMS])
def test_conv3d_lattice(cid, flavour, vxcfg):
    row = _BY_ID[cid]
    vxcfg.set(**dict(dict(conv_fp32=0), **row[2]))
    c = _case3d(row, flavour)
    got, _, kn = _launch3d(row, c, padded=(flavour == "hi"))
    assert kn.startswith(row[7]), (kn, row[7])
    L.check(got, c.E, c.tol, c)
    if flavour == "hi":
        assert torch.equal(got.double(), c.E)
        got, st, kn = _launch3d(row, c, stats=True)
        assert kn.startswith(row[8] or L._S16), (kn, row[8])
        L.check_equal(got, c.E, c)
        _check_stats(st, c.E, 1, (2, 3, 4))


def _check_lrelu_hash(got, E, keep, case=None):
    """LeakyReLU + hash dropout on the hi-lattice: bit-equal to 2 * keep * E where the pre-activation is >= 0, zero where dropped, and
    within two float32 roundings of 0.02 * E on the negative side (whose exact bits stay with the dense tests)"""
    got = got.double()
    pos = E >= 0
    zero = torch.zeros_like(E)
    L.check_equal(torch.where(pos, got, zero), torch.where(pos, E * keep * 2.0, zero), case)
    assert bool((got[keep == 0] == 0).all())
    neg = 0.02 * E * keep
    assert bool(((got - neg).abs()[~pos] <= 2.0 ** -22 * neg.abs()[~pos]).all())


@pytest.mark.parametrize("cid", L.EPILOGUE_IDS)
def test_conv3d_exact_epilogues(cid, vxcfg):
    row = _BY_ID[cid]
    fam, cout, (n, d, h, w) = row[1], row[4], row[5]
    vxcfg.set(**dict(dict(conv_fp32=0), **row[2]))
    c = _case3d(row, "hi")
    relu = torch.relu(c.E)
    got, _, kn = _launch3d(row, c, act=_lib.VX_ACT_RELU)
    assert kn.startswith(row[7]), kn
    L.check_equal(got, relu, c)
    keep = K._hash_mask(31, 7, n, cout, d, h, w)
    assert 0.4 < keep.mean().item() < 0.6
    # LeakyReLU + hash dropout (the instance the decoder layers run): exact where the pre-activation is >= 0
    got, _, kn = _launch3d(row, c, act=_lib.VX_ACT_LRELU, drop=_lib.VX_DROP_HASH, seed=31, layer=7)
    assert kn.startswith(row[7]), kn
    _check_lrelu_hash(got, c.E, keep, c)
    if fam in ("s16", "fp32"):          # the tile kernels also take ReLU + hash dropout and an injected mask
        got, _, kn = _launch3d(row, c, act=_lib.VX_ACT_RELU, drop=_lib.VX_DROP_HASH, seed=31, layer=7)
        assert kn.startswith(row[7]), kn
        L.check_equal(got, relu * keep * 2.0, c)
        mask = torch.from_numpy(K.formula_tensor((n, cout, d, h, w), 914)) > 0
        got, _, kn = _launch3d(row, c, act=_lib.VX_ACT_RELU, drop=_lib.VX_DROP_MASK, mask=mask)
        assert kn.startswith(row[7]), kn
        L.check_equal(got, relu * mask * 2.0, c)


_IMPULSE_PARAMS = [(i, f) for i in L.IMPULSE_IDS for f in (("imp_a",) if _BY_ID[i][1] == "fp32" else ("imp_a", "imp_b"))]


@pytest.mark.parametrize("cid,form", _IMPULSE_PARAMS, ids=["%s-%s" % p for p in _IMPULSE_PARAMS])
def test_conv3d_impulses(cid, form, vxcfg):
    row = _BY_ID[cid]
    vxcfg.set(**dict(dict(conv_fp32=0), **row[2]))
    c = _case3d(row, form)
    got, _, kn = _launch3d(row, c)
    assert kn.startswith(row[7]), kn
    L.check(got, c.E, c.tol, c)


# ---- composed launches on the hi-lattice (conv_lattice.HI_ONLY_BOUND) -----------------------------------------------------------------
@pytest.mark.parametrize("shape", L.PLANAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3d_zc16_planar_handover_lattice(shape, vxcfg):
    """producer with out_planar (fp16 hi / lo planes in the consumer's LDS row order), consumer with in_planar staging them by LDS-DMA:
    on the hi-lattice the planes hold ReLU(E1) and zeros exactly, and the consumer's output is the exact second convolution"""
    n, d, h, w = shape
    p = L.planar_case(tuple(shape))
    c = p.first
    xd = K.cl(c.x.float()).to(K.dev())
    wp1, bd1 = _pack3d(c.w, 16, 16), c.b.float().contiguous().to(K.dev())
    wp2, bd2 = _pack3d(p.w2, 16, 16), p.b2.float().contiguous().to(K.dev())
    y, _, _, k1 = K._zc16_launch(xd, 16, wp1, bd1, n, d, h, w, act=_lib.VX_ACT_RELU, out_planar=True)
    assert k1 == "conv3d_zc16_kernel<16,6,0,0,0>", k1
    pl = y.contiguous().view(torch.float16).view(n, d, h, 2, 2, w, 8).float()        # [n][d][h][octet][hi | lo][w][8 halves]
    hi = pl[:, :, :, :, 0].permute(0, 1, 2, 4, 3, 5).reshape(n, d, h, w, 16)
    L.check_equal(K.ncdhw(hi).cpu(), p.y, c)
    assert bool((pl[:, :, :, :, 1] == 0).all())
    z, _, _, k2 = K._zc16_launch(y, 16, wp2, bd2, n, d, h, w, act=_lib.VX_ACT_RELU, in_planar=True)
    assert k2 == "conv3d_zc16_kernel<16,3,4,0,0>", k2
    L.check_equal(K.ncdhw(z).cpu(), torch.relu(p.E2))
    # the LeakyReLU + hash dropout instances: the producer's planes (hi + lo / 2048), and the consumer on the exact planar tensor above
    y5, _, _, k3 = K._zc16_launch(xd, 16, wp1, bd1, n, d, h, w, act=_lib.VX_ACT_LRELU, drop=_lib.VX_DROP_HASH, seed=21, layer=11, out_planar=True)
    assert k3 == "conv3d_zc16_kernel<16,5,0,0,0>", k3
    pl = y5.contiguous().view(torch.float16).view(n, d, h, 2, 2, w, 8).double()
    back = (pl[:, :, :, :, 0] + pl[:, :, :, :, 1] / 2048.0).permute(0, 1, 2, 4, 3, 5).reshape(n, d, h, w, 16)
    _check_lrelu_hash(K.ncdhw(back).cpu(), c.E, K._hash_mask(21, 11, n, 16, d, h, w), c)
    z, _, _, k4 = K._zc16_launch(y, 16, wp2, bd2, n, d, h, w, act=_lib.VX_ACT_LRELU, drop=_lib.VX_DROP_HASH, seed=21, layer=12, in_planar=True)
    assert k4 == "conv3d_zc16_kernel<16,1,4,0,0>", k4
    _check_lrelu_hash(K.ncdhw(z).cpu(), p.E2, K._hash_mask(21, 12, n, 16, d, h, w))


@pytest.mark.parametrize("shape,xblk", L.UPFUSE_XP8W, ids=["%s-xb%d" % ("x".join(map(str, s)), x) for s, x in L.UPFUSE_XP8W])
def test_conv3d_xp8w_fused_upconvolution_lattice(shape, xblk, vxcfg):
    """upscale -> cat([up, skip]) -> conv in one launch: the up half (fp16-exact on the hi-lattice) evaluated per step, and composed into
    the conv's weights (vx_pack_conv3d_upfused)"""
    lib = _lib.load()
    n, d, h, w = shape
    assert lib.vx_conv3d_k3_upfuse_ok(d, h, w, 16, 8) == 1
    u = L.upfused_case(tuple(shape), 16, 8, 8, 8)
    cd = K.cl(u.coarse.float()).to(K.dev())
    garbage = torch.full((n, 8, d, h, w), 1e30)
    xd = (K.to_xblk(garbage, u.skip.float(), xblk) if xblk else K.cl(u.skip.float())).to(K.dev())
    for compose, up_form in ((False, 1), (True, 2)):
        got, _, _, flag = K._xp8_conv(xd, 16, u.w, u.b, n, d, h, w, act=_lib.VX_ACT_RELU, xblk=xblk, in_pitch=None if xblk else 8,
                                      up=(cd, u.uw, u.ub), compose=compose)
        kn = _kn()
        assert kn.startswith("conv3d_xp8w_kernel<2,3,0,%d," % up_form), kn
        assert flag == 0.0
        L.check_equal(got, torch.relu(u.E))
        got, _, _, _ = K._xp8_conv(xd, 16, u.w, u.b, n, d, h, w, act=_lib.VX_ACT_LRELU, drop=_lib.VX_DROP_HASH, seed=93, layer=15, xblk=xblk,
                                   in_pitch=None if xblk else 8, up=(cd, u.uw, u.ub), compose=compose)
        kn = _kn()
        assert kn.startswith("conv3d_xp8w_kernel<2,1,0,%d," % up_form), kn
        _check_lrelu_hash(got, u.E, K._hash_mask(93, 15, n, 8, d, h, w))


@pytest.mark.parametrize("shape", L.UPFUSE_ZC16, ids=lambda s: "x".join(map(str, s)))
def test_conv3d_zc16_fused_upconvolution_lattice(shape, vxcfg):
    """the call sequence of test_conv3d_zc16_fused_upconvolution_matches_oracle: plain and pre-split coarse tensor, with and without
    partial sums, ReLU and LeakyReLU + hash dropout"""
    lib = _lib.load()
    n, d, h, w = shape
    assert lib.vx_conv3d_k3_upfuse_ok(d, h, w, 16, 16) == 2
    u = L.upfused_case(tuple(shape), 32, 16, 0, 16)
    uwd = u.uw.float().contiguous().to(K.dev())
    uwp = torch.empty(lib.vx_convT_zc16_packed_floats(), dtype=torch.float32, device=K.dev())
    _lib.check(lib.vx_pack_convT_zc16(_lib.ptr(uwd), _lib.ptr(uwp), _lib.stream_ptr()), "vx_pack_convT_zc16")
    ubd, cd = u.ub.float().contiguous().to(K.dev()), K.cl(u.coarse.float()).to(K.dev())
    wp, bd = _pack3d(u.w, 16, 16), u.b.float().contiguous().to(K.dev())
    part = torch.from_numpy(L.lattice((n, 16, d, h, w), 977, False)[0])          # partial sums of an earlier launch (acc_in)
    keep = K._hash_mask(9, 14, n, 16, d, h, w)
    cds = cd.reshape(-1, 4)                                                        # the coarse tensor as fp16 (hi, lo) pairs: lo = 0 here
    cds = torch.cat([cds.half(), torch.zeros_like(cds).half()], 1).view(torch.float32).reshape(cd.shape).contiguous()
    for split, acc, hashed in ((0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0), (1, 1, 1)):
        src = cds if split else cd
        out = K.cl(part.float()).to(K.dev()).contiguous() if acc else torch.full((n, d, h, w, 16), -77.0, dtype=torch.float32, device=K.dev())
        a = _lib.ConvArgs()
        a.w_family = lib.vx_conv3d_k3_family(16, 16)
        a.in_ = src.data_ptr(); a.w_packed = wp.data_ptr(); a.bias = bd.data_ptr(); a.out = out.data_ptr()
        a.in_pitch, a.out_pitch, a.out_coff = 16, 16, 0
        a.N, a.D, a.H, a.W, a.Cin, a.Cout = n, d, h, w, 16, 16
        a.act = _lib.VX_ACT_LRELU if hashed else _lib.VX_ACT_RELU
        if hashed:
            a.drop_mode, a.drop_seed, a.drop_layer = _lib.VX_DROP_HASH, 9, 14
        a.up_in, a.up_w, a.up_b, a.up_pitch, a.up_split = src.data_ptr(), uwp.data_ptr(), ubd.data_ptr(), 32, split
        if acc:
            a.acc_in, a.acc_pitch = out.data_ptr(), 16
        _lib.check(lib.vx_conv3d_k3(C.byref(a), _lib.stream_ptr()), "vx_conv3d_k3 (fused up-convolution)")
        torch.cuda.synchronize()
        assert _kn() == "conv3d_zc16_kernel<16,%d,0,%d,1>" % (1 if hashed else 3, acc), _kn()
        pre = (u.E - u.b.view(1, 16, 1, 1, 1) + part) if acc else u.E                # with partial sums the bias came with the first launch
        got = K.ncdhw(out).cpu()
        if hashed:
            _check_lrelu_hash(got, pre, keep)
        else:
            L.check_equal(got, torch.relu(pre))


# ---- vx_conv3d_k3_c1 ---------------------------------------------------------------------------------------------------------------
def _run_c1(c, cout, shape, flipcode):
    """the call sequence of test_conv3d_c1_matches_oracle: every input volume read by two output samples, the odd one flipped"""
    lib = _lib.load()
    v, d, h, w = shape
    repeat = 2
    N = v * repeat
    xd, wd, bd = c.x.float().to(K.dev()), c.w.float().to(K.dev()), c.b.float().to(K.dev())
    out = torch.empty((N, d, h, w, cout), dtype=torch.float32, device=K.dev())
    nt = lib.vx_conv3d_k3_c1_tiles(d, h, w)
    st = torch.zeros((N, nt, cout, 2), dtype=torch.float32, device=K.dev())
    flips = torch.tensor([flipcode if n % 2 else 0 for n in range(N)], dtype=torch.int32, device=K.dev())
    _lib.check(lib.vx_conv3d_k3_c1(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(out), cout, N, d, h, w, cout, repeat,
                                   None, _lib.ptr(flips), _lib.ptr(st), _lib.stream_ptr()), "c1")
    torch.cuda.synchronize()
    assert _kn() == "conv3d_k3_c1_kernel<%d>" % cout, _kn()
    return K.ncdhw(out).cpu(), st.cpu()


def _c1_expect(c, n, flipcode, factor):
    dims = [2 + k for k in range(3) if (flipcode if n % 2 else 0) >> k & 1]
    sl = slice(n // 2, n // 2 + 1)
    hx, lx = torch.from_numpy(c.hi_x[sl]), torch.from_numpy(c.lo_x[sl])
    if dims:
        hx, lx = torch.flip(hx, dims), torch.flip(lx, dims)
    return L.expectation("conv3d", hx.numpy(), lx.numpy(), c.hi_w, c.lo_w, c.b.numpy(), 3, 1, factor)


@pytest.mark.parametrize("cout,shape,flipcode", L.C1_CASES)
def test_conv3d_c1_lattice(cout, shape, flipcode):
    c = L.make_case("conv3d", 1, cout, tuple(shape), "hi", 3, 1)
    got, st = _run_c1(c, cout, shape, flipcode)
    for n in range(got.shape[0]):
        _, _, E, _ = _c1_expect(c, n, flipcode, 0.0)
        L.check_equal(got[n:n + 1], E)
        _check_stats(st[n:n + 1], E, 1, (2, 3, 4))


def test_conv3d_c1_impulses():
    cout, shape, flipcode = L.C1_CASES[0]
    c = L.make_case("conv3d", 1, cout, tuple(shape), "imp_a", 3, 1)
    got, _ = _run_c1(c, cout, shape, flipcode)
    for n in range(got.shape[0]):
        _, _, E, _ = _c1_expect(c, n, flipcode, 0.0)
        L.check(got[n:n + 1], E, 2.0 ** -23 * E.abs())


# ---- vx_convT_k2s2 -----------------------------------------------------------------------------------------------------------------
def _run_convT(c, cin, cout, shape, *, act=0, mask=None, xblk=0):
    """the call sequence of test_convT_matches_oracle -> (out NCDHW cpu, kernel name)"""
    lib = _lib.load()
    n, d, h, w = shape
    xd, wd, bd = K.cl(c.x.float()).to(K.dev()), c.w.float().contiguous().to(K.dev()), c.b.float().to(K.dev())
    wp = torch.empty(lib.vx_convT_k2s2_packed_floats(cin, cout), dtype=torch.float32, device=K.dev())
    _lib.check(lib.vx_pack_convT_k2s2(_lib.ptr(wd), _lib.ptr(wp), cin, cout, _lib.stream_ptr()), "packT")
    a = _lib.ConvTArgs()
    a.in_ = xd.data_ptr(); a.in_pitch = cin; a.w_packed = wp.data_ptr(); a.bias = bd.data_ptr()
    a.N, a.D, a.H, a.W, a.Cin, a.Cout = n, d, h, w, cin, cout
    a.act = act
    flag = torch.zeros((1,), dtype=torch.int32, device=K.dev())
    a.range_flag = flag.data_ptr()
    if mask is not None:
        md = K.cl(mask).to(torch.uint8).to(K.dev())
        a.drop_mode, a.drop_mask = _lib.VX_DROP_MASK, md.data_ptr()
    if xblk:
        out = torch.full((n, 2 * d, 2 * h, (2 * w) // xblk, 2, xblk, cout), -77.0, dtype=torch.float32, device=K.dev())
        a.out = out.data_ptr(); a.out_xblk = xblk; a.out_half = 0
    else:
        pitch = 2 * cout
        out = torch.full((n, 2 * d, 2 * h, 2 * w, pitch), -77.0, dtype=torch.float32, device=K.dev())
        a.out = out.data_ptr(); a.out_pitch = pitch; a.out_coff = 0
    _lib.check(lib.vx_convT_k2s2(C.byref(a), _lib.stream_ptr()), "convT")
    torch.cuda.synchronize()
    kn = _kn()
    assert flag.item() == 0
    if xblk:
        assert (out[:, :, :, :, 1] == -77.0).all()
        return K.from_xblk(out, 0, n, cout, 2 * d, 2 * h, 2 * w, xblk).cpu(), kn
    assert (out[..., cout:] == -77.0).all()
    return K.ncdhw(out[..., :cout]).cpu(), kn


@pytest.mark.parametrize("cin,cout,shape,names", L.CONVT_CASES, ids=["%d-%d" % (r[0], r[1]) for r in L.CONVT_CASES])
def test_convT_lattice(cin, cout, shape, names, conv_mode):
    name = names[conv_mode]
    split = name.startswith("convT_k2s2_s16_kernel")
    n, d, h, w = shape
    for flavour in (("hi", "lo") if split else ("hi",)):
        c = L.make_case("convT", cin, cout, tuple(shape), flavour, 2, 2)
        for xblk in (0, 4):
            got, kn = _run_convT(c, cin, cout, shape, xblk=xblk)
            assert kn.startswith(name) and kn.endswith(",false>"), kn
            L.check(got, c.E, c.tol, c)
            if flavour == "hi":
                assert torch.equal(got.double(), c.E)
    # ReLU + mask dropout stay exact
    c = L.make_case("convT", cin, cout, tuple(shape), "hi", 2, 2)
    mask = torch.from_numpy(K.formula_tensor((n, cout, 2 * d, 2 * h, 2 * w), 915)) > 0
    got, kn = _run_convT(c, cin, cout, shape, act=_lib.VX_ACT_RELU, mask=mask)
    assert kn.startswith(name) and kn.endswith(",true>"), kn
    L.check_equal(got, torch.relu(c.E) * mask * 2.0, c)


_MODE_FORMS = [("split16", "imp_a"), ("split16", "imp_b"), ("fp32", "imp_a")]    # fp32 kernels: products of lo-carrying weights are not exact


@pytest.mark.parametrize("mode,form", _MODE_FORMS)
def test_convT_impulses(mode, form, vxcfg):
    vxcfg.set(conv_fp32=int(mode == "fp32"))
    cin, cout, shape = L.CONVT_IMPULSE[mode]
    c = L.make_case("convT", cin, cout, tuple(shape), form, 2, 2)
    got, kn = _run_convT(c, cin, cout, shape)
    assert kn.startswith("convT_k2s2_s16_kernel<64," if mode == "split16" else "convT_k2s2_mfma_kernel<32,"), kn
    L.check(got, c.E, c.tol, c)


# ---- vx_conv2d ---------------------------------------------------------------------------------------------------------------------
def _conv2d_name(mode, ks, s):
    return ("conv2d_s16_kernel<%d,%d," if mode == "split16" else "conv2d_mfma_kernel<%d,%d,") % (ks, s)


@pytest.mark.parametrize("cin,cout,ks,s,shape,narrow", L.CONV2D_CASES, ids=["%d-%d-k%ds%d" % r[:4] for r in L.CONV2D_CASES])
def test_conv2d_lattice(cin, cout, ks, s, shape, narrow, conv_mode):
    lib = _lib.load()
    assert (lib.vx_conv2d_family(cin, cout, ks) == 3) == (conv_mode == "fp32")
    c4 = (cout + 3) // 4 * 4
    for flavour in (("hi", "lo") if conv_mode == "split16" else ("hi",)):
        c = L.make_case("conv2d", cin, cout, tuple(shape), flavour, ks, s)
        got, st, raw = K2.run_conv2d(c.x, c.w, c.b, ks, s, narrow=narrow, out_pitch=c4 + 16, out_coff=8)
        kn = _kn()
        assert kn.startswith(_conv2d_name(conv_mode, ks, s)), kn
        assert got.shape == c.E.shape
        L.check(got, c.E, c.tol, c)
        assert (raw[..., :8] == -77.0).all() and (raw[..., 8 + c4:] == -77.0).all()
        if flavour == "hi":
            assert torch.equal(got.double(), c.E)
            _check_stats(st, c.E, 0, (0, 2, 3))


@pytest.mark.parametrize("mode,form", _MODE_FORMS)
def test_conv2d_impulses(mode, form, vxcfg):
    vxcfg.set(conv_fp32=int(mode == "fp32"))
    cin, cout, ks, s, shape, narrow = L.CONV2D_IMPULSE
    c = L.make_case("conv2d", cin, cout, tuple(shape), form, ks, s)
    got, _, _ = K2.run_conv2d(c.x, c.w, None, ks, s, stats=False, narrow=narrow)
    assert _kn().startswith(_conv2d_name(mode, ks, s)), _kn()
    L.check(got, c.E, c.tol, c)
