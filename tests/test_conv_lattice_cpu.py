"""CPU: the conditions under which tests/test_gpu_conv_lattice.py may ask the conv kernels for exact results, checked on the float64
reference alone, for every case of the GPU matrix (the parametrisation lists are the ones the GPU test uses).

  sum condition   max over outputs of sum |hi_x||hi_w| + (sum |hi_x||lo_w| + sum |lo_x||hi_w|) / 2048 + |b| < 2^8: every partial sum,
                  in any order, is then a multiple of 2^-15 below 2^8 and exact in a float32 accumulator
  coverage        every (input channel, tap) pair multiplies a non-zero activation at some in-bounds output (the lattice has no zero
                  value, so hi and lo share the pattern; both are checked)
  teeth           emulated faults move some output by >= 16 tolerances: the weights' lo dropped for one (octet, tap) piece -- EVERY
                  piece of every case --, the activations' lo zeroed on the x = 0 plane, two taps swapped; on the impulse inputs a
                  lo rounded to 5 bits
  exactness       split() of every generated value returns the parts put in; the hi-lattice expectation is float32-representable
"""
import numpy as np
import pytest
import torch

from tests import conv_lattice as L

LATTICE_KEYS = L.all_lattice_keys()
IMPULSE_KEYS = L.all_impulse_keys()
TEETH = 16.0


def _id(key):
    kind, cin, cout, shape, ks, stride = key
    return "%s-%d-%d-%s-k%ds%d" % (kind, cin, cout, "x".join(map(str, shape)), ks, stride)


def test_split_restates_the_kernels_split_and_the_lattice_is_its_fixed_point():
    # hand values: 1 + 2^-11 + 2^-13 is past the tie -> hi = 1 + 2^-10, lo = (2^-13 - 2^-11) * 2048; 1 + 2^-11 ties to even
    hi, lo = L.split(np.array([1.0 + 2.0 ** -11 + 2.0 ** -13, -0.75, 3.0 + 2.0 ** -12, 1.0 + 2.0 ** -11]))
    assert hi.tolist() == [1.0 + 2.0 ** -10, -0.75, 3.0, 1.0] and lo.tolist() == [-0.75, 0.0, 0.5, 1.0]
    # the pair the plain draw would get wrong (module docstring of tests/conv_lattice.py): 0.5 - 0.375 * 2^-11 splits elsewhere
    hi, lo = L.split(np.array([0.5 - 0.375 / 2048.0]))
    assert (hi[0], lo[0]) == (0.5 - 2.0 ** -12, 0.125)
    h, l = L.lattice((4096,), 5)
    assert set(np.unique(h)) == set(L.HI_SET) and set(np.unique(l)) == set(L.LO_SET)
    sh, sl = L.split(h + l / 2048.0)
    assert np.array_equal(sh, h) and np.array_equal(sl, l)
    b = L.lattice_bias(64, 9)
    assert np.array_equal(b * 4, np.round(b * 4)) and np.abs(b).max() <= 2.0 and len(np.unique(b)) > 8


def test_impulse_sites_reach_every_border_class():
    for dims in ((6, 10, 20), (16, 16, 16), (4, 4, 4), (4, 8, 32)):
        sites = L.impulse_sites((1, 8) + dims)
        classes = {L.border_class(s[2:], dims) for s in sites}
        for name in "zyx":
            assert any(name + "0" in c.split() for c in classes) and any(name + "N" in c.split() for c in classes), (dims, name)
        assert "z0 y0 x0" in classes and "zN yN xN" in classes                         # corners
        if dims != (4, 4, 4):                                                                 # (4^3: every site is a corner)
            assert any(len(c.split()) == 2 for c in classes) and any(len(c.split()) == 1 for c in classes)   # edges, faces
        pos = np.array([s[2:] for s in sites])
        for a in range(3):
            u = np.unique(pos[:, a])
            assert (np.diff(u) >= 3).all()                                                # 3-tap footprints never overlap
        assert [s[1] for s in sites[:8]] == list(range(8))                                # the channel cycles


@pytest.mark.parametrize("key", LATTICE_KEYS, ids=_id)
def test_lattice_case_conditions(key):
    kind, cin, cout, shape, ks, stride = key
    hi_case = L.case_from_key(key, "hi")
    lo_case = L.case_from_key(key, "lo")
    # ---- exactness: the split is the identity on the parts; the hi-lattice expectation is a float32 value
    for c in (hi_case, lo_case):
        for v, h, l in ((c.x.numpy(), c.hi_x, c.lo_x), (c.w.numpy(), c.hi_w, c.lo_w)):
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
            sh, sl = L.split(v)
            assert np.array_equal(sh, h) and np.array_equal(sl, l)
    assert torch.equal(hi_case.E.float().double(), hi_case.E) and bool((hi_case.tol >= 0).all())
    assert bool((hi_case.X == 0).all())
    assert np.array_equal(hi_case.hi_x, lo_case.hi_x) and np.array_equal(hi_case.hi_w, lo_case.hi_w)
    # ---- sum condition
    s = L.abs_sum(kind, lo_case.hi_x, lo_case.lo_x, lo_case.hi_w, lo_case.lo_w, lo_case.b.numpy(), ks, stride)
    assert float(s.max()) < L.SUM_BOUND, float(s.max())
    # ---- coverage: outputs per (cin, tap) at which a non-zero activation is multiplied
    for part in (lo_case.hi_x, lo_case.lo_x):
        nz = torch.from_numpy((part != 0).astype(np.float64))
        if kind == "convT":
            counts = nz.sum((0,) + tuple(range(2, nz.dim())))                             # every tap multiplies every input voxel
            assert float(counts.min()) >= 1
        else:
            one = torch.zeros((len(L.taps(kind, ks)), 1) + (ks,) * (nz.dim() - 2), dtype=torch.float64)
            for i, t in enumerate(L.taps(kind, ks)):
                one[(i, 0) + t] = 1.0
            per = L._conv(kind, nz.sum(0).unsqueeze(1), one, ks, stride)                 # channels as the batch: (cin, taps, *out)
            counts = per.sum(tuple(range(2, per.dim())))                                   # (cin, taps)
            assert float(counts.min()) >= 1, (float(counts.min()), np.argwhere(counts.numpy() < 1)[:4].tolist())
    # ---- teeth
    ratios = L.piece_fault_ratios(lo_case)
    assert len(ratios) == len(L.taps(kind, ks)) * ((cin + 7) // 8)
    worst = min(ratios, key=ratios.get)
    assert ratios[worst] >= TEETH, (worst, ratios[worst])
    assert L.border_plane_fault_ratio(lo_case) >= TEETH
    if len(L.taps(kind, ks)) > 1:
        assert L.tap_swap_fault_ratio(lo_case) >= TEETH and L.tap_swap_fault_ratio(hi_case) >= TEETH
    # ---- the report names what moved
    bad = lo_case.E.clone()
    idx = (0,) * bad.dim()
    bad[idx] += 3 * L.UNIT
    msg = L.report(bad, lo_case.E, lo_case.tol)
    assert "1 of" in msg and "+3.000 units" in msg and str(idx) in msg and ("z0" in msg or "y0" in msg)
    assert L.report(lo_case.E, lo_case.E, lo_case.tol) == ""


@pytest.mark.parametrize("key", IMPULSE_KEYS, ids=_id)
@pytest.mark.parametrize("form", ["imp_a", "imp_b"])
def test_impulse_case_conditions(key, form):
    kind, cin, cout, shape, ks, stride = key
    c = L.case_from_key(key, form)
    for v, h, l in ((c.x.numpy(), c.hi_x, c.lo_x), (c.w.numpy(), c.hi_w, c.lo_w)):
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
        sh, sl = L.split(v)
        assert np.array_equal(sh, h) and np.array_equal(sl, l)
    # at most one product per output, each term exact in float32
    nz = torch.from_numpy((c.hi_x != 0).astype(np.float64))
    ones = torch.ones(L.weight_shape(kind, cin, cout, ks), dtype=torch.float64)
    assert float(L._conv(kind, nz, ones, ks, stride).max()) == 1.0
    for term in (c.M, c.X):
        assert torch.equal(term.float().double(), term)
    # full operands: the last significand bit of hi and of lo is in use somewhere (11 bits each)
    full = (c.hi_x, c.lo_x) if form == "imp_a" else (c.hi_w, c.lo_w)
    for part in full:
        m, _ = np.frexp(part[part != 0])
        assert (np.round(np.abs(m) * 2048) % 2 == 1).all()
    assert L.lo_rounded_fault_ratio(c, bits=5) >= TEETH
    # the report reads the tap and the channel from the coordinates
    idx = tuple(int(v) for v in (c.E != 0).nonzero()[0])
    bad = c.E.clone()
    bad[idx] *= 1.0 + 2.0 ** -12
    msg = L.report(bad, c.E, c.tol, c)
    assert " tap (" in msg and " channel " in msg
    tap, ch = L._impulse_source(c, idx)
    w = c.w[(ch, idx[1]) + tap] if kind == "convT" else c.w[(idx[1], ch) + tap]
    site = next(s for s in c.sites if s[0] == idx[0] and s[1] == ch)
    assert float(c.E[idx]) == float(c.x[site]) * float(w)                               # 22 x 11 bits: exact in float64


def test_composed_hi_lattice_cases_stay_exact():
    """planar hand-over and fused up-convolution: lo = 0 throughout, so every partial sum is a multiple of 2^-3 and exact in float32
    below 2^20; the handed-over / up-convolved intermediate is fp16-exact (a multiple of 2^-2 below 2^9), its lo plane zero"""
    def fp16_exact(t):
        return torch.equal(t.half().double(), t) and bool((t * 4 == (t * 4).round()).all())
    for shape in L.PLANAR_SHAPES:
        p = L.planar_case(tuple(shape))
        assert p.bound < L.HI_ONLY_BOUND and fp16_exact(p.y) and torch.equal(p.E2.float().double(), p.E2)
        assert float((p.y > 0).double().mean()) > 0.2                       # the ReLU leaves a dense second input
    cases = [L.upfused_case(tuple(s), 16, 8, 8, 8) for s, _ in L.UPFUSE_XP8W] + [L.upfused_case(tuple(s), 32, 16, 0, 16) for s in L.UPFUSE_ZC16]
    for u in cases:
        assert u.bound < L.HI_ONLY_BOUND and fp16_exact(u.up) and torch.equal(u.E.float().double(), u.E)
        assert bool((u.E * 8 == (u.E * 8).round()).all())


def test_matrix_rows_route_to_the_named_instances(vxcfg):
    """the dry run of the route (vx_conv3d_k3_route) names, for every row and every launch form of the GPU test, the family and instance
    the row is there for -- a row that another family would take is a mistake in the matrix, found here and not on the GPU"""
    import ctypes as C
    from values_amd import _lib
    from tests.conv3d_route_cases import dry_run
    lib = _lib.load()
    for cid, fam, cfg, ci, co, (n, d, h, w), kw, name, sname in L.CONV3D_CASES + L.CONV3D_FP32_CASES:
        vxcfg.restore()
        vxcfg.set(**dict(dict(conv_fp32=0), **cfg))
        pads = {"s16": dict(out_pitch=co + 16, out_coff=8), "fp32": dict(out_pitch=co + 16, out_coff=8), "deep": dict(out_pitch=co + 8, out_coff=4),
                "xp8w": dict(out_xblk=4, out_half=1, out_pitch=8), "zc16": dict(out_xblk=4, out_half=1, out_pitch=32)}[fam]
        forms = {"plain": {}, "padded": pads, "stats": dict(stats_partial=0x50000), "relu": dict(act=_lib.VX_ACT_RELU),
                 "lrelu+hash": dict(act=_lib.VX_ACT_LRELU, drop_mode=_lib.VX_DROP_HASH)}
        for form, extra in forms.items():
            a = _lib.ConvArgs()
            a.in_, a.w_packed, a.bias, a.out = 0x10000, 0x20000, 0x30000, 0x40000
            a.in_pitch, a.out_pitch, a.out_coff = kw.get("in_pitch", ci), co, 0
            a.in_xblk = kw.get("xblk", 0)
            a.N, a.D, a.H, a.W, a.Cin, a.Cout = n, d, h, w, ci, co
            a.w_family = lib.vx_conv3d_k3_family(ci, co)
            for k, v in extra.items():
                setattr(a, k, v)
            rc, kn = dry_run(lib, a)
            want = (sname or L._S16) if form == "stats" else name
            assert rc == 0 and kn.startswith(want), (cid, form, rc, kn, want)


@pytest.mark.parametrize("key", LATTICE_KEYS, ids=_id)
def test_statistics_conditions_are_recorded(key):
    """the GPU test asks for exact statistics where these hold; the sum column must be exact for EVERY case"""
    E = L.case_from_key(key, "hi").E
    sum_ok, _ = L.stats_exact(E)
    assert sum_ok
