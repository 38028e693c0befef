"""GPU: every dispatch branch of the uncertainty reduction family (unc_reduce.hip, vx_softmax_accumulate) against the
float64 restatement in tests/reduce_ref.py: the extras of vx_unc_reduce_ex (variance, in_count, out_count) in f32 and
f64, every class-count instance of the fused logit kernel and of the statistics pair, second trips of the grid-stride
loops, the scalar fall-back for misaligned pointers, logits at -inf, and the sliding-window accumulation with
overlapping and overhanging patches.

Tolerances.  Plain maps and the mean on paths without counts keep the bounds test_gpu_kernels.py holds these kernels
to (5e-6 / 2e-6).  Where the kernel works on un-normalised sums (counts up to 8) rounding scales with the count, so
the bound comes from the REFERENCE: reduce_ref.maps evaluated once in float64 and once with the input and every
accumulator rounded to float32, over the inputs of test_extras_against_float64; the largest difference is the GAP_*
below (tests/test_reduce_ref_cpu.py recomputes them), and the contract bound is max(5e-6, 4 x gap) -- the factor 4
covers the kernel's different summation order and the hardware exp / log / rcp forms (< 5e-8 absolute on a
probability, unc_reduce.hip).  OBS is the largest device deviation measured on an MI355X over this module (f32 and
f64 inputs), REG a regression bound at 5 x that where it is tighter than the contract, asserted beside each contract
bound.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import reduce_ref as rr
from tests.formula import formula_tensor
from values_amd import _lib

pytestmark = pytest.mark.gpu

# ---- bounds (see the module docstring) ----------------------------------------------------------------------------
PLAIN_MAPS, PLAIN_MEAN = 5e-6, 2e-6                   # as test_unc_reduce_logits_and_probs_vs_oracle
GAP_COUNT_MAPS = 3.82e-6                               # float64 vs float32 reference, maps of sums / divided by counts
GAP_COUNT_MEAN = 6.7e-7                                # ... their mean
GAP_VARIANCE = 1.57e-6                                # ... the variance map, every extras case
COUNT_MAPS = max(5e-6, 4 * GAP_COUNT_MAPS)
COUNT_MEAN = max(5e-6, 4 * GAP_COUNT_MEAN)
VARIANCE = max(5e-6, 4 * GAP_VARIANCE)
OBS = {"plain_maps": 7.16e-7, "plain_mean": 1.47e-7, "count_maps": 4.77e-6, "count_mean": 6.68e-7, "variance": 4.18e-6}
CONTRACT = {"plain_maps": PLAIN_MAPS, "plain_mean": PLAIN_MEAN, "count_maps": COUNT_MAPS, "count_mean": COUNT_MEAN,
            "variance": VARIANCE}
REG = {k: min(CONTRACT[k], 5 * OBS[k]) for k in CONTRACT}       # (count_maps, variance: the contract is the tighter one)
ARGMAX_EXCLUDED = 0.005                               # share of voxels the top-2 margin may take out of an arg-max check

MAPS = ("pred_entropy", "expected_entropy", "mutual_information")
COUNT_CYCLE = np.array([0, 1, 2, 3, 8], dtype=np.float32)
SENT_F, SENT_U8 = -77.0, 201


def _np(t):
    return t.detach().cpu().numpy()


def _close(got, want, group, name):
    """contract and regression bound of `group` on the whole array; the first and the last 1024 elements of the voxel
    axis first, so that a failure in a loop's tail is named as such"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert not np.isnan(got).any(), f"{name}: NaN"
    if got.shape[-1] > 4096:
        for part, sl in (("head", slice(0, 1024)), ("tail", slice(-1024, None))):
            e = float(np.abs(got[..., sl] - want[..., sl]).max())
            assert e <= CONTRACT[group], f"{name} [{part}]: {e:.3e} > {CONTRACT[group]:.1e}"
    err = float(np.abs(got - want).max()) if got.size else 0.0
    print(f"deviation {group} {name} {err:.3e}")
    assert err <= CONTRACT[group], f"{name}: {err:.3e} > contract {CONTRACT[group]:.1e}"
    assert err <= REG[group], f"{name}: {err:.3e} > regression bound {REG[group]:.1e}"


def _equal_on(got, want, mask, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape == mask.shape, (name, got.shape, want.shape, mask.shape)
    excluded = 1.0 - float(mask.mean())
    assert excluded <= ARGMAX_EXCLUDED, f"{name}: the margin excludes {excluded:.4%} of the voxels"
    if got.shape[-1] > 4096:
        assert (got[..., :1024] == want[..., :1024])[mask[..., :1024]].all(), f"{name} [head]"
        assert (got[..., -1024:] == want[..., -1024:])[mask[..., -1024:]].all(), f"{name} [tail]"
    bad = (got != want) & mask
    assert not bad.any(), f"{name}: {int(bad.sum())} differ, first at {tuple(np.argwhere(bad)[0])}"


def _check_maps(m, ref, counted, name, sample_mask=None, zero=None):
    """m: uncertainty_maps' dict for x (B, T, C, nvox); ref: reduce_ref.maps of the same input.  zero (B, nvox) bool:
    voxels whose input is all zeros (count 0 in the sums): a tie both sides break towards class 0, so they stay in the
    arg-max check."""
    g = "count" if counted else "plain"
    for k in MAPS:
        _close(_np(m[k]), ref[k], g + "_maps", f"{name} {k}")
    if "mean_softmax" in m:
        _close(_np(m["mean_softmax"]), ref["mean_softmax"], g + "_mean", f"{name} mean_softmax")
    if "softmax_variance" in m:
        _close(_np(m["softmax_variance"]), ref["variance"], "variance", f"{name} variance")
    clear = rr.clear_mean(ref["mean_softmax"])
    if zero is not None:
        clear = clear | zero
    if "argmax" in m:
        _equal_on(_np(m["argmax"]), ref["argmax"], clear, f"{name} argmax")
    if "sample_argmax" in m:
        _equal_on(_np(m["sample_argmax"]), ref["sample_argmax"], sample_mask, f"{name} sample_argmax")


def _counts(B, nvox):
    return COUNT_CYCLE[np.arange(B * nvox) % len(COUNT_CYCLE)].reshape(B, nvox)


def extras_case(from_logits, extras, nvox, T, Cc, np_dtype, B=2):
    """inputs of one case of test_extras_against_float64 (numpy only: test_reduce_ref_cpu.py measures the float32 gap of
    the reference on the same arrays).  -> x (B, T, C, nvox) of np_dtype, kwargs of the count maps, counts"""
    logits = formula_tensor((B, T, Cc, nvox), 700 + 10 * T + Cc + (nvox & 1), scale=4.0)
    cnt = _counts(B, nvox)
    if from_logits:
        x = logits
    else:   # un-normalised sums as the accumulator leaves them: count x softmax, zeros where no patch reached
        from oracle import uncertainty_oracle as uo
        x = uo.softmax(logits, axis=2) * cnt[:, None, None, :].astype(np.float64)
    kw = {"var": {}, "out": {"out_count": cnt}, "in": {"in_count": cnt}}[extras]
    return x.astype(np_dtype), kw, cnt


EXTRAS_CASES = [(fl, ex, nvox, T, Cc) for fl in (False, True) for ex in (("var", "out") if fl else ("var", "out", "in"))
                for nvox in (1028, 1029) for (T, Cc) in ((1, 2), (5, 3), (4, 8))]


# ---- a. the extras of vx_unc_reduce_ex ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("from_logits,extras,nvox,T,Cc", EXTRAS_CASES)
def test_extras_against_float64(dtype, from_logits, extras, nvox, T, Cc):
    from values_amd import uncertainty_maps
    x, kw, cnt = extras_case(from_logits, extras, nvox, T, Cc, np.float32 if dtype == torch.float32 else np.float64)
    ref = rr.maps(x, from_logits, **kw)
    m = uncertainty_maps(torch.from_numpy(x).cuda(), from_logits=from_logits, want_sample_argmax=True, want_variance=True,
                         **{k: torch.from_numpy(v).cuda() for k, v in kw.items()})
    counted = (not from_logits) or extras != "var"
    xe = x.astype(np.float64) / np.clip(cnt, 1, None)[:, None, None, :] if extras == "in" else x
    zero = None if from_logits else np.broadcast_to(cnt == 0, (x.shape[0], nvox))
    smask = rr.clear_sample(xe, from_logits)
    if zero is not None:
        smask = smask | zero[:, None, :]
    name = f"{'logits' if from_logits else 'sums'} {extras} {nvox} T{T} C{Cc}"
    _check_maps(m, ref, counted, name, smask, zero)
    for k, t in m.items():
        assert not torch.isnan(t.float()).any(), k
    if zero is not None:    # no patch reached the voxel: zero maps, class 0
        z = torch.from_numpy(zero.copy()).cuda()
        assert z.any()
        for k in MAPS + ("softmax_variance", "argmax"):
            assert (m[k][z] == 0).all(), k
        assert (m["mean_softmax"].permute(0, 2, 1)[z] == 0).all()
        assert (m["sample_argmax"].permute(0, 2, 1)[z] == 0).all()


def test_in_count_with_logits_is_refused():
    from values_amd import uncertainty_maps
    x = torch.zeros((1, 2, 3, 16), device="cuda")
    with pytest.raises(_lib.VxError, match=r"rc=-3\).*in_count applies to probability sums, not to logits"):
        uncertainty_maps(x, from_logits=True, in_count=torch.ones((1, 16), device="cuda"))
    o = _lib.UncOutputs()
    t = torch.zeros(16, device="cuda")
    o.pred_entropy = o.exp_entropy = o.mutual_info = o.in_count = _lib.ptr(t)
    rc = _lib.load().vx_unc_reduce_ex(_lib.ptr(x), _lib.VX_F32, 1, 1, 2, 3, 16, C.byref(o), _lib.stream_ptr())
    assert rc == -3 and b"in_count" in _lib.load().vx_last_error_string()      # VX_E_DTYPE


@pytest.mark.parametrize("from_logits", [False, True])
def test_out_rows_of_a_larger_batch_are_written_and_their_neighbours_kept(from_logits):
    from values_amd.uncertainty import alloc_uncertainty_maps, uncertainty_maps
    B, T, Cc, nvox = 2, 5, 3, 1028
    x, kw, _ = extras_case(from_logits, "out", nvox, T, Cc, np.float32)
    xd = torch.from_numpy(x).cuda()
    cnt = torch.from_numpy(kw["out_count"]).cuda()
    want = uncertainty_maps(xd, from_logits=from_logits, want_sample_argmax=True, want_variance=True, out_count=cnt)
    big = alloc_uncertainty_maps(B + 2, T, Cc, (nvox,), xd.device, want_sample_argmax=True, want_variance=True)
    for t in big.values():
        t.fill_(SENT_U8 if t.dtype == torch.uint8 else SENT_F)
    got = uncertainty_maps(xd, from_logits=from_logits, out={k: t[1:1 + B] for k, t in big.items()}, out_count=cnt)
    assert set(got) == set(want)
    for k, t in big.items():
        sent = SENT_U8 if t.dtype == torch.uint8 else SENT_F
        assert torch.equal(t[1:1 + B], want[k]), k
        assert (t[0] == sent).all() and (t[-1] == sent).all(), k


# ---- b. every instance of the fused logit kernel and of the statistics pair ------------------------------------------
def _stats_maps(parts, T_total, Cc, nvox):
    """vx_unc_stats_accumulate over the (B, T_i, C, nvox) parts into one zeroed buffer, then vx_unc_stats_finalize"""
    lib = _lib.load()
    B = parts[0].shape[0]
    dev = parts[0].device
    st = torch.zeros((B, Cc + 1, nvox), dtype=torch.float32, device=dev)
    for p in parts:
        p = p.contiguous()
        _lib.check(lib.vx_unc_stats_accumulate(_lib.ptr(p), B, p.shape[1], Cc, nvox, _lib.ptr(st), _lib.stream_ptr()),
                   "vx_unc_stats_accumulate")
    out = {k: torch.empty((B, nvox), dtype=torch.float32, device=dev) for k in MAPS}
    out["mean_softmax"] = torch.empty((B, Cc, nvox), dtype=torch.float32, device=dev)
    out["argmax"] = torch.empty((B, nvox), dtype=torch.uint8, device=dev)
    _lib.check(lib.vx_unc_stats_finalize(_lib.ptr(st), B, T_total, Cc, nvox, _lib.ptr(out["mean_softmax"]),
                                         _lib.ptr(out["pred_entropy"]), _lib.ptr(out["expected_entropy"]),
                                         _lib.ptr(out["mutual_information"]), _lib.ptr(out["argmax"]), _lib.stream_ptr()),
               "vx_unc_stats_finalize")
    return out


@pytest.mark.parametrize("nvox", [260, 257])
@pytest.mark.parametrize("Cc", [2, 3, 4, 5, 6, 7, 8])
def test_every_class_count_instance_against_float64(Cc, nvox):
    from values_amd import uncertainty_maps
    B, T = 2, 3
    logits = formula_tensor((B, T, Cc, nvox), 740 + Cc, scale=4.0)
    for dtype in (np.float32, np.float64):
        x = logits.astype(dtype)
        ref = rr.maps(x, True)
        smask = rr.clear_sample(x, True)
        xd = torch.from_numpy(x).cuda()
        m = uncertainty_maps(xd, from_logits=True, want_sample_argmax=True)
        _check_maps(m, ref, False, f"logit C{Cc} {nvox} {np.dtype(dtype).name}", smask)
        if dtype == np.float32:   # (the statistics kernels take float32 logits)
            s = _stats_maps([xd[:, :1], xd[:, 1:]], T, Cc, nvox)
            _check_maps(s, ref, False, f"stats C{Cc} {nvox}")


# ---- c. second trips of the grid-stride loops --------------------------------------------------------------------
N_BIG = 4 * 8192 * 256 + 4         # unc_reduce / unc_stats vector path: 8192 blocks x 256 threads x 4 voxels, and one more group
N_SCALAR = 8192 * 256 + 5          # ... the scalar path
N_16K = 16384 * 256 + 77           # the element-wise kernels capped at 16384 blocks


@pytest.fixture(scope="module")
def big():
    """(1, 1, 2, N_BIG) logits, their float64 class softmax and reference maps -- computed once; every reduction here is
    per voxel, so a test on fewer voxels takes a slice"""
    logits = formula_tensor((1, 1, 2, N_BIG), 760, scale=4.0).astype(np.float32)
    ref = rr.maps(logits, True)
    p = ref["mean_softmax"][:, None]          # T = 1: the mean IS the sample's float64 softmax
    for v in list(ref.values()) + [logits]:
        v.setflags(write=False)
    return {"logits": logits, "p": p, "ref": ref, "smask": rr.clear_mean(p)}


def _cut(big, n):
    ref = {k: v[..., :n] for k, v in big["ref"].items()}
    return big["logits"][..., :n].copy(), ref, big["smask"][..., :n]


@pytest.mark.parametrize("n", [N_BIG, N_SCALAR], ids=["vector", "scalar"])
def test_reduction_takes_a_second_loop_trip(big, n):
    from values_amd import uncertainty_maps
    x, ref, smask = _cut(big, n)
    m = uncertainty_maps(torch.from_numpy(x).cuda(), from_logits=True, want_sample_argmax=True, want_variance=True)
    _check_maps(m, ref, False, f"logits {n}", smask)


def test_statistics_pair_takes_a_second_loop_trip(big):
    x, ref, _ = _cut(big, N_BIG)
    s = _stats_maps([torch.from_numpy(x).cuda()], 1, 2, N_BIG)
    _check_maps(s, ref, False, f"stats {N_BIG}")


def test_elementwise_kernels_take_a_second_loop_trip(big):
    from oracle import uncertainty_oracle as uo
    from values_amd import calculate_one_minus_msr, uncertainty_maps
    from values_amd.uncertainty import softmax_variance
    lib = _lib.load()
    n = N_16K
    lg, p = big["logits"][0, 0], big["p"][0, 0]
    # vx_softmax_planar, C = 3
    z = np.stack([lg[0, :n], lg[1, :n], lg[0, -n:]])
    zd = torch.from_numpy(z).cuda()
    out = torch.full_like(zd, SENT_F)
    _lib.check(lib.vx_softmax_planar(_lib.ptr(zd), 1, 3, n, _lib.ptr(out), _lib.stream_ptr()), "vx_softmax_planar")
    _close(_np(out), uo.softmax(z.astype(np.float64), axis=0), "plain_mean", f"softmax_planar {n}")
    # the probability path: sample_argmax_kernel beside the reduction
    p32 = np.ascontiguousarray(p[:, :n]).astype(np.float32)
    _, ref, smask = _cut(big, n)
    m = uncertainty_maps(torch.from_numpy(p32).cuda()[None, None], from_logits=False, want_sample_argmax=True)
    _check_maps(m, ref, False, f"probabilities {n}", smask)
    # calculate_one_minus_msr: exact in the input's precision
    r = calculate_one_minus_msr(torch.from_numpy(p32).cuda())["pred_entropy"]
    want = np.float32(1) - p32.max(0)
    got = _np(r)
    assert np.array_equal(got[:1024], want[:1024]) and np.array_equal(got[-1024:], want[-1024:])
    assert np.array_equal(got, want)
    # vx_softmax_variance, T = 2, C = 2
    x2 = np.stack([lg[:, :n], lg[:, -n:]])[None]
    want = np.stack([p[:, :n], p[:, -n:]]).var(axis=0).mean(axis=0)[None]
    _close(_np(softmax_variance(torch.from_numpy(x2).cuda(), from_logits=True)), want, "variance", f"softmax_variance {n}")


# ---- d. misaligned pointers through the C ABI ---------------------------------------------------------------------
class _Buf:
    """a device array inside a sentinel-filled buffer of its own: 16 bytes of sentinel before it (plus `off` elements,
    which take the pointer off its alignment) and at least 16 bytes after it"""

    def __init__(self, shape, dtype, off, data=None):
        n = int(np.prod(shape))
        pad = 16 if dtype == torch.uint8 else 4
        self.sent = SENT_U8 if dtype == torch.uint8 else SENT_F
        self.full = torch.full((n + 3 * pad,), self.sent, dtype=dtype, device="cuda")
        assert self.full.data_ptr() % 16 == 0
        self.lo, self.n = pad + off, n
        self.view = self.full[self.lo:self.lo + n]
        if data is not None:
            self.view.copy_(data.reshape(-1))
        self.shape = tuple(shape)

    def guards_kept(self):
        return bool((self.full[:self.lo] == self.sent).all() and (self.full[self.lo + self.n:] == self.sent).all())


MISALIGN = {False: ["x", "mean_softmax", "pred_entropy", "expected_entropy", "mutual_information", "softmax_variance",
                    "in_count", "out_count", "argmax", "sample_argmax", "all"],
            True: ["x", "mean_softmax", "pred_entropy", "expected_entropy", "mutual_information", "softmax_variance",
                   "out_count", "argmax", "sample_argmax", "all"]}


def _raw_reduce(x, from_logits, cnt, shape, off):
    """vx_unc_reduce_ex on buffers of the test's own; off: name -> element offset.  -> dict of _Buf"""
    B, T, Cc, nvox = shape
    f32, u8 = torch.float32, torch.uint8
    bufs = {"x": _Buf(shape, f32, off.get("x", 0), x), "out_count": _Buf((B, nvox), f32, off.get("out_count", 0), cnt)}
    if not from_logits:
        bufs["in_count"] = _Buf((B, nvox), f32, off.get("in_count", 0), cnt)
    for k in MAPS + ("softmax_variance",):
        bufs[k] = _Buf((B, nvox), f32, off.get(k, 0))
    bufs["mean_softmax"] = _Buf((B, Cc, nvox), f32, off.get("mean_softmax", 0))
    bufs["argmax"] = _Buf((B, nvox), u8, off.get("argmax", 0))
    bufs["sample_argmax"] = _Buf((B, T, nvox), u8, off.get("sample_argmax", 0))
    o = _lib.UncOutputs()
    p = {k: _lib.ptr(b.view) for k, b in bufs.items()}
    o.mean_prob, o.pred_entropy, o.exp_entropy, o.mutual_info = (p["mean_softmax"], p["pred_entropy"], p["expected_entropy"],
                                                               p["mutual_information"])
    o.variance, o.argmax, o.sample_argmax = p["softmax_variance"], p["argmax"], p["sample_argmax"]
    o.in_count, o.out_count = p.get("in_count"), p["out_count"]
    rc = _lib.load().vx_unc_reduce_ex(p["x"], _lib.VX_F32, int(from_logits), B, T, Cc, nvox, C.byref(o), _lib.stream_ptr())
    _lib.check(rc, "vx_unc_reduce_ex")
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("from_logits,which", [(fl, w) for fl in (False, True) for w in MISALIGN[fl]])
def test_misaligned_pointers_take_the_scalar_path_with_the_same_bits(from_logits, which):
    shape = (2, 3, 3, 1024)
    x, kw, cnt = extras_case(from_logits, "out", 1024, 3, 3, np.float32)
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(cnt).cuda()
    names = MISALIGN[from_logits][:-1]
    off = {k: 1 for k in (names if which == "all" else [which])}
    ref = _raw_reduce(xd, from_logits, cd, shape, {})
    got = _raw_reduce(xd, from_logits, cd, shape, off)
    for k, b in got.items():
        assert (b.view.data_ptr() % (4 if b.full.dtype == torch.uint8 else 16) != 0) == (k in off), k
        assert torch.equal(b.view, ref[k].view), f"{k} differs from the aligned call"
        assert b.guards_kept() and ref[k].guards_kept(), f"{k}: written outside the array"
        assert not (b.view == b.sent).all(), f"{k} was not written"
    # ... and the aligned call is the right answer
    want = rr.maps(x, from_logits, out_count=cnt, **({} if from_logits else {"in_count": cnt}))
    for k in MAPS:
        _close(_np(ref[k].view).reshape(2, -1), want[k], "count_maps", f"raw {k}")


# ---- e. logits at -inf ---------------------------------------------------------------------------------------------
def _masked_logits(Cc, nvox, T=2, B=1):
    """rows with one class at -inf in one sample, two classes at -inf in every sample, and classes so far below the
    maximum that their exponential underflows (-200, -1e30)"""
    x = formula_tensor((B, T, Cc, nvox), 780 + Cc, scale=4.0)
    v = np.arange(nvox)
    c1, c2 = v % Cc, (v + 1) % Cc
    kind = v % 5            # (kind 4: untouched)
    for b in range(B):
        x[b, 0, c1[kind == 0], v[kind == 0]] = -np.inf
        for t in range(T):
            x[b, t, c1[kind == 1], v[kind == 1]] = -np.inf
            x[b, t, c2[kind == 1], v[kind == 1]] = -np.inf
            x[b, t, c1[kind == 2], v[kind == 2]] = -200.0
        x[b, T - 1, c2[kind == 3], v[kind == 3]] = -1e30
    return x


@pytest.mark.parametrize("nvox", [260, 257], ids=["vector", "scalar"])
@pytest.mark.parametrize("Cc", [3, 8])
def test_masked_classes_give_the_reference_maps_not_nan(Cc, nvox):
    """A class logit of -inf is p = 0 exactly; the reference softmaxes first and skips the NaN product 0 * log 0
    (test_3D.py:503-504), so its maps are finite.  The log-softmax form p * (z - m - log den) is 0 * -inf there."""
    from values_amd import uncertainty_maps
    logits = _masked_logits(Cc, nvox)
    assert np.isinf(logits).any()
    for dtype in (np.float32, np.float64):
        x = logits.astype(dtype)
        ref = rr.maps(x, True)
        assert all(np.isfinite(v).all() for v in ref.values())
        smask = rr.clear_sample(x, True)
        xd = torch.from_numpy(x).cuda()
        for want_variance in (False, True):
            m = uncertainty_maps(xd, from_logits=True, want_sample_argmax=True, want_variance=want_variance)
            for k, t in m.items():
                assert torch.isfinite(t.float()).all(), f"{k}: not finite ({np.dtype(dtype).name}, variance={want_variance})"
            _check_maps(m, ref, False, f"masked C{Cc} {nvox} {np.dtype(dtype).name} var={want_variance}", smask)
        if dtype == np.float32:
            s = _stats_maps([xd[:, :1], xd[:, 1:]], 2, Cc, nvox)
            for k, t in s.items():
                assert torch.isfinite(t.float()).all(), f"stats {k}: not finite"
            _check_maps(s, ref, False, f"masked stats C{Cc} {nvox}")


# ---- f. vx_softmax_accumulate ----------------------------------------------------------------------------------------
ACC_SUM = 2e-6          # as test_accumulate_matches_reference_concat_data (sums of up to 8 softmax values there, 4 here)


def _accumulate(logits, crops, image, overlap):
    lib = _lib.load()
    B, T, Cc, P0, P1, P2 = logits.shape
    ssum = torch.zeros((T, Cc) + tuple(image), dtype=torch.float32, device="cuda")
    count = torch.zeros(tuple(image), dtype=torch.float32, device="cuda")
    crop_t = torch.tensor(crops, dtype=torch.int32, device="cuda")
    _lib.check(lib.vx_softmax_accumulate(_lib.ptr(logits), B, T, Cc, P0, P1, P2, _lib.ptr(crop_t), _lib.ptr(ssum),
                                         _lib.ptr(count), image[0], image[1], image[2], overlap, _lib.stream_ptr()),
               "vx_softmax_accumulate")
    torch.cuda.synchronize()
    return ssum, count


@pytest.mark.parametrize("Cc", [2, 3, 8])
def test_accumulate_overlapping_and_overhanging_patches(Cc):
    patch, image, T, B = (12, 8, 20), (20, 12, 28), 2, 5
    logits = formula_tensor((B, T, Cc) + patch, 800 + Cc, scale=4.0).astype(np.float32)
    ld = torch.from_numpy(logits).cuda()
    # four patches over one another; the last one hangs over the image on every axis
    crops = [(0, 0, 0), (4, 2, 4), (6, 3, 6), (8, 4, 8), (12, 6, 14)]
    want_sum, want_cnt = rr.accumulate(logits, crops, image)
    assert want_cnt.max() == 4 and want_cnt.min() == 0
    assert all(crops[-1][a] + patch[a] > image[a] for a in range(3))
    ssum, count = _accumulate(ld, crops, image, 1)
    np.testing.assert_array_equal(_np(count), want_cnt)
    err = float(np.abs(_np(ssum) - want_sum).max())
    print(f"deviation accumulate C{Cc} overlapping {err:.3e}")
    assert err <= ACC_SUM
    # disjoint patches (four of them overhanging): one addend per voxel, so atomics and plain stores agree to the bit
    crops = [(0, 0, 0), (12, 0, 0), (0, 8, 0), (0, 0, 20), (12, 8, 20)]
    want_sum, want_cnt = rr.accumulate(logits, crops, image)
    assert want_cnt.max() == 1
    s0, c0 = _accumulate(ld, crops, image, 0)
    s1, c1 = _accumulate(ld, crops, image, 1)
    assert torch.equal(s0, s1) and torch.equal(c0, c1)
    np.testing.assert_array_equal(_np(c0), want_cnt)
    err = float(np.abs(_np(s0) - want_sum).max())
    print(f"deviation accumulate C{Cc} disjoint {err:.3e}")
    assert err <= ACC_SUM


def test_accumulate_takes_a_second_loop_trip():
    patch, B, T, Cc = (96, 80, 64), 3, 3, 2
    assert B * T * patch[0] * patch[1] * patch[2] > 16384 * 256
    image = (96, 80, 3 * 64)
    logits = formula_tensor((B, T, Cc) + patch, 810, scale=4.0).astype(np.float32)
    crops = [(0, 0, 64 * b) for b in range(B)]
    want_sum, want_cnt = rr.accumulate(logits, crops, image)
    ssum, count = _accumulate(torch.from_numpy(logits).cuda(), crops, image, 0)
    np.testing.assert_array_equal(_np(count), want_cnt)
    got = _np(ssum).reshape(T * Cc, -1)
    want = want_sum.reshape(T * Cc, -1)
    for part, sl in (("head", slice(0, 1024)), ("tail", slice(-1024, None)), ("all", slice(None))):
        err = float(np.abs(got[:, sl] - want[:, sl]).max())
        assert err <= ACC_SUM, f"[{part}] {err:.3e}"
    print(f"deviation accumulate stride {err:.3e}")
