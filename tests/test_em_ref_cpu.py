"""CPU: the conditions tests/test_gpu_evalmetrics_matrix.py rests on, proven without a device for the reference, the
bounds and the input matrix of tests/em_ref.py.

* An independent float64 evaluation (tests/em_inputs.platt_sums_raters_numpy and calib_bins_numpy: numpy's libm, numpy's
  pairwise summation, np.digitize and np.bincount) stays inside every bound of every matrix case, its counts and bin ids
  equal the reference's.
* The guard band holds for every voxel: no bin depends on the libm.
* The bounds catch what they are for: nine mutants of a float64 stand-in that walks the elements as the kernel does each
  push a number outside its bound.
In the saturated cases ((A, B) = (40, -7) and beyond) the Hessian sums have little power: P is 1 to the last bit on most
voxels, w = P (1 - P) is dominated by the absolute error u of the subtraction, and the bound, which has to allow that,
is far above the sums themselves.  Those cases are there for the overflow behaviour (finite sums, p = 0 / p = 1 in the
right bins), not for the Hessian."""
import numpy as np
import pytest

from tests import em_ref
from tests.em_inputs import calib_bins_numpy, platt_sums_raters_numpy
from tests.em_ref import EDGES, LD


def _platt_numpy(c):
    return platt_sums_raters_numpy(c.ref, c.pred, c.unc, c.A, c.B, c.t_pos, c.t_neg, c.ignore)


def _valid(c):
    return np.ones(c.ref.shape, dtype=bool) if c.ignore is None else c.ref != c.ignore


@pytest.mark.parametrize("R", em_ref.RATERS)
@pytest.mark.parametrize("ignore", em_ref.IGNORES)
def test_float64_numpy_evaluation_is_inside_every_bound(ignore, R):
    worst_platt, worst_bins = np.zeros(8), 0.0
    for c in em_ref.matrix(ignores=(ignore,), raters=(R,)):
        want, tol = em_ref.platt_reference(c)
        got = np.array(_platt_numpy(c))
        assert np.isfinite(got).all() and np.isfinite(want.astype(np.float64)).all(), c
        assert got[0] == c.n_valid and got[1] == c.n_correct, c
        r = em_ref.ratio(got, want, tol)
        assert (r[2:] < 1).all(), (c, r)
        worst_platt = np.maximum(worst_platt, r)
        bs, bt, bn, ids = calib_bins_numpy(c.ref, c.pred, c.unc, c.A, c.B, c.ignore)
        ws, wt, wn, wtol, wid = em_ref.bins_reference(c)
        assert np.array_equal(bt, wt) and np.array_equal(bn, wn), c
        assert np.array_equal(ids, np.broadcast_to(wid[None], c.ref.shape)[_valid(c)]), c
        rb = em_ref.ratio(bs, ws, wtol)
        assert (rb < 1).all(), (c, rb)
        worst_bins = max(worst_bins, rb.max())
    print(f"R = {R}, ignore {ignore}: largest |err| / tol of the float64 numpy evaluation: "
          + ", ".join(f"{n} {v:.3g}" for n, v in zip(em_ref.SUM_NAMES[2:], worst_platt[2:])) + f"; bin_sums {worst_bins:.3g}")


def test_matrix_is_the_one_the_issue_sets():
    cases = em_ref.matrix()
    assert len(cases) == 2 * 3 * 6 * 2 * 6 and max(c.R * c.nvox for c in cases) == 4 * 300001
    for c in cases:
        lo, hi = float(c.unc.min()), float(c.unc.max())
        assert 0.0 <= lo and hi < 5.0 and (c.nvox < 255 or hi > 0.7), c
        if c.R * c.nvox > 1:
            assert (c.ref == 2).any(), c                          # the ignored label is present
        assert c.n_valid > 0 and (c.ignore is None or c.R * c.nvox == 1) == (c.n_valid == c.R * c.nvox), c
        assert (c.t_pos, c.t_neg) == em_ref.platt_targets(c.n_valid, c.n_correct)
    z = [np.abs(em_ref.terms_of(c)["z"]).max() for c in cases if c.nvox == 300001 and c.R == 1 and c.ignore is None]
    assert sum(v > 36 for v in z) == 6 and sum(v > 709 for v in z) == 4   # (three parameter pairs, two dtypes)


def test_guard_band_holds_for_every_voxel():
    for n in em_ref.SIZES:
        for dt in em_ref.DTYPES:
            for A, B in em_ref.PARAMS:
                vt = em_ref._matrix_voxel_terms(n, dt, A, B)
                assert np.isfinite(vt["P"].astype(np.float64)).all()
                assert em_ref.guard_band_margin(vt) > 0, (n, dt, A, B)
    c = em_ref.special_cases()["mixed"]              # its ordinary voxels; the special values are exact on any libm
    assert em_ref.guard_band_margin(em_ref.voxel_terms(c.unc[np.abs(c.unc) < 1], c.A, c.B)) > 0


def test_reference_sums_are_the_sums_of_their_terms():
    """platt_reference multiplies the linear terms out; term by term (platt_terms) the sums agree to a thousandth of
    the bound at the least"""
    for c in em_ref.matrix(raters=(3,), sizes=(257, 131073), dtypes=(np.float32,)) + em_ref.lattice_cases():
        want, tol = em_ref.platt_reference(c)
        for k, (name, (pos, neg)) in enumerate(em_ref.platt_terms(c).items(), 2):
            by_terms = (c.n_c * pos).sum() + (c.n_w * neg).sum()
            assert name == em_ref.SUM_NAMES[k] and abs(float(by_terms - want[k])) <= 1e-3 * tol[k], (c, name)


def test_lattice_sums_are_exact_in_any_association():
    """A = B = 0 on the lattice m / 1024: every term of sums[3..7] is a multiple of 2^-22 and the sum of their magnitudes
    stays below 2^53 such units, so any order of float64 additions gives the same number, the reference's"""
    for c in em_ref.lattice_cases():
        want, tol = em_ref.platt_reference(c)
        terms = em_ref.platt_terms(c)
        vt = em_ref.terms_of(c)
        assert (vt["z"] == 0).all() and (vt["P"] == 0.5).all() and (vt["w"] == 0.25).all()
        for name in em_ref.SUM_NAMES[3:]:
            units = 0
            for n, t in zip((c.n_c, c.n_w), terms[name]):
                scaled = t * LD(2.0 ** 22)
                assert np.array_equal(scaled, np.rint(scaled)), (c, name)
                units += float((n * np.abs(scaled)).sum())
            assert 0 < units < 2.0 ** 53, (c, name)
        got = np.array(_platt_numpy(c))
        assert np.array_equal(got[[0, 1, 3, 4, 5, 6, 7]].astype(LD), want[[0, 1, 3, 4, 5, 6, 7]]), c
        assert em_ref.ratio(got, want, tol)[2] < 1 and abs(got[2] - c.n_valid * np.log(2.0)) < tol[2]


def test_special_values_fall_in_their_bins_on_any_libm():
    cases = em_ref.special_cases()
    for name, (_, _, _, k) in em_ref.SPECIALS.items():
        c = cases[name]
        ws, wt, wn, _, _ = em_ref.bins_reference(c)
        bs, bt, bn, _ = calib_bins_numpy(c.ref, c.pred, c.unc, c.A, c.B, c.ignore)
        assert wn[k] == c.n_valid and wn.sum() == c.n_valid and wt[k] == c.n_correct, name
        assert np.array_equal(bn, wn) and np.array_equal(bt, wt), name
        assert np.array_equal(bs, ws.astype(np.float64), equal_nan=True), name
        assert np.array_equal(float(ws[k]), {9: 0.5, 19: 1.0, 0: 0.0, 20: np.nan}[k] * c.n_valid, equal_nan=True), name
    c = cases["mixed"]
    ws, wt, wn, wtol, _ = em_ref.bins_reference(c)
    bs, bt, bn, _ = calib_bins_numpy(c.ref, c.pred, c.unc, c.A, c.B, c.ignore)
    assert np.array_equal(bn, wn) and np.array_equal(bt, wt) and wn[[0, 9, 19, 20]].min() >= 5 and wn.sum() == c.n_valid
    assert np.isnan(bs[20]) and np.isnan(ws[20]) and (em_ref.ratio(bs[:20], ws[:20], wtol[:20]) < 1).all()


# ---------------------------------------------------------------------------------------------------------- mutants
MUTANTS = ("drop_last", "next_voxel", "voxel_by_rater_count", "swap_targets", "ignore_on_pred", "T_in_negative_branch",
           "z_float32", "strict_edge", "true_for_sums")


def _standin(c, mutant=None):
    """the eight sums and 63 bin numbers of a case in float64 numpy, element i = rater * nvox + voxel read as
    em_platt_body and em_bins_body read it, with one of MUTANTS applied"""
    i = np.arange(c.R * c.nvox)
    vx = i // c.R if mutant == "voxel_by_rater_count" else i % c.nvox
    src = (vx + 1) % c.nvox if mutant == "next_voxel" else vx
    ref, pred, unc = c.ref.reshape(-1)[i], c.pred[src], c.unc[src].astype(np.float64)
    valid = np.ones(len(i), dtype=bool) if c.ignore is None else (pred if mutant == "ignore_on_pred" else ref) != c.ignore
    if mutant == "drop_last":
        valid[np.flatnonzero(valid)[-1]] = False
    ref, pred, F = ref[valid], pred[valid], -unc[valid]
    correct = ref == pred
    t_pos, t_neg = (c.t_neg, c.t_pos) if mutant == "swap_targets" else (c.t_pos, c.t_neg)
    T = np.where(correct, t_pos, t_neg)
    with np.errstate(over="ignore", invalid="ignore"):
        if mutant == "z_float32":
            z = (np.float32(c.A) * F.astype(np.float32) + np.float32(c.B)).astype(np.float64)
        else:
            z = c.A * F + c.B
        e = np.exp(-np.abs(z))
        P = np.where(z >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
        loss = np.where(z >= 0, T * z, (T if mutant == "T_in_negative_branch" else T - 1.0) * z) + np.log1p(e)
        d, w = T - P, P * (1.0 - P)
        sums = [float(len(F)), float(correct.sum()), loss.sum(), (d * F).sum(), d.sum(), (w * F * F).sum(), (w * F).sum(), w.sum()]
        prob = 1.0 / (1.0 + np.exp(z))
        below = (EDGES[None] < prob[:, None]) if mutant == "strict_edge" else (EDGES[None] <= prob[:, None])
    binid = below.sum(1) - 1
    binid[np.isnan(prob)] = 20
    keep = binid >= 0                                                    # (no edge below the value: the kernel drops it)
    bins = [np.array([prob[binid == k].sum() for k in range(21)]), np.bincount(binid[keep], weights=correct[keep], minlength=21),
            np.bincount(binid[keep], minlength=21).astype(np.float64)]
    if mutant == "true_for_sums":
        bins[0] = bins[1]
    return np.array(sums), bins


def _outside(c, sums, bins):
    want, tol = em_ref.platt_reference(c)
    ws, wt, wn, wtol, _ = em_ref.bins_reference(c)
    ok = ~np.isnan(ws.astype(np.float64))
    return (sums[0] != c.n_valid or sums[1] != c.n_correct or (em_ref.ratio(sums, want, tol)[2:] >= 1).any()
            or not np.array_equal(bins[1], wt) or not np.array_equal(bins[2], wn)
            or (em_ref.ratio(bins[0][ok], ws[ok], wtol[ok]) >= 1).any() or not np.isnan(bins[0][~ok]).all())


def _applies(mutant, c):
    """where a mutant changes what the kernel computes at all"""
    return {"next_voxel": c.nvox > 1, "voxel_by_rater_count": c.R > 1, "ignore_on_pred": c.ignore is not None,
            "T_in_negative_branch": (c.A, c.B) == (2.0, -1.0),           # the other two pairs keep z >= 0 on every voxel
            "z_float32": (c.A, c.B) != (0.0, 0.0),                       # z = 0 exactly in either format
            "strict_edge": False}.get(mutant, True)                      # the guard band keeps p off every edge: see below


@pytest.fixture(scope="module")
def mutant_cases():
    params = ((-3.5, 1.25), (0.0, 0.0), (2.0, -1.0))
    return em_ref.matrix(params=params, sizes=(257,)) + em_ref.matrix(ignores=(2,), params=params, raters=(3,), sizes=(131073,),
                                                                      dtypes=(np.float32,))


def test_standin_is_inside_every_bound_before_it_is_mutated(mutant_cases):
    for c in mutant_cases + list(em_ref.special_cases().values()):
        sums, bins = _standin(c)
        assert not _outside(c, sums, bins), c
        with np.errstate(invalid="ignore"):                               # (the special maps hold inf and NaN)
            assert np.array_equal(sums[:2], _platt_numpy(c)[:2])


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_leaves_a_bound(mutant, mutant_cases):
    """Each fault of the list pushes a sum or a bin outside its bound on every case on which it changes the arithmetic:
    (A, B) = (-3.5, 1.25) and (0, 0), and (2, -1) besides, because the first two keep z >= 0 on every voxel and never
    enter the z < 0 branch.  `<` for `<=` in the bin search can only show where p equals an edge; the guard band keeps
    the matrix off the interior edges, so that mutant is held to the p = 0 items (edge 0) of special_cases()."""
    if mutant == "strict_edge":
        hit = {name: c for name, c in em_ref.special_cases().items() if name in ("zero", "inf_neg_a", "mixed")}
    else:
        hit = {repr(c): c for c in mutant_cases if _applies(mutant, c)}
    assert len(hit) >= 3
    for name, c in hit.items():
        assert _outside(c, *_standin(c, mutant)), (mutant, name)
