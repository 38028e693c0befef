"""High-precision reference, error bounds and the input matrix for the calibration half of values_amd/csrc/evalmetrics.hip
(vx_platt_sums_batched: loss, gradient and Hessian sums of the Platt fit; vx_calib_bins_batched: the 63 numbers ACE is made
of).  No device code: tests/test_em_ref_cpu.py proves the conditions below with a float64 stand-in,
tests/test_gpu_evalmetrics_matrix.py holds the device to them.

Reference.  evaluation/metrics/ace.py:19-34 and :44-82 restated in np.longdouble (64-bit significand): F = -unc, the map
widened from its stored dtype to float64 first; rater-voxels with ref == ignore_value dropped; T = t_pos where
ref == pred, else t_neg; z = A F + B; P = 1 / (1 + exp(z)), loss = -(T log P + (1 - T) log(1 - P)) and w = P (1 - P) in the
overflow-free form (e = exp(-|z|); 1 - P is formed as e / (1 + e) or 1 / (1 + e), never by subtraction).  An element is a
(rater, voxel) pair; its terms depend on the voxel and on whether that rater is correct there, nothing else, and are
linear in T.  So the terms are kept PER VOXEL (platt_terms: once for T = t_pos and once for T = t_neg), with the number
of correct and of wrong valid raters of the voxel (Case.n_c, Case.n_w) as multiplicities: the sums over elements are sums
over voxels of n_c * term(t_pos) + n_w * term(t_neg).

Bound of Platt sum k.  With u = 2^-53, a_i = |A F_i| + |B| and E_i = (2 L + 2 a_i + 4) u (operations counted in
em_platt_body; L: error of the device exp / log1p in ulp),
    tol_k = 4 sum_i E_i M_ki + D u sum_i M_ki,      D = ceil(R nvox / 131072) + 6 + 4 + 512
(D: the longest chain of additions of the documented association: a thread's elements, the shuffle tree, the four waves,
the 512 rows).  Majorants M: loss a_i + ln 2; dA (T_i + P_i) |F_i|; dB T_i + P_i; AA P_i F_i^2; AB P_i |F_i|; BB P_i.  The
Hessian majorants hold P, not w: the device forms 1 - P by subtraction, with an absolute error of u where P is near 1.
Bound of bin_sums[k]: 4 sum_{i in bin k} E_i p_i + D u sum_{i in bin k} p_i.

Guard band.  The bin a voxel falls in must not depend on the libm, so every voxel of the matrix keeps
|p_i - edge_j| > 4 E_i p_i for the interior edges j = 1..19 (edges 0 and 20 cannot be crossed: 0 <= p <= 1 < 1 + 1e-8).
That is a condition on the seeds, asserted for every voxel in tests/test_em_ref_cpu.py; nothing is filtered out.
"""
import functools
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "tests/em_ref.py needs a long double with a 64-bit significand"

U = 2.0 ** -53
L_ULP = 2                                 # error of the device exp / log1p in ulp (measured: 0.85 and 1.0)
GRID = 512 * 256                          # threads of every reduction of evalmetrics.hip
EDGES = np.linspace(0.0, 1.0 + 1e-8, 21)  # calib_stats' bins (ace.py:67)
SUM_NAMES = ("valid", "correct", "loss", "dA", "dB", "AA", "AB", "BB")

RATERS = (1, 3, 4)
SIZES = (1, 255, 257, 131072, 131073, 300001)    # 257, 131073: the rater boundary falls inside a wave
DTYPES = (np.float32, np.float64)
IGNORES = (None, 2)
PARAMS = ((0.0, 0.0), (-3.5, 1.25), (2.0, -1.0), (40.0, -7.0), (-900.0, 30.0), (1e-3, -745.0))
_SEED = 4391


@functools.lru_cache(maxsize=None)
def unc_map(nvox, dtype):
    """uniform in [0, 0.7), a tenth of the voxels scaled up to [0, 5); one map per (size, dtype), read-only"""
    rng = np.random.default_rng([_SEED, nvox, np.dtype(dtype).itemsize])
    u = rng.random(nvox) * 0.7
    u = np.where(rng.random(nvox) < 0.1, u * (5.0 / 0.7), u).astype(dtype)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def labels(R, nvox):
    """(ref [R][nvox], pred [nvox]) int32, labels 0..2 (2 is the ignored one), a rater agreeing with the prediction on
    seven voxels of ten; read-only"""
    rng = np.random.default_rng([_SEED + 1, R, nvox])
    if nvox == 1:                         # one voxel: the first rater valid and correct, the ignored label among the others
        pred, ref = np.array([1], dtype=np.int32), np.array([1, 2, 0, 1][:R], dtype=np.int32)[:, None]
    else:
        pred = rng.integers(0, 3, nvox).astype(np.int32)
        ref = np.where(rng.random((R, nvox)) < 0.7, pred[None], rng.integers(0, 3, (R, nvox))).astype(np.int32)
    ref.setflags(write=False)
    pred.setflags(write=False)
    return ref, pred


def rater_counts(ref, pred, ignore):
    """per voxel: the number of valid raters that agree with the prediction, and of valid raters that do not"""
    valid = np.ones(ref.shape, dtype=bool) if ignore is None else ref != ignore
    correct = valid & (ref == pred[None])
    return correct.sum(0), (valid & ~correct).sum(0)


def platt_targets(n_valid, n_correct):
    """Platt's regularised targets for the counts of an image (sklearn.calibration._sigmoid_calibration)"""
    return (n_correct + 1.0) / (n_correct + 2.0), 1.0 / (n_valid - n_correct + 2.0)


class Case:
    """one item of the matrix: inputs, parameters, and the exact counts"""

    def __init__(self, ref, pred, unc, ignore, A, B, t_pos=None, t_neg=None, key=None):
        self.ref, self.pred, self.unc, self.ignore, self.A, self.B, self.key = ref, pred, unc, ignore, float(A), float(B), key
        self.R, self.nvox = ref.shape
        self.n_c, self.n_w = rater_counts(ref, pred, ignore)
        self.n_valid, self.n_correct = int(self.n_c.sum() + self.n_w.sum()), int(self.n_c.sum())
        tp, tn = platt_targets(self.n_valid, self.n_correct)
        self.t_pos, self.t_neg = (tp if t_pos is None else t_pos), (tn if t_neg is None else t_neg)

    def __repr__(self):
        return (f"Case(R={self.R}, nvox={self.nvox}, {np.dtype(self.unc.dtype).name}, ignore={self.ignore}, "
                f"A={self.A}, B={self.B})")


def matrix(ignores=IGNORES, params=PARAMS, raters=RATERS, sizes=SIZES, dtypes=DTYPES):
    return [Case(*labels(R, n), unc_map(n, dt), ign, A, B, key=(n, dt, A, B))
            for ign in ignores for R in raters for n in sizes for dt in dtypes for A, B in params]


def chain_length(n_elements):
    """D: the longest chain of additions behind one sum of n_elements in the documented association"""
    return math.ceil(n_elements / GRID) + 6 + 4 + 512


def voxel_terms(unc, A, B):
    """what every element of a voxel shares.  In long double: F, z split by its sign into zp + zn, P, P F, log1p(e),
    w = P (1 - P) with 1 - P formed without subtraction, w F, w F^2.  In float64, for the bounds: |F|, P, a = |A F| + |B|,
    the error unit E.  The bin of P and the voxels of every bin."""
    F = -np.asarray(unc).astype(np.float64).astype(LD)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        z = LD(A) * F + LD(B)
        e = np.exp(-np.abs(z))
        P = np.where(z >= 0, e / (1 + e), 1 / (1 + e))
        w = P * np.where(z >= 0, 1 / (1 + e), e / (1 + e))
        f64 = np.abs(F.astype(np.float64))
        a = abs(A) * f64 + abs(B)
        wF = w * F
        vt = dict(F=F, z=z, zp=np.where(z >= 0, z, 0), zn=np.where(z < 0, z, 0), P=P, PF=P * F, l1p=np.log1p(e), w=w, wF=wF,
                  wFF=wF * F, f64=f64, p64=P.astype(np.float64), a=a, E=(2 * L_ULP + 2 * a + 4) * U)
    binid = np.searchsorted(EDGES.astype(LD), P, side="right") - 1      # np.digitize(P, bins) - 1; NaN sorts last: bin 20
    vt.update(bin=binid, members=[np.flatnonzero(binid == k) for k in range(len(EDGES))])
    return vt


@functools.lru_cache(maxsize=None)
def _matrix_voxel_terms(nvox, dtype, A, B):
    return voxel_terms(unc_map(nvox, dtype), A, B)


def terms_of(case):
    return _matrix_voxel_terms(*case.key) if case.key is not None else voxel_terms(case.unc, case.A, case.B)


def guard_band_margin(vt):
    """min over the voxels and the interior edges of |p - edge_j| - 4 E p: positive when no voxel can change its bin"""
    p = vt["p64"]
    gap = np.abs(p[:, None] - EDGES[None, 1:20]).min(1)
    return float((gap - 4 * vt["E"] * p).min())


def platt_terms(case):
    """{name: (per-voxel term at t_pos, at t_neg)} of sums[2..7] in long double; an element's term is its voxel's, at t_pos
    where its rater is correct and at t_neg where not, so the sums weight them with case.n_c and case.n_w"""
    vt = terms_of(case)
    with np.errstate(invalid="ignore"):
        both = lambda f: (f(LD(case.t_pos)), f(LD(case.t_neg)))
        return {"loss": both(lambda T: T * vt["zp"] + (T - 1) * vt["zn"] + vt["l1p"]),   # T z | (T - 1) z, + log1p(exp(-|z|))
                "dA": both(lambda T: (T - vt["P"]) * vt["F"]), "dB": both(lambda T: T - vt["P"]),
                "AA": (vt["wFF"],) * 2, "AB": (vt["wF"],) * 2, "BB": (vt["w"],) * 2}


def platt_majorants(case):
    """{name: (per-voxel majorant at t_pos, at t_neg)} in float64"""
    vt = terms_of(case)
    p, f, loss = vt["p64"], vt["f64"], vt["a"] + math.log(2.0)
    with np.errstate(invalid="ignore"):
        return {"loss": (loss, loss), "dA": ((case.t_pos + p) * f, (case.t_neg + p) * f), "dB": (case.t_pos + p, case.t_neg + p),
                "AA": (p * f * f,) * 2, "AB": (p * f,) * 2, "BB": (p,) * 2}


def _weighted_sums(n, arrays):
    """[sum_i n_i x_i] for every long double x of `arrays` and small integer weights n: numpy's pairwise sum over the
    voxels of each weight, times the weight"""
    groups = [(LD(j), np.flatnonzero(n == j)) for j in range(1, int(n.max()) + 1)]
    return [sum((j * x[idx].sum() for j, idx in groups), LD(0)) for x in arrays]


def platt_reference(case):
    """(sums [8] long double, tol [8] float64); tol[0] = tol[1] = 0: the counts are exact.  Every term is linear in T, so
    the sums are formed from sums over the voxels of n_c X and n_w X for the shared X of voxel_terms, each multiplied out
    in long double and added with numpy's pairwise sum: off by less than 2^-58 of the sum of the magnitudes, a 1e-4 of
    the smallest bound.  platt_terms(case) gives the same numbers term by term."""
    vt = terms_of(case)
    D = chain_length(case.R * case.nvox)
    tp, tn = LD(case.t_pos), LD(case.t_neg)
    with np.errstate(invalid="ignore"):
        keys = ("zp", "zn", "l1p", "F", "PF", "P")
        c = dict(zip(keys, _weighted_sums(case.n_c, [vt[k] for k in keys])))
        w = dict(zip(keys, _weighted_sums(case.n_w, [vt[k] for k in keys])))
        hess = _weighted_sums(case.n_c + case.n_w, [vt["wFF"], vt["wF"], vt["w"]])
        sums = [LD(case.n_valid), LD(case.n_correct),
                tp * c["zp"] + (tp - 1) * c["zn"] + c["l1p"] + tn * w["zp"] + (tn - 1) * w["zn"] + w["l1p"],
                tp * c["F"] - c["PF"] + tn * w["F"] - w["PF"],
                tp * LD(case.n_correct) - c["P"] + tn * LD(case.n_valid - case.n_correct) - w["P"],
                *hess]
        tol = [0.0, 0.0]
        for name, (m_pos, m_neg) in platt_majorants(case).items():
            m = case.n_c * m_pos + case.n_w * m_neg
            tol.append(float(4.0 * np.dot(vt["E"], m) + D * U * m.sum()))
    return np.array(sums, dtype=LD), np.array(tol)


def bins_reference(case):
    """(bin_sums [21] long double, bin_true [21], bin_total [21] float64 (exact counts), tol [21] float64, bin [nvox])"""
    vt = terms_of(case)
    p, binid = vt["P"], vt["bin"]
    n = case.n_c + case.n_w
    nb = len(EDGES)
    bin_true = np.bincount(binid, weights=case.n_c, minlength=nb)
    bin_total = np.bincount(binid, weights=n, minlength=nb)
    np_ld = n.astype(LD) * p
    bin_sums = np.array([np_ld[m].sum() for m in vt["members"]], dtype=LD)
    D = chain_length(case.R * case.nvox)
    with np.errstate(invalid="ignore"):
        p64 = n * vt["p64"]
        tol = 4.0 * np.bincount(binid, weights=vt["E"] * p64, minlength=nb) + D * U * np.bincount(binid, weights=p64, minlength=nb)
    return bin_sums, bin_true, bin_total, tol, binid


def ratio(got, want, tol):
    """|got - want| / tol per number (0 where both differences and bounds are 0, inf where only the bound is)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(np.asarray(got).astype(LD) - want).astype(np.float64)
        return np.where(err == 0, 0.0, err / tol)


# ------------------------------------------------------------------------------------------------ the exact cases
def lattice_cases():
    """A = B = 0, t_pos = 0.75, t_neg = 0.25, unc = m / 1024 with m < 1024: z = 0, exp(0) = 1, P = 0.5 and w = 0.25
    exactly, so sums[3..7] are sums of multiples of 2^-22 and exact in any association"""
    cases = []
    for ign in IGNORES:
        for R in RATERS:
            for k, n in enumerate((257, 131073)):
                rng = np.random.default_rng([_SEED + 2, R, n])
                unc = (rng.integers(0, 1024, n) / 1024.0).astype(DTYPES[(R + k) % 2])
                cases.append(Case(*labels(R, n), unc, ign, 0.0, 0.0, 0.75, 0.25))
    return cases


SPECIALS = {"half": (0.5, 2.0, 1.0, 9), "one": (400.0, 2.0, 1.0, 19), "zero": (-400.0, 2.0, 1.0, 0),
            "inf_neg_a": (np.inf, -2.0, 1.0, 0), "inf_pos_a": (np.inf, 2.0, 1.0, 19), "nan": (np.nan, 2.0, 1.0, 20)}


def special_cases():
    """{name: Case} of 67 voxels (R = 3) that all hold one special map value -- p = 0.5 (A F + B = 0: bin 9, edge 10 is
    0.500000005), p = 1 (exp underflows to 0: bin 19), p = 0 (exp overflows: bin 0), +inf under A < 0 (bin 0) and A > 0
    (bin 19), NaN (bin 20, as np.digitize) -- and "mixed": all of them among 300 ordinary voxels at (A, B) = (2, 1).
    exp(0), exp(-large) and exp(large) are exact on any libm, so the bins and their sums are."""
    ref, pred = labels(3, 67)
    cases = {name: Case(ref, pred, np.full(67, v, dtype=np.float64), 2, A, B) for name, (v, A, B, _) in SPECIALS.items()}
    rng = np.random.default_rng(_SEED + 3)
    unc = rng.random(330) * 0.7
    unc[::11] = np.resize([0.5, 400.0, -400.0, np.inf, -np.inf, np.nan], 30)
    cases["mixed"] = Case(*labels(3, 330), unc, 2, 2.0, 1.0)
    return cases
