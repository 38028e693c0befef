"""GPU: the sampling kernels of accumulate.hip (vx_aleatoric_sample, vx_ssn_sample, vx_ssn2d_lowres, vx_ssn2d_add_diag
and their generator vx_gauss), vx_pack_input_cl8 and vx_colorize_u8 through the C ABI, against the restatement in
tests/sample_ref.py: injected and generated normals, batch > 1 with distinct normals in every (draw, image) cell, pitches
wider than the channel count, second trips of the grid-stride loops, every refusal, and the two drivers whose batch-1
tests could not see a transposed stride.

Every output lives in a buffer with GUARD sentinel elements before and after it; they must come back untouched.

Tolerances (the convention of tests/test_gpu_reduce.py).  For each group -- aleatoric, ssn, comb, expm, add_diag,
generated -- the bound comes from the REFERENCE: GAP_* is the largest difference between the restatement in float64
and with the inputs and every intermediate rounded to float32, over this module's own inputs (reference_matrix();
tests/test_sample_ref_cpu.py recomputes them).  CONTRACT = min(1e-4, 4 x GAP): 1e-4 is the project's logit contract,
the factor 4 covers the device's expf / logf / sqrtf / cospif forms and fmaf contraction against numpy's.  Deviations
are absolute; the cases whose magnitudes leave the logit range (s up to 20: sigma up to 2.2e4; log_cov_diag = 40: sd
4.9e8) are measured relative to max(1, |reference|), in the gap and on the device alike (`rel` beside those cases).
OBS is the largest device deviation measured on an MI355X over this module, REG = min(CONTRACT, 5 x OBS) a regression
bound asserted beside each contract bound.  The index kernels (pack, colorize) and the refusals are exact.
"""

import numpy as np
import pytest
import torch

from tests import sample_ref as sr
from tests.formula import formula_tensor
from values_amd import _lib

pytestmark = pytest.mark.gpu

# ---- bounds (see the module docstring) ----------------------------------------------------------------------------
GAP = {"aleatoric": 1.73e-6, "ssn": 1.17e-6, "comb": 5.24e-7, "expm": 1.91e-6, "add_diag": 8.75e-7, "generated": 3.41e-7}
OBS = {"aleatoric": 1.91e-6, "ssn": 1.17e-6, "comb": 5.24e-7, "expm": 3.13e-6, "add_diag": 8.75e-7, "generated": 3.82e-7}
CONTRACT = {k: min(1e-4, 4 * g) for k, g in GAP.items()}
REG = {k: min(CONTRACT[k], 5 * OBS[k]) for k in CONTRACT}             # (the contract is the tighter one in every group)

NVOX = 1029                 # odd, five blocks of 256, a ragged last one
GUARD = 64
SENT_F, SENT_U8 = -77.0, 201
PAD = 1e30                  # what the channels between C (or R*C) and the pitch hold
SEEDS = (0, 5, 0xFFFFFFFF)
F32 = np.float32


# ---- inputs (numpy only: tests/test_sample_ref_cpu.py measures the float32 gap of the restatement on the same arrays) --
def _ft(shape, tag, scale):
    return formula_tensor(shape, tag, scale=scale).astype(F32)


ALEATORIC_CASES = [(C_, T, False) for C_ in (1, 2, 3) for T in (1, 5)] + [(2, 2, True)]     # (C, T, s spans [-20, 20]: rel)


def aleatoric_case(C_, T, wide=False, N=3, nvox=NVOX):
    """-> mu_s [N][2C][nvox], eps [N][T][C][nvox]; samples reach |4 + e * 1.7| ~ 8.6"""
    tag = 900 + 10 * C_ + T + (50 if wide else 0)
    mu, s = _ft((N, C_, nvox), tag, 4.0), _ft((N, C_, nvox), tag + 100, 20.0 if wide else 2.0)
    return np.concatenate([mu, s], axis=1), _ft((N, T, C_, nvox), tag + 200, 1.7)


SSN_CASES = [(3, 2, 2, 10, None), (2, 3, 3, 1, None), (3, 2, 2, 0, None), (1, 4, 1, 2, None),
             (3, 2, 2, 10, "neginf"), (2, 3, 3, 1, "p40")]                                    # (N, S, C, R, special); p40: rel


def ssn_case(N, S, C_, R, special=None, nvox=NVOX):
    """-> head [N][(2+R)C][nvox], eps_w [S][N][R], eps_d [S][N][C][nvox]: a different value in every (s, n) cell.
    special "neginf": log_cov_diag = -inf on the last class plane (sd = sqrt(epsilon)); "p40": +40 on class 0"""
    tag = 1300 + 100 * N + 10 * S + R + {None: 0, "neginf": 3000, "p40": 6000}[special]
    mean, logd = _ft((N, C_, nvox), tag, 4.0), _ft((N, C_, nvox), tag + 1, 2.0)
    fac = _ft((N, R * C_, nvox), tag + 2, 1.5 / max(R, 1) ** 0.5)
    if special == "neginf":
        logd[:, C_ - 1] = -np.inf
    if special == "p40":
        logd[:, 0] = 40.0
    return np.concatenate([mean, logd, fac], axis=1), _ft((S, N, R), tag + 3, 1.7), _ft((S, N, C_, nvox), tag + 4, 1.7)


SSN2D_CASES = [(2, 23 * 7, 3, 4, 10, 4, 40), (3, 161, 2, 19, 10, 32, 192), (1, 161, 1, 19, 0, 32, 0)]  # (B, pix, S, C, R, pm, pf)


def lowres_case(B, pix, S, C_, R, pm, pf):
    """-> mean [B*pix][pm], fac [B*pix][pf] (None for R = 0), eps_w [S][B][R]; channels past C / R*C hold PAD"""
    tag = 1700 + 10 * C_ + R + B
    mean = np.full((B * pix, pm), PAD, dtype=F32)
    mean[:, :C_] = _ft((B * pix, C_), tag, 4.0)
    fac = None
    if R:
        fac = np.full((B * pix, pf), PAD, dtype=F32)
        fac[:, :R * C_] = _ft((B * pix, R * C_), tag + 1, 1.5 / R ** 0.5)
    return mean, fac, _ft((S, B, R), tag + 2, 1.7)


def add_diag_case(B, S, per):
    """-> out [B][S][per] (non-zero), diag [B][per] in [0, 7), eps_d [S][B][per]"""
    tag = 1900 + 10 * B + S
    return _ft((B, S, per), tag, 4.0), np.abs(_ft((B, per), tag + 1, 7.0)), _ft((S, B, per), tag + 2, 1.7)


def unit_factor_head(N, Cc, nvox):
    """vx_ssn_sample head with R = C: mean 0, log_cov_diag -inf, factor plane k = 1 on class k, 0 elsewhere; with
    epsilon = 0 the call returns eps_w[s][n][c] at every voxel of class c"""
    head = np.zeros((N, (2 + Cc) * Cc, nvox), dtype=F32)
    head[:, Cc:2 * Cc] = -np.inf
    for k in range(Cc):
        head[:, 2 * Cc + k * Cc + k] = 1.0
    return head


N_3D = (1 << 21) + 1029            # C = 2: one element more than 16384 x 256 threads cover, and a ragged rest
PER_2D = (1 << 22) + 517
PIX_BIG = (1 << 16) + 33           # B = 2, C = 19: past 8192 x 256
GEN = dict(N=3, T=4, C=2, S=2, R=4, pix=161)       # shapes of the generated-normals checks


def generated_reference(seed, dtype=np.float64):
    """what the three generated-only calls must return for `seed` -> dict of arrays"""
    g = GEN
    zeros = np.zeros((g["N"], 2 * g["C"], NVOX), dtype=F32)
    per = g["C"] * NVOX
    comb, _ = sr.ssn2d_lowres(np.zeros((g["N"] * g["pix"], g["R"]), F32), g["R"], _unit_fac2d(), g["R"] * g["R"], None, seed,
                              g["N"], g["pix"], g["S"], g["R"], g["R"], dtype=dtype)
    return {"aleatoric": sr.aleatoric(zeros, None, seed, g["N"], g["T"], g["C"], NVOX, dtype=dtype)[0],
            "add_diag": sr.ssn2d_add_diag(np.zeros((g["N"], g["S"], per), F32), np.ones((g["N"], per), F32), None, seed,
                                          g["S"], g["N"], per, 0.0, dtype=dtype),
            "lowres": comb}


def _unit_fac2d():
    """vx_ssn2d_lowres factor with C = R: channel k*C + c is 1 where c == k, so comb[s][pix][c] = eps_w[s][b][c]"""
    R, P = GEN["R"], GEN["N"] * GEN["pix"]
    return np.broadcast_to(np.eye(R, dtype=F32).reshape(1, R * R), (P, R * R)).copy()


def big_case(which):
    """inputs of the second-trip cases -> (args of the restatement, kwargs)"""
    if which in ("aleatoric_injected", "aleatoric_generated"):
        mu_s, eps = aleatoric_case(2, 1, N=1, nvox=N_3D)
        return (mu_s, eps if which.endswith("injected") else None), dict(seed=11, N=1, T=1, C=2, nvox=N_3D)
    if which == "ssn":
        head, ew, ed = ssn_case(1, 1, 2, 1, nvox=N_3D)
        return (head, ew, ed), dict(seed=0, N=1, S=1, C=2, R=1, nvox=N_3D, epsilon=1e-5)
    if which == "add_diag":
        out, diag, ed = add_diag_case(1, 1, PER_2D)
        return (out, diag, ed), dict(seed=0, S=1, B=1, per=PER_2D, epsilon=1e-5)
    mean, fac, ew = lowres_case(2, PIX_BIG, 1, 19, 1, 32, 32)
    return (mean, 32, fac, 32, ew), dict(seed=0, B=2, pix=PIX_BIG, S=1, C=19, R=1)


BIG = {"aleatoric_injected": ("aleatoric", sr.aleatoric), "aleatoric_generated": ("aleatoric", sr.aleatoric),
       "ssn": ("ssn", sr.ssn), "add_diag": ("add_diag", sr.ssn2d_add_diag), "lowres": ("comb", sr.ssn2d_lowres)}
MIXED = (("eps_w", 77), ("eps_d", 78))          # (what is injected, seed of the generated other half)


def reference_matrix():
    """every float comparison of this module as (group, name, rel, ref): ref(dtype) -> tuple of arrays.  The GPU tests
    compare the device with ref(np.float64); the CPU test measures max |ref(float64) - ref(float32)| per group."""
    for C_, T, wide in ALEATORIC_CASES:
        mu_s, eps = aleatoric_case(C_, T, wide)
        yield ("aleatoric", f"aleatoric C{C_} T{T} wide={wide}", wide,
               lambda dtype, a=(mu_s, eps, 0, 3, T, C_, NVOX): sr.aleatoric(*a, dtype=dtype))
    for N, S, C_, R, special in SSN_CASES:
        head, ew, ed = ssn_case(N, S, C_, R, special)
        yield ("ssn", f"ssn {N} {S} {C_} {R} {special}", special == "p40",
               lambda dtype, a=(head, ew if R else None, ed, 0, N, S, C_, R, NVOX, 1e-5): (sr.ssn(*a, dtype=dtype),))
    head, ew, ed = ssn_case(3, 2, 2, 10)
    for inj, seed in MIXED:
        yield ("ssn", f"ssn mixed {inj}", False,
               lambda dtype, a=(head, ew if inj == "eps_w" else None, ed if inj == "eps_d" else None, seed, 3, 2, 2, 10, NVOX,
                                1e-5): (sr.ssn(*a, dtype=dtype),))
    for B, pix, S, C_, R, pm, pf in SSN2D_CASES:
        mean, fac, ew = lowres_case(B, pix, S, C_, R, pm, pf)
        a = (mean, pm, fac, pf, ew if R else None, 0, B, pix, S, C_, R)
        yield ("comb", f"comb {B} {C_} {R}", False, lambda dtype, a=a: (sr.ssn2d_lowres(*a, dtype=dtype)[0],))
        yield ("expm", f"expm {B} {C_} {R}", False, lambda dtype, a=a: (sr.ssn2d_lowres(*a, dtype=dtype)[1],))
        out, diag, ed = add_diag_case(B, S, C_ * NVOX)
        yield ("add_diag", f"add_diag {B} {S} {C_}", False,
               lambda dtype, a=(out, diag, ed, 0, S, B, C_ * NVOX, 1e-5): (sr.ssn2d_add_diag(*a, dtype=dtype),))
    for seed in SEEDS:
        yield ("generated", f"generated seed {seed}", False,
               lambda dtype, seed=seed: tuple(generated_reference(seed, dtype).values()))
    yield ("generated", "generated eps_w", False,
           lambda dtype: (sr._eps_w(None, 21, 2, 3, 3, dtype),))
    for which, (group, fn) in BIG.items():
        args, kw = big_case(which)

        def ref(dtype, fn=fn, args=args, kw=kw, pick=None):
            r = fn(*args, dtype=dtype, **kw)
            r = r if isinstance(r, tuple) else (r,)
            return r if pick is None else (r[pick],)
        if which == "lowres":
            yield ("comb", "second trip lowres comb", False, lambda dtype, ref=ref: ref(dtype, pick=0))
            yield ("expm", "second trip lowres expm", False, lambda dtype, ref=ref: ref(dtype, pick=1))
        else:
            yield (group, f"second trip {which}", False, ref)


def deviation(got, want, rel=False):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
    d = np.where(got == want, 0.0, d)          # (equal infinities)
    if rel:
        d = d / np.maximum(1.0, np.abs(want))
    return float(d.max()) if d.size else 0.0


# ---- device helpers --------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


class _Out:
    """an output array inside a buffer of its own with GUARD sentinel elements on either side"""

    def __init__(self, shape, dtype=torch.float32, data=None):
        self.shape = tuple(int(s) for s in shape)
        self.n = int(np.prod(self.shape))
        self.sent = SENT_U8 if dtype == torch.uint8 else SENT_F
        self.full = torch.full((self.n + 2 * GUARD,), self.sent, dtype=dtype, device="cuda")
        self.view = self.full[GUARD:GUARD + self.n]
        if data is not None:
            self.view.copy_(_dev(data).reshape(-1))

    @property
    def p(self):
        return _lib.ptr(self.view)

    def get(self, written=True):
        """the array, after checking the guards (and that no element kept the sentinel)"""
        torch.cuda.synchronize()
        assert bool((self.full[:GUARD] == self.sent).all()), "written before the array"
        assert bool((self.full[GUARD + self.n:] == self.sent).all()), "written past the array"
        if written and self.full.dtype != torch.uint8:
            assert not bool((self.view == self.sent).any()), "elements left unwritten"
        return _np(self.view).reshape(self.shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.full == self.sent).all())


def _close(got, want, group, name, rel=False):
    """contract and regression bound of `group`; on a long last axis the first and the last 1024 elements first, so that
    a failure in a loop's tail is named as such"""
    assert not np.isnan(got).any(), f"{name}: NaN"
    if got.shape[-1] > 4096:
        for part, sl in (("head", slice(0, 1024)), ("tail", slice(-1024, None))):
            e = deviation(got[..., sl], want[..., sl], rel)
            assert e <= CONTRACT[group], f"{name} [{part}]: {e:.3e} > {CONTRACT[group]:.1e}"
    err = deviation(got, want, rel)
    print(f"deviation {group} {name} {err:.3e}")
    assert err <= CONTRACT[group], f"{name}: {err:.3e} > contract {CONTRACT[group]:.1e}"
    assert err <= REG[group], f"{name}: {err:.3e} > regression bound {REG[group]:.1e}"


def _aleatoric(mu_s, eps, seed, N, T, Cc, nvox, want_sigma=True):
    out = _Out((N, T, Cc, nvox))
    sig = _Out((N, Cc, nvox)) if want_sigma else None
    hold = (_dev(mu_s), _dev(eps))
    _lib.check(_lib.load().vx_aleatoric_sample(_lib.ptr(hold[0]), _lib.ptr(hold[1]), seed, N, T, Cc, nvox, out.p,
                                               sig.p if sig else None, _lib.stream_ptr()), "vx_aleatoric_sample")
    return out.get(), (sig.get() if sig else None)


def _ssn(head, eps_w, eps_d, seed, N, S, Cc, R, nvox, epsilon):
    out = _Out((N, S, Cc, nvox))
    hold = (_dev(head), _dev(eps_w), _dev(eps_d))
    _lib.check(_lib.load().vx_ssn_sample(_lib.ptr(hold[0]), _lib.ptr(hold[1]), _lib.ptr(hold[2]), seed, N, S, Cc, R, nvox,
                                         epsilon, out.p, _lib.stream_ptr()), "vx_ssn_sample")
    return out.get()


def _lowres(mean, pm, fac, pf, eps_w, seed, B, pix, S, Cc, R, want_expm=True):
    comb = _Out((S, B * pix, Cc))
    expm = _Out((B * pix, Cc)) if want_expm else None
    hold = (_dev(mean), _dev(fac), _dev(eps_w))
    _lib.check(_lib.load().vx_ssn2d_lowres(_lib.ptr(hold[0]), pm, _lib.ptr(hold[1]), pf, _lib.ptr(hold[2]), seed, B, pix, S, Cc,
                                           R, comb.p, expm.p if expm else None, _lib.stream_ptr()), "vx_ssn2d_lowres")
    return comb.get(), (expm.get() if expm else None)


def _add_diag(out0, diag, eps_d, seed, S, B, per, epsilon):
    out = _Out((B, S, per), data=out0)
    hold = (_dev(diag), _dev(eps_d))
    _lib.check(_lib.load().vx_ssn2d_add_diag(out.p, _lib.ptr(hold[0]), _lib.ptr(hold[1]), seed, S, B, per, epsilon,
                                             _lib.stream_ptr()), "vx_ssn2d_add_diag")
    return out.get(written=False)


# ---- a. vx_aleatoric_sample, injected eps -------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,T,wide", ALEATORIC_CASES)
def test_aleatoric_injected_against_float64(Cc, T, wide):
    """wide: s spans [-20, 20], sigma up to e^10 -- deviations relative to max(1, |reference|)"""
    N = 3
    mu_s, eps = aleatoric_case(Cc, T, wide)
    want, want_sigma = sr.aleatoric(mu_s, eps, 0, N, T, Cc, NVOX)
    got, sigma = _aleatoric(mu_s, eps, 0, N, T, Cc, NVOX)
    _close(got, want, "aleatoric", f"C{Cc} T{T} out", rel=wide)
    _close(sigma, want_sigma, "aleatoric", f"C{Cc} T{T} sigma", rel=wide)
    alone, _ = _aleatoric(mu_s, eps, 0, N, T, Cc, NVOX, want_sigma=False)
    assert np.array_equal(alone, got), "out depends on whether sigma is requested"
    if wide:
        assert np.abs(mu_s[:, Cc:]).max() > 19.9 and np.abs(want).max() > 1e4
    else:
        assert 7.0 < np.abs(want).max() < 12.0


# ---- b. vx_ssn_sample, injected -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,Cc,R,special", SSN_CASES)
def test_ssn_injected_against_float64(N, S, Cc, R, special):
    """p40: log_cov_diag = 40 on a class plane, sd = 4.9e8 -- deviations relative to max(1, |reference|)"""
    head, ew, ed = ssn_case(N, S, Cc, R, special)
    if S > 1 and N > 1 and R:
        assert len(np.unique(ew)) == ew.size                      # no two (s, n, k) cells share a value
    assert not np.array_equal(ed[0, -1], ed[-1, 0]) or S * N == 1
    want = sr.ssn(head, ew if R else None, ed, 0, N, S, Cc, R, NVOX, 1e-5)
    got = _ssn(head, ew if R else None, ed, 0, N, S, Cc, R, NVOX, 1e-5)
    assert np.isfinite(got).all()
    _close(got, want, "ssn", f"ssn N{N} S{S} C{Cc} R{R} {special}", rel=special == "p40")
    if special == "neginf":        # sd = sqrt(epsilon) there: eps_d moves the sample by 0.00316 * eps_d
        flat = sr.ssn(head, ew, np.zeros_like(ed), 0, N, S, Cc, R, NVOX, 1e-5)
        assert 1e-3 < np.abs(want - flat)[:, :, Cc - 1].max() < 0.00317 * 1.7
    if special == "p40":
        assert np.abs(want[:, :, 0]).max() > 1e8


# ---- c. mixed injection, and the low-rank vector itself --------------------------------------------------------------------
@pytest.mark.parametrize("inject,seed", MIXED)
def test_ssn_one_half_injected_the_other_generated(inject, seed):
    N, S, Cc, R = 3, 2, 2, 10
    head, ew, ed = ssn_case(N, S, Cc, R)
    ew, ed = (ew, None) if inject == "eps_w" else (None, ed)
    want = sr.ssn(head, ew, ed, seed, N, S, Cc, R, NVOX, 1e-5)
    _close(_ssn(head, ew, ed, seed, N, S, Cc, R, NVOX, 1e-5), want, "ssn", f"ssn mixed, {inject} injected")


def test_ssn_generated_low_rank_vector_is_one_value_per_draw_and_image():
    """mean 0, log_cov_diag -inf, epsilon 0, factor plane k = 1 on class k: out[n][s][k][v] is eps_w[s][n][k] itself --
    the same at all voxels of a draw, different between draws, images and ranks, and gauss(seed ^ 0x5bd1e995, k, n*S + s)"""
    N, S, R, seed = 3, 2, 3, 21
    got = _ssn(unit_factor_head(N, R, NVOX), None, None, seed, N, S, R, R, NVOX, 0.0)       # (N, S, R, nvox)
    assert (got == got[..., :1]).all(), "the low-rank vector differs between the voxels of a draw"
    cell = got[..., 0]
    assert len(np.unique(cell)) == N * S * R
    want = sr._eps_w(None, seed, S, N, R, np.float64).transpose(1, 0, 2)                         # [s][n][k] -> [n][s][k]
    np.testing.assert_array_equal(want, sr.gauss(seed ^ 0x5bd1e995, np.arange(R)[None, None, :],
                                                 (np.arange(N)[:, None] * S + np.arange(S)[None, :])[..., None]))
    _close(cell, want, "generated", "generated eps_w of vx_ssn_sample")


# ---- d. the generator on the device is the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_generated_normals_are_the_restatement(seed):
    """mu = 0, s = 0 (or diag = 1, out = 0; or a unit factor): the call returns the normals exactly, fmaf(1, e, 0).  One
    flipped hash bit moves a value by order 1, so this pins every constant of vx_gauss and the slot of every stream."""
    g = GEN
    N, T, Cc, S, R, pix = g["N"], g["T"], g["C"], g["S"], g["R"], g["pix"]
    want = generated_reference(seed)
    per = Cc * NVOX
    got, sigma = _aleatoric(np.zeros((N, 2 * Cc, NVOX), F32), None, seed, N, T, Cc, NVOX)
    assert (sigma == 1).all()
    _close(got, want["aleatoric"], "generated", f"aleatoric seed {seed}")
    got = _add_diag(np.zeros((N, S, per), F32), np.ones((N, per), F32), None, seed, S, N, per, 0.0)
    _close(got, want["add_diag"], "generated", f"add_diag seed {seed}")
    got, _ = _lowres(np.zeros((N * pix, R), F32), R, _unit_fac2d(), R * R, None, seed, N, pix, S, R, R)
    _close(got, want["lowres"], "generated", f"lowres seed {seed}")
    assert np.abs(want["aleatoric"]).max() > 3.5 and len(np.unique(want["lowres"])) == N * S * R


# ---- e. vx_ssn2d_lowres / vx_ssn2d_add_diag, injected ------------------------------------------------------------------------
@pytest.mark.parametrize("B,pix,S,Cc,R,pm,pf", SSN2D_CASES)
def test_ssn2d_injected_against_float64(B, pix, S, Cc, R, pm, pf):
    mean, fac, ew = lowres_case(B, pix, S, Cc, R, pm, pf)
    ew = ew if R else None
    want_comb, want_expm = sr.ssn2d_lowres(mean, pm, fac, pf, ew, 0, B, pix, S, Cc, R)
    comb, expm = _lowres(mean, pm, fac, pf, ew, 0, B, pix, S, Cc, R)
    assert np.abs(comb).max() < 1e3, "a padding channel leaked into comb"
    _close(comb, want_comb, "comb", f"comb B{B} C{Cc} R{R}")
    _close(expm, want_expm, "expm", f"expm B{B} C{Cc} R{R}")
    alone, _ = _lowres(mean, pm, fac, pf, ew, 0, B, pix, S, Cc, R, want_expm=False)
    assert np.array_equal(alone, comb), "comb depends on whether expm is requested"
    per = Cc * NVOX
    out0, diag, ed = add_diag_case(B, S, per)
    _close(_add_diag(out0, diag, ed, 0, S, B, per, 1e-5), sr.ssn2d_add_diag(out0, diag, ed, 0, S, B, per, 1e-5), "add_diag",
           f"add_diag B{B} S{S} per {per}")


# ---- f. second trips of the grid-stride loops ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(BIG))
def test_second_loop_trip(which):
    group, fn = BIG[which]
    args, kw = big_case(which)
    want = fn(*args, **kw)
    if which.startswith("aleatoric"):
        assert kw["N"] * kw["C"] * kw["nvox"] > 16384 * 256
        got, sigma = _aleatoric(*args, kw["seed"], 1, 1, 2, N_3D)
        _close(sigma, want[1], group, f"second trip {which} sigma")
        want = want[0]
    elif which == "ssn":
        got = _ssn(*args, 0, 1, 1, 2, 1, N_3D, 1e-5)
    elif which == "add_diag":
        assert PER_2D > 16384 * 256
        got = _add_diag(*args, 0, 1, 1, PER_2D, 1e-5)
    else:
        assert 2 * PIX_BIG * 19 > 8192 * 256
        got, expm = _lowres(*args, 0, 2, PIX_BIG, 1, 19, 1)
        _close(expm.reshape(-1), want[1].reshape(-1), "expm", f"second trip {which} expm")
        want = want[0]
    n = got.shape[0] if which == "lowres" else 1
    _close(got.reshape(n, -1), want.reshape(n, -1), group, f"second trip {which}")


# ---- g. refusals ----------------------------------------------------------------------------------------------------------
OK, E_NULL, E_SHAPE = 0, -1, -2


def test_refusals_return_before_any_launch():
    lib = _lib.load()
    st = _lib.stream_ptr()
    src = torch.zeros(4096, device="cuda")
    out = _Out((256,))
    s, o = _lib.ptr(src), out.p
    big = 1 << 31                       # C = 2: C * nvox = 2^32
    calls = {
        "aleatoric too large": (lib.vx_aleatoric_sample(s, None, 0, 1, 1, 2, big, o, None, st), E_SHAPE),
        "aleatoric N = 0": (lib.vx_aleatoric_sample(s, None, 0, 0, 1, 2, 16, o, None, st), E_SHAPE),
        "aleatoric T = 0": (lib.vx_aleatoric_sample(s, None, 0, 1, 0, 2, 16, o, None, st), E_SHAPE),
        "aleatoric null out": (lib.vx_aleatoric_sample(s, None, 0, 1, 1, 2, 16, None, None, st), E_NULL),
        "aleatoric null mu_s": (lib.vx_aleatoric_sample(None, None, 0, 1, 1, 2, 16, o, None, st), E_NULL),
        "aleatoric nvox = 0": (lib.vx_aleatoric_sample(s, None, 0, 1, 1, 2, 0, o, None, st), OK),
        "ssn too large": (lib.vx_ssn_sample(s, None, None, 0, 1, 1, 2, 1, big, 1e-5, o, st), E_SHAPE),
        "ssn N = 0": (lib.vx_ssn_sample(s, None, None, 0, 0, 1, 2, 1, 16, 1e-5, o, st), E_SHAPE),
        "ssn R < 0": (lib.vx_ssn_sample(s, None, None, 0, 1, 1, 2, -1, 16, 1e-5, o, st), E_SHAPE),
        "ssn null out": (lib.vx_ssn_sample(s, None, None, 0, 1, 1, 2, 1, 16, 1e-5, None, st), E_NULL),
        "ssn null head": (lib.vx_ssn_sample(None, None, None, 0, 1, 1, 2, 1, 16, 1e-5, o, st), E_NULL),
        "ssn nvox = 0": (lib.vx_ssn_sample(s, None, None, 0, 1, 1, 2, 1, 0, 1e-5, o, st), OK),
        "add_diag per = 2^32": (lib.vx_ssn2d_add_diag(o, s, None, 0, 1, 1, 1 << 32, 1e-5, st), E_SHAPE),
        "add_diag per = 0": (lib.vx_ssn2d_add_diag(o, s, None, 0, 1, 1, 0, 1e-5, st), E_SHAPE),
        "add_diag B = 0": (lib.vx_ssn2d_add_diag(o, s, None, 0, 1, 0, 16, 1e-5, st), E_SHAPE),
        "add_diag null out": (lib.vx_ssn2d_add_diag(None, s, None, 0, 1, 1, 16, 1e-5, st), E_NULL),
        "add_diag null diag": (lib.vx_ssn2d_add_diag(o, None, None, 0, 1, 1, 16, 1e-5, st), E_NULL),
        "lowres mean_pitch < C": (lib.vx_ssn2d_lowres(s, 3, s, 8, None, 0, 1, 4, 1, 4, 2, o, None, st), E_SHAPE),
        "lowres factor_pitch < R*C": (lib.vx_ssn2d_lowres(s, 4, s, 7, None, 0, 1, 4, 1, 4, 2, o, None, st), E_SHAPE),
        "lowres null factor": (lib.vx_ssn2d_lowres(s, 4, None, 8, None, 0, 1, 4, 1, 4, 2, o, None, st), E_NULL),
        "lowres null comb": (lib.vx_ssn2d_lowres(s, 4, s, 8, None, 0, 1, 4, 1, 4, 2, None, None, st), E_NULL),
        "lowres B = 0": (lib.vx_ssn2d_lowres(s, 4, s, 8, None, 0, 0, 4, 1, 4, 2, o, None, st), E_SHAPE),
        "lowres pix = 0": (lib.vx_ssn2d_lowres(s, 4, s, 8, None, 0, 1, 0, 1, 4, 2, o, None, st), E_SHAPE),
        "lowres B * pix = 2^32": (lib.vx_ssn2d_lowres(s, 4, s, 8, None, 0, 2, big, 1, 4, 2, o, None, st), E_SHAPE),
        "lowres B * S = 2^31": (lib.vx_ssn2d_lowres(s, 4, s, 8, None, 0, 1 << 16, 1, 1 << 15, 4, 2, o, None, st), E_SHAPE),
        "lowres R*C past an int": (lib.vx_ssn2d_lowres(s, 1 << 16, s, 8, None, 0, 1, 4, 1, 1 << 16, 1 << 16, o, None, st),
                                   E_SHAPE),
    }
    for name, (rc, want) in calls.items():
        assert rc == want, f"{name}: rc = {rc}, expected {want}"
    assert out.untouched(), "a refused call wrote to its output"
    # R = 0 needs no factor
    comb = _Out((1, 4, 4))
    _lib.check(lib.vx_ssn2d_lowres(s, 4, None, 0, None, 0, 1, 4, 1, 4, 0, comb.p, None, st), "vx_ssn2d_lowres R = 0")
    assert (comb.get() == 0).all()


# ---- h. vx_pack_input_cl8 -----------------------------------------------------------------------------------------------
def _pack(x, N, repeat, src, flip):
    V, Cin, D, H, W = x.shape
    out = _Out((N, D, H, W, 8))
    hold = (_dev(x), _dev(src, np.int32), _dev(flip, np.int32))
    rc = _lib.load().vx_pack_input_cl8(_lib.ptr(hold[0]), out.p, N, Cin, D, H, W, repeat, _lib.ptr(hold[1]), _lib.ptr(hold[2]),
                                       _lib.stream_ptr())
    return rc, out


@pytest.mark.parametrize("Cin", [1, 2, 3, 4, 5, 8])
def test_pack_input_cl8_is_the_index_arithmetic(Cin):
    D, H, W = 3, 5, 7
    modes = [(8, 8, 1, None, np.arange(8)),                                   # (V, N, repeat, src, flip)
             (3, 9, 3, None, np.arange(9) % 8),
             (3, 8, 1, np.array([2, 0, 1, 1, 0, 2, 2, 1]), np.arange(8)[::-1].copy()),
             (2, 2, 1, None, None)]
    for V, N, repeat, src, flip in modes:
        x = _ft((V, Cin, D, H, W), 2100 + 10 * Cin + V, 3.0)
        assert (x != 0).all()
        rc, out = _pack(x, N, repeat, src, flip)
        assert rc == 0
        got = out.get()
        np.testing.assert_array_equal(got, sr.pack_input_cl8(x, N, repeat, src, flip))
        assert (got[..., Cin:] == 0).all() and (got[..., :Cin] != 0).all()
        if flip is not None and src is None and repeat == 1:     # the restatement's flips are torch.flip's (test_3D.py:430)
            for n in range(N):
                dims = [d + 1 for d in range(3) if flip[n] >> d & 1]
                np.testing.assert_array_equal(got[n, ..., :Cin], np.moveaxis(np.flip(x[n], dims) if dims else x[n], 0, -1))


def test_pack_input_cl8_refuses_nine_channels_and_takes_a_second_loop_trip():
    rc, out = _pack(np.ones((1, 9, 1, 2, 2), F32), 1, 1, None, None)
    assert rc == E_SHAPE and out.untouched()
    D, H, W = 1, 17, 246739
    assert D * H * W == (1 << 22) + 259 > 16384 * 256
    x = _ft((1, 2, D, H, W), 2190, 3.0)
    rc, out = _pack(x, 1, 1, None, np.array([7]))
    assert rc == 0
    got, want = out.get().reshape(-1, 8), sr.pack_input_cl8(x, 1, 1, None, [7]).reshape(-1, 8)
    assert np.array_equal(got[:1024], want[:1024]), "head"
    assert np.array_equal(got[-1024:], want[-1024:]), "tail"
    assert np.array_equal(got, want)


# ---- i. vx_colorize_u8 ----------------------------------------------------------------------------------------------------
def _colorize(labels, ignore, lut, unlabeled):
    n = len(labels)
    rgb = _Out((n, 3), torch.uint8)
    hold = (_dev(labels, np.uint8), _dev(ignore, np.uint8), _dev(lut, np.uint8))
    rc = _lib.load().vx_colorize_u8(_lib.ptr(hold[0]), _lib.ptr(hold[1]), n, _lib.ptr(hold[2]), unlabeled, rgb.p,
                                    _lib.stream_ptr())
    return rc, rgb


@pytest.mark.parametrize("n", [1, 255, (1 << 20) + 517])
def test_colorize_u8_is_the_lookup(n):
    lut = ((formula_tensor((256, 3), 2200, 1.0) + 1.0) * 128).astype(np.uint8)
    assert len(np.unique(lut, axis=0)) > 250
    labels = ((np.arange(n) * 167 + 255) % 256).astype(np.uint8)          # n >= 256: all 256 labels, 255 first
    ignore = (formula_tensor((n,), 2201, 1.0) > 0.5).astype(np.uint8) * 3
    if n > 256:
        assert len(np.unique(labels)) == 256 and 0 < ignore.astype(bool).mean() < 1
    for ign in (None, ignore):
        for unlabeled in (0, 255):
            rc, rgb = _colorize(labels, ign, lut, unlabeled)
            assert rc == 0
            got, want = rgb.get(), sr.colorize(labels, ign, lut, unlabeled)
            assert np.array_equal(got[:1024], want[:1024]) and np.array_equal(got[-1024:], want[-1024:])
            assert np.array_equal(got, want), f"ignore={'given' if ign is not None else 'null'} unlabeled={unlabeled}"
    rc, rgb = _colorize(labels, ignore, lut, 256)
    assert rc == E_SHAPE and rgb.untouched()
    rc, rgb = _colorize(labels, ignore, lut, -1)
    assert rc == E_SHAPE and rgb.untouched()


# ---- j. the drivers, at batch 2 ---------------------------------------------------------------------------------------------
def test_ssn_unet3d_samples_a_batch_of_two_with_its_own_head():
    """dist.sample against lowrank_rsample fed with the DEVICE head's loc / cov_diag / cov_factor: the sampling alone, at
    a batch size where the (draw, image) strides of eps_w / eps_d and the head stride matter.  mean_only (rank 0) on the
    same batch: the head handed to the kernel must then hold 2 * C planes per image."""
    from oracle.ssn_oracle import lowrank_rsample
    from tests.formula import formula_ssn_state_dict, formula_volume
    from values_amd import SsnUNet3D
    NC, R, size, B, S = 2, 10, 16, 2, 3
    m = SsnUNet3D(num_classes=NC, rank=R)
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in formula_ssn_state_dict(NC, R).items()}, strict=True)
    m = m.cuda()
    x = torch.from_numpy(np.concatenate([formula_volume((1, 1, size, size, size), tag=t) for t in (7, 8)], 0)).float().cuda()
    vox = size ** 3
    dist = m(x)
    head = _np(dist._head).astype(np.float64).reshape(B, (2 + R) * NC, vox)
    assert not np.allclose(head[0], head[1])
    loc = head[:, :NC].reshape(B, -1)
    diag = (np.exp(head[:, NC:2 * NC]) + float(F32(1e-5))).reshape(B, -1)
    fac = head[:, 2 * NC:].reshape(B, R, NC * vox).transpose(0, 2, 1)          # view/flatten/transpose of :52-55
    ew, ed = _ft((S, B, R), 2300, 1.7), _ft((S, B, NC * vox), 2301, 1.7)
    smp = dist.sample([S], eps_w=torch.from_numpy(ew), eps_d=torch.from_numpy(ed))
    assert tuple(smp.shape) == (S, B, NC * vox)
    _close(_np(smp), lowrank_rsample(loc, diag, fac, ew, ed), "ssn", "SsnUNet3D batch 2")
    d0 = m(x, mean_only=True)
    smp0 = d0.sample([S], eps_d=torch.from_numpy(ed))
    _close(_np(smp0), lowrank_rsample(loc, diag, np.zeros((B, NC * vox, 0)), np.zeros((S, B, 0)), ed), "ssn",
           "SsnUNet3D batch 2, mean_only")


def test_predict_uncertainty_places_each_aleatoric_member_samples():
    """two aleatoric-head members, two volumes, three draws each with eps per member: member mi's samples land in
    [:, mi*3:(mi+1)*3] and are mu_mi + exp(s_mi / 2) * eps_mi (test_3D.py:458-469), mu and s from the oracle forward"""
    from oracle.unet3d_oracle import unet3d_forward
    from tests.formula import formula_unet3d_state_dict, formula_volume
    from tests.test_gpu_unet3d import LOGIT_TOL
    from values_amd import UNet3D, predict_uncertainty
    V, Ts, NC, size = 2, 3, 2, 16
    x = torch.from_numpy(np.concatenate([formula_volume((1, 1, size, size, size), tag=t) for t in (44, 46)], 0))
    models, sds, eps = [], [], []
    for mi in range(2):
        sd = formula_unet3d_state_dict(seed_tag=4 + mi, aleatoric_loss=True)
        model = UNet3D(num_classes=NC, aleatoric_loss=True)
        model.load_state_dict({k: torch.from_numpy(v).float() for k, v in sd.items()})
        models.append(model.cuda())
        sds.append(sd)
        eps.append(torch.from_numpy(formula_tensor((V, Ts, NC, size, size, size), 2400 + mi, scale=1.7)))
    out = predict_uncertainty(models, x.float().cuda(), n_aleatoric_samples=Ts, eps=eps)
    logits = _np(out["logits"])
    assert logits.shape == (V, 2 * Ts, NC, size, size, size)
    for mi in range(2):
        with torch.no_grad():
            mu, s = unet3d_forward({k: torch.from_numpy(v) for k, v in sds[mi].items()}, x, aleatoric_loss=True, num_classes=NC)
        want = mu.numpy()[:, None] + np.exp(s.numpy()[:, None] / 2) * eps[mi].numpy()
        err = deviation(logits[:, mi * Ts:(mi + 1) * Ts], want)
        print(f"deviation driver aleatoric member {mi} {err:.3e}")
        assert err < LOGIT_TOL, (mi, err)
