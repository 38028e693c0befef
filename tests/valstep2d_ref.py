"""Restatement of the 2D SSN head's validation reduction (numpy, no GPU, nothing from values_amd): the float32 sample
formation that vx_val_ssn2d_sums_batched (valstep.hip) fuses -- the route of LowRankNormal2D.sample_images -- feeding
tests/valstep_ref.np_val_ssn_sums and ssn_loss_dice_from_sums.  Pinned to torch and to tests/golden/valstep2d_kat.npz by
tests/test_valstep2d_ref_cpu.py; the kernel is held to it in tests/test_gpu_valstep2d.py.

The head lives at h0 x w0, channels-last: mean (B, h0, w0, pm >= C), factor (B, h0, w0, pf >= R C; channel r C + c).
    comb_s = mean + sum_r fmaf(factor_r, eps_w[s][b][r], .)      (the chain starts at 0; one rounding per fmaf)
    expm   = expf(mean)
    interp(x)(oy, ox) = hy * (hx * x00 + lx * x01) + ly * (hx * x10 + lx * x11)     every operation rounded to float32
        with (i0, i1, l) = bil_coord(o, n_in, n_out): ratio = f32(n_in) / f32(n_out), s = max((f32(o) + 0.5f) * ratio - 0.5f, 0),
        i0 = min(int(s), n_in - 1), i1 = i0 + (i0 < n_in - 1), l = s - f32(i0), h = 1 - l
    sd_c   = sqrtf(interp(expm)_c + epsilon)
    y_s,c  = interp(comb_s)_c + sd_c * eps_d[s][b][c][pixel]
numpy's float32 arithmetic rounds once per operation, which is the device's arithmetic without contraction.  The fmaf is
formed in float64 (the product of two float32 is exact there) and rounded once to float32; expf and sqrtf are evaluated in
float64 on the float32 argument and rounded once.

WHAT SEPARATES THESE SAMPLES FROM THE DEVICE'S (u = 2^-23, one float32 ulp is at most u relative):
  the combination and its interpolation are the same correctly rounded operations on the same inputs: the same bits (but
  for a double rounding of the float64-formed fmaf, within the ulp32 allowance of valstep_ref, item 3);
  the diagonal term goes through the device's expf and sqrtf.  OpenCL C specification, single precision: exp <= 3 ulp,
  sqrt <= 3 ulp; this file's are within 0.5 ulp.  So expm differs by <= 3.5 u relative.  The interpolation adds positive
  terms with positive weights (no cancellation) through 4 roundings on the longest path, each of which can fall one ulp
  apart on perturbed operands: <= 7.5 u;  + epsilon, one more rounding: <= 8.5 u;  the square root halves a relative
  perturbation and adds its own 3.5 u: <= 7.75 u;  the product with eps_d rounds once more: <= 8.75 u < 9 u relative, i.e.
  below 18 ulp32(sd_c * eps_d) (u |x| < 2 ulp32(x)).  A log-softmax follows its inputs with slope <= 2, so a log term moves by
         DIAG_ULP * ulp32(max_c |sd_c * eps_d_c|),   DIAG_ULP = 2 * 18 = 36
  per pixel that takes one, on top of valstep_ref's 2 ulp32(max_c |y_c|) for the closing addition (diag_allow below).
  The input builder keeps every top-two gap wider than twice the whole sample deviation (or an exact tie), so no arg-max
  depends on it.
"""
from __future__ import annotations

import numpy as np

from tests import valstep_ref as vr
from tests.ops2d_ref import bil_coord_f32 as bil_coord     # the float32 coordinate rule, restated once for all 2D kernels

F32 = np.float32
DIAG_ULP = 36.0


def interp(x, H, W):
    """x (..., h0, w0, C) float32 -> (..., H, W, C) float32: the expression of the module docstring"""
    x = np.asarray(x)
    assert x.dtype == F32
    h0, w0 = x.shape[-3:-1]
    y0, y1, ly = bil_coord(np.arange(H), h0, H)
    x0, x1, lx = bil_coord(np.arange(W), w0, W)
    hy, hx = (F32(1) - ly)[:, None, None], (F32(1) - lx)[None, :, None]
    ly, lx = ly[:, None, None], lx[None, :, None]
    r0, r1 = x[..., y0, :, :], x[..., y1, :, :]
    p00, p01, p10, p11 = r0[..., x0, :], r0[..., x1, :], r1[..., x0, :], r1[..., x1, :]
    out = hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11)
    assert out.dtype == F32
    return out


def _f(fn, x):
    with np.errstate(over="ignore"):
        return fn(np.asarray(x, np.float64)).astype(F32)


def lowres(mean, fac, eps_w, C, R):
    """mean (B, h0, w0, pm), fac (B, h0, w0, pf) or None, eps_w (S, B, R) -> comb (S, B, h0, w0, C), expm (B, h0, w0, C)"""
    m = np.asarray(mean, F32)[..., :C]
    S = eps_w.shape[0]
    comb = np.empty((S,) + m.shape, F32)
    for s in range(S):
        low = np.zeros(m.shape, F32)
        for k in range(R):
            f = np.asarray(fac, F32)[..., k * C:(k + 1) * C].astype(np.float64)
            low = (f * eps_w[s, :, k].astype(np.float64)[:, None, None, None] + low.astype(np.float64)).astype(F32)   # fmaf
        comb[s] = m + low
    return comb, _f(np.exp, m)


def samples(mean, fac, eps_w, eps_d, C, R, H, W, epsilon=1e-5):
    """-> y (B, S, C, H * W) float32 the sample logits, dmag (B, S, H * W) float64 = max_c |sd_c * eps_d_c|.
    eps_w (S, B, R) (anything of S rows at R = 0), eps_d (S, B, C * H * W)"""
    B = mean.shape[0]
    S = eps_d.shape[0]
    if R == 0:
        eps_w = np.zeros((S, B, 0), F32)
    comb, expm = lowres(mean, fac, np.asarray(eps_w, F32), C, R)
    sd = _f(np.sqrt, interp(expm, H, W) + F32(epsilon))                             # (B, H, W, C)
    sd = np.moveaxis(sd, -1, 1).reshape(B, C, H * W)
    ed = np.asarray(eps_d, F32).reshape(S, B, C, H * W)
    y = np.empty((B, S, C, H * W), F32)
    dmag = np.empty((B, S, H * W))
    for s in range(S):
        up = np.moveaxis(interp(comb[s], H, W), -1, 1).reshape(B, C, H * W)
        diag = sd * ed[s]
        assert diag.dtype == F32
        y[:, s] = up + diag
        dmag[:, s] = np.abs(diag).max(1)
    return y, dmag


def sample_deviation(y, dmag):
    """the bound of the module docstring on |device sample - this file's| per (b, s, pixel): 18 ulp32 of the diagonal term
    + 2 ulp32 of the logit"""
    return 0.5 * DIAG_ULP * vr.ulp32(dmag) + 2 * vr.ulp32(np.abs(y).max(2))


def gaps_ok(y, dmag, min_gap_ulp=4):
    """every pixel of every sample: the top-two gap exceeds twice the sample deviation, or is an exact tie; and valstep_ref's own
    rule holds with min_gap_ulp"""
    srt = np.sort(np.asarray(y, np.float64), axis=2)
    gap = srt[:, :, -1] - srt[:, :, -2]
    return bool(np.all((gap > 2 * sample_deviation(y, dmag)) | (gap == 0.0))) and vr.top_two_gap_ok(y, n_ulp=min_gap_ulp)


def diag_allow(dmag, labels, C, ignore_label):
    """(B, S): sum over the pixels that take a log term of DIAG_ULP * ulp32(max_c |sd_c eps_d_c|)"""
    B, S = dmag.shape[:2]
    out = np.zeros((B, S))
    for b in range(B):
        _, take, _ = vr._label_masks(labels[b], C, ignore_label)
        out[b] = (DIAG_ULP * vr.ulp32(dmag[b]))[:, take].sum(1)
    return out


def np_val_ssn2d_sums(y, dmag, labels, ignore_label=-1):
    """valstep_ref.np_val_ssn_sums on numpy-formed samples with the diagonal term's allowance added to the log-term slot"""
    C = y.shape[2]
    ss, smag, sallow, ts = vr.np_val_ssn_sums(y, labels, ignore_label, numpy_samples=True)
    sallow[:, :, 0] += diag_allow(dmag, labels, C, ignore_label)
    return ss, smag, sallow, ts


def case(rng, B, S, C, R, h0, w0, H, W, pm=None, pf=None, epsilon=1e-5, tie=True, min_gap_ulp=4):
    """a head with pitches pm / pf (padding lanes hold a sentinel the kernels must not read as data), normals, and the
    float32 samples; tie: full-resolution pixel (H * W) // 3 of item 0 has one value in every class of every sample (its
    source pixels carry one mean in every class and no factor, its eps_d is zero); min_gap_ulp: the top-two gaps also exceed
    that many ulp32 of the two logits' larger magnitude"""
    pm = pm or C + 3
    pf = pf or R * C + 1
    mean = np.full((B, h0, w0, pm), 1e30, F32)
    mean[..., :C] = (rng.standard_normal((B, h0, w0, C)) * 1.5).astype(F32)
    fac = None
    if R:
        fac = np.full((B, h0, w0, pf), 1e30, F32)
        fac[..., :R * C] = (rng.standard_normal((B, h0, w0, R * C)) * 0.2).astype(F32)
    eps_w = rng.standard_normal((S, B, max(R, 1))).astype(F32)[:, :, :R]
    eps_d = rng.standard_normal((S, B, C, H * W)).astype(F32)
    tp = (H * W) // 3
    if tie:
        y0, y1, _ = bil_coord(np.array([tp // W]), h0, H)
        x0, x1, _ = bil_coord(np.array([tp % W]), w0, W)
        for yy in (int(y0[0]), int(y1[0])):
            for xx in (int(x0[0]), int(x1[0])):
                mean[0, yy, xx, :C] = F32(0.75)
                if R:
                    fac[0, yy, xx, :R * C] = 0.0
        eps_d[:, 0, :, tp] = 0.0
    for _ in range(12):
        y, dmag = samples(mean, fac, eps_w, eps_d.reshape(S, B, -1), C, R, H, W, epsilon)
        srt = np.sort(y.astype(np.float64), axis=2)
        gap = srt[:, :, -1] - srt[:, :, -2]
        bad = (gap <= np.maximum(2 * sample_deviation(y, dmag), min_gap_ulp * vr.ulp32(np.abs(y).max(2)))) & (gap != 0.0)   # (B, S, HW)
        if not bad.any():
            break
        bs, ss_, vs_ = np.nonzero(bad)
        eps_d[ss_, bs, 0, vs_] += F32(1.0)     # local: one pixel of one sample
    assert gaps_ok(y, dmag, min_gap_ulp), "input builder (ssn2d): a top-two gap within the sample deviation"
    if tie:
        assert (y[0, :, :, tp] == y[0, :, :1, tp]).all()
    return mean, fac, eps_w, eps_d.reshape(S, B, C * H * W), y, dmag
