"""Restatement of the sampling kernels (numpy only, no GPU, nothing from values_amd): what vx_aleatoric_sample,
vx_ssn_sample, vx_ssn2d_lowres, vx_ssn2d_add_diag and their Gaussian generator vx_gauss (accumulate.hip), and the two
index kernels vx_pack_input_cl8 (conv3d_c1.hip) and vx_colorize_u8 (png.hip), are held to in tests/test_gpu_sample.py.

dtype=np.float64 is the reference.  dtype=np.float32 rounds the inputs and every intermediate to float32 (each
transcendental is evaluated in float64 on the rounded argument and rounded once, so the figure does not depend on a
platform's float32 libm); the tests use that form only to measure what float32 arithmetic alone costs on their inputs
(the "gap" of the tolerance rule).  Pinned to oracle.ssn_oracle.lowrank_rsample, to ssn_16.npz and to the aleatoric
formula by tests/test_sample_ref_cpu.py.
"""
from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
W_XOR = 0x5bd1e995          # generated eps_w of a seed comes from the streams of seed ^ W_XOR


def _u(x):
    return np.asarray(x).astype(np.uint64) & _M32


def _mul(x, k):
    return (_u(x) * np.uint64(k)) & _M32


def mix32(h):
    """vx_mix32 (common.h): two multiply-xorshift rounds on a 32-bit word"""
    h = _u(h)
    h = h ^ (h >> np.uint64(16))
    h = _mul(h, 0x7feb352d)
    h = h ^ (h >> np.uint64(15))
    h = _mul(h, 0x846ca68b)
    return h ^ (h >> np.uint64(16))


def stream_key(seed, b):
    """the ONE word that keys stream (slot) b of a seed: seed ^ (b * 0x85EBCA6B + 0x165667B1); two (seed, slot) pairs
    with the same word are the same stream"""
    return _u(seed) ^ ((_mul(b, 0x85EBCA6B) + np.uint64(0x165667B1)) & _M32)


def gauss_words(seed, a, b):
    """the two hash words of element a of stream b -> (h1, h2), uint64 arrays holding 32-bit values"""
    a = _u(a)
    h1 = mix32(_mul(a, 0x9E3779B1) ^ mix32(stream_key(seed, b)))
    h2 = mix32(h1 ^ np.uint64(0x27D4EB2F) ^ _mul(a, 0xC2B2AE35))
    return h1, h2


def uniforms(seed, a, b):
    """u1 in (0, 1], u2 in [0, 1): exact in float32 and float64 alike"""
    h1, h2 = gauss_words(seed, a, b)
    u1 = ((h1 >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (h2 >> np.uint64(8)).astype(np.float64) / 16777216.0
    return u1, u2


def _f(fn, x, dtype):
    """a transcendental in float64 on the (already rounded) argument, rounded once to dtype"""
    return fn(np.asarray(x, dtype=np.float64)).astype(dtype)


def gauss(seed, a, b, dtype=np.float64):
    """vx_gauss(seed, a, b) = sqrt(-2 log u1) * cos(pi * 2 u2), Box-Muller on the two words; a, b broadcast"""
    u1, u2 = uniforms(seed, a, b)
    u1, u2 = u1.astype(dtype), u2.astype(dtype)
    lg = _f(np.log, u1, dtype)
    rad = _f(np.sqrt, dtype(-2.0) * lg, dtype)
    ang = dtype(2.0) * u2
    cs = _f(lambda t: np.cos(np.pi * t), ang, dtype)
    return (rad * cs).astype(dtype)


def aleatoric(mu_s, eps=None, seed=0, N=1, T=1, C=1, nvox=1, dtype=np.float64):
    """mu_s [N][2C][nvox] (mu | s), eps [N][T][C][nvox] or None (generated: gauss(seed, c*nvox + v, n*T + t))
    -> out [N][T][C][nvox] = mu + exp(s / 2) * eps, sigma [N][C][nvox] = exp(s / 2)"""
    mu_s = np.asarray(mu_s).astype(dtype).reshape(N, 2 * C, nvox)
    mu, s = mu_s[:, :C], mu_s[:, C:]
    sigma = _f(np.exp, dtype(0.5) * s, dtype)
    if eps is None:
        a = np.arange(C * nvox).reshape(1, 1, C, nvox)
        b = (np.arange(N)[:, None] * T + np.arange(T)[None, :]).reshape(N, T, 1, 1)
        e = gauss(seed, a, b, dtype)
    else:
        e = np.asarray(eps).astype(dtype).reshape(N, T, C, nvox)
    out = mu[:, None] + (sigma[:, None] * e).astype(dtype)
    return out.astype(dtype), sigma


def _eps_w(eps_w, seed, S, N, R, dtype):
    """[S][N][R]: injected, or gauss(seed ^ W_XOR, k, n*S + s)"""
    if eps_w is not None:
        return np.asarray(eps_w).astype(dtype).reshape(S, N, R)
    b = (np.arange(N)[None, :] * S + np.arange(S)[:, None]).reshape(S, N, 1)
    return gauss((int(seed) ^ W_XOR) & 0xFFFFFFFF, np.arange(R).reshape(1, 1, R), b, dtype)


def _eps_d(eps_d, seed, S, N, per, dtype):
    """[S][N][per]: injected, or gauss(seed, r, n*S + s)"""
    if eps_d is not None:
        return np.asarray(eps_d).astype(dtype).reshape(S, N, per)
    b = (np.arange(N)[None, :] * S + np.arange(S)[:, None]).reshape(S, N, 1)
    return gauss(seed, np.arange(per).reshape(1, 1, per), b, dtype)


def ssn(head, eps_w=None, eps_d=None, seed=0, N=1, S=1, C=1, R=0, nvox=1, epsilon=1e-5, dtype=np.float64):
    """head [N][(2+R)C][nvox] = mean | log_cov_diag | cov_factor (channel r*C + c), eps_w [S][N][R], eps_d [S][N][C][nvox]
    (None: generated) -> out [N][S][C][nvox] = (mean + sum_r factor_r * eps_w[s][n][r]) + sqrt(exp(logd) + epsilon) * eps_d"""
    head = np.asarray(head).astype(dtype).reshape(N, (2 + R) * C, nvox)
    per = C * nvox
    mean, logd = head[:, :C].reshape(N, per), head[:, C:2 * C].reshape(N, per)
    fac = head[:, 2 * C:].reshape(N, R, per)
    with np.errstate(over="ignore"):
        sd = _f(np.sqrt, _f(np.exp, logd, dtype) + dtype(np.float32(epsilon)), dtype)
    ew = _eps_w(eps_w, seed, S, N, R, dtype) if R else None
    ed = _eps_d(eps_d, seed, S, N, per, dtype)
    out = np.empty((N, S, per), dtype=dtype)
    for s in range(S):
        low = np.zeros((N, per), dtype=dtype)
        for k in range(R):
            low = (low + (fac[:, k] * ew[s, :, k, None]).astype(dtype)).astype(dtype)
        out[:, s] = (mean + low).astype(dtype) + (sd * ed[s]).astype(dtype)
    return out.reshape(N, S, C, nvox)


def ssn2d_lowres(mean, pm, fac, pf, eps_w=None, seed=0, B=1, pix=1, S=1, C=1, R=0, dtype=np.float64):
    """channels-last mean [B*pix][pm] (C used), fac [B*pix][pf] (channel r*C + c; None for R = 0), eps_w [S][B][R]
    (None: generated) -> comb [S][B*pix][C] = mean + sum_r fac_r * eps_w[s][b][r], expm [B*pix][C] = exp(mean)"""
    P = B * pix
    m = np.asarray(mean).reshape(P, pm)[:, :C].astype(dtype)
    expm = _f(np.exp, m, dtype)
    comb = np.empty((S, P, C), dtype=dtype)
    if R:
        f = np.asarray(fac).reshape(P, pf)[:, :R * C].astype(dtype).reshape(B, pix, R, C)
        ew = _eps_w(eps_w, seed, S, B, R, dtype)
    for s in range(S):
        low = np.zeros((B, pix, C), dtype=dtype)
        for k in range(R):
            low = (low + (f[:, :, k] * ew[s, :, k, None, None]).astype(dtype)).astype(dtype)
        comb[s] = (m + low.reshape(P, C)).astype(dtype)
    return comb, expm


def ssn2d_add_diag(out, diag, eps_d=None, seed=0, S=1, B=1, per=1, epsilon=1e-5, dtype=np.float64):
    """out [B][S][per], diag [B][per], eps_d [S][B][per] (None: generated, slot b*S + s)
    -> out + sqrt(diag + epsilon) * eps_d, [B][S][per]"""
    out = np.asarray(out).astype(dtype).reshape(B, S, per)
    diag = np.asarray(diag).astype(dtype).reshape(B, per)
    sd = _f(np.sqrt, diag + dtype(np.float32(epsilon)), dtype)
    ed = _eps_d(eps_d, seed, S, B, per, dtype)
    return (out + (sd[:, None] * ed.transpose(1, 0, 2)).astype(dtype)).astype(dtype)


def pack_input_cl8(x, N, repeat=1, src=None, flip=None):
    """x (V, Cin, D, H, W) -> (N, D, H, W, 8): sample n is volume src[n] (None: n // repeat) with the axes of flip[n]
    reversed (bit 0: D, bit 1: H, bit 2: W; None: 0), channels last, channels Cin..7 zero"""
    x = np.asarray(x)
    V, Cin, D, H, W = x.shape
    out = np.zeros((N, D, H, W, 8), dtype=x.dtype)
    z, y, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    for n in range(N):
        vol = int(src[n]) if src is not None else n // repeat
        fl = int(flip[n]) if flip is not None else 0
        zs = D - 1 - z if fl & 1 else z
        ys = H - 1 - y if fl & 2 else y
        xs = W - 1 - xx if fl & 4 else xx
        for c in range(Cin):
            out[n, :, :, :, c] = x[vol, c][zs, ys, xs]
    return out


def colorize(labels, ignore, lut, unlabeled):
    """labels [n] u8, ignore [n] u8 or None, lut [256][3] u8 -> rgb [n][3] = lut[unlabeled where ignore else label]"""
    lab = np.asarray(labels).astype(np.int64)
    if ignore is not None:
        lab = np.where(np.asarray(ignore) != 0, int(unlabeled), lab)
    return np.asarray(lut).reshape(256, 3)[lab]
