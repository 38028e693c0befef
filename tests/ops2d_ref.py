"""Host restatement of the streaming operations of the 2D (HRNet) path, from their documented formulas in
include/values_amd.h: BatchNorm scale / shift from (sum, sumsq) partials, the affine + bilinear gather, the SUM fusion,
the NCHW upsample with slots and un-flips, and the keep-bits of the hash dropout.  Plain numpy on channels-last arrays
[N][H][W][C] of REAL channels (pitches are the caller's business); no GPU, no product code.

Every *_f32 function rounds once per operation, in the header's order, so a kernel built without contraction must give
the same BITS; its *_f64 twin evaluates the same formula in float64 with the float32 source coordinates of
bil_coord_f32 (the float32 coordinate is part of the operation's definition: the reference interpolates in float32)."""
from __future__ import annotations

import collections
import math

import numpy as np

F32 = np.float32
_M32 = np.uint64(0xFFFFFFFF)
EPS32 = np.float32(1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# hash dropout: host restatement of the generator (csrc/common.h: vx_drop_key / vx_drop_word), pinned to the device's
# words by tests/test_gpu_kernels.py
def _np_mix32(h):
    h = h.astype(np.uint64) & _M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7feb352d)) & _M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846ca68b)) & _M32
    h ^= h >> np.uint64(16)
    return h


def _np_key(seed, layer, sample):
    """host restatement of vx_drop_key: the two key words of a (seed, layer, sample) stream"""
    s, l, n = (np.asarray(v, dtype=np.uint64) for v in (seed, layer, sample))
    a = _np_mix32((s * np.uint64(0x9E3779B1) + l * np.uint64(0x85EBCA6B) + n * np.uint64(0xC2B2AE35) + np.uint64(0x27D4EB2F)) & _M32)
    b = _np_mix32((s * np.uint64(0xC2B2AE3D) + l * np.uint64(0x27D4EB2F) + n * np.uint64(0x165667B1) + np.uint64(0x9E3779B9)) & _M32)
    return a, b


def _np_words(a, b, nwords, old=False):
    """keep-words 0 .. nwords - 1 of the stream keyed (a, b); old = the one-word construction of rounds 1-5 (vx_mix32(index ^ a))"""
    w = np.arange(nwords, dtype=np.uint64) ^ np.uint64(a)
    if old:
        return _np_mix32(w)
    w ^= w >> np.uint64(16)
    w = (w * np.uint64(0x7feb352d)) & _M32
    w = (w + np.uint64(b)) & _M32
    w ^= w >> np.uint64(15)
    w = (w * np.uint64(0x846ca68b)) & _M32
    w ^= w >> np.uint64(16)
    return w


def hash_keep_mask(seed, layer, n, elems):
    """keep-mask [n][elems] (uint8 0/1) of VX_DROP_HASH: element e of sample s is bit e % 32 of keep-word e / 32 of the
    stream keyed (seed, layer, s)"""
    nw = (elems + 31) // 32
    out = np.empty((n, elems), dtype=np.uint8)
    sh = np.arange(32, dtype=np.uint64)
    for s in range(n):
        a, b = _np_key(seed, layer, s)
        w = _np_words(int(a), int(b), nw)
        out[s] = ((w[:, None] >> sh[None, :]) & np.uint64(1)).reshape(-1)[:elems].astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm2d, training mode: scale = gamma * rstd, shift = beta - mean * scale (biased variance, eps = float32 1e-5)
def exact_sums(partials_f32):
    """[..., ntiles, C, 2] float32 -> [..., C, 2] float64: every (sum, sumsq) column summed exactly (math.fsum: the correctly
    rounded float64 of the exact sum)"""
    p = np.asarray(partials_f32)
    assert p.dtype == np.float32 and p.ndim >= 3 and p.shape[-1] == 2
    cols = np.moveaxis(p.astype(np.float64), -3, -1)                # [..., C, 2, ntiles]
    flat = cols.reshape(-1, cols.shape[-1])
    return np.array([math.fsum(r) for r in flat.tolist()]).reshape(cols.shape[:-1])


def bn_scale_shift_from_sums(s, q, count, eps_f32=EPS32, gamma=None, beta=None):
    """float64 throughout: mu = s / n, var = max(q / n - mu^2, 0), scale = gamma / sqrt(var + eps), shift = beta - mu * scale;
    eps is the float32 value; null gamma / beta mean 1 / 0"""
    s, q = np.asarray(s, dtype=np.float64), np.asarray(q, dtype=np.float64)
    mu = s / count
    var = np.maximum(q / count - mu * mu, 0.0)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps_f32)))
    g = 1.0 if gamma is None else np.asarray(gamma).astype(np.float64)
    b = 0.0 if beta is None else np.asarray(beta).astype(np.float64)
    scale = g * rstd
    return scale, b - mu * scale


def bn_scale_shift_exact(partials_f32, count, eps_f32=EPS32, gamma=None, beta=None):
    """partials_f32 [ntiles][C][2] float32 (sum, sumsq) -> (scale, shift) float64 [C]: exact summation of the partials, then
    float64; variance clamped at 0; null gamma / beta mean 1 / 0."""
    sums = exact_sums(partials_f32)
    assert sums.ndim == 2
    return bn_scale_shift_from_sums(sums[:, 0], sums[:, 1], count, eps_f32, gamma, beta)


def bn_scale_shift_exact_groups(partials_f32, groups, cpitch, count_per_group, eps_f32=EPS32, gamma=None, beta=None):
    """G statistics groups: group g owns tiles [g * ntiles, (g + 1) * ntiles) of the partials and row g of the returned
    scale / shift [G][cpitch] (float64); columns [C, cpitch) are NaN: nobody writes them."""
    p = np.asarray(partials_f32)
    assert p.shape[0] % groups == 0 and cpitch >= p.shape[1]
    nt, c = p.shape[0] // groups, p.shape[1]
    scale, shift = np.full((groups, cpitch), np.nan), np.full((groups, cpitch), np.nan)
    for g in range(groups):
        scale[g, :c], shift[g, :c] = bn_scale_shift_exact(p[g * nt:(g + 1) * nt], count_per_group, eps_f32, gamma, beta)
    return scale, shift


def ulp32(ref64):
    """the spacing of float32 at |ref| (of the float32 nearest to it), as float64"""
    r = np.abs(np.asarray(ref64, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(r, np.float32(np.inf)) - r).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# bilinear source coordinates of F.interpolate(align_corners=False), float32 as the reference computes them
def bil_coord_f32(d, n_in, n_out):
    """ratio = f32(n_in) / f32(n_out); s = (f32(d) + 0.5f) * ratio - 0.5f, clamped at 0; i0 = min(int(s), n_in - 1);
    i1 = i0 + (i0 < n_in - 1); l1 = s - i0.  Every operation rounded to float32.  Returns (i0, i1, l1)."""
    d = np.asarray(d)
    ratio = F32(n_in) / F32(n_out)
    s = (d.astype(F32) + F32(0.5)) * ratio - F32(0.5)
    s = np.where(s < F32(0), F32(0), s).astype(F32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(F32)).astype(F32)
    assert ratio.dtype == np.float32 and l1.dtype == np.float32
    return i0, i1, l1


def _corners(v, oh, ow):
    _, h, w, _ = v.shape
    y0, y1, ly = bil_coord_f32(np.arange(oh), h, oh)
    x0, x1, lx = bil_coord_f32(np.arange(ow), w, ow)
    r0, r1 = v[:, y0], v[:, y1]
    return (r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]), ly, lx


def _resize(v, oh, ow, dt):
    """hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11), hy = 1 - ly, hx = 1 - lx; identity at equal sizes"""
    if v.shape[1:3] == (oh, ow):
        return v
    (v00, v01, v10, v11), ly, lx = _corners(v, oh, ow)
    hy, hx = (F32(1) - ly).astype(dt)[None, :, None, None], (F32(1) - lx).astype(dt)[None, None, :, None]
    ly, lx = ly.astype(dt)[None, :, None, None], lx.astype(dt)[None, None, :, None]
    out = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11)
    assert out.dtype == dt
    return out


def corner_abs_sum(x, out_hw):
    """sum of |corner| over the four source pixels of every output element (float64): the scale of a resize's rounding"""
    v = np.abs(np.asarray(x, dtype=np.float64))
    if v.shape[1:3] == tuple(out_hw):
        return v
    (v00, v01, v10, v11), _, _ = _corners(v, *out_hw)
    return v00 + v01 + v10 + v11


def _rows(t, n, group_images, dt):
    """scale / shift [C] or [G][C] -> [N][1][1][C]: image i takes row i / group_images"""
    t = np.asarray(t).astype(dt)
    if group_images > 0:
        assert t.ndim == 2
        return t[np.arange(n) // group_images][:, None, None, :]
    assert t.ndim == 1
    return np.broadcast_to(t, (n, 1, 1, t.shape[0]))


def _affine_gather(dt, x, out_hw=None, scale=None, shift=None, add=None, relu=False, keep=None, group_images=0):
    v = np.asarray(x).astype(dt)
    n, h, w, _ = v.shape
    oh, ow = out_hw or (h, w)
    if keep is not None:                                 # F.dropout(p = 0.5, training): times 2 or times 0
        v = v * np.where(np.asarray(keep).reshape(v.shape) != 0, dt(2), dt(0))
    v = _resize(v, oh, ow, dt)
    if scale is not None:
        v = v * _rows(scale, n, group_images, dt) + _rows(shift, n, group_images, dt)
    if add is not None:
        v = np.asarray(add).astype(dt) + v
    if relu:
        v = np.maximum(v, dt(0))
    assert v.dtype == dt
    return v


def affine_gather_f32(x, **kw):
    """act(add + scale * G(drop(x)) + shift) in float32, one rounding per operation"""
    return _affine_gather(np.float32, x, **kw)


def affine_gather_f64(x, **kw):
    return _affine_gather(np.float64, x, **kw)


def _fuse_sum(dt, terms, out_hw, relu=False, group_images=0, reverse=False):
    """terms: [(x [N][H][W][C], scale or None, shift or None)], summed in term order (reverse: last term first)"""
    vals = [_affine_gather(dt, x, out_hw=tuple(out_hw), scale=sc, shift=sh, group_images=group_images) for x, sc, sh in terms]
    if reverse:
        vals = vals[::-1]
    acc = vals[0]
    for v in vals[1:]:
        acc = acc + v
    if relu:
        acc = np.maximum(acc, dt(0))
    assert acc.dtype == dt
    return acc


def fuse_sum_f32(terms, out_hw, **kw):
    return _fuse_sum(np.float32, terms, out_hw, **kw)


def fuse_sum_f64(terms, out_hw, **kw):
    return _fuse_sum(np.float64, terms, out_hw, **kw)


def _bilinear_nchw(dt, x, out_hw, slots=None, dst=None, flip=None, fill=np.nan):
    """x [N][H][W][C] -> out [slots][C][OH][OW] (filled with `fill`): image n lands in slot dst[n], its value for output
    pixel (oy, ox) at (OH - 1 - oy if flip[n] & 2 else oy, OW - 1 - ox if flip[n] & 1 else ox)"""
    v = np.asarray(x).astype(dt)
    n = v.shape[0]
    up = _resize(v, out_hw[0], out_hw[1], dt).transpose(0, 3, 1, 2)
    dst = list(range(n)) if dst is None else [int(d) for d in dst]
    slots = slots or (max(dst) + 1)
    out = np.full((slots,) + up.shape[1:], fill, dtype=dt)
    for i in range(n):
        u = up[i]
        f = 0 if flip is None else int(flip[i])
        if f & 1:
            u = u[:, :, ::-1]
        if f & 2:
            u = u[:, ::-1, :]
        out[dst[i]] = u
    return out


def bilinear_nchw_f32(x, out_hw, **kw):
    return _bilinear_nchw(np.float32, x, out_hw, **kw)


def bilinear_nchw_f64(x, out_hw, **kw):
    return _bilinear_nchw(np.float64, x, out_hw, **kw)


def softmax_f64(x, axis=1):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------------
# inputs shared by the CPU pin (tests/test_ops2d_ref_cpu.py) and the GPU matrix (tests/test_gpu_ops2d.py)
def f32_tensor(shape, tag, scale=1.0, offset=0.0):
    from tests.formula import formula_tensor
    return (formula_tensor(shape, tag, scale) + offset).astype(np.float32)


FINALIZE_NTILES = (1, 63, 64, 65, 255, 256, 257, 1000)
FINALIZE_C = (1, 3, 20, 720)
FINALIZE_TILE_PIXELS = 16           # every tile of the finalize inputs stands for 16 pixels
FinalizeCase = collections.namedtuple("FinalizeCase", "grouped ntiles C G cpitch tag")


def finalize_cases():
    """the inputs of the GPU matrix: ntiles x C through vx_bn_finalize, then G in {1, 3, 8} x cpitch in {C, round16(C) + 4}
    through vx_bn_finalize_groups"""
    cases = [FinalizeCase(False, nt, c, 1, c, 400 + 10 * i + j) for i, nt in enumerate(FINALIZE_NTILES) for j, c in enumerate(FINALIZE_C)]
    for nt, c in ((65, 20), (257, 3), (5, 720)):
        for g in (1, 3, 8):
            for cp in (c, (c + 15) // 16 * 16 + 4):
                cases.append(FinalizeCase(True, nt, c, g, cp, 500 + len(cases)))
    return cases


def finalize_case_id(c):
    return f"{'groups' if c.grouped else 'plain'}-nt{c.ntiles}-C{c.C}-G{c.G}-cp{c.cpitch}"


def finalize_partials(ntiles, c, tag, groups=1):
    """Statistics partials [groups * ntiles][c][2] float32 as a conv epilogue would leave them, and the pixel count per
    group.  Every tile holds 16 values u + off[g][ch] with u from formula_tensor in [-1, 1) and a per-(group, channel)
    offset in [-3, 3]: variance ~ 1/3, mean^2 / var <= 27 -- the condition (<= 1e4) under which the device's float64
    summation order cannot move a result by a float32 ulp.  The partials are the exact float64 sums rounded once to
    float32; groups differ visibly through their offsets."""
    from tests.formula import formula_tensor
    px = FINALIZE_TILE_PIXELS
    u = formula_tensor((groups * ntiles, px, c), tag)
    off = 3.0 * formula_tensor((groups, 1, 1, c), tag + 1)
    v = (u.reshape(groups, ntiles, px, c) + off).reshape(groups * ntiles, px, c)
    v = v.astype(np.float32).astype(np.float64)
    part = np.stack([v.sum(1), (v * v).sum(1)], -1).astype(np.float32)
    return part, ntiles * px


def clamp_partials():
    """The two degenerate inputs of the variance clamp, [4 tiles][2 channels][2] and the count (256 = 4 tiles of 64 pixels).
    Channel 0: the constant 0.5 -- every sum is exact and var == 0.  Channel 1: the constant 1 + 2^-12, whose exact sumsq per
    tile, 64 + 2^-5 + 2^-18, is no float32; rounded DOWN (64 + 2^-5) it gives q / n = 1 + 2^-11 < mu^2 = 1 + 2^-11 + 2^-24."""
    part = np.empty((4, 2, 2), dtype=np.float32)
    part[:, 0, 0], part[:, 0, 1] = 32.0, 16.0
    v = 1.0 + 2.0 ** -12
    q = np.float32(64.0 * v * v)
    if float(q) >= 64.0 * v * v:
        q = np.nextafter(q, np.float32(0))
    part[:, 1, 0], part[:, 1, 1] = np.float32(64.0 * v), q
    assert float(part[0, 1, 0]) == 64.0 * v and float(q) == 64.0 + 2.0 ** -5
    return part, 256


def order_sensitive_terms(n=2, c=4, hw=(8, 12)):
    """Three fusion terms (identity, 2x, 4x upsampled with scale / shift) of magnitudes 1, 1000 and 1000 with opposite
    signs of the large ones: (a + b) + c and (c + b) + a round differently on many elements."""
    h, w = hw
    a = f32_tensor((n, h, w, c), 901)
    b = f32_tensor((n, h // 2, w // 2, c), 902, scale=1000.0)
    d = f32_tensor((n, h // 4, w // 4, c), 903, scale=1000.0)
    sb, hb = f32_tensor((c,), 904, 0.3, 1.0), f32_tensor((c,), 905, 0.2)
    sd, hd = f32_tensor((c,), 906, 0.3, -1.0), f32_tensor((c,), 907, 0.2)
    return [(a, None, None), (b, sb, hb), (d, sd, hd)], (h, w)
