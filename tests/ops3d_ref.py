"""Host restatement of the 3D streaming operations between the convolutions, from their documented formulas in
include/values_amd.h: InstanceNorm statistics from (sum, sumsq) partials, normalise + activation + dropout, the 2x2x2 max-pool,
the window maxima / any-dropped words a pooling conv leaves and the finish passes over them, the pre-split, the 1x1x1 head with
slots and un-flips, and the x-blocked concat buffer.  Plain numpy on channels-last arrays [N][D][H][W][C] of REAL channels
(pitches are the caller's business); no GPU, no product code.

Every *_f32 function rounds once per operation, in the header's order.  None of these expressions offers the compiler a
contraction (no product feeds a sum), so the *_f32 forms define the device's BITS; the *_f64 twins evaluate the same formula in
float64.

The conditioning statement (stat_bounds / y_bound) is derived, not observed.  The statistics are var = q / n - mu^2 over float32
(sum, sumsq) partials.  Let u = 2^-24 and let every partial be the exact sum over its tile rounded ONCE to float32 (a producer
whose running sum over m values rounds m times: u -> m u).  With A = sum_t |s_t| / n (<= mean |x|) and Q = sum_t q_t / n
(= sigma^2 + mu^2, all q_t >= 0), the finalize's float64 arithmetic being negligible beside u:

    |d mu|  <= u A
    |d var| <= u (sigma^2 + mu^2) + 2 |mu| u A + (u A)^2

and for y = (x - mu) * rstd, rstd = 1 / sqrt(var + eps):

    |d y| <= |d mu| rstd + |y| |d var| / (2 (var + eps))         (first order, the second factor applied to the bound's own
                                                                  worst case var - |d var| where that stays positive)
             + three float32 roundings of the stored result (mean and rstd stored as float32, then the subtraction and the
               product: each at most u relative to |x - mu| rstd or |y|)

The second term grows like (mu / sigma)^2 u |y| / 2: at |mu| / sigma = 30 it is ~5e-5 |y|, at 300 ~5e-3 |y| -- between the two
the formula leaves the project's 1e-4 map contract, whatever kernel evaluates it."""
from __future__ import annotations

import numpy as np

from tests.conv_lattice import split
from tests.ops2d_ref import exact_sums, hash_keep_mask, ulp32  # noqa: F401  (re-exported: the GPU matrix takes them from here)

F32 = np.float32
U24 = 2.0 ** -24
EPS32 = np.float32(1e-5)
ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2          # VX_ACT_* of include/values_amd.h


# ---------------------------------------------------------------------------------------------------------------------
# statistics
def instnorm_from_partials(partials_f32, count, eps=EPS32):
    """partials [..., ntiles, C, 2] float32 (sum, sumsq) -> (mean, rstd, mean_f32, rstd_f32), [..., C]: the partials summed
    exactly, then the header's formula in float64 -- mu = s / n, var = max(q / n - mu^2, 0), rstd = 1 / sqrt(var + eps) with the
    float32 eps -- and the two values rounded once to float32 (what a correctly rounding kernel stores)."""
    sums = exact_sums(partials_f32)
    mu = sums[..., 0] / count
    var = np.maximum(sums[..., 1] / count - mu * mu, 0.0)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    return mu, rstd, mu.astype(F32), rstd.astype(F32)


def instnorm_two_pass(x, eps=EPS32):
    """float64 two-pass InstanceNorm statistics of x [N][...][C] over the middle axes: (mean, var, rstd), [N][C]"""
    v = np.asarray(x, dtype=np.float64)
    v = v.reshape(v.shape[0], -1, v.shape[-1])
    mu = v.mean(1)
    var = ((v - mu[:, None, :]) ** 2).mean(1)
    return mu, var, 1.0 / np.sqrt(var + float(np.float32(eps)))


def ideal_partials(x, tiles):
    """x [N][...][C] -> partials [N][tiles][C][2] float32 of a tiling into `tiles` nearly equal runs of voxels: exact tile sums
    (math.fsum through exact_sums of the float32 squares is not available for products, so the squares are formed in float64,
    exact for float32 inputs, and summed exactly) rounded ONCE to float32; and the count per channel"""
    import math
    v = np.asarray(x)
    assert v.dtype == np.float32
    v = v.astype(np.float64).reshape(v.shape[0], -1, v.shape[-1])
    n, nvox, c = v.shape
    edges = [(nvox * t) // tiles for t in range(tiles + 1)]
    part = np.zeros((n, tiles, c, 2), dtype=np.float32)
    for t in range(tiles):
        seg = v[:, edges[t]:edges[t + 1]]
        if seg.shape[1] == 0:
            continue
        cols = np.moveaxis(seg, 1, -1).reshape(n * c, -1)
        part[:, t, :, 0] = np.array([math.fsum(r) for r in cols.tolist()]).reshape(n, c).astype(np.float32)
        part[:, t, :, 1] = np.array([math.fsum(r) for r in (cols * cols).tolist()]).reshape(n, c).astype(np.float32)
    return part, nvox


def stat_bounds(partials_f32, count, mu, var, u=U24):
    """(|d mu| bound, |d var| bound) of the module docstring, [..., C], for statistics (mu, var: the true float64 two-pass
    values) estimated from partials that carry a relative error u each"""
    p = np.asarray(partials_f32).astype(np.float64)
    a = np.abs(p[..., 0]).sum(-2) / count
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    dmu = u * a
    dvar = u * (var + mu * mu) + 2.0 * np.abs(mu) * u * a + (u * a) ** 2
    return dmu, dvar


def y_bound(x, partials_f32, count, eps=EPS32, u=U24):
    """Per-element bound [N][...][C] on |(x - mean_dev) * rstd_dev (float32, stored) - (x - mu) * rstd (float64 two-pass)| for a
    device that reduces `partials_f32` by the header's formula: the statistics' bound propagated, plus three float32 roundings.
    `u` is the relative error of one partial (2^-24 for ideal partials, m 2^-24 for a running sum over m values)."""
    x64 = np.asarray(x, dtype=np.float64)
    mu, var, rstd = instnorm_two_pass(x64, eps)
    dmu, dvar = stat_bounds(partials_f32, count, mu, var, u)
    e = float(np.float32(eps))
    shape = (x64.shape[0],) + (1,) * (x64.ndim - 2) + (x64.shape[-1],)
    mu, var, rstd, dmu, dvar = (t.reshape(shape) for t in (mu, var, rstd, dmu, dvar))
    lo = np.maximum(var - dvar, 0.0) + e                         # the smallest var + eps the device can have formed
    rstd_hi = 1.0 / np.sqrt(lo)
    y = np.abs(x64 - mu) * rstd
    stat = dmu * rstd_hi + (np.abs(x64 - mu) + dmu) * dvar / (2.0 * lo * np.sqrt(lo))
    # stored result: mean_f32 (u |mu|, times rstd), then rstd_f32, the subtraction and the product (u |y| each)
    return stat + 3.0 * U24 * (y + stat) + U24 * (np.abs(mu) + dmu) * rstd_hi


def out_bound(yb, y64, act, dropped_scale=1.0):
    """y_bound carried through the activation (Lipschitz 1; LeakyReLU's 0.01f t adds one rounding of |0.01 t| and the distance
    of 0.01f from 0.01, together below u |t|) and the dropout's exact factor"""
    extra = U24 * np.abs(y64) if act == ACT_LRELU else 0.0
    return dropped_scale * (yb + extra)


# ---------------------------------------------------------------------------------------------------------------------
# normalise, activation, dropout, pool
def _rows(t, x, dt):
    """statistics [N][C] (or None) -> broadcastable against x [N][...][C]"""
    t = np.asarray(t).astype(dt)
    return t.reshape((x.shape[0],) + (1,) * (x.ndim - 2) + (x.shape[-1],))


def _act(t, act, dt):
    if act == ACT_LRELU:
        return np.maximum(t, dt(0.01) * t)
    if act == ACT_RELU:
        return np.maximum(t, dt(0))
    assert act == ACT_NONE
    return t


def _norm_act_drop(dt, x, mean, rstd, act, keep, scale2):
    x = np.asarray(x)
    t = x.astype(dt)
    if mean is not None:
        t = (t - _rows(mean, x, dt)) * _rows(rstd, x, dt)
    t = _act(t, act, dt)
    if keep is not None:
        k = np.asarray(keep).reshape(x.shape) != 0
        t = np.where(k, (dt(2) if scale2 else dt(1)) * t, dt(0))
    assert t.dtype == dt
    return t


def norm_act_drop_f32(x, mean_f32, rstd_f32, act=ACT_LRELU, keep=None, scale2=True):
    """The kernel's order, one float32 rounding per operation: t = (x - mean) * rstd (mean None: t = x); LeakyReLU as
    max(t, 0.01f * t), ReLU as max(t, 0); kept -> 2 t (t when scale2 is false), dropped -> 0.  keep None: no dropout."""
    if mean_f32 is not None:
        assert np.asarray(mean_f32).dtype == np.float32 and np.asarray(rstd_f32).dtype == np.float32
    return _norm_act_drop(np.float32, x, mean_f32, rstd_f32, act, keep, scale2)


def norm_act_drop_f64(x, mean, rstd, act=ACT_LRELU, keep=None, scale2=True):
    return _norm_act_drop(np.float64, x, mean, rstd, act, keep, scale2)


def _windows(v):
    """[N][D][H][W][C] -> [N][D/2][H/2][W/2][8][C]"""
    n, d, h, w, c = v.shape
    assert d % 2 == 0 and h % 2 == 0 and w % 2 == 0
    return v.reshape(n, d // 2, 2, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4, 6, 7).reshape(n, d // 2, h // 2, w // 2, 8, c)


def maxpool2_f32(y):
    y = np.asarray(y)
    assert y.dtype == np.float32
    return _windows(y).max(4)


def maxpool2_f64(y):
    return _windows(np.asarray(y, dtype=np.float64)).max(4)


def _pack_flags(any_dropped):
    """[..., C] bool -> [..., C / 4] uint32: bit j of word q = channel 4 q + j"""
    a = np.asarray(any_dropped).astype(np.uint32)
    a = a.reshape(a.shape[:-1] + (a.shape[-1] // 4, 4))
    return (a << np.arange(4, dtype=np.uint32)).sum(-1).astype(np.uint32)


def pool_windows(x_raw, keep, layout=1):
    """What vx_conv3d_args.pool_out / pool_flags are documented to hold, from the raw tensor [N][D][H][W][C] and its keep-mask:
    per window and channel the maximum over KEPT raw values (-inf when none is kept) and the any-dropped bit, bit j of word q =
    channel 4 q + j.  layout 1 (C = 8): whole 2x2x2 windows, raw [N][D/2][H/2][W/2][C], flags [..][C/4]; layout 2 (C = 16): the
    (y, x) half of every window per z-plane, raw [N][D][H/2][W/2][C], flags [..][C/4]."""
    x = np.asarray(x_raw)
    assert x.dtype == np.float32
    k = np.asarray(keep).reshape(x.shape) != 0
    v = np.where(k, x, F32(-np.inf))
    if layout == 1:
        return _windows(v).max(4), _pack_flags(_windows(~k).any(4))
    assert layout == 2
    n, d, h, w, c = x.shape

    def yx(t):
        return t.reshape(n, d, h // 2, 2, w // 2, 2, c).transpose(0, 1, 2, 4, 3, 5, 6).reshape(n, d, h // 2, w // 2, 4, c)
    return yx(v).max(4), _pack_flags(yx(~k).any(4))


def _unpack_flags(flags, c):
    f = np.asarray(flags).astype(np.uint32)
    return ((f[..., None] >> np.arange(4, dtype=np.uint32)) & np.uint32(1)).reshape(f.shape[:-1] + (c,)) != 0


def pool_finish_f32(raw, flags, mean_f32, rstd_f32, scale2=True):
    """any_dropped ? max(s f(m), 0) : s f(m), f(m) = LeakyReLU((m - mean) * rstd), s = 2 with dropout else 1; one float32
    rounding per operation, in that order.  raw [N][...][C], flags [N][...][C/4]."""
    raw = np.asarray(raw)
    assert raw.dtype == np.float32
    with np.errstate(invalid="ignore"):
        v = norm_act_drop_f32(raw, mean_f32, rstd_f32, ACT_LRELU) * (F32(2) if scale2 else F32(1))
    return np.where(_unpack_flags(flags, raw.shape[-1]), np.maximum(v, F32(0)), v).astype(F32)


def pool_finish_z_f32(raw, flags, mean_f32, rstd_f32, scale2=True):
    """layout 2: the maximum / the OR over the z pair, then pool_finish_f32.  raw [N][2 Dp][...][16] -> [N][Dp][...][16]"""
    raw, flags = np.asarray(raw), np.asarray(flags)
    m = np.maximum(raw[:, 0::2], raw[:, 1::2])
    return pool_finish_f32(m, flags[:, 0::2] | flags[:, 1::2], mean_f32, rstd_f32, scale2)


# ---------------------------------------------------------------------------------------------------------------------
# pre-split
def prenorm_split_t_f32(x, mean_f32, rstd_f32, scale):
    """t = (x - mean) * (rstd * scale), LeakyReLU; float32, one rounding per operation (the scale joins rstd first)"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    sc = (_rows(rstd_f32, x, F32) * F32(scale)).astype(F32)
    t = ((x - _rows(mean_f32, x, F32)) * sc).astype(F32)
    return np.maximum(t, F32(0.01) * t)


def prenorm_split_f32(x, mean_f32, rstd_f32, scale):
    """x [N][nvox][8] float32 -> float16 [N][nvox][2][2][4]: per 16-byte piece (4 channels) [hi0 hi1 hi2 hi3 | lo0 lo1 lo2 lo3]
    with (hi, lo) = conv_lattice.split(t)"""
    t = prenorm_split_t_f32(x, mean_f32, rstd_f32, scale)
    with np.errstate(over="ignore", invalid="ignore"):          # |t| past 65504: hi = inf, as on the device (range_flag's business)
        hi, lo = split(t)
    n, nvox, c = t.shape
    out = np.stack([hi.reshape(n, nvox, c // 4, 4), lo.reshape(n, nvox, c // 4, 4)], 3)
    return out.astype(np.float16)


def unsplit(halves):
    """[..][2][4] (hi | lo) -> hi + lo / 2048 in float64, [..][4]"""
    h = np.asarray(halves).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return h[..., 0, :] + h[..., 1, :] / 2048.0


# ---------------------------------------------------------------------------------------------------------------------
# 1x1x1 head
def conv1x1_f64(x, w, b, dst=None, flip=None, slots=None, fill=np.nan):
    """x [N][D][H][W][F], w [C][F], b [C] -> (out, mag) float64 [slots][C][D][H][W]: sample n lands in slot dst[n] (None: n),
    un-flipped by flip[n] (bit 0 = D, bit 1 = H, bit 2 = W); unwritten slots hold `fill`.  mag = sum_k |w x| + |b| per element,
    the scale of the fma chain's rounding."""
    x64, w64, b64 = (np.asarray(t, dtype=np.float64) for t in (x, w, b))
    n = x64.shape[0]
    val = np.einsum("ndhwf,cf->ncdhw", x64, w64) + b64[None, :, None, None, None]
    mag = np.einsum("ndhwf,cf->ncdhw", np.abs(x64), np.abs(w64)) + np.abs(b64)[None, :, None, None, None]
    dst = list(range(n)) if dst is None else [int(d) for d in dst]
    slots = slots or (max(dst) + 1)
    out = np.full((slots,) + val.shape[1:], fill, dtype=np.float64)
    om = np.zeros_like(out)
    for i in range(n):
        f = 0 if flip is None else int(flip[i])
        axes = tuple(1 + k for k in range(3) if f >> k & 1)
        out[dst[i]] = np.flip(val[i], axes) if axes else val[i]
        om[dst[i]] = np.flip(mag[i], axes) if axes else mag[i]
    return out, om


# ---------------------------------------------------------------------------------------------------------------------
# the decoder's concat buffer CAT[N][D][H][W/xb][2][xb][C] (numpy, channels-last)
def to_xblk(half_tensor, half, xb, fill):
    """[N][D][H][W][C] -> concat buffer with `half_tensor` as half `half` and `fill` in the other"""
    t = np.asarray(half_tensor)
    n, d, h, w, c = t.shape
    assert w % xb == 0
    buf = np.full((n, d, h, w // xb, 2, xb, c), fill, dtype=t.dtype)
    buf[:, :, :, :, half] = t.reshape(n, d, h, w // xb, xb, c)
    return buf


def from_xblk(buf, half):
    b = np.asarray(buf)
    n, d, h, wb, _, xb, c = b.shape
    return b[:, :, :, :, half].reshape(n, d, h, wb * xb, c)


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's index decode: magic = 2^32 / d + 1 (0 for d = 1), mulhi(i, magic) == i // d while i * d < 2^32
def magic(d):
    return 0 if d == 1 else (1 << 32) // d + 1


def magic_div(i, d):
    i = np.asarray(i, dtype=np.uint64)
    m = magic(d)
    return i if m == 0 else (i * np.uint64(m)) >> np.uint64(32)


# ---------------------------------------------------------------------------------------------------------------------
# inputs shared by the CPU pin and the GPU matrix
MU_OVER_SIGMA = (0.0, 3.0, 30.0, 300.0, 3000.0)
CONSTANTS = (0.37, 1.0, 1000.0, -3.3e-3)


def conditioned(shape, tag, ratios, constant=None):
    """[N][nvox][C] float32: channel c of every sample is sigma * u + ratio[c % len] * sigma with u from formula_tensor
    (uniform in [-1, 1): sigma = 1 / sqrt(3) of the amplitude), amplitude 1.7; the LAST channel is `constant` where given"""
    from tests.formula import formula_tensor
    n, nvox, c = shape
    u = formula_tensor((n, nvox, c), tag)
    amp = 1.7
    sigma = amp / np.sqrt(3.0)
    off = np.array([ratios[i % len(ratios)] * sigma * (-1.0 if i % 2 else 1.0) for i in range(c)])
    v = (amp * u + off[None, None, :]).astype(np.float32)
    if constant is not None:
        v[:, :, -1] = np.float32(constant)
    return v


def plant_split_values(x, mean_f32, rstd_f32, scale):
    """plants into sample 0 of x [N][nvox][8] the elements whose normalised value t lands on: +-0 and an fp16-subnormal, values
    whose lo underflows (1e-7), values just past either side of hi's tie (1 + 2^-11 -+ 2^-20), a tiny negative (LeakyReLU then
    underflow) -- x = mean + t / (rstd * scale) in float32; returns the t wanted"""
    want = [0.0, 1e-7, -1e-7, 1.0 + 2.0 ** -11 + 2.0 ** -20, 1.0 + 2.0 ** -11 - 2.0 ** -20, -6e-8, 3e-5, -3e-5]
    for j, t in enumerate(want):
        c = j % 8
        x[0, j, c] = np.float32(mean_f32[0, c] + np.float32(t) / (rstd_f32[0, c] * np.float32(scale)))
    return want


# ---------------------------------------------------------------------------------------------------------------------
# the thinned matrix of vx_norm_act_drop_pool and its forms (tests/test_gpu_stream3d.py launches it; tests/test_ops3d_ref_cpu.py
# proves its coverage and checks the index decode for every divisor it produces)
import collections  # noqa: E402

NormCase = collections.namedtuple("NormCase", "inst C shape act drop layout tiles repeat")
INSTANCES = {          # name -> (entry point, pooling, kernel name vx_last_kernel_name() must report)
    "plain": ("plain", False, "norm_act_drop_pool_kernel<false,false>"),
    "pool": ("plain", True, "norm_act_drop_pool_kernel<true,false>"),
    "wide": ("plain", True, "norm_act_drop_pool_kernel<true,true>"),
    "plain_stats": ("stats", False, "norm_act_drop_pool_kernel<false,false,true>"),
    "pool_stats": ("stats", True, "norm_act_drop_pool_kernel<true,false,true>"),
    "wide_stats": ("stats", True, "norm_act_drop_pool_kernel<true,true,true>"),
    "fanout": ("bcast", False, "norm_act_drop_fanout_kernel"),
}
POOL_SHAPES = ((3, 2, 2, 2), (2, 4, 6, 10), (1, 2, 2, 66))
NOPOOL_SHAPES = ((2, 1, 1, 1), (3, 3, 5, 7), (1, 1, 1, 21))
XB4_SHAPES = {True: (2, 2, 4, 8), False: (2, 1, 3, 8)}       # where a concat layout's block does not divide W of the shape drawn
C_SHUFFLE, C_WIDE, C_NOPOOL = (4, 8, 16, 32, 64, 128), (132, 256), (4, 8, 12, 20, 96, 16)
POOL_REFUSED_C = (12, 20, 96)
_COMMON_LAYOUTS = ["dense", "x_pitch", "out_pitch"] + [f"out_xblk{xb}_{h}" for xb in (1, 2, 4) for h in (0, 1)]
_POOL_LAYOUTS = _COMMON_LAYOUTS + ["pool_pitch"] + [f"x_xblk{xb}_{h}{o}" for xb in (1, 2, 4) for h, o in ((0, ""), (1, "_poolonly"))] \
    + [f"x_xblk{xb}_{h}{o}" for xb in (2,) for h, o in ((1, ""), (0, "_poolonly"))]


def parse_layout(layout):
    """layout name -> dict(x_pad, out_pitch2, pool_pad, out_xblk, out_half, x_xblk, x_half, pool_only)"""
    d = dict(x_pad=0, out_pitch2=False, pool_pad=0, out_xblk=0, out_half=0, x_xblk=0, x_half=0, pool_only=False)
    if layout == "x_pitch":
        d["x_pad"] = 4
    elif layout == "out_pitch":
        d["out_pitch2"] = True
    elif layout == "pool_pitch":
        d["pool_pad"] = 8
    elif layout.startswith("out_xblk"):
        d["out_xblk"], d["out_half"] = int(layout[8]), int(layout[10])
    elif layout.startswith("x_xblk"):
        d["x_xblk"], d["x_half"], d["pool_only"] = int(layout[6]), int(layout[8]), layout.endswith("_poolonly")
    else:
        assert layout == "dense", layout
    return d


def norm_cases():
    cases = []
    for inst, (entry, pool, _) in INSTANCES.items():
        layouts = _POOL_LAYOUTS if pool else _COMMON_LAYOUTS
        cs = C_WIDE if inst.startswith("wide") else C_SHUFFLE if pool else C_NOPOOL
        shapes = POOL_SHAPES if pool else NOPOOL_SHAPES
        for k, layout in enumerate(layouts):
            lay = parse_layout(layout)
            shape = shapes[(k + k // 3) % 3]
            xb = max(lay["out_xblk"], lay["x_xblk"])
            if xb and shape[3] % xb:
                shape = XB4_SHAPES[pool]
            act, drop = k % 3, (k // 3) % 3                          # VX_ACT_* / VX_DROP_*: all nine pairs within nine cases
            if drop == 1:
                shape = (3,) + shape[1:]                             # hash dropout: N >= 3, the per-sample key matters
            repeat = (2, 5)[k % 2] if inst == "fanout" else 1
            cases.append(NormCase(inst, cs[k % len(cs)], shape, act, drop, layout, (1, 5, 37)[k % 3], repeat))
    return cases


def norm_case_id(c):
    return f"{c.inst}-C{c.C}-{'x'.join(map(str, c.shape))}-act{c.act}-drop{c.drop}-{c.layout}-t{c.tiles}-r{c.repeat}"


def decode_divisors(pool, wide, c, d, h, w):
    """(PW, C4, RH) the launcher decodes a piece index with, and the pieces per sample"""
    c4 = c // 4
    pw = (w // 2 if wide else w) * c4
    rh = h // 2 if pool else h
    return (pw, c4, rh), (d // 2 if pool else d) * rh * pw


DECODE_LIMIT = dict(C=12, W=341, H=57, D=72)          # PW = 1023, per = 72 * 57 * 1023 = 4 198 392, per * PW = 2^32 - 12 280
# (pool, wide, C, D, H, W) of the launches whose grid-stride loops run more than one trip
TRIP_SHAPES = ((False, False, 8, 2, 3, 50),          # N = 20000: the 16384 / N cap leaves one block for 600 pieces
               (False, False, 16, 1, 1, 70),         # fan-out, ns = 33000: one block for 280 pieces
               (False, False, 8, 3, 7, 30),          # _stats, no pooling: 1260 pieces against (bx + 3) / 4 = 2 blocks
               (True, False, 8, 6, 10, 36),          # _stats, pooling: 1080 pieces (not a multiple of 256) against 2 blocks
               (True, True, 132, 4, 6, 12),          # _stats, wide: 1188 work items against 2 blocks
               (True, False, 16, 2, 6, 10))          # plain pooling, 120 pieces: a partly idle wave beside the shuffle
