"""Inputs whose convolution is exactly representable, and the float64 expectation the conv kernels must hit on them.

The split-fp16 kernels (values_amd/csrc/s16_common.h, conv3d_s16.hip) evaluate a float32 product as

    x = hi + lo * 2^-11,  hi = fp16(x),  lo = fp16((x - hi) * 2048)
    a * b = hi_a hi_b  +  2^-11 (hi_a lo_b + lo_a hi_b)                 (the lo * lo term is dropped, as the scheme documents)

with a main (hi * hi) and a cross accumulator in float32, combined as fmaf(cross, 1 / 2048, main), then the bias.  On dense random
data that can only be compared with a float64 convolution under a tolerance (2e-5 .. 4e-5 in tests/test_gpu_kernels.py), which
is 35 to 70 times the scheme's own error and hides a fault the size of one 16-byte piece.  The generators here pick inputs for
which every product and every partial sum, in ANY order and ANY arrangement of accumulators, is exact in float32:

  lattice      hi in {+-0.5, +-1, +-1.5}, lo in {+-1, +-2, +-3} / 8, value = hi + lo * 2^-11; the hi-lattice has lo = 0.  Weights
               dense, activations non-zero where (channel + 7 * voxel index) % P == 0 with P = ceil(K / 160), K the products per
               output.  Biases are multiples of 0.25 in [-2, 2].  hi * hi is a multiple of 2^-2, hi * lo of 2^-4 (2^-15 once
               scaled by 2^-11); while the sum of the absolute products stays below 2^8 (the sum condition, proven per case by
               tests/test_conv_lattice_cpu.py) every partial sum fits 23 bits.  What is left is the combine and the bias add, one
               rounding each, of values bounded by |M| + |X| / 2048 + |b|; a third rounding is allowed as spare:
                   tol = 3 * 2^-24 * (|M| + |X| / 2048 + |b|)   per element;   on the hi-lattice X = 0 and E is exact: tol = 0.
  impulses     single non-zero voxels on a grid of pitch 4 (plus the last index of every axis: faces, edges, corners), the channel
               cycling with the impulse index, so every output holds at most one product.  Form (a): activations with a full
               11-bit hi and a full 11-bit lo, weights fp16-exact; form (b) the converse.  E = hi * w + lo * w / 2048, both terms
               exact in float32, tol = 2^-23 |E| (one combine rounding and a spare), bias 0.  A lo that is truncated or wrongly
               scaled, which the 2-bit lattice lo cannot see, moves these by 2^-18 |w|.

One departure from the plain draw: hi = +-0.5 with lo = -+3/8 is NOT a fixed point of the split (fp16 spacing below 0.5 is 2^-12, so
fp16(0.5 - 0.375 * 2^-11) = 0.5 - 2^-12); for that pair the sign of lo follows hi.  split(value) == (hi, lo) then holds for every
element, and the CPU test asserts it.

CPU only (numpy / torch); nothing here calls the library."""
import functools
import math
import zlib
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from tests.formula import hash_uniform

HI_SET = np.array([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5])
LO_SET = np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]) / 8.0
SUM_BOUND = 256.0          # the sum condition: sum |hi_x||hi_w| + (sum |hi_x||lo_w| + sum |lo_x||hi_w|) / 2048 + |b| < 2^8
U24 = 2.0 ** -24
UNIT = 2.0 ** -15          # failure reports print got - want in these units: one lo-plane product is a small integer


def split(x):
    """s16_common.h restated: x (float32-representable) -> (hi, lo) as float64 arrays"""
    x = np.asarray(x, dtype=np.float64).astype(np.float32)
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)   # the residual and its scaling are exact in fp32
    return hi.astype(np.float64), lo.astype(np.float64)


def _pick(shape, tag, values):
    n = int(np.prod(shape))
    idx = np.floor((hash_uniform(n, tag) + 1.0) * 0.5 * len(values)).astype(np.int64)
    return values[np.clip(idx, 0, len(values) - 1)].reshape(shape)


def lattice(shape, tag, with_lo=True):
    """(hi, lo) lattice parts, a pure function of (index, tag)"""
    hi = _pick(shape, tag, HI_SET)
    if not with_lo:
        return hi, np.zeros(shape)
    lo = _pick(shape, tag + 7001, LO_SET)
    unstable = (np.abs(hi) == 0.5) & (np.abs(lo) == 0.375) & (np.sign(lo) != np.sign(hi))    # see the module docstring
    lo = np.where(unstable, -lo, lo)
    return hi, lo


def lattice_bias(cout, tag):
    return np.round(hash_uniform(cout, tag) * 8.0) / 4.0


def products_per_output(kind, cin, ks):
    return cin if kind == "convT" else cin * ks ** (2 if kind == "conv2d" else 3)


def sparsity(kind, cin, ks):
    return max(1, math.ceil(products_per_output(kind, cin, ks) / 160))


def activation_mask(shape, P):
    """(N, C, *spatial) -> bool, True where (channel + 7 * voxel index) % P == 0; the voxel index runs over (n, spatial)"""
    n, c = shape[:2]
    nvox = n * int(np.prod(shape[2:]))
    vox = np.arange(nvox, dtype=np.int64).reshape((n, 1) + tuple(shape[2:]))
    ch = np.arange(c, dtype=np.int64).reshape((1, c) + (1,) * (len(shape) - 2))
    return (ch + 7 * vox) % P == 0


def _full11(shape, tag, lo_exp):
    """fp16 values with all 11 significand bits in use (odd last bit), magnitude in [2^lo_exp, 2^(lo_exp + 1)), random sign"""
    n = int(np.prod(shape))
    m = np.floor((hash_uniform(n, tag) + 1.0) * 256.0).astype(np.int64) * 2 + 1            # odd, 1 .. 1023
    s = np.where(hash_uniform(n, tag + 3) < 0, -1.0, 1.0)
    return (s * (1024 + m) / 1024.0 * 2.0 ** lo_exp).reshape(shape)


def impulse_axis(dim):
    """grid of pitch 4 from 0 plus the last index (gaps stay >= 3, so 3-tap footprints never overlap)"""
    p = list(range(0, dim, 4))
    last = dim - 1
    if p[-1] != last:
        if last - p[-1] >= 3:
            p.append(last)
        elif len(p) > 1:
            p[-1] = last
    return p


def impulse_sites(shape):
    """[(n, channel, *coords)] for an (N, C, *spatial) tensor: the channel cycles with the impulse index"""
    n, c = shape[:2]
    axes = [impulse_axis(d) for d in shape[2:]]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, len(axes))
    sites, k = [], 0
    for i in range(n):
        for pos in grid:
            sites.append((i, k % c) + tuple(int(v) for v in pos))
            k += 1
    return sites


def _conv(kind, x, w, ks, stride):
    if kind == "conv3d":
        return F.conv3d(x, w, padding=ks // 2)
    if kind == "conv2d":
        return F.conv2d(x, w, stride=stride, padding=ks // 2)
    return F.conv_transpose3d(x, w, stride=2)


def _bview(b, ndim):
    return b.view((1, -1) + (1,) * (ndim - 2))


def expectation(kind, hi_x, lo_x, hi_w, lo_w, b, ks=3, stride=1, tol_factor=3.0 * U24):
    """float64 (exact) M, X, E and the per-element tolerance, all as torch tensors in the reference's layout"""
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) for a in (hi_x, lo_x, hi_w, lo_w, b)]
    hx, lx, hw, lw, bb = t
    M = _conv(kind, hx, hw, ks, stride)
    X = torch.zeros_like(M)
    if bool((lw != 0).any()):
        X = X + _conv(kind, hx, lw, ks, stride)
    if bool((lx != 0).any()):
        X = X + _conv(kind, lx, hw, ks, stride)
    bv = _bview(bb, M.dim())
    E = M + X / 2048.0 + bv
    tol = tol_factor * (M.abs() + X.abs() / 2048.0 + bv.abs())
    return M, X, E, tol


def abs_sum(kind, hi_x, lo_x, hi_w, lo_w, b, ks=3, stride=1):
    """the left side of the sum condition, per output"""
    t = [torch.from_numpy(np.ascontiguousarray(np.abs(a), dtype=np.float64)) for a in (hi_x, lo_x, hi_w, lo_w, b)]
    hx, lx, hw, lw, bb = t
    s = _conv(kind, hx, hw, ks, stride) + (_conv(kind, hx, lw, ks, stride) + _conv(kind, lx, hw, ks, stride)) / 2048.0
    return s + _bview(bb, s.dim())


def _tag(*key):
    return zlib.crc32(repr(key).encode()) & 0xFFFFF


def weight_shape(kind, cin, cout, ks):
    if kind == "convT":
        return (cin, cout, 2, 2, 2)
    return (cout, cin) + (ks,) * (2 if kind == "conv2d" else 3)


@functools.lru_cache(maxsize=6)
def make_case(kind, cin, cout, shape, flavour, ks=3, stride=1, bias=True):
    """kind: 'conv3d' | 'conv2d' | 'convT'; shape: (N, *spatial); flavour: 'hi' | 'lo' | 'imp_a' | 'imp_b'.
    Returns a namespace: x, w, b (float64 torch tensors, every value float32-representable), their parts hi_x, lo_x, hi_w, lo_w
    (numpy), M, X, E, tol, and for the impulse flavours the list of sites."""
    tag = _tag(kind, cin, cout, tuple(shape), ks, stride)
    xs = (shape[0], cin) + tuple(shape[1:])
    ws = weight_shape(kind, cin, cout, ks)
    c = SimpleNamespace(kind=kind, cin=cin, cout=cout, shape=tuple(shape), flavour=flavour, ks=ks, stride=stride, sites=None)
    if flavour in ("hi", "lo"):
        with_lo = flavour == "lo"
        c.P = sparsity(kind, cin, ks)
        hx, lx = lattice(xs, tag, with_lo)
        keep = activation_mask(xs, c.P)
        hx, lx = hx * keep, lx * keep
        hw, lw = lattice(ws, tag + 1, with_lo)
        b = lattice_bias(cout, tag + 2) if bias else np.zeros(cout)
        factor = 3.0 * U24
    else:
        c.P = None
        c.sites = impulse_sites(xs)
        full_h, full_l = _full11(xs, tag + 11, 0), _full11(xs, tag + 12, -1)        # |hi| in [1, 2), |lo| in [0.5, 1): |lo| 2^-11 < ulp / 2
        exact = _full11(xs, tag + 13, -1)
        sel = np.zeros(xs, dtype=bool)
        for s in c.sites:
            sel[s] = True
        if flavour == "imp_a":
            hx, lx = full_h * sel, full_l * sel
            hw, lw = _full11(ws, tag + 14, -1), np.zeros(ws)
        else:
            hx, lx = exact * sel, np.zeros(xs)
            hw, lw = _full11(ws, tag + 15, 0), _full11(ws, tag + 16, -1)
        b = np.zeros(cout)
        factor = 2.0 * U24
    c.hi_x, c.lo_x, c.hi_w, c.lo_w = hx, lx, hw, lw
    c.x = torch.from_numpy(hx + lx / 2048.0)
    c.w = torch.from_numpy(hw + lw / 2048.0)
    c.b = torch.from_numpy(b)
    c.M, c.X, c.E, c.tol = expectation(kind, hx, lx, hw, lw, b, ks, stride, factor)
    if flavour in ("imp_a", "imp_b"):
        c.tol = factor * c.E.abs()
    return c


# ---- failure report -----------------------------------------------------------------------------------------------------------
def border_class(coords, dims):
    """which faces an output voxel touches, e.g. 'z0 xN' or 'interior'"""
    names = "zyx"[-len(dims):]
    t = []
    for a, (p, d) in enumerate(zip(coords, dims)):
        if p == 0:
            t.append(names[a] + "0")
        if p == d - 1:
            t.append(names[a] + "N")
    return " ".join(t) if t else "interior"


def _impulse_source(case, idx):
    """(tap, channel) of the one product behind output idx = (n, cout, *coords) of an impulse case, or None"""
    n, coords = idx[0], idx[2:]
    for s in case.sites:
        if s[0] != n:
            continue
        if case.kind == "convT":
            if all(o // 2 == p for o, p in zip(coords, s[2:])):
                return tuple(o % 2 for o in coords), s[1]
        else:
            tap = tuple(p - o * case.stride + case.ks // 2 for o, p in zip(coords, s[2:]))
            if all(0 <= t < case.ks for t in tap):
                return tap, s[1]
    return None


def report(got, want, tol, case=None, limit=8):
    """'' when |got - want| <= tol everywhere, else the first failing outputs: (n, cout, z, y, x), border class, got - want in units
    of 2^-15, and for impulse cases the tap and channel of the product"""
    got, want = got.double(), want.double()
    bad = ((got - want).abs() > tol) | torch.isnan(got)
    nbad = int(bad.sum())
    if nbad == 0:
        return ""
    lines = ["%d of %d outputs differ; worst %.3g (%.1f units of 2^-15)" % (
        nbad, bad.numel(), float((got - want).abs().max()), float((got - want).abs().max()) / UNIT)]
    for idx in bad.nonzero()[:limit].tolist():
        idx = tuple(idx)
        line = "  %s [%s] got %.9g want %.9g diff %+.3f units" % (
            idx, border_class(idx[2:], want.shape[2:]), float(got[idx]), float(want[idx]), float(got[idx] - want[idx]) / UNIT)
        if case is not None and case.sites is not None:
            src = _impulse_source(case, idx)
            if src is not None:
                line += " tap %s channel %d" % src
        lines.append(line)
    return "\n".join(lines)


def check(got, want, tol, case=None):
    msg = report(got, want, tol, case)
    assert not msg, msg


def check_equal(got, want, case=None):
    """bit equality with a float32-representable expectation"""
    check(got, want, torch.zeros_like(want), case)


# ---- emulated faults (float64), for the teeth of the CPU test ---------------------------------------------------------------------
def taps(kind, ks):
    nd = 2 if kind == "conv2d" else 3
    k = 2 if kind == "convT" else ks
    return [tuple(int(v) for v in t) for t in np.ndindex(*(k,) * nd)]


def _tap_view(case, xpad, tap, out_sp):
    """the activations tap `tap` multiplies, aligned with the outputs: (N, C, *out spatial)"""
    sl = [slice(None), slice(None)]
    for t, o in zip(tap, out_sp):
        sl.append(slice(t, t + case.stride * (o - 1) + 1, case.stride))
    return xpad[tuple(sl)]


def piece_fault_ratios(case):
    """the weights' lo dropped for ONE (channel octet, tap) piece: for every piece, the largest |error| / tol over the outputs
    (inf where an output with tol == 0 moves).  Returns {(octet, tap): ratio}."""
    hx = torch.from_numpy(case.hi_x)
    lw = torch.from_numpy(case.lo_w)
    out = {}
    nd = hx.dim() - 2
    if case.kind != "convT":
        p = case.ks // 2
        xpad = F.pad(hx, (p, p) * nd)
    for tap in taps(case.kind, case.ks):
        for o in range((case.cin + 7) // 8):
            cs = slice(8 * o, min(8 * o + 8, case.cin))
            if case.kind == "convT":
                d = torch.zeros_like(case.E)
                sl = (slice(None), slice(None)) + tuple(slice(t, None, 2) for t in tap)
                d[sl] = torch.einsum("nc...,ck->nk...", hx[:, cs], lw[(cs, slice(None)) + tap])
            else:
                d = torch.einsum("nc...,kc->nk...", _tap_view(case, xpad, tap, case.E.shape[2:])[:, cs], lw[(slice(None), cs) + tap])
            out[(o, tap)] = _ratio(d / 2048.0, case.tol)
    return out


def _ratio(err, tol):
    err = err.abs()
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max())


def border_plane_fault_ratio(case, axis=-1, index=0):
    """the activations' lo zeroed on one border plane (default x = 0)"""
    lx = np.zeros_like(case.lo_x)
    sl = [slice(None)] * lx.ndim
    sl[axis] = index
    lx[tuple(sl)] = case.lo_x[tuple(sl)]
    d = _conv(case.kind, torch.from_numpy(lx), torch.from_numpy(case.hi_w), case.ks, case.stride) / 2048.0
    return _ratio(d, case.tol)


def tap_swap_fault_ratio(case, a=None, b=None):
    """two taps of the weights swapped"""
    tp = taps(case.kind, case.ks)
    a, b = tp[0] if a is None else a, tp[len(tp) // 2 + 1] if b is None else b
    hw, lw = case.hi_w.copy(), case.lo_w.copy()
    for w in (hw, lw):
        ia, ib = (slice(None), slice(None)) + a, (slice(None), slice(None)) + b
        tmp = w[ia].copy()
        w[ia] = w[ib]
        w[ib] = tmp
    _, _, E, _ = expectation(case.kind, case.hi_x, case.lo_x, hw, lw, case.b.numpy(), case.ks, case.stride)
    return _ratio(E - case.E, case.tol)


def lo_rounded_fault_ratio(case, bits=5):
    """impulse cases: the full lo (of whichever operand carries one) rounded to `bits` significand bits"""
    def rnd(v):
        m, e = np.frexp(v)
        return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)
    _, _, E, _ = expectation(case.kind, case.hi_x, rnd(case.lo_x), case.hi_w, rnd(case.lo_w), case.b.numpy(), case.ks, case.stride)
    return _ratio(E - case.E, case.tol)


# ---- the case matrix (shared by tests/test_conv_lattice_cpu.py and tests/test_gpu_conv_lattice.py) ---------------------------------
# The smallest shapes that still reach every staging path, border class and tile form of each kernel family.
# conv3d: (id, family, vx_config fields, Cin, Cout, (N, D, H, W), launch keywords,
#          kernel-name prefix of a launch without statistics, kernel-name prefix of a statistics launch or None where the family has
#          no statistics instance for the shape and the tile kernel takes the launch)
_S16 = "conv3d_k3_s16_kernel<"
CONV3D_CASES = [
    # the split-fp16 tile kernel (conv3d_s16.hip): x-pair ragged, two chunks ragged, three chunks of 8, plain ragged, H >= 32, two
    # row tiles per wave, the x-blocked concat input (staggered double-buffered instance), an input pitch wider than Cin
    ("s16-xp-ragged", "s16", {}, 8, 8, (1, 6, 10, 20), {}, _S16 + "8,1,8,8,4,8,1,", _S16 + "8,1,8,8,4,8,1,"),
    ("s16-xp-2chunk", "s16", {}, 16, 8, (1, 5, 7, 38), {}, _S16 + "8,1,16,4,4,8,1,", _S16 + "8,1,16,4,4,8,1,"),
    ("s16-cb8", "s16", {}, 24, 8, (1, 4, 8, 16), {}, _S16 + "8,1,8,8,4,8,1,", _S16 + "8,1,8,8,4,8,1,"),
    ("s16-small", "s16", {}, 16, 16, (1, 3, 5, 9), {}, _S16 + "16,1,8,8,4,8,0,", _S16 + "16,1,8,8,4,8,0,"),
    ("s16-h40", "s16", {}, 32, 32, (1, 4, 40, 16), {}, _S16 + "16,2,16,4,4,8,0,", _S16 + "16,2,16,4,4,8,0,"),
    ("s16-nt2", "s16", dict(s16_no_deep=1), 64, 128, (4, 4, 4, 4), {}, _S16 + "16,2,4,4,4,4,0,", _S16 + "16,2,4,4,4,4,0,"),
    ("s16-xblk4", "s16", {}, 16, 16, (1, 4, 8, 16), dict(xblk=4), _S16 + "16,1,16,4,4,8,0,2,", _S16 + "16,1,16,4,4,8,0,2,"),
    ("s16-pitch", "s16", {}, 16, 8, (1, 5, 7, 38), dict(in_pitch=24), _S16 + "8,1,16,4,4,8,1,", _S16 + "8,1,16,4,4,8,1,"),
    # the tile kernel on the shapes the column kernels take by default (vx_config knobs)
    ("s16-no-xp8", "s16", dict(s16_no_xp8=1), 8, 8, (2, 8, 8, 32), {}, _S16 + "8,1,16,4,4,8,1,", _S16 + "8,1,16,4,4,8,1,"),
    ("s16-no-zc16", "s16", dict(s16_no_zc16=1), 16, 16, (2, 4, 8, 32), {}, _S16 + "16,1,16,4,4,8,0,2,", _S16 + "16,1,16,4,4,8,0,2,"),
    # the z-column kernel of the Cout = 8 layers (conv3d_xp8w.hip): one and two chunks, the x-blocked concat input
    ("xp8w-8", "xp8w", {}, 8, 8, (2, 8, 8, 32), {}, "conv3d_xp8w_kernel<1,", "conv3d_xp8w_kernel<1,0,"),
    ("xp8w-16", "xp8w", {}, 16, 8, (1, 8, 16, 64), {}, "conv3d_xp8w_kernel<2,", None),
    ("xp8w-16-xblk", "xp8w", {}, 16, 8, (1, 8, 16, 64), dict(xblk=4), "conv3d_xp8w_kernel<2,", None),
    # the z-column kernel of the Cout = 16 layers (conv3d_zc16.hip); W = 96: an interior column tile
    ("zc16-8", "zc16", {}, 8, 16, (2, 4, 8, 32), {}, "conv3d_zc16_kernel<8,", "conv3d_zc16_kernel<8,0,"),
    ("zc16-16", "zc16", {}, 16, 16, (2, 4, 8, 32), {}, "conv3d_zc16_kernel<16,", "conv3d_zc16_kernel<16,0,"),
    ("zc16-8-w96", "zc16", {}, 8, 16, (1, 4, 8, 96), {}, "conv3d_zc16_kernel<8,", "conv3d_zc16_kernel<8,0,"),
    ("zc16-16-w96", "zc16", {}, 16, 16, (1, 4, 8, 96), {}, "conv3d_zc16_kernel<16,", "conv3d_zc16_kernel<16,0,"),
    # the deep kernel (conv3d_deep.hip): R = 4 and R = 2 tiles, four 4^3 samples per tile, D % 4 == 2, an x-blocked concat input
    ("deep-16-32", "deep", {}, 16, 32, (1, 8, 8, 16), {}, "conv3d_deep_kernel<4,", "conv3d_deep_kernel<4,0,"),
    ("deep-32-32", "deep", {}, 32, 32, (2, 16, 16, 16), {}, "conv3d_deep_kernel<4,", "conv3d_deep_kernel<4,0,"),
    ("deep-64-64", "deep", {}, 64, 64, (4, 8, 8, 8), {}, "conv3d_deep_kernel<4,", "conv3d_deep_kernel<4,0,"),
    ("deep-128-128", "deep", {}, 128, 128, (4, 4, 4, 4), {}, "conv3d_deep_kernel<2,", None),
    ("deep-32-64", "deep", {}, 32, 64, (1, 6, 8, 16), {}, "conv3d_deep_kernel<2,", None),
    ("deep-xblk", "deep", {}, 32, 32, (1, 8, 8, 16), dict(xblk=4), "conv3d_deep_kernel<4,", "conv3d_deep_kernel<4,0,"),
]
# the native-fp32 kernels (vx_config.conv_fp32 = 1): the 4x4x1 register-tile kernel and the fp32 matrix-instruction tile kernel.
# Their products of lo-carrying values are not exact: hi-lattice and impulse form (a) only.
CONV3D_FP32_CASES = [
    ("c8-8", "fp32", dict(conv_fp32=1), 8, 8, (1, 6, 10, 20), {}, "conv3d_k3_c8_kernel<1,", "conv3d_k3_c8_kernel<1,"),
    ("c8-16", "fp32", dict(conv_fp32=1), 16, 8, (1, 5, 7, 38), {}, "conv3d_k3_c8_kernel<2,", "conv3d_k3_c8_kernel<2,"),
    ("mfma-16-16", "fp32", dict(conv_fp32=1), 16, 16, (1, 3, 5, 9), {}, "conv3d_k3_mfma_kernel<16,1,", "conv3d_k3_mfma_kernel<16,1,"),
    ("mfma-32-64", "fp32", dict(conv_fp32=1), 32, 64, (1, 6, 8, 16), {}, "conv3d_k3_mfma_kernel<16,2,", "conv3d_k3_mfma_kernel<16,2,"),
]
# ids of the cases that also carry the exact epilogues (ReLU, hash dropout, mask dropout where the family takes a mask) and the
# impulse forms: one per family (two for the tile kernel: x-pair and plain packing)
EPILOGUE_IDS = ("s16-xp-ragged", "xp8w-8", "zc16-16", "deep-32-32", "c8-8", "mfma-16-16")
IMPULSE_IDS = ("s16-xp-ragged", "s16-small", "xp8w-8", "zc16-16", "deep-32-32", "c8-8", "mfma-16-16")
# vx_conv3d_k3_c1 (one input channel, fp32 FMAs): (Cout, (V, D, H, W), flip code of the odd output samples)
C1_CASES = [(8, (2, 6, 10, 40), 5), (16, (1, 4, 8, 16), 0)]
# vx_convT_k2s2: (Cin, Cout, (N, D, H, W), kernel-name prefix by conv mode); Cin 16 / 32 run the fp32 matrix instruction in both modes
CONVT_CASES = [
    (16, 8, (4, 4, 4, 4), {"split16": "convT_k2s2_mfma_kernel<16,", "fp32": "convT_k2s2_mfma_kernel<16,"}),
    (32, 16, (4, 4, 4, 4), {"split16": "convT_k2s2_mfma_kernel<32,", "fp32": "convT_k2s2_mfma_kernel<32,"}),
    (64, 32, (4, 4, 4, 4), {"split16": "convT_k2s2_s16_kernel<64,", "fp32": "convT_k2s2_mfma_kernel<64,"}),
    (128, 64, (4, 4, 4, 4), {"split16": "convT_k2s2_s16_kernel<128,", "fp32": "convT_k2s2_mfma_kernel<128,"}),
]
# vx_conv2d: (Cin, Cout, KS, S, (N, H, W), narrow input pitch)
CONV2D_CASES = [
    (16, 16, 3, 1, (2, 16, 16), False), (18, 18, 3, 1, (1, 9, 17), True),
    (3, 64, 3, 2, (1, 32, 48), False), (48, 96, 3, 2, (1, 17, 31), False),
    (256, 64, 1, 1, (1, 16, 24), False), (240, 4, 1, 1, (1, 16, 24), False),
]
CONV2D_IMPULSE = (16, 16, 3, 1, (2, 16, 16), False)
CONVT_IMPULSE = {"split16": (64, 32, (4, 4, 4, 4)), "fp32": (32, 16, (4, 4, 4, 4))}


def all_lattice_keys():
    """(kind, cin, cout, shape, ks, stride) of every lattice case of the GPU matrix, once each"""
    keys = []
    for c in CONV3D_CASES + CONV3D_FP32_CASES:
        keys.append(("conv3d", c[3], c[4], c[5], 3, 1))
    keys += [("conv3d", 1, co, sh, 3, 1) for co, sh, _ in C1_CASES]
    keys += [("convT", ci, co, sh, 2, 2) for ci, co, sh, _ in CONVT_CASES]
    keys += [("conv2d", ci, co, sh, ks, s) for ci, co, ks, s, sh, _ in CONV2D_CASES]
    return list(dict.fromkeys(keys))


def all_impulse_keys():
    by_id = {c[0]: c for c in CONV3D_CASES + CONV3D_FP32_CASES}
    keys = [("conv3d", by_id[i][3], by_id[i][4], by_id[i][5], 3, 1) for i in IMPULSE_IDS]
    keys.append(("conv3d", 1, C1_CASES[0][0], C1_CASES[0][1], 3, 1))
    keys += [("convT", ci, co, sh, 2, 2) for ci, co, sh in CONVT_IMPULSE.values()]
    ci, co, ks, s, sh, _ = CONV2D_IMPULSE
    keys.append(("conv2d", ci, co, sh, ks, s))
    return list(dict.fromkeys(keys))


def case_from_key(key, flavour):
    kind, cin, cout, shape, ks, stride = key
    return make_case(kind, cin, cout, tuple(shape), flavour, ks, stride)


# ---- composed launches on the hi-lattice ----------------------------------------------------------------------------------------------
# With lo = 0 everywhere only the main accumulator is used: a product of a 2^-2 multiple (an intermediate result) and a 2^-1 multiple
# (a lattice weight) is a multiple of 2^-3, and every partial sum is exact in float32 while the sum of absolute products stays below
# 2^20 (HI_ONLY_BOUND; 24 bits above 2^-4).  Intermediate results must also be fp16-exact: multiples of 2^-2 below 2^9.
HI_ONLY_BOUND = 2.0 ** 20
# zc16 planar hand-over (producer with out_planar, consumer with in_planar), both 16 -> 16 with a ReLU
PLANAR_SHAPES = [(2, 4, 8, 32), (1, 4, 8, 96)]
# fused up-convolution: xp8w (coarse 16 -> up 8, + skip 8 -> 8), ((N, D, H, W), x-blocking of the skip input); zc16 (coarse 32 -> up 16 -> 16)
UPFUSE_XP8W = [((2, 8, 8, 32), 0), ((1, 8, 16, 64), 4)]
UPFUSE_ZC16 = [(2, 8, 16, 32), (1, 4, 24, 64)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


@functools.lru_cache(maxsize=2)
def planar_case(shape):
    """x -> ReLU(conv1) -> ReLU(conv2), hi-lattice throughout.  .bound: the largest sum of absolute products + |bias| of either conv"""
    first = make_case("conv3d", 16, 16, tuple(shape), "hi", 3, 1)
    tag = _tag("planar", tuple(shape))
    w2, b2 = lattice((16, 16, 3, 3, 3), tag, False)[0], lattice_bias(16, tag + 1)
    y = torch.relu(first.E)
    E2 = F.conv3d(y, _t(w2), _t(b2), padding=1)
    bound2 = F.conv3d(y, _t(np.abs(w2)), _t(np.abs(b2)), padding=1).max()
    return SimpleNamespace(first=first, y=y, w2=_t(w2), b2=_t(b2), E2=E2, bound=float(bound2))


@functools.lru_cache(maxsize=2)
def upfused_case(shape, ccoarse, cup, cskip, cout):
    """coarse -> ConvTranspose3d(k = 2, s = 2) -> cat([up, skip]) -> conv 3x3x3 + bias, hi-lattice throughout (cskip may be 0)"""
    n, d, h, w = shape
    tag = _tag("upfused", tuple(shape), ccoarse, cup, cskip, cout)
    coarse = lattice((n, ccoarse, d // 2, h // 2, w // 2), tag, False)[0]
    uw, ub = lattice((ccoarse, cup, 2, 2, 2), tag + 1, False)[0], lattice_bias(cup, tag + 2)
    skip = lattice((n, cskip, d, h, w), tag + 3, False)[0] if cskip else None
    wt, b = lattice((cout, cup + cskip, 3, 3, 3), tag + 4, False)[0], lattice_bias(cout, tag + 5)
    up = F.conv_transpose3d(_t(coarse), _t(uw), _t(ub), stride=2)
    up_bound = F.conv_transpose3d(_t(np.abs(coarse)), _t(np.abs(uw)), _t(np.abs(ub)), stride=2).max()
    xin = torch.cat([up, _t(skip)], 1) if cskip else up
    E = F.conv3d(xin, _t(wt), _t(b), padding=1)
    bound = F.conv3d(xin.abs(), _t(np.abs(wt)), _t(np.abs(b)), padding=1).max()
    return SimpleNamespace(coarse=_t(coarse), uw=_t(uw), ub=_t(ub), skip=None if skip is None else _t(skip), w=_t(wt), b=_t(b), up=up,
                           E=E, bound=float(max(bound, up_bound)))


def stats_exact(E):
    """(sum column exact, sum-of-squares column exact): sum |E| < 2^22 and sum E^2 < 2^20 per (n, c) -- then every fp32 partial, in any
    order, is exact (E is a multiple of 2^-2, E^2 of 2^-4)"""
    red = tuple(range(2, E.dim()))
    return bool((E.abs().sum(red) < 2.0 ** 22).all()), bool(((E * E).sum(red) < 2.0 ** 20).all())
