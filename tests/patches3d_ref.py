"""Plain numpy restatements, float64 or int64 throughout, of the three batched kernels of the 3D test split (patches3d.hip:
vx_gather_patches_3d, vx_softmax_accumulate_cases, vx_case_composite) and of the per-image accumulate they grew from
(accumulate.hip: vx_softmax_accumulate), with the inputs and the placement cases tests/test_gpu_patches3d_matrix.py runs.
tests/test_patches3d_ref_cpu.py holds this file to the reference's fixtures and to compose_case without a GPU."""
import numpy as np

IMAGE_DTYPES = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "float32", "float64")
LABEL_DTYPES = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64")
PATCHES = ((3, 5, 7), (2, 3, 9), (5, 2, 6), (1, 1, 1), (4, 4, 4))
PREFILL_SUM, PREFILL_COUNT = 5.0, 2.0          # what the destinations hold before a placement run: tells += from =


# ---------------------------------------------------------------------------------------------------------------------
# gather

def gather_ref(vol, origin, P):
    """the crop [origin, origin + P) of vol as numpy's astype(float32) converts it"""
    sl = tuple(slice(int(o), int(o) + int(p)) for o, p in zip(origin, P))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(vol)[sl].astype(np.float32)


def gather_specials(dtype):
    """the values whose conversion to float32 can go wrong, per stored dtype (others: none)"""
    dtype = np.dtype(dtype)
    if dtype == np.float64:      # float32 denormal range, a tie at the bottom of it, beyond the float32 maximum, ties of the rounding
        return np.array([1e-40, 2.0 ** -150, 1.5 * 2.0 ** -149, 1e39, -1e39, 0.0, -0.0, np.nan, np.inf, -np.inf,
                         1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -(1 + 2.0 ** -24)], dtype=dtype)
    if dtype == np.float32:
        return np.array([1e-40, -1e-40, 2.0 ** -149, 0.0, -0.0, np.nan], dtype=dtype)
    if dtype == np.uint32:       # 2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4, 2^32 - 1 -> 2^32
        return np.array([2 ** 24 + 1, 2 ** 24 + 3, 2 ** 32 - 1], dtype=dtype)
    if dtype == np.int32:
        return np.array([2 ** 31 - 1, -2 ** 31, -(2 ** 24 + 1), 2 ** 24 + 3], dtype=dtype)
    return np.zeros(0, dtype=dtype)


def random_volume(rng, shape, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return (rng.standard_normal(shape) * 1e3 / 3).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)


# ---------------------------------------------------------------------------------------------------------------------
# accumulate

def accumulate_ref(logits, origins, dims, T, C, image=None, decode=None):
    """DataCarrier3D.concat_data for a batch of patches, in float64: logits (B, T, C, P0, P1, P2); patch b adds the class
    softmax of logits[b] (float64, running maximum) into image image[b] (default 0) at origins[b], in patch order; voxels
    outside the image are skipped.  dims: one (X, Y, Z) -> (sum (T, C, X, Y, Z) float64, count (X, Y, Z) int64), or a list
    of them -> (list of sums, list of counts).  decode "01" / "12" reads a patch's memory as a kernel with (P0, P1) /
    (P1, P2) swapped in its index decode would: the CPU tests use it to prove a case can see such a kernel."""
    logits = np.asarray(logits, dtype=np.float64)
    B, P = logits.shape[0], tuple(logits.shape[3:])
    assert logits.shape[1:3] == (T, C) and len(P) == 3
    single = isinstance(dims[0], (int, np.integer))
    dl = [tuple(int(v) for v in dims)] if single else [tuple(int(v) for v in d) for d in dims]
    image = [0] * B if image is None else [int(i) for i in image]
    sums = [np.zeros((T, C) + d, dtype=np.float64) for d in dl]
    counts = [np.zeros(d, dtype=np.int64) for d in dl]
    for b in range(B):
        lg = logits[b]
        if decode == "01":
            lg = lg.reshape(T, C, P[1], P[0], P[2]).transpose(0, 1, 3, 2, 4)
        elif decode == "12":
            lg = lg.reshape(T, C, P[0], P[2], P[1]).transpose(0, 1, 2, 4, 3)
        else:
            assert decode is None
        e = np.exp(lg - lg.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        d, o = dl[image[b]], [int(v) for v in origins[b]]
        n = [max(0, min(P[a], d[a] - o[a])) for a in range(3)]
        dst = tuple(slice(o[a], o[a] + n[a]) for a in range(3))
        sums[image[b]][(slice(None), slice(None)) + dst] += p[:, :, :n[0], :n[1], :n[2]]
        counts[image[b]][dst] += 1
    return (sums[0], counts[0]) if single else (sums, counts)


def softmax_f32(lg, axis):
    """the kernels' expressions in float32 numpy: running maximum, exp, den added class by class from 0, ONE reciprocal,
    e * inv"""
    l = np.moveaxis(np.asarray(lg, dtype=np.float32), axis, 0)
    with np.errstate(under="ignore"):
        m = l[0]
        for c in range(1, l.shape[0]):
            m = np.maximum(m, l[c])
        e = [np.exp(l[c] - m) for c in range(l.shape[0])]
        den = np.zeros_like(m)
        for c in range(l.shape[0]):
            den = den + e[c]
        inv = np.float32(1) / den
        p = np.stack([e[c] * inv for c in range(l.shape[0])])
    assert p.dtype == np.float32
    return np.moveaxis(p, 0, axis)


def accumulate_f32(logits, origins, dims, image=None):
    """accumulate_ref's placement with softmax_f32 addends added in float32, in patch order: what a kernel without
    atomics computes, up to its expf"""
    logits = np.asarray(logits, dtype=np.float32)
    B, T, C = logits.shape[:3]
    P = tuple(logits.shape[3:])
    single = isinstance(dims[0], (int, np.integer))
    dl = [tuple(dims)] if single else [tuple(d) for d in dims]
    image = [0] * B if image is None else list(image)
    sums = [np.zeros((T, C) + d, dtype=np.float32) for d in dl]
    for b in range(B):
        p = softmax_f32(logits[b], 1)
        d, o = dl[image[b]], origins[b]
        n = [max(0, min(P[a], d[a] - o[a])) for a in range(3)]
        dst = (slice(None), slice(None)) + tuple(slice(o[a], o[a] + n[a]) for a in range(3))
        sums[image[b]][dst] = sums[image[b]][dst] + p[:, :, :n[0], :n[1], :n[2]]
    return sums[0] if single else sums


def hot_class(B, T, C, P):
    """the hot class at patch-local (i, j, k) of sample t of patch b.  The linear part alone is, at C = 2, the parity of
    i + j + k + t + b, and the parity of a row's index P1 i + j is that of i + j when P1 is odd: a kernel that swapped two
    ODD extents in its decode would pass (3, 5, 7) at C = 2.  The products i j + j k are there so that every placement case
    sees both swaps (test_placement_cases_can_see_a_transposed_decode)."""
    b, t, i, j, k = np.ogrid[:B, :T, :P[0], :P[1], :P[2]]
    return (3 * i + 5 * j + 7 * k + 11 * t + 13 * b + i * j + j * k) % C


def hot_logits(B, T, C, P):
    """(B, T, C, P0, P1, P2) float32: 0.0 at class hot_class of patch-local (i, j, k), -200.0 elsewhere.  expf(-200) == 0
    in float32, so den == 1, inv == 1 and the softmax is exactly one-hot: the sums are small integers, and float adds of
    integers below 2^24 are exact in any order.  (In float64 exp(-200) is 1.4e-87: accumulate_ref's sums round to those
    integers when cast to float32.)"""
    h = hot_class(B, T, C, P)
    out = np.full((B, T, C) + tuple(P), -200.0, dtype=np.float32)
    out[np.arange(C).reshape(1, 1, C, 1, 1, 1) == h[:, :, None]] = 0.0
    return out


def numeric_logits(B, T, C, P, seed):
    """random float32 logits of scale 3 with patch rows of equal logits and rows where one class stands +-80 and +-100
    off the others (exp of the gap: a float32 denormal at -100, far below it at -200 between the two)"""
    rng = np.random.default_rng(seed)
    lg = (rng.standard_normal((B, T, C) + tuple(P)) * 3).astype(np.float32)
    lg[0, :, :, 0, 0, :] = np.float32(1.5)
    lg[0, :, 0, 0, 1, :] += np.float32(80)
    lg[0, :, C - 1, 0, 2, :] -= np.float32(80)
    lg[1, :, 0, 1, 0, :] += np.float32(100)
    lg[1, :, C - 1, 1, 1, :] -= np.float32(100)
    lg[2, :, 0, 2, 0, :] += np.float32(100)
    lg[2, :, C - 1, 2, 0, :] -= np.float32(100)
    return lg


def numeric_bound(count, C):
    """n (C + 4) 2^-23 + (n - 1) n 2^-24 per voxel, n its count (the derivation: test_accumulate_numeric's docstring)"""
    n = np.asarray(count, dtype=np.float64)
    return n * (C + 4) * 2.0 ** -23 + (n - 1) * n * 2.0 ** -24


def _z_row(P2):
    """four z origins of disjoint crops with phases 0, 1, 2, 3 mod 4, then the origin and the image size Z (odd) of a fifth
    that reaches P2 - P2 // 2 voxels past the image (P2 == 1: it lies wholly outside)"""
    zs = [0]
    for k in range(1, 4):
        z = zs[-1] + P2
        while z % 4 != k:
            z += 1
        zs.append(z)
    h = P2 // 2
    z = zs[-1] + P2
    while (z + h) % 2 == 0:
        z += 1
    return zs, z, z + h


def placement(P, overlap, multi):
    """-> (dims [(X, Y, Z)], patches [(image, origin)]).  Image 0, odd z pitch: four crops along z whose origins take every
    phase mod 4, and one crop per axis that reaches past the image on that axis only -- all disjoint; with `overlap` also
    a 2 x 2 x 3 lattice of crops one voxel apart (count 12 where they all meet).  multi: two more images of other sizes
    with two disjoint crops each (one of them three times over with `overlap`), the patches of the three interleaved."""
    P0, P1, P2 = P
    zs, z_over, Z = _z_row(P2)
    dims = [(P0 + P0 // 2, P1 + P1 // 2, Z)]
    per = [[(0, 0, z) for z in zs] + [(0, 0, z_over), (P0, 0, 0), (0, P1, 0)]]
    if overlap:
        s = [min(1, p - 1) for p in P]
        per[0] += [(a * s[0], b * s[1], 1 + c * s[2]) for a in range(2) for b in range(2) for c in range(3)]
    if multi:
        dims += [(P0 + 1, P1 + 2, 2 * P2 + 5), (P0 + 2, P1, 2 * P2 + 1)]
        per += [[(1, 2, 2), (0, 0, P2 + 3)] + ([(1, 2, 2)] * 2 if overlap else []), [(2, 0, 0), (0, 0, P2 + 1)]]
    patches, k = [], 0
    while any(k < len(p) for p in per):
        patches += [(i, p[k]) for i, p in enumerate(per) if k < len(p)]
        k += 1
    return dims, patches


def placement_T(P):
    return 1 if P in ((2, 3, 9), (1, 1, 1)) else 3


def placement_patches(C):
    """every C meets (3, 5, 7) and (2, 3, 9); every patch meets C = 2, 5, 8"""
    return PATCHES if C in (2, 5, 8) else PATCHES[:2]


# ---------------------------------------------------------------------------------------------------------------------
# composite

def composite_ref(image, labels, count):
    """What compose_case computes, from an arbitrary integer count map instead of a crop list: data (float64: float64(image)
    added count times to 0, divided by max(count, 1)), gt_seg (R, ...) (float64: the intc sum of count additions of
    astype(intc) of the label, WRAPPING as intc does, divided the same way), gt = intc(gt_seg), and n_bad: the number of
    (rater, voxel) pairs whose stored label is outside 0..255 -- every voxel, those under count 0 too, and by the STORED
    value (int64 2^32 + 7 is bad although astype(intc) gives 7)."""
    count = np.asarray(count).astype(np.int64)
    clip = np.maximum(count, 1).astype(np.float64)
    out = {"n_bad": 0}
    with np.errstate(invalid="ignore", over="ignore"):
        if image is not None:
            img = np.asarray(image).astype(np.float64)
            data = np.zeros(count.shape, dtype=np.float64)
            for k in range(int(count.max()) if count.size else 0):
                data = np.where(count > k, data + img, data)
            out["data"] = data / clip
    labels = [np.asarray(l) for l in labels]
    seg = np.zeros((len(labels),) + count.shape, dtype=np.float64)
    for r, l in enumerate(labels):
        assert l.dtype.kind in "iub" and l.shape == count.shape
        lab = l.astype(np.intc).astype(np.int64)
        s = lab * count                                            # |.| < 2^31 * 2^31: exact in int64
        s = ((s + 2 ** 31) % 2 ** 32) - 2 ** 31                    # what count wrapping intc additions leave
        seg[r] = s.astype(np.float64) / clip
        bad = (l > 255) if l.dtype.kind in "ub" else ((l < 0) | (l > 255))
        out["n_bad"] += int(bad.sum())
    out["gt_seg"] = seg
    out["gt"] = seg.astype(np.intc)
    return out


def count_map_of(shape, crops):
    cnt = np.zeros(shape, dtype=np.int64)
    for c in crops:
        cnt[tuple(slice(a, b) for a, b in c)] += 1
    return cnt
