"""Test infrastructure, not product code: the map -> scalar aggregations as include/values_amd.h documents them for
vx_aggregate_batched (K38), restated on the host with numpy, one float64 operation at a time.  The GPU tests compare the
library's result dicts with these using `==`; tests/test_aggregate_batched_cpu.py checks them against
oracle/aggregation_oracle.py and checks that the wide-range inputs below can tell one summation order from another."""
import numpy as np

_KINDS = ("patch_level_aggregation", "image_level_aggregation", "threshold_aggregation")


def as_map(image):
    """the array the device sees: float64 stays float64, anything else becomes float32"""
    if not isinstance(image, np.ndarray):
        import torch
        image = image.detach().cpu()
        image = image.numpy() if image.dtype == torch.float64 else image.float().numpy()
    return image if image.dtype == np.float64 else image.astype(np.float32)


def sums(image, thr=float("inf")):
    """(sum, sum of the elements >= thr, their count): element i belongs to lane i % 1024, which adds its elements in
    ascending i from 0.0 (a float32 map is widened first, the comparison runs in float64); in every wave of 64 lanes the
    xor butterfly v = v + v[lane ^ off] for off = 1, 2, ..., 32; the 16 waves are added in order from 0.0"""
    x = as_map(image).reshape(-1).astype(np.float64)
    n = len(x)
    sel = x >= np.float64(thr)
    rows = -(-n // 1024)
    out = []
    # (an element that does not take part adds +0.0 to a lane that started at +0.0: no operation)
    for v in (x, np.where(sel, x, 0.0), sel.astype(np.float64)):
        padded = np.zeros(rows * 1024)
        padded[:n] = v
        acc = np.zeros(1024)
        for r in padded.reshape(rows, 1024):
            acc = acc + r
        w = acc.reshape(16, 64)
        for off in (1, 2, 4, 8, 16, 32):
            w = w + w[:, np.arange(64) ^ off]
        total = np.float64(0.0)
        for k in range(16):
            total = total + w[k, 0]
        out.append(float(total))
    return tuple(out)


def box_sums(image, patch, descending=False):
    """the 'valid' box sums of a 2D / 3D map as a 3D float64 array: the map narrowed to float32 and widened to float64; sums
    along W, then H, then D, each a zero array plus the p shifted slices in ascending k (an axis with p = 1 keeps its
    0.0 + x).  descending=True adds the slices in descending k: another order, for the sensitivity checks only."""
    x = as_map(image).astype(np.float32).astype(np.float64)
    x = x.reshape((1,) * (3 - x.ndim) + x.shape)
    patch = (1,) * (3 - len(patch)) + tuple(int(p) for p in patch)
    for ax in (2, 1, 0):
        p, no = patch[ax], x.shape[ax] - patch[ax] + 1
        acc = np.zeros(x.shape[:ax] + (no,) + x.shape[ax + 1:])
        for k in (range(p - 1, -1, -1) if descending else range(p)):
            acc = acc + np.take(x, np.arange(k, k + no), axis=ax)
        x = acc
    return x


def box_max(image, patch, descending=False):
    """(maximum, first C-order index with |v - max| <= 1e-8 + 1e-5 |max|, unravelled to the map's rank)"""
    v = box_sums(image, patch, descending)
    mx = np.max(v)
    first = int(np.argmax((np.abs(v - mx) <= 1e-8 + 1e-5 * np.abs(mx)).reshape(-1)))
    return float(mx), [int(i) for i in np.unravel_index(first, v.shape)][3 - len(patch):]


def patch_level_aggregation(image, patch_size, mean=False, **kwargs):
    if type(patch_size) == int:
        patch_size = len(image.shape) * [patch_size]
    mx, first = box_max(image, patch_size)
    if mean:
        mx = mx / float(np.prod(patch_size))
    return {"max_score": mx, "bounding_box": [(int(i), int(i + patch_size[d])) for d, i in enumerate(first)]}


def image_level_aggregation(image, mean=False, **kwargs):
    s = sums(image)[0]
    n = int(np.prod(image.shape, dtype=np.int64))
    return float(s / n) if mean else {"max_score": s}


def threshold_aggregation(image, threshold, mean=True, **kwargs):
    _, st, ct = sums(image, float(threshold))
    return {"max_score": st / ct if mean and ct > 0 else st, "threshold": threshold}


def restated(images, aggregations):
    """[{name: result}] for a list of maps and an aggregations dict whose `_target_`s end in one of the three names"""
    out = []
    for im in images:
        res = {}
        for name, cfg in aggregations.items():
            params = {k: v for k, v in cfg.items() if k != "_target_"}
            fn = cfg["_target_"].rpartition(".")[2]
            assert fn in _KINDS, fn
            res[name] = globals()[fn](im, **params)
        out.append(res)
    return out


def wide_range(shape, seed, dtype=np.float32):
    """a map whose values span about 60 binades: float64 sums of such values are not exact, so their order shows"""
    rng = np.random.default_rng(seed)
    v = rng.random(shape) * 2.0 ** rng.integers(-30, 31, shape)
    return v.astype(dtype)


# (shape, patch, seed): wide-range maps of the box tests.  The seeds are chosen so that every maximum changes when the box
# sums are added in descending k (about half of all box sums do for any seed, the maximum for one seed in four)
WIDE_BOX = [((19, 37, 70), [5, 4, 10], 2), ((12, 10, 33), 3, 10), ((150, 301), 10, 0)]
# (shape, dtype, seed, threshold) of the sums tests: the restated sum and thresholded sum differ from numpy's pairwise sums
WIDE_SUMS = [((25, 41), np.float64, 10, 1.0), ((11, 467), np.float32, 1, 1.0)]
