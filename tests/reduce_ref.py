"""Float64 restatement of the uncertainty reduction family (numpy only, no GPU): what vx_unc_reduce_ex, the
vx_unc_stats_* pair and vx_softmax_accumulate are held to in tests/test_gpu_reduce.py and tools/fuzz_reduce.py.

Built on oracle.uncertainty_oracle.{softmax, calculate_uncertainty, mean_and_argmax}, so the reference's float32
accumulators round where the oracle has them.  Pinned to the reference's own outputs (unc_kat.npz, accum_24.npz) by
tests/test_reduce_ref_cpu.py.
"""
from __future__ import annotations

import numpy as np

from oracle import uncertainty_oracle as uo

MARGIN = 1e-5      # top-2 margin below which an arg-max may legitimately differ (the value the existing tests use)


def _count(count, B, nvox, dtype):
    return np.clip(np.asarray(count, dtype=dtype).reshape(B, nvox), 1, None)


def maps(x, from_logits, in_count=None, out_count=None, dtype=np.float64):
    """x (B, T, C, nvox) probabilities (or un-normalised sums of them) or logits -> dict of
    pred_entropy / expected_entropy / mutual_information / variance (B, nvox), mean_softmax (B, C, nvox),
    argmax (B, nvox) u8, sample_argmax (B, T, nvox) u8.
      in_count  (B, nvox): x is divided by clip(count, 1) before everything else (the normalised sliding-window sums)
      out_count (B, nvox): the maps and the mean are divided by clip(count, 1) afterwards, the variance by its square
                           (quirk D10: calculate_uncertainty on the UN-normalised sums, divided at save time)
      variance : p.var(axis=T).mean(axis=C)
    dtype: float64 is the reference; float32 rounds the input and every accumulator to float32, which is how the tests
    measure what float32 arithmetic alone costs on their inputs (the "gap" of the tolerance rule)."""
    x = np.asarray(x).astype(dtype)
    B, T, C, nvox = x.shape
    out = {k: np.zeros((B, nvox), dtype=np.float64) for k in ("pred_entropy", "expected_entropy", "mutual_information",
                                                               "variance")}
    out["mean_softmax"] = np.zeros((B, C, nvox), dtype=np.float64)
    out["argmax"] = np.zeros((B, nvox), dtype=np.uint8)
    out["sample_argmax"] = np.zeros((B, T, nvox), dtype=np.uint8)
    if in_count is not None:
        x = x / _count(in_count, B, nvox, dtype)[:, None, None, :]
    for b in range(B):
        p = uo.softmax(x[b], axis=1) if from_logits else x[b]
        cu = uo.calculate_uncertainty(p)
        mean, am, sam = uo.mean_and_argmax(p)
        res = {"pred_entropy": cu["pred_entropy"], "expected_entropy": cu["aleatoric_uncertainty"],
               "mutual_information": cu["epistemic_uncertainty"], "variance": p.var(axis=0, dtype=dtype).mean(axis=0, dtype=dtype),
               "mean_softmax": mean}
        if out_count is not None:
            cl = _count(out_count, B, nvox, dtype)[b]
            for k in res:
                res[k] = res[k].astype(dtype) / (cl * cl if k == "variance" else cl)
        for k, v in res.items():
            out[k][b] = v
        out["argmax"][b], out["sample_argmax"][b] = am, sam
    return out


def clear_mean(mean, margin=MARGIN):
    """mean (..., C, nvox) -> bool (..., nvox): the best class leads the second by more than `margin`"""
    s = np.sort(np.asarray(mean, dtype=np.float64), axis=-2)
    return (s[..., -1, :] - s[..., -2, :]) > margin


def clear_sample(x, from_logits, margin=MARGIN):
    """x (B, T, C, nvox) -> bool (B, T, nvox): the same margin on every sample's class probabilities"""
    x = np.asarray(x, dtype=np.float64)
    return clear_mean(uo.softmax(x, axis=2) if from_logits else x, margin)


def accumulate(logits, crops, image_shape):
    """DataCarrier3D.concat_data for a batch of patches in float64: logits (B, T, C, P0, P1, P2), crops B x (x0, y0, z0)
    -> sums (T, C, X, Y, Z) of the class softmax, counts (X, Y, Z) of the patches covering a voxel.  Patch voxels outside
    the image are dropped."""
    logits = np.asarray(logits, dtype=np.float64)
    B, T, C = logits.shape[:3]
    sums = np.zeros((T, C) + tuple(image_shape), dtype=np.float64)
    counts = np.zeros(tuple(image_shape), dtype=np.float64)
    for b in range(B):
        p = uo.softmax(logits[b], axis=1)
        n = [max(0, min(int(logits.shape[3 + a]), int(image_shape[a]) - int(crops[b][a]))) for a in range(3)]
        dst = tuple(slice(int(crops[b][a]), int(crops[b][a]) + n[a]) for a in range(3))
        sums[(slice(None), slice(None)) + dst] += p[:, :, :n[0], :n[1], :n[2]]
        counts[dst] += 1
    return sums, counts
