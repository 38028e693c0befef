"""Direct numpy definitions of the two reductions behind the 3D per-case metrics (test helpers, no device code):
the soft sums of vx_soft_metric_sums(_batched) and the class-agreement counts of vx_mask_agreement(_batched)."""
import numpy as np


def np_soft_sums(p, g):
    """p (B, C, nvox) float32 probabilities, g (B, R, nvox) integer labels -> (sums, mag), both (B, R, 3C + 1) float64:
    per class  sum p_c [g_r = c],  sum [g_r = c],  sum p_c,  then  sum log p_{g_r}  with the log taken in float32 (the
    kernel's term) and widened; a label >= C is in no class and has no log term.  mag: the same sums over |term|."""
    B, C, nvox = p.shape
    R = g.shape[1]
    p64 = p.astype(np.float64)
    logp = np.log(p.astype(np.float32)).astype(np.float64)
    sums = np.zeros((B, R, 3 * C + 1), np.float64)
    mag = np.zeros_like(sums)
    for b in range(B):
        for r in range(R):
            for c in range(C):
                m = g[b, r] == c
                sums[b, r, 3 * c] = mag[b, r, 3 * c] = p64[b, c][m].sum()
                sums[b, r, 3 * c + 1] = mag[b, r, 3 * c + 1] = int(m.sum())
                sums[b, r, 3 * c + 2] = mag[b, r, 3 * c + 2] = p64[b, c].sum()
                sums[b, r, 3 * C] += logp[b, c][m].sum()
                mag[b, r, 3 * C] += np.abs(logp[b, c][m]).sum()
    return sums, mag


def np_counts(m, C):
    """(B, M, nvox) labels -> (B, M, M, C): #{v : m_i(v) == c and m_j(v) == c}"""
    m = m.astype(np.int64)
    out = np.zeros(m.shape[:2] + (m.shape[1], C), np.int64)
    for c in range(C):
        out[..., c] = ((m[:, :, None] == c) & (m[:, None, :] == c)).sum(-1)
    return out


def formula_case(C, T, R, shape, tag):
    """One case as tests/test_gpu_results.py::test_metrics_match_oracle builds it: sm (T, C, *shape) float32 softmax of
    formula logits, gt (R, *shape) int64 labels < C"""
    from tests.formula import formula_tensor
    logits = formula_tensor((T, C) + shape, 8100 + C + tag, scale=2.5)
    e = np.exp(logits - logits.max(1, keepdims=True))
    sm = (e / e.sum(1, keepdims=True)).astype(np.float32)
    gt = ((formula_tensor((R,) + shape, 8200 + C + tag) + 1.0) * 0.5 * C).astype(np.int64).clip(0, C - 1)
    return sm, gt
