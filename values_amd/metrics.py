"""Per-image segmentation metrics of the reference's test loop, computed from two device reductions.

Mirrors `calculate_test_metrics` and `calculate_ged` of uncertainty_modeling/test_3D.py:250-358 (same names,
arguments, result keys).  The reference evaluates them with torchmetrics' `dice` (torchmetrics==0.11.4,
functional/classification/dice.py; average="micro", mdmc_average="global", zero_division=0) on repeated tensors --
T*R + T*T + R*R + 2*T*R mask comparisons per image.  Here ONE pass (`vx_mask_agreement`) counts, for every pair of
masks, the voxels on which both carry class c; every Dice is then a ratio of sums of these integers:
    tp = sum_c I[a][b][c],  fp = sum_c (I[a][a][c] - I[a][b][c]),  fn = sum_c (I[b][b][c] - I[a][b][c])
with c running over the classes that survive `ignore_index` (torchmetrics deletes that one-hot column for micro
averaging).  SoftDiceLoss + NLLLoss (loss_modules.py:7-97) come from `vx_soft_metric_sums`.

Whole steps: `process_metrics_2d` (test_2D.py:205-244) and `process_metrics_3d` (calculate_metrics, test_3D.py:537-575)
take the B images of an inference step through `vx_mask_agreement_batched` (and, 3D, `vx_soft_metric_sums_batched`) at once.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib


def mask_agreement(masks: torch.Tensor, num_classes: int) -> np.ndarray:
    """masks (M, *spatial) integer labels on the device -> counts (M, M, C) int64 (host)."""
    _lib.require_gpu()
    lib = _lib.load()
    m = masks.reshape(masks.shape[0], -1).to(torch.uint8).contiguous()
    M, nvox = m.shape
    out = torch.empty((M, M, num_classes), dtype=torch.int64, device=m.device)
    _lib.check(lib.vx_mask_agreement(m.data_ptr(), M, num_classes, nvox, out.data_ptr(), _lib.stream_ptr()), "vx_mask_agreement")
    return out.cpu().numpy()


def mask_agreement_batched(masks: torch.Tensor, num_classes: int, remap_from: Optional[int] = None) -> np.ndarray:
    """masks (B, M, *spatial) integer labels on the device -> counts (B, M, M, C) int64 (host): `mask_agreement` of every
    image of a batch with ONE launch (`vx_mask_agreement_batched`: C <= 32) and one device-to-host copy.  A label equal
    to remap_from counts as class C - 1 (the 2D ground truth's ignore label 255 -> the appended class, on load)."""
    _lib.require_gpu()
    lib = _lib.load()
    if masks.dim() < 2:
        raise ValueError("mask_agreement_batched: masks (B, M, *spatial) expected")
    B, M = int(masks.shape[0]), int(masks.shape[1])
    m = masks.reshape(B, M, -1).to(torch.uint8).contiguous()
    out = torch.empty((B, M, M, num_classes), dtype=torch.int64, device=m.device)
    _lib.check(lib.vx_mask_agreement_batched(m.data_ptr(), B, M, num_classes, m.shape[2], -1 if remap_from is None else int(remap_from),
                                             out.data_ptr(), _lib.stream_ptr()), "vx_mask_agreement_batched")
    return out.cpu().numpy()


def soft_metric_sums_batched(mean_softmax: torch.Tensor, gt: torch.Tensor) -> np.ndarray:
    """mean_softmax (B, C, *spatial) float32 and gt (B, R, *spatial) integer labels on the device -> sums (B, R, 3C + 1)
    float64 (host): per image, rater and class  sum p_c [g_r = c],  sum [g_r = c],  sum p_c,  then  sum log p_{g_r}  --
    `vx_soft_metric_sums` of every image of a batch with one launch pair (`vx_soft_metric_sums_batched`: C <= 32,
    R <= 31) and one device-to-host copy.  An image's row is bit-equal to what the same image gives when submitted alone."""
    _lib.require_gpu()
    lib = _lib.load()
    if mean_softmax.dim() < 2 or gt.dim() < 2 or gt.shape[0] != mean_softmax.shape[0]:
        raise ValueError("soft_metric_sums_batched: mean_softmax (B, C, *spatial) and gt (B, R, *spatial) expected")
    B, C, R = int(mean_softmax.shape[0]), int(mean_softmax.shape[1]), int(gt.shape[1])
    p = mean_softmax.reshape(B, C, -1).to(torch.float32).contiguous()
    g8 = gt.reshape(B, R, -1).to(torch.uint8).contiguous()
    nvox = int(p.shape[2])
    if g8.shape[2] != nvox:
        raise ValueError(f"soft_metric_sums_batched: {nvox} voxels of probabilities, {g8.shape[2]} of labels")
    sums = torch.empty((B, R, 3 * C + 1), dtype=torch.float64, device=p.device)
    ws = torch.empty(max(int(lib.vx_soft_metric_batched_workspace_bytes(B, C, R, nvox)), 8), dtype=torch.uint8, device=p.device)
    _lib.check(lib.vx_soft_metric_sums_batched(p.data_ptr(), g8.data_ptr(), B, C, R, nvox, sums.data_ptr(), ws.data_ptr(),
                                               _lib.stream_ptr()), "vx_soft_metric_sums_batched")
    return sums.cpu().numpy()


def _micro_dice(I: np.ndarray, a_idx, b_idx, classes) -> float:
    """torchmetrics dice(average='micro', mdmc_average='global', zero_division=0) pooled over the listed (a, b) pairs."""
    tp = fp = fn = 0
    for a, b in zip(a_idx, b_idx):
        iab = int(I[a, b, classes].sum())
        tp += iab
        fp += int(I[a, a, classes].sum()) - iab
        fn += int(I[b, b, classes].sum()) - iab
    den = 2 * tp + fp + fn
    return 0.0 if den == 0 else 2.0 * tp / den


def _classes(num_classes: int, ignore_index: Optional[int]):
    return [c for c in range(num_classes) if c != ignore_index]


def _to_dev(t, dev):
    return t.to(dev) if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t), device=dev)


def calculate_test_metrics(output_softmax: torch.Tensor, ground_truth: torch.Tensor) -> Dict:
    """output_softmax (1, C, *spatial) mean softmax; ground_truth (R, *spatial) integer -> {"loss", "dice"}
    (test_3D.py:250-281: per rater SoftDiceLoss + NLLLoss and Dice(ignore_index=0), averaged over raters)."""
    _lib.require_gpu()
    lib = _lib.load()
    dev = output_softmax.device if output_softmax.is_cuda else torch.device("cuda", torch.cuda.current_device())
    p = _to_dev(output_softmax, dev).to(torch.float32)
    if p.shape[0] != 1:
        raise ValueError("calculate_test_metrics: output_softmax must be (1, C, ...) -- the mean prediction")
    C = p.shape[1]
    p = p[0].reshape(C, -1).contiguous()
    gt = _to_dev(ground_truth, dev)
    R = gt.shape[0]
    g8 = gt.reshape(R, -1).to(torch.uint8).contiguous()
    nvox = p.shape[1]
    sums = torch.empty((R, 3 * C + 1), dtype=torch.float64, device=dev)
    ws = torch.empty(max(int(lib.vx_soft_metric_workspace_bytes(C, R)), 8), dtype=torch.uint8, device=dev)
    _lib.check(lib.vx_soft_metric_sums(p.data_ptr(), g8.data_ptr(), C, R, nvox, sums.data_ptr(), ws.data_ptr(),
                                       _lib.stream_ptr()), "vx_soft_metric_sums")
    # hard Dice of the arg-max of the mean prediction against every rater
    # (the arg-max itself is one of vx_unc_reduce's outputs; recomputed here from p for a self-contained signature)
    from .uncertainty import uncertainty_maps
    am = uncertainty_maps(p.reshape(1, 1, C, nvox), from_logits=False)["argmax"].reshape(1, nvox)
    I = mask_agreement(torch.cat([am, g8], 0), C)
    return _test_metrics_from_sums(sums.cpu().numpy(), I, C, nvox)


def _test_metrics_from_sums(sums_row: np.ndarray, I: np.ndarray, C: int, nvox: int, pred: int = 0, raters=None) -> Dict:
    """calculate_test_metrics' ratios for one image: sums_row (R, 3C + 1) the soft sums of its raters (vx_soft_metric_sums'
    layout), I (M, M, C) its agreement counts; pred / raters: the rows of I that hold the arg-max of the mean prediction
    and the R raters (default: row 0 and rows 1 .. R)."""
    s = np.asarray(sums_row)
    R = s.shape[0]
    G = list(range(1, 1 + R)) if raters is None else list(raters)
    smooth = 1e-5
    losses, dices = [], []
    cls = _classes(C, 0)
    for r in range(R):
        inter, cnt, psum = s[r, 0:3 * C:3], s[r, 1:3 * C:3], s[r, 2:3 * C:3]
        soft = np.mean(-((2.0 * inter + smooth) / ((psum + cnt) + smooth)))      # soft_dice, B = 1
        nll = -s[r, 3 * C] / nvox                                                 # NLLLoss mean reduction
        losses.append(soft + nll)
        dices.append(_micro_dice(I, [pred], [G[r]], cls))
    return {"loss": float(np.mean(np.array(losses))), "dice": float(np.mean(np.array(dices)))}


def calculate_ged(output_softmax: torch.Tensor, ground_truth: torch.Tensor, ignore_index: int = 0, ged_only: bool = False,
                  pred_masks: Optional[torch.Tensor] = None) -> Dict:
    """output_softmax (T, C, *spatial); ground_truth (R, *spatial) -> {"ged", "max dice rater i", "max dice pred"}
    (test_3D.py:284-358).  pred_masks (T, *spatial): the per-sample arg-max masks when the caller already has them
    (vx_unc_reduce's sample_argmax), otherwise they are taken from output_softmax."""
    _lib.require_gpu()
    dev = output_softmax.device if output_softmax.is_cuda else torch.device("cuda", torch.cuda.current_device())
    sm = _to_dev(output_softmax, dev)
    T, C = sm.shape[0], sm.shape[1]
    gt = _to_dev(ground_truth, dev)
    R = gt.shape[0]
    if pred_masks is None:
        from .uncertainty import uncertainty_maps
        nvox = sm[0, 0].numel()
        pred_masks = uncertainty_maps(sm.reshape(1, T, C, nvox).to(torch.float32), from_logits=False,
                                      want_sample_argmax=True)["sample_argmax"].reshape(T, nvox)
    pm = _to_dev(pred_masks, dev).reshape(T, -1).to(torch.uint8)
    g8 = gt.reshape(R, -1).to(torch.uint8)
    stack = torch.cat([pm, g8], 0)
    # up to 8 classes: the one-image kernel, as ever (same integers either way); more (2D: 19 + 1): the batched one with B = 1
    I = mask_agreement(stack, C) if C <= 8 else mask_agreement_batched(stack[None], C)[0]
    return _ged_from_counts(I, list(range(T)), [T + r for r in range(R)], C, ignore_index, ged_only)


def _ged_from_counts(I: np.ndarray, P, G, C: int, ignore_index, ged_only: bool) -> Dict:
    """calculate_ged's ratios from one image's agreement counts I (M, M, C); P / G: the rows of the predictions / raters"""
    T, R = len(P), len(G)
    cls = _classes(C, ignore_index)
    # pooled distances over the repeated tensors of :290-320 (order of a pair does not change pooled tp / fp+fn)
    d_gp = 1.0 - _micro_dice(I, [p for _ in G for p in P], [g for g in G for _ in P], cls)
    d_pp = 1.0 - _micro_dice(I, [a for a in P for _ in P], [b for _ in P for b in P],
                             cls if ignore_index == 0 else _classes(C, None))
    gt_has_ignored = bool(ignore_index is not None and 0 <= ignore_index < C and any(I[g, g, ignore_index] > 0 for g in G))
    d_gg = 1.0 - _micro_dice(I, [a for a in G for _ in G], [b for _ in G for b in G],
                             cls if gt_has_ignored else _classes(C, None))
    out = {"ged": float(2 * d_gp - d_pp - d_gg)}
    if R > 1 and not ged_only:
        pair = np.array([[np.float32(_micro_dice(I, [p], [g], cls)) for g in G] for p in P], dtype=np.float32)
        # per rater: best prediction (starts from 0, strict >; :326-337); per prediction: best rater, averaged
        for r in range(R):
            out["max dice rater {}".format(r)] = float(max(np.float32(0), pair[:, r].max()))
        out["max dice pred"] = float(np.float32(sum(max(np.float32(0), pair[p].max()) for p in range(T))) / np.float32(T))
    return out


def _extended_gt(ground_truth, dev, ignore_label):
    """(R, *spatial) labels -> (R, nvox) uint8 on the device; ignore_label must survive the cast to be remapped on load"""
    if ignore_label is not None and not 0 <= int(ignore_label) <= 255:
        raise ValueError(f"ignore_label {ignore_label} is no uint8 label")
    gt = _to_dev(ground_truth, dev)
    return gt.reshape(gt.shape[0], -1).to(torch.uint8)


def calculate_test_metrics_2d(mean_softmax: torch.Tensor, ground_truth: torch.Tensor, ignore_label: Optional[int] = None,
                              pred_seg: Optional[torch.Tensor] = None) -> Dict:
    """Tester.calculate_test_metrics of test_2D.py:161-173: mean_softmax (C_ext, H, W), the mean prediction WITH the
    appended zero channel; ground_truth (R, H, W) integer -> {"dice"}: per rater the Dice of the arg-max of the mean
    prediction with ignore_index = C_ext - 1 (the appended class), averaged over raters.  ignore_label: ground-truth
    pixels carrying it count as class C_ext - 1 (what process_output does to the tensor beforehand; None: already done).
    pred_seg (H, W): the arg-max when the caller has it (process_output_2d's "pred_seg")."""
    _lib.require_gpu()
    dev = mean_softmax.device if mean_softmax.is_cuda else torch.device("cuda", torch.cuda.current_device())
    p = _to_dev(mean_softmax, dev)
    C = int(p.shape[0])
    if pred_seg is None:
        from .uncertainty import uncertainty_maps
        nvox = p[0].numel()
        pred_seg = uncertainty_maps(p.reshape(1, 1, C, nvox).to(torch.float32), from_logits=False)["argmax"]
    am = _to_dev(pred_seg, dev).reshape(1, -1).to(torch.uint8)
    g8 = _extended_gt(ground_truth, dev, ignore_label)
    I = mask_agreement_batched(torch.cat([am, g8], 0)[None], C, ignore_label)[0]
    return _test_metrics_2d_from_counts(I, 0, range(1, 1 + g8.shape[0]), C)


def _test_metrics_2d_from_counts(I, p, G, C):
    cls = _classes(C, C - 1)
    return {"dice": float(np.mean(np.array([_micro_dice(I, [p], [g], cls) for g in G])))}


def process_metrics_2d(out: Dict, gt: torch.Tensor, ignore_label: int = 255, ged_only: bool = True, image_ids=None,
                       sample_argmax: Optional[torch.Tensor] = None):
    """The metrics half of Tester.process_output (test_2D.py:205-244) for a whole batch: per image
    calculate_test_metrics ("dice") and calculate_ged(ignore_index = C, ged_only) ("ged", and with ged_only=False and
    several raters the "max dice ..." keys of process_image_prediction).

    out: what process_output_2d returns -- softmax_pred (B, T, C, H, W), pred_seg (B, H, W); gt (B, R, H, W) integer
    labels that still carry ignore_label.  sample_argmax (B, T, H, W): the per-sample arg-max masks when the caller has
    them (uncertainty_maps(..., want_sample_argmax=True), which also feeds the results writer), else taken from
    softmax_pred.  Returns a list of metric dicts in batch order, or {image_id: dict} with image_ids.

    The reference appends a zero channel to the softmax so that class C exists for the ignored pixels.  It is never
    materialised here: a softmax is > 0 everywhere, so the zero channel never wins an arg-max, and the arg-max masks of
    the C-channel tensor ARE those of the extended one; only the ground truth sees class C (ignore_label is mapped to
    it on load).  One vx_mask_agreement_batched call over the stacked [mean arg-max, T sample arg-maxes, R raters]
    (M = 1 + T + R <= 32) and one host copy; every ratio is formed on the host from the integers."""
    _lib.require_gpu()
    sm = out["softmax_pred"]
    dev = sm.device if sm.is_cuda else torch.device("cuda", torch.cuda.current_device())
    B, T, C = (int(v) for v in sm.shape[:3])
    g = _to_dev(gt, dev)
    if g.dim() < 3 or g.shape[0] != B:
        raise ValueError(f"process_metrics_2d: gt (B, R, H, W) expected for {B} images, got {tuple(g.shape)}")
    R = int(g.shape[1])
    if 1 + T + R > 32:
        raise ValueError(f"process_metrics_2d: 1 + T + R = {1 + T + R} masks per image (at most 32)")
    if ignore_label is not None and not 0 <= int(ignore_label) <= 255:
        raise ValueError(f"ignore_label {ignore_label} is no uint8 label")
    if image_ids is not None and len(image_ids) != B:
        raise ValueError(f"process_metrics_2d: {len(image_ids)} image ids for {B} images")
    if sample_argmax is None:
        from .uncertainty import uncertainty_maps
        smd = _to_dev(sm, dev).to(torch.float32)
        sample_argmax = uncertainty_maps(smd.reshape(B, T, C, -1), from_logits=False, want_sample_argmax=True)["sample_argmax"]
    stack = torch.cat([_to_dev(out["pred_seg"], dev).reshape(B, 1, -1).to(torch.uint8),
                       _to_dev(sample_argmax, dev).reshape(B, T, -1).to(torch.uint8),
                       g.reshape(B, R, -1).to(torch.uint8)], 1)
    Ce = C + 1
    I = mask_agreement_batched(stack, Ce, ignore_label)
    P, G = list(range(1, 1 + T)), list(range(1 + T, 1 + T + R))
    res = []
    for b in range(B):
        m = _test_metrics_2d_from_counts(I[b], 0, G, Ce)
        m.update(_ged_from_counts(I[b], P, G, Ce, Ce - 1, ged_only))
        res.append(m)
    return res if image_ids is None else dict(zip(image_ids, res))


def _first(d: Dict, *keys):
    for k in keys:
        if d.get(k) is not None:
            return d[k]
    return None


def process_metrics_3d(out: Dict, gt: torch.Tensor, image_ids=None, sample_argmax: Optional[torch.Tensor] = None,
                       probs: Optional[torch.Tensor] = None):
    """calculate_metrics of test_3D.py:537-575 for the B cases of a step: per case calculate_test_metrics ("loss": SoftDice +
    NLL, "dice": Dice with ignore_index = 0, both averaged over the raters) and, when R > 1 or T > 1 (the reference's
    condition), the keys of calculate_ged(..., ignore_index=0, ged_only=False).

    out: what uncertainty_maps / predict_uncertainty return -- mean_softmax (B, C, *spatial), the arg-max of the mean
    prediction ("argmax" or "pred_seg_mean", (B, *spatial); taken from mean_softmax when absent) and optionally the
    per-sample arg-max masks ("sample_argmax" or "pred_seg", (B, T, *spatial)).  gt (B, R, *spatial) integer labels.
    sample_argmax overrides out's; when neither is there the masks are taken from probs (B, T, C, *spatial) through
    uncertainty_maps(want_sample_argmax=True); with none of the three T is unknown and only "loss" / "dice" are produced.
    Returns a list of metric dicts in batch order, or {image_id: dict} with image_ids (what results.log_metrics takes).

    One vx_soft_metric_sums_batched call, one vx_mask_agreement_batched call over the stacked [mean arg-max, T sample
    arg-maxes, R raters] and two host copies; every ratio is formed on the host by the helpers the per-case functions use
    (same integers, same float64 arithmetic).  The counts kernel takes at most 32 masks and 32 classes: with
    1 + T + R > 32 or C > 32 the cases go through calculate_test_metrics / calculate_ged one at a time instead (same
    results, the per-case launch count, and those functions' own limits)."""
    _lib.require_gpu()
    mean = out["mean_softmax"]
    dev = mean.device if mean.is_cuda else torch.device("cuda", torch.cuda.current_device())
    mean = _to_dev(mean, dev).to(torch.float32)
    if mean.dim() < 3:
        raise ValueError("process_metrics_3d: out['mean_softmax'] (B, C, *spatial) expected")
    B, C = int(mean.shape[0]), int(mean.shape[1])
    g = _to_dev(gt, dev)
    if g.dim() < 3 or g.shape[0] != B:
        raise ValueError(f"process_metrics_3d: gt (B, R, *spatial) expected for {B} cases, got {tuple(g.shape)}")
    R = int(g.shape[1])
    if image_ids is not None and len(image_ids) != B:
        raise ValueError(f"process_metrics_3d: {len(image_ids)} image ids for {B} cases")
    nvox = mean[0, 0].numel()
    from .uncertainty import uncertainty_maps
    if sample_argmax is None:
        sample_argmax = _first(out, "sample_argmax", "pred_seg")
    if sample_argmax is None and probs is not None:
        pd = _to_dev(probs, dev).to(torch.float32)
        sample_argmax = uncertainty_maps(pd.reshape(B, pd.shape[1], C, nvox), from_logits=False, want_sample_argmax=True)["sample_argmax"]
    T = None
    if sample_argmax is not None:
        sample_argmax = _to_dev(sample_argmax, dev)
        T = int(sample_argmax.shape[1])
    want_ged = _ged_due(T, R)
    if 1 + (T or 0) + R > 32 or C > 32:
        res = []
        for b in range(B):
            m = calculate_test_metrics(mean[b:b + 1], g[b])
            if want_ged:
                m.update(calculate_ged(mean[b:b + 1].expand((T,) + tuple(mean.shape[1:])), g[b], ignore_index=0,
                                       pred_masks=sample_argmax[b]))   # (only T and C are read off the first argument)
            res.append(m)
        return res if image_ids is None else dict(zip(image_ids, res))
    am = _first(out, "argmax", "pred_seg_mean")
    if am is None:
        am = uncertainty_maps(mean.reshape(B, 1, C, nvox), from_logits=False)["argmax"]
    g8 = g.reshape(B, R, nvox).to(torch.uint8)
    parts = [_to_dev(am, dev).reshape(B, 1, nvox).to(torch.uint8)]
    if want_ged:
        parts.append(sample_argmax.reshape(B, T, nvox).to(torch.uint8))
    sums = soft_metric_sums_batched(mean, g8)
    I = mask_agreement_batched(torch.cat(parts + [g8], 1), C)
    res = _metrics_3d_from_reductions(sums, I, C, nvox, T, R)
    return res if image_ids is None else dict(zip(image_ids, res))


def _ged_due(T: Optional[int], R: int) -> bool:
    """test_3D.py:554: the GED keys exist for several raters or several predictions (T None: no per-sample masks at all)"""
    return T is not None and (R > 1 or T > 1)


def _metrics_3d_from_reductions(sums: np.ndarray, I: np.ndarray, C: int, nvox: int, T: Optional[int], R: int):
    """The host half of process_metrics_3d: sums (B, R, 3C + 1) and the counts I (B, M, M, C) of the stack
    [mean arg-max, the T sample arg-maxes (only when the GED is due), R raters] -> the metric dicts in batch order."""
    nP = T if _ged_due(T, R) else 0
    P, G = list(range(1, 1 + nP)), list(range(1 + nP, 1 + nP + R))
    res = []
    for b in range(len(sums)):
        m = _test_metrics_from_sums(sums[b], I[b], C, nvox, 0, G)
        if nP:
            m.update(_ged_from_counts(I[b], P, G, C, 0, False))
        res.append(m)
    return res
