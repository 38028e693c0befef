"""The validation step on MI355X: validation/val_loss and validation/val_dice for all three 3D model kinds, the 2D
HighResolutionNet with the SSN head (and any model that returns logits), as LightningExperiment.validation_step and
forward_ssn(val=True) compute them (lightning_experiment.py:175-219, 278-377).

The reference materialises S x B x C x voxels logit samples and runs cross_entropy, S arg-maxes and S dice calls over
them.  Here one fused reduction per branch (valstep.hip) reads the model's output once and returns a few hundred bytes of
float64 sums and integer counts; every ratio is formed on the host from those:
    val_sums            logits (B, C, *spatial)                 -> (B, 5C + 3)      vx_val_sums_batched
    val_sums_aleatoric  mu_s   (B, 2C, *spatial), T samples     -> (B, 5C + 3)      vx_val_aleatoric_sums_batched
    val_sums_ssn        head   (B, (2 + R)C, *spatial), S       -> (B, S, 1 + 2C), (B, C + 2)   vx_val_ssn_sums_batched
    val_sums_ssn2d      a LowRankNormal2D (head at 1/4 res.), S -> (B, S, 1 + 2C), (B, C + 2)   vx_val_ssn2d_sums_batched
The 2D SSN head's samples are formed per full-resolution pixel from the low-resolution head inside the reduction (the
bits LowRankNormal2D.sample_images writes): neither the S x B x C x H x W samples nor the reference's (B, C*H*W, R) factor
tensor exist.
The host arithmetic follows the reference, its ignore_index quirk included: with ignore_index == 0 (the 3D default) the
cross-entropy ignores NOTHING and the loss is SoftDice + CE; with ignore_index != 0 the loss is CE(ignore_index) alone;
the aleatoric branch is SoftDice + NLL either way; `dice` always deletes the ignore_index column (torchmetrics 0.11.4,
average='micro', mdmc_average='global' -- the counting metrics.py does).

Not here: the validation data loader (the caller supplies batches), training / gradients, the
visualisation sample and TensorBoard grids.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from . import _lib
from .metrics import _classes, _micro_dice

_SMOOTH = 1e-5   # SoftDiceLoss()


def _check_ignore(ignore_label):
    if ignore_label is None:
        return -1
    if not -1 <= int(ignore_label) <= 255:
        raise ValueError(f"ignore_label {ignore_label} is no uint8 label (None / -1: nothing is ignored)")
    return int(ignore_label)


def _labels_u8(target, dev, B: int, nvox: int, ignore: int) -> torch.Tensor:
    """(B, *spatial) or (B, 1, *spatial) integer labels -> (B, nvox) uint8 on the device; a label outside 0..255 becomes
    one that is in no class and not the ignore label, so the kernel counts it as invalid"""
    t = target.to(dev) if isinstance(target, torch.Tensor) else torch.as_tensor(np.asarray(target), device=dev)
    if t.numel() != B * nvox:
        raise ValueError(f"{tuple(t.shape)} labels for {B} items of {nvox} voxels")
    t = t.reshape(B, nvox)
    if t.dtype != torch.uint8:
        bad = 254 if ignore == 255 else 255
        t = torch.where((t < 0) | (t > 255), torch.full_like(t, bad), t).to(torch.uint8)
    return t.contiguous()


def _raise_invalid(n, who):
    if n:
        raise ValueError(f"{who}: {int(n)} voxels carry a label that is neither a class nor the ignore label")


def val_sums(logits: torch.Tensor, target, ignore_label: Optional[int] = None, raise_invalid: bool = True) -> np.ndarray:
    """logits (B, C, *spatial) float32 on the device, target (B, *spatial) integer labels -> (B, 5C + 3) float64 (host):
    per class  sum softmax_c [t = c], sum [t = c], sum softmax_c, tp_c, pred_c;  then  sum log_softmax_t, the count of voxels
    that take a log term, the invalid count (a label >= C other than ignore_label: ValueError unless raise_invalid=False)."""
    _lib.require_gpu()
    lib = _lib.load()
    ig = _check_ignore(ignore_label)
    if logits.dim() < 2:
        raise ValueError("val_sums: logits (B, C, *spatial) expected")
    B, C = int(logits.shape[0]), int(logits.shape[1])
    x = logits.reshape(B, C, -1).to(torch.float32).contiguous()
    nvox = int(x.shape[2])
    g = _labels_u8(target, x.device, B, nvox, ig)
    sums = torch.empty((B, 5 * C + 3), dtype=torch.float64, device=x.device)
    need = int(lib.vx_val_sums_workspace_bytes(B, C, nvox))
    ws = _lib.workspace(x.device, need)
    _lib.check(lib.vx_val_sums_batched(x.data_ptr(), g.data_ptr(), B, C, nvox, ig, sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _lib.stream_ptr()), "vx_val_sums_batched")
    out = sums.cpu().numpy()
    if raise_invalid:
        _raise_invalid(out[:, 5 * C + 2].sum(), "val_sums")
    return out


def val_sums_aleatoric(mu_s: torch.Tensor, target, n_samples: int = 10, eps: Optional[torch.Tensor] = None, seed: int = 0,
                       item0: int = 0, ignore_label: Optional[int] = None, raise_invalid: bool = True) -> np.ndarray:
    """mu_s (B, 2C, *spatial) the aleatoric head (mu | s), eps (B, T, C, *spatial) injected normals or None (generated
    from seed; item b draws the streams of the global item index item0 + b) -> (B, 5C + 3) float64 as val_sums, with
    p = exp(lavg), the log term lavg_t and the arg-max of lavg, lavg_c = logsumexp_t log_softmax(y_t)_c - log T."""
    _lib.require_gpu()
    lib = _lib.load()
    ig = _check_ignore(ignore_label)
    if mu_s.dim() < 2 or mu_s.shape[1] % 2:
        raise ValueError("val_sums_aleatoric: mu_s (B, 2C, *spatial) expected")
    B, C, T = int(mu_s.shape[0]), int(mu_s.shape[1]) // 2, int(n_samples)
    x = mu_s.reshape(B, 2 * C, -1).to(torch.float32).contiguous()
    nvox = int(x.shape[2])
    g = _labels_u8(target, x.device, B, nvox, ig)
    e = None
    if eps is not None:
        e = eps.to(device=x.device, dtype=torch.float32).contiguous()
        if e.numel() != B * T * C * nvox:
            raise ValueError(f"val_sums_aleatoric: eps of {tuple(eps.shape)} for (B, T, C, voxels) = {(B, T, C, nvox)}")
    sums = torch.empty((B, 5 * C + 3), dtype=torch.float64, device=x.device)
    ws = _lib.workspace(x.device, int(lib.vx_val_aleatoric_sums_workspace_bytes(B, C, nvox)))
    _lib.check(lib.vx_val_aleatoric_sums_batched(x.data_ptr(), _lib.ptr(e), int(seed) & 0xFFFFFFFF, int(item0) & 0xFFFFFFFF,
                                                 g.data_ptr(), B, T, C, nvox, ig, sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 _lib.stream_ptr()), "vx_val_aleatoric_sums_batched")
    out = sums.cpu().numpy()
    if raise_invalid:
        _raise_invalid(out[:, 5 * C + 2].sum(), "val_sums_aleatoric")
    return out


def val_sums_ssn(head: torch.Tensor, target, num_classes: int, rank: int, n_samples: int = 10,
                 eps_w: Optional[torch.Tensor] = None, eps_d: Optional[torch.Tensor] = None, seed: int = 0, item0: int = 0,
                 epsilon: float = 1e-5, ignore_label: Optional[int] = None, raise_invalid: bool = True):
    """head (B, (2 + R)C, *spatial) in vx_ssn_sample's layout (LowRankNormal.head; rank 0: the mean_only head of 2C planes),
    eps_w (S, B, R) / eps_d (S, B, C * voxels) injected normals or None (generated from seed, keyed by item0 + b)
    -> sample_sums (B, S, 1 + 2C): sum_v log_softmax(y_s)[t], tp_c, pred_c;  target_sums (B, C + 2): sum [t = c], the count
    of voxels that take a log term, the invalid count."""
    _lib.require_gpu()
    lib = _lib.load()
    ig = _check_ignore(ignore_label)
    C, R, S = int(num_classes), int(rank), int(n_samples)
    if head.dim() < 2 or head.shape[1] != (2 + R) * C:
        raise ValueError(f"val_sums_ssn: head (B, {(2 + R) * C}, *spatial) expected, got {tuple(head.shape)}")
    B = int(head.shape[0])
    h = head.reshape(B, (2 + R) * C, -1).to(torch.float32).contiguous()
    nvox = int(h.shape[2])
    g = _labels_u8(target, h.device, B, nvox, ig)
    ew = ed = None
    if eps_w is not None and R:
        ew = eps_w.to(device=h.device, dtype=torch.float32).contiguous()
        if ew.numel() != S * B * R:
            raise ValueError(f"val_sums_ssn: eps_w of {tuple(eps_w.shape)} for (S, B, R) = {(S, B, R)}")
    if eps_d is not None:
        ed = eps_d.to(device=h.device, dtype=torch.float32).contiguous()
        if ed.numel() != S * B * C * nvox:
            raise ValueError(f"val_sums_ssn: eps_d of {tuple(eps_d.shape)} for (S, B, C * voxels) = {(S, B, C * nvox)}")
    ss = torch.empty((B, S, 1 + 2 * C), dtype=torch.float64, device=h.device)
    ts = torch.empty((B, C + 2), dtype=torch.float64, device=h.device)
    ws = _lib.workspace(h.device, int(lib.vx_val_ssn_sums_workspace_bytes(B, S, C, nvox)))
    _lib.check(lib.vx_val_ssn_sums_batched(h.data_ptr(), _lib.ptr(ew), _lib.ptr(ed), int(seed) & 0xFFFFFFFF, int(item0) & 0xFFFFFFFF,
                                           g.data_ptr(), B, S, C, R, nvox, float(epsilon), ig, ss.data_ptr(), ts.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "vx_val_ssn_sums_batched")
    ss, ts = ss.cpu().numpy(), ts.cpu().numpy()
    if raise_invalid:
        _raise_invalid(ts[:, C + 1].sum(), "val_sums_ssn")
    return ss, ts


def val_sums_ssn2d(dist, target, n_samples: int = 10, eps_w: Optional[torch.Tensor] = None, eps_d: Optional[torch.Tensor] = None,
                   seed: Optional[int] = None, item0: int = 0, ignore_label: Optional[int] = None, raise_invalid: bool = True):
    """dist: the LowRankNormal2D of an SSN HighResolutionNet (head at h0 x w0, image H x W); target (B, H, W) or (B, 1, H, W)
    integer labels; eps_w (S, B, R) / eps_d (S, B, C * H * W) injected normals or None (generated from seed, keyed by
    item0 + b; seed None: the distribution's next draw seed, the one sample_images would take)
    -> sample_sums (B, S, 1 + 2C), target_sums (B, C + 2) as val_sums_ssn, over the samples dist.sample_images(S) writes."""
    _lib.require_gpu()
    lib = _lib.load()
    ig = _check_ignore(ignore_label)
    lo = dist.lowres()
    C, R, S = int(dist.num_classes), int(dist.rank), int(n_samples)
    B, h0, w0, H, W = (int(lo[k]) for k in ("B", "h0", "w0", "H", "W"))
    mean, fac = lo["mean"], lo["factor"]
    dev = mean.device
    if seed is None:
        seed = dist.next_seed()
    g = _labels_u8(target, dev, B, H * W, ig)
    ew = ed = None
    if eps_w is not None and R:
        ew = eps_w.to(device=dev, dtype=torch.float32).contiguous()
        if ew.numel() != S * B * R:
            raise ValueError(f"val_sums_ssn2d: eps_w of {tuple(eps_w.shape)} for (S, B, R) = {(S, B, R)}")
    if eps_d is not None:
        ed = eps_d.to(device=dev, dtype=torch.float32).contiguous()
        if ed.numel() != S * B * C * H * W:
            raise ValueError(f"val_sums_ssn2d: eps_d of {tuple(eps_d.shape)} for (S, B, C * H * W) = {(S, B, C * H * W)}")
    ss = torch.empty((B, S, 1 + 2 * C), dtype=torch.float64, device=dev)
    ts = torch.empty((B, C + 2), dtype=torch.float64, device=dev)
    ws = _lib.workspace(dev, int(lib.vx_val_ssn2d_sums_workspace_bytes(B, S, C, h0, w0, H, W)))
    _lib.check(lib.vx_val_ssn2d_sums_batched(mean.data_ptr(), int(lo["mean_pitch"]), _lib.ptr(fac), int(lo["factor_pitch"]), _lib.ptr(ew),
                                             _lib.ptr(ed), int(seed) & 0xFFFFFFFF, int(item0) & 0xFFFFFFFF, g.data_ptr(), B, S, C, R, h0, w0,
                                             H, W, float(dist.epsilon), ig, ss.data_ptr(), ts.data_ptr(), ws.data_ptr(), ws.numel(),
                                             _lib.stream_ptr()), "vx_val_ssn2d_sums_batched")
    ss, ts = ss.cpu().numpy(), ts.cpu().numpy()
    if raise_invalid:
        _raise_invalid(ts[:, C + 1].sum(), "val_sums_ssn2d")
    return ss, ts


# ---- host arithmetic --------------------------------------------------------------------------------------------------------------
def ce_ignore_label(ignore_index: int) -> int:
    """the label the cross-entropy ignores: the reference calls it WITHOUT ignore_index when ignore_index == 0"""
    return -1 if ignore_index == 0 else int(ignore_index)


def _dice_from_counts(tp, pred, tgt, C: int, ignore_index: int) -> float:
    """micro Dice of a prediction against a target from their per-class counts, through metrics._micro_dice: the agreement
    counts of the two masks are I[p][p] = pred, I[t][t] = tgt, I[p][t] = tp"""
    I = np.zeros((2, 2, C), dtype=np.int64)
    I[0, 0], I[1, 1] = np.rint(pred).astype(np.int64), np.rint(tgt).astype(np.int64)
    I[0, 1] = I[1, 0] = np.rint(tp).astype(np.int64)
    return _micro_dice(I, [0], [1], _classes(C, ignore_index))


def loss_dice_from_sums(sums: np.ndarray, C: int, ignore_index: int = 0, aleatoric: bool = False):
    """sums (B, 5C + 3) of one batch -> (val_loss, val_dice) of the deterministic (or, aleatoric=True, the aleatoric) branch"""
    sums = np.asarray(sums, dtype=np.float64)
    B = sums.shape[0]
    cls = sums[:, :5 * C].reshape(B, C, 5)
    inter, cnt, psum, tp, pred = (cls[:, :, k] for k in range(5))
    lsum, nval = float(sums[:, 5 * C].sum()), float(sums[:, 5 * C + 1].sum())
    ce = -lsum / nval if nval else float("nan")     # mean over the voxels that take a log term; none: nan, as torch
    if ignore_index == 0 or aleatoric:
        loss = float(np.mean(-((2.0 * inter + _SMOOTH) / ((psum + cnt) + _SMOOTH)))) + ce
    else:
        loss = ce
    return loss, _dice_from_counts(tp.sum(0), pred.sum(0), cnt.sum(0), C, ignore_index)


def ssn_loss_dice_from_sums(sample_sums: np.ndarray, target_sums: np.ndarray, C: int, ignore_index: int = 0):
    """sample_sums (B, S, 1 + 2C), target_sums (B, C + 2) -> (val_loss, val_dice) of forward_ssn(val=True):
    loss = -mean_b(logsumexp_s ll[b][s] - log S); val_dice = the mean of the S per-sample Dice values over the whole batch"""
    ss, ts = np.asarray(sample_sums, dtype=np.float64), np.asarray(target_sums, dtype=np.float64)
    S = ss.shape[1]
    ll = ss[:, :, 0]
    mx = ll.max(1, keepdims=True)
    loss = -float(np.mean(mx[:, 0] + np.log(np.exp(ll - mx).sum(1)) - math.log(S)))
    tgt = ts[:, :C].sum(0)
    dice = [_dice_from_counts(ss[:, s, 1:1 + C].sum(0), ss[:, s, 1 + C:].sum(0), tgt, C, ignore_index) for s in range(S)]
    return loss, float(np.mean(np.array(dice)))


# ---- the step -----------------------------------------------------------------------------------------------------------------------
def validation_step(model, data: torch.Tensor, seg, n_aleatoric_samples: int = 10, ignore_index: int = 0,
                    mean_only: bool = False, seed: Optional[int] = None, eps=None) -> Dict[str, float]:
    """LightningExperiment.validation_step for one batch: data (B, Cin, *spatial), seg (B, 1, *spatial) or (B, *spatial)
    integer labels -> {"validation/val_loss", "validation/val_dice"}.  Dispatch as the reference (:290-330): an SsnUNet3D
    or a model with `ssn` set (the 2D HighResolutionNet, which returns a LowRankNormal2D) takes the SSN branch (mean_only:
    the pretraining epochs' rank-0 distribution), a model with aleatoric_loss the aleatoric one, anything else that returns
    logits (B, C, *spatial) the plain one.
    eps: the standard normals, for parity -- aleatoric: (B, T, C, *spatial); SSN: (eps_w (S, B, R), eps_d (S, B, C * voxels))
    (either may be None; 2D: eps_d (S, B, C * H * W)); None: generated on the device from seed (None: the model's next
    seed; 2D: the distribution's)."""
    from .ssn import SsnUNet3D
    _lib.require_gpu()
    ignore_index = int(ignore_index)
    ce_ig = ce_ignore_label(ignore_index)
    if isinstance(model, SsnUNet3D):
        dist = model(data, mean_only=mean_only)
        if seed is None:
            seed = model.next_seed()
        ew, ed = eps if eps is not None else (None, None)
        ss, ts = val_sums_ssn(dist.head, seg, dist.num_classes, dist.rank, n_aleatoric_samples, ew, ed, seed, 0, dist.epsilon, ce_ig)
        loss, dice = ssn_loss_dice_from_sums(ss, ts, dist.num_classes, ignore_index)
    elif getattr(model, "ssn", False):
        from .hrnet import LowRankNormal2D
        dist = model(data, mean_only=mean_only)
        if not isinstance(dist, LowRankNormal2D):
            raise NotImplementedError("validation_step: a model with `ssn` set must return a values_amd.hrnet.LowRankNormal2D (the 2D "
                                      f"HighResolutionNet's SSN head), got {type(dist).__name__}")
        ew, ed = eps if eps is not None else (None, None)
        ss, ts = val_sums_ssn2d(dist, seg, n_aleatoric_samples, ew, ed, seed, 0, ce_ig)
        loss, dice = ssn_loss_dice_from_sums(ss, ts, dist.num_classes, ignore_index)
    elif getattr(model, "aleatoric_loss", False):
        mu, s = model(data)
        if seed is None:
            seed = model.next_seed() if hasattr(model, "next_seed") else 0
        mu_s = torch.cat([mu, s], 1)
        C = int(mu.shape[1])
        sums = val_sums_aleatoric(mu_s, seg, n_aleatoric_samples, eps, seed, 0, None)   # nll_loss: nothing is ignored
        loss, dice = loss_dice_from_sums(sums, C, ignore_index, aleatoric=True)
    else:
        out = model(data.float())
        if not isinstance(out, torch.Tensor) or out.dim() < 3:
            raise ValueError("validation_step: the model must return logits (B, C, *spatial)")
        C = int(out.shape[1])
        sums = val_sums(out, seg, ce_ig)
        loss, dice = loss_dice_from_sums(sums, C, ignore_index)
    return {"validation/val_loss": float(loss), "validation/val_dice": float(dice)}


def validate(model, batches: Iterable, **kw) -> Dict:
    """validation_step over batches -- each (data, seg) or {"data", "seg"} -- and Lightning's on_epoch means, weighted by
    batch size: {"validation/val_loss", "validation/val_dice", "batches": [the per-batch dicts]}"""
    per, sizes = [], []
    for batch in batches:
        data, seg = (batch["data"], batch["seg"]) if isinstance(batch, dict) else batch
        per.append(validation_step(model, data, seg, **kw))
        sizes.append(int(data.shape[0]))
    out = {"batches": per}
    w = np.array(sizes, dtype=np.float64)
    for k in ("validation/val_loss", "validation/val_dice"):
        out[k] = float((np.array([p[k] for p in per]) * w).sum() / w.sum()) if per else float("nan")
    return out


def validate_split(model, datamodule_or_loader, **kw) -> Dict:
    """The validation epoch from a directory: validate() over the validation loader of a values_amd.datamodule3d
    datamodule (its val_dataloader(); setup() must have run) or over a loader given as such.  A host loader's numpy
    batches go to the model's device first."""
    loader = datamodule_or_loader.val_dataloader() if hasattr(datamodule_or_loader, "val_dataloader") else datamodule_or_loader
    dev = next(model.parameters()).device

    def batches():
        for b in loader:
            data = b["data"] if isinstance(b["data"], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(b["data"])).to(dev)
            yield data, b["seg"]

    return validate(model, batches(), **kw)
