"""Threshold search for the threshold aggregation (evaluation/uncertainty_aggregation/find_threshold.py).

Same function names and JSON files as the reference script:
    quantile_analysis.json   {pred_model: mean over images and versions of 1 - foreground / size of pred_seg}
    threshold_analysis.json  {pred_model: {"Mean <unc> threshold": quantile of ALL its validation maps}, "Mean": ...}
(`threshold_aggregation` reads "Mean {predictive|aleatoric|epistemic} threshold", aggregate_uncertainties.py:59-60).

np.quantile over every voxel of every validation map is a selection problem on tens of millions of floats; here the
two order statistics around q * (n - 1) come from ONE `vx_select_segments` call (radix select on the device, over the maps
where they lie) and numpy's linear interpolation (`_lerp`, method="linear") is applied to them in float64 with a float64
virtual index -- what numpy 1.24.3 (the reference's pin, requirements.txt:48) computes for a python-float q, and
bit-identical to np.quantile(maps.astype(float64), q) on any numpy.  (numpy >= 2 rounds q, the index and the interpolation
to float32 when the data are float32; the two differ in the 8th digit.)

The device drivers work on whole reader batches: `get_foreground_quantile_device` counts a batch of predicted masks with
one `vx_count_nonzero_batched` call (`count_nonzero_batch`), and `find_threshold(device_io=True)` selects from the maps
where the readers left them (`quantile_segments`: no concatenation, no float32 copy; NIfTI volumes and the 2D tree's TIFF
maps alike).  `quantile` / `count_nonzero` are the single-array forms: a batch of one.

Note on the reference: `find_threshold` calls `calculate_threshold_image(np.array(unc_images), pred_model)` although
the function is defined as `(quantile_path, image, method)` (find_threshold.py:61-66 vs :93) -- as shipped it raises
a TypeError.  This module implements what the two pieces say together: threshold = quantile of the stacked maps at
the model's foreground quantile read from quantile_analysis.json.
"""
from __future__ import annotations

import json
import os
from itertools import chain
from pathlib import Path
from typing import Dict, Iterable

import numpy as np
import torch

from . import _lib, nifti
from .experiment import _read_batches_device


def count_nonzero(mask: torch.Tensor) -> int:
    return count_nonzero_batch([mask])[0]


_dense_block = _lib.dense_block


_COUNT_KINDS = {torch.bool: _lib.VX_COUNT_B1, torch.uint8: _lib.VX_COUNT_B1, torch.int8: _lib.VX_COUNT_B1,
                torch.int16: _lib.VX_COUNT_B2, torch.int32: _lib.VX_COUNT_B4, torch.int64: _lib.VX_COUNT_B8,
                torch.float32: _lib.VX_COUNT_F32, torch.float64: _lib.VX_COUNT_F64}


def count_nonzero_batch(masks) -> list:
    """[np.count_nonzero(m) for m in masks] for device tensors of any integer, bool, float32 or float64 dtype and any
    shape: one vx_count_nonzero_batched call and one device -> host copy per VX_SELECT_MAX_ITEMS masks."""
    masks = list(masks)
    if not masks:
        return []
    _lib.require_gpu()
    lib = _lib.load()
    dev = masks[0].device
    blocks = []
    for m in masks:
        if not m.is_cuda:
            raise ValueError("count_nonzero_batch: device tensors only")
        if m.dtype not in _COUNT_KINDS:
            m = (m != 0).to(torch.uint8)
        blocks.append(_dense_block(m))
    out = []
    with torch.cuda.device(dev):
        for i in range(0, len(blocks), _lib.VX_SELECT_MAX_ITEMS):
            part = blocks[i:i + _lib.VX_SELECT_MAX_ITEMS]
            items = (_lib.CountItem * len(part))(*[_lib.CountItem(t.data_ptr() if t.numel() else None, t.numel(),
                                                                  _COUNT_KINDS[t.dtype], 0) for t in part])
            ws = _lib.workspace(dev, int(lib.vx_count_nonzero_batched_workspace_bytes(len(part))))
            counts = torch.empty(len(part), dtype=torch.int64, device=dev)
            _lib.check(lib.vx_count_nonzero_batched(items, len(part), _lib.ptr(counts), _lib.ptr(ws), ws.numel(),
                                                    _lib.stream_ptr()), "vx_count_nonzero_batched")
            out += counts.cpu().tolist()
    return out


def calculate_foreground_quantile_image(image) -> float:
    """find_threshold.py:11-13"""
    t = image if isinstance(image, torch.Tensor) else torch.as_tensor(np.asarray(image))
    if not t.is_cuda:
        _lib.require_gpu()
        t = t.cuda()
    return 1 - (count_nonzero(t) / t.numel())


def quantile(values: torch.Tensor, q: float) -> float:
    """np.quantile(values, q) (method='linear') of a tensor of any shape: quantile_segments over the one tensor.  A host
    tensor goes up to the device; a dtype other than float32 / float64 is cast to float32, float64 is narrowed on load."""
    _lib.require_gpu()
    return quantile_segments([values], q)


def _lerp(a, b, gamma: float) -> float:
    """numpy's _lerp (method="linear") of two order statistics in float64"""
    a, b = np.float64(a), np.float64(b)
    diff = b - a
    res = a + diff * gamma
    if gamma >= 0.5:
        res = b - diff * (1 - gamma)
    return float(res)


def quantile_segments(tensors, q: float) -> float:
    """np.quantile(np.concatenate([t.ravel() for t in tensors]).astype(float32), q) (method='linear') of device tensors
    where they lie: one vx_select_segments call over all of them -- float32 and float64 tensors are read in place, the
    latter narrowed on load -- and one host copy of the two order statistics and the status.  NaN anywhere: nan."""
    if not 0.0 <= q <= 1.0:
        raise ValueError("Quantiles must be in the range [0, 1]")
    tensors = [t for t in tensors if t.numel()]
    n = sum(t.numel() for t in tensors)
    if n == 0:
        raise ValueError("quantile of an empty array")
    if len(tensors) > _lib.VX_SELECT_MAX_ITEMS:
        raise ValueError(f"quantile_segments: more than {_lib.VX_SELECT_MAX_ITEMS} tensors")
    _lib.require_gpu()
    lib = _lib.load()
    dev = next((t.device for t in tensors if t.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    blocks = []
    for t in tensors:
        if not t.is_cuda:
            t = t.to(dev)
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float32)
        blocks.append(_dense_block(t))
    virt = q * (n - 1)                      # numpy: _compute_virtual_index(n, q, alpha=1, beta=1)
    lo = int(np.floor(virt))
    gamma = virt - lo
    with torch.cuda.device(dev):
        items = (_lib.SelectItem * len(blocks))(*[_lib.SelectItem(t.data_ptr(), t.numel(), _lib.VX_F64 if t.dtype == torch.float64
                                                                  else _lib.VX_F32, 0) for t in blocks])
        ws = _lib.workspace(dev, int(lib.vx_select_segments_workspace_bytes(len(blocks))))
        res = torch.empty(3, dtype=torch.int32, device=dev)       # two float32 order statistics, then the status
        _lib.check(lib.vx_select_segments(items, len(blocks), lo, _lib.ptr(res), res.data_ptr() + 8, _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr()), "vx_select_segments")
        host = res.cpu().numpy()
    if int(host[2]) == _lib.VX_SELECT_NAN:
        return float("nan")
    a, b = host[:2].view(np.float32)
    return _lerp(a, b, gamma)


def get_foreground_quantile(exp_dataloader) -> Dict:
    """find_threshold.py:16-29"""
    all_quantiles = []
    for image_id in exp_dataloader.image_ids:
        for pred_seg in exp_dataloader.get_pred_segs(image_id):
            img = pred_seg if isinstance(pred_seg, torch.Tensor) else np.asarray(pred_seg)   # device tensors: DeviceExperimentDataloader
            all_quantiles.append(calculate_foreground_quantile_image(img))
    return {exp_dataloader.exp_version.pred_model: {exp_dataloader.exp_version.version_name: all_quantiles}}


def get_foreground_quantile_device(exp_dataloader, batch: int = 32) -> Dict:
    """get_foreground_quantile with the predicted masks read by the pipelined device readers, `batch` files per reader
    call, and counted with one count_nonzero_batch call per reader batch.  The same dict, the list in the same order:
    image ids in order, for each the paths get_pred_seg_paths returns (save_foreground_quantiles takes a float mean of
    the list, and that mean depends on the order)."""
    order = [str(p) for image_id in exp_dataloader.image_ids for p in exp_dataloader.get_pred_seg_paths(image_id)]
    value, pending = {}, []

    def flush():
        for (p, t), c in zip(pending, count_nonzero_batch([t for _, t in pending])):
            value[p] = 1 - (c / t.numel())
        pending.clear()

    for p, t in _read_batches_device(list(dict.fromkeys(order)), batch):
        pending.append((p, t))
        if len(pending) == batch:
            flush()
    if pending:
        flush()
    ev = exp_dataloader.exp_version
    return {ev.pred_model: {ev.version_name: [value[p] for p in order]}}


def save_foreground_quantiles(results_dict: Dict, save_path) -> Dict:
    """find_threshold.py:32-41"""
    methods = {m: float(np.mean(list(chain.from_iterable(v.values())))) for m, v in results_dict.items()}
    if not os.path.isfile(save_path):
        save_path = Path(save_path) / "quantile_analysis.json"
    with open(save_path, "w") as f:
        json.dump(methods, f, indent=2)
    return methods


def threshold_images_paths(exp_dataloader) -> Dict:
    """find_threshold.py:44-58"""
    ev = exp_dataloader.exp_version
    d = {ev.pred_model: {ev.version_name: {}}}
    for unc_type in ev.unc_types:
        p = exp_dataloader.unc_path_dict[unc_type]
        d[ev.pred_model][ev.version_name][unc_type] = [p / f"{i}{ev.unc_ending}" for i in exp_dataloader.image_ids]
    return d


def calculate_threshold_image(quantile_path, image, method: str) -> float:
    """find_threshold.py:61-66; `image`: array / device tensor / iterable of maps (stacked).  A list or tuple of device
    tensors is selected from where the tensors lie (quantile_segments)."""
    with open(quantile_path) as f:
        all_quantiles = json.load(f)
    if isinstance(image, (list, tuple)) and image and all(isinstance(i, torch.Tensor) and i.is_cuda for i in image):
        return quantile_segments(image, all_quantiles[method])
    if isinstance(image, torch.Tensor):
        t = image
    elif isinstance(image, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(image))
    else:
        t = torch.cat([torch.as_tensor(np.asarray(i)).reshape(-1) for i in image])
    return quantile(t, all_quantiles[method])


def find_threshold(results_dict: Dict, quantile_path, save_path, loader=None, device_io: bool = False,
                   batch: int = 64) -> Dict:
    """find_threshold.py:69-117.  results_dict: {pred_model: {version: {unc_type: [paths]}}} (threshold_images_paths,
    merged over versions).  Maps are read with the package's NIfTI reader unless `loader(path) -> array` is given;
    device_io=True reads every kind of results file (NIfTI volumes, TIFF maps) with the pipelined device readers, `batch`
    files per call, and selects from the tensors as read -- no concatenation, no float32 copy -- with one
    quantile_segments call per (pred model, uncertainty type): the same thresholds."""
    if not os.path.isfile(quantile_path):
        quantile_path = Path(quantile_path) / "quantile_analysis.json"
    if not os.path.isfile(save_path):
        save_path = Path(save_path) / "threshold_analysis.json"
    load = loader or (lambda p: nifti.load(p)[0])
    per_model = {}
    for pred_model, versions in results_dict.items():
        per_model[pred_model] = {}
        for _version, uncs in versions.items():
            for unc, paths in uncs.items():
                per_model[pred_model].setdefault(unc, []).extend(paths)
    threshold_dict = {}
    for pred_model, uncs in per_model.items():
        threshold_dict[pred_model] = {}
        for unc, paths in uncs.items():
            if device_io and loader is None:
                maps = [t for _, t in _read_batches_device(paths, batch)]
            else:
                maps = [np.asarray(load(p), dtype=np.float32) for p in paths]
            thr = calculate_threshold_image(quantile_path, maps, pred_model)
            threshold_dict[pred_model][f"Mean {unc.split('_')[0]} threshold"] = thr
    al, ep, pr = [], [], []
    for key, value in threshold_dict.items():
        if key != "Softmax":
            al.append(value["Mean aleatoric threshold"])
            ep.append(value["Mean epistemic threshold"])
        pr.append(value["Mean predictive threshold"])
    threshold_dict["Mean"] = {"Mean aleatoric threshold": float(np.mean(al)), "Mean epistemic threshold": float(np.mean(ep)),
                              "Mean predictive threshold": float(np.mean(pr))}
    with open(save_path, "w") as f:
        json.dump(threshold_dict, f, indent=2)
    return threshold_dict
