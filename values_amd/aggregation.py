"""Map -> scalar aggregations on MI355X; same names / arguments / return dicts as
evaluation/uncertainty_aggregation/aggregate_uncertainties.py:13-67, so the hydra `_target_`
strings of evaluation/configs/tasks/aggregation_*.yaml can be re-pointed here.
"""
from __future__ import annotations

import json

import numpy as np
import torch

from . import _lib


def patch_level_aggregation(image, patch_size, mean=False, **kwargs):
    return _one(image, "patch", {"patch_size": patch_size, "mean": mean})


def image_level_aggregation(image, mean=False, **kwargs):
    return _one(image, "image", {"mean": mean})  # the reference returns a bare float for mean=True (:35-36)


def threshold_aggregation(image, threshold=None, threshold_path=None, pred_model=None, unc_type=None, mean=True):
    threshold = _threshold(threshold, threshold_path, pred_model, unc_type, {})
    return _one(image, "threshold", {"threshold": threshold, "mean": mean})


def _threshold(threshold, threshold_path, pred_model, unc_type, files):
    """the threshold of a threshold_aggregation call: as given, or from the json file (read once per `files` dict); the
    reference's order of checks and messages (:40-59)"""
    if threshold is None:
        if threshold_path is None:
            raise Exception("A threshold needs to be provided for threshold aggregation!")
        if threshold_path not in files:
            with open(threshold_path) as f:
                files[threshold_path] = json.load(f)
        if pred_model is None or unc_type is None:
            raise Exception("If you want to load the threshold from a json file, you have to provide the prediction "
                            "model and the uncertainty type")
        unc_type_split = unc_type.split("_")[0]
        threshold = files[threshold_path][pred_model][f"Mean {unc_type_split} threshold"]
    return threshold


# ---------------------------------------------------------------------------------------------------------------------
# One device path: a list of maps and a plan [(name, kind, params)] -> one vx_aggregate_batched call and one device ->
# host copy per chunk.  The three functions above are a plan of one entry for a batch of one map.

_REF_MODULES = ("evaluation.uncertainty_aggregation.aggregate_uncertainties", "uncertainty_aggregation.aggregate_uncertainties")
_KINDS = {"image_level_aggregation": "image", "threshold_aggregation": "threshold", "patch_level_aggregation": "patch"}


def register_targets():
    """the reference's `_target_` spellings of the three functions -> this module's, in io.TARGET_MAP"""
    from .io import TARGET_MAP
    for mod in _REF_MODULES:
        for fn in _KINDS:
            TARGET_MAP.setdefault(f"{mod}.{fn}", "values_amd.aggregation." + fn)
    return TARGET_MAP


def _plan(aggregations, pred_model=None, unc_type=None):
    """[(name, kind, params)] for an aggregations dict: kind "image" / "threshold" / "patch" with the arguments the
    per-image function would receive (a threshold file is read here, once per file), or "foreign" with the config for any
    other `_target_`.  Needs no device."""
    target_map = register_targets()
    files, plan = {}, []
    for name, cfg in aggregations.items():
        params = dict(cfg)
        target = params.pop("_target_")
        target = target_map.get(target, target)
        mod, _, fn = target.rpartition(".")
        if mod != "values_amd.aggregation" or fn not in _KINDS:
            plan.append((name, "foreign", dict(cfg)))
            continue
        params.pop("_partial_", None)
        params.update(pred_model=pred_model, unc_type=unc_type)
        kind = _KINDS[fn]
        if kind == "image":
            plan.append((name, kind, {"mean": params.get("mean", False)}))
        elif kind == "patch":
            if "patch_size" not in params:
                raise TypeError("patch_level_aggregation() missing 1 required positional argument: 'patch_size'")
            plan.append((name, kind, {"patch_size": params["patch_size"], "mean": params.get("mean", False)}))
        else:
            extra = set(params) - {"threshold", "threshold_path", "pred_model", "unc_type", "mean"}
            if extra:
                raise TypeError(f"threshold_aggregation() got an unexpected keyword argument {sorted(extra)[0]!r}")
            threshold = _threshold(params.get("threshold"), params.get("threshold_path"), pred_model, unc_type, files)
            plan.append((name, kind, {"threshold": threshold, "mean": params.get("mean", True)}))
    return plan


def _patch_of(patch_size, ndim):
    """patch_level_aggregation's patch list for a map of rank ndim (an int expands to the rank)"""
    if type(patch_size) == int:
        patch_size = ndim * [patch_size]
    if ndim not in (2, 3):
        raise ValueError("patch_level_aggregation: 2D or 3D maps only")
    if len(patch_size) != ndim:
        raise ValueError(f"patch_level_aggregation: patch_size {list(patch_size)} for a map of rank {ndim}")
    return patch_size


def _specs_for(plan, ndim):
    """(specs, index): the distinct device specs (kind, pd, ph, pw, thr) the plan needs for maps of rank ndim, and for every
    plan entry the position of its spec (None for a foreign entry)"""
    specs, index = [], []
    for _, kind, params in plan:
        if kind == "foreign":
            index.append(None)
            continue
        if kind == "image":
            spec = (_lib.VX_AGG_IMAGE, 1, 1, 1, 0.0)
        elif kind == "threshold":
            spec = (_lib.VX_AGG_THRESHOLD, 1, 1, 1, float(params["threshold"]))
        else:
            patch = (1,) * (3 - ndim) + tuple(int(p) for p in _patch_of(params["patch_size"], ndim))
            spec = (_lib.VX_AGG_PATCH,) + patch + (0.0,)
        if spec not in specs:
            specs.append(spec)
        index.append(specs.index(spec))
    return specs, index


def _assemble(plan, index, rows, shape):
    """{name: result} of one map of `shape` from its device rows ([n_specs][4] floats), as the per-image functions return
    them; foreign entries are left to the caller (None)"""
    res = {}
    for (name, kind, params), si in zip(plan, index):
        if kind == "foreign":
            res[name] = None
        elif kind == "image":
            s = rows[si][0]
            res[name] = float(s / int(np.prod(shape, dtype=np.int64))) if params["mean"] else {"max_score": float(s)}
        elif kind == "threshold":
            st, ct = rows[si][0], rows[si][1]
            res[name] = {"max_score": st / ct if params["mean"] and ct > 0 else st, "threshold": params["threshold"]}
        else:
            patch_size = _patch_of(params["patch_size"], len(shape))
            mx = float(rows[si][0])
            first = [int(v) for v in rows[si][1:]][3 - len(shape):]
            if params["mean"]:
                mx = mx / float(np.prod(patch_size))
            res[name] = {"max_score": mx, "bounding_box": [(int(i), int(i + patch_size[d])) for d, i in enumerate(first)]}
    return res


def _dhw(shape):
    if len(shape) in (2, 3):
        return (1,) * (3 - len(shape)) + tuple(shape)
    if len(shape) < 2:
        return (1, 1, int(np.prod(shape, dtype=np.int64)))
    return (int(np.prod(shape[:-2], dtype=np.int64)), shape[-2], shape[-1])


def _copy_bytes(image):
    """bytes of the device copy _to_device makes of a map (0: it is used where it lies)"""
    if isinstance(image, np.ndarray):
        return image.size * (8 if image.dtype == np.float64 else 4)
    f64 = image.dtype == torch.float64
    if image.is_cuda and image.is_contiguous() and image.dtype in (torch.float32, torch.float64):
        return 0
    return image.numel() * (8 if f64 else 4)


def _to_device(image, dev):
    """the per-image functions' conversion: a float64 map stays float64, anything else becomes float32; contiguous"""
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image))
    return image.to(dev, torch.float64 if image.dtype == torch.float64 else torch.float32).contiguous()


def _item(t_ptr, f64, shape):
    d, h, w = _dhw(shape)
    return _lib.AggItem(t_ptr, _lib.VX_F64 if f64 else _lib.VX_F32, d, h, w)


def _spec_array(specs):
    return (_lib.AggSpec * max(len(specs), 1))(*[_lib.AggSpec(*s) for s in specs])


def _chunks(images, plan, lib, budget_bytes):
    """([(rank, [image numbers])], {rank: _specs_for(plan, rank)}): consecutive maps of one rank, at most VX_AGG_MAX_ITEMS; a
    chunk ends where the device copies of its maps plus their calls' workspaces would pass budget_bytes.  One map is one
    chunk and asks the library nothing."""
    rank = len(images[0].shape)
    if len(images) == 1:
        return [(rank, [0])], {rank: _specs_for(plan, rank)}
    by_rank, chunks, used = {}, [], 0
    for i, im in enumerate(images):
        shape = tuple(im.shape)
        if len(shape) not in by_rank:
            by_rank[len(shape)] = _specs_for(plan, len(shape))
        specs, _ = by_rank[len(shape)]
        dhw = _dhw(shape)
        for s in specs:
            if s[0] == _lib.VX_AGG_PATCH and any(p > n for p, n in zip(s[1:4], dhw)):
                raise _lib.VxError(f"aggregate_batch: image {i}: patch {s[1:4]} must fit map {dhw}")
        one = _item(0x100, False, shape)      # (the size query reads no map)
        need = _copy_bytes(im) + int(lib.vx_aggregate_workspace_bytes(one, 1, _spec_array(specs), len(specs)))
        if not chunks or len(chunks[-1][1]) == _lib.VX_AGG_MAX_ITEMS or chunks[-1][0] != len(shape) or used + need > budget_bytes:
            chunks.append((len(shape), []))
            used = 0
        chunks[-1][1].append(i)
        used += need
    return chunks, by_rank


def _run(images, plan, budget_bytes=1 << 30):
    """[{name: result}] of a plan's device entries for a list of maps (a foreign entry: None)"""
    if all(kind == "foreign" for _, kind, _ in plan):
        return [{name: None for name, _, _ in plan} for _ in images]
    _lib.require_gpu()
    lib = _lib.load()
    dev = next((im.device for im in images if not isinstance(im, np.ndarray) and im.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))
    chunks, by_rank = _chunks(images, plan, lib, budget_bytes)
    results = [None] * len(images)
    with torch.cuda.device(dev):
        for rank, members in chunks:
            specs, index = by_rank[rank]
            maps = [_to_device(images[i], dev) for i in members]
            # (an empty map has no storage: the pointer stands in, so that the library refuses the shape and not a null map)
            items = (_lib.AggItem * len(maps))(*[_item(t.data_ptr() or 0x100, t.dtype == torch.float64, tuple(t.shape)) for t in maps])
            sp = _spec_array(specs)
            need = int(lib.vx_aggregate_workspace_bytes(items, len(maps), sp, len(specs)))
            ws = _lib.workspace(dev, need)
            out = torch.empty((len(maps), len(specs), 4), dtype=torch.float64, device=dev)
            rc = lib.vx_aggregate_batched(items, len(maps), sp, len(specs), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr())
            _lib.check(rc, "vx_aggregate_batched")
            for i, r in zip(members, out.cpu().tolist()):
                results[i] = _assemble(plan, index, r, tuple(images[i].shape))
    return results


def _one(image, kind, params):
    return _run([image], [("r", kind, params)])[0]["r"]


def aggregate_batch(images, aggregations, pred_model=None, unc_type=None, budget_bytes=1 << 30):
    """[{name: result}] for a list of maps (numpy arrays or tensors, host or device; shapes and dtypes may differ) and an
    aggregations dict {name: {"_target_": ..., **params}}: entry i equals what the three functions above return for
    images[i].  One vx_aggregate_batched call and one device -> host copy per chunk of consecutive maps of one rank; a chunk
    ends where the device copies of its maps plus the call's workspace would pass budget_bytes.  A threshold file is read
    once per call.  A config with any other `_target_` is evaluated per image with io.instantiate."""
    from .io import instantiate
    images = list(images)
    if not images:
        return []
    plan = _plan(aggregations, pred_model, unc_type)
    results = _run(images, plan, budget_bytes)
    for name, kind, cfg in plan:
        if kind == "foreign":
            for i, im in enumerate(images):
                results[i][name] = instantiate(dict(cfg), image=im, pred_model=pred_model, unc_type=unc_type)
    return results
