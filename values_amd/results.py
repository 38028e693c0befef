"""Results-directory writer: the tree DataCarrier3D.save_data / log_metrics produce
(uncertainty_modeling/data_carrier_3D.py:17-57, 181-391), fed from device tensors.

    <root>/<exp_name>/test_results/<version>/<split>/
        input/<id>.nii.gz                    gt_seg/<id>_<RR>.nii.gz
        pred_seg/<id>_mean.nii.gz, <id>_<NN>.nii.gz          (uint8 argmax; NN = 1-based prediction index)
        pred_prob/<id>_mean_<CC>.nii.gz, <id>_<NN>_<CC>.nii.gz   (float64 like the reference's numpy buffers)
        pred_entropy/, aleatoric_uncertainty/, epistemic_uncertainty/<id>.nii.gz   (float32 maps / clip(count,1))
        metrics.json
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from . import _devio, nifti


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def save_case(save_dir: str, image_id: str, softmax_pred, maps: Optional[Dict] = None, data=None, gt_seg=None,
              num_predictions=None, header=False) -> None:
    """softmax_pred: (T, C, X,Y,Z) probabilities (sums if num_predictions is given: divided by clip(count, 1) like
    data_carrier_3D.py:208-217); maps: pred_entropy / aleatoric_uncertainty / epistemic_uncertainty, already
    normalised."""
    sub = {k: os.path.join(save_dir, k) for k in ("input", "gt_seg", "pred_seg", "pred_prob")}
    for d in sub.values():
        os.makedirs(d, exist_ok=True)
    sm = _np(softmax_pred).astype(np.float64)
    if num_predictions is not None:
        sm = sm / np.clip(_np(num_predictions), 1, None)
    if data is not None:
        nifti.save(_np(data), os.path.join(sub["input"], f"{image_id}.nii.gz"), header)
    if gt_seg is not None:
        for r, g in enumerate(_np(gt_seg)):
            nifti.save(g, os.path.join(sub["gt_seg"], f"{image_id}_{str(r).zfill(2)}.nii.gz"), header)
    T, C = sm.shape[:2]
    if T > 1:  # data_carrier_3D.py:253-279
        mean = sm.mean(axis=0)
        nifti.save(np.argmax(mean, axis=0).astype(np.uint8), os.path.join(sub["pred_seg"], f"{image_id}_mean.nii.gz"), header)
        for c in range(C):
            nifti.save(mean[c], os.path.join(sub["pred_prob"], f"{image_id}_mean_{str(c + 1).zfill(2)}.nii.gz"), header)
    for t in range(T):  # :281-307
        tag = str(t + 1).zfill(2)
        nifti.save(np.argmax(sm[t], axis=0).astype(np.uint8), os.path.join(sub["pred_seg"], f"{image_id}_{tag}.nii.gz"), header)
        for c in range(C):
            nifti.save(sm[t, c], os.path.join(sub["pred_prob"], f"{image_id}_{tag}_{str(c + 1).zfill(2)}.nii.gz"), header)
    for k in ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty"):  # :323-371
        if maps and k in maps:
            os.makedirs(os.path.join(save_dir, k), exist_ok=True)
            nifti.save(_np(maps[k]), os.path.join(save_dir, k, f"{image_id}.nii.gz"), header)


class PlannedFile(NamedTuple):
    """One file of a case's results tree: path relative to save_dir, payload kind (vx_nifti_item kinds: "COPY", "PROB",
    "MEAN_PROB", "ARGMAX", "ARGMAX_MEAN"), source (("input",), ("gt_seg", r), ("prob", t, c), ("mean", c), ("seg", t),
    ("seg_mean",), ("map", name)), voxel shape and the numpy dtype the file stores."""
    path: str
    kind: str
    source: tuple
    shape: tuple
    dtype: np.dtype


def _shape_dtype(a):
    """(shape, dtype name) of a numpy array or a torch tensor without copying it"""
    if hasattr(a, "detach"):
        return tuple(a.shape), str(a.dtype).replace("torch.", "")
    a = np.asarray(a)
    return a.shape, a.dtype


def _np_dtype(d) -> np.dtype:
    return np.dtype("bool" if d == "bool" else d) if isinstance(d, str) else np.dtype(d)


def plan_case(image_id: str, softmax_pred, maps: Optional[Dict] = None, data=None, gt_seg=None) -> List[PlannedFile]:
    """The files save_case writes for these arguments, in its order: same names, the same T > 1 rule for the mean files,
    the same dtypes.  Host logic only: nothing is read but shapes and dtypes."""
    out = []
    if data is not None:
        shp, dt = _shape_dtype(data)
        out.append(PlannedFile(os.path.join("input", f"{image_id}.nii.gz"), "COPY", ("input",), shp, _file_dtype(dt)))
    if gt_seg is not None:
        shp, dt = _shape_dtype(gt_seg)
        for r in range(shp[0]):
            out.append(PlannedFile(os.path.join("gt_seg", f"{image_id}_{str(r).zfill(2)}.nii.gz"), "COPY", ("gt_seg", r),
                                   tuple(shp[1:]), _file_dtype(dt)))
    shp, _ = _shape_dtype(softmax_pred)
    T, C = shp[:2]
    vol = tuple(shp[2:])
    f64, u8 = np.dtype("float64"), np.dtype("uint8")
    if T > 1:
        out.append(PlannedFile(os.path.join("pred_seg", f"{image_id}_mean.nii.gz"), "ARGMAX_MEAN", ("seg_mean",), vol, u8))
        for c in range(C):
            out.append(PlannedFile(os.path.join("pred_prob", f"{image_id}_mean_{str(c + 1).zfill(2)}.nii.gz"), "MEAN_PROB",
                                   ("mean", c), vol, f64))
    for t in range(T):
        tag = str(t + 1).zfill(2)
        out.append(PlannedFile(os.path.join("pred_seg", f"{image_id}_{tag}.nii.gz"), "ARGMAX", ("seg", t), vol, u8))
        for c in range(C):
            out.append(PlannedFile(os.path.join("pred_prob", f"{image_id}_{tag}_{str(c + 1).zfill(2)}.nii.gz"), "PROB",
                                   ("prob", t, c), vol, f64))
    for k in ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty"):
        if maps and k in maps:
            shp, dt = _shape_dtype(maps[k])
            out.append(PlannedFile(os.path.join(k, f"{image_id}.nii.gz"), "COPY", ("map", k), shp, _file_dtype(dt)))
    return out


def _file_dtype(d) -> np.dtype:
    try:
        return nifti.file_dtype(_np_dtype(d))
    except TypeError:   # a torch dtype numpy has no name for (bfloat16, ...): not in the table
        return np.dtype("float64")


# ---------------------------------------------------------------------------------------------------------------------
# device results writer

_TORCH_OK = ("uint8", "int8", "int16", "int32", "int64", "float32", "float64", "uint16", "uint32", "uint64")


def _to_device(a, dev):
    """a torch tensor on `dev` holding the array (numpy, CPU or device tensor); numpy inputs go up as native-order bytes"""
    import torch
    if isinstance(a, torch.Tensor):
        return a.detach().to(dev)
    a = np.asarray(a)
    if not a.dtype.isnative:
        a = a.astype(a.dtype.newbyteorder("="))
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    if a.dtype.name in ("uint16", "uint32", "uint64"):
        a = a.view(a.dtype.name[1:])    # same bytes; the file dtype is decided from the plan
    if a.dtype.name not in _TORCH_OK:
        a = a.astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _copy_source(t, dtype: np.dtype):
    """(contiguous device tensor of the file's dtype with the voxels in an order the COPY kernel turns into Fortran
    order, X, Y, Z)"""
    import torch
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    name = str(t.dtype).replace("torch.", "")
    if name != dtype.name and not (dtype.name in ("uint16", "uint32", "uint64") and name == dtype.name[1:]):
        t = t.double()    # outside the NIfTI table (float16, bfloat16, ...): stored as float64 like nifti.save
    shp = tuple(t.shape)
    if len(shp) <= 3:
        X, Y, Z = (1,) * (3 - len(shp)) + shp
        return t.contiguous(), X, Y, Z
    # more than three axes: reverse them on the device; the kernel then copies in order
    return t.permute(*reversed(range(len(shp)))).contiguous(), 1, 1, int(np.prod(shp))


def _nifti_gzip(bufs, items, hints, zipped, dev, timing):
    """The NIfTI-and-gzip stage.  items: a NiftiItem table filled but for dst_off; hints: per item the stride hints of its
    payload; zipped: the indices of the items that become gzip members.  Places the payloads at 16-byte multiples, one
    vx_nifti_payload launch, places the members by gz.bound, one gz.encode_into over them and one read of their sizes ->
    ((payload buffer, its bytes), (member buffer, its bytes), per item ("gz" or "nii", offset in that buffer, size))."""
    import torch
    from . import _lib, gz
    lib = _lib.load()
    parts, off = [], 0
    for it in items:
        it.dst_off = off
        n = int(lib.vx_nifti_payload_bytes(C.byref(it)))
        parts.append(("nii", off, n))
        off += (n + 15) // 16 * 16
    payload = bufs.get("payload", off, dev)
    nws = bufs.get("nifti_ws", int(lib.vx_nifti_workspace_bytes(len(items))), dev)
    stages = _devio.Stages(timing)
    stages.mark()
    _lib.check(lib.vx_nifti_payload(items, len(items), _lib.ptr(payload), payload.numel(), _lib.ptr(nws), nws.numel(),
                                    _lib.stream_ptr()), "vx_nifti_payload")
    stages.mark()
    if not zipped:
        return (payload, off), (None, 0), parts
    slots, goff = [], 0
    for k in zipped:
        slots.append(goff)
        goff += gz.bound(parts[k][2])
    members = bufs.get("members", goff, dev)
    sizes = bufs.get("sizes", 8 * len(zipped), dev)[:8 * len(zipped)].view(torch.int64)
    gws = bufs.get("gzip_ws", gz.workspace_bytes([parts[k][2] for k in zipped]), dev)
    base = payload.data_ptr()
    gz.encode_into([(base + parts[k][1], parts[k][2], s, hints[k]) for k, s in zip(zipped, slots)], members, sizes, gws)
    stages.mark()
    host_sizes = sizes.cpu().tolist()      # synchronises the stream
    stages.add(("payload_ms", "encode_ms"), {"payload_bytes": sum(parts[k][2] for k in zipped)})
    for k, s, n in zip(zipped, slots, host_sizes):
        parts[k] = ("gz", s, n)
    return (payload, off), (members, max(s + n for s, n in zip(slots, host_sizes))), parts


def _encode_case(bufs, image_id, softmax_pred, maps, data, gt_seg, num_predictions, header, timing=None):
    """payload launch + encode launch + one D2H copy: -> (plan, host uint8 array, [(offset, size)])"""
    import torch
    from . import _lib, gz
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    plan = plan_case(image_id, softmax_pred, maps, data, gt_seg)
    sm = _to_device(softmax_pred, dev)
    if sm.dtype not in (torch.float32, torch.float64):
        sm = sm.double()
    sm = sm.contiguous()
    T, Cn = int(sm.shape[0]), int(sm.shape[1])
    vol = tuple(int(v) for v in sm.shape[2:])
    if len(vol) != 3:
        raise _lib.VxError(f"save_case_device: softmax_pred (T, C, X, Y, Z) expected, got {tuple(sm.shape)}")
    cnt = None
    if num_predictions is not None:
        cnt = _to_device(num_predictions, dev).double()
        while cnt.dim() > 3 and cnt.shape[0] == 1:
            cnt = cnt[0]
        try:
            cnt = torch.broadcast_to(cnt, vol)
        except RuntimeError:
            raise _lib.VxError(f"save_case_device: num_predictions {tuple(cnt.shape)} does not broadcast to {vol}")
        cnt = cnt.contiguous()
    keep = [sm, cnt]
    items = (_lib.NiftiItem * len(plan))()
    kinds = {"COPY": _lib.VX_NIFTI_COPY, "PROB": _lib.VX_NIFTI_PROB, "MEAN_PROB": _lib.VX_NIFTI_MEAN_PROB,
             "ARGMAX": _lib.VX_NIFTI_ARGMAX, "ARGMAX_MEAN": _lib.VX_NIFTI_ARGMAX_MEAN}
    dsrc = _to_device(data, dev) if data is not None else None
    gsrc = _to_device(gt_seg, dev) if gt_seg is not None else None
    for it, f in zip(items, plan):
        it.kind = kinds[f.kind]
        if f.kind == "COPY":
            src = dsrc if f.source[0] == "input" else gsrc[f.source[1]] if f.source[0] == "gt_seg" else \
                _to_device(maps[f.source[1]], dev)
            src, X, Y, Z = _copy_source(src, f.dtype)
            keep.append(src)
            it.src = src.data_ptr() if src.numel() else None
            it.esize = f.dtype.itemsize
        else:
            X, Y, Z = vol
            it.src = sm.data_ptr()
            it.count = cnt.data_ptr() if cnt is not None else None
            it.src_dtype = _lib.VX_F64 if sm.dtype == torch.float64 else _lib.VX_F32
            it.T, it.C = T, Cn
            it.t = f.source[1] if f.kind in ("PROB", "ARGMAX") else 0
            it.c = f.source[-1] if f.kind in ("PROB", "MEAN_PROB") else 0
        it.X, it.Y, it.Z = X, Y, Z
        C.memmove(it.header, nifti.header_bytes(f.shape, f.dtype, header), 352)
    _, members, parts = _nifti_gzip(bufs, items, [gz.hints_for(f.dtype.itemsize, f.shape) for f in plan], list(range(len(plan))),
                                    dev, timing)
    host, (base,) = _devio.gather(bufs, [members], dev)
    del keep
    return plan, host, [(base + o, n) for _, o, n in parts]


_DIRS = ("input", "gt_seg", "pred_seg", "pred_prob")   # save_case creates these four whatever it writes


def save_case_device(save_dir: str, image_id: str, softmax_pred, maps: Optional[Dict] = None, data=None, gt_seg=None,
                     num_predictions=None, header=False, _timing=None) -> None:
    """save_case on the device: the same arguments, the same tree, the same decoded bytes in every file.  Device tensors
    are used where they are; numpy arrays and CPU tensors are uploaded.  One vx_nifti_payload launch assembles every
    payload, one vx_gzip_encode compresses them, one copy brings the members back into reused pinned memory, and the
    host writes the files."""
    _devio.save_once(save_dir, _DIRS, _encode_case, image_id, softmax_pred, maps, data, gt_seg, num_predictions, header,
                     _timing)


class ResultsWriter(_devio.PipelinedWriter):
    """Pipelined save_case_device: submit() encodes a case on the GPU and hands its files to a small thread pool, so the
    files of case i are written while case i + 1 is encoded.  Two buffer sets alternate; a set is reused only once its
    files are written.  close() (or leaving the `with` block) waits and re-raises the first write error."""

    _encode = staticmethod(_encode_case)
    _dirs = _DIRS

    def submit(self, save_dir: str, image_id: str, softmax_pred, maps: Optional[Dict] = None, data=None, gt_seg=None,
               num_predictions=None, header=False) -> None:
        self._submit(save_dir, image_id, softmax_pred, maps, data, gt_seg, num_predictions, header)


# ---------------------------------------------------------------------------------------------------------------------
# maps a dataloader writes itself (pred_entropy of a Softmax tree), from the device

class PlannedMap(NamedTuple):
    """One map file of save_maps_device: its path, "gz" (a gzipped NIfTI), "nii" (a plain one) or "tif", voxel shape and
    the numpy dtype the file stores."""
    path: str
    kind: str
    shape: tuple
    dtype: np.dtype


def plan_maps(paths, tensors) -> List[PlannedMap]:
    """What experiment._save_file writes for each (path, map): host logic on endings, shapes and dtypes only."""
    if len(paths) != len(tensors):
        raise ValueError(f"save_maps_device: {len(paths)} paths for {len(tensors)} maps")
    out = []
    for p, t in zip(paths, tensors):
        p = os.path.abspath(str(p))
        low = p.lower()
        shp, dt = _shape_dtype(t)
        if low.endswith((".tif", ".tiff")):
            if len(shp) != 2:
                raise ValueError(f"save_maps_device: {p}: a TIFF map is 2D, got {tuple(shp)}")
            out.append(PlannedMap(p, "tif", (shp[1], shp[0]), np.dtype("float32")))   # the file is (H, W): axes swapped back
        elif low.endswith((".nii.gz", ".nii")):
            out.append(PlannedMap(p, "gz" if low.endswith(".gz") else "nii", tuple(shp), _file_dtype(dt)))
        else:
            raise ValueError(f"save_maps_device: {p}: .nii, .nii.gz, .tif or .tiff expected")
    return out


def _encode_maps(bufs, paths, tensors, header=False, timing=None):
    """COPY payloads of the NIfTI maps and one gz.encode_into over the .gz ones (_nifti_gzip), the .tif maps through the
    TIFF stage (_devio.TiffStage, uncompressed), and one copy per kind of file into pinned memory: -> (plan, host uint8
    array, spans)"""
    import torch
    from . import _lib, gz
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    plan = plan_maps(paths, tensors)
    vols = [i for i, f in enumerate(plan) if f.kind != "tif"]
    tifs = [i for i, f in enumerate(plan) if f.kind == "tif"]
    keep, spans = [], {}
    regions = {"gz": (None, 0), "nii": (None, 0)}
    if vols:
        items = (_lib.NiftiItem * len(vols))()
        for it, i in zip(items, vols):
            f, t = plan[i], _to_device(tensors[i], dev)
            rev = t.permute(*reversed(range(t.dim())))
            if 1 < t.dim() <= 3 and rev.is_contiguous() and str(t.dtype).replace("torch.", "") == f.dtype.name:
                src, X, Y, Z = rev, 1, 1, int(t.numel())   # a reader's [x, y, z] view, x fastest in memory: copied in order
            else:
                src, X, Y, Z = _copy_source(t, f.dtype)
            keep.append(src)
            it.kind, it.src, it.esize = _lib.VX_NIFTI_COPY, (src.data_ptr() if src.numel() else None), f.dtype.itemsize
            it.X, it.Y, it.Z = X, Y, Z
            C.memmove(it.header, nifti.header_bytes(f.shape, f.dtype, header), 352)
        payload, regions["gz"], parts = _nifti_gzip(bufs, items, [gz.hints_for(plan[i].dtype.itemsize, plan[i].shape) for i in vols],
                                                    [k for k, i in enumerate(vols) if plan[i].kind == "gz"], dev, timing)
        if any(plan[i].kind == "nii" for i in vols):   # the plain files are spans of the payload buffer
            regions["nii"] = payload
        spans.update(zip(vols, parts))
    maps = [_to_device(tensors[i], dev).to(torch.float32).transpose(0, 1).contiguous() for i in tifs]   # the file is (H, W)
    tif = _devio.TiffStage("save_maps_device", [tuple(int(v) for v in m.shape) for m in maps])
    regions["tif"] = (tif.launch(bufs, maps, None, dev, None), tif.raw_bytes)
    spans.update(zip(tifs, (("tif",) + p for p in tif.finish(None)[1])))
    host, bases = _devio.gather(bufs, list(regions.values()), dev)
    base = dict(zip(regions, bases))
    del keep
    return plan, host, [(base[spans[i][0]] + spans[i][1],) + tuple(spans[i][2:]) for i in range(len(plan))]


def save_maps_device(paths, tensors, header=False, _timing=None) -> None:
    """experiment._save_file for a batch of device maps: path i gets tensors[i], a map indexed [x, y(, z)] as the readers
    return it.  A .nii.gz / .nii file holds the 352 header bytes and voxel bytes nifti.save writes for the same array (a
    float64 map stays float64), a .tif file is byte-identical to the host writer's (float32, axes swapped back).  One
    vx_nifti_payload launch (COPY items), one gz.encode_into and one device -> host copy into reused pinned memory; the
    host writes the files before the call returns.  MapsWriter is the pipelined form."""
    _devio.save_once("", (), _encode_maps, list(paths), list(tensors), header, _timing)


class MapsWriter(_devio.PipelinedWriter):
    """Pipelined save_maps_device: submit() encodes a batch of maps on the GPU and hands its files to a small thread pool,
    so the files of batch i are written while batch i + 1 is read and reduced.  close() (or leaving the `with` block)
    waits and re-raises the first write error."""

    _encode = staticmethod(_encode_maps)

    def submit(self, paths, tensors, header=False) -> None:
        self._submit("", list(paths), list(tensors), header)


def results_dir(root_dir: str, exp_name: str, version, test_split: str = "id") -> str:
    return os.path.join(root_dir, exp_name, "test_results", str(version), test_split)  # data_carrier_3D.py:40-42


def log_metrics(save_dir: str, per_image_metrics: Dict[str, Dict[str, float]]) -> None:
    """metrics.json with a "mean" entry (data_carrier_3D.py:373-391)."""
    out = {k: dict(v) for k, v in per_image_metrics.items()}
    names = sorted({m for v in per_image_metrics.values() for m in v})
    out["mean"] = {m: float(np.mean([v[m] for v in per_image_metrics.values() if m in v])) for m in names}
    with open(os.path.join(save_dir, "metrics.json"), "w") as f:
        json.dump(out, f, indent=2)
