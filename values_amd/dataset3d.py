"""The 3D test split: what test_3D.py starts with and what DataCarrier3D keeps beside the predictions
(uncertainty_modeling/test_3D.py:123-219, toy_datamodule_3D.py:581-664, lidc_idri_datamodule_3D.py:667-747,
data_carrier_3D.py:130-153, 173-179, 209-214), Lightning- and batchgenerators-free.

Host mirror (numpy; the reference restated):
    dir_and_subjects_from_train[_lidc]   the split's data directory and subject ids from the checkpoint's hparams
    get_val_test_data_samples            the sample dicts of both datamodules (layout "toy" | "lidc")
    cases(samples)                       one record per image: paths, shape, stored dtypes, crop list (.npy headers only)
    compose_case(image, labels, crops)   the composites concat_data / save_data / calculate_metrics make of a case
    HostTestLoader3D                     groups of case records holding np.load'ed arrays
Device loader:
    DeviceTestLoader3D   per group ONE pinned upload of the .npy payloads of the images and all rater files; the payloads
                         stay on the device in their stored dtype (no cast copy, no per-patch file access -- the reference
                         memory-maps each file once per patch); the next group's files are read while this one computes.
    composite_device     one vx_case_composite call for the cases of a group

Pinned against the reference: parity by restatement -- tests/test_dataset3d_cpu.py restates the reference's listing loops
and concat_data / save_data expressions literally and compares (the reference modules import Lightning and
batchgenerators, which are absent here).
"""
from __future__ import annotations

import ctypes as C
import fnmatch
import os
import pickle
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _devio, _lib
from .dataset2d import _npy_header, check_label_status
from .predict import crop_indices

_IMAGE_KIND = {"uint8": _lib.VX_PREP_U8, "bool": _lib.VX_PREP_U8, "int8": _lib.VX_PREP_I8, "uint16": _lib.VX_PREP_U16,
               "int16": _lib.VX_PREP_I16, "uint32": _lib.VX_PREP_U32, "int32": _lib.VX_PREP_I32, "float32": _lib.VX_PREP_F32,
               "float64": _lib.VX_PREP_F64}
_LABEL_KIND = {1: _lib.VX_COUNT_B1, 2: _lib.VX_COUNT_B2, 4: _lib.VX_COUNT_B4, 8: _lib.VX_COUNT_B8}


# ---------------------------------------------------------------------------------------------------------------------
# host mirror

def dir_and_subjects_from_train(hparams: Dict, data_input_dir=None, test_split: str = "id_test"):
    """test_3D.py:123-152 (args.data_input_dir / args.test_split as arguments) -> (test_data_dir, subject_ids)"""
    data_input_dir = data_input_dir if data_input_dir is not None else hparams["data_input_dir"]
    dataset_name = hparams["datamodule"]["dataset_name"]
    with open(os.path.join(data_input_dir, dataset_name, "splits.pkl"), "rb") as f:
        splits = pickle.load(f)
    fold = hparams["datamodule"]["data_fold_id"]
    subject_ids = splits[fold][test_split]
    return os.path.join(data_input_dir, dataset_name, "preprocessed"), subject_ids


def dir_and_subjects_from_train_lidc(hparams: Dict, data_input_dir=None, test_split: str = "id"):
    """test_3D.py:155-219: the splits file is datamodule.splits_path (with hparams' data_input_dir replaced by the given
    one), or <data_input_dir>/splits_<shift_feature>.pkl ("all" without a shift feature, as there); test_split
    "unlabeled" joins the two unlabeled pools, "val" / "train" are taken as they are, anything else is "<split>_test"."""
    arg_dir = data_input_dir
    data_input_dir = arg_dir if arg_dir is not None else hparams["data_input_dir"]
    shift_feature = hparams["datamodule"]["shift_feature"]
    default = os.path.join(data_input_dir, "splits_{}.pkl".format(shift_feature) if shift_feature is not None else "all")
    if "splits_path" in hparams["datamodule"].keys() and hparams["datamodule"]["splits_path"] is not None:
        splits_path = hparams["datamodule"]["splits_path"]
        if arg_dir is not None:
            splits_path = splits_path.replace(hparams["data_input_dir"], arg_dir)
    else:
        splits_path = default
    with open(splits_path, "rb") as f:
        splits = pickle.load(f)
    fold = hparams["datamodule"]["data_fold_id"]
    if test_split == "unlabeled":
        subject_ids = np.concatenate((splits[fold]["id_unlabeled_pool"], splits[fold]["ood_unlabeled_pool"]))
    elif test_split in ("val", "train"):
        subject_ids = splits[fold][test_split]
    else:
        subject_ids = splits[fold]["{}_test".format(test_split)]
    return os.path.join(data_input_dir, "preprocessed"), subject_ids


def _npy_file_header(path):
    """(shape, dtype) of a .npy file from its header alone"""
    with open(path, "rb") as f:
        try:
            version = np.lib.format.read_magic(f)
            read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
            shape, _, dtype = read(f)
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None
    return tuple(int(v) for v in shape), dtype


def get_val_test_data_samples(base_dir, pattern: str = "*.npy", subject_ids=None, num_raters: int = 1, test=False,
                              patch_size: int = 64, patch_overlap: float = 1, layout: str = "toy") -> List[Dict]:
    """toy_datamodule_3D.py:581-664 (layout "toy": images{Tr,Ts} / labels{Tr,Ts}, <id>_<rr>.npy, subject_ids=None lists
    everything) and lidc_idri_datamodule_3D.py:667-747 (layout "lidc": images / labels, <id>_<rr>_mask.npy,
    subject_ids=None lists nothing).  One dict per crop: image_path, label_paths (the rater files that exist, None when
    none does), crop_idx; images in sorted order, crops z outermost and x innermost.  The image's shape comes from its
    header (the reference memory-maps the file for it)."""
    if layout not in ("toy", "lidc"):
        raise ValueError(f"get_val_test_data_samples: layout {layout!r} is not 'toy' or 'lidc'")
    toy = layout == "toy"
    train_test = ("Tr" if not test else "Ts") if toy else ""
    (image_dir, _, image_filenames) = next(os.walk(os.path.join(base_dir, "images{}".format(train_test))))
    (label_dir, _, label_filenames) = next(os.walk(os.path.join(base_dir, "labels{}".format(train_test))))
    name = "{}_{}.npy" if toy else "{}_{}_mask.npy"
    samples = []
    for image_filename in sorted(fnmatch.filter(image_filenames, pattern)):
        listed = (subject_ids is None or image_filename in subject_ids) if toy else \
            (subject_ids is not None and image_filename in subject_ids)
        if not listed:
            continue
        image_path = os.path.join(image_dir, image_filename)
        label_paths = []
        for rater in range(num_raters):
            label_name = name.format(image_filename.split(".")[0], str(rater).zfill(2))
            if label_name in label_filenames:
                label_paths.append(os.path.join(label_dir, label_name))
        label_paths = label_paths if len(label_paths) > 0 else None
        shape, _ = _npy_file_header(image_path)
        for crop_index in crop_indices(shape, patch_size, patch_overlap):
            samples.append({"image_path": image_path, "label_paths": label_paths, "crop_idx": crop_index})
    return samples


def get_val_test_data_samples_toy(base_dir, **kw):
    """toy_datamodule_3D.get_val_test_data_samples (the seam values_amd.io re-points)"""
    return get_val_test_data_samples(base_dir, layout="toy", **kw)


def get_val_test_data_samples_lidc(base_dir, **kw):
    """lidc_idri_datamodule_3D.get_val_test_data_samples (the seam values_amd.io re-points)"""
    return get_val_test_data_samples(base_dir, layout="lidc", **kw)


def cases(samples: Sequence[Dict]) -> List[Dict]:
    """The listing grouped by image, in its order: {"image_path", "label_paths" (a list, possibly empty), "image_id",
    "shape", "dtype", "label_dtypes", "crops"}.  Shapes and dtypes are read from the .npy headers only."""
    out, index = [], {}
    for s in samples:
        p = s["image_path"]
        if p not in index:
            shape, dtype = _npy_file_header(p)
            labels = list(s["label_paths"] or [])
            index[p] = len(out)
            out.append({"image_path": p, "label_paths": labels, "image_id": os.path.basename(p).split(".")[0], "shape": shape,
                        "dtype": dtype, "label_dtypes": [_npy_file_header(q)[1] for q in labels], "crops": []})
        out[index[p]]["crops"].append(tuple(tuple(int(v) for v in ax) for ax in s["crop_idx"]))
    return out


def compose_case(image: np.ndarray, labels, crops) -> Dict[str, np.ndarray]:
    """What concat_data / save_data / calculate_metrics make of a case fed patch by patch (data_carrier_3D.py:130-153,
    173-179, 209-214; test_3D.py:555-562): num_predictions (float64, patches per voxel), data (float64: the patch values
    ADDED once per covering patch, in crop order, then divided by clip(count, 1)), gt_seg (float64: the intc sum of the
    raters' patches divided the same way, (R, X, Y, Z)) and gt (that cast to intc).  A voxel under no patch is 0 in all."""
    image = np.asarray(image)
    labels = [np.asarray(l) for l in (labels if labels is not None else [])]
    num = np.zeros(image.shape)
    data = np.zeros(image.shape)
    seg = np.zeros([len(labels), *image.shape], dtype=np.intc)
    for c in crops:
        sl = tuple(slice(a, b) for a, b in c)
        data[sl] += image[sl]
        if labels:
            seg[(slice(None),) + sl] += np.array([l[sl] for l in labels], dtype=np.intc)
        num[sl] += 1
    clip = np.clip(num, 1, None)
    gt_seg = np.asarray(seg / clip)
    return {"num_predictions": num, "data": np.asarray(data / clip), "gt_seg": gt_seg, "gt": np.asarray(gt_seg, dtype=np.intc)}


def _groups(case_list, group_cases):
    if group_cases < 1:
        raise ValueError("group_cases >= 1")
    case_list = list(case_list)
    return [case_list[i:i + group_cases] for i in range(0, len(case_list), group_cases)]


class HostTestLoader3D:
    """Groups of at most group_cases case records, each with "image" (np.load of the file) and "labels" (a list)."""

    def __init__(self, cases, group_cases: int):
        self.groups = _groups(cases, int(group_cases))

    def __len__(self):
        return len(self.groups)

    def __iter__(self):
        for g in self.groups:
            yield [dict(c, image=np.load(c["image_path"]), labels=[np.load(p) for p in c["label_paths"]]) for c in g]


# ---------------------------------------------------------------------------------------------------------------------
# device

def _check_case_files(case, heads):
    """heads: [(name, shape, dtype)] of the case's image and rater files; ValueError naming the file that does not fit"""
    name, shape, dtype = heads[0]
    if len(shape) != 3:
        raise ValueError(f"{name}: a 3-D image expected, got shape {shape}")
    if not dtype.isnative or dtype.name not in _IMAGE_KIND:
        raise ValueError(f"{name}: dtype {dtype} is not one the device kernels read (bool, 8 / 16 / 32-bit integers, float32, float64)")
    for lname, lshape, ldtype in heads[1:]:
        if tuple(lshape) != tuple(shape):
            raise ValueError(f"{lname}: label shape {lshape} differs from its image's {shape}")
        if not ldtype.isnative or ldtype.kind not in "iub" or ldtype.itemsize not in _LABEL_KIND:
            raise ValueError(f"{lname}: dtype {ldtype} is not an integer of 1 / 2 / 4 / 8 bytes")


def _typed(buf, off, nbytes, shape, dtype):
    """the payload at buf[off : off + nbytes] as a tensor of the stored dtype (bool as uint8)"""
    import torch
    name = "uint8" if dtype.name == "bool" else dtype.name
    return buf[off:off + nbytes].view(getattr(torch, name)).view(shape)


def upload_group(group, device=None):
    """A host loader's group -> the records a DeviceTestLoader3D yields: "image" / "labels" device tensors in their stored
    dtype.  The same checks, the same errors."""
    import torch
    _lib.require_gpu()
    dev = _devio.current_device(device)
    out = []
    for c in group:
        arrays = [np.ascontiguousarray(c["image"])] + [np.ascontiguousarray(l) for l in c["labels"]]
        _check_case_files(c, [(n, a.shape, a.dtype) for n, a in zip([c["image_path"]] + list(c["label_paths"]), arrays)])
        ts = [torch.from_numpy(a.view(np.uint8) if a.dtype == np.bool_ else a).to(dev) for a in arrays]
        out.append(dict(c, image=ts[0], labels=ts[1:]))
    return out


class DeviceTestLoader3D(_devio.PipelinedReader):
    """The case records of a split on the device, in groups of at most group_cases: per group the files' headers are parsed
    on the host and the payloads of the images and all rater files go up in ONE pinned upload; "image" (X, Y, Z) and
    "labels" [(X, Y, Z)] are views of that buffer in the stored dtype.  prefetch: the files of group i + 1 are read on the
    reader's pool while group i computes.  ValueError, naming the file: a Fortran-order or object array, an image that is
    not 3-D, a label file whose shape differs from its image's, an image dtype outside the VX_PREP_* kinds (a label dtype
    that is not an integer of 1 / 2 / 4 / 8 bytes)."""

    def __init__(self, cases, group_cases: int, device=None, workers: int = 8, prefetch: bool = True):
        super().__init__(device, workers)
        self.groups, self.prefetch = _groups(cases, int(group_cases)), bool(prefetch)
        self._group_of = {g[0]["image_path"]: g for g in self.groups}

    def __len__(self):
        return len(self.groups)

    def _batches(self):
        for g in self.groups:
            yield [c["image_path"] for c in g] + [p for c in g for p in c["label_paths"]]

    def __iter__(self):
        if self.prefetch:
            yield from self.read(self._batches())
        else:
            _lib.require_gpu()
            dev = _devio.current_device(self.device)
            for names in self._batches():
                yield self._decode(names, [_devio._read(p) for p in names], dev)

    def _decode(self, names, raws, device):
        group = self._group_of[names[0]]
        heads = [_npy_header(nm, raw) for nm, raw in zip(names, raws)]
        n, k = len(group), len(group)
        per_case = []
        for i, c in enumerate(group):
            r = len(c["label_paths"])
            idx = [i] + list(range(k, k + r))
            k += r
            _check_case_files(c, [(names[j], heads[j][0], heads[j][1]) for j in idx])
            per_case.append(idx)
        pieces = [(raw, [(off, int(np.prod(shape, dtype=np.int64)) * dtype.itemsize)]) for raw, (shape, dtype, off) in zip(raws, heads)]
        buf, offs, sizes = self._staging.upload(pieces, device)
        out = []
        for c, idx in zip(group, per_case):
            ts = [_typed(buf, offs[j], sizes[j], heads[j][0], heads[j][1]) for j in idx]
            out.append(dict(c, image=ts[0], labels=ts[1:]))
        return out


def composite_device(group, counts, want_data: bool = True, want_gt_seg: bool = True, want_gt: bool = True, gt_out=None):
    """One vx_case_composite call for the device records of a group.  counts: per case the (X, Y, Z) float32 count map
    the accumulation left.  -> per case {"data": (X, Y, Z) float64, "gt_seg": (R, X, Y, Z) float64, "gt": (R, X, Y, Z)
    uint8} (the wanted ones), device tensors; gt_out: per case a contiguous (R, X, Y, Z) uint8 tensor to write gt into
    instead of a new one.  A label outside 0..255 raises ValueError naming the rater file."""
    import torch
    _lib.require_gpu()
    lib = _lib.load()
    n = len(group)
    if n == 0:
        return []
    dev = counts[0].device
    items = (_lib.CompositeItem * n)()
    n_labels = sum(len(c["labels"]) for c in group)
    labels = (_lib.CompositeLabel * max(n_labels, 1))()
    out, keep, k = [], [], 0
    for it, c, cnt in zip(items, group, counts):
        img = c["image"]
        shape = tuple(int(v) for v in img.shape)
        R = len(c["labels"])
        if not cnt.is_contiguous() or cnt.dtype != torch.float32 or tuple(cnt.shape) != shape:
            raise ValueError(f"composite_device: {c['image_path']}: a contiguous float32 count map of shape {shape} expected")
        keep.append(img.contiguous())
        it.image, it.count = keep[-1].data_ptr(), cnt.data_ptr()
        it.image_kind = _IMAGE_KIND[str(img.dtype).replace("torch.", "")]
        it.first_label, it.R = k, R
        it.dims[0], it.dims[1], it.dims[2] = shape
        o = {}
        if want_data:
            o["data"] = torch.empty(shape, dtype=torch.float64, device=dev)
            it.data = o["data"].data_ptr()
        if want_gt_seg:
            o["gt_seg"] = torch.empty((R,) + shape, dtype=torch.float64, device=dev)
            it.gt_seg = o["gt_seg"].data_ptr() if R else None
        if want_gt:
            o["gt"] = torch.empty((R,) + shape, dtype=torch.uint8, device=dev) if gt_out is None else gt_out[len(out)]
            if not o["gt"].is_contiguous() or o["gt"].dtype != torch.uint8 or tuple(o["gt"].shape) != (R,) + shape:
                raise ValueError(f"composite_device: {c['image_path']}: gt_out must be a contiguous uint8 tensor of shape {(R,) + shape}")
            it.gt = o["gt"].data_ptr() if R else None
        for lab in c["labels"]:
            if tuple(lab.shape) != shape or lab.dtype.is_floating_point or lab.element_size() not in _LABEL_KIND:
                raise ValueError(f"composite_device: {c['image_path']}: integer label maps of shape {shape} expected")
            keep.append(lab.contiguous())
            labels[k].ptr, labels[k].kind = keep[-1].data_ptr(), _LABEL_KIND[lab.element_size()]
            labels[k].flags = _lib.VX_LABEL_SIGNED if lab.dtype.is_signed else 0     # a negative label is counted, at any width
            k += 1
        out.append(o)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ws = _lib.workspace(dev, int(lib.vx_case_composite_workspace_bytes(n, n_labels)))
    _lib.check(lib.vx_case_composite(items, n, labels, n_labels, _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "vx_case_composite")
    check_label_status(status.cpu().tolist(), [", ".join(c["label_paths"]) or c["image_path"] for c in group])
    del keep
    return out
