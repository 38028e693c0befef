"""The 2D test split: what test_2D.py starts with (uncertainty_modeling/data/torch_dataloader.py:124-210, :287-300,
data/cityscapes_dataset.py:12-171, augmentations.py:9-50), albumentations- and Lightning-free.

Host mirror (numpy; the reference restated):
    split_keys, test_split_name, get_data_samples      the split's keys, the name of its test split, the listing
    label_switch_references(mask, R, decisions=None)   StochasticLabelSwitches.apply_to_mask: the R raters of a label map
    switch_decisions(seed, indices, R)                 the decisions vx_label_switch_batched draws, restated in integers
    CityscapesTestSet                                  Cityscapes_dataset (test side: Normalize, label switches, ToTensorV2)
    TestDataModule2D                                   BaseDataModule (setup("test"), test_dataloader())
Device loader (device_io=True):
    DeviceTestLoader2D   per batch the .npy headers are parsed on the host, image and label payloads go up in one pinned
                         upload, one vx_tta_views_2d call makes the views and one vx_label_switch_batched call the raters.

Pinned against the reference: the rater draw from np.random (tests/golden/label_switch_kat.npz, written by the reference
class), the listing and the split names.  NOT pinned: torch's DataLoader collation of ids (torch.utils.data.default_collate
is called as the DataLoader calls it, but the DataLoader itself is not run), albumentations' Normalize rounding (data.py)
and the device draw -- with a `seed` the decisions come from this project's generator, not from numpy's stream.
"""
from __future__ import annotations

import ctypes as C
import fnmatch
import io as _io
import os
import pickle
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _devio, _lib, gta
from .data import TTA_2D_VIEW_CODES, tta_views_2d

# augmentations.py:13-19: the classes a switch starts from in dict order, their "_2" classes (cityscapes_labels.py:98-102)
SWITCH_NAMES = tuple(gta.LABEL_SWITCHES)
NAME2TRAINID_2 = {"sidewalk": 19, "person": 20, "car": 21, "vegetation": 22, "road": 23}
VX_LSWITCH_XOR = 0xA54FF53A   # gauss.h


def switch_table():
    """[(from, to, p)] in the reference's dict order"""
    return [(gta.NAME2TRAINID[c], NAME2TRAINID_2[c], gta.LABEL_SWITCHES[c]) for c in SWITCH_NAMES]


def switch_thresholds():
    """thr = (uint32)(p * 2^24), in double: what vx_label_switch_batched compares a 24-bit hash against"""
    return [int(float(p) * float(1 << 24)) for _, _, p in switch_table()]


def switch_variance_table() -> np.ndarray:
    """256 float32: the variance of the Bernoulli switch for a class that switches, 0 elsewhere -- every value made by the
    expression of gta._switch_variance, assigned into float32 as there"""
    tab = np.zeros(256, dtype=np.single)
    for c, p in gta.LABEL_SWITCHES.items():
        mean = p
        tab[gta.NAME2TRAINID[c]] = (1 - p) * np.square(0 - mean) + p * np.square(1 - mean)
    return tab


# ---------------------------------------------------------------------------------------------------------------------
# host mirror

def split_keys(splits_path, fold: int = 0) -> Dict[str, object]:
    """Cityscapes_dataset.get_split_keys (cityscapes_dataset.py:116-130): the keys of every split of one fold"""
    with open(splits_path, "rb") as f:
        splits = pickle.load(f)
    s = splits[fold]
    return {"train": s["train"], "val": s["val"], "id_test": s["id_test"], "ood_test": s["ood_test"],
            "unlabeled": np.concatenate((s["id_unlabeled_pool"], s["ood_unlabeled_pool"]))}


def test_split_name(test_split):
    """torch_dataloader.py:199-203"""
    return test_split if test_split == "unlabeled" or test_split == "val" else f"{test_split}_test"


test_split_name.__test__ = False   # (a product function, not a test)


def get_data_samples(base_dir, pattern: str = "*.npy", subject_ids=None, dataset: str = "gta") -> List[Dict]:
    """cityscapes_dataset.py:133-171"""
    samples = []
    (image_dir, _, image_filenames) = next(os.walk(os.path.join(base_dir, "images")))
    (label_dir, _, label_filenames) = next(os.walk(os.path.join(base_dir, "labels")))
    for image_filename in sorted(fnmatch.filter(image_filenames, pattern)):
        if subject_ids is not None and image_filename in subject_ids:
            samples.append({"image_path": os.path.join(image_dir, image_filename),
                            "label_path": os.path.join(label_dir, image_filename) if image_filename in label_filenames else None,
                            "image_id": image_filename.split(".")[0], "dataset": dataset})
    return samples


def label_switch_references(mask: np.ndarray, n_reference_samples: int = 1, decisions=None) -> np.ndarray:
    """StochasticLabelSwitches.apply_to_mask (augmentations.py:25-40).  decisions: (R, 5) 0 / 1 in the reference's class
    order, or None: np.random.binomial(1, p, 1) per reference, then per class in dict order -- after np.random.seed(s)
    the reference class's own output.  One reference gives (H, W), several (R, H, W), as there."""
    masks = []
    for reference in range(n_reference_samples):
        mask_copy = mask.copy()
        for k, (init_id, final_id, p) in enumerate(switch_table()):
            switch = np.random.binomial(1, p, 1)[0] if decisions is None else decisions[reference][k]
            if switch:
                mask_copy[mask_copy == init_id] = final_id
        masks.append(mask_copy)
    return np.array(masks) if len(masks) > 1 else masks[0]


def _mix32(h):
    h = h & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x846CA68B) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def switch_decisions(seed: int, indices: Sequence[int], R: int) -> np.ndarray:
    """(len(indices), R, 5) uint8: decision(index, r, k) = (h1 >> 8) < thr_k, h1 the first word of vx_gauss_words(seed ^
    VX_LSWITCH_XOR, a = r * 5 + k, b = index) (gauss.h) -- the kernel's draw in integers: a value depends on (seed, index,
    r, k) alone."""
    thr, n = switch_thresholds(), len(SWITCH_NAMES)
    out = np.zeros((len(indices), int(R), n), dtype=np.uint8)
    s = (int(seed) ^ VX_LSWITCH_XOR) & 0xFFFFFFFF
    for i, index in enumerate(indices):
        key = _mix32(s ^ ((int(index) * 0x85EBCA6B + 0x165667B1) & 0xFFFFFFFF))
        for r in range(int(R)):
            for k in range(n):
                a = r * n + k
                h1 = _mix32(((a * 0x9E3779B1) & 0xFFFFFFFF) ^ key)
                out[i, r, k] = (h1 >> 8) < thr[k]
    return out


class TestTransforms2D:
    """What the TEST Compose of the 2D configs holds: Normalize(mean, std), StochasticLabelSwitches(n_reference_samples),
    ToTensorV2."""
    __test__ = False

    def __init__(self, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), n_reference_samples: int = 1,
                 max_pixel_value: float = 255.0):
        self.mean, self.std = [float(v) for v in mean], [float(v) for v in std]
        self.n_reference_samples, self.max_pixel_value = int(n_reference_samples), float(max_pixel_value)


def parse_test_transforms(augmentations) -> TestTransforms2D:
    """augmentations["TEST"][0]["Compose"]["transforms"] (a plain, resolved dict) -> TestTransforms2D; a transform other
    than Normalize / StochasticLabelSwitches / ToTensorV2 raises ValueError naming it."""
    kw = {}
    for entry in augmentations["TEST"][0]["Compose"]["transforms"]:
        for name, params in dict(entry).items():
            params = dict(params or {})
            if name == "Normalize":
                for k in ("mean", "std", "max_pixel_value"):
                    if k in params:
                        kw[k] = params[k]
            elif name == "StochasticLabelSwitches":
                kw["n_reference_samples"] = params.get("n_reference_samples", 1)
            elif name != "ToTensorV2":
                raise ValueError(f"TestDataModule2D: TEST transform {name!r} is not one of Normalize, StochasticLabelSwitches, ToTensorV2")
    return TestTransforms2D(**kw)


def set_n_reference_samples(hparams, n_reference_samples):
    """Tester.set_n_reference_samples (test_2D.py:62-73)"""
    transforms = hparams["AUGMENTATIONS"]["TEST"][0]["Compose"]["transforms"]
    label_switch_index = [i for i, aug in enumerate(transforms) if "StochasticLabelSwitches" in aug][0]
    transforms[label_switch_index]["StochasticLabelSwitches"]["n_reference_samples"] = n_reference_samples
    return hparams


class CityscapesTestSet:
    """Cityscapes_dataset (cityscapes_dataset.py:12-114): the attributes imgs, masks, image_ids, datasets, samples, and
    __getitem__ with the reference's keys.  transforms: a TestTransforms2D (None: its defaults).  `data` comes from
    data.tta_views_2d: the normalised (3, H, W) float32 tensor, or under tta the list of four views (the two noisy ones
    without a field: albumentations' GaussNoise is absent) with `transforms`.  `seg`: label_switch_references of the
    label, drawn from np.random when seed is None and from switch_decisions(seed, [idx], R) otherwise."""
    __test__ = False

    def __init__(self, splits_path, base_dir, split="train", file_pattern: str = "*.npy", transforms=None, data_fold_id: int = 0,
                 tta: bool = False, seed=None):
        self.splits_path, self.data_fold_id = splits_path, data_fold_id
        keys = split_keys(splits_path, data_fold_id)
        self.tr_keys, self.val_keys, self.id_test_keys = keys["train"], keys["val"], keys["id_test"]
        self.ood_test_keys, self.unlabeled_keys = keys["ood_test"], keys["unlabeled"]
        if split not in keys:
            raise ValueError(f"{split} split not specified!")
        subject_ids = keys[split]
        self.samples = []
        for dataset in ["gta", "cs"]:
            ds_subjects = [subject[0] for subject in subject_ids if subject[1] == dataset]
            ds_dir = os.path.join(base_dir, "OriginalData" if dataset == "gta" else "CityScapesOriginalData", "preprocessed")
            self.samples.extend(get_data_samples(base_dir=ds_dir, pattern=file_pattern, subject_ids=ds_subjects, dataset=dataset))
        self.imgs = [sample["image_path"] for sample in self.samples]
        self.masks = [sample["label_path"] for sample in self.samples]
        self.image_ids = [sample["image_id"] for sample in self.samples]
        self.datasets = [sample["dataset"] for sample in self.samples]
        self.transforms = transforms if transforms is not None else TestTransforms2D()
        self.tta, self.seed = tta, seed

    def __len__(self):
        return len(self.imgs)

    def references(self, idx: int, mask: np.ndarray) -> np.ndarray:
        R = self.transforms.n_reference_samples
        dec = None if self.seed is None else switch_decisions(self.seed, [idx], R)[0]
        return label_switch_references(mask, R, dec)

    def __getitem__(self, idx):
        import torch
        img = np.load(self.imgs[idx])
        mask = np.load(self.masks[idx])
        t = self.transforms
        views, names = tta_views_2d(img, t.mean, t.std, max_pixel_value=t.max_pixel_value)
        seg = torch.from_numpy(np.ascontiguousarray(self.references(idx, mask)))
        if self.tta:
            return {"data": [torch.from_numpy(v) for v in views], "seg": seg, "image_id": self.image_ids[idx],
                    "dataset": self.datasets[idx], "transforms": names}
        return {"data": torch.from_numpy(views[0]), "seg": seg, "image_id": self.image_ids[idx], "dataset": self.datasets[idx]}


class HostTestLoader2D:
    """DataLoader(DS_test, batch_size=val_batch_size) of torch_dataloader.py:287-300 without worker processes: the items in
    order, batch_size per batch and the last one short, collated by torch.utils.data.default_collate."""

    def __init__(self, dataset, batch_size: int):
        if batch_size < 1:
            raise ValueError("HostTestLoader2D: batch_size >= 1")
        self.dataset, self.batch_size = dataset, int(batch_size)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        from torch.utils.data import default_collate
        for b in range(0, len(self.dataset), self.batch_size):
            yield default_collate([self.dataset[i] for i in range(b, min(b + self.batch_size, len(self.dataset)))])


# ---------------------------------------------------------------------------------------------------------------------
# device

_KIND = {1: _lib.VX_COUNT_B1, 2: _lib.VX_COUNT_B2, 4: _lib.VX_COUNT_B4, 8: _lib.VX_COUNT_B8}


def switch_rows():
    """the reference's switch table as vx_lswitch_row[5]"""
    rows = (_lib.LswitchRow * len(SWITCH_NAMES))()
    for k, ((f, t, _), thr) in enumerate(zip(switch_table(), switch_thresholds())):
        rows[k].from_, rows[k].to, rows[k].thr = f, t, thr
    return rows


def label_switch_call(items, n: int, R: int, status, seed: int = 0, decisions=None, rows=None, var_table=None, device=None):
    """One vx_label_switch_batched call over the first n entries of the vx_lswitch_item array `items` on the current
    stream.  status: int32 device tensor (n,); decisions: (n, R, n_switch) uint8 array or None (drawn from `seed`);
    rows: a vx_lswitch_row array (default: the reference's table); var_table: 256 float32 (default:
    switch_variance_table()).  Nothing is waited for."""
    lib = _lib.load()
    rows = switch_rows() if rows is None else rows
    dev = status.device if device is None else device
    ws = _lib.workspace(dev, int(lib.vx_label_switch_batched_workspace_bytes(n, R)))   # (0: refused, the call names the reason)
    vt = np.ascontiguousarray(switch_variance_table() if var_table is None else var_table, dtype=np.float32)
    dec = None
    if decisions is not None:
        dec = np.ascontiguousarray(decisions, dtype=np.uint8)
        if dec.shape != (n, R, len(rows)):
            raise ValueError(f"label_switch_call: decisions of shape {(n, R, len(rows))} expected, got {dec.shape}")
    _lib.check(lib.vx_label_switch_batched(items, n, R, rows, len(rows), None if dec is None else dec.ctypes.data_as(C.c_void_p),
                                           int(seed) & 0xFFFFFFFF, vt.ctypes.data_as(C.POINTER(C.c_float)), _lib.ptr(status),
                                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "vx_label_switch_batched")


def label_switch_device(labels, indices, R: int, seed: int = 0, decisions=None, refs: bool = True, variance: bool = False,
                        names=None):
    """The raters and / or variance maps of a batch of label maps: labels a list of (H, W) integer device tensors (1 / 2 /
    4 / 8-byte; sizes may differ), indices their split positions.  -> ([(R, H, W) uint8] or None, [(W, H) float32] or
    None), device tensors.  A label outside 0..255 raises ValueError naming the item (names[i], default its number); an
    int8 map goes in widened to int16, so its negative labels are among them."""
    import torch
    _lib.require_gpu()
    n = len(labels)
    if n == 0:
        return ([] if refs else None), ([] if variance else None)
    dev = labels[0].device
    arr = (_lib.LswitchItem * n)()
    out_r, out_v, keep = [], [], []
    for i, (lab, index) in enumerate(zip(labels, indices)):
        if lab.dim() != 2 or lab.dtype.is_floating_point or lab.element_size() not in _KIND:
            raise ValueError("label_switch_device: (H, W) integer label maps expected")
        # VX_COUNT_B1 is read as unsigned bytes: signed bytes go up as int16, whose negatives the kernel counts
        lab = lab.to(torch.int16).contiguous() if lab.dtype == torch.int8 else lab.contiguous()
        keep.append(lab)
        H, W = int(lab.shape[0]), int(lab.shape[1])
        it = arr[i]
        it.labels, it.H, it.W, it.kind, it.index = lab.data_ptr(), H, W, _KIND[lab.element_size()], int(index) & 0xFFFFFFFF
        if refs:
            out_r.append(torch.empty((R, H, W), dtype=torch.uint8, device=dev))
            it.refs = out_r[-1].data_ptr()
        if variance:
            out_v.append(torch.empty((W, H), dtype=torch.float32, device=dev))
            it.variance = out_v[-1].data_ptr()
    status = torch.empty(n, dtype=torch.int32, device=dev)
    label_switch_call(arr, n, R, status, seed, decisions)
    check_label_status(status.cpu().tolist(), names if names is not None else [f"item {i}" for i in range(n)])
    return (out_r if refs else None), (out_v if variance else None)


def check_label_status(status, names):
    """status: the host list of a batch; a non-zero count is a label file that holds something other than 0..255"""
    for count, name in zip(status, names):
        if count:
            raise ValueError(f"{name}: {count} labels outside 0..255")


def _npy_header(name, raw):
    """-> (shape, dtype, payload offset) of a C-order .npy file's bytes"""
    f = _io.BytesIO(raw)
    try:
        version = np.lib.format.read_magic(f)
        read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
        shape, fortran, dtype = read(f)
    except ValueError as e:
        raise ValueError(f"{name}: {e}") from None
    off = f.tell()
    n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    if fortran or dtype.hasobject or off + n > len(raw):
        raise ValueError(f"{name}: a complete C-order .npy array expected")
    return tuple(int(v) for v in shape), dtype, off


class DeviceTestLoader2D(_devio.PipelinedReader):
    """The test loader of a CityscapesTestSet on the device.  Iterating yields per batch
        data        (G, B, H, W, 4) float32 views, channels-last at the stem's pitch (G = 1, or the reference's four under
                    tta; the noisy views are drawn from `seed`, stream = the image's split index)
        seg         (B, R, H, W) uint8, always 4-D
        image_id, dataset   lists;   transforms   the views' transform names (tta)
    With the same seed the host mirror gives the same seg, and the same data for the views that carry no noise.  The
    images of a batch have one size (the views kernel takes one size).  prefetch: the files of batch i + 1 are read from
    disk while batch i is on the device.  reference_segs / gt_unc_map: one image, a batch of one of the same kernel,
    keyed by the image's split index."""

    def __init__(self, dataset: CityscapesTestSet, batch_size: int, seed, device=None, workers: int = 8, prefetch: bool = True):
        if seed is None:
            raise ValueError("DeviceTestLoader2D: a seed is required (the raters are drawn on the device)")
        if batch_size < 1:
            raise ValueError("DeviceTestLoader2D: batch_size >= 1")
        super().__init__(device, workers)
        self.dataset, self.batch_size, self.seed, self.prefetch = dataset, int(batch_size), int(seed), bool(prefetch)
        self._index = {str(p): i for i, p in enumerate(dataset.imgs)}

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _batches(self):
        ds = self.dataset
        for b in range(0, len(ds), self.batch_size):
            idx = range(b, min(b + self.batch_size, len(ds)))
            yield [str(ds.imgs[i]) for i in idx] + [str(ds.masks[i]) for i in idx]

    def __iter__(self):
        if self.prefetch:
            yield from self.read(self._batches())
        else:
            _lib.require_gpu()
            dev = _devio.current_device(self.device)
            for names in self._batches():
                yield self._decode(names, [_devio._read(p) for p in names], dev)

    def _decode(self, names, raws, device):
        import torch
        from .data import tta_views_2d_device
        ds, B = self.dataset, len(names) // 2
        t = ds.transforms
        R = t.n_reference_samples
        heads = [_npy_header(nm, raw) for nm, raw in zip(names, raws)]
        for nm, (shape, dtype, _) in zip(names[:B], heads[:B]):
            if len(shape) != 3 or shape[2] != 3 or dtype != np.uint8:
                raise ValueError(f"{nm}: an (H, W, 3) uint8 image expected, got {shape} {dtype}")
        H, W = heads[0][0][:2]
        for nm, (shape, dtype, _) in zip(names, heads):
            if tuple(shape[:2]) != (H, W):
                raise ValueError(f"{nm}: {shape[:2]} in a batch of {(H, W)} images: a batch has one size")
        for nm, (shape, dtype, _) in zip(names[B:], heads[B:]):
            if len(shape) != 2 or dtype.kind not in "iub" or dtype.itemsize not in _KIND:
                raise ValueError(f"{nm}: an (H, W) integer label map expected, got {shape} {dtype}")
        pieces = [(raw, [(off, int(np.prod(shape, dtype=np.int64)) * dtype.itemsize)]) for raw, (shape, dtype, off) in zip(raws, heads)]
        buf, offs, sizes = self._staging.upload(pieces, device)
        first = self._index[names[0]]
        img = torch.stack([buf[o:o + n].view(H, W, 3) for o, n in zip(offs[:B], sizes[:B])])
        views, tr = tta_views_2d_device(img, t.mean, t.std, max_pixel_value=t.max_pixel_value,
                                        view_codes=list(TTA_2D_VIEW_CODES) if ds.tta else [0], noise_seed=self.seed, image_index0=first)
        seg = torch.empty((B, R, H, W), dtype=torch.uint8, device=device)
        status = torch.empty(B, dtype=torch.int32, device=device)
        arr = (_lib.LswitchItem * B)()
        wide = []
        for b in range(B):
            it, (shape, dtype, _) = arr[b], heads[B + b]
            it.labels, it.refs = buf.data_ptr() + offs[B + b], seg[b].data_ptr()
            it.H, it.W, it.kind, it.index = H, W, _KIND[dtype.itemsize], first + b
            if dtype == np.int8:   # VX_COUNT_B1 is read as unsigned bytes: signed bytes go in as int16
                wide.append(buf[offs[B + b]:offs[B + b] + sizes[B + b]].view(torch.int8).to(torch.int16))
                it.labels, it.kind = wide[-1].data_ptr(), _KIND[2]
        label_switch_call(arr, B, R, status, self.seed)
        check_label_status(status.cpu().tolist(), names[B:])
        out = {"data": views, "seg": seg, "image_id": [ds.image_ids[first + b] for b in range(B)],
               "dataset": [ds.datasets[first + b] for b in range(B)]}
        if ds.tta:
            out["transforms"] = tr
        return out

    def _one(self, image_id, refs, variance):
        import torch
        _lib.require_gpu()
        ds = self.dataset
        idx = ds.image_ids.index(image_id)
        lab = torch.from_numpy(np.ascontiguousarray(np.load(str(ds.masks[idx])))).to(_devio.current_device(self.device))
        return label_switch_device([lab], [idx], ds.transforms.n_reference_samples, self.seed, refs=refs, variance=variance,
                                   names=[str(ds.masks[idx])])

    def reference_segs(self, image_id):
        """(R, H, W) uint8 device tensor ((H, W) for one rater, as the host getter squeezes): the raters of the image"""
        r = self._one(image_id, True, False)[0][0]
        return r[0] if r.shape[0] == 1 else r

    def gt_unc_map(self, image_id):
        """(W, H) float32 device tensor: gta.gt_unc_map of the image's label"""
        return self._one(image_id, False, True)[1][0]


class TestDataModule2D:
    """BaseDataModule (torch_dataloader.py:124-210, :287-300) for the test stage: setup("test") builds the dataset from the
    `dataset` config (its `_target_` re-pointed by values_amd.io) with the TEST transforms, test_dataloader() returns a
    loader with `.dataset` that yields batches of val_batch_size in order.  device_io=True: a DeviceTestLoader2D (needs
    `seed`); else the host mirror, whose raters come from np.random when seed is None, as in the reference."""
    __test__ = False

    def __init__(self, data_input_dir, dataset, batch_size: int, val_batch_size: int, num_workers: int, augmentations,
                 tta: bool = False, device_io: bool = False, seed=None, **kwargs):
        self.num_workers, self.batch_size, self.val_batch_size = num_workers, batch_size, val_batch_size
        self.augmentations, self.data_input_dir, self.dataset = augmentations, data_input_dir, dataset
        self.test_split = kwargs.get("test_split", None)
        self.tta, self.device_io, self.seed = tta, bool(device_io), seed
        if self.device_io and seed is None:
            raise ValueError("TestDataModule2D: device_io=True needs a seed (the raters are drawn on the device)")
        self.DS_test = None

    def setup(self, stage: Optional[str] = None) -> None:
        if stage not in (None, "test"):
            raise ValueError(f"TestDataModule2D: stage {stage!r}: only the test stage exists here")
        from .io import instantiate
        transforms_test = parse_test_transforms(self.augmentations)
        self.DS_test = instantiate(dict(self.dataset), base_dir=self.data_input_dir, split=test_split_name(self.test_split),
                                   transforms=transforms_test, tta=self.tta, seed=self.seed)

    def test_dataloader(self):
        if self.DS_test is None:
            raise RuntimeError("TestDataModule2D: call setup(\"test\") first")
        if self.device_io:
            return DeviceTestLoader2D(self.DS_test, self.val_batch_size, self.seed, workers=max(int(self.num_workers), 1))
        return HostTestLoader2D(self.DS_test, self.val_batch_size)
