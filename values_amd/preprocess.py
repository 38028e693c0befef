"""Preprocessing of a 3D data set (the reference's datasets/preprocess_datasets_3d.py:66-168): every raw .nii.gz volume is
z-scored, padded to shape + shape % int(patch_size * patch_overlap) with the normalised minimum, every rater's label is
padded the same way with the label's minimum, and all of it is stored as .npy -- the files predict_image_sliding's
callers load.

Two routes to the same files.  The host mirror (preprocess_volume, preprocess_dataset(device_io=False)) is the reference's
numpy expressions line for line and needs no device.  The device route (preprocess_batch_device, PreprocessReader,
preprocess_dataset(device_io=True), load_cases_device) starts from the volumes nifti.load_device leaves in HBM in their
stored dtype: one vx_volume_stats_batched call for all volumes and labels of a batch, one vx_zscore_pad_batched call
behind it, no wait on the host in between (preprocess.hip).

The padding is placed as batchgenerators.augmentations.utils.pad_nd_image places it.  batchgenerators is absent here, so
its placement is restated from the published algorithm: parity unpinned.
"""
from __future__ import annotations

import io
import os
from collections import deque

import numpy as np

from . import _lib, nifti
from ._devio import PipelinedWriter, align


def pad_sizes(shape, patch_size: int = 64, patch_overlap: float = 1.0):
    """-> (padded shape, [(below, above)] per axis).  The padded extent is the reference's expression s + s % m with
    m = int(patch_size * patch_overlap) (preprocess_datasets_3d.py:140-148) -- NOT the next multiple of m: 70 -> 76 for
    m = 64.  The difference is split as pad_nd_image splits it (restated, parity unpinned): below = diff // 2,
    above = diff // 2 + diff % 2."""
    m = int(patch_size * patch_overlap)
    if m < 1:
        raise ValueError(f"pad_sizes: int(patch_size * patch_overlap) = {m}")
    new = tuple(int(s) + int(s) % m for s in shape)
    split = [((n - int(s)) // 2, (n - int(s)) // 2 + (n - int(s)) % 2) for s, n in zip(shape, new)]
    return new, split


def preprocess_volume(image, labels=(), patch_size: int = 64, patch_overlap: float = 1.0):
    """The host mirror: one case as the reference's loop body treats it (preprocess_datasets_3d.py:135-168), on the arrays
    nifti.load returns -> (image, [labels]) as it np.saves them.  This is what the device route is held to."""
    image = (image - image.mean()) / (image.std() + 1e-8)
    new, split = pad_sizes(image.shape, patch_size, patch_overlap)
    image = np.pad(image, split, "constant", constant_values=image.min())
    out = []
    for label in labels:
        # pad_nd_image pads up to the IMAGE's padded shape, from the label's own shape
        diff = [max(n - s, 0) for n, s in zip(new, label.shape)]
        out.append(np.pad(label, [(d // 2, d // 2 + d % 2) for d in diff], "constant", constant_values=label.min()))
    return image, out


# ---------------------------------------------------------------------------------------------
# The device route

_KIND = {"bool": _lib.VX_PREP_U8, "uint8": _lib.VX_PREP_U8, "int8": _lib.VX_PREP_I8, "uint16": _lib.VX_PREP_U16,
         "int16": _lib.VX_PREP_I16, "uint32": _lib.VX_PREP_U32, "int32": _lib.VX_PREP_I32, "float32": _lib.VX_PREP_F32,
         "float64": _lib.VX_PREP_F64}


def _kind(t, what):
    name = str(t.dtype).replace("torch.", "")
    if name not in _KIND:
        raise TypeError(f"{what}: dtype {name}: integers and bool of 1 / 2 / 4 bytes, float32 and float64 are preprocessed on the device")
    return _KIND[name]


def volume_stats_device(tensors):
    """-> (len(tensors), 4) float64 device tensor of {mean, std, min, n}: one vx_volume_stats_batched call.  A tensor's
    row is bit-equal whatever else is in the batch."""
    import torch
    _lib.require_gpu()
    ts = [_lib.dense_block(t) for t in tensors]
    dev = ts[0].device if ts else torch.device("cuda", torch.cuda.current_device())
    stats = torch.empty((len(ts), 4), dtype=torch.float64, device=dev)
    if not ts:
        return stats
    _stats_call(ts, stats, dev)
    return stats


def _stats_call(ts, stats, dev):
    lib = _lib.load()
    arr = (_lib.PrepItem * len(ts))()
    for i, t in enumerate(ts):
        arr[i].ptr, arr[i].n, arr[i].kind = t.data_ptr(), t.numel(), _kind(t, "vx_volume_stats_batched")
    need = int(lib.vx_volume_stats_batched_workspace_bytes(arr, len(ts)))
    ws = _lib.workspace(dev, need)
    _lib.check(lib.vx_volume_stats_batched(arr, len(ts), _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "vx_volume_stats_batched")


def _pad_call(arr, n, stats, dev):
    lib = _lib.load()
    need = int(lib.vx_zscore_pad_batched_workspace_bytes(arr, n))
    ws = _lib.workspace(dev, need)   # (need = 0: refused, the call names the reason)
    _lib.check(lib.vx_zscore_pad_batched(arr, n, _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "vx_zscore_pad_batched")


def _plan_batch(volumes, labels, patch_size, patch_overlap, out_dtype):
    """Nothing is launched -> (sources: the volumes, then the labels case by case; the vx_prep_pad_item table; the
    outputs, views of ONE device buffer so that a writer downloads a batch in one copy; that buffer; each output's
    (offset, bytes) in it; the labels per case)."""
    import torch
    _lib.require_gpu()
    if out_dtype not in (None, torch.float32, torch.float64):
        raise ValueError(f"preprocess_batch_device: out_dtype {out_dtype}: None, torch.float32 or torch.float64")
    labels = [[] for _ in volumes] if labels is None else [list(ls) for ls in labels]
    if len(labels) != len(volumes):
        raise ValueError(f"preprocess_batch_device: {len(volumes)} volumes, {len(labels)} label lists")
    dev = volumes[0].device if volumes else torch.device("cuda", torch.cuda.current_device())
    srcs, plan, pads, off = [], [], [], 0   # plan: (output dtype, padded shape, below, mode, offset, bytes)
    for v, case in [(v, None) for v in volumes] + [(l, i) for i, ls in enumerate(labels) for l in ls]:
        if v.dim() != 3:
            raise ValueError(f"preprocess_batch_device: a {tuple(v.shape)} tensor: volumes and labels are (X, Y, Z)")
        _kind(v, "preprocess_batch_device")
        if case is None:
            new, split = pad_sizes(v.shape, patch_size, patch_overlap)
            pads.append(new)
            below = [b for b, _ in split]
            dt = out_dtype if out_dtype is not None else (torch.float32 if v.dtype == torch.float32 else torch.float64)
            mode = _lib.VX_PREP_ZSCORE
        else:   # pad_nd_image pads a label up to the image's padded shape, from the label's own
            new = tuple(max(n, s) for n, s in zip(pads[case], v.shape))
            below = [(n - s) // 2 for n, s in zip(new, v.shape)]
            dt, mode = v.dtype, _lib.VX_PREP_COPY
        srcs.append(v.contiguous())
        nbytes = int(np.prod(new)) * torch.empty(0, dtype=dt).element_size()
        plan.append((dt, new, below, mode, off, nbytes))
        off += align(nbytes)
    arena = torch.empty(off, dtype=torch.uint8, device=dev)
    arr = (_lib.PrepPadItem * max(len(srcs), 1))()
    outs = []
    for i, (v, (dt, new, below, mode, o, nbytes)) in enumerate(zip(srcs, plan)):
        out = arena[o:o + nbytes].view(dt).view(new)
        outs.append(out)
        it = arr[i]
        it.src, it.dst, it.kind = v.data_ptr(), out.data_ptr(), _kind(v, "vx_zscore_pad_batched")
        for a in range(3):
            it.dims[a], it.out_dims[a], it.pad_below[a] = v.shape[a], new[a], below[a]
        it.mode, it.stats_row = mode, i
        it.out_dtype = _lib.VX_PREP_OWN if mode == _lib.VX_PREP_COPY else (_lib.VX_F32 if dt == torch.float32 else _lib.VX_F64)
    return srcs, arr, outs, arena, [(p[4], p[5]) for p in plan], labels


def _batch(volumes, labels, patch_size, patch_overlap, out_dtype):
    """-> (images, labels, stats of the volumes and then the labels, the outputs' buffer, their (offset, bytes) in it)"""
    import torch
    srcs, arr, outs, arena, spans, labels = _plan_batch(volumes, labels, patch_size, patch_overlap, out_dtype)
    stats = torch.empty((len(srcs), 4), dtype=torch.float64, device=arena.device)
    if srcs:
        _stats_call(srcs, stats, arena.device)
        _pad_call(arr, len(srcs), stats, arena.device)
    lab_out, k = [], len(volumes)
    for ls in labels:
        lab_out.append(outs[k:k + len(ls)])
        k += len(ls)
    return outs[:len(volumes)], lab_out, stats, arena, spans


def preprocess_batch_device(volumes, labels=None, patch_size: int = 64, patch_overlap: float = 1.0, out_dtype=None):
    """volumes: (X, Y, Z) device tensors as nifti.load_device returns them, shapes and dtypes mixed; labels: per volume
    the list of its raters' device tensors (None: no labels) -> (images, labels, stats).
    images[i] is the z-scored volume padded to pad_sizes(shape), labels[i][r] the label padded to the same shape with its
    minimum and in its own dtype, stats the (B, 4) float64 device tensor {mean, std, min, n} of the volumes.  One
    vx_volume_stats_batched call over all volumes and labels, one vx_zscore_pad_batched call; the host waits for neither.
    Output dtype as numpy promotes (image - mean) / (std + 1e-8): a float32 volume gives float32, every other float64;
    out_dtype=torch.float32 opts into float32 for all (half the bytes; one rounding from the float64 quotient).
    The outputs of one call are views of one device buffer."""
    images, labs, stats, _, _ = _batch(list(volumes), labels, patch_size, patch_overlap, out_dtype)
    return images, labs, stats[:len(images)]


class PreprocessReader(nifti.NiftiReader):
    """Pipelined preprocessing over batches of cases: a batch is a list of (image_path, [label_paths]); read(batches)
    yields per batch [(image, labels, stats_row, header)], everything on the device, stats_row the (4,) float64 row of
    the image.  The files of batch i + 1 are read from disk while batch i is inflated, decoded and preprocessed: the
    reader core's one thread pool, no second one."""

    def __init__(self, device=None, workers: int = 8, patch_size: int = 64, patch_overlap: float = 1.0, out_dtype=None,
                 _timing=None):
        super().__init__(device=device, workers=workers, _timing=_timing)
        self.patch_size, self.patch_overlap, self.out_dtype = patch_size, patch_overlap, out_dtype
        self._cases = deque()   # labels per case of every submitted batch, oldest first
        self.last = None        # (arena, spans) of the batch yielded last: preprocess_dataset downloads from it

    def _submit(self, batch):
        cases = [(str(im), [str(p) for p in labs]) for im, labs in batch]
        self._cases.append([len(labs) for _, labs in cases])
        return super()._submit([p for im, labs in cases for p in [im] + labs])

    def _decode(self, names, raws, device):
        counts = self._cases.popleft()
        loaded = nifti._decode(names, raws, device, self._staging, self._timing)
        vols, labs, heads, k = [], [], [], 0
        for c in counts:
            vols.append(loaded[k][0])
            heads.append(loaded[k][1])
            labs.append([t for t, _ in loaded[k + 1:k + 1 + c]])
            k += 1 + c
        images, lab_out, stats, arena, spans = _batch(vols, labs, self.patch_size, self.patch_overlap, self.out_dtype)
        self.last = (arena, spans)
        return [(images[i], lab_out[i], stats[i], heads[i]) for i in range(len(vols))]

    def read(self, batches):
        for out in super().read(batches):
            if not out:
                self._cases.popleft()   # an empty batch never reaches _decode
            yield out


def load_cases_device(image_paths, patch_size: int = 64, patch_overlap: float = 1.0, device=None, batch: int = 8):
    """-> the float32 device volumes predict_image_sliding takes, straight from the raw .nii / .nii.gz files: no .npy copy
    of the data set on disk.  A volume is what preprocess_dataset stores, cast to float32 the way the data loader casts
    the stored file: a float32 file's volume as it is, every other volume rounded to float64 and then to float32, so the
    result equals the .npy route bit for bit."""
    import torch
    paths = [str(p) for p in image_paths]
    out = []
    with PreprocessReader(device=device, patch_size=patch_size, patch_overlap=patch_overlap) as reader:
        for res in reader.read([[(p, []) for p in paths[b:b + batch]] for b in range(0, len(paths), batch)]):
            out.extend(img if img.dtype == torch.float32 else img.to(torch.float32) for img, _, _, _ in res)
    return out


# ---------------------------------------------------------------------------------------------
# The data set

def npy_header(shape, dtype) -> bytes:
    """the bytes np.save writes in front of a C-ordered array of `shape` and `dtype` (np.lib.format, version 1.0)"""
    f = io.BytesIO()
    np.lib.format.write_array_header_1_0(f, {"descr": np.lib.format.dtype_to_descr(np.dtype(dtype)), "fortran_order": False,
                                             "shape": tuple(int(s) for s in shape)})
    return f.getvalue()


class _File:
    def __init__(self, path):
        self.path = path


def _encode_npy(bufs, arena, files):
    """one pinned download of the batch's arena; a file is its host-built .npy header and its span of the arena"""
    host = bufs.get("host", arena.numel(), arena.device, pinned=True)
    if arena.numel():
        host[:arena.numel()].copy_(arena)
    return [_File(p) for p, _, _, _ in files], host.numpy(), [(o, n, head, b"") for _, o, n, head in files]


class _NpyWriter(PipelinedWriter):
    _encode = staticmethod(_encode_npy)

    def submit(self, save_dir, arena, files):
        self._submit(save_dir, arena, files)


def _cases(image_dir, label_dir, num_raters, dataset):
    """the reference's listing: every .nii.gz of image_dir in sorted order, with the rater files that exist"""
    lidc = dataset in ("lidc", "lidc-idri")
    files = sorted(f for f in os.listdir(image_dir) if f.endswith(".nii.gz") and os.path.isfile(os.path.join(image_dir, f)))
    out = []
    for f in files:
        labs = []
        for r in range(num_raters):
            name = f.replace(".nii.gz", "_{}_mask.nii.gz" if lidc else "_{}.nii.gz").format(str(r).zfill(2))
            if os.path.isfile(os.path.join(label_dir, name)):
                labs.append(os.path.join(label_dir, name))
        out.append((f, os.path.join(image_dir, f), labs))
    return out, lidc


def _label_name(f, rater, lidc):
    # (the reference numbers the raters it FOUND: a missing file shifts the later raters down, :156-167)
    return f"{f.split('.')[0]}_{str(rater).zfill(2)}{'_mask' if lidc else ''}.npy"


def preprocess_dataset(root_dir, save_path, num_raters: int, image_dirs=None, label_dirs=None, dataset=None,
                       patch_size: int = 64, patch_overlap: float = 1, device_io: bool = False, batch: int = 8) -> None:
    """The reference's preprocess_dataset: for every (image_dir, label_dir) pair under root_dir, each <id>.nii.gz becomes
    save_path/preprocessed/<image_dir>/<id>.npy and each rater file that exists
    save_path/preprocessed/<label_dir>/<id>_<rr>.npy (<id>_<rr>_mask.npy for dataset "lidc" / "lidc-idri").
    device_io=False: the host mirror.  device_io=True: PreprocessReader batches of `batch` cases; a batch's results come
    down in one pinned copy and are written on the writer pool while the next batch is computed.  Either way a file
    np.loads to a C-ordered array and starts with the header bytes np.save writes for it."""
    image_dirs = ["images"] if image_dirs is None else image_dirs
    label_dirs = ["labels"] if label_dirs is None else label_dirs
    if batch < 1:
        raise ValueError("preprocess_dataset: batch >= 1")
    for image_dir_name, label_dir_name in zip(image_dirs, label_dirs):
        out_images = os.path.join(str(save_path), "preprocessed", image_dir_name)
        out_labels = os.path.join(str(save_path), "preprocessed", label_dir_name)
        os.makedirs(out_images, exist_ok=True)
        os.makedirs(out_labels, exist_ok=True)
        cases, lidc = _cases(os.path.join(str(root_dir), image_dir_name), os.path.join(str(root_dir), label_dir_name),
                             num_raters, dataset)
        if not device_io:
            for f, image_path, label_paths in cases:
                image, labels = preprocess_volume(nifti.load(image_path)[0], [nifti.load(p)[0] for p in label_paths],
                                                  patch_size, patch_overlap)
                np.save(os.path.join(out_images, f.split(".")[0] + ".npy"), image)
                for r, label in enumerate(labels):
                    np.save(os.path.join(out_labels, _label_name(f, r, lidc)), label)
            continue
        groups = [cases[b:b + batch] for b in range(0, len(cases), batch)]
        with PreprocessReader(patch_size=patch_size, patch_overlap=patch_overlap) as reader, _NpyWriter() as writer:
            results = reader.read([[(ip, lps) for _, ip, lps in g] for g in groups])
            for g, res in zip(groups, results):
                arena, spans = reader.last
                tensors = [img for img, _, _, _ in res] + [l for _, labs, _, _ in res for l in labs]
                paths = [os.path.join(out_images, f.split(".")[0] + ".npy") for f, _, _ in g]
                paths += [os.path.join(out_labels, _label_name(f, r, lidc)) for f, _, lps in g for r in range(len(lps))]
                files = [(p, o, n, npy_header(t.shape, str(t.dtype).replace("torch.", "")))
                         for p, t, (o, n) in zip(paths, tensors, spans)]
                writer.submit("", arena, files)
