"""Minimal NIfTI-1 single-file codec (.nii / .nii.gz) for the results directory.

The reference writes and reads its result volumes through MedPy (`medpy.io.save / load`, i.e. SimpleITK;
data_carrier_3D.py:233-371, experiment_dataloader.py:44-169).  MedPy is a third-party dependency that is absent
here, so byte-level parity of the files is UNPINNED; this module follows the published NIfTI-1 layout (348-byte
header, vox_offset 352, little endian) and MedPy's axis convention: a numpy array indexed [x, y, z] is stored with x
varying fastest (dim[1..3] = X, Y, Z), which is what SimpleITK produces for `medpy.io.save(arr, ...)`.
Files written by the reference load here with the same [x, y, z] indexing.
"""
from __future__ import annotations

import ctypes as C
import gzip
import struct

import numpy as np

from ._devio import PipelinedReader, Stages, load_once

_DT = {np.dtype("uint8"): (2, 8), np.dtype("int16"): (4, 16), np.dtype("int32"): (8, 32), np.dtype("float32"): (16, 32),
       np.dtype("float64"): (64, 64), np.dtype("int8"): (256, 8), np.dtype("uint16"): (512, 16),
       np.dtype("uint32"): (768, 32), np.dtype("int64"): (1024, 64), np.dtype("uint64"): (1280, 64)}
_CODE = {v[0]: k for k, v in _DT.items()}


def file_dtype(dtype) -> np.dtype:
    """The dtype `save` stores an array of `dtype` as: bool -> uint8, anything outside the NIfTI table -> float64."""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return np.dtype("uint8")
    if dt.newbyteorder("<") not in _DT and dt not in _DT:
        return np.dtype("float64")
    return np.dtype(dt.name)


def header_bytes(shape, dtype, header=None) -> bytes:
    """The 352 bytes in front of the voxels of a file `save` writes: the 348-byte header of an array of `shape` and
    `dtype` (already one of the table's, see file_dtype) plus the 4 zero extension bytes."""
    code, bitpix = _DT[np.dtype(np.dtype(dtype).name)]
    nd = len(shape)
    if not 1 <= nd <= 7:
        raise ValueError("NIfTI-1 stores 1..7 dimensions")
    dim = [nd] + [int(v) for v in shape] + [1] * (7 - nd)
    pixdim = [1.0] * 8
    affine = np.eye(4)
    if isinstance(header, dict):
        for i, p in enumerate(header.get("pixdim", [])[:nd]):
            pixdim[1 + i] = float(p)
        affine = np.asarray(header.get("affine", np.diag(pixdim[1:4] + [1.0])), dtype=np.float64)
    else:
        affine = np.diag(pixdim[1:4] + [1.0])
    h = bytearray(348)
    struct.pack_into("<i", h, 0, 348)
    struct.pack_into("<8h", h, 40, *dim)
    struct.pack_into("<h", h, 70, code)
    struct.pack_into("<h", h, 72, bitpix)
    struct.pack_into("<8f", h, 76, *pixdim)
    struct.pack_into("<f", h, 108, 352.0)       # vox_offset
    struct.pack_into("<f", h, 112, 1.0)         # scl_slope
    struct.pack_into("<B", h, 123, 2)           # xyzt_units: mm
    struct.pack_into("<h", h, 252, 0)           # qform_code
    struct.pack_into("<h", h, 254, 2)           # sform_code: aligned
    struct.pack_into("<4f", h, 280, *affine[0])
    struct.pack_into("<4f", h, 296, *affine[1])
    struct.pack_into("<4f", h, 312, *affine[2])
    h[344:348] = b"n+1\0"
    return bytes(h) + b"\0\0\0\0"


def save(arr, path: str, header=None) -> None:
    """arr: numpy array (or anything np.asarray accepts) indexed [x, y(, z, ...)].  `header` (a dict with optional
    "pixdim" and "affine") plays the role of medpy's header argument; False / None = identity geometry."""
    a = np.asarray(arr)
    a = a.astype(file_dtype(a.dtype).newbyteorder("<"), copy=False)
    payload = header_bytes(a.shape, a.dtype, header) + np.asfortranarray(a).tobytes(order="F")
    if str(path).endswith(".gz"):
        with gzip.open(path, "wb", compresslevel=1) as f:
            f.write(payload)
    else:
        with open(path, "wb") as f:
            f.write(payload)


class Header:
    """What nifti.load reads from the 348-byte header (parse_header): shape, dtype (native byte order) and endian
    ("<" / ">") of the voxels, data_offset (bytes before the voxels), nbytes (data_offset + voxel bytes), slope / inter,
    scaled (load applies a * slope + inter), out_dtype (the dtype load returns), code and the header dict."""

    __slots__ = ("shape", "dtype", "endian", "vox_offset", "data_offset", "nbytes", "slope", "inter", "scaled",
                 "out_dtype", "code", "header")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def parse_header(raw, name: str = "") -> Header:
    """The header of a NIfTI-1 payload (its first 348 bytes are enough): what load reads, and how."""
    raw = bytes(raw[:352]) if len(raw) >= 352 else bytes(raw)
    pre = f"{name}: " if name else ""
    if len(raw) < 348:
        raise ValueError(f"{pre}not a NIfTI-1 file ({len(raw)} bytes)")
    if struct.unpack_from("<i", raw, 0)[0] == 348:
        e = "<"
    elif struct.unpack_from(">i", raw, 0)[0] == 348:
        e = ">"
    else:
        raise ValueError(f"{pre}not a NIfTI-1 file")
    dim = struct.unpack_from(e + "8h", raw, 40)
    code = struct.unpack_from(e + "h", raw, 70)[0]
    pixdim = struct.unpack_from(e + "8f", raw, 76)
    vox_offset = int(struct.unpack_from(e + "f", raw, 108)[0])
    slope, inter = struct.unpack_from(e + "2f", raw, 112)
    if code not in _CODE:
        raise ValueError(f"{pre}unsupported NIfTI datatype {code}")
    shape = tuple(int(d) for d in dim[1:1 + dim[0]])
    dt = _CODE[code]
    scaled = slope not in (0.0, 1.0) or inter != 0.0
    out_dtype = (np.zeros(1, dt) * slope + inter).dtype if scaled else dt
    affine = np.eye(4)
    affine[0] = struct.unpack_from(e + "4f", raw, 280)
    affine[1] = struct.unpack_from(e + "4f", raw, 296)
    affine[2] = struct.unpack_from(e + "4f", raw, 312)
    data_offset = max(vox_offset, 352)
    return Header(shape=shape, dtype=dt, endian=e, vox_offset=vox_offset, data_offset=data_offset,
                  nbytes=data_offset + int(np.prod(shape)) * dt.itemsize, slope=slope, inter=inter, scaled=scaled,
                  out_dtype=out_dtype, code=code,
                  header={"pixdim": list(pixdim[1:1 + dim[0]]), "affine": affine, "datatype": code})


def load(path: str):
    """-> (array indexed [x, y, z], header dict) like medpy.io.load."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as f:
        raw = f.read()
    h = parse_header(raw, str(path))
    dt = h.dtype.newbyteorder(h.endian)
    n = int(np.prod(h.shape))
    a = np.frombuffer(raw, dtype=dt, count=n, offset=h.data_offset).reshape(h.shape, order="F")
    a = np.ascontiguousarray(a.astype(dt.newbyteorder("=")))
    if h.scaled:
        a = a * h.slope + h.inter
    return a, h.header


# ---------------------------------------------------------------------------------------------
# Reading on the device: files read on the host, inflated (vx_inflate) and decoded (vx_nifti_decode) on the GPU.

MAX_FILE = 1 << 32   # ISIZE and the decoder's windows are 32-bit
_TORCH = {"uint8": "uint8", "int8": "int8", "int16": "int16", "int32": "int32", "int64": "int64", "float32": "float32",
          "float64": "float64", "uint16": "uint16", "uint32": "uint32", "uint64": "uint64"}


def _torch_dtype(dt):
    import torch
    return getattr(torch, _TORCH[np.dtype(dt).name])


def _decode(names, raws, device, staging, timing=None):
    """the device half of load_device for one batch of file contents"""
    import torch
    from . import _lib
    from .gz import inflate_into, status_name
    for nm, r in zip(names, raws):
        if len(r) >= MAX_FILE:
            raise ValueError(f"{nm}: {len(r)} bytes: files of 4 GiB or more are not read on the device")
    src, soffs, _ = staging.upload([(r, [(0, len(r))]) for r in raws], device)
    gz = [str(nm).endswith(".gz") for nm in names]
    stages = Stages(timing)
    stages.mark()
    items = []
    for i, r in enumerate(raws):
        if gz[i]:
            cap = max(int.from_bytes(r[-4:], "little") if len(r) >= 4 else 0, 352)
            items.append((C.c_void_p(src.data_ptr() + soffs[i]) if r else None, len(r), _lib.VX_INFLATE_GZIP, cap))
    dst, doffs, dn, dst_st = inflate_into(items, device) if items else (None, [], [], [])
    # where each payload lies: (tensor, offset, size)
    where, k = [], 0
    for i, r in enumerate(raws):
        if gz[i]:
            where.append([dst, doffs[k], dn[k], dst_st[k]])
            k += 1
        else:
            where.append([src, soffs[i], len(r), 0])
    # one D2H: the first 352 bytes of every payload
    idx = []
    for t, o, n, _ in where:
        idx.append((0 if t is src else 1, o))
    hdr = torch.empty((len(raws), 352), dtype=torch.uint8, device=device)
    ar = torch.arange(352, device=device)
    for which in (0, 1):
        rows = [i for i, (w, _) in enumerate(idx) if w == which]
        if rows:
            t = src if which == 0 else dst
            base = torch.tensor([idx[i][1] for i in rows], dtype=torch.int64, device=device)
            g = (base[:, None] + ar[None, :]).clamp_(max=t.numel() - 1)
            hdr[torch.tensor(rows, device=device)] = t[g]
    hdr_host = hdr.cpu().numpy()
    heads, retry = [], []
    for i, nm in enumerate(names):
        t, o, n, st = where[i]
        if st not in (0, _lib.VX_INFLATE_CAPACITY) or (st == _lib.VX_INFLATE_CAPACITY and n < 352):
            raise _lib.VxError(f"{nm}: {status_name(st)} (status {st}, {n} bytes decoded)")
        h = parse_header(hdr_host[i][:min(n, 352)], str(nm))
        if st == _lib.VX_INFLATE_CAPACITY:
            retry.append((i, h.nbytes))
        heads.append(h)
    if retry:
        # ISIZE under-states a file of several members (it is the last member's size): decode again with the exact
        # size of the payload from its header
        items2 = [(C.c_void_p(src.data_ptr() + soffs[i]), len(raws[i]), _lib.VX_INFLATE_GZIP, nb) for i, nb in retry]
        dst2, offs2, n2, st2 = inflate_into(items2, device)
        for k, (i, nb) in enumerate(retry):
            if st2[k] != 0:
                raise _lib.VxError(f"{names[i]}: {status_name(st2[k])} (status {st2[k]}, {n2[k]} bytes decoded)")
            where[i] = [dst2, offs2[k], n2[k], 0]
    stages.mark()
    outs = []
    arr = (_lib.NiftiDecItem * len(raws))()
    for i, h in enumerate(heads):
        t, o, n, _ = where[i]
        if n < h.nbytes:
            raise ValueError(f"{names[i]}: {n} bytes hold no {h.shape} {h.dtype} volume at offset {h.data_offset}")
        out = torch.empty(h.shape, dtype=_torch_dtype(h.out_dtype), device=device)
        outs.append(out)
        it = arr[i]
        it.src, it.src_n, it.vox_offset = C.c_void_p(t.data_ptr() + o), n, h.data_offset
        it.dst, it.dst_n = C.c_void_p(out.data_ptr()) if out.numel() else None, out.numel() * out.element_size()
        it.ndim = len(h.shape)
        for a, d in enumerate(h.shape):
            it.dims[a] = d
        it.code, it.big_endian = h.code, int(h.endian == ">")
        it.out_dtype = -1 if not h.scaled else (_lib.VX_F32 if h.out_dtype == np.float32 else _lib.VX_F64)
        it.slope, it.inter = float(h.slope), float(h.inter)
    ws = torch.empty(int(_lib.load().vx_nifti_decode_workspace_bytes(len(raws))), dtype=torch.uint8, device=device)
    _lib.check(_lib.load().vx_nifti_decode(arr, len(raws), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "vx_nifti_decode")
    stages.mark()
    stages.add(("inflate_ms", "decode_ms"), {"payload_bytes": sum(h.nbytes for h in heads)})
    return [(o, h.header) for o, h in zip(outs, heads)]


class NiftiReader(PipelinedReader):
    """Pipelined load_device over batches of files: the files of batch i + 1 are read from disk on a thread pool while
    batch i is decoded on the device.  read(batches) yields one load_device result per batch, in order."""

    def _decode(self, names, raws, device):
        return _decode(names, raws, device, self._staging, self._timing)


def load_device(paths, device=None, _timing=None):
    """-> [(device tensor, header dict)] for a batch of .nii / .nii.gz files: the arrays and header dicts nifti.load
    returns, as tensors on `device` (default: the current device).  The files are read on a thread pool into a reused
    pinned buffer and uploaded in one copy; the .gz files are inflated in one vx_inflate call (capacities from their
    ISIZE trailers), the voxels decoded in one vx_nifti_decode call."""
    from . import _lib
    _lib.require_gpu()
    return load_once(NiftiReader, paths, device, _timing)
