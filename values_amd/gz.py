"""gzip members and CRC-32 computed on the device (values_amd/csrc/gzip.hip: vx_gzip_encode, vx_crc32).

The results writer (results.save_case_device) compresses every NIfTI payload of a case in one vx_gzip_encode call; these
wrappers expose the same encoder for any list of device byte tensors.  The members are complete RFC 1952 files:
gzip.decompress reads them.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

from . import _lib

MAX_HINT = 32768   # a DEFLATE distance reaches 32 KiB back


def _bytes_view(t):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.VxError("gz: expected a device tensor")
    t = t.contiguous()
    return t.view(-1).view(torch.uint8) if t.numel() else t.reshape(-1).to(torch.uint8)


def bound(n: int) -> int:
    """Worst-case size of the gzip member of n bytes (vx_gzip_bound)."""
    return int(_lib.load().vx_gzip_bound(int(n)))


def crc32(t) -> int:
    """zlib.crc32 of a device tensor's bytes, computed on the device."""
    import torch
    _lib.require_gpu()
    b = _bytes_view(t)
    out = torch.empty(1, dtype=torch.int32, device=b.device)
    _lib.check(_lib.load().vx_crc32(_lib.ptr(b), b.numel(), _lib.ptr(out), _lib.stream_ptr()), "vx_crc32")
    return int(out.item()) & 0xFFFFFFFF


def hints_for(esize: int, shape: Sequence[int]) -> tuple:
    """Stride hints of a Fortran-order volume of `shape` (x fastest) with `esize` bytes per element: the previous voxel,
    row and slice; a distance beyond the DEFLATE window is 0 (none)."""
    s = list(shape) + [1, 1, 1]
    d = (esize, esize * s[0], esize * s[0] * s[1])
    return tuple(int(v) if 0 < v <= MAX_HINT else 0 for v in d)


def encode_into(items: List[tuple], dst, out_sizes, workspace) -> None:
    """items: (device byte pointer, n, dst_off, hints) -> members at dst[dst_off:]; sizes to out_sizes (device int64).
    dst / workspace: device uint8 tensors sized with bound() / workspace_bytes()."""
    arr = (_lib.GzItem * len(items))()
    for i, (ptr, n, off, hints) in enumerate(items):
        arr[i].src = ptr
        arr[i].n = int(n)
        arr[i].dst_off = int(off)
        for k in range(3):
            arr[i].stride_hint[k] = int(hints[k]) if hints else 0
    _lib.check(_lib.load().vx_gzip_encode(arr, len(items), _lib.ptr(dst), dst.numel(), _lib.ptr(out_sizes),
                                          _lib.ptr(workspace), workspace.numel(), _lib.stream_ptr()), "vx_gzip_encode")


def workspace_bytes(sizes: Sequence[int]) -> int:
    a = (C.c_int64 * len(sizes))(*[int(n) for n in sizes])
    return int(_lib.load().vx_gzip_workspace_bytes(a, len(sizes)))


def gzip_encode(tensors, stride_hints: Optional[Sequence] = None) -> List[bytes]:
    """One gzip member per device tensor (its bytes), all in one vx_gzip_encode call.  stride_hints: per tensor a
    3-tuple of match distances (or None)."""
    import torch
    _lib.require_gpu()
    views = [_bytes_view(t) for t in tensors]
    if not views:
        return []
    hints = list(stride_hints) if stride_hints is not None else [None] * len(views)
    if len(hints) != len(views):
        raise ValueError("gzip_encode: one stride hint per tensor")
    offs, off = [], 0
    for v in views:
        offs.append(off)
        off += bound(v.numel())
    dev = views[0].device
    dst = torch.empty(max(off, 1), dtype=torch.uint8, device=dev)
    sizes = torch.empty(len(views), dtype=torch.int64, device=dev)
    ws = torch.empty(max(workspace_bytes([v.numel() for v in views]), 1), dtype=torch.uint8, device=dev)
    encode_into([(_lib.ptr(v) if v.numel() else None, v.numel(), o, h) for v, o, h in zip(views, offs, hints)], dst, sizes, ws)
    host = dst.cpu().numpy()
    return [host[o:o + int(n)].tobytes() for o, n in zip(offs, sizes.cpu().tolist())]
