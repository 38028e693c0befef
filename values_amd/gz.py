"""gzip members and CRC-32 computed on the device (values_amd/csrc/gzip.hip: vx_gzip_encode, vx_crc32).

The results writer (results.save_case_device) compresses every NIfTI payload of a case in one vx_gzip_encode call; these
wrappers expose the same encoder for any list of device byte tensors.  The members are complete RFC 1952 files:
gzip.decompress reads them.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

from . import _lib
from ._devio import current_device, decode_windows, plan

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


# ---------------------------------------------------------------------------------------------
# Decoding (values_amd/csrc/inflate.hip: vx_inflate)

FORMATS = {"gzip": _lib.VX_INFLATE_GZIP, "zlib": _lib.VX_INFLATE_ZLIB, "raw": _lib.VX_INFLATE_RAW}
MAX_RATIO = 1032   # DEFLATE expands at most 1032:1 (258-byte matches of 2 bits); a capacity that always suffices


def inflate_into(items: List[tuple], device, dst=None, offsets: Optional[Sequence[int]] = None):
    """items: (device pointer, src_n, format, capacity) -> (dst, offsets, sizes, statuses): one vx_inflate call, item i
    decoded into dst[offsets[i]:offsets[i] + sizes[i]] (dst: a device uint8 tensor; sizes / statuses: host lists).
    With dst and offsets given, item i is decoded into the caller's dst at offsets[i] (windows of `capacity` bytes that
    do not overlap); otherwise dst is allocated here, the windows back to back at 256-byte boundaries."""
    import torch
    if dst is None:
        offs, _, off = plan([(None, [(0, int(cap))]) for _, _, _, cap in items])
        dst = torch.empty(max(off, 1), dtype=torch.uint8, device=device)
    else:
        offs = [int(o) for o in offsets]
    if not items:
        return dst, offs, [], []
    arr = (_lib.InflateItem * len(items))()
    for i, (ptr, n, fmt, cap) in enumerate(items):
        arr[i].src, arr[i].src_n, arr[i].dst_off, arr[i].dst_cap, arr[i].format = ptr, int(n), offs[i], int(cap), int(fmt)
    sizes, statuses = decode_windows("vx_inflate", arr, dst, device)
    return dst, offs, sizes, statuses


def status_name(st: int) -> str:
    return _lib.INFLATE_STATUS[st] if 0 <= st < len(_lib.INFLATE_STATUS) else f"status {st}"


def gunzip(blobs, fmt: str = "gzip", sizes: Optional[Sequence[int]] = None, device=None) -> list:
    """One device uint8 tensor per compressed blob (bytes or a device uint8 tensor), all in one vx_inflate call --
    the counterpart of gzip_encode.  fmt: "gzip" (several members decode to their concatenation), "zlib" or "raw".
    sizes: the decoded sizes if known; otherwise a gzip blob's ISIZE trailer, else 4x the input, and an item that
    fills its window is decoded again with the DEFLATE bound.  A bad stream raises VxError naming the item and the
    status."""
    import torch
    _lib.require_gpu()
    if fmt not in FORMATS:
        raise ValueError(f"gunzip: format {fmt!r} (gzip, zlib or raw)")
    f = FORMATS[fmt]
    dev = current_device(device)
    srcs, keep = [], []
    for b in blobs:
        if isinstance(b, torch.Tensor):
            t = _bytes_view(b)
            srcs.append((t, t[-4:].cpu().numpy().tobytes() if t.numel() >= 4 else b""))
        else:
            mv = bytes(b)
            t = torch.frombuffer(bytearray(mv), dtype=torch.uint8).to(dev) if mv else torch.empty(0, dtype=torch.uint8, device=dev)
            srcs.append((t, mv[-4:]))
        keep.append(srcs[-1][0])
    if not srcs:
        return []
    caps = []
    for i, (t, tail) in enumerate(srcs):
        if sizes is not None:
            caps.append(int(sizes[i]))
        elif f == _lib.VX_INFLATE_GZIP and len(tail) == 4:
            caps.append(int.from_bytes(tail, "little"))
        else:
            caps.append(4 * t.numel() + 1024)
    items = [(_lib.ptr(t) if t.numel() else None, t.numel(), f, c) for (t, _), c in zip(srcs, caps)]
    dst, offs, out_n, st = inflate_into(items, dev)
    out = [None] * len(items)
    retry = []
    for i, s in enumerate(st):
        if s == _lib.VX_INFLATE_CAPACITY and sizes is None:
            retry.append(i)
        elif s != 0:
            raise _lib.VxError(f"gunzip: item {i}: {status_name(s)} (status {s}, {out_n[i]} bytes decoded)")
        else:
            out[i] = dst[offs[i]:offs[i] + out_n[i]]
    if retry:
        items2 = [(items[i][0], items[i][1], f, MAX_RATIO * items[i][1] + 64) for i in retry]
        dst2, offs2, n2, st2 = inflate_into(items2, dev)
        for k, i in enumerate(retry):
            if st2[k] != 0:
                raise _lib.VxError(f"gunzip: item {i}: {status_name(st2[k])} (status {st2[k]}, {n2[k]} bytes decoded)")
            out[i] = dst2[offs2[k]:offs2[k] + n2[k]].clone()
    return out
