"""What the device results writers (results.py: 3D, results2d.py: 2D) share: the grow-only buffer set of one case or
batch in flight, the step that puts an encoded plan on disk, and the pipelined writer built on the two.  Below them, what
the device readers (nifti.py: 3D, images.py: 2D) share: the pinned staging buffer of a batch, the pipelined reader, the
one-shot loaders' shared reader, stage timing, and the batched decoder calls (gz.py, images.py).

An encoder is a function (bufs, *arguments) -> (plan, host, spans): the planned files (each with a `path` relative to the
save directory), the pinned host array their bytes were copied into, and per file the arguments of write_span after the
array: (offset, size) or (offset, size, head, tail).
"""
from __future__ import annotations

import os
import threading
from concurrent.futures import ThreadPoolExecutor

from . import _lib


class Buffers:
    """device payload / member / workspace buffers and the pinned host buffer of one case in flight (grown, never shrunk)"""

    def __init__(self):
        self.t = {}

    def get(self, name, nbytes, dev, pinned=False):
        import torch
        b = self.t.get(name)
        if b is None or b.numel() < nbytes:
            n = max(int(nbytes * 1.25), 1 << 16)
            b = torch.empty(n, dtype=torch.uint8, pin_memory=True) if pinned else torch.empty(n, dtype=torch.uint8, device=dev)
            self.t[name] = b
        return b


def write_span(path, buf, off, n, head=b"", tail=b""):
    """buf[off:off + n] to a new file, between `head` and `tail` (the host-built ends of a TIFF; a NIfTI member or a PNG
    file is complete on the device)"""
    with open(path, "wb") as fh:
        fh.write(head)
        fh.write(memoryview(buf)[off:off + n])
        fh.write(tail)


def emit(save_dir, dirs, encoded, run=lambda fn, *a: fn(*a)):
    """Creates `dirs` (the ones the host writer creates whatever it writes) and the plan's own directories under save_dir,
    then writes every planned file through run(write_span, ...); -> what the calls to `run` returned."""
    plan, host, spans = encoded
    for d in list(dirs) + [os.path.dirname(f.path) for f in plan]:
        os.makedirs(os.path.join(save_dir, d), exist_ok=True)
    return [run(write_span, os.path.join(save_dir, f.path), host, *sp) for f, sp in zip(plan, spans)]


_shared_bufs = Buffers()
_shared_lock = threading.Lock()


def save_once(save_dir, dirs, encode, *args):
    """The one-shot entry points: encode into the process-wide buffer set and write the files before returning, one
    call at a time."""
    with _shared_lock:
        emit(save_dir, dirs, encode(_shared_bufs, *args))


class PipelinedWriter:
    """submit() encodes a case or batch on the GPU and hands its files to a small thread pool, so the files of submission
    i are written while submission i + 1 is encoded.  Two buffer sets alternate; a set is reused only once its files are
    written.  close() (or leaving the `with` block) waits and re-raises the first write error.  A subclass sets `_encode`
    and `_dirs` and gives submit() its signature; its class name is the one the messages use."""

    _encode = None
    _dirs = ()

    def __init__(self, workers: int = 4):
        if workers < 1:
            raise ValueError(f"{type(self).__name__}: workers >= 1")
        self._pool = ThreadPoolExecutor(max_workers=int(workers))
        self._bufs = [Buffers(), Buffers()]
        self._pending = [[], []]
        self._all = []
        self._n = 0
        self._closed = False

    def _submit(self, save_dir, *args):
        if self._closed:
            raise RuntimeError(f"{type(self).__name__} is closed")
        k = self._n % 2
        self._n += 1
        for f in self._pending[k]:   # the buffer set's previous files must be on disk before it is overwritten
            f.exception()
        futs = emit(save_dir, self._dirs, self._encode(self._bufs[k], *args), self._pool.submit)
        self._pending[k] = futs
        self._all.extend(futs)

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        self._pool.shutdown(wait=True)
        for f in self._all:
            e = f.exception()
            if e is not None:
                raise e

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# ---------------------------------------------------------------------------------------------
# Reading

ALIGN = 256


def align(n: int) -> int:
    return (int(n) + ALIGN - 1) // ALIGN * ALIGN


def plan(pieces):
    """pieces: per item (bytes, [(offset, size)]), the spans of `bytes` that make up the item -> (offsets, sizes, total):
    the items back to back at 256-byte boundaries (an empty item still has a region of its own), each item's size the
    sum of its spans.  Only the spans are looked at."""
    offs, sizes, off = [], [], 0
    for _, spans in pieces:
        n = sum(s for _, s in spans)
        offs.append(off)
        sizes.append(n)
        off += align(max(n, 1))
    return offs, sizes, off


class Staging:
    """a pinned host buffer reused across batches (grown when a batch needs more): spans of the files' bytes are joined
    in it and uploaded in one copy; that copy is waited for before the buffer is written again"""

    def __init__(self):
        self.buf = None
        self.event = None

    def upload(self, pieces, device):
        """pieces: as plan() takes them -> (device uint8 tensor, item offsets, item sizes)"""
        import numpy as np
        import torch
        offs, sizes, off = plan(pieces)
        if self.event is not None:
            self.event.synchronize()
        if self.buf is None or self.buf.numel() < off:
            self.buf = torch.empty(max(off, 1 << 20), dtype=torch.uint8, pin_memory=True)
        host = self.buf.numpy()
        for (raw, spans), o in zip(pieces, offs):
            view = np.frombuffer(raw, np.uint8)
            for so, sn in spans:
                host[o:o + sn] = view[so:so + sn]
                o += sn
        dev = self.buf[:max(off, 1)].to(device, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        return dev, offs, sizes


def current_device(device=None):
    import torch
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


class Stages:
    """GPU time of the stages of a decode, added into a `timing` dict (None: nothing is recorded): mark() before the
    first stage and after every stage, then add(keys) adds the milliseconds between consecutive marks to timing[key]."""

    def __init__(self, timing):
        self.timing = timing
        self.marks = []

    def mark(self):
        if self.timing is not None:
            import torch
            self.marks.append(torch.cuda.Event(enable_timing=True))
            self.marks[-1].record()

    def add(self, keys, payload_bytes):
        if self.timing is not None:
            self.marks[-1].synchronize()
            for k, a, b in zip(keys, self.marks, self.marks[1:]):
                self.timing[k] = self.timing.get(k, 0.0) + a.elapsed_time(b)
            self.timing["payload_bytes"] = self.timing.get("payload_bytes", 0) + payload_bytes


def _read(path):
    with open(path, "rb") as f:
        return f.read()


class PipelinedReader:
    """read(batches) yields one decoded result per batch of files, in order: the files of batch i + 1 are read from disk
    on a thread pool while batch i is decoded on the device.  A subclass supplies _decode(names, raws, device), which
    may use the pinned staging buffer (self._staging) and fills self._timing where that is a dict; its class name is the
    one the messages use."""

    def __init__(self, device=None, workers: int = 8, _timing=None):
        if workers < 1:
            raise ValueError(f"{type(self).__name__}: workers >= 1")
        self.device = device
        self._pool = ThreadPoolExecutor(max_workers=int(workers))
        self._staging = Staging()
        self._timing = _timing

    def _decode(self, names, raws, device):
        raise NotImplementedError

    def _submit(self, batch):
        return [str(p) for p in batch], [self._pool.submit(_read, str(p)) for p in batch]

    def read(self, batches):
        _lib.require_gpu()
        dev = current_device(self.device)
        it = iter(batches)
        nxt = next(it, None)
        pending = self._submit(nxt) if nxt is not None else None
        while pending is not None:
            names, futs = pending
            nxt = next(it, None)
            raws = [f.result() for f in futs]
            pending = self._submit(nxt) if nxt is not None else None
            yield self._decode(names, raws, dev) if names else []

    def close(self):
        self._pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


_shared_readers = {}   # reader class -> (its lock, its reader)


def load_once(cls, paths, device=None, timing=None):
    """The one-shot entry points: read and decode one batch with the process-wide reader of class `cls` (its thread pool
    and pinned staging buffer), one call per class at a time."""
    paths = [str(p) for p in paths]
    if not paths:
        return []
    dev = current_device(device)
    with _shared_lock:
        if cls not in _shared_readers:
            _shared_readers[cls] = (threading.Lock(), cls())
        lock, reader = _shared_readers[cls]
    with lock:
        reader._timing = timing
        raws = list(reader._pool.map(_read, paths))
        return reader._decode(paths, raws, dev)


def decode_windows(name, arr, dst, device):
    """One call of the batched decoder `name` (vx_inflate, vx_tiff_lzw) over the item array `arr`, whose items name their
    windows of dst (a device uint8 tensor) -> (sizes, statuses), host lists."""
    import torch
    lib, n = _lib.load(), len(arr)
    res = torch.empty(n * 3, dtype=torch.int32, device=device)   # [sizes (int64) | statuses]
    sizes, status = res[:2 * n].view(torch.int64), res[2 * n:]
    ws = torch.empty(int(getattr(lib, name + "_workspace_bytes")(n)), dtype=torch.uint8, device=device)
    _lib.check(getattr(lib, name)(arr, n, _lib.ptr(dst), dst.numel(), _lib.ptr(sizes), _lib.ptr(status), _lib.ptr(ws), ws.numel(),
                                  _lib.stream_ptr()), name)
    host = res.cpu()
    return host[:2 * n].view(torch.int64).tolist(), host[2 * n:].tolist()


def item_statuses(name, arr, device):
    """One call of the batched pass `name` (vx_png_unfilter, vx_tiff_unpredict) over the item array `arr`, whose items
    carry their own pointers -> the items' statuses, a host list."""
    import torch
    lib, n = _lib.load(), len(arr)
    status = torch.empty(n, dtype=torch.int32, device=device)
    ws = torch.empty(int(getattr(lib, name + "_workspace_bytes")(n)), dtype=torch.uint8, device=device)
    _lib.check(getattr(lib, name)(arr, n, _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), name)
    return status.cpu().tolist()
