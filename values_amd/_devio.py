"""What the device results writers (results.py: 3D, results2d.py: 2D) share: the grow-only buffer set of one case or
batch in flight, the step that puts an encoded plan on disk, and the pipelined writer built on the two.

An encoder is a function (bufs, *arguments) -> (plan, host, spans): the planned files (each with a `path` relative to the
save directory), the pinned host array their bytes were copied into, and per file the arguments of write_span after the
array: (offset, size) or (offset, size, head, tail).
"""
from __future__ import annotations

import os
import threading
from concurrent.futures import ThreadPoolExecutor


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
