"""What the device results writers (results.py: 3D and maps, results2d.py: 2D) share: the grow-only buffer set of one case
or batch in flight, `gather` (the encoded regions into the pinned host buffer), the TIFF stage (raw or LZW float32
maps), the step that puts an encoded plan on disk, and the pipelined writer built on them.  Below them, what the device
readers (nifti.py: 3D, images.py: 2D) share: the pinned staging buffer of a batch, the pipelined reader, the one-shot
loaders' shared reader, and the batched decoder calls (gz.py, images.py).  Writers and readers time their stages with
`Stages`.

An encoder is a function (bufs, *arguments) -> (plan, host, spans): the planned files (each with a `path` relative to the
save directory), the pinned host array their bytes were copied into, and per file the arguments of write_span after the
array: (offset, size) or (offset, size, head, tail).
"""
from __future__ import annotations

import ctypes
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .image_io import lzw_bound, tiff_f32_parts, tiff_lzw_parts, tiff_rows_per_strip


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


class Stages:
    """GPU time of the stages of an encode or a decode, added into a `timing` dict (None: nothing is recorded): mark()
    before the first stage and after every stage, then add(keys, counters) adds the milliseconds between consecutive
    marks to timing[key] (a key of None: that interval is no stage) and every counter (bytes) to timing[its name]."""

    def __init__(self, timing):
        self.timing = timing
        self.marks = []

    def mark(self):
        if self.timing is not None:
            import torch
            self.marks.append(torch.cuda.Event(enable_timing=True))
            self.marks[-1].record()

    def add(self, keys, counters):
        if self.timing is not None:
            self.marks[-1].synchronize()
            for k, a, b in zip(keys, self.marks, self.marks[1:]):
                if k is not None:
                    self.timing[k] = self.timing.get(k, 0.0) + a.elapsed_time(b)
            for k, v in counters.items():
                self.timing[k] = self.timing.get(k, 0) + v


def gather(bufs, regions, dev):
    """regions: (device uint8 tensor, nbytes) each -> (the buffer set's pinned host buffer as a numpy array, each region's base in it): the
    regions at 16-byte multiples, one copy per region that holds bytes."""
    bases, total = [], 0
    for _, n in regions:
        bases.append(total)
        total += (n + 15) // 16 * 16
    host = bufs.get("host", total, dev, pinned=True)
    for (t, n), b in zip(regions, bases):
        if n:
            host[b:b + n].copy_(t[:n])
    return host.numpy(), bases


_LZW_ITEM = np.dtype([("src", "<u8"), ("src_n", "<i8"), ("dst_off", "<i8"), ("dst_cap", "<i8")])   # vx_tiff_lzw_item
_UNPREDICT_ITEM = np.dtype([("src", "<u8"), ("dst", "<u8"), ("rows", "<i4"), ("W", "<i4"), ("predictor", "<i4"), ("pad", "<i4")])


def _tiff_strips(shapes, rows_per_strip):
    """The LZW strips of a batch of (h, w) maps lying back to back: -> (per map (rows per strip, number of strips), table
    of vx_tiff_lzw_item whose src is the strip's byte offset in the maps, bytes of the windows)"""
    layout, parts, base, off = [], [], 0, 0
    for h, w in shapes:
        rps = tiff_rows_per_strip(h, w, rows_per_strip)
        r0 = np.arange(0, h, rps, dtype=np.int64)
        it = np.zeros(len(r0), dtype=_LZW_ITEM)
        it["src"] = base + 4 * w * r0
        it["src_n"] = 4 * w * np.minimum(rps, h - r0)
        it["dst_cap"] = lzw_bound(it["src_n"])
        win = (it["dst_cap"] + 15) // 16 * 16   # every window starts at a multiple of 16: whole-word stores
        it["dst_off"] = off + np.cumsum(win) - win
        off += int(win.sum())
        base += 4 * h * w
        layout.append((rps, len(r0)))
        parts.append(it)
    return layout, np.concatenate(parts), off


class TiffStage:
    """The float32 TIFF maps of a batch, uncompressed (tiff=None) or as LZW strips with Predictor 1, 2 or 3 (tiff="lzw"),
    planned from the maps' (h, w) shapes.  launch() puts the maps' file bytes -- all but the host-built ends -- into one
    device region; with LZW the strips' sizes, their places in the region and their statuses go to `place`, place_bytes
    of a device buffer the caller reads back in its one small read; finish() then gives the region's bytes and each
    map's (offset, size, head, tail).  `who` names the entry point in the messages."""

    def __init__(self, who, shapes, tiff=None, predictor=3, rows_per_strip=None):
        if tiff not in (None, "lzw"):
            raise ValueError(f"{who}: tiff={tiff!r}: None or \"lzw\"")
        if tiff == "lzw" and predictor not in (1, 2, 3):
            raise ValueError(f"{who}: tiff_predictor={predictor}: 1, 2 or 3")
        self.who, self.shapes, self.predictor = who, list(shapes), predictor
        self.lzw = tiff == "lzw" and bool(self.shapes)
        self.raw_bytes = sum(4 * h * w for h, w in self.shapes)
        self.ns = 0
        if self.lzw:
            self.layout, self.strips, self.win_bytes = _tiff_strips(self.shapes, rows_per_strip)
            self.ns = len(self.strips)
        self.place_bytes = 8 * (2 * self.ns + 1) + 4 * self.ns if self.lzw else 0

    def _place(self, buf):
        """[strip sizes | strip places, the region's bytes] int64, then the strips' statuses int32: views of buf"""
        import torch
        a, b = 8 * self.ns, 8 * (2 * self.ns + 1)
        return buf[:a].view(torch.int64), buf[a:b].view(torch.int64), buf[b:b + 4 * self.ns].view(torch.int32)

    def launch(self, bufs, maps, place, dev, stages):
        """maps: the (h, w) float32 device tensors -> the device region (uint8; None without maps).  LZW: vx_tiff_predict
        over all maps (predictor 2 / 3), vx_tiff_lzw_encode over all strips, vx_tiff_lzw_pack, a mark of `stages`
        before the first and after each."""
        import torch
        if not maps:
            return None
        flat = torch.cat([m.reshape(-1) for m in maps])
        if not self.lzw:
            return flat.view(torch.uint8)
        lib, n, shapes = _lib.load(), self.ns, self.shapes
        sizes, offsets, status = self._place(place)
        src = flat
        stages.mark()
        if self.predictor != 1:
            src = bufs.get("tif_pred", self.raw_bytes, dev)
            pi = np.zeros(len(shapes), dtype=_UNPREDICT_ITEM)
            o = 0
            for k, (h, w) in enumerate(shapes):
                pi[k] = (flat.data_ptr() + o, src.data_ptr() + o, h, w, self.predictor, 0)
                o += 4 * h * w
            pst = bufs.get("tif_pst", 4 * len(shapes), dev)
            ws = bufs.get("tif_pws", int(lib.vx_tiff_predict_workspace_bytes(len(shapes))), dev)
            _lib.check(lib.vx_tiff_predict(pi.ctypes.data_as(ctypes.POINTER(_lib.TiffUnpredictItem)), len(shapes), pst.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "vx_tiff_predict")
        stages.mark()
        items = self.strips.copy()
        items["src"] += src.data_ptr()
        table = items.ctypes.data_as(ctypes.POINTER(_lib.TiffLzwItem))
        win_bytes = self.win_bytes
        enc = bufs.get("tif_enc", win_bytes, dev)
        ws = bufs.get("tif_ws", max(int(lib.vx_tiff_lzw_encode_workspace_bytes(n)), int(lib.vx_tiff_lzw_pack_workspace_bytes(n))), dev)
        _lib.check(lib.vx_tiff_lzw_encode(table, n, enc.data_ptr(), win_bytes, sizes.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                          ws.numel(), _lib.stream_ptr()), "vx_tiff_lzw_encode")
        stages.mark()
        packed = bufs.get("tif_pack", win_bytes, dev)
        _lib.check(lib.vx_tiff_lzw_pack(table, n, enc.data_ptr(), win_bytes, sizes.data_ptr(), packed.data_ptr(), win_bytes,
                                        offsets.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "vx_tiff_lzw_pack")
        stages.mark()
        return packed

    def finish(self, place_host):
        """place_host: the host copy of `place` -> (bytes of the region, per map (offset, size, head, tail))"""
        if not self.lzw:
            parts, u = [], 0
            for h, w in self.shapes:   # TIFF: host-built header + the map's bytes + IFD
                parts.append((u, 4 * h * w) + tiff_f32_parts(h, w))
                u += 4 * h * w
            return u, parts
        sizes, _, status = (v.tolist() for v in self._place(place_host))
        bad = [i for i, v in enumerate(status) if v != _lib.VX_LZW_OK]
        if bad:
            raise RuntimeError(f"{self.who}: vx_tiff_lzw_encode: strip {bad[0]} of the batch did not fit its window")
        parts, u, s0 = [], 0, 0
        for (h, w), (rps, cnt) in zip(self.shapes, self.layout):   # host-built header + the map's strips + IFD and strip table
            mine = sizes[s0:s0 + cnt]
            parts.append((u, sum(mine)) + tiff_lzw_parts(h, w, mine, rps, self.predictor))
            u += sum(mine)
            s0 += cnt
        return u, parts


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
