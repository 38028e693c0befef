"""Reading the 2D results tree on the device: the PNG masks and float32 TIFF maps results2d.py writes (and any file
image_io.read_png / read_tiff_f32 read) as device tensors -- the 2D counterpart of nifti.load_device / NiftiReader.

    PNG    files read on a thread pool, png_parse on the host, the IDAT chunks' bytes joined in a pinned staging
           buffer and uploaded in one copy; one vx_inflate call (zlib) for the batch, then one vx_png_unfilter call
           reconstructs every image's scanlines into its own tensor.
    TIFF   tiff_parse on the host; every Deflate strip is one vx_inflate item that decodes straight into its rows of
           the map, an uncompressed strip is copied into place.  Every LZW strip (what libtiff writes: cv2.imwrite, PIL,
           GDAL) is one vx_tiff_lzw item: with predictor 1 it decodes straight into its rows of the map, with predictor
           2 or 3 into a scratch area of the same layout, and one vx_tiff_unpredict call undoes the predictor of every
           such file into its map.  The maps of a batch are views of one device buffer.  A big-endian file is decoded
           on the host and uploaded.

The arrays are the ones the host readers return: (H, W) or (H, W, 3 | 4) uint8, (H, W) float32.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._devio import PipelinedReader, Stages, decode_windows, item_statuses, load_once, plan
from .image_io import png_parse, tiff_decode, tiff_parse
from .nifti import MAX_FILE

PNG_ENDINGS, TIFF_ENDINGS = (".png",), (".tif", ".tiff")


def kind_of(path) -> str:
    """"png" / "tiff" by the file's ending, else ValueError."""
    p = str(path).lower()
    if p.endswith(PNG_ENDINGS):
        return "png"
    if p.endswith(TIFF_ENDINGS):
        return "tiff"
    raise ValueError(f"{path}: neither a .png nor a .tif / .tiff file")


def png_unfilter(entries, device):
    """entries: (src pointer, src_n, H, W, bpp, dst pointer) -> the items' statuses (host list): one vx_png_unfilter call."""
    if not entries:
        return []
    arr = (_lib.PngUnfilterItem * len(entries))()
    for it, (src, n, h, w, bpp, dst) in zip(arr, entries):
        it.src, it.src_n, it.dst, it.H, it.W, it.bpp = src, int(n), dst, int(h), int(w), int(bpp)
    return item_statuses("vx_png_unfilter", arr, device)


def lzw_into(items, device, dst):
    """items: (device pointer, src_n, dst_off, capacity) -> (sizes, statuses), host lists: one vx_tiff_lzw call, item i
    decoded into dst[dst_off:dst_off + capacity] (dst: a device uint8 tensor; the windows do not overlap)."""
    if not items:
        return [], []
    arr = (_lib.TiffLzwItem * len(items))()
    for it, (ptr, n, off, cap) in zip(arr, items):
        it.src, it.src_n, it.dst_off, it.dst_cap = ptr, int(n), int(off), int(cap)
    return decode_windows("vx_tiff_lzw", arr, dst, device)


def tiff_unpredict(entries, device):
    """entries: (src pointer, dst pointer, rows, W, predictor) -> the items' statuses (host list): one vx_tiff_unpredict
    call over float32 rows of little-endian files."""
    if not entries:
        return []
    arr = (_lib.TiffUnpredictItem * len(entries))()
    for it, (src, dst, rows, w, pred) in zip(arr, entries):
        it.src, it.dst, it.rows, it.W, it.predictor = src, dst, int(rows), int(w), int(pred)
    return item_statuses("vx_tiff_unpredict", arr, device)


def lzw_status_name(st: int) -> str:
    return _lib.LZW_STATUS[st] if 0 <= st < len(_lib.LZW_STATUS) else f"status {st}"


def _decode_png(names, raws, device, staging, timing=None, heads=None):
    """heads: the files' (w, h, ctype, bpp, IDAT spans) where the caller has parsed them already (preprocess2d: a palette
    file is a bpp = 1 image of indices); None: png_parse"""
    import torch
    from .gz import inflate_into, status_name
    parsed, heads = heads, []
    for k, (nm, r) in enumerate(zip(names, raws)):
        if len(r) >= MAX_FILE:
            raise ValueError(f"{nm}: {len(r)} bytes: files of 4 GiB or more are not read on the device")
        try:
            heads.append(png_parse(r) if parsed is None else parsed[k])
        except ValueError as e:
            raise ValueError(f"{nm}: {e}") from None
    src, soffs, sizes = staging.upload([(r, h[4]) for r, h in zip(raws, heads)], device)
    stages = Stages(timing)
    stages.mark()
    need = [h * (1 + w * bpp) for w, h, _, bpp, _ in heads]
    items = [(C.c_void_p(src.data_ptr() + o) if n else None, n, _lib.VX_INFLATE_ZLIB, cap)
             for o, n, cap in zip(soffs, sizes, need)]
    lines, loffs, ln, st = inflate_into(items, device)
    for nm, s, n in zip(names, st, ln):
        if s != 0:
            raise _lib.VxError(f"{nm}: IDAT: {status_name(s)} (status {s}, {n} bytes decoded)")
    stages.mark()
    outs = [torch.empty((h, w) if bpp == 1 else (h, w, bpp), dtype=torch.uint8, device=device) for w, h, _, bpp, _ in heads]
    st = png_unfilter([(C.c_void_p(lines.data_ptr() + lo), n, h, w, bpp, C.c_void_p(out.data_ptr()))
                       for lo, n, (w, h, _, bpp, _), out in zip(loffs, ln, heads, outs)], device)
    for nm, s in zip(names, st):
        if s != 0:
            what = _lib.PNG_STATUS[s] if 0 <= s < len(_lib.PNG_STATUS) else "?"
            raise _lib.VxError(f"{nm}: scanlines: {what} (status {s})")
    stages.mark()
    stages.add(("inflate_ms", "unfilter_ms"), {"payload_bytes": sum(need)})
    return outs


def _decode_tiff(names, raws, device, staging, timing=None):
    import torch
    from .gz import inflate_into, status_name
    lay = [tiff_parse(r, str(nm)) for nm, r in zip(names, raws)]
    on_dev = [i for i, t in enumerate(lay) if t.endian == "<"]
    # the maps of the batch: one buffer, every map at a 256-byte boundary; behind them, where a file has a predictor,
    # a scratch area of the same layout for the strips as they decode
    offs, _, off = plan([(None, [(0, 4 * lay[i].h * lay[i].w)]) for i in on_dev])
    moffs = dict(zip(on_dev, offs))
    predicted = [i for i in on_dev if lay[i].lzw and lay[i].predictor != 1]
    maps = torch.empty(max(off * (2 if predicted else 1), 1), dtype=torch.uint8, device=device)
    strips = [(i, s) for i in on_dev for s in lay[i].strips]
    src, soffs, sizes = staging.upload([(raws[i], [(s[2], s[3])]) for i, s in strips], device)
    stages = Stages(timing)
    stages.mark()
    items, at, who = [], [], []
    litems, lwho = [], []
    for (i, (r0, rows, _, _)), so, n in zip(strips, soffs, sizes):
        w = lay[i].w
        d0, nb = moffs[i] + 4 * r0 * w, 4 * rows * w
        if lay[i].deflate:
            items.append((C.c_void_p(src.data_ptr() + so) if n else None, n, _lib.VX_INFLATE_ZLIB, nb))
            at.append(d0)
            who.append((i, r0, nb))
        elif lay[i].lzw:
            litems.append((C.c_void_p(src.data_ptr() + so) if n else None, n, d0 + (off if lay[i].predictor != 1 else 0), nb))
            lwho.append((i, r0, nb))
        else:
            if n < nb:
                raise ValueError(f"{names[i]}: strip at row {r0} holds {n} bytes, {nb} expected")
            maps[d0:d0 + nb].copy_(src[so:so + nb])
    if items:
        _, _, dn, st = inflate_into(items, device, dst=maps, offsets=at)
        for (i, r0, nb), s, n in zip(who, st, dn):
            if s != 0 or n != nb:
                raise _lib.VxError(f"{names[i]}: strip at row {r0}: {status_name(s)} (status {s}, {n} of {nb} bytes decoded)")
    stages.mark()
    if litems:
        dn, st = lzw_into(litems, device, maps)
        for (i, r0, nb), s, n in zip(lwho, st, dn):
            if s != 0 or n != nb:
                raise _lib.VxError(f"{names[i]}: strip at row {r0}: LZW: {lzw_status_name(s)} (status {s}, {n} of {nb} bytes decoded)")
    stages.mark()
    if predicted:
        base = maps.data_ptr()
        tiff_unpredict([(C.c_void_p(base + off + moffs[i]), C.c_void_p(base + moffs[i]), lay[i].h, lay[i].w, lay[i].predictor)
                        for i in predicted if lay[i].h * lay[i].w], device)
    stages.mark()
    stages.add(("inflate_ms", "lzw_ms", "unpredict_ms"), {"payload_bytes": sum(4 * t.h * t.w for t in lay)})
    outs = []
    for i, t in enumerate(lay):
        if i in moffs:
            outs.append(maps[moffs[i]:moffs[i] + 4 * t.h * t.w].view(torch.float32).reshape(t.h, t.w))
        else:   # big endian: the host reader's array, uploaded
            out = tiff_decode(raws[i], t, str(names[i]))
            outs.append(torch.from_numpy(out).to(device))
    return outs


def _decode(names, raws, device, staging, timing=None):
    """the device half of one batch of file contents, PNG and TIFF files mixed: -> tensors in the order of `names`"""
    kinds = [kind_of(nm) for nm in names]
    outs = [None] * len(names)
    for kind, fn in (("png", _decode_png), ("tiff", _decode_tiff)):
        sel = [i for i, k in enumerate(kinds) if k == kind]
        if sel:
            for i, t in zip(sel, fn([names[i] for i in sel], [raws[i] for i in sel], device, staging, timing)):
                outs[i] = t
    return outs


def _load(paths, device, timing, kind):
    _lib.require_gpu()
    paths = [str(p) for p in paths]
    for p in paths:
        if kind_of(p) != kind:
            raise ValueError(f"{p}: not a {kind} file")
    return load_once(ImageReader, paths, device, timing)


class ImageReader(PipelinedReader):
    """Pipelined load_png_device / load_tiff_device over batches of files (PNG and TIFF may be mixed): the files of batch
    i + 1 are read from disk on a thread pool while batch i is decoded on the device.  read(batches) yields one list of
    tensors per batch, in order -- nifti.NiftiReader for the 2D tree."""

    def _decode(self, names, raws, device):
        return _decode(names, raws, device, self._staging, self._timing)


def load_png_device(paths, device=None, _timing=None):
    """-> [uint8 device tensor (H, W) or (H, W, 3 | 4)] for a batch of 8-bit non-interlaced PNG files: the arrays
    image_io.read_png returns, on `device` (default: the current device).  One vx_inflate call and one vx_png_unfilter
    call per batch; a bad stream raises VxError naming the file and the status."""
    return _load(paths, device, _timing, "png")


def load_tiff_device(paths, device=None, _timing=None):
    """-> [float32 device tensor (H, W)] for a batch of single-channel float32 strip TIFF files: the arrays
    image_io.read_tiff_f32 returns (uncompressed, Deflate or LZW strips; LZW with predictor 1, 2 or 3).  The tensors of a
    batch are views of one device buffer.  A strip that does not decode raises VxError naming the file, the strip's
    first row, the status and the bytes decoded of the bytes expected."""
    return _load(paths, device, _timing, "tiff")
