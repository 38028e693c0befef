"""Minimal PNG (8-bit RGB / grey) and TIFF (32-bit float, single channel) codecs for the 2D results directory.

The reference writes the 2D outputs with OpenCV (test_2D.py:116-159): `cv2.imwrite(<id>_NN.png, BGR colour image)` for
the arg-max masks and `cv2.imwrite(<id>.tif, float32 map)` for the uncertainty maps, and the evaluation side reads them
back with cv2.imread.  OpenCV is not a dependency here; these writers produce standard files any reader (OpenCV,
PIL, tifffile) decodes to the same arrays.  Byte streams are not the same as OpenCV's (different deflate; the TIFFs are
uncompressed unless compression="lzw" is asked for): parity is on decoded content.  CPU I/O code -- not on the GPU path.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np


# ----------------------------------------------------------------------------------------------- PNG
def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, img: np.ndarray, level: int = 3) -> None:
    """img: (H, W, 3) RGB or (H, W) grey, uint8."""
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError("write_png: uint8 (H, W) or (H, W, 3) expected")
    h, w = a.shape[:2]
    color_type = 2 if a.ndim == 3 else 0
    rows = a.reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()   # filter type 0 on every scanline
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color_type, 0, 0, 0)))
        f.write(_chunk(b"IDAT", zlib.compress(raw, level)))
        f.write(_chunk(b"IEND", b""))


def png_parse(buf):
    """The layout of an 8-bit non-interlaced grey / RGB / RGBA PNG file held in `buf`:
    -> (w, h, ctype, bpp, [(offset, size) of every IDAT chunk's data]).  The chunks' data joined in order are one zlib
    stream; inflated, it is h rows of one filter byte and w * bpp pixel bytes.  Shared by read_png and the device reader
    (values_amd.images.load_png_device).  Not read: interlaced, palette, 16-bit and 1/2/4-bit files (ValueError)."""
    if bytes(buf[:8]) != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos + 8 <= len(buf):
        n, tag = struct.unpack(">I4s", buf[pos:pos + 8])
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", buf[pos + 8:pos + 8 + n])
        elif tag == b"IDAT":
            idat.append((pos + 8, min(n, len(buf) - pos - 8)))
        elif tag == b"IEND":
            break
        pos += 12 + n
    if hdr is None:
        raise ValueError("not a PNG file: no IHDR chunk")
    w, h, depth, ctype, _, _, interlace = hdr
    if depth != 8 or interlace != 0 or ctype not in (0, 2, 6):
        raise ValueError("read_png: only 8-bit non-interlaced grey/RGB/RGBA")
    return w, h, ctype, {0: 1, 2: 3, 6: 4}[ctype], idat


def read_png(path) -> np.ndarray:
    """8-bit grey / RGB / RGBA, non-interlaced (all five scanline filters).  None, Sub and Up rows are numpy row
    operations (Sub: a wrapping running sum per byte lane -- what OpenCV writes for every row of a mask); Average and Paeth
    rows run byte by byte."""
    with open(path, "rb") as f:
        buf = f.read()
    w, h, _, bpp, spans = png_parse(buf)
    return _png_unfilter(path, buf, w, h, bpp, spans)


def _png_unfilter(path, buf, w, h, bpp, spans) -> np.ndarray:
    """the IDAT spans of `buf` inflated and their scanlines reconstructed: (h, w) for bpp 1, else (h, w, bpp)"""
    raw = np.frombuffer(zlib.decompress(b"".join(buf[o:o + n] for o, n in spans)), dtype=np.uint8).reshape(h, 1 + w * bpp)
    out = np.zeros((h, w * bpp), dtype=np.uint8)
    prev = np.zeros(w * bpp, dtype=np.int32)
    for y in range(h):
        ft, line = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 1:
            cur = np.cumsum(raw[y, 1:].reshape(w, bpp), axis=0, dtype=np.uint8).reshape(-1).astype(np.int32)
        elif ft == 2:
            cur = (line + prev) & 0xFF
        elif ft in (3, 4):  # average, Paeth: sequential along the scanline
            cur = np.zeros_like(line)
            for i in range(w * bpp):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (line[i] + pred) & 0xFF
        else:
            raise ValueError(f"read_png: {path}: row {y}: filter type {ft}")
        out[y] = cur
        prev = cur
    return out.reshape(h, w) if bpp == 1 else out.reshape(h, w, bpp)


def png_parse_indexed(buf):
    """The layout of an 8-bit non-interlaced PALETTE PNG (colour type 3) held in `buf`: -> (w, h, palette, [(offset, size)
    of every IDAT chunk's data]); palette is (256, 3) uint8 RGB, the PLTE chunk's entries padded with black (an index
    beyond the file's own palette is the file's error).  The inflated stream is h rows of one filter byte and w index
    bytes: one bpp = 1 image.  A tRNS chunk is not looked at.  Beside png_parse, which keeps refusing these files; the 2D
    preprocessing (values_amd.preprocess2d) is the only caller."""
    if bytes(buf[:8]) != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file")
    pos, idat, hdr, plte = 8, [], None, None
    while pos + 8 <= len(buf):
        n, tag = struct.unpack(">I4s", buf[pos:pos + 8])
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", buf[pos + 8:pos + 8 + n])
        elif tag == b"PLTE":
            plte = bytes(buf[pos + 8:pos + 8 + n])
        elif tag == b"IDAT":
            idat.append((pos + 8, min(n, len(buf) - pos - 8)))
        elif tag == b"IEND":
            break
        pos += 12 + n
    if hdr is None:
        raise ValueError("not a PNG file: no IHDR chunk")
    w, h, depth, ctype, _, _, interlace = hdr
    if depth != 8 or interlace != 0 or ctype != 3:
        raise ValueError("png_parse_indexed: only 8-bit non-interlaced palette files")
    if plte is None or len(plte) % 3 or not 3 <= len(plte) <= 768:
        raise ValueError("png_parse_indexed: no PLTE chunk of 1..256 entries")
    palette = np.zeros((256, 3), dtype=np.uint8)
    palette[:len(plte) // 3] = np.frombuffer(plte, np.uint8).reshape(-1, 3)
    return w, h, palette, idat


def png_color_type(buf) -> int:
    """the colour type byte of a PNG file's IHDR (-1: not a PNG file that starts with IHDR)"""
    if bytes(buf[:8]) != b"\x89PNG\r\n\x1a\n" or bytes(buf[12:16]) != b"IHDR" or len(buf) < 26:
        return -1
    return buf[25]


def read_png_any(path) -> np.ndarray:
    """read_png, and palette files besides: those come back expanded to (H, W, 3) RGB, as cv2.imread(path, -1) followed
    by BGR2RGB gives them."""
    with open(path, "rb") as f:
        buf = f.read()
    if png_color_type(buf) != 3:
        return read_png(path)
    w, h, palette, spans = png_parse_indexed(buf)
    return palette[_png_unfilter(path, buf, w, h, 1, spans)]


# ----------------------------------------------------------------------------------------------- TIFF
def tiff_f32_parts(h: int, w: int):
    """(head, tail) of write_tiff_f32's file for an (h, w) float32 map: the file is head + the map's 4 h w little-endian
    bytes + tail (8-byte header, the pixel strip, then the IFD).  The 2D device writer (results2d.save_images_device)
    wraps the map bytes it copies back from the device in these."""
    nbytes = 4 * h * w
    tags = [  # (tag, type, count, value)   type 3 = SHORT, 4 = LONG
        (256, 4, 1, w), (257, 4, 1, h), (258, 3, 1, 32), (259, 3, 1, 1), (262, 3, 1, 1), (273, 4, 1, 8),
        (277, 3, 1, 1), (278, 4, 1, h), (279, 4, 1, nbytes), (284, 3, 1, 1), (339, 3, 1, 3),
    ]
    ifd_off = 8 + nbytes
    pad = b""
    if ifd_off % 2:
        pad = b"\x00"
        ifd_off += 1
    ifd = struct.pack("<H", len(tags))
    for tag, typ, cnt, val in tags:
        ifd += struct.pack("<HHI", tag, typ, cnt) + (struct.pack("<HH", val, 0) if typ == 3 else struct.pack("<I", val))
    ifd += struct.pack("<I", 0)
    return b"II*\x00" + struct.pack("<I", ifd_off), pad + ifd


def lzw_bound(n: int) -> int:
    """The largest strip lzw_encode makes of n bytes (vx_tiff_lzw_bound): at most n data codes, one ClearCode at the start
    and one more per 3836 table insertions, one EndOfInformation, each at most 12 bits."""
    return (12 * (n + n // 3836 + 2) + 7) // 8


def lzw_encode(data) -> bytes:
    """data -> a TIFF LZW strip (TIFF 6.0 section 13 with libtiff's policy: ClearCode 256 first, greedy longest match,
    codes MSB first, 9 to 12 bits, early change, a ClearCode when the next free entry would be 4094, EndOfInformation 257,
    the last byte zero-padded).  Greedy matching with a fixed reset rule has one output per input: the device encoder
    (vx_tiff_lzw_encode) writes the same bytes.  Plain Python like lzw_decode: a reference writer, correct and not fast."""
    out = bytearray()
    acc = nacc = 0
    table = {}
    nxt, k = 258, 0       # the next free entry; codes since the last ClearCode
    width = 9             # of the next code: the decoder's next free entry is 258 + k - 1 when it reads it

    def put(code):
        nonlocal acc, nacc
        acc = (acc << width) | code
        nacc += width
        while nacc >= 8:
            nacc -= 8
            out.append((acc >> nacc) & 0xFF)
        acc &= (1 << nacc) - 1

    put(256)
    w = -1
    for c in bytes(data):
        if w < 0:
            w = c
            continue
        key = (w << 8) | c
        hit = table.get(key)
        if hit is not None:
            w = hit
            continue
        put(w)
        k += 1
        nfree = 258 + k - 1
        width = 9 + (nfree >= 511) + (nfree >= 1023) + (nfree >= 2047)
        table[key] = nxt
        nxt += 1
        w = c
        if nxt >= 4094:
            put(256)
            table, nxt, k, width = {}, 258, 0, 9
    if w >= 0:
        put(w)
        k += 1
        nfree = 258 + k - 1
        width = 9 + (nfree >= 511) + (nfree >= 1023) + (nfree >= 2047)
    put(257)
    if nacc:
        out.append((acc << (8 - nacc)) & 0xFF)
    return bytes(out)


def _predict(m: np.ndarray, predictor: int) -> np.ndarray:
    """the forward predictor of tag 317 on the (h, w) float32 map m -> (h, 4 w) uint8, the bytes the strips of a
    little-endian file hold (the inverse of _unpredict)"""
    h, w = m.shape
    if predictor == 1:
        return np.ascontiguousarray(m, dtype="<f4").view(np.uint8).reshape(h, 4 * w)
    if predictor == 2:       # horizontal differencing on the 32-bit words
        words = np.ascontiguousarray(m, dtype=np.float32).view(np.uint32)
        d = words.copy()
        d[:, 1:] -= words[:, :-1]
        return np.ascontiguousarray(d.astype("<u4")).view(np.uint8).reshape(h, 4 * w)
    # 3, libtiff's fpDiff: the row's four byte planes, the most significant bytes first, then a byte difference over the row
    planes = np.ascontiguousarray(np.ascontiguousarray(m, dtype=">f4").view(np.uint8).reshape(h, w, 4).transpose(0, 2, 1)).reshape(h, 4 * w)
    d = planes.copy()
    d[:, 1:] -= planes[:, :-1]
    return d


def tiff_rows_per_strip(h: int, w: int, rows_per_strip=None) -> int:
    """RowsPerStrip of an LZW file: the argument capped at h, by default libtiff's 8 KiB rule max(1, 8192 // (4 w))"""
    rps = max(1, 8192 // (4 * w)) if rows_per_strip is None else int(rows_per_strip)
    if rps < 1:
        raise ValueError(f"write_tiff_f32: rows_per_strip={rows_per_strip}")
    return min(rps, h)


def tiff_lzw_parts(h: int, w: int, strip_sizes, rows_per_strip: int, predictor: int):
    """(head, tail) of write_tiff_f32(compression="lzw")'s file for an (h, w) float32 map whose LZW strips have the given
    sizes: the file is head + the strips back to back from offset 8 in row order + tail (a pad byte where the IFD would
    start at an odd offset, the IFD, then the StripOffsets and StripByteCounts arrays; with one strip both are inline).
    The 2D device writer (results2d.save_images_device(tiff="lzw")) wraps the strips it copies back in these."""
    sizes = [int(v) for v in strip_sizes]
    n = len(sizes)
    if predictor not in (1, 2, 3):
        raise ValueError(f"write_tiff_f32: predictor={predictor}: 1, 2 or 3")
    if rows_per_strip < 1 or n != -(-h // rows_per_strip):
        raise ValueError(f"write_tiff_f32: {n} strips for {h} rows of {rows_per_strip} per strip")
    offs, o = [], 8
    for v in sizes:
        offs.append(o)
        o += v
    pad = b"\x00" * (o % 2)
    ifd_off = o + len(pad)
    ntags = 12
    extra_off = ifd_off + 2 + 12 * ntags + 4
    tags = [  # (tag, type, count, value)   type 3 = SHORT, 4 = LONG
        (256, 4, 1, w), (257, 4, 1, h), (258, 3, 1, 32), (259, 3, 1, 5), (262, 3, 1, 1),
        (273, 4, n, offs[0] if n == 1 else extra_off), (277, 3, 1, 1), (278, 4, 1, rows_per_strip),
        (279, 4, n, sizes[0] if n == 1 else extra_off + 4 * n), (284, 3, 1, 1), (317, 3, 1, predictor), (339, 3, 1, 3),
    ]
    ifd = struct.pack("<H", ntags)
    for tag, typ, cnt, val in tags:
        ifd += struct.pack("<HHI", tag, typ, cnt) + (struct.pack("<HH", val, 0) if typ == 3 else struct.pack("<I", val))
    ifd += struct.pack("<I", 0)
    if n > 1:
        ifd += struct.pack(f"<{n}I", *offs) + struct.pack(f"<{n}I", *sizes)
    return b"II*\x00" + struct.pack("<I", ifd_off), pad + ifd


def write_tiff_f32(path, img: np.ndarray, compression=None, predictor: int = 3, rows_per_strip=None) -> None:
    """img (H, W) float32 -> a little-endian TIFF, SampleFormat = IEEE float.  compression=None: baseline, one
    uncompressed strip (predictor and rows_per_strip are not looked at).  compression="lzw": Compression 5 with Predictor
    1, 2 (horizontal differencing) or 3 (floating point), what libtiff writes; strips of rows_per_strip rows (default:
    libtiff's 8 KiB rule, max(1, 8192 // (4 W)), capped at H; the last strip may be shorter), laid out as tiff_lzw_parts
    says."""
    a = np.ascontiguousarray(img, dtype="<f4")
    if a.ndim != 2:
        raise ValueError("write_tiff_f32: (H, W) expected")
    if compression is None:
        head, tail = tiff_f32_parts(*a.shape)
        body = [a.tobytes()]
    elif compression == "lzw":
        h, w = a.shape
        if predictor not in (1, 2, 3):
            raise ValueError(f"write_tiff_f32: predictor={predictor}: 1, 2 or 3")
        rps = tiff_rows_per_strip(h, w, rows_per_strip)
        rows = _predict(a, predictor)
        body = [lzw_encode(rows[r:r + rps].tobytes()) for r in range(0, h, rps)]
        head, tail = tiff_lzw_parts(h, w, [len(b) for b in body], rps, predictor)
    else:
        raise ValueError(f"write_tiff_f32: compression={compression!r}: None or \"lzw\"")
    with open(path, "wb") as f:
        f.write(head)
        for b in body:
            f.write(b)
        f.write(tail)


class TiffLayout:
    """What tiff_parse reads from a single-channel float32 strip TIFF: w, h, endian ("<" / ">"), deflate (the strips are
    zlib streams), lzw (the strips are LZW streams), predictor (tag 317: 1, or 2 / 3 with lzw) and strips: [(first row,
    rows, offset, size)] in row order."""

    __slots__ = ("w", "h", "endian", "deflate", "lzw", "predictor", "strips")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def tiff_parse(buf, name: str = "") -> TiffLayout:
    """The layout of a single-channel 32-bit float strip TIFF held in `buf` (either byte order; any RowsPerStrip;
    Compression 1 = none or 8 / 32946 = Deflate with Predictor 1; Compression 5 = LZW -- what libtiff writes: cv2.imwrite,
    PIL, GDAL -- with Predictor 1, 2 = horizontal differencing or 3 = floating point).  Shared by read_tiff_f32 and the
    device reader (values_amd.images.load_tiff_device).  A predictor with Deflate or uncompressed strips is not decoded:
    ValueError naming the tag and its value."""
    pre = f"{name}: " if name else ""
    bo = {b"II": "<", b"MM": ">"}.get(bytes(buf[:2]))
    if bo is None or len(buf) < 8 or struct.unpack(bo + "H", buf[2:4])[0] != 42:
        raise ValueError(f"{pre}not a TIFF file")
    off = struct.unpack(bo + "I", buf[4:8])[0]
    n = struct.unpack(bo + "H", buf[off:off + 2])[0]
    tags = {}
    for i in range(n):
        e = buf[off + 2 + 12 * i: off + 14 + 12 * i]
        tag, typ, cnt = struct.unpack(bo + "HHI", e[:8])
        size = {1: 1, 3: 2, 4: 4}.get(typ)
        if size is None:
            continue
        fmt = {1: "B", 3: "H", 4: "I"}[typ]
        if size * cnt <= 4:
            vals = struct.unpack(bo + fmt * cnt, e[8:8 + size * cnt])
        else:
            p = struct.unpack(bo + "I", e[8:12])[0]
            vals = struct.unpack(bo + fmt * cnt, buf[p:p + size * cnt])
        tags[tag] = vals
    w, h = tags[256][0], tags[257][0]
    comp, pred = tags.get(259, (1,))[0], tags.get(317, (1,))[0]
    if comp not in (1, 5, 8, 32946):
        raise ValueError(f"{pre}read_tiff_f32: Compression (tag 259) = {comp}: only 1 (none), 5 (LZW) and 8 / 32946 (Deflate)")
    if comp == 5 and pred not in (1, 2, 3):
        raise ValueError(f"{pre}read_tiff_f32: Predictor (tag 317) = {pred}: only 1 (none), 2 and 3 with LZW")
    if comp != 5 and pred != 1:
        what = " (floating point)" if pred == 3 else ""
        raise ValueError(f"{pre}read_tiff_f32: Predictor (tag 317) = {pred}{what}: only 1 (none)")
    if tags.get(258, (0,))[0] != 32 or tags.get(339, (1,))[0] != 3 or tags.get(277, (1,))[0] != 1:
        raise ValueError(f"{pre}read_tiff_f32: only single-channel 32-bit float")
    rps = min(tags.get(278, (h,))[0], h) or h
    offs, counts = tags[273], tags[279]
    if len(offs) != len(counts) or len(offs) != -(-h // rps):
        raise ValueError(f"{pre}read_tiff_f32: {len(offs)} strip offsets, {len(counts)} byte counts for {h} rows of {rps} per strip")
    strips = []
    for k, (o, c) in enumerate(zip(offs, counts)):
        if o + c > len(buf):
            raise ValueError(f"{pre}read_tiff_f32: strip {k} [{o}, +{c}) beyond the file's {len(buf)} bytes")
        strips.append((k * rps, min(rps, h - k * rps), o, c))
    return TiffLayout(w=w, h=h, endian=bo, deflate=comp in (8, 32946), lzw=comp == 5, predictor=pred, strips=strips)


def lzw_decode(data, want: int):
    """The first `want` bytes a TIFF LZW strip (TIFF 6.0 section 13: codes MSB first, 9 to 12 bits, ClearCode 256,
    EndOfInformation 257, early change) decodes to -> (bytes, None) or (bytes so far, what went wrong).  As libtiff's
    decoder: the strip ends when `want` bytes are there, whatever follows, or at EndOfInformation; with a full table and
    no ClearCode it goes on at 12 bits without new entries.  The first code must be ClearCode (the old LSB-first
    variant is not decoded)."""
    out = bytearray()
    table = None           # strings of the entries from 258 on
    prev = None
    acc = nacc = 0
    width, i, n, k = 9, 0, len(data), 0
    while len(out) < want:
        while nacc < width:
            if i >= n:
                return bytes(out), "the strip ends before EndOfInformation or its last row"
            acc = ((acc << 8) | data[i]) & 0xFFFFFFFF
            i += 1
            nacc += 8
        nacc -= width
        code = (acc >> nacc) & ((1 << width) - 1)
        if code == 256:
            table, prev, width, k = [], None, 9, 0
            continue
        if table is None:
            return bytes(out), f"the first code is {code}, not ClearCode (256)"
        if code == 257:
            break
        if code < 256:
            cur = bytes((code,))
        elif prev is not None and code - 258 < len(table):
            cur = table[code - 258]
        elif prev is not None and code - 258 == len(table):
            cur = prev + prev[:1]          # KwKwK
        else:
            return bytes(out), f"code {code} above the next free entry ({258 + len(table)})"
        out += cur
        if prev is not None and len(table) < 4096 - 258:
            table.append(prev + cur[:1])
        prev = cur
        # the next free entry after this code: one entry per code after the first since the ClearCode
        k += 1
        nfree = 258 + k - 1
        width = 9 + (nfree >= 511) + (nfree >= 1023) + (nfree >= 2047)
    return bytes(out[:want]), None


def _unpredict(rows: np.ndarray, predictor: int, endian: str) -> np.ndarray:
    """rows: (n, 4 w) uint8, the decoded bytes of n rows -> (n, w) float32 with the predictor of tag 317 undone"""
    n, w = rows.shape[0], rows.shape[1] // 4
    if predictor == 2:       # horizontal differencing on the file's 32-bit words
        words = rows.view(endian + "u4").astype(np.uint32)
        return np.cumsum(words, axis=1, dtype=np.uint32).view(np.float32)
    # 3, libtiff's fpAcc: a running byte sum over the row, then sample x from the four byte planes, plane 0 the most
    # significant bytes -- in either byte order of the file
    acc = np.cumsum(rows, axis=1, dtype=np.uint8).reshape(n, 4, w)
    return np.ascontiguousarray(acc.transpose(0, 2, 1)).view(">f4").reshape(n, w).astype(np.float32)


def tiff_decode(buf, t: TiffLayout, name: str = "") -> np.ndarray:
    """The (h, w) float32 map of a file held in `buf` whose layout tiff_parse read.  LZW strips are decoded code by code
    in Python and the predictor undone with numpy: a reference reader like read_png's loop, correct and not fast (the
    fast path is values_amd.images.load_tiff_device)."""
    out = np.empty((t.h, t.w), dtype=np.float32)
    for r0, rows, o, c in t.strips:
        need = 4 * rows * t.w
        if t.lzw:
            data, err = lzw_decode(bytes(buf[o:o + c]), need)
            if err is None and len(data) < need:
                err = f"the strip holds {len(data)} bytes, {need} expected"
            if err is not None:
                raise ValueError(f"{name}: read_tiff_f32: Compression (tag 259) = 5 (LZW): strip at row {r0}: {err}")
            if t.predictor != 1:
                out[r0:r0 + rows] = _unpredict(np.frombuffer(data, np.uint8).reshape(rows, 4 * t.w), t.predictor, t.endian)
                continue
        else:
            data = zlib.decompress(buf[o:o + c]) if t.deflate else buf[o:o + c]
        if len(data) < need:
            raise ValueError(f"{name}: read_tiff_f32: strip at row {r0} holds {len(data)} bytes, {need} expected")
        out[r0:r0 + rows] = np.frombuffer(data, dtype=t.endian + "f4", count=rows * t.w).reshape(rows, t.w)
    return out


def read_tiff_f32(path) -> np.ndarray:
    """Reads what write_tiff_f32 writes and any single-channel float32 strip TIFF tiff_parse accepts: either byte order,
    several strips of any RowsPerStrip, uncompressed or Deflate without predictor, LZW with predictor 1, 2 or 3."""
    with open(path, "rb") as f:
        buf = f.read()
    return tiff_decode(buf, tiff_parse(buf, str(path)), str(path))
