"""Builders shared by tests/test_images_read_cpu.py and tests/test_gpu_images_read.py: PNG files with a chosen filter
per row (a numpy forward filter, then zlib.compress -- neither PIL nor OpenCV), float32 TIFF files in the layouts the
readers take or refuse, and the grid of shapes and row patterns of the unfilter tests."""
import struct
import zlib

import numpy as np

HS, WS, BPPS = (1, 2, 63, 64, 65, 130), (1, 2, 67), (1, 3, 4)   # a band edge (64 rows) before, at and after a row
PATTERNS = ("none", "sub", "up", "average", "paeth", "cyclic", "random")


def content(h, w, bpp, seed=0):
    """a smooth ramp with a noise band (rows h/4 .. h/2) and a flat band (rows from 3h/4: Paeth ties)"""
    rng = np.random.default_rng(seed + 1000 * h + 10 * w + bpp)
    yy, xx, cc = np.mgrid[0:h, 0:w, 0:bpp]
    a = (3 * xx + 2 * yy + 40 * cc) % 256
    a[h // 4:h // 2] = rng.integers(0, 256, a[h // 4:h // 2].shape)
    a[(3 * h) // 4:] = 200
    return a.astype(np.uint8)


def filters(pattern, h, seed=0):
    if pattern in PATTERNS[:5]:
        return np.full(h, PATTERNS.index(pattern), dtype=np.uint8)
    if pattern == "cyclic":
        return (np.arange(h) % 5).astype(np.uint8)
    return np.random.default_rng(seed + h).integers(0, 5, h).astype(np.uint8)


def scanlines(img, ft):
    """the PNG forward filter (RFC 2083 section 6): img (H, W, bpp) uint8, ft (H,) filter types -> the H * (1 + W * bpp)
    bytes a PNG's IDAT stream inflates to"""
    h, w, bpp = img.shape
    x = img.reshape(h, w * bpp).astype(np.int32)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = np.stack([np.zeros_like(x), a, b, (a + b) >> 1, paeth])
    rows = (x - pred[ft.astype(np.int64), np.arange(h)]) & 0xFF
    return np.concatenate([ft.reshape(h, 1).astype(np.uint8), rows.astype(np.uint8)], axis=1).tobytes()


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_bytes(img, ft, n_idat=1, level=6):
    """a PNG file of img ((H, W) or (H, W, 3 | 4) uint8) whose row y has filter ft[y]; the zlib stream cut into n_idat chunks"""
    a = img if img.ndim == 3 else img[..., None]
    h, w, bpp = a.shape
    z = zlib.compress(scanlines(a, ft), level)
    cuts = [len(z) * k // n_idat for k in range(n_idat + 1)]
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[bpp], 0, 0, 0))
    for k in range(n_idat):
        out += _chunk(b"IDAT", z[cuts[k]:cuts[k + 1]])
    return out + _chunk(b"IEND", b"")


def squeeze(img):
    return img[..., 0] if img.shape[-1] == 1 else img


def grid_cases():
    """(name, img (H, W, bpp), ft) for every shape and row pattern of the grid"""
    for h in HS:
        for w in WS:
            for bpp in BPPS:
                img = content(h, w, bpp)
                for pat in PATTERNS:
                    yield f"{h}x{w}x{bpp}-{pat}", img, filters(pat, h)


def tiff_bytes(m, endian="<", rows_per_strip=None, compression=1, predictor=None):
    """a single-channel float32 strip TIFF of the map m: either byte order, strips of rows_per_strip rows (default: one
    strip), compression 1 (none), 8 or 32946 (Deflate: zlib streams) -- or 5 with a placeholder payload, for the readers'
    refusal; predictor: the value of tag 317, or None for no tag"""
    h, w = m.shape
    rps = rows_per_strip or h
    data = [np.ascontiguousarray(m[r:r + rps], dtype=endian + "f4").tobytes() for r in range(0, h, rps)]
    if compression in (8, 32946):
        data = [zlib.compress(d, 6) for d in data]
    n = len(data)
    tags = [(256, 4, [w]), (257, 4, [h]), (258, 3, [32]), (259, 3, [compression]), (262, 3, [1]), (273, 4, None),
            (277, 3, [1]), (278, 4, [rps]), (279, 4, [len(d) for d in data])]
    if predictor is not None:
        tags.append((317, 3, [predictor]))
    tags.append((339, 3, [3]))
    ifd_off = 8
    ifd_len = 2 + 12 * len(tags) + 4
    extra_off = ifd_off + ifd_len                       # arrays too long for an entry's value field
    extra = b""
    strip0 = extra_off + (8 * n if n > 1 else 0)
    offs, o = [], strip0
    for d in data:
        offs.append(o)
        o += len(d)
    ifd = struct.pack(endian + "H", len(tags))
    for tag, typ, vals in tags:
        vals = offs if vals is None else vals
        fmt = {3: "H", 4: "I"}[typ]
        raw = struct.pack(endian + fmt * len(vals), *vals)
        if len(raw) <= 4:
            field = raw + b"\0" * (4 - len(raw))
        else:
            field = struct.pack(endian + "I", extra_off + len(extra))
            extra += raw
        ifd += struct.pack(endian + "HHI", tag, typ, len(vals)) + field
    ifd += struct.pack(endian + "I", 0)
    assert len(extra) == strip0 - extra_off
    head = (b"II" if endian == "<" else b"MM") + struct.pack(endian + "HI", 42, ifd_off)
    return head + ifd + extra + b"".join(data)


def mean_and_max(image, pred_model=None, unc_type=None, scale=1.0):
    """an aggregation `_target_` that runs without a device (values_amd.aggregation's run on the GPU)"""
    a = np.asarray(image, dtype=np.float64)
    return {"max_score": float(a.mean() * scale), "max": float(a.max()), "shape": list(a.shape)}
