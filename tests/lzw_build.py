"""Builders shared by tests/test_tiff_lzw_cpu.py and tests/test_gpu_tiff_lzw.py: a TIFF LZW encoder of this project's
own (TIFF 6.0 section 13; neither PIL nor libtiff), the forward predictors 2 and 3 in numpy, a strip TIFF around them
(modelled on png_build.tiff_bytes), and the host reference decoder built from values_amd/csrc/lzw_core.h
(tests/lzw_host.cpp).  The encoder is validated against libtiff in tests/test_tiff_lzw_cpu.py: every variant it writes
decodes, through PIL, to its source."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_LZW = os.path.join(ROOT, "tests", "golden", "tiff_lzw")
OK, TRUNCATED, BAD_CODE = 0, 1, 2
CLEAR, EOI, FIRST, LAST = 256, 257, 258, 4095


class _Bits:
    """codes packed MSB first"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, code, width):
        self.acc = (self.acc << width) | code
        self.n += width
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 0xFF)
        return bytes(self.out)


def _width(k):
    """the width of the code that follows k codes since the last ClearCode: the decoder's next free entry is then
    258 + k - 1 (one entry per code after the first), and the width grows when that reaches 511, 1023, 2047"""
    nfree = FIRST + max(k, 1) - 1
    return 9 + (nfree >= 511) + (nfree >= 1023) + (nfree >= 2047)


def lzw_encode(data, defer=0, eoi=True, early_eoi=None, mid_clear=None, clear_at=4094):
    """data -> an LZW strip.  The table is cleared when its next entry would be `clear_at` (libtiff's encoder: 4094), or
    with defer > 0: only `defer` codes after the table is full (4096 entries), decoding going on at 12 bits without new
    entries meanwhile.  eoi=False: no EndOfInformation.  early_eoi=n: only the first n bytes are encoded, then
    EndOfInformation.  mid_clear=n: an extra ClearCode at the first code boundary at or after n bytes."""
    data = bytes(data if early_eoi is None else data[:early_eoi])
    b = _Bits()
    b.put(CLEAR, 9)
    table, nxt, k, since_full = {}, FIRST, 0, 0
    w = None
    for pos, c in enumerate(data):
        if w is None:
            w = c
            continue
        key = (w << 8) | c
        hit = table.get(key)
        if hit is not None:
            w = hit
            continue
        b.put(w, _width(k))
        k += 1
        if nxt <= LAST:
            table[key] = nxt
            nxt += 1
        else:
            since_full += 1
        w = c
        clear = (nxt >= clear_at) if not defer else (nxt > LAST and since_full >= defer)
        if mid_clear is not None and pos >= mid_clear:
            clear, mid_clear = True, None
        if clear:
            b.put(CLEAR, _width(k))
            table, nxt, k, since_full = {}, FIRST, 0, 0
    if w is not None:
        b.put(w, _width(k))
        k += 1
    if eoi:
        b.put(EOI, _width(k))
    return b.done()


def lzw_encode_run(byte, n, defer=0, eoi=True, clear_at=4094):
    """lzw_encode(bytes([byte]) * n, ...) without walking the bytes: after a ClearCode the codes of a constant run are the
    byte, then 258, 259, ... -- each the entry the decoder has not finished yet (KwKwK), one byte longer than the last"""
    b = _Bits()
    b.put(CLEAR, 9)
    nxt, k, since_full, rem = FIRST, 0, 0, n
    while rem > 0:
        longest = 1 if k == 0 else nxt - FIRST + 1 if nxt <= LAST else LAST - FIRST + 2   # the longest entry's bytes
        if k == 0 or rem == 1:
            code, ln = byte, 1
        else:
            ln = min(longest, rem)
            code = FIRST + ln - 2
        if rem == ln:                  # the last code: nothing follows it
            b.put(code, _width(k))
            k += 1
            break
        b.put(code, _width(k))
        k += 1
        rem -= ln
        if nxt <= LAST:
            nxt += 1
        else:
            since_full += 1
        clear = (nxt >= clear_at) if not defer else (nxt > LAST and since_full >= defer)
        if clear:
            b.put(CLEAR, _width(k))
            nxt, k, since_full = FIRST, 0, 0
    if eoi:
        b.put(EOI, _width(k))
    return b.done()


def predict2(m, endian="<"):
    """forward predictor 2 on the float32 map m: per row, word[i] -= word[i - 1] mod 2^32 -> (h, 4 w) uint8, the bytes
    of the file's rows"""
    words = np.ascontiguousarray(m, dtype=np.float32).view(np.uint32)
    d = words.copy()
    d[:, 1:] = words[:, 1:] - words[:, :-1]
    return np.ascontiguousarray(d.astype(endian + "u4")).view(np.uint8).reshape(m.shape[0], -1)


def predict3(m):
    """forward predictor 3 (libtiff's fpDiff) on the float32 map m: per row the four byte planes, the most significant
    bytes first, then byte[i] -= byte[i - 1] mod 256 over the row's 4 w bytes -> (h, 4 w) uint8 (either byte order)"""
    h, w = m.shape
    be = np.ascontiguousarray(m, dtype=">f4").view(np.uint8).reshape(h, w, 4)
    planes = np.ascontiguousarray(be.transpose(0, 2, 1)).reshape(h, 4 * w)
    d = planes.copy()
    d[:, 1:] = planes[:, 1:] - planes[:, :-1]
    return d


def row_bytes(m, endian="<", predictor=1):
    """(h, 4 w) uint8: what the strips of the file decode to"""
    if predictor == 2:
        return predict2(m, endian)
    if predictor == 3:
        return predict3(m)
    return np.ascontiguousarray(m, dtype=endian + "f4").view(np.uint8).reshape(m.shape[0], -1)


def tiff_file(h, w, strips, endian="<", rows_per_strip=None, compression=5, predictor=None):
    """a single-channel float32 strip TIFF around the given strip payloads (png_build.tiff_bytes' layout)"""
    rps = rows_per_strip or h
    n = len(strips)
    assert n == -(-h // rps)
    tags = [(256, 4, [w]), (257, 4, [h]), (258, 3, [32]), (259, 3, [compression]), (262, 3, [1]), (273, 4, None),
            (277, 3, [1]), (278, 4, [rps]), (279, 4, [len(d) for d in strips])]
    if predictor is not None:
        tags.append((317, 3, [predictor]))
    tags.append((339, 3, [3]))
    ifd_off = 8
    extra_off = ifd_off + 2 + 12 * len(tags) + 4
    extra = b""
    strip0 = extra_off + (8 * n if n > 1 else 0)
    offs, o = [], strip0
    for d in strips:
        offs.append(o)
        o += len(d)
    ifd = struct.pack(endian + "H", len(tags))
    for tag, typ, vals in tags:
        vals = offs if vals is None else vals
        raw = struct.pack(endian + {3: "H", 4: "I"}[typ] * len(vals), *vals)
        if len(raw) <= 4:
            field = raw + b"\0" * (4 - len(raw))
        else:
            field = struct.pack(endian + "I", extra_off + len(extra))
            extra += raw
        ifd += struct.pack(endian + "HHI", tag, typ, len(vals)) + field
    ifd += struct.pack(endian + "I", 0)
    assert len(extra) == strip0 - extra_off
    head = (b"II" if endian == "<" else b"MM") + struct.pack(endian + "HI", 42, ifd_off)
    return head + ifd + extra + b"".join(strips)


def tiff_lzw_bytes(m, endian="<", rows_per_strip=None, predictor=1, write_tag=True, **enc):
    """the map m as an LZW strip TIFF written by lzw_encode(**enc) behind the forward predictor"""
    h, w = m.shape
    rps = rows_per_strip or h
    rb = row_bytes(m, endian, predictor)
    strips = [lzw_encode(rb[r:r + rps].tobytes(), **enc) for r in range(0, h, rps)]
    return tiff_file(h, w, strips, endian, rps, 5, predictor if (write_tag or predictor != 1) else None)


def half_random_map(h=40, w=300, seed=5):
    """upper half random bits (finite floats), lower half constant: as one strip it reaches all four code widths and
    several table resets"""
    rng = np.random.default_rng(seed)
    m = np.full((h, w), 0.25, dtype=np.float32)
    m[:h // 2] = rng.standard_normal((h // 2, w)).astype(np.float32) * 3.0
    return m


def smooth_map(h, w, seed=0):
    """a smooth field with noise: what an uncertainty map looks like to a predictor"""
    rng = np.random.default_rng(seed + 31 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    m = 0.5 + 0.4 * np.sin(0.07 * xx + 0.11 * yy) + 0.01 * rng.standard_normal((h, w))
    m[h // 2:, : w // 3] = 0.0
    return m.astype(np.float32)


def golden_files():
    """[(tif path, npy path)] of tests/golden/tiff_lzw (written by libtiff through PIL: tools/gen_tiff_lzw_golden.py)"""
    names = sorted(f[:-4] for f in os.listdir(GOLDEN_LZW) if f.endswith(".tif"))
    return [(os.path.join(GOLDEN_LZW, n + ".tif"), os.path.join(GOLDEN_LZW, n + ".npy")) for n in names]


def build_host_decoder(dst_dir, sanitize=True):
    exe = os.path.join(dst_dir, "lzw_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "lzw_host.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd)
    return exe


def run_host_decoder(exe, items, work_dir):
    """items: [(bytes, capacity)] -> [(status, bytes)]"""
    src = os.path.join(work_dir, "in.bin")
    dst = os.path.join(work_dir, "out.bin")
    with open(src, "wb") as f:
        for data, cap in items:
            f.write(struct.pack("<qq", cap, len(data)) + data)
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    res, o = [], 0
    for _ in items:
        st, _pad, n = struct.unpack_from("<iiq", raw, o)
        o += 16
        res.append((st, raw[o:o + n]))
        o += n
    assert o == len(raw)
    return res


def stream_corpus():
    """name -> (LZW strip, the bytes it decodes to, window size): every option of the encoder over payloads that reach
    widths 9 to 12, a full table, several ClearCodes and the longest strings"""
    rng = np.random.default_rng(11)
    rnd = rng.integers(0, 256, 48000, dtype=np.uint8).tobytes()
    walk = np.cumsum(rng.integers(-2, 3, 30000)).astype(np.int16).tobytes()
    text = b"the quick brown fox jumps over the lazy dog; " * 300
    const = bytes([7]) * 200000
    out = {}
    for name, d in (("empty", b""), ("b1", b"A"), ("b3", b"ABA"), ("b4", b"AAAA"), ("random", rnd), ("walk", walk),
                    ("text", text), ("const", const)):
        out[name] = (lzw_encode(d), d, len(d))
        out[name + "_noeoi"] = (lzw_encode(d, eoi=False), d, len(d))
    for name, d in (("random", rnd), ("walk", walk), ("const", const)):
        out[name + "_defer"] = (lzw_encode(d, defer=300), d, len(d))
        out[name + "_midclear"] = (lzw_encode(d, mid_clear=len(d) // 3), d, len(d))
        out[name + "_early"] = (lzw_encode(d, early_eoi=len(d) // 2), d[:len(d) // 2], len(d))
        out[name + "_cut"] = (lzw_encode(d), d[:len(d) // 2 + 1], len(d) // 2 + 1)   # the window ends inside a string
    return out
