"""The DEFLATE / gzip / zlib corpus of the decoder tests (generated with zlib at run time) and the host reference decoder
built from values_amd/csrc/inflate_core.h (tests/inflate_host.cpp)."""
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GZIP, ZLIB, RAW = 0, 1, 2
(OK, TRUNCATED, BAD_HEADER, BAD_BLOCK, BAD_LENGTHS, BAD_SYMBOL, BAD_DISTANCE, CAPACITY, BAD_CHECK, BAD_ISIZE, TRAILING,
 BAD_STORED, DICT) = range(13)


def _deflate(data, fmt, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    wbits = {GZIP: 31, ZLIB: 15, RAW: -15}[fmt]
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(data) + c.flush()


def _gzip_member(data, flags=0, name=b"", extra=b"", comment=b"", level=6):
    """an RFC 1952 member with the given header fields (FHCRC: the low 16 bits of the header's CRC-32)"""
    h = bytearray(b"\x1f\x8b\x08" + bytes([flags]) + b"\x00\x00\x00\x00\x00\xff")
    if flags & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        h += name + b"\0"
    if flags & 16:
        h += comment + b"\0"
    if flags & 2:
        h += struct.pack("<H", zlib.crc32(bytes(h)) & 0xFFFF)
    return bytes(h) + _deflate(data, RAW, level) + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def payloads():
    rng = np.random.default_rng(7)
    text = (b"the quick brown fox jumps over the lazy dog; " * 400)
    walk = np.cumsum(rng.integers(-2, 3, 200000)).astype(np.int16).tobytes()
    far = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    return {
        "empty": b"",
        "one": b"A",
        "text": text,
        "walk": walk,
        "zeros": bytes(300000),                                   # distance-1 matches, 258-byte matches
        "far": far + far[:5000] + far,                            # distance-32768 matches
        "random": rng.integers(0, 256, 200000, dtype=np.uint8).tobytes(),   # > 64 KiB incompressible: stored blocks
        "f64": np.sin(np.arange(40000) * 0.01).tobytes(),
    }


def good_corpus():
    """name -> (format, compressed bytes, decoded bytes)"""
    p = payloads()
    out = {}
    for k in ("empty", "one", "text", "walk"):
        for lvl in (0, 1, 6, 9):
            out[f"{k}_l{lvl}"] = (GZIP, _deflate(p[k], GZIP, lvl), p[k])
    for strat, sname in ((zlib.Z_FIXED, "fixed"), (zlib.Z_HUFFMAN_ONLY, "huff"), (zlib.Z_RLE, "rle")):
        out[f"walk_{sname}"] = (GZIP, _deflate(p["walk"], GZIP, 6, strat), p["walk"])
        out[f"text_{sname}"] = (RAW, _deflate(p["text"], RAW, 6, strat), p["text"])
    out["zeros_l9"] = (GZIP, _deflate(p["zeros"], GZIP, 9), p["zeros"])
    out["far_l6"] = (GZIP, _deflate(p["far"], GZIP, 6), p["far"])
    out["random_l6"] = (GZIP, _deflate(p["random"], GZIP, 6), p["random"])
    out["random_l0_zlib"] = (ZLIB, _deflate(p["random"], ZLIB, 0), p["random"])
    out["f64_l1"] = (GZIP, gzip.compress(p["f64"], compresslevel=1), p["f64"])
    out["text_zlib"] = (ZLIB, _deflate(p["text"], ZLIB, 6), p["text"])
    out["walk_zlib_l1"] = (ZLIB, _deflate(p["walk"], ZLIB, 1), p["walk"])
    out["walk_raw_l9"] = (RAW, _deflate(p["walk"], RAW, 9), p["walk"])
    out["empty_raw"] = (RAW, _deflate(b"", RAW), b"")
    out["empty_zlib"] = (ZLIB, _deflate(b"", ZLIB), b"")
    mm = [p["text"][:1000], b"", p["walk"][:70000], p["one"]]
    out["multi_member"] = (GZIP, b"".join(gzip.compress(m) for m in mm), b"".join(mm))
    out["multi_member_padded"] = (GZIP, gzip.compress(p["text"]) + b"\0\0\0" + gzip.compress(b"xyz") + b"\0", p["text"] + b"xyz")
    out["hdr_fname"] = (GZIP, _gzip_member(p["text"], 8, name=b"case0.nii"), p["text"])
    out["hdr_all"] = (GZIP, _gzip_member(p["walk"], 1 | 2 | 4 | 8 | 16, name=b"n" * 300, extra=b"\x01\x02" * 40,
                                         comment=b"c" * 5000), p["walk"])
    out["hdr_fhcrc"] = (GZIP, _gzip_member(b"abc", 2), b"abc")
    return out


def _flip(b, bit):
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def _raw_block(bits):
    """bytes of an LSB-first bit string '0101...'"""
    bits = bits + "0" * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8][::-1], 2) for i in range(0, len(bits), 8))


def corrupt_corpus():
    """name -> (format, bytes, capacity or None, expected status or None).  None: the expected status is whatever the
    host reference decoder reports, but not OK unless the output equals the original (bit flips in MTIME, say)."""
    p = payloads()
    short = gzip.compress(b"hello hello hello, world")
    out = {}
    for i in range(len(short)):
        out[f"trunc_gz_{i}"] = (GZIP, short[:i], None, TRUNCATED)
    zs = _deflate(b"hello hello hello, world", ZLIB)
    for i in range(len(zs)):
        out[f"trunc_zlib_{i}"] = (ZLIB, zs[:i], None, TRUNCATED)
    rs = _deflate(p["text"][:3000], RAW)
    for i in range(0, len(rs), 7):
        out[f"trunc_raw_{i}"] = (RAW, rs[:i], None, TRUNCATED)
    flipsrc = _deflate(p["text"][:2000], GZIP, 9)
    for bit in range(0, len(flipsrc) * 8, 5):
        out[f"flip_{bit}"] = (GZIP, _flip(flipsrc, bit), None, None)
    # BTYPE 3: final bit 1, type 11
    out["btype3"] = (RAW, _raw_block("111") + b"\0" * 8, None, BAD_BLOCK)
    # dynamic header with HLIT = 287 (30 + 257): 1, 01 (dynamic), HLIT 11110
    out["hlit_287"] = (RAW, _raw_block("1" + "01" + "01111" + "00000" + "0000") + b"\0" * 40, None, BAD_LENGTHS)
    # over-subscribed code-length code: 19 lengths of 1
    out["oversub"] = (RAW, _raw_block("1" + "01" + "00000" + "00000" + "1111" + "100" * 19) + b"\0" * 40, None, BAD_LENGTHS)
    # fixed block: literal 'a' then a match at distance 2 with one byte of output
    lit_a = format(0x30 + ord("a"), "08b")    # fixed codes are written MSB first
    out["dist_far"] = (RAW, _raw_block("1" + "10" + lit_a + "0000001" + "00001") + b"\0\0", None, BAD_DISTANCE)
    # stored block whose NLEN is not ~LEN
    out["bad_nlen"] = (RAW, b"\x01\x05\x00\x00\x00hello", None, BAD_STORED)
    good = gzip.compress(p["text"])
    crc = bytearray(good)
    crc[-8] ^= 1
    out["bad_crc"] = (GZIP, bytes(crc), None, BAD_CHECK)
    isz = bytearray(good)
    isz[-4] ^= 1
    out["bad_isize"] = (GZIP, bytes(isz), None, BAD_ISIZE)
    ad = bytearray(_deflate(p["text"], ZLIB))
    ad[-1] ^= 0x80
    out["bad_adler"] = (ZLIB, bytes(ad), None, BAD_CHECK)
    out["small_capacity"] = (GZIP, good, 1000, CAPACITY)
    out["trailing_gz"] = (GZIP, good + b"garbage", None, TRAILING)
    out["trailing_zlib"] = (ZLIB, _deflate(p["text"], ZLIB) + b"\0", None, TRAILING)
    out["trailing_raw"] = (RAW, _deflate(p["text"], RAW) + b"x", None, TRAILING)
    out["bad_magic"] = (GZIP, b"\x1f\x8c" + good[2:], None, BAD_HEADER)
    out["bad_zlib_hdr"] = (ZLIB, b"\x78\x02" + _deflate(p["text"], RAW), None, BAD_HEADER)
    out["zlib_dict"] = (ZLIB, b"\x78\xbb" + b"\0" * 20, None, DICT)
    out["bad_symbol_fixed"] = (RAW, _raw_block("1" + "10" + "11000110") + b"\0\0", None, BAD_SYMBOL)   # lit/len code 286
    return out


def build_host_decoder(dst_dir, sanitize=True):
    exe = os.path.join(dst_dir, "inflate_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "inflate_host.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd)
    return exe


def run_host_decoder(exe, items, work_dir):
    """items: [(format, bytes, capacity)] -> [(status, bytes)]"""
    src = os.path.join(work_dir, "in.bin")
    dst = os.path.join(work_dir, "out.bin")
    with open(src, "wb") as f:
        for fmt, data, cap in items:
            f.write(struct.pack("<iiqq", fmt, 0, cap, len(data)) + data)
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


def capacity_for(data_len):
    return data_len + 64
