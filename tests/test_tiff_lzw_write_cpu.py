"""CPU: the host writer of LZW-compressed float32 TIFF maps -- image_io.lzw_encode against the test encoder
(tests/lzw_build.lzw_encode, validated against libtiff in test_tiff_lzw_cpu.py), its bound, write_tiff_f32(compression=
"lzw") read back by this project's reader and by PIL (libtiff) and checked field by field against the layout the device
writer shares, the unchanged default file, and the encoder's serial core (values_amd/csrc/lzw_enc_core.h) built as a
stand-alone program under the address and undefined-behaviour sanitizers (tests/lzw_enc_host.cpp)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import lzw_build as lb
from tests.helpers import build_host_program

ROOT = lb.ROOT
NO_ROOM = 3


@pytest.fixture(scope="module")
def corpus():
    """name -> payload: empty, 1, 3 and 4 bytes, 48 000 random bytes (all four widths, a dozen resets), a random walk,
    text, 200 000 constant bytes (the longest strings) -- with the strip the test encoder makes of each"""
    out = {}
    for name, (strip, data, _) in lb.stream_corpus().items():
        if "_" not in name:
            out[name] = (data, strip)
    assert sorted(out) == ["b1", "b3", "b4", "const", "empty", "random", "text", "walk"]
    return out


def test_lzw_encode_equals_the_test_encoder_and_keeps_its_bound(corpus):
    from values_amd.image_io import lzw_bound, lzw_decode, lzw_encode
    for name, (data, strip) in corpus.items():
        got = lzw_encode(data)
        assert got == strip, (name, len(got), len(strip))
        assert len(got) <= lzw_bound(len(data)), name
        assert lzw_decode(got, len(data)) == (data, None), name
    assert lzw_encode(b"") == bytes([0x80, 0x40, 0x40])                   # ClearCode + EndOfInformation
    rng = np.random.default_rng(3)
    for n in (1, 2, 100, 8192):
        for d in (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), bytes(n)):
            assert len(lzw_encode(d)) <= lzw_bound(n), n
    assert [lzw_bound(n) for n in (0, 1, 3835, 3836, 8192)] == [3, 5, 5756, 5759, 12294]


def _special_map(h, w, seed):
    """random finite floats with -0.0, both infinities, a NaN with payload and denormals among them"""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((h, w)).astype(np.float32)
    flat = m.reshape(-1).view(np.uint32)
    special = [0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFA00001, 0x00000001, 0x807FFFFF, 0x00400000]
    for k, v in enumerate(special):
        flat[(k * 7) % flat.size] = v
    return m


def _maps():
    return [("1x1", _special_map(1, 1, 0)), ("7x700", _special_map(7, 700, 1)), ("9x37", _special_map(9, 37, 2)),
            ("half_random", lb.half_random_map())]


def _ifd(buf):
    """-> (ifd offset, [(tag, type, count, value field bytes)], the offset behind the IFD)"""
    assert buf[:4] == b"II*\0"
    off = struct.unpack("<I", buf[4:8])[0]
    n = struct.unpack("<H", buf[off:off + 2])[0]
    ents = [struct.unpack("<HHI4s", buf[off + 2 + 12 * i:off + 14 + 12 * i]) for i in range(n)]
    assert buf[off + 2 + 12 * n:off + 6 + 12 * n] == b"\0\0\0\0"          # no further IFD
    return off, ents, off + 6 + 12 * n


@pytest.mark.parametrize("predictor", (1, 2, 3))
def test_written_files_read_back_and_have_the_fixed_layout(tmp_path, predictor):
    from values_amd.image_io import read_tiff_f32, tiff_parse, write_tiff_f32
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for name, m in _maps():
        h, w = m.shape
        default = min(h, max(1, 8192 // (4 * w)))
        if name == "7x700":
            assert default == 2
        for rps_arg in (None, 1, h):
            rps = default if rps_arg is None else rps_arg
            p = str(tmp_path / f"{name}_{predictor}_{rps_arg}.tif")
            write_tiff_f32(p, m, compression="lzw", predictor=predictor, rows_per_strip=rps_arg)
            buf = open(p, "rb").read()
            # both readers, bit for bit
            assert np.array_equal(read_tiff_f32(p).view(np.uint32), m.view(np.uint32)), (name, rps_arg)
            if Image is not None:
                with Image.open(p) as im:
                    got = np.asarray(im)
                assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), m.view(np.uint32)), (name, rps_arg)
            # the layout: header, strips back to back from offset 8 in row order, an even IFD offset, ascending tags, the
            # strip arrays behind the IFD (inline with one strip)
            rb = lb.row_bytes(m, "<", predictor)
            strips = [lb.lzw_encode(rb[r:r + rps].tobytes()) for r in range(0, h, rps)]
            n = len(strips)
            if name == "7x700" and rps_arg is None:
                assert n == 4 and len(rb[6:8]) == 1                      # a short last strip
            body = b"".join(strips)
            assert buf[8:8 + len(body)] == body
            off, ents, behind = _ifd(buf)
            assert off % 2 == 0 and off == 8 + len(body) + len(body) % 2 and buf[8 + len(body):off] == bytes(len(body) % 2)
            assert [e[0] for e in ents] == [256, 257, 258, 259, 262, 273, 277, 278, 279, 284, 317, 339]
            offs = [8 + sum(len(s) for s in strips[:k]) for k in range(n)]
            long_, short = lambda v: struct.pack("<I", v), lambda v: struct.pack("<HH", v, 0)
            want = {256: (4, 1, long_(w)), 257: (4, 1, long_(h)), 258: (3, 1, short(32)), 259: (3, 1, short(5)),
                    262: (3, 1, short(1)), 277: (3, 1, short(1)), 278: (4, 1, long_(rps)), 284: (3, 1, short(1)),
                    317: (3, 1, short(predictor)), 339: (3, 1, short(3)),
                    273: (4, n, long_(offs[0] if n == 1 else behind)),
                    279: (4, n, long_(len(strips[0]) if n == 1 else behind + 4 * n))}
            for tag, typ, cnt, field in ents:
                assert (typ, cnt, field) == want[tag], (name, rps_arg, tag)
            if n > 1:
                assert buf[behind:] == struct.pack(f"<{n}I", *offs) + struct.pack(f"<{n}I", *[len(s) for s in strips])
            else:
                assert len(buf) == behind
            t = tiff_parse(buf)
            assert t.lzw and not t.deflate and t.predictor == predictor and (t.w, t.h, t.endian) == (w, h, "<")
            assert t.strips == [(k * rps, min(rps, h - k * rps), offs[k], len(strips[k])) for k in range(n)]


def test_default_file_and_refused_arguments(tmp_path):
    from values_amd.image_io import tiff_f32_parts, tiff_parse, write_tiff_f32
    from values_amd.results2d import save_uncertainty
    m = _special_map(9, 37, 4)
    head, tail = tiff_f32_parts(9, 37)
    p = str(tmp_path / "plain.tif")
    write_tiff_f32(p, m)
    assert open(p, "rb").read() == head + m.tobytes() + tail
    write_tiff_f32(p, m, compression=None, predictor=2, rows_per_strip=1)   # not looked at without compression
    assert open(p, "rb").read() == head + m.tobytes() + tail
    for kw in ({"compression": "deflate"}, {"compression": "LZW"}, {"compression": 5}, {"compression": "lzw", "predictor": 4},
               {"compression": "lzw", "predictor": 0}, {"compression": "lzw", "rows_per_strip": 0}):
        with pytest.raises(ValueError):
            write_tiff_f32(str(tmp_path / "bad.tif"), m, **kw)
    # save_uncertainty passes the keywords through; without them the file is the default one
    save_uncertainty(str(tmp_path / "a"), "img", {"u": m})
    assert open(tmp_path / "a" / "u" / "img.tif", "rb").read() == head + m.tobytes() + tail
    save_uncertainty(str(tmp_path / "b"), "img", {"u": m}, compression="lzw", predictor=2, rows_per_strip=4)
    write_tiff_f32(p, m, "lzw", 2, 4)
    got = open(tmp_path / "b" / "u" / "img.tif", "rb").read()
    assert got == open(p, "rb").read()
    t = tiff_parse(got)
    assert t.lzw and t.predictor == 2 and [s[:2] for s in t.strips] == [(0, 4), (4, 4), (8, 1)]


def test_the_serial_core_as_a_sanitized_program(tmp_path, corpus):
    """tests/lzw_enc_host.cpp (its own main, values_amd/csrc/lzw_enc_core.h) built with the address and undefined-
    behaviour sanitizers and run as a program: every payload with a window of exactly the strip, a larger one, one byte
    too small (VX_LZW_NO_ROOM, the strip's first bytes, nothing more) and an empty one"""
    exe = str(tmp_path / "lzw_enc_host")
    build_host_program(os.path.join(ROOT, "tests", "lzw_enc_host.cpp"), exe, extra=("-Werror", "-I", os.path.join(ROOT, "include")))
    items = []
    for name, (data, strip) in corpus.items():
        items += [(name, data, len(strip), 0, strip), (name, data, len(strip) + 7, 0, strip),
                  (name, data, len(strip) - 1, NO_ROOM, strip[:-1]), (name, data, 0, NO_ROOM, b"")]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        for _, data, cap, _, _ in items:
            f.write(struct.pack("<qq", cap, len(data)) + data)
    subprocess.check_call([exe, src, dst])                                # a sanitizer report ends it with a status
    raw, o = open(dst, "rb").read(), 0
    for name, data, cap, st, want in items:
        got_st, _, n = struct.unpack_from("<iiq", raw, o)
        o += 16
        assert (got_st, raw[o:o + n]) == (st, want), (name, cap)
        o += n
    assert o == len(raw)
