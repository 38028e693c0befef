"""CPU: LZW-compressed float32 TIFF maps (Compression 5, Predictor 1 / 2 / 3) through the host reader
(image_io.read_tiff_f32) against libtiff (through PIL) and the source arrays; the test encoder (tests/lzw_build.py)
validated against libtiff; the serial decoder core (values_amd/csrc/lzw_core.h) as a stand-alone program under the
sanitizers."""
import os

import numpy as np
import pytest

from tests import lzw_build as lb
from tests import png_build as pb


def _same(a, b):
    return a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _pil():
    PIL = pytest.importorskip("PIL")
    from PIL import Image, features
    if not features.check("libtiff"):
        pytest.skip("PIL without libtiff")
    return Image


def _pil_read(Image, path, endian="<"):
    """PIL's array of a float32 TIFF.  For a big-endian COMPRESSED file libtiff hands PIL native floats and PIL swaps them
    once more (it does the same to a big-endian Deflate file): the swap is undone here, so the check still pins what
    libtiff decoded."""
    a = np.array(Image.open(path))
    assert a.dtype == np.float32
    return a.byteswap() if endian == ">" else a


def test_golden_files_read_as_libtiff_wrote_them():
    from values_amd.image_io import read_tiff_f32, tiff_parse
    files = lb.golden_files()
    assert len(files) >= 9
    seen = set()
    for tif, npy in files:
        want = np.load(npy)
        buf = open(tif, "rb").read()
        t = tiff_parse(buf, tif)
        assert t.lzw and not t.deflate and t.endian == "<"
        seen.add((t.predictor, len(t.strips) == 1, len(t.strips) == t.h))
        assert _same(read_tiff_f32(tif), want), tif
    assert {p for p, _, _ in seen} == {1, 2, 3}
    assert any(one for _, one, _ in seen) and any(per_row for _, _, per_row in seen)
    assert sum(os.path.getsize(p) for pair in files for p in pair) < 200_000


def test_golden_files_decode_the_same_through_pil():
    Image = _pil()
    for tif, npy in lb.golden_files():
        assert _same(_pil_read(Image, tif), np.load(npy)), tif


@pytest.mark.parametrize("shape", [(1, 1), (6, 5), (21, 13), (40, 300)])
def test_pil_written_grid(tmp_path, shape):
    """libtiff's writer, every predictor and strip height: read_tiff_f32 == PIL's decode == the source"""
    Image = _pil()
    from values_amd.image_io import read_tiff_f32, tiff_parse
    m = lb.half_random_map(*shape) if shape == (40, 300) else lb.smooth_map(*shape)
    p = str(tmp_path / "m.tif")
    for pred in (1, 2, 3):
        for rps in (None, 1, 7):
            info = {317: pred}
            if rps is not None:
                info[278] = rps
            Image.fromarray(m).save(p, compression="tiff_lzw", tiffinfo=info)
            t = tiff_parse(open(p, "rb").read())
            assert t.lzw and t.predictor == pred
            if rps is not None:
                assert len(t.strips) == -(-shape[0] // rps)
            assert _same(_pil_read(Image, p), m), (pred, rps)
            assert _same(read_tiff_f32(p), m), (pred, rps)


ENCODINGS = [{}, {"defer": 300}, {"eoi": False}, {"mid_clear": 5000}, {"defer": 1, "eoi": False}]


def test_the_test_encoder_is_read_by_libtiff_and_by_the_host_reader(tmp_path):
    """every variant of lzw_build's encoder -- ClearCode deferred past a full table, no EndOfInformation, a ClearCode in
    the middle -- decodes through libtiff to its source (this validates the encoder), and through read_tiff_f32, in both
    byte orders"""
    Image = _pil()
    from values_amd.image_io import read_tiff_f32
    p = str(tmp_path / "m.tif")
    for m, rps_list in ((lb.half_random_map(), (None, 7)), (lb.smooth_map(6, 5), (None, 1)), (lb.smooth_map(1, 1), (None,))):
        for endian in "<>":
            for pred in (1, 2, 3):
                for rps in rps_list:
                    for enc in ENCODINGS:
                        open(p, "wb").write(lb.tiff_lzw_bytes(m, endian, rps, pred, **enc))
                        assert _same(_pil_read(Image, p, endian), m), (endian, pred, rps, enc)
                        assert _same(read_tiff_f32(p), m), (endian, pred, rps, enc)
    # no Predictor tag at all is predictor 1
    open(p, "wb").write(lb.tiff_lzw_bytes(lb.smooth_map(6, 5), "<", 2, 1, write_tag=False))
    assert _same(read_tiff_f32(p), lb.smooth_map(6, 5))


def test_the_encoder_of_a_constant_run_is_the_general_encoder():
    for n in (1, 2, 5, 4000, 100000):
        for kw in ({}, {"defer": 50}, {"eoi": False}):
            assert lb.lzw_encode_run(7, n, **kw) == lb.lzw_encode(bytes([7]) * n, **kw), (n, kw)


def test_host_reader_reports_the_strip_and_what_went_wrong(tmp_path):
    from values_amd.image_io import read_tiff_f32
    m = lb.smooth_map(6, 5)
    rb = lb.row_bytes(m)
    good = [lb.lzw_encode(rb[r:r + 2].tobytes()) for r in range(0, 6, 2)]
    p = tmp_path / "m.tif"
    for bad, what in ((good[1][:10], "ends before"), (b"\x80\x1f\xff\xff\xff", "above the next free entry"),
                      (rb[2:4].tobytes(), "not ClearCode"), (b"", "ends before"),
                      (lb.lzw_encode(rb[2:4].tobytes(), early_eoi=7), "holds 7 bytes, 40 expected")):
        p.write_bytes(lb.tiff_file(6, 5, [good[0], bad, good[2]], "<", 2, 5, 1))
        with pytest.raises(ValueError, match=r"Compression \(tag 259\) = 5 \(LZW\): strip at row 2: .*" + what):
            read_tiff_f32(p)
    p.write_bytes(lb.tiff_file(6, 5, good, "<", 2, 5, 4))
    with pytest.raises(ValueError, match=r"Predictor \(tag 317\) = 4"):
        read_tiff_f32(p)


def test_predictors_without_lzw_stay_refused(tmp_path):
    """Deflate or uncompressed strips with a predictor: no writer in scope produces them"""
    from values_amd.image_io import read_tiff_f32
    m = lb.smooth_map(6, 5)
    p = tmp_path / "m.tif"
    for comp in (1, 8):
        for pred, what in ((2, r"Predictor \(tag 317\) = 2: only 1 \(none\)"),
                           (3, r"Predictor \(tag 317\) = 3 \(floating point\): only 1 \(none\)")):
            p.write_bytes(pb.tiff_bytes(m, "<", 2, comp, predictor=pred))
            with pytest.raises(ValueError, match=what):
                read_tiff_f32(p)
        p.write_bytes(pb.tiff_bytes(m, "<", 2, comp, predictor=1))
        assert _same(read_tiff_f32(p), m)


# ---------------------------------------------------------------------------------------------------------------------
# the decoder core as its own program (never loaded into Python)

@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lzw_host"))
    try:
        return lb.build_host_decoder(d, sanitize=True), d
    except Exception:
        return lb.build_host_decoder(d, sanitize=False), d      # a compiler without the sanitizers' runtimes


def test_core_decodes_the_corpus_bit_exactly(host_decoder):
    exe, d = host_decoder
    corpus = lb.stream_corpus()
    names = sorted(corpus)
    res = lb.run_host_decoder(exe, [(corpus[n][0], corpus[n][2]) for n in names], d)
    for n, (st, out) in zip(names, res):
        assert st == lb.OK and out == corpus[n][1], n
    # the golden files' strips, as libtiff's encoder wrote them
    from values_amd.image_io import tiff_parse
    items, want = [], []
    for tif, npy in lb.golden_files():
        buf = open(tif, "rb").read()
        t = tiff_parse(buf)
        if t.predictor != 1:
            continue
        m = np.load(npy)
        for r0, rows, o, c in t.strips:
            items.append((buf[o:o + c], 4 * rows * t.w))
            want.append(m[r0:r0 + rows].tobytes())
    assert len(items) > 20
    for (st, out), w in zip(lb.run_host_decoder(exe, items, d), want):
        assert st == lb.OK and out == w


def test_core_statuses(host_decoder):
    exe, d = host_decoder
    data = np.random.default_rng(3).integers(0, 256, 3000, dtype=np.uint8).tobytes()
    good = lb.lzw_encode(data)
    bits = lb._Bits()
    for code in (256, 65, 66, 300):          # 300 with the next free entry at 259
        bits.put(code, 9)
    above = bits.done() + b"\0" * 8
    bits = lb._Bits()
    for code in (256, 258):                  # the first free entry right after ClearCode: no string before it
        bits.put(code, 9)
    first = bits.done() + b"\0" * 8
    items = [(good[:len(good) // 2], len(data)), (above, 100), (first, 100), (data, len(data)), (good[1:], len(data)),
             (b"", 10), (b"", 0), (good, len(data)), (lb.lzw_encode(data, eoi=False), len(data) + 1), (b"\x80", 10)]
    res = lb.run_host_decoder(exe, items, d)
    assert [st for st, _ in res] == [lb.TRUNCATED, lb.BAD_CODE, lb.BAD_CODE, lb.BAD_CODE, lb.BAD_CODE, lb.TRUNCATED, lb.OK,
                                     lb.OK, lb.TRUNCATED, lb.TRUNCATED]
    assert data.startswith(res[0][1]) and len(res[0][1]) > 1000       # what came before the end of the input
    assert res[1][1] == b"AB" and res[2][1] == b"" and res[7][1] == data and res[8][1] == data


def test_core_survives_mutations(host_decoder):
    """a few hundred seeded single-byte mutations of valid streams: each returns a status, its size stays within the
    window (the program checks both, under the sanitizers), and an OK with a full window of the right length is possible
    only where the window was reached"""
    exe, d = host_decoder
    rng = np.random.default_rng(17)
    corpus = lb.stream_corpus()
    items = []
    for name in ("random", "walk_defer", "text", "const_midclear", "random_noeoi", "b4"):
        src, data, cap = corpus[name]
        for _ in range(60):
            a = bytearray(src)
            a[int(rng.integers(0, len(a)))] = int(rng.integers(0, 256))
            items.append((bytes(a), cap))
            if rng.random() < 0.3:
                items.append((bytes(a[:int(rng.integers(0, len(a)))]), cap))
    assert len(items) >= 360
    res = lb.run_host_decoder(exe, items, d)
    assert len(res) == len(items)
    for (src, cap), (st, out) in zip(items, res):
        assert st in (lb.OK, lb.TRUNCATED, lb.BAD_CODE) and len(out) <= cap
    assert {st for st, _ in res} == {lb.OK, lb.TRUNCATED, lb.BAD_CODE}
