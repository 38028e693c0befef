"""CPU: the host side of reading the results tree on the device -- the ctypes mirrors of vx_inflate_item /
vx_nifti_dec_item, argument refusals before any HIP call, nifti.parse_header against nifti.load, and the host reference
decoder built from values_amd/csrc/inflate_core.h against zlib on a generated corpus and a corrupt set."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import inflate_corpus as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(1 << 20)   # never dereferenced: every call below is refused before it touches the device


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from values_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_struct_sizes_match_c(lib):
    from values_amd import _lib
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "values_amd.h"
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(vx_inflate_item), offsetof(vx_inflate_item, dst_cap),
 offsetof(vx_inflate_item, format), sizeof(vx_nifti_dec_item), offsetof(vx_nifti_dec_item, dims),
 offsetof(vx_nifti_dec_item, out_dtype), offsetof(vx_nifti_dec_item, inter)); return 0;}
'''
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write(code)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(_lib.InflateItem), _lib.InflateItem.dst_cap.offset, _lib.InflateItem.format.offset,
                     ctypes.sizeof(_lib.NiftiDecItem), _lib.NiftiDecItem.dims.offset, _lib.NiftiDecItem.out_dtype.offset,
                     _lib.NiftiDecItem.inter.offset]


def test_inflate_refusals(lib):
    from values_amd import _lib
    it = (_lib.InflateItem * 2)()
    for i in range(2):
        it[i].src, it[i].src_n, it[i].dst_off, it[i].dst_cap = FAKE, 100, 1000 * i, 1000
    ws = lib.vx_inflate_workspace_bytes(2)
    assert ws > 0 and lib.vx_inflate_workspace_bytes(-1) < 0
    big = 1 << 30
    call = lambda items=it, n=2, dst=FAKE, dst_n=big, sz=FAKE, st=FAKE, w=FAKE, wb=ws: lib.vx_inflate(
        items, n, dst, dst_n, sz, st, w, wb, None)
    assert call(items=None) == -1
    assert call(dst=None) == -1
    assert call(sz=None) == -1
    assert call(st=None) == -1
    assert call(w=None) == -1
    assert call(n=-1) == -2
    assert call(n=0) == 0
    assert call(wb=ws - 1) == -4
    assert call(dst_n=1500) == -2                    # the second window ends beyond dst
    it[1].dst_off = 500
    assert call() == -2                              # overlapping windows
    it[1].dst_off = -5
    assert call() == -2
    it[1].dst_off, it[1].dst_cap = 2**63 - 51, 100
    assert call() == -2                              # dst_off + dst_cap overflows int64: still a window beyond dst
    it[1].dst_off, it[1].dst_cap = 1000, 1000
    it[0].src_n = -1
    assert call() == -2
    it[0].src_n = 100
    it[0].dst_cap = -1
    assert call() == -2
    it[0].dst_cap = 1000
    it[0].format = 3
    assert call() == -3
    it[0].format = 0
    it[0].src = None
    assert call() == -1


def test_nifti_decode_refusals(lib):
    from values_amd import _lib
    it = (_lib.NiftiDecItem * 1)()
    it[0].src, it[0].src_n, it[0].vox_offset, it[0].dst, it[0].dst_n = FAKE, 352 + 64 * 4, 352, FAKE, 64 * 4
    it[0].ndim, it[0].code, it[0].out_dtype = 3, 16, -1
    for k in range(3):
        it[0].dims[k] = 4
    ws = lib.vx_nifti_decode_workspace_bytes(1)
    assert ws > 0
    assert lib.vx_nifti_decode(None, 1, FAKE, ws, None) == -1
    assert lib.vx_nifti_decode(it, 1, None, ws, None) == -1
    assert lib.vx_nifti_decode(it, -1, FAKE, ws, None) == -2
    assert lib.vx_nifti_decode(it, 0, FAKE, ws, None) == 0
    assert lib.vx_nifti_decode(it, 1, FAKE, ws - 1, None) == -4
    it[0].src_n = 352 + 63 * 4
    assert lib.vx_nifti_decode(it, 1, FAKE, ws, None) == -2          # voxels beyond the payload
    it[0].src_n = 352 + 64 * 4
    it[0].dst_n = 10
    assert lib.vx_nifti_decode(it, 1, FAKE, ws, None) == -2          # output beyond dst
    it[0].dst_n = 64 * 4
    it[0].code = 3
    assert lib.vx_nifti_decode(it, 1, FAKE, ws, None) == -3
    it[0].code = 16
    it[0].ndim = 8
    assert lib.vx_nifti_decode(it, 1, FAKE, ws, None) == -2
    it[0].ndim = 3
    it[0].dims[1] = -1
    assert lib.vx_nifti_decode(it, 1, FAKE, ws, None) == -2
    it[0].dims[1] = 4
    it[0].out_dtype = 5
    assert lib.vx_nifti_decode(it, 1, FAKE, ws, None) == -3
    it[0].out_dtype = -1
    it[0].src = None
    assert lib.vx_nifti_decode(it, 1, FAKE, ws, None) == -1


def _same_header(a, b):
    assert a["pixdim"] == b["pixdim"]
    assert a["datatype"] == b["datatype"]
    np.testing.assert_array_equal(a["affine"], b["affine"])


def test_parse_header_equals_load(tmp_path):
    import gzip
    import struct
    from values_amd import nifti
    hdr = {"pixdim": [0.7, 0.8, 2.5], "affine": np.diag([0.7, -0.8, 2.5, 1.0])}
    for dt in nifti._DT:
        a = (np.arange(2 * 3 * 5).reshape(2, 3, 5) % 7).astype(dt)
        p = str(tmp_path / f"{dt.str}.nii.gz")
        nifti.save(a, p, hdr)
        arr, h = nifti.load(p)
        ph = nifti.parse_header(gzip.open(p).read())
        _same_header(ph.header, h)
        assert ph.shape == arr.shape and ph.dtype == arr.dtype and ph.vox_offset == 352 and ph.endian == "<"
        assert not ph.scaled and ph.out_dtype == arr.dtype
    # big endian: the header and the voxels swapped
    a = np.arange(24, dtype=np.int16).reshape(2, 3, 4)
    h = bytearray(nifti.header_bytes(a.shape, a.dtype))
    be = bytearray(352)
    for off, fmt in ((0, "i"), (40, "8h"), (70, "h"), (72, "h"), (76, "8f"), (108, "f"), (112, "2f"), (280, "12f")):
        struct.pack_into(">" + fmt, be, off, *struct.unpack_from("<" + fmt, h, off))
    be[344:348] = h[344:348]
    raw = bytes(be) + np.asfortranarray(a).astype(">i2").tobytes(order="F")
    p = str(tmp_path / "be.nii")
    open(p, "wb").write(raw)
    arr, hd = nifti.load(p)
    ph = nifti.parse_header(raw)
    assert ph.endian == ">" and ph.shape == arr.shape and ph.dtype == arr.dtype
    _same_header(ph.header, hd)
    np.testing.assert_array_equal(arr, a)
    # slope and intercept: the promoted dtype of a * slope + inter
    for dt, want in ((np.uint8, np.float64), (np.float32, np.float32), (np.int64, np.float64), (np.float64, np.float64)):
        h = bytearray(nifti.header_bytes((4, 5), np.dtype(dt)))
        struct.pack_into("<2f", h, 112, 2.5, -1.25)
        raw = bytes(h) + (np.arange(20) % 9).astype(dt).tobytes()
        p = str(tmp_path / f"s{np.dtype(dt).str}.nii")
        open(p, "wb").write(raw)
        arr, hd = nifti.load(p)
        ph = nifti.parse_header(raw)
        assert ph.scaled and ph.out_dtype == arr.dtype == np.dtype(want)
        assert (ph.slope, ph.inter) == (2.5, -1.25)
        _same_header(ph.header, hd)


def test_parse_header_refuses_non_nifti():
    from values_amd import nifti
    with pytest.raises(ValueError):
        nifti.parse_header(b"\0" * 352)
    with pytest.raises(ValueError):
        nifti.parse_header(b"\0" * 10)


@pytest.fixture(scope="module")
def host_decoder():
    with tempfile.TemporaryDirectory() as td:
        yield ic.build_host_decoder(td), td


def test_host_decoder_matches_zlib(host_decoder):
    exe, td = host_decoder
    corpus = ic.good_corpus()
    names = list(corpus)
    res = ic.run_host_decoder(exe, [(corpus[k][0], corpus[k][1], ic.capacity_for(len(corpus[k][2]))) for k in names], td)
    for k, (st, out) in zip(names, res):
        assert st == ic.OK, (k, st)
        assert out == corpus[k][2], k


def test_host_decoder_exact_capacity(host_decoder):
    exe, td = host_decoder
    corpus = ic.good_corpus()
    fmt, comp, data = corpus["walk_l6"]
    (st, out), (st2, out2) = ic.run_host_decoder(exe, [(fmt, comp, len(data)), (fmt, comp, len(data) - 1)], td)
    assert st == ic.OK and out == data
    assert st2 == ic.CAPACITY and data.startswith(out2)


def test_host_decoder_rejects_corrupt_set(host_decoder):
    exe, td = host_decoder
    bad = ic.corrupt_corpus()
    names = list(bad)
    res = ic.run_host_decoder(exe, [(bad[k][0], bad[k][1], bad[k][2] or 1 << 16) for k in names], td)
    text = ic.payloads()["text"][:2000]
    seen = set()
    for k, (st, out) in zip(names, res):
        want = bad[k][3]
        if want is None:   # a bit flip: refused, or harmless (MTIME, OS, ...) with the original output
            assert st != ic.OK or out == text, (k, st)
        else:
            assert st == want, (k, st, want)
        seen.add(st)
    assert {ic.TRUNCATED, ic.BAD_BLOCK, ic.BAD_LENGTHS, ic.BAD_DISTANCE, ic.BAD_CHECK, ic.BAD_ISIZE, ic.CAPACITY,
            ic.TRAILING, ic.BAD_SYMBOL, ic.BAD_HEADER, ic.BAD_STORED, ic.DICT} <= seen
