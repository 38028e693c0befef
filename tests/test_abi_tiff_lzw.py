"""CPU: the LZW TIFF entry points (vx_tiff_lzw, vx_tiff_unpredict) are exported and bound, their item structs have the
C sizes, and their argument checks run before any launch -- so a wrong call is refused on a box without a GPU too."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vx_tiff_lzw_workspace_bytes", "vx_tiff_lzw", "vx_tiff_unpredict_workspace_bytes", "vx_tiff_unpredict")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from values_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from values_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "values_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vx_[a-zA-Z0-9_]+)\s*\(", hdr))
    for n in NEW:
        assert n in declared and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert (_lib.VX_LZW_OK, _lib.VX_LZW_TRUNCATED, _lib.VX_LZW_BAD_CODE) == (0, 1, 2) and len(_lib.LZW_STATUS) == 3


def test_item_struct_sizes_match_c(lib):
    from values_amd import _lib
    code = r'''
#include <stdio.h>
#include "values_amd.h"
int main(void){printf("%zu %zu %d %d %d\n", sizeof(vx_tiff_lzw_item), sizeof(vx_tiff_unpredict_item), VX_LZW_OK, VX_LZW_TRUNCATED,
 VX_LZW_BAD_CODE); return 0;}
'''
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write(code)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])  # header is plain C
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(_lib.TiffLzwItem), C.sizeof(_lib.TiffUnpredictItem), 0, 1, 2]
    assert C.sizeof(_lib.TiffLzwItem) == 32 and C.sizeof(_lib.TiffUnpredictItem) == 32


def test_argument_errors_are_refused_without_a_gpu(lib):
    from values_amd import _lib
    dummy = 0x10000                      # never dereferenced: every call below is refused by a host-side check
    big = 1 << 20
    assert lib.vx_tiff_lzw_workspace_bytes(-1) == -1 and lib.vx_tiff_unpredict_workspace_bytes(-1) == -1
    assert lib.vx_tiff_lzw_workspace_bytes(3) >= 256 + 3 * 32 and lib.vx_tiff_unpredict_workspace_bytes(3) >= 256 + 3 * 32

    def lzw(items, n=None, dst=dummy, dst_n=4096, ws=dummy, ws_n=big, table=True):
        arr = (_lib.TiffLzwItem * max(len(items), 1))()
        for it, (src, src_n, off, cap) in zip(arr, items):
            it.src, it.src_n, it.dst_off, it.dst_cap = src, src_n, off, cap
        return lib.vx_tiff_lzw(arr if table else None, len(items) if n is None else n, dst, dst_n, dummy, dummy, ws, ws_n, None)

    ok = (dummy, 10, 0, 100)
    assert lzw([], n=0, table=False) == 0                                   # nothing to do
    refused = [lzw([ok], table=False), lzw([ok], n=-1), lzw([ok], dst=None), lzw([ok], ws=None),
               lzw([ok], ws_n=lib.vx_tiff_lzw_workspace_bytes(1) - 1),
               lzw([(None, 10, 0, 100)]), lzw([(dummy, -1, 0, 100)]), lzw([(dummy, 10, -1, 100)]), lzw([(dummy, 10, 0, -1)]),
               lzw([(dummy, 10, 4000, 100)]),                                # a window beyond dst_n
               lzw([(dummy, 10, 0, 1 << 33)], dst_n=1 << 34),                # a window of 4 GiB or more
               lzw([ok, (dummy, 10, 50, 100)])]                              # windows that overlap
    for rc in refused:
        assert rc < 0, (rc, lib.vx_last_error_string())
    assert b"overlaps" in lib.vx_last_error_string()
    assert lzw([(dummy, 10, 2**63 - 51, 100)]) == -2                         # dst_off + dst_cap overflows int64

    def unp(items, n=None, status=dummy, ws=dummy, ws_n=big, table=True):
        arr = (_lib.TiffUnpredictItem * max(len(items), 1))()
        for it, (src, dst, rows, w, pred) in zip(arr, items):
            it.src, it.dst, it.rows, it.W, it.predictor = src, dst, rows, w, pred
        return lib.vx_tiff_unpredict(arr if table else None, len(items) if n is None else n, status, ws, ws_n, None)

    a, b = 0x10000, 0x90000
    good = (a, b, 4, 16, 3)
    assert unp([], n=0, table=False) == 0
    refused = [unp([good], table=False), unp([good], n=-1), unp([good], status=None), unp([good], ws=None),
               unp([good], ws_n=lib.vx_tiff_unpredict_workspace_bytes(1) - 1),
               unp([(a, b, 4, 0, 3)]), unp([(a, b, 4, -5, 2)]), unp([(a, b, 0, 16, 2)]),          # W < 1, rows < 1
               unp([(a, b, 4, 16, 1)]), unp([(a, b, 4, 16, 4)]), unp([(a, b, 4, 16, 0)]),         # predictor outside 2 / 3
               unp([(None, b, 4, 16, 2)]), unp([(a, None, 4, 16, 2)]),
               unp([(a, a, 4, 16, 3)]),                                                             # in place: predictor 2 only
               unp([(a, a + 64, 4, 16, 2)])]                                                        # a partial overlap
    for rc in refused:
        assert rc < 0, (rc, lib.vx_last_error_string())
