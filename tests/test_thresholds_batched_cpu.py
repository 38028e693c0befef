"""CPU: the host side of the batched threshold search -- the ctypes mirrors of vx_count_item / vx_select_item, the
refusals of vx_count_nonzero_batched / vx_select_segments before any HIP call, and the Python argument errors of
thresholds.quantile_segments / count_nonzero_batch that need no device."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(1 << 20)   # never dereferenced: every call below is refused before it touches the device
E_NULL, E_SHAPE, E_DTYPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5


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
int main(void){printf("%zu %zu %zu %zu %zu %zu %d %d %d %d\n", sizeof(vx_count_item), offsetof(vx_count_item, n),
 offsetof(vx_count_item, kind), sizeof(vx_select_item), offsetof(vx_select_item, n), offsetof(vx_select_item, dtype),
 VX_SELECT_MAX_ITEMS, VX_COUNT_F32, VX_COUNT_F64, VX_SELECT_NAN); return 0;}
'''
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write(code)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(_lib.CountItem), _lib.CountItem.n.offset, _lib.CountItem.kind.offset,
                     ctypes.sizeof(_lib.SelectItem), _lib.SelectItem.n.offset, _lib.SelectItem.dtype.offset,
                     _lib.VX_SELECT_MAX_ITEMS, _lib.VX_COUNT_F32, _lib.VX_COUNT_F64, _lib.VX_SELECT_NAN]


def test_count_refusals(lib):
    from values_amd import _lib
    it = (_lib.CountItem * 3)()
    for i, kind in enumerate((_lib.VX_COUNT_B1, _lib.VX_COUNT_B4, _lib.VX_COUNT_F64)):
        it[i].ptr, it[i].n, it[i].kind = 1 << 20, 100, kind
    ws = lib.vx_count_nonzero_batched_workspace_bytes(3)
    assert lib.vx_version() >= 770
    assert ws > 0 and lib.vx_count_nonzero_batched_workspace_bytes(-1) == 0
    assert lib.vx_count_nonzero_batched_workspace_bytes(_lib.VX_SELECT_MAX_ITEMS + 1) == 0
    call = lambda items=it, n=3, counts=FAKE, w=FAKE, wb=ws: lib.vx_count_nonzero_batched(items, n, counts, w, wb, None)
    assert call(items=None) == E_NULL
    assert call(n=-1) == E_SHAPE
    assert call(n=_lib.VX_SELECT_MAX_ITEMS + 1) == E_SHAPE
    assert call(n=0) == 0                                  # nothing to count: no device call
    assert call(counts=None) == E_NULL
    assert call(w=None) == E_NULL
    assert call(wb=ws - 1) == E_WORKSPACE
    assert call(w=ctypes.c_void_p((1 << 20) + 8)) == E_ALIGN
    for kind in (-1, 6):
        it[1].kind = kind
        assert call() == E_DTYPE
        assert b"item 1" in lib.vx_last_error_string()
    it[1].kind = _lib.VX_COUNT_B4
    it[2].n = -1
    assert call() == E_SHAPE
    it[2].n = 100
    it[2].ptr = (1 << 20) + 4                              # a float64 item off its 8-byte alignment
    assert call() == E_ALIGN
    it[2].ptr = None
    assert call() == E_NULL
    assert b"item 2" in lib.vx_last_error_string()


def test_select_refusals(lib):
    from values_amd import _lib
    it = (_lib.SelectItem * 3)()
    for i, (dt, n) in enumerate(((_lib.VX_F32, 100), (_lib.VX_F64, 0), (_lib.VX_F32, 50))):
        it[i].ptr, it[i].n, it[i].dtype = (1 << 20) + 4 * i, n, dt
    it[1].ptr = None                                       # an empty item's pointer is not looked at
    ws = lib.vx_select_segments_workspace_bytes(3)
    assert ws > 0 and lib.vx_select_segments_workspace_bytes(0) == 0 and lib.vx_select_segments_workspace_bytes(-1) == 0
    call = lambda items=it, n=3, k=0, out=FAKE, st=FAKE, w=FAKE, wb=ws: lib.vx_select_segments(items, n, k, out, st, w, wb, None)
    assert call(items=None) == E_NULL
    assert call(n=-1) == E_SHAPE
    assert call(n=0) == E_SHAPE
    assert call(k=-1) == E_SHAPE
    assert call(k=150) == E_SHAPE                          # k >= n_total
    assert call(k=1 << 40) == E_SHAPE
    assert call(out=None, k=149) == E_NULL
    assert call(st=None) == E_NULL
    assert call(w=None) == E_NULL
    assert call(wb=ws - 1) == E_WORKSPACE
    assert call(w=ctypes.c_void_p((1 << 20) + 8)) == E_ALIGN
    it[2].dtype = 2
    assert call() == E_DTYPE
    assert b"item 2" in lib.vx_last_error_string()
    it[2].dtype = _lib.VX_F32
    it[0].ptr = None
    assert call() == E_NULL
    it[0].ptr = (1 << 20) + 2                              # a float32 item off its 4-byte alignment
    assert call() == E_ALIGN
    it[0].ptr = 1 << 20
    it[0].n, it[2].n = 0, 0
    assert call() == E_SHAPE                               # the empty union
    it[0].n = -5
    assert call() == E_SHAPE


def test_python_argument_errors_need_no_device():
    from values_amd import thresholds
    x = torch.zeros(5)
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="Quantiles must be in the range"):
            thresholds.quantile_segments([x], q)
    with pytest.raises(ValueError, match="empty"):
        thresholds.quantile_segments([], 0.5)
    with pytest.raises(ValueError, match="empty"):
        thresholds.quantile_segments([torch.zeros(0), torch.zeros((3, 0))], 0.5)
    assert thresholds.count_nonzero_batch([]) == []


def test_dense_views_are_passed_as_their_block():
    from values_amd.thresholds import _dense_block
    x = torch.arange(2 * 3 * 4.).reshape(2, 3, 4)
    for v in (x, x.transpose(0, 1), x.permute(2, 0, 1), x[1], x[:1].transpose(0, 2), x.reshape(6, 4).t()):
        b = _dense_block(v)
        assert b is v and b.data_ptr() == v.data_ptr()
    for v in (x[:, :, ::2], x[:, 1:], x.expand(2, 2, 3, 4)[:, 0], x.transpose(0, 2)[1:]):
        b = _dense_block(v)
        assert b.is_contiguous() and torch.equal(b, v)
