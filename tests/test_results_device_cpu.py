"""CPU: the host side of the device results writer -- vx_gzip_bound, the ctypes mirrors of vx_nifti_item / vx_gz_item,
argument refusals before any HIP call, nifti.header_bytes and results.plan_case against the host writer."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from values_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_gzip_bound_formula_and_overhead(lib):
    for n in (0, 1, 7, 32767, 32768, 32769, 1 << 20, 5 << 20, 48 << 20, (1 << 20) + 12345):
        chunks = max(1, -(-n // 32768))
        assert lib.vx_gzip_bound(n) == n + 5 * chunks + 18, n
        if n >= 1 << 20:
            assert lib.vx_gzip_bound(n) <= n + n // 1000 + 64, n
    assert lib.vx_gzip_bound(-1) < 0


def test_gzip_workspace_bytes_grows_with_chunks(lib):
    from values_amd import gz
    one = gz.workspace_bytes([32768])
    assert gz.workspace_bytes([32769]) > one > 0
    assert gz.workspace_bytes([10, 20]) > one
    assert lib.vx_gzip_workspace_bytes((ctypes.c_int64 * 1)(-5), 1) == 0


def test_new_struct_sizes_match_c(lib):
    from values_amd import _lib
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "values_amd.h"
int main(void){printf("%zu %zu %zu %zu\n", sizeof(vx_nifti_item), sizeof(vx_gz_item), offsetof(vx_nifti_item, header),
 offsetof(vx_gz_item, stride_hint)); return 0;}
'''
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write(code)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(_lib.NiftiItem), ctypes.sizeof(_lib.GzItem), _lib.NiftiItem.header.offset,
                     _lib.GzItem.stride_hint.offset]


FAKE = ctypes.c_void_p(1 << 20)   # never dereferenced: every call below is refused before it touches the device


def test_gzip_encode_refusals(lib):
    from values_amd import _lib
    item = (_lib.GzItem * 1)()
    item[0].src, item[0].n, item[0].dst_off = FAKE, 100, 0
    big = 1 << 30
    assert lib.vx_gzip_encode(None, 1, FAKE, big, FAKE, FAKE, big, None) == -1
    assert lib.vx_gzip_encode(item, 1, None, big, FAKE, FAKE, big, None) == -1
    assert lib.vx_gzip_encode(item, 1, FAKE, big, None, FAKE, big, None) == -1
    assert lib.vx_gzip_encode(item, -1, FAKE, big, FAKE, FAKE, big, None) == -2
    item[0].n = -1
    assert lib.vx_gzip_encode(item, 1, FAKE, big, FAKE, FAKE, big, None) == -2
    item[0].n = 100
    assert lib.vx_gzip_encode(item, 1, FAKE, 50, FAKE, FAKE, big, None) == -2           # slot beyond dst
    item[0].stride_hint[1] = 40000
    assert lib.vx_gzip_encode(item, 1, FAKE, big, FAKE, FAKE, big, None) == -2          # hint beyond the window
    item[0].stride_hint[1] = 0
    assert lib.vx_gzip_encode(item, 1, FAKE, big, FAKE, FAKE, 16, None) == -4           # workspace too small
    item[0].src = None
    assert lib.vx_gzip_encode(item, 1, FAKE, big, FAKE, FAKE, big, None) == -1
    assert lib.vx_gzip_encode(item, 0, FAKE, big, FAKE, FAKE, big, None) == 0           # nothing to do


def test_crc32_refusals(lib):
    assert lib.vx_crc32(FAKE, -1, FAKE, None) == -2
    assert lib.vx_crc32(FAKE, 10, None, None) == -1
    assert lib.vx_crc32(None, 10, FAKE, None) == -1


def test_nifti_payload_refusals(lib):
    from values_amd import _lib
    it = (_lib.NiftiItem * 1)()
    it[0].src, it[0].kind, it[0].esize, it[0].X, it[0].Y, it[0].Z = FAKE, _lib.VX_NIFTI_COPY, 4, 4, 4, 4
    big = 1 << 30
    ws = lib.vx_nifti_workspace_bytes(1)
    assert ws > 0
    assert lib.vx_nifti_payload_bytes(it) == 352 + 64 * 4
    assert lib.vx_nifti_payload(None, 1, FAKE, big, FAKE, ws, None) == -1
    assert lib.vx_nifti_payload(it, 1, None, big, FAKE, ws, None) == -1
    assert lib.vx_nifti_payload(it, 1, FAKE, big, None, ws, None) == -1
    assert lib.vx_nifti_payload(it, -1, FAKE, big, FAKE, ws, None) == -2
    assert lib.vx_nifti_payload(it, 1, ctypes.c_void_p((1 << 20) + 4), big, FAKE, ws, None) == -5
    assert lib.vx_nifti_payload(it, 1, FAKE, 100, FAKE, ws, None) == -2                # payload beyond dst
    assert lib.vx_nifti_payload(it, 1, FAKE, big, FAKE, ws - 1, None) == -4
    it[0].dst_off = 8
    assert lib.vx_nifti_payload(it, 1, FAKE, big, FAKE, ws, None) == -5
    it[0].dst_off = 0
    it[0].esize = 3
    assert lib.vx_nifti_payload(it, 1, FAKE, big, FAKE, ws, None) == -3
    it[0].kind = 7
    assert lib.vx_nifti_payload(it, 1, FAKE, big, FAKE, ws, None) == -3
    it[0].kind, it[0].src_dtype, it[0].T, it[0].C, it[0].t = _lib.VX_NIFTI_PROB, 0, 2, 2, 2
    assert lib.vx_nifti_payload(it, 1, FAKE, big, FAKE, ws, None) == -2                # t out of range
    it[0].t, it[0].src_dtype = 0, 5
    assert lib.vx_nifti_payload(it, 1, FAKE, big, FAKE, ws, None) == -3


@pytest.mark.parametrize("header", [None, {"pixdim": [0.7, 0.8, 2.5], "affine": np.diag([0.7, -0.8, 2.5, 1.0])}])
def test_header_bytes_is_the_front_of_save(tmp_path, header):
    from values_amd import nifti
    for dt in list(nifti._DT) + [np.dtype("bool"), np.dtype("float16"), np.dtype(">i4")]:
        a = (np.arange(24).reshape(2, 3, 4) % 2).astype(dt)
        p = str(tmp_path / f"{dt.str}.nii")
        nifti.save(a, p, header)
        raw = open(p, "rb").read()
        fd = nifti.file_dtype(a.dtype)
        assert nifti.header_bytes(a.shape, fd, header) == raw[:352], dt
        assert len(raw) == 352 + a.size * fd.itemsize


def _tree(d):
    out = set()
    for root, _, files in os.walk(d):
        for f in files:
            out.add(os.path.relpath(os.path.join(root, f), d))
    return out


@pytest.mark.parametrize("T", [1, 10])
@pytest.mark.parametrize("with_gt", [False, True])
@pytest.mark.parametrize("with_maps", [False, True])
def test_plan_case_lists_what_save_case_writes(tmp_path, T, with_gt, with_maps):
    from values_amd.results import plan_case, save_case
    rng = np.random.default_rng(T)
    sm = rng.random((T, 2, 3, 4, 5)).astype(np.float32)
    maps = {"pred_entropy": rng.random((3, 4, 5)).astype(np.float32),
            "epistemic_uncertainty": rng.random((3, 4, 5)).astype(np.float16)} if with_maps else None
    gt = (rng.random((3, 3, 4, 5)) > 0.5) if with_gt else None
    data = rng.random((3, 4, 5))
    save_case(str(tmp_path), "c7", sm, maps, data=data, gt_seg=gt)
    plan = plan_case("c7", sm, maps, data=data, gt_seg=gt)
    assert {f.path for f in plan} == _tree(str(tmp_path))
    assert len(plan) == len({f.path for f in plan})
    from values_amd import nifti
    for f in plan:
        a, h = nifti.load(str(tmp_path / f.path))
        assert a.shape == tuple(f.shape), f.path
        assert a.dtype == f.dtype, f.path
    assert sum(f.kind == "MEAN_PROB" for f in plan) == (2 if T > 1 else 0)
