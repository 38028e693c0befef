"""CPU: the host logic of the device Softmax tree setup -- the chunk size under the byte budget, the item / plane tables of
a batched 1 - max softmax call, the plan of the map files -- and the C ABI of the new entry point."""
import ctypes
import os

import numpy as np
import pytest


def test_chunk_size_under_the_byte_budget():
    from values_amd.experiment import DeviceExperimentDataloader, softmax_chunk_size
    assert DeviceExperimentDataloader.softmax_chunk == 32 and DeviceExperimentDataloader.softmax_budget_bytes == 1 << 30
    f64, f32 = np.dtype("float64"), np.dtype("float32")
    # small volumes: the chunk stays what it is
    assert softmax_chunk_size([(5, 4, 3), (16, 9, 7)], [f64, f64], 2, 32, 1 << 30) == 32
    # the LARGEST image sizes the chunk: 2 classes x 100^3 float64 = 16 MB per image
    shapes, dts = [(10, 10, 10), (100, 100, 100), (20, 20, 20)], [f64] * 3
    assert softmax_chunk_size(shapes, dts, 2, 32, 16_000_000 * 5) == 5
    assert softmax_chunk_size(shapes, dts, 2, 32, 16_000_000 * 5 - 1) == 4
    assert softmax_chunk_size(shapes, dts, 2, 3, 16_000_000 * 5) == 3
    # the dtype and the class count enter: float32 planes are half the bytes, 4 classes twice
    assert softmax_chunk_size(shapes, [f32] * 3, 2, 32, 16_000_000 * 5) == 10
    assert softmax_chunk_size(shapes, dts, 4, 32, 16_000_000 * 5) == 2
    # the floor: one image, however small the budget
    assert softmax_chunk_size(shapes, dts, 2, 32, 1) == 1
    assert softmax_chunk_size(shapes, dts, 2, 32, 0) == 1
    assert softmax_chunk_size([(6, 5)], [f32], 3, 1, 1 << 30) == 1
    # nothing to size by
    assert softmax_chunk_size([], [], 2, 32, 1 << 30) == 32
    assert softmax_chunk_size([(0, 4, 4)], [f64], 2, 32, 1 << 30) == 32


def test_item_and_plane_tables_of_mixed_items():
    from values_amd import _lib
    from values_amd.uncertainty import msr_tables
    entries = [(0x1000, 60, _lib.VX_F32, [0x2000, 0x3000]),
               (None, 0, _lib.VX_F64, [None, None, None]),
               (0x4000, 7, _lib.VX_F64, [0x5000]),
               (0x6000, 9, _lib.VX_F32, [0x7000 + 4 * k for k in range(19)])]
    items, table, n_planes = msr_tables(entries)
    assert n_planes == 2 + 3 + 1 + 19 and len(table) == n_planes and len(items) == 4
    assert [it.first_plane for it in items] == [0, 2, 5, 6]
    assert [it.C for it in items] == [2, 3, 1, 19]
    assert [it.n for it in items] == [60, 0, 7, 9]
    assert [it.dtype for it in items] == [_lib.VX_F32, _lib.VX_F64, _lib.VX_F64, _lib.VX_F32]
    assert [it.out for it in items] == [0x1000, None, 0x4000, 0x6000]
    assert list(table) == [0x2000, 0x3000, None, None, None, 0x5000] + [0x7000 + 4 * k for k in range(19)]
    for it, (_, _, _, planes) in zip(items, entries):
        assert list(table[it.first_plane:it.first_plane + it.C]) == planes
    # no entries at all: a table that can still be passed (one null pointer), zero planes
    items, table, n_planes = msr_tables([])
    assert len(items) == 0 and n_planes == 0 and len(table) == 1


def test_map_plan_follows_the_host_writer():
    import torch
    from values_amd.results import plan_maps
    plan = plan_maps(["a/x.nii.gz", "a/y.nii", "a/z.tif", "a/w.TIFF"],
                     [torch.zeros((5, 4, 3), dtype=torch.float64), np.zeros((2, 3), np.float32),
                      torch.zeros((7, 5), dtype=torch.float64), np.zeros((4, 6), np.float32)])
    assert [f.kind for f in plan] == ["gz", "nii", "tif", "tif"]
    assert [f.shape for f in plan] == [(5, 4, 3), (2, 3), (5, 7), (6, 4)]     # a TIFF is stored (H, W): axes swapped back
    assert [f.dtype for f in plan] == [np.dtype("float64"), np.dtype("float32"), np.dtype("float32"), np.dtype("float32")]
    assert all(os.path.isabs(f.path) for f in plan)
    with pytest.raises(ValueError):
        plan_maps(["a/x.png"], [np.zeros((2, 2), np.float32)])
    with pytest.raises(ValueError):
        plan_maps(["a/x.tif"], [np.zeros((2, 2, 2), np.float32)])
    with pytest.raises(ValueError):
        plan_maps(["a/x.tif"], [])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from values_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_entry_point_is_declared_exported_bound_and_refuses_on_the_host(lib):
    from tests.test_abi import declared_functions
    from values_amd import _lib
    names = declared_functions()
    for n in ("vx_one_minus_msr", "vx_one_minus_msr_batched", "vx_one_minus_msr_batched_workspace_bytes"):
        assert n in names and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.vx_version() >= 820
    assert ctypes.sizeof(_lib.MsrItem) == 32
    # the workspace holds the two tables, each rounded up to 256 bytes; 0 for counts the call refuses
    assert lib.vx_one_minus_msr_batched_workspace_bytes(1, 1) == 512
    assert lib.vx_one_minus_msr_batched_workspace_bytes(9, 33) == 512 + 512
    assert lib.vx_one_minus_msr_batched_workspace_bytes(0, 4) == 0 and lib.vx_one_minus_msr_batched_workspace_bytes(4, 0) == 0
    assert lib.vx_one_minus_msr_batched_workspace_bytes(_lib.VX_MSR_MAX_ITEMS + 1, 4) == 0
    # every refusal comes before any device call: they answer on a machine without a GPU too (pointers never dereferenced)
    from values_amd.uncertainty import msr_tables
    ws = 0x100000

    def rc(entries, n_items=None, n_planes=None, ws_ptr=ws, ws_bytes=1 << 20):
        items, table, count = msr_tables(entries)
        return lib.vx_one_minus_msr_batched(items, len(entries) if n_items is None else n_items, table,
                                            count if n_planes is None else n_planes, ws_ptr, ws_bytes, None)
    good = (0x10000, 16, _lib.VX_F64, [0x20000, 0x30000])
    assert lib.vx_one_minus_msr_batched(None, 1, None, 1, ws, 1 << 20, None) == -1
    assert rc([(0x10000, 16, _lib.VX_F64, [0x20000, None])]) == -1
    assert rc([good], ws_ptr=None) == -1
    assert rc([good], n_items=0) == -2 and rc([(0x10000, -1, _lib.VX_F64, [0x20000])]) == -2
    assert rc([good], n_planes=1) == -2 and rc([(0x10000, 16, _lib.VX_F64, [])], n_planes=1) == -2
    assert rc([(0x10000, 16, 5, [0x20000])]) == -3
    assert rc([(0x10004, 16, _lib.VX_F64, [0x20000])]) == -5 and rc([(0x10000, 16, _lib.VX_F32, [0x20002])]) == -5
    assert rc([good], ws_ptr=ws + 8) == -5
    assert rc([good], ws_bytes=511) == -4
    assert b"vx_one_minus_msr_batched" in lib.vx_last_error_string()
