"""CPU: the host side of the 2D device results writer -- vx_png_bound, vx_png_workspace_bytes, the ctypes mirror of
vx_png_item, vx_png_encode's refusals before any HIP call, results2d.plan_images against the files the host writer
writes, and image_io.tiff_f32_parts against write_tiff_f32."""
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


def test_png_bound_formula(lib):
    for H, W in ((1, 1), (1, 5461), (2, 5461), (3, 5461), (512, 1024), (1024, 2048), (256, 478), (7, 1), (4096, 1)):
        n = H * (3 * W + 1)
        chunks = max(1, -(-n // 32768))
        assert lib.vx_png_bound(H, W) == n + 5 * chunks + 63, (H, W)
    assert lib.vx_png_bound(0, 5) < 0
    assert lib.vx_png_bound(5, 0) < 0
    assert lib.vx_png_bound(-1, 5) < 0


def _items(shapes):
    from values_amd import _lib
    arr = (_lib.PngItem * len(shapes))()
    for i, (h, w) in enumerate(shapes):
        arr[i].labels, arr[i].ignore, arr[i].H, arr[i].W = 1 << 20, None, h, w
    return arr


def test_png_workspace_bytes_grows_with_chunks(lib):
    one = lib.vx_png_workspace_bytes(_items([(1, 5461)]), 1)           # 16 384 scanline bytes: one chunk
    assert one > 0
    assert lib.vx_png_workspace_bytes(_items([(2, 5461)]), 1) > one    # 32 768: still one chunk, larger raw buffer
    two = lib.vx_png_workspace_bytes(_items([(3, 5461)]), 1)            # 49 152: two chunks
    assert two >= one + 32768
    assert lib.vx_png_workspace_bytes(_items([(1, 5461), (1, 5461)]), 2) > one
    assert lib.vx_png_workspace_bytes(_items([(0, 5)]), 1) == 0
    assert lib.vx_png_workspace_bytes(None, 1) == 0
    assert lib.vx_png_workspace_bytes(_items([(1, 1)]), 0) == 0


def test_png_item_size_matches_c(lib):
    from values_amd import _lib
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "values_amd.h"
int main(void){printf("%zu %zu %zu\n", sizeof(vx_png_item), offsetof(vx_png_item, H), offsetof(vx_png_item, W)); return 0;}
'''
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write(code)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(_lib.PngItem), _lib.PngItem.H.offset, _lib.PngItem.W.offset]


FAKE = ctypes.c_void_p(1 << 20)   # never dereferenced: every call below is refused before it touches the device


def test_png_encode_refusals(lib):
    it = _items([(4, 6)])
    big = 1 << 30
    enc = lib.vx_png_encode

    def call(items=it, n=1, lut=FAKE, unl=255, dst=FAKE, dst_bytes=big, offs=FAKE, sizes=FAKE, ws=FAKE, ws_bytes=big):
        return enc(items, n, lut, unl, dst, dst_bytes, offs, sizes, ws, ws_bytes, None)

    assert call(items=None) == -1
    assert call(lut=None) == -1
    assert call(dst=None) == -1
    assert call(offs=None) == -1
    assert call(sizes=None) == -1
    assert call(ws=None) == -1
    assert call(n=0) == -2
    assert call(n=-3) == -2
    assert call(unl=-1) == -2
    assert call(unl=256) == -2
    for h, w in ((0, 6), (4, 0), (-2, 6)):
        assert call(items=_items([(h, w)])) == -2, (h, w)
    assert call(items=_items([(1 << 16, 1 << 15)])) == -2                    # 2^31 or more scanline bytes
    assert call(dst_bytes=lib.vx_png_bound(4, 6) - 1) == -2                  # below the sum of bounds
    two = _items([(4, 6), (9, 3)])
    assert call(items=two, n=2, dst_bytes=lib.vx_png_bound(4, 6) + lib.vx_png_bound(9, 3) - 1) == -2
    need = lib.vx_png_workspace_bytes(it, 1)
    assert call(ws_bytes=need - 1) == -4                                       # short workspace
    assert call(ws=ctypes.c_void_p((1 << 20) + 8)) == -5                      # workspace not 16-byte aligned
    nolab = _items([(4, 6)])
    nolab[0].labels = None
    assert call(items=nolab) == -1


def test_png_encode_refusals_leave_a_message(lib):
    assert lib.vx_png_encode(_items([(4, 6)]), 1, FAKE, 300, FAKE, 1 << 30, FAKE, FAKE, FAKE, 1 << 30, None) == -2
    assert b"unlabeled" in lib.vx_last_error_string()


def _listing(d):
    out = []
    for root, _, fs in os.walk(d):
        out += [os.path.relpath(os.path.join(root, f), d) for f in fs]
    return sorted(out)


@pytest.mark.parametrize("n_pred", [1, 4])
def test_plan_images_matches_the_host_writer(tmp_path, monkeypatch, n_pred):
    """save_prediction / save_uncertainty on the host (colorize replaced by a host lookup: no GPU) -- the planned paths
    are exactly the files they write"""
    import torch
    from values_amd import results2d
    monkeypatch.setattr(results2d, "colorize", lambda lab, ign=None: torch.from_numpy(results2d._lut()[lab.numpy()]))
    ids = ["img0", "frankfurt_000001"]
    unc = ["pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty"]
    rng = np.random.default_rng(0)
    os.makedirs(tmp_path / "pred_seg")
    for iid in ids:
        pm = torch.from_numpy(rng.integers(0, 19, (n_pred, 5, 7), dtype=np.uint8))
        results2d.save_prediction(str(tmp_path / "pred_seg"), iid, pm, pm[0] if n_pred > 1 else None)
        results2d.save_uncertainty(str(tmp_path), iid, {k: torch.rand(5, 7) for k in unc})
    plan = results2d.plan_images(ids, n_pred, unc)
    assert sorted(f.path for f in plan) == _listing(tmp_path)
    assert len(plan) == len(ids) * ((n_pred + 1 if n_pred > 1 else 1) + len(unc))
    assert any(f.path.endswith("_mean.png") for f in plan) == (n_pred > 1)
    assert plan[0].source == (("mean", 0) if n_pred > 1 else ("pred", 0, 0))


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (512, 1024), (7, 1), (1, 9)])
def test_tiff_parts_around_the_data_equal_write_tiff(tmp_path, shape):
    from values_amd.image_io import read_tiff_f32, tiff_f32_parts, write_tiff_f32
    a = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    p = str(tmp_path / "m.tif")
    write_tiff_f32(p, a)
    head, tail = tiff_f32_parts(*shape)
    assert open(p, "rb").read() == head + a.astype("<f4").tobytes() + tail
    np.testing.assert_array_equal(read_tiff_f32(p), a)
