"""CPU: the host half of the toy data set generator (values_amd/toydata.py) -- the restated blur against
scipy.ndimage.gaussian_filter bit for bit and the product mirror against the restatement, the plan against a literal replay
of the reference's calls on `random`, both embed functions, the rater thresholds with np.arange's quirk, the data set tree
read back -- and the C ABI of the toy data kernels: symbols and every refusal with its code, all before any device call.
The host plan (values_amd/csrc/toy_plan.h) also runs in a stand-alone program under ASan / UBSan."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

from tests import toy_ref
from tests.helpers import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_DTYPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5
BLUR_CASES = [((5, 7, 3), 2), ((40, 33, 17), 8), ((9, 70, 12), 8), ((1, 2, 66), 3)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from values_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------
# the blur

@pytest.mark.parametrize("shape,sigma", BLUR_CASES)
def test_restated_blur_equals_scipy_bit_for_bit(shape, sigma):
    ndimage = pytest.importorskip("scipy.ndimage")
    a = toy_ref.sparse_volume(shape, 3)
    want = ndimage.gaussian_filter(a, sigma=sigma)
    got = toy_ref.gaussian_blur(a, sigma)
    assert got.dtype == want.dtype == np.float64
    assert np.array_equal(got, want)
    assert (got != 0).any()


@pytest.mark.parametrize("shape,sigma", BLUR_CASES + [((3, 3, 3), 8)])
def test_product_mirror_blur_equals_the_restatement(shape, sigma):
    from values_amd import toydata
    a = toy_ref.sparse_volume(shape, 4)
    assert np.array_equal(toydata.gaussian_blur(a, sigma), toy_ref.gaussian_blur(a, sigma))
    w, r = toydata.gaussian_weights(sigma)
    w2, r2 = toy_ref.gaussian_weights(sigma)
    assert r == r2 == int(4.0 * sigma + 0.5) and np.array_equal(w, w2) and len(w) == 2 * r + 1
    for n in (1, 2, 3, 5):
        idx = np.arange(-130, n + 130)
        assert list(toydata.reflect_index(idx, n)) == [toy_ref.reflect_index(i, n) for i in idx]


def test_reflect_index_is_the_mirrored_extension():
    # d c b a | a b c d | d c b a
    assert [toy_ref.reflect_index(i, 4) for i in range(-4, 8)] == [3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0]
    assert [toy_ref.reflect_index(i, 1) for i in range(-3, 4)] == [0] * 7


# ---------------------------------------------------------------------------------------------
# the plan and the embed functions

def replay(object_fn, n_samples, image_size, min_ratio, max_ratio, over_border, gray, seed):
    """the reference's create_dataset_samples reduced to its calls on `random`, in its order"""
    random.seed(seed)
    out = []
    for _ in range(n_samples):
        obj = object_fn(random.randint(int(max(image_size) / min_ratio), int(max(image_size) / max_ratio)))
        room = [image_size[a] - obj.shape[a] for a in range(3)]
        lr = ud = False
        if not over_border:
            offset = [random.randint(0, room[0]), random.randint(0, room[1]), random.randint(0, room[2])]
        else:
            lows = [int(-2 * s / 3) for s in obj.shape]
            bits = format(random.randint(1, 7), "b").zfill(3)      # which axes take a negative offset
            offset = []
            for a in range(3):                                      # one draw per axis, axis 0 first
                offset.append(random.randint(lows[a], 0) if bits[a] == "1" else random.randint(0, room[a]))
            lr = random.random() > 0.5                              # np.fliplr is drawn first
            ud = random.random() > 0.5
        g = random.uniform(0.5, 0.9) if gray else None
        out.append((obj.shape, offset, lr, ud, g))
    return out


@pytest.mark.parametrize("seed", [22, 7])
@pytest.mark.parametrize("over_border", [False, True])
def test_plan_samples_replays_the_reference_random_calls(seed, over_border):
    from values_amd.toydata import box_object, plan_samples, sphere_object
    for fn, gray in ((sphere_object, True), (box_object, False)):
        plan = plan_samples(fn, 6, (48, 40, 64), 10, 2, over_border, gray, seed)
        want = replay(fn, 6, (48, 40, 64), 10, 2, over_border, gray, seed)
        got = [(p["object"].shape, p["offset"], p["fliplr"], p["flipud"], p["gray"]) for p in plan]
        assert got == want
        assert all(p["object"].dtype == np.float32 and p["negative"] == over_border for p in plan)
        if over_border:
            assert any(min(p["offset"]) < 0 for p in plan)
    assert plan_samples(sphere_object, 1, 32)[0]["image_size"] == (32, 32, 32)


def test_embed_equals_the_literal_restatement():
    from values_amd.toydata import embed
    rng = np.random.default_rng(5)
    obj = (rng.random((9, 7, 11)) > 0.3).astype(np.float32) * rng.random((9, 7, 11)).astype(np.float32)
    size = (20, 16, 24)
    item = lambda **kw: dict({"object": obj, "image_size": size, "negative": False, "fliplr": False, "flipud": False, "gray": None}, **kw)
    got = embed(item(offset=[3, 9, 13]))
    assert got.dtype == np.float64 and np.array_equal(got, toy_ref.embed_positive([3, 9, 13], obj, size))
    assert np.array_equal(got[3:12, 9:16, 13:24], obj.astype(np.float64)) and got.sum() == obj.astype(np.float64).sum()
    for off in ([-6, -4, -7], [-6, 2, 0], [4, -1, 13], [0, 0, 0]):          # the first clips on all three axes
        for lr in (False, True):
            for ud in (False, True):
                want = toy_ref.embed_negative(off, obj, size)
                if lr:
                    want = np.fliplr(want)
                if ud:
                    want = np.flipud(want)
                got = embed(item(offset=off, negative=True, fliplr=lr, flipud=ud, gray=0.7))
                assert np.array_equal(got, want * 0.7), (off, lr, ud)
    clipped = embed(item(offset=[-6, -4, -7], negative=True))
    assert np.array_equal(clipped[:3, :3, :4], obj[6:, 4:, 7:].astype(np.float64)) and clipped[3:].sum() == 0
    with pytest.raises(ValueError):
        embed(item(offset=[15, 0, 0]))     # does not fit: the reference prints and goes on with the bare object


# ---------------------------------------------------------------------------------------------
# raters, segmentations, noise

def test_rater_thresholds_keep_the_arange_quirk():
    from values_amd.toydata import rater_thresholds, segment
    image = toy_ref.gaussian_blur(toy_ref.sparse_volume((12, 10, 14), 6), 1.5)
    assert rater_thresholds(image, 1) == [0.1]
    assert rater_thresholds(image, 4, all_raters_same=True) == [0.1] * 4
    for n_raters in (3, 5):
        step = (1 - 0.1) / (n_raters - 1)
        perc = np.arange(0.1, 1 + step, step)           # the length is numpy's: it may be n_raters + 1
        ratio = np.count_nonzero(image >= 0.1) / image.size
        want = np.quantile(image, 1 - perc * ratio)
        got = rater_thresholds(image, n_raters)
        assert len(got) == len(perc) and len(perc) in (n_raters, n_raters + 1)
        assert np.array_equal(got, want)
        assert (np.diff(got) <= 0).all()                 # later raters segment more
        segs = segment(image, got)
        assert len(segs) == len(perc)
        for s, t in zip(segs, got):
            assert s.dtype == np.intc and np.array_equal(s, np.where(image >= t, 1, 0))
    assert len(np.arange(0.1, 1 + 0.9 / 2, 0.9 / 2)) == len(rater_thresholds(image, 3))


def test_add_noise_draws_numpys_stream_like_the_reference():
    from values_amd.toydata import add_noise
    image = toy_ref.gaussian_blur(toy_ref.sparse_volume((6, 5, 7), 8), 1.0)
    np.random.seed(22)
    got = add_noise(image.copy(), 0.5)
    np.random.seed(22)
    prob = np.random.rand(6, 5, 7)
    noise = np.random.rand(6, 5, 7)
    noise[prob <= 0.5] = 0
    want = np.where(image < 0.1, noise, image)
    assert np.array_equal(got, want) and np.array_equal(got[image >= 0.1], image[image >= 0.1])


def test_noise_restatement_words_and_ranges():
    h1, h2 = toy_ref.hash_words(22, 3, 1000)
    assert h1.max() < 2 ** 32 and len(set(h1.tolist())) > 990 and not np.array_equal(h1, h2)
    a1, _ = toy_ref.hash_words(22, 4, 1000)
    assert not np.array_equal(h1, a1)
    out = toy_ref.add_noise(np.zeros((10, 10, 10)), 22, 0)
    assert ((out >= 0) & (out < 1)).all() and 0.4 < (out == 0).mean() < 0.6


# ---------------------------------------------------------------------------------------------
# the data set on the host

def test_dataset_info_suffix_search(tmp_path):
    from values_amd.toydata import _info_path
    d = str(tmp_path)
    assert _info_path(d) == os.path.join(d, "dataset_info_1.json")
    open(os.path.join(d, "dataset_info_1.json"), "w").close()
    open(os.path.join(d, "dataset_info_3.json"), "w").close()
    assert _info_path(d) == os.path.join(d, "dataset_info_2.json")
    open(os.path.join(d, "dataset_info_2.json"), "w").close()
    assert _info_path(d) == os.path.join(d, "dataset_info_4.json")


def test_host_mirror_tree_reads_back_transposed(tmp_path):
    from values_amd import generate_toy_dataset, nifti
    from values_amd.toydata import (add_noise, embed, gaussian_blur, plan_samples, rater_thresholds, segment, sphere_object)
    save = str(tmp_path / "toy")
    kw = dict(n_samples=2, image_size=(20, 16, 24), gauss_sigma=1.5, object_gray=True, blur=True, noise=True, segmentation=True,
              n_raters=3, sample_offset=5, seed=7)
    generate_toy_dataset(save, sphere_object, **kw)
    plan = plan_samples(sphere_object, 2, (20, 16, 24), object_gray=True, seed=7)
    np.random.seed(7)
    n_seg = None
    for i, item in enumerate(plan):
        image = gaussian_blur(embed(item), 1.5)
        thr = rater_thresholds(image, 3)
        n_seg = len(thr)
        for r, seg in enumerate(segment(image, thr)):
            got, _ = nifti.load(os.path.join(save, "segmentation", f"{5 + i:04d}_{r:02d}.nii.gz"))
            assert got.dtype == np.int32 and np.array_equal(got, seg.transpose(2, 1, 0))
        image = add_noise(image, 0.5)
        got, _ = nifti.load(os.path.join(save, f"{5 + i:04d}.nii.gz"))
        assert got.dtype == np.float64 and got.shape == (24, 16, 20) and np.array_equal(got, image.transpose(2, 1, 0))
    assert sorted(os.listdir(save)) == ["0005.nii.gz", "0006.nii.gz", "dataset_info_1.json", "segmentation"]
    assert len(os.listdir(os.path.join(save, "segmentation"))) == 2 * n_seg
    info = json.load(open(os.path.join(save, "dataset_info_1.json")))
    assert list(info) == ["json_config", "input_files", "save_path", "n_samples", "image_size", "min_object_ratio", "max_object_ratio",
                          "gauss_sigma", "object_gray", "blur", "noise", "segmentation", "all_raters_same", "n_raters",
                          "object_over_border", "sample_offset", "seed"]
    assert info["image_size"] == [20, 16, 24] and info["seed"] == 7 and info["save_path"] == save
    generate_toy_dataset(save, sphere_object, n_samples=1, image_size=(20, 16, 24))
    assert os.path.isfile(os.path.join(save, "dataset_info_2.json")) and os.path.isfile(os.path.join(save, "0000.nii.gz"))


def test_device_route_fails_loudly_without_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from values_amd import _lib, generate_toy_dataset
    with pytest.raises(_lib.VxError):
        generate_toy_dataset(str(tmp_path / "t"), n_samples=1, image_size=16, device_io=True)


# ---------------------------------------------------------------------------------------------
# the C ABI

NAMES = ("vx_toy_embed", "vx_gauss_blur_axis_f64", "vx_count_ge_f64", "vx_order_stats_f64", "vx_order_stats_f64_workspace_bytes",
         "vx_order_stats_f64_reads", "vx_toy_segment", "vx_toy_noise")
A, B, W = 0x10000, 0x4000000, 0x8000000   # made-up device addresses: every call below is refused before anything looks at them


def i3(*v):
    return (C.c_int32 * 3)(*v)


def test_new_symbols_are_bound(lib):
    from values_amd import _lib
    header = open(os.path.join(ROOT, "include", "values_amd.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in header
    assert lib.vx_version() >= 890


def test_blur_and_embed_refusals_without_a_gpu(lib):
    blur = lambda src=A, dst=B, dims=(4, 4, 4), axis=0, w=W, r=2: lib.vx_gauss_blur_axis_f64(src, dst, i3(*dims), axis, w, r, None)
    cases = [(E_NULL, dict(src=None)), (E_NULL, dict(dst=None)), (E_NULL, dict(w=None)),
             (E_SHAPE, dict(axis=3)), (E_SHAPE, dict(axis=-1)), (E_SHAPE, dict(r=129)), (E_SHAPE, dict(r=-1)),
             (E_SHAPE, dict(dims=(4, 0, 4))), (E_SHAPE, dict(dims=(1 << 20, 1 << 20, 4))),
             (E_SHAPE, dict(dst=A)), (E_SHAPE, dict(dst=A + 64)), (E_SHAPE, dict(src=A + 64, dst=A)),
             (E_ALIGN, dict(src=A + 4)), (E_ALIGN, dict(dst=B + 4)), (E_ALIGN, dict(w=W + 2))]
    for k, (code, kw) in enumerate(cases):
        assert blur(**kw) == code, (k, lib.vx_last_error_string())
        assert lib.vx_last_error_string().startswith(b"vx_gauss_blur_axis_f64")
    assert lib.vx_gauss_blur_axis_f64(A, B, None, 0, W, 2, None) == E_NULL
    emb = lambda obj=A, od=(4, 4, 4), off=(0, 0, 0), img=B, d=(8, 8, 8): lib.vx_toy_embed(obj, i3(*od), i3(*off), 1.0, 0, 0, img, i3(*d), None)
    for k, (code, kw) in enumerate([(E_NULL, dict(obj=None)), (E_NULL, dict(img=None)), (E_SHAPE, dict(od=(4, 0, 4))),
                                    (E_SHAPE, dict(d=(0, 8, 8))), (E_SHAPE, dict(d=(1 << 20, 1 << 20, 4))),
                                    (E_ALIGN, dict(obj=A + 2)), (E_ALIGN, dict(img=B + 4))]):
        assert emb(**kw) == code, (k, lib.vx_last_error_string())
        assert lib.vx_last_error_string().startswith(b"vx_toy_embed")


def test_selection_segment_noise_refusals_without_a_gpu(lib):
    ks = lambda *v: (C.c_int64 * max(len(v), 1))(*v)
    need = int(lib.vx_order_stats_f64_workspace_bytes(3))
    assert need > 0 and need % 256 == 0 and lib.vx_order_stats_f64_workspace_bytes(0) == 0 == lib.vx_order_stats_f64_workspace_bytes(33)
    os_ = lambda x=A, n=100, k=(0, 50, 99), nk=None, out=B, st=W, ws=W + 256, nb=1 << 20: lib.vx_order_stats_f64(
        x, n, ks(*k) if k is not None else None, len(k) if nk is None else nk, out, st, ws, nb, None)
    cases = [(E_NULL, dict(x=None)), (E_NULL, dict(k=None, nk=2)), (E_NULL, dict(out=None)), (E_NULL, dict(st=None)), (E_NULL, dict(ws=None)),
             (E_SHAPE, dict(nk=0)), (E_SHAPE, dict(nk=33)), (E_SHAPE, dict(n=0)), (E_SHAPE, dict(n=(1 << 40) + 1)),
             (E_SHAPE, dict(k=(0, 100))), (E_SHAPE, dict(k=(-1,))),
             (E_ALIGN, dict(x=A + 4)), (E_ALIGN, dict(out=B + 4)), (E_ALIGN, dict(st=W + 2)), (E_ALIGN, dict(ws=W + 8)),
             (E_WORKSPACE, dict(nb=need - 1))]
    for k, (code, kw) in enumerate(cases):
        assert os_(**kw) == code, (k, lib.vx_last_error_string())
        assert lib.vx_last_error_string().startswith(b"vx_order_stats_f64")
    # the reads of the data: eight passes per sixteen distinct ranks among {k, k + 1}
    assert lib.vx_order_stats_f64_reads(100, ks(0, 50, 99), 3) == 8       # {0, 1, 50, 51, 99}
    assert lib.vx_order_stats_f64_reads(1000, ks(*range(0, 24, 3)), 8) == 8 and lib.vx_order_stats_f64_reads(1000, ks(*range(0, 27, 3)), 9) == 16
    assert lib.vx_order_stats_f64_reads(1000, ks(*range(0, 96, 3)), 32) == 32 and lib.vx_order_stats_f64_reads(10, ks(10), 1) == 0
    thr = (C.c_double * 3)(0.1, 0.2, 0.3)
    seg = lambda x=A, n=64, t=thr, R=3, out=B: lib.vx_toy_segment(x, n, t, R, out, None)
    for k, (code, kw) in enumerate([(E_NULL, dict(x=None)), (E_NULL, dict(t=None)), (E_NULL, dict(out=None)), (E_SHAPE, dict(R=0)),
                                    (E_SHAPE, dict(R=65)), (E_SHAPE, dict(n=0)), (E_ALIGN, dict(x=A + 4)), (E_ALIGN, dict(out=B + 2))]):
        assert seg(**kw) == code, (k, lib.vx_last_error_string())
    assert lib.vx_toy_noise(None, 8, 1, 0, 0.5, None) == E_NULL and lib.vx_toy_noise(A + 4, 8, 1, 0, 0.5, None) == E_ALIGN
    assert lib.vx_toy_noise(A, 1 << 32, 1, 0, 0.5, None) == E_SHAPE and lib.vx_toy_noise(A, -1, 1, 0, 0.5, None) == E_SHAPE
    assert lib.vx_toy_noise(A, 8, 1, 0, 1.5, None) == E_SHAPE and lib.vx_toy_noise(A, 8, 1, 0, float("nan"), None) == E_SHAPE
    assert lib.vx_toy_noise(None, 0, 1, 0, 0.5, None) == 0      # an empty image is a no-op
    assert lib.vx_count_ge_f64(None, 8, 0.1, B, None) == E_NULL and lib.vx_count_ge_f64(A, 8, 0.1, None, None) == E_NULL
    assert lib.vx_count_ge_f64(A, -1, 0.1, B, None) == E_SHAPE and lib.vx_count_ge_f64(A + 4, 8, 0.1, B, None) == E_ALIGN


# ---------------------------------------------------------------------------------------------
# the host plan under sanitizers: a stand-alone program, no sanitizer runtime in this process

def test_host_plan_under_asan_ubsan(lib, tmp_path):
    exe = str(tmp_path / "toy_plan_host")
    build_host_program(os.path.join(ROOT, "tests", "toy_plan_host.cpp"), exe)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "BAD-" not in res.stdout
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in res.stdout.splitlines()}
    assert rows["reflect"] == [0]            # n = 1 .. 5 against radius 0 .. 128, every index equals the walked extension
    codes = {k: v[0] for k, v in rows.items() if k != "reflect"}
    ok = {"e_inside", "e_clip_low", "e_clip_high", "e_outside", "b_256_a0", "b_256_a1", "b_256_a2", "b_r0", "b_r56", "b_r57", "b_r112",
          "b_r113", "b_r128", "b_r128_a2", "b_odd", "b_off16", "b_touch", "o_ok", "o_32", "o_n1"}
    want = {"e_null": E_NULL, "e_dim0": E_SHAPE, "e_huge": E_SHAPE, "e_align": E_ALIGN, "e_align_img": E_ALIGN,
            "b_r129": E_SHAPE, "b_rneg": E_SHAPE, "b_axis": E_SHAPE, "b_dim0": E_SHAPE, "b_null": E_NULL, "b_nullw": E_NULL,
            "b_align": E_ALIGN, "b_inplace": E_SHAPE, "b_overlap": E_SHAPE, "b_huge": E_SHAPE,
            "o_nk0": E_SHAPE, "o_nk33": E_SHAPE, "o_n0": E_SHAPE, "o_rank": E_SHAPE, "o_rank_neg": E_SHAPE, "o_null": E_NULL,
            "o_null_ks": E_NULL, "o_align": E_ALIGN, "o_ws_align": E_ALIGN, "o_ws_short": E_WORKSPACE}
    want.update({k: 0 for k in ok})
    assert codes == want
    # box clipping: [lo, hi) per axis in image coordinates; an object wholly outside leaves an empty range on that axis
    assert rows["e_inside"][1:] == [3, 8, 4, 10, 5, 12] and rows["e_clip_low"][1:] == [0, 3, 0, 7, 0, 1]
    assert rows["e_clip_high"][1:] == [15, 20, 0, 9, 19, 20]
    lo0, hi0, lo1, hi1 = rows["e_outside"][1:5]
    assert hi0 <= lo0 and hi1 <= lo1
    # blur tiles: [tw, ring rows, workgroups, LDS bytes, 16-byte path].  A thread produces 2 consecutive rows, so a step is
    # 16 / 32 / 64 rows for slabs of 64 / 32 / 16 columns.  The widest slab whose ring of 2 r + step rows fits 64 KB:
    # 64 columns up to radius 56, 32 up to 112, 16 beyond
    assert rows["b_256_a0"][1:] == [64, 80, 1024, 80 * 64 * 8, 1] and rows["b_256_a1"][1:] == [64, 80, 256 * 4, 80 * 64 * 8, 1]
    assert rows["b_256_a2"][3:] == [256 * 256 // 4 * 2, 4 * (128 + 64) * 8, 1]
    assert rows["b_r56"][1:3] == [64, 128] and rows["b_r57"][1:3] == [32, 2 * 57 + 32]
    assert rows["b_r112"][1:3] == [32, 256] and rows["b_r113"][1:3] == [16, 2 * 113 + 64] and rows["b_r128"][1:3] == [16, 320]
    assert rows["b_r57"][3] == -(-65 * 130 // 32) and rows["b_r128"][3] == 70 * -(-130 // 16)
    assert rows["b_odd"][5] == 0 and rows["b_off16"][5] == 0 and rows["b_r0"][2] == 16
    assert rows["b_r128_a2"][3:] == [3, 4 * (128 + 256) * 8, 0]
    # order statistics: [distinct ranks, reads, workspace bytes, then (k, k + 1) per rank; the last rank repeats itself]
    assert rows["o_ok"][1:] == [6, 8, lib.vx_order_stats_f64_workspace_bytes(5), 0, 1, 98, 99, 99, 99, 50, 51, 50, 51]
    assert rows["o_32"][1:3] == [64, 32] and rows["o_n1"][1:] == [1, 8, lib.vx_order_stats_f64_workspace_bytes(1), 0, 0]
