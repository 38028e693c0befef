"""CPU: the host half of reading a 2D results tree -- image_io.read_png over all five scanline filters and files of a
foreign encoder, read_tiff_f32 over strips / Deflate / byte orders and its refusals, the GTA hooks against the
reference's colour table, ExperimentDataloader on a PNG / TIFF tree, and the argument checks of the new entry points."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import png_build as pb
from tests.helpers import GOLDEN


def test_read_png_grid_every_filter_and_shape(tmp_path):
    p = tmp_path / "g.png"
    from values_amd.image_io import read_png
    n = 0
    for name, img, ft in pb.grid_cases():
        p.write_bytes(pb.png_bytes(img, ft, n_idat=1 + n % 3))
        got = read_png(p)
        want = pb.squeeze(img)
        assert got.dtype == np.uint8 and got.shape == want.shape, name
        assert np.array_equal(got, want), name
        n += 1
    assert n == 6 * 3 * 3 * 7


def test_read_png_refuses_what_it_does_not_decode(tmp_path):
    from values_amd.image_io import png_parse, read_png
    good = bytearray(pb.png_bytes(pb.content(4, 5, 3), pb.filters("sub", 4)))
    w, h, ctype, bpp, spans = png_parse(bytes(good))
    assert (w, h, ctype, bpp) == (5, 4, 2, 3) and len(spans) == 1
    for at, value in ((24, 16), (28, 1), (25, 3)):      # IHDR: bit depth 16, interlaced, palette
        bad = bytearray(good)
        bad[at] = value
        with pytest.raises(ValueError, match="8-bit non-interlaced"):
            png_parse(bytes(bad))
    with pytest.raises(ValueError, match="not a PNG"):
        png_parse(b"GIF89a" + bytes(20))
    img = pb.content(3, 4, 1)
    raw = bytearray(pb.scanlines(img, pb.filters("none", 3)))
    raw[5] = 5                                            # row 1's filter byte
    import struct
    import zlib
    f = (b"\x89PNG\r\n\x1a\n" + pb._chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 3, 8, 0, 0, 0, 0))
         + pb._chunk(b"IDAT", zlib.compress(bytes(raw))) + pb._chunk(b"IEND", b""))
    (tmp_path / "f.png").write_bytes(f)
    with pytest.raises(ValueError, match="filter type 5"):
        read_png(tmp_path / "f.png")


def test_read_png_foreign_encoder_fixtures():
    from values_amd.image_io import read_png
    d = os.path.join(GOLDEN, "images2d")
    for name, shape in (("rgb", (44, 37, 3)), ("grey", (44, 37)), ("rgba", (44, 37, 4))):
        want = np.load(os.path.join(d, f"pil_{name}.npy"))
        got = read_png(os.path.join(d, f"pil_{name}.png"))
        assert got.shape == shape and np.array_equal(got, want), name


def _map(h, w, seed=0):
    m = np.random.default_rng(seed).random((h, w), dtype=np.float32)
    m[h // 2:] = 0.25       # compressible
    return m


def test_read_tiff_strips_deflate_and_byte_orders(tmp_path):
    from values_amd.image_io import read_tiff_f32, write_tiff_f32
    m = _map(21, 13)
    p = tmp_path / "m.tif"
    for endian in "<>":
        for rps in (None, 1, 4, 8, 21, 64):
            for comp in (1, 8, 32946):
                for pred in (None, 1):
                    p.write_bytes(pb.tiff_bytes(m, endian, rps, comp, pred))
                    got = read_tiff_f32(p)
                    assert got.dtype == np.float32 and np.array_equal(got, m), (endian, rps, comp, pred)
    write_tiff_f32(p, m)
    assert np.array_equal(read_tiff_f32(p), m)


def test_read_tiff_refuses_lzw_and_the_float_predictor(tmp_path):
    from values_amd.image_io import read_tiff_f32
    m = _map(6, 5)
    p = tmp_path / "m.tif"
    p.write_bytes(pb.tiff_bytes(m, "<", None, 5))
    with pytest.raises(ValueError, match=r"Compression \(tag 259\) = 5 \(LZW\)"):
        read_tiff_f32(p)
    p.write_bytes(pb.tiff_bytes(m, "<", 2, 8, predictor=3))
    with pytest.raises(ValueError, match=r"Predictor \(tag 317\) = 3"):
        read_tiff_f32(p)
    p.write_bytes(pb.tiff_bytes(m, ">", None, 1, predictor=2))
    with pytest.raises(ValueError, match=r"Predictor \(tag 317\) = 2"):
        read_tiff_f32(p)


def _palette_image():
    """every colour of the fixture table, then two colours of no class"""
    with open(os.path.join(GOLDEN, "cityscapes_color2trainid.json")) as f:
        tab = json.load(f)
    cols = [r[:3] for r in tab["color2trainId"]] + [[1, 2, 3], [128, 64, 129]]
    ids = [r[3] for r in tab["color2trainId"]] + [tab["default"]] * 2
    assert tab["default"] == 128 and len(cols) == 37
    img = np.array(cols, dtype=np.uint8).reshape(1, -1, 3).repeat(3, axis=0)
    img = np.concatenate([img, img[:, ::-1]], axis=1)                 # (3, 74, 3)
    want = np.array(ids, dtype=np.int64).reshape(1, -1).repeat(3, axis=0)
    return tab, img, np.concatenate([want, want[:, ::-1]], axis=1)


def test_gta_hooks_agree_with_the_reference_table(tmp_path):
    from values_amd import gta
    from values_amd.image_io import write_png
    from values_amd.io import TARGET_MAP, instantiate
    tab, img, want = _palette_image()
    assert gta.COLOR2TRAINID == {tuple(r[:3]): r[3] for r in tab["color2trainId"]}
    assert {k: gta.NAME2TRAINID[k] for k in gta.LABEL_SWITCHES} == tab["name2trainId"] and gta.UNKNOWN == tab["default"]
    write_png(tmp_path / "m.png", img)
    got = gta.pred_seg_loading(tmp_path / "m.png")
    assert got.dtype == np.int64 and got.shape == (3, 74) and np.array_equal(got, want)
    for spelling in ("evaluation.utils.gta.pred_seg_loading", "utils.gta.pred_seg_loading"):
        assert TARGET_MAP[spelling] == "values_amd.gta.pred_seg_loading"
        assert np.array_equal(instantiate({"_target_": spelling}, pred_seg_path=tmp_path / "m.png"), want)
    for spelling in ("evaluation.utils.gta.gt_unc_map", "utils.gta.gt_unc_map"):
        assert TARGET_MAP[spelling] == "values_amd.gta.gt_unc_map"

    # gt_unc_map: variance 2/9 on the five switch classes, 0 elsewhere, float32, axes swapped
    label = np.arange(4 * 7).reshape(4, 7) % 25
    np.save(tmp_path / "lab.npy", label)

    class _DS:
        image_ids = ["a", "b"]
        masks = [None, str(tmp_path / "lab.npy")]

    class _DL:
        dataset = _DS()

    m = gta.gt_unc_map("b", _DL())
    assert m.dtype == np.float32 and m.shape == (7, 4)
    p = 1.0 / 3.0
    var = np.single((1 - p) * np.square(0 - p) + p * np.square(1 - p))
    want_m = np.where(np.isin(label, list(tab["name2trainId"].values())), var, np.single(0)).astype(np.float32)
    assert np.array_equal(m, want_m.T)


def _write_tree_host(save_dir, ids, pred_masks, mean_masks, unc):
    """the tree results2d.save_prediction / save_uncertainty write.  save_prediction colours the masks with a device
    kernel; here the same table (results2d._lut) is applied on the host and the files are written by the same writer
    under the names of results2d.plan_images."""
    from values_amd import results2d
    from values_amd.image_io import write_png
    os.makedirs(os.path.join(save_dir, "pred_seg"), exist_ok=True)
    lut = results2d._lut()
    for f in results2d.plan_images(ids, pred_masks.shape[1], []):
        b = f.source[1]
        mask = mean_masks[b] if f.source[0] == "mean" else pred_masks[b, f.source[2]]
        write_png(os.path.join(save_dir, f.path), lut[mask])
    for b, iid in enumerate(ids):
        results2d.save_uncertainty(save_dir, iid, {k: v[b] for k, v in unc.items()})


def test_host_dataloader_on_a_2d_tree(tmp_path):
    import torch
    from values_amd.experiment import ExperimentDataloader, ExperimentVersion, aggregate_uncertainties
    rng = np.random.default_rng(5)
    ids, T, H, W = ["img_a", "img_b", "img_c"], 2, 20, 33
    pm = rng.integers(0, 24, (3, T, H, W)).astype(np.uint8)
    mm = rng.integers(0, 24, (3, H, W)).astype(np.uint8)
    mm[0, :2] = 255                                               # unlabeled: black, train id 255
    unc = {k: torch.from_numpy(rng.random((3, H, W), dtype=np.float32)) for k in ("pred_entropy", "aleatoric_uncertainty")}
    ev = ExperimentVersion(base_path=tmp_path, naming_scheme_version="seed{seed}", pred_model="Dropout", image_ending=".png",
                           unc_ending=".tif", unc_types=["predictive_uncertainty", "aleatoric_uncertainty"], aggregations=None,
                           n_reference_segs=1, pred_seg_loading={"_target_": "evaluation.utils.gta.pred_seg_loading"}, seed=7)
    _write_tree_host(str(ev.exp_path / "val"), ids, pm, mm, unc)
    dl = ExperimentDataloader(ev, "val")
    assert dl.image_ids == ids
    for b, iid in enumerate(ids):
        for u, k in (("predictive_uncertainty", "pred_entropy"), ("aleatoric_uncertainty", "aleatoric_uncertainty")):
            got = dl.get_unc_map(iid, u)
            assert got.dtype == np.float32 and got.shape == (W, H)                 # the first two axes swapped
            assert np.array_equal(got, unc[k][b].numpy().T)
        mean = dl.get_mean_pred_seg(iid)                                           # through the hook: as the hook returns it
        assert mean.dtype == np.int64 and mean.shape == (H, W) and np.array_equal(mean, mm[b].astype(np.int64))
        segs = dl.get_pred_segs(iid)
        assert len(segs) == T + 1 and all(s.shape == (W, H, 3) for s in segs)
    aggs = {"mean": {"_target_": "tests.png_build.mean_and_max"}, "scaled": {"_target_": "tests.png_build.mean_and_max", "scale": 2.0}}
    aggregate_uncertainties(dl, aggs)
    for u, k in (("predictive_uncertainty", "pred_entropy"), ("aleatoric_uncertainty", "aleatoric_uncertainty")):
        want = {f"{iid}.tif": {"mean": pb.mean_and_max(unc[k][b].numpy().T), "scaled": pb.mean_and_max(unc[k][b].numpy().T, scale=2.0)}
                for b, iid in enumerate(ids)}
        with open(dl.dataset_path / f"aggregated_{u}.json") as f:
            assert f.read() == json.dumps(want, indent=4)

    # a Softmax model's 2D tree: pred_entropy is written as .tif and read back in the same orientation
    from values_amd.experiment import _load_file, _save_file
    m = rng.random((W, H), dtype=np.float32)
    _save_file(m, tmp_path / "e.tif")
    assert np.array_equal(_load_file(tmp_path / "e.tif"), m)
    with pytest.raises(ValueError, match="not a results file"):
        _load_file(tmp_path / "e.jpg")


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    from values_amd import _lib
    lib = _lib.load()
    assert lib.vx_version() >= 730
    dummy = 0x10000                      # never dereferenced: every call below is refused by a host-side check

    def item(h=4, w=4, bpp=3, src=dummy, dst=dummy):
        arr = (_lib.PngUnfilterItem * 1)()
        arr[0].src, arr[0].src_n, arr[0].dst, arr[0].H, arr[0].W, arr[0].bpp = src, h * (1 + w * bpp), dst, h, w, bpp
        return arr
    ws = lib.vx_png_unfilter_workspace_bytes(1)
    assert ws >= 256 and lib.vx_png_unfilter_workspace_bytes(-1) == -1
    assert lib.vx_png_unfilter(None, 0, None, None, 0, None) == 0
    assert lib.vx_png_unfilter(None, 1, dummy, dummy, ws, None) == -1            # null table: VX_E_NULL
    assert lib.vx_png_unfilter(item(), 1, None, dummy, ws, None) == -1           # null statuses
    assert lib.vx_png_unfilter(item(), 1, dummy, None, ws, None) == -1           # null workspace
    assert lib.vx_png_unfilter(item(src=None), 1, dummy, dummy, ws, None) == -1  # null source
    assert lib.vx_png_unfilter(item(), 1, dummy, dummy, ws - 1, None) == -4      # VX_E_WORKSPACE
    assert lib.vx_png_unfilter(item(bpp=2), 1, dummy, dummy, ws, None) == -3     # VX_E_DTYPE
    assert b"bpp 2" in lib.vx_last_error_string()
    assert lib.vx_png_unfilter(item(w=65537, bpp=1), 1, dummy, dummy, ws, None) == -2    # a row over 64 KiB: VX_E_SHAPE
    assert lib.vx_png_unfilter(item(w=16385, bpp=4), 1, dummy, dummy, ws, None) == -2
    assert lib.vx_png_unfilter(item(h=0), 1, dummy, dummy, ws, None) == -2
    assert lib.vx_png_unfilter(item(h=1 << 20, w=16384, bpp=4), 1, dummy, dummy, ws, None) == -2   # H (W bpp + 1) >= 2^31
    assert lib.vx_rgb_to_trainid(None, 0, None, 0, 128, None, None) == 0
    assert lib.vx_rgb_to_trainid(dummy, 8, None, 4, 128, dummy, None) == -1      # null table
    assert lib.vx_rgb_to_trainid(None, 8, dummy, 4, 128, dummy, None) == -1
    assert lib.vx_rgb_to_trainid(dummy, 8, dummy, 257, 128, dummy, None) == -2   # more than 256 pairs
    assert lib.vx_rgb_to_trainid(dummy, 8, dummy, 4, 256, dummy, None) == -3
    assert lib.vx_rgb_to_trainid(dummy, -1, dummy, 4, 128, dummy, None) == -2
    assert C.sizeof(_lib.PngUnfilterItem) == 40
