"""CPU: the host mirror of the GTA / Cityscapes 2D preprocessing (values_amd.preprocess2d) against an independent
restatement of OpenCV's fixed-point resize (tests/prep2d_ref.py) and against the reference's label loops restated
literally over the golden tables; palette PNG files; the data-set driver on two tiny trees; the host plan of
vx_crop_resize_batched under the sanitizers.  Every comparison is on integers and exact."""
import io
import json
import os
import subprocess

import numpy as np
import pytest

from tests import png_build, prep2d_ref, prep2d_trees
from tests.helpers import GOLDEN, build_host_program
from values_amd import gta, image_io
from values_amd import preprocess2d as p2d
from values_amd.preprocess import npy_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_DTYPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5
SHAPES = ((8, 16), (13, 22), (9, 17), (6, 6), (7, 5), (12, 18), (3, 11), (24, 30))


@pytest.fixture(scope="module")
def tables():
    with open(os.path.join(GOLDEN, "cityscapes_id_tables.json")) as f:
        t = json.load(f)
    return {k: v for k, v in t["id2trainId"]}, {k: tuple(v) for k, v in t["trainId2color"]}


def _images(h, w):
    rng = np.random.default_rng(100 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    yield "random", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yield "random grey", rng.integers(0, 256, (h, w), dtype=np.uint8)
    yield "all 255", np.full((h, w, 3), 255, np.uint8)
    yield "all 0", np.zeros((h, w, 3), np.uint8)
    yield "checkerboard", (((yy + xx) % 2) * 255).astype(np.uint8)              # sums of 510 + 2: the rounding term
    yield "checkerboard of pairs", ((((yy // 2) + xx) % 2) * 255).astype(np.uint8)
    yield "three of four", np.where((yy + 2 * xx) % 4 == 0, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("factor", [2, 4, 6])
def test_resize_linear_is_opencvs_fixed_point(factor):
    seen_rounding = False
    for h, w in SHAPES:
        if prep2d_ref.out_size(h, factor) < 1 or prep2d_ref.out_size(w, factor) < 1:
            continue
        for name, img in _images(h, w):
            got, want = p2d.resize_linear_u8(img, factor), prep2d_ref.resize_linear_fixed(img, factor)
            assert got.dtype == np.uint8 and got.shape == want.shape, (h, w, name)
            assert got.shape[:2] == (p2d.out_size(h, factor), p2d.out_size(w, factor))
            np.testing.assert_array_equal(got, want, err_msg=f"{h}x{w} {name} factor {factor}")
            seen_rounding |= bool(np.isin(got, (64, 128, 191)).any())           # (255 + 2) >> 2, (510 + 2) >> 2, (765 + 2) >> 2
    assert seen_rounding


@pytest.mark.parametrize("factor", [2, 4, 6])
def test_resize_nearest_is_opencvs(factor):
    for h, w in SHAPES:
        if prep2d_ref.out_size(h, factor) < 1 or prep2d_ref.out_size(w, factor) < 1:
            continue
        for name, img in _images(h, w):
            got = p2d.resize_nearest(img, factor)
            assert got.dtype == img.dtype
            np.testing.assert_array_equal(got, prep2d_ref.resize_nearest_ref(img, factor), err_msg=f"{h}x{w} {name}")


def test_out_size_rounds_half_to_even_and_refuses_odd_factors():
    assert [p2d.out_size(s, 4) for s in (1024, 1912, 8, 16, 6, 10, 2, 1, 14)] == [256, 478, 2, 4, 2, 2, 0, 0, 4]
    for k in (2, 4, 6, 8):
        for s in range(1, 70):
            assert p2d.out_size(s, k) == prep2d_ref.out_size(s, k)
    for k in (0, -2, 3, 5):
        with pytest.raises(ValueError):
            p2d.out_size(8, k)
        with pytest.raises(ValueError):
            p2d.resize_linear_u8(np.zeros((8, 8), np.uint8), k)


def test_center_crop_box():
    assert p2d.center_crop_box(1024, 2048) == (0, 68, 1024, 1912)
    assert p2d.center_crop_box(1052, 1914) == (14, 1, 1024, 1912)
    assert p2d.center_crop_box(1024, 1912) == (0, 0, 1024, 1912)
    assert p2d.center_crop_box(13, 22, (8, 16)) == (2, 3, 8, 16)
    for h, w in ((1023, 1912), (1024, 1911), (720, 1280)):
        with pytest.raises(ValueError):
            p2d.center_crop_box(h, w)


def test_label_tables_are_the_references_loops(tables):
    id2trainid, trainid2color = tables
    every = np.arange(256, dtype=np.uint8).reshape(16, 16)
    # preprocess_gta_cityscapes.py:147-154, literally
    mask_train_indices = every.copy()
    for k, v in id2trainid.items():
        mask_train_indices[every == k] = v
    mask_color = np.zeros((*mask_train_indices.shape, 3), dtype=np.uint8)
    for k, v in trainid2color.items():
        mask_color[mask_train_indices == k] = np.array(v)
    got_ids = p2d.id_to_trainid_lut()[every]
    np.testing.assert_array_equal(got_ids, mask_train_indices)
    np.testing.assert_array_equal(p2d.trainid_to_color_lut()[got_ids], mask_color)
    assert got_ids.dtype == np.uint8 and got_ids[2, 8] == 40 and got_ids[0, 7] == 0       # id 40 keeps its value
    # and through preprocess_image: a (16, 32) mask of every id twice, crop = the image, factor 2 reads the even columns
    wide = np.repeat(every, 2, axis=1).repeat(2, axis=0)
    image = np.zeros(wide.shape + (3,), np.uint8)
    _, ids, colour = p2d.preprocess_image(image, wide, "cityscapes", crop=wide.shape, factor=2)
    np.testing.assert_array_equal(ids, mask_train_indices)
    np.testing.assert_array_equal(colour, mask_color)


def test_gta_labels_are_int64_and_an_unknown_colour_asserts():
    with open(os.path.join(GOLDEN, "cityscapes_color2trainid.json")) as f:
        color2trainid = {tuple(r[:3]): r[3] for r in json.load(f)["color2trainId"]}
    idx, colour = prep2d_trees.label_colours(13, 22, 5)
    image = prep2d_trees.rgb_image(13, 22, 6)
    img, ids, mask_color = p2d.preprocess_image(image, colour, "gta", (8, 16), 4, "x.png")
    want_color = colour[2:10, 3:19][::4, ::4]
    want = np.apply_along_axis(lambda x: color2trainid.get(tuple(x), 128), axis=-1, arr=want_color)   # :167-171
    assert ids.dtype == np.int64 == want.dtype and ids.shape == (2, 4)
    np.testing.assert_array_equal(ids, want)
    np.testing.assert_array_equal(mask_color, want_color)
    np.testing.assert_array_equal(img, prep2d_ref.resize_linear_fixed(image[2:10, 3:19], 4))
    rgba = np.concatenate([colour, np.full((13, 22, 1), 9, np.uint8)], -1)                  # alpha is dropped
    np.testing.assert_array_equal(p2d.preprocess_image(image, rgba, "gta", (8, 16), 4)[1], want)
    bad = colour.copy()
    bad[6, 11] = (1, 2, 3)                                                                   # on the nearest grid
    with pytest.raises(AssertionError, match="Unknown color value in mask for image x.png!"):
        p2d.preprocess_image(image, bad, "gta", (8, 16), 4, "x.png")
    bad = colour.copy()
    bad[7, 11] = (1, 2, 3)                                                                   # off the grid: never read
    p2d.preprocess_image(image, bad, "gta", (8, 16), 4, "x.png")


def test_palette_png_files(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    full = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    short = full[:7]
    for pal, top, tag in ((full, 256, "full"), (short, 7, "short")):
        idx = rng.integers(0, top, (11, 19)).astype(np.uint8)
        # PIL's own writer
        im = Image.fromarray(idx, "P")
        im.putpalette(pal.tobytes())
        path = tmp_path / f"pil_{tag}.png"
        im.save(path, bits=8)             # (PIL would pack a short palette's indices into fewer bits)
        raw = path.read_bytes()
        w, h, palette, spans = image_io.png_parse_indexed(raw)
        assert (w, h) == (19, 11) and palette.shape == (256, 3) and palette.dtype == np.uint8 and spans
        np.testing.assert_array_equal(palette[:top], pal[:top])
        got = image_io.read_png_any(path)
        assert got.shape == (11, 19, 3) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, pal[idx])
        np.testing.assert_array_equal(got, np.asarray(Image.open(path).convert("RGB")))
        with pytest.raises(ValueError, match="only 8-bit non-interlaced grey/RGB/RGBA"):
            image_io.png_parse(raw)
        with pytest.raises(ValueError, match="only 8-bit non-interlaced grey/RGB/RGBA"):
            image_io.read_png(path)
        # all five filters, several IDAT chunks
        for pat in png_build.PATTERNS:
            raw = prep2d_trees.indexed_png_bytes(idx, pal, png_build.filters(pat, 11), n_idat=3)
            path = tmp_path / f"{tag}_{pat}.png"
            path.write_bytes(raw)
            w, h, palette, spans = image_io.png_parse_indexed(raw)
            assert (w, h, len(spans)) == (19, 11, 3)
            assert not palette[top:].any()                                                   # padded with black
            np.testing.assert_array_equal(image_io.read_png_any(path), pal[idx], err_msg=f"{tag} {pat}")
            np.testing.assert_array_equal(np.asarray(Image.open(path).convert("RGB")), pal[idx])
            with pytest.raises(ValueError):
                image_io.png_parse(raw)
    # read_png_any is read_png for everything else; png_parse_indexed refuses what is no palette file
    rgb = prep2d_trees.rgb_image(5, 6, 1)
    image_io.write_png(tmp_path / "rgb.png", rgb)
    np.testing.assert_array_equal(image_io.read_png_any(tmp_path / "rgb.png"), rgb)
    image_io.write_png(tmp_path / "grey.png", rgb[..., 0])
    np.testing.assert_array_equal(image_io.read_png_any(tmp_path / "grey.png"), rgb[..., 0])
    with pytest.raises(ValueError):
        image_io.png_parse_indexed((tmp_path / "rgb.png").read_bytes())
    with pytest.raises(ValueError):
        image_io.png_parse_indexed(b"not a png")
    no_plte = prep2d_trees.indexed_png_bytes(np.zeros((2, 2), np.uint8), full, [0, 0]).replace(b"PLTE", b"pLTE")
    with pytest.raises(ValueError, match="PLTE"):
        image_io.png_parse_indexed(no_plte)


def check_tree(out, cases, dataset):
    """the four files of every case against the mirror's arrays; -> the relative paths of all files"""
    from PIL import Image
    root = os.path.join(str(out), "preprocessed")
    for image_id, (image, label) in cases.items():
        want_image, want_ids, want_color = p2d.preprocess_image(image, label, dataset, prep2d_trees.CROP, prep2d_trees.FACTOR)
        np.testing.assert_array_equal(want_image, prep2d_ref.resize_linear_fixed(
            image[slice(*_box(image)[0]), slice(*_box(image)[1])], prep2d_trees.FACTOR))
        for sub, want, dtype in (("images", want_image, np.uint8), ("labels", want_ids, np.uint8 if dataset == "cityscapes" else np.int64)):
            path = os.path.join(root, sub, f"{image_id}.npy")
            got = np.load(path)
            assert got.dtype == dtype and got.shape == want.shape and got.flags.c_contiguous, path
            np.testing.assert_array_equal(got, want, err_msg=path)
            with open(path, "rb") as f:
                raw = f.read()
            head = npy_header(want.shape, dtype)
            assert raw[:len(head)] == head and raw[len(head):] == want.tobytes(), path
            buf = io.BytesIO()
            np.save(buf, want)
            assert raw == buf.getvalue(), path
        assert want_image.shape == (2, 4, 3) and want_ids.shape == (2, 4)
        for sub, want in (("images", want_image), ("labels", want_color)):
            path = os.path.join(root, sub, "vis", f"{image_id}.png")
            im = Image.open(path)
            assert im.mode == "RGB"
            np.testing.assert_array_equal(np.asarray(im), want, err_msg=path)
            np.testing.assert_array_equal(image_io.read_png(path), want, err_msg=path)
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _box(image):
    y0, x0, ch, cw = p2d.center_crop_box(image.shape[0], image.shape[1], prep2d_trees.CROP)
    return (y0, y0 + ch), (x0, x0 + cw)


def expected_files(cases, done=()):
    ids = sorted(list(cases) + list(done))
    return sorted([os.path.join(s, f"{i}.npy") for s in ("images", "labels") for i in ids]
                  + [os.path.join(s, "vis", f"{i}.png") for s in ("images", "labels") for i in ids])


def finished_case(out, image_id):
    """the four outputs of a case that is already done, with a content no writer would produce"""
    root = os.path.join(str(out), "preprocessed")
    for path in p2d._out_paths(root, image_id):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(b"finished earlier")


def untouched(out, image_id):
    root = os.path.join(str(out), "preprocessed")
    return all(open(path, "rb").read() == b"finished earlier" for path in p2d._out_paths(root, image_id))


def test_dataset_cityscapes_host(tmp_path, capsys):
    cases = prep2d_trees.cityscapes_tree(tmp_path / "raw")
    done = "zurich_000001_000019"
    finished_case(tmp_path / "out", done)                   # skip rule: all four outputs exist
    n = p2d.preprocess_dataset_2d(tmp_path / "raw", tmp_path / "out", "cityscapes", crop=prep2d_trees.CROP, factor=prep2d_trees.FACTOR)
    assert n == 1                                           # the case whose label has another resolution
    assert "Different resolutions between image and mask for aachen_000009_000019_leftImg8bit.png!" in capsys.readouterr().out
    todo = {k: v for k, v in cases.items() if k != done}
    assert check_tree(tmp_path / "out", todo, "cityscapes") == expected_files(todo, [done])
    assert untouched(tmp_path / "out", done)
    # three of the four outputs do not make a case finished
    os.remove(p2d._out_paths(os.path.join(str(tmp_path / "out"), "preprocessed"), done)[3])
    assert p2d.preprocess_dataset_2d(tmp_path / "raw", tmp_path / "out", "cityscapes", crop=prep2d_trees.CROP, factor=prep2d_trees.FACTOR) == 1
    assert check_tree(tmp_path / "out", cases, "cityscapes") == expected_files(cases)


def test_dataset_gta_host(tmp_path, capsys):
    cases = prep2d_trees.gta_tree(tmp_path / "raw")
    n = p2d.preprocess_dataset_2d(tmp_path / "raw", tmp_path / "out", "gta", crop=prep2d_trees.CROP, factor=prep2d_trees.FACTOR)
    assert n == 1 and "Different resolutions between image and mask for 00003.png!" in capsys.readouterr().out
    assert check_tree(tmp_path / "out", cases, "gta") == expected_files(cases)      # no 15188, no 17705, no 00003
    before = {f: os.stat(os.path.join(tmp_path, "out", "preprocessed", f)).st_mtime_ns for f in expected_files(cases)}
    assert p2d.preprocess_dataset_2d(tmp_path / "raw", tmp_path / "out", "gta", crop=prep2d_trees.CROP, factor=prep2d_trees.FACTOR) == 1
    assert before == {f: os.stat(os.path.join(tmp_path, "out", "preprocessed", f)).st_mtime_ns for f in expected_files(cases)}


def test_dataset_gta_unknown_colour_and_small_image(tmp_path):
    prep2d_trees.gta_tree(tmp_path / "raw", unknown=True)
    with pytest.raises(AssertionError, match="Unknown color value in mask for image 00001.png!"):
        p2d.preprocess_dataset_2d(tmp_path / "raw", tmp_path / "out", "gta", crop=prep2d_trees.CROP, factor=prep2d_trees.FACTOR)
    with pytest.raises(ValueError):                        # the sources are smaller than the contract's crop
        p2d.preprocess_dataset_2d(tmp_path / "raw", tmp_path / "out2", "gta")
    with pytest.raises(ValueError):
        p2d.preprocess_dataset_2d(tmp_path / "raw", tmp_path / "out3", "gta", crop=prep2d_trees.CROP, factor=3)
    with pytest.raises(ValueError):
        p2d.preprocess_dataset_2d(tmp_path / "raw", tmp_path / "out3", "gta", batch=0)


def test_device_route_fails_loudly_without_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from values_amd import _lib, preprocess_dataset_2d, preprocess_images_device
    prep2d_trees.gta_tree(tmp_path / "raw")
    with pytest.raises(_lib.VxError):
        preprocess_dataset_2d(tmp_path / "raw", tmp_path / "out", "gta", device_io=True, crop=prep2d_trees.CROP)
    with pytest.raises(_lib.VxError):
        preprocess_images_device(["a.png"], ["b.png"], "gta")


# ---------------------------------------------------------------------------------------------
# the C entry points' refusals need no device: they happen before any device call

def test_refusals_without_a_device():
    import ctypes as C
    from values_amd import _lib
    lib = _lib.load()
    assert lib.vx_version() >= 900
    assert [lib.vx_p2d_out_size(s, 4) for s in (1024, 1912, 6, 10, 1, 0)] == [256, 478, 2, 2, 0, 0]
    assert lib.vx_p2d_out_size(8, 3) == 0 and lib.vx_p2d_out_size(8, -2) == 0
    dummy = 0x10000                      # never dereferenced: every call below is refused by a host-side check
    t = _lib.P2dTables()
    t.id2trainid = t.trainid2color = t.color2trainid = dummy
    t.n_color, t.default_id = 35, 128

    def item(mode=_lib.VX_P2D_IMAGE, bpp=3, pal=None, H=13, W=22, y0=2, x0=3, ch=8, cw=16, k=4):
        a = (_lib.P2dItem * 1)()
        a[0].src, a[0].palette, a[0].out_rgb, a[0].out_ids = dummy, pal, dummy, dummy
        a[0].H, a[0].W, a[0].bpp, a[0].y0, a[0].x0, a[0].crop_h, a[0].crop_w, a[0].factor, a[0].mode = H, W, bpp, y0, x0, ch, cw, k, mode
        return a
    call = lambda a, tab=t, status=dummy, ws=dummy, n=1: lib.vx_crop_resize_batched(a, n, C.byref(tab) if tab is not None else None, status, ws, 1 << 20, None)
    assert lib.vx_crop_resize_batched(None, 0, None, None, None, 0, None) == 0              # an empty batch is a no-op
    assert lib.vx_crop_resize_batched_workspace_bytes(item(), 1, C.byref(t)) == 256
    for a, code in ((item(x0=7), E_SHAPE), (item(y0=6), E_SHAPE), (item(y0=-1), E_SHAPE), (item(k=3), E_SHAPE), (item(k=0), E_SHAPE),
                    (item(k=-4), E_SHAPE), (item(ch=1), E_SHAPE), (item(H=1 << 15, W=1 << 14, bpp=4), E_SHAPE),
                    (item(bpp=2), E_DTYPE), (item(bpp=3, pal=dummy), E_DTYPE), (item(mode=_lib.VX_P2D_LABEL_COLOR, bpp=1), E_DTYPE),
                    (item(mode=_lib.VX_P2D_LABEL_IDS, bpp=3), E_DTYPE), (item(mode=5), E_DTYPE)):
        assert call(a) == code, lib.vx_last_error_string()
        assert lib.vx_crop_resize_batched_workspace_bytes(a, 1, C.byref(t)) == 0
    assert call(None) == E_NULL and call(item(), status=None) == E_NULL and call(item(), ws=None) == E_NULL
    assert call(item(mode=_lib.VX_P2D_LABEL_IDS, bpp=1), tab=None) == E_NULL
    a = item()
    a[0].src = None
    assert call(a) == E_NULL
    assert call(item(), ws=dummy + 8) == E_ALIGN
    assert lib.vx_crop_resize_batched(item(), 1, C.byref(t), dummy, dummy, 8, None) == E_WORKSPACE
    # the RGB PNG encoder: vx_png_encode's refusals
    r = (_lib.PngRgbItem * 1)()
    r[0].rgb, r[0].H, r[0].W = dummy, 4, 5
    assert lib.vx_png_encode_rgb_workspace_bytes(r, 1) == lib.vx_png_workspace_bytes((_lib.PngItem * 1)(_lib.PngItem(dummy, None, 4, 5)), 1) > 0
    assert lib.vx_png_encode_rgb(r, 0, dummy, 1 << 20, dummy, dummy, dummy, 1 << 30, None) == E_SHAPE
    assert lib.vx_png_encode_rgb(r, 1, None, 1 << 20, dummy, dummy, dummy, 1 << 30, None) == E_NULL
    assert lib.vx_png_encode_rgb(r, 1, dummy, 10, dummy, dummy, dummy, 1 << 30, None) == E_SHAPE      # dst below vx_png_bound
    assert lib.vx_png_encode_rgb(r, 1, dummy, 1 << 20, dummy, dummy, dummy, 16, None) == E_WORKSPACE
    r[0].rgb = None
    assert lib.vx_png_encode_rgb(r, 1, dummy, 1 << 20, dummy, dummy, dummy, 1 << 30, None) == E_NULL
    r[0].rgb, r[0].H = dummy, 0
    assert lib.vx_png_encode_rgb(r, 1, dummy, 1 << 20, dummy, dummy, dummy, 1 << 30, None) == E_SHAPE
    assert lib.vx_png_encode_rgb_workspace_bytes(r, 1) == 0


# ---------------------------------------------------------------------------------------------
# the host plan under sanitizers: a stand-alone program, no sanitizer runtime in this process

def test_host_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "prep2d_plan_host")
    build_host_program(os.path.join(ROOT, "tests", "prep2d_plan_host.cpp"), exe)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "BAD-BLOCKS" not in res.stdout and "NO-MESSAGE" not in res.stdout
    lines = [ln.split() for ln in res.stdout.splitlines()]
    sizes = [(int(a), int(b), int(c)) for tag, a, b, c in lines if tag == "size"]
    assert len(sizes) == 49
    for size, k, out in sizes:
        ok = size >= 1 and k >= 1 and k % 2 == 0
        assert out == (prep2d_ref.out_size(size, k) if ok else 0), (size, k, out)
    rows = {ln[0]: [int(v) for v in ln[1:]] for ln in lines if ln[0] != "size"}
    codes = {k: v[0] for k, v in rows.items()}
    assert codes == {
        "empty": 0, "null": E_NULL, "count": E_SHAPE, "negative": E_SHAPE, "one_image": 0, "one_ids": 0, "one_color": 0,
        "contract": 0, "mixed": 0, "many": 0, "bpp": E_DTYPE, "mode": E_DTYPE, "pal_bpp3": E_DTYPE, "color_grey": E_DTYPE,
        "image_grey": E_DTYPE, "ids_rgb": E_DTYPE, "ids_pal": E_DTYPE, "dim0": E_SHAPE, "huge": E_SHAPE, "below_huge": 0,
        "odd": E_SHAPE, "factor0": E_SHAPE, "factor_neg": E_SHAPE, "crop_right": E_SHAPE, "crop_below": E_SHAPE,
        "crop_neg": E_SHAPE, "crop_empty": E_SHAPE, "crop_wrap": E_SHAPE, "out0": E_SHAPE, "null_src": E_NULL,
        "null_rgb": E_NULL, "image_no_ids": 0, "null_ids": E_NULL, "null_tables": E_NULL, "null_id_table": E_NULL,
        "null_colour_table": E_NULL, "null_lookup": E_NULL, "lookup_unused": 0, "n_color": E_SHAPE, "default_id": E_DTYPE,
        "ids_align": E_ALIGN}
    blk = lambda oh, ow: -(-(oh * ow) // 2048)              # 2048 output pixels per work block, counted per item
    assert rows["one_image"][1:] == [1, 256] and rows["contract"][1] == blk(256, 478) == 60
    assert rows["one_color"][1] == blk(4, 8)
    assert rows["mixed"][1] == blk(2, 4) + blk(256, 478) + blk(30, 101) + blk(4, 8) + blk(2, 2) and blk(30, 101) == 2
    assert 2048 % 101 != 0                                  # ... and the block boundary lies inside a row
    assert rows["many"][1] == 4096 and rows["many"][2] % 256 == 0 and rows["many"][2] >= 4096 * (4 * 8 + 8 + 13 * 4)
