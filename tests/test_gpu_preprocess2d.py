"""GPU: vx_crop_resize_batched (preprocess2d.hip) in its three modes against the host mirror, vx_png_encode_rgb, and
the device route of the GTA / Cityscapes 2D preprocessing against the host route on the trees of the CPU test.  Every
comparison is on integers and exact."""
import ctypes as C
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from tests import prep2d_trees, writer_trees
from tests.test_preprocess2d_cpu import check_tree, expected_files, finished_case, untouched

pytestmark = pytest.mark.gpu

E_NULL, E_SHAPE, E_DTYPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5
SENTINEL = 0xA5
IMG, IDS, COL = 0, 1, 2


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


class Spec:
    """one item: the source array ((H, W) or (H, W, 3 | 4) uint8), an optional (256, 3) palette, the crop box, factor, mode;
    src_off / rgb_off / ids_off: byte offsets that take the pointers off their natural alignment"""

    def __init__(self, src, mode, box, k=4, pal=None, src_off=0, rgb_off=0, ids_off=0):
        self.src, self.mode, self.box, self.k, self.pal = np.ascontiguousarray(src), mode, box, k, pal
        self.src_off, self.rgb_off, self.ids_off = src_off, rgb_off, ids_off

    def want(self):
        """the mirror: -> (rgb, ids or None)"""
        from values_amd import gta
        from values_amd import preprocess2d as p2d
        y0, x0, ch, cw = self.box
        a = self.src[y0:y0 + ch, x0:x0 + cw]
        if self.mode == IDS:
            ids = p2d.id_to_trainid_lut()[p2d.resize_nearest(a, self.k)]
            return p2d.trainid_to_color_lut()[ids], ids
        a = self.pal[a] if self.pal is not None else a[..., :3]
        if self.mode == IMG:
            return p2d.resize_linear_u8(a, self.k), None
        rgb = p2d.resize_nearest(a, self.k)
        return rgb, gta.rgb_to_trainid_host(rgb)


def run(specs, dev, tables=True):
    """one vx_crop_resize_batched call -> (rc, [(rgb bytes, ids bytes)], status list); the outputs are pre-filled with a
    sentinel and carry 64 bytes of margin on both sides, which must come back untouched"""
    import torch
    from values_amd import _lib
    from values_amd import preprocess2d as p2d
    lib = _lib.load()
    n = len(specs)
    arr = (_lib.P2dItem * n)()
    keep, outs = [], []
    for it, s in zip(arr, specs):
        src = torch.empty(s.src.size + s.src_off, dtype=torch.uint8, device=dev)
        src[s.src_off:] = torch.from_numpy(s.src.reshape(-1)).to(dev)
        pal = torch.from_numpy(np.ascontiguousarray(s.pal)).to(dev) if s.pal is not None else None
        oh, ow = max(lib.vx_p2d_out_size(s.box[2], s.k), 1), max(lib.vx_p2d_out_size(s.box[3], s.k), 1)
        nid = oh * ow * (8 if s.mode == COL else 1)
        rgb = torch.full((128 + 3 * oh * ow + s.rgb_off,), SENTINEL, dtype=torch.uint8, device=dev)
        ids = torch.full((128 + nid + s.ids_off,), SENTINEL, dtype=torch.uint8, device=dev)
        it.src, it.palette = src.data_ptr() + s.src_off, (pal.data_ptr() if pal is not None else None)
        it.H, it.W, it.bpp = s.src.shape[0], s.src.shape[1], (1 if s.src.ndim == 2 else s.src.shape[2])
        it.y0, it.x0, it.crop_h, it.crop_w, it.factor, it.mode = *s.box, s.k, s.mode
        it.out_rgb, it.out_ids = rgb.data_ptr() + 64 + s.rgb_off, ids.data_ptr() + 64 + s.ids_off
        keep.append((src, pal))
        outs.append((rgb, ids, 3 * oh * ow, nid, s))
    status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    t = p2d._device_tables(dev) if tables else None
    need = int(lib.vx_crop_resize_batched_workspace_bytes(arr, n, t))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    rc = lib.vx_crop_resize_batched(arr, n, t, status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    res = []
    for rgb, ids, nrgb, nid, s in outs:
        r, i = rgb.cpu().numpy(), ids.cpu().numpy()
        for buf, a, b in ((r, 64 + s.rgb_off, nrgb), (i, 64 + s.ids_off, nid)):
            assert (buf[:a] == SENTINEL).all() and (buf[a + b:] == SENTINEL).all(), "a write outside the output"
        res.append((r[64 + s.rgb_off:64 + s.rgb_off + nrgb].tobytes(), i[64 + s.ids_off:64 + s.ids_off + nid].tobytes()))
    return rc, res, status.cpu().tolist()


def check(specs, dev):
    rc, res, status = run(specs, dev)
    assert rc == 0
    for k, (s, (rgb, ids)) in enumerate(zip(specs, res)):
        want_rgb, want_ids = s.want()
        assert want_rgb.dtype == np.uint8 and rgb == np.ascontiguousarray(want_rgb).tobytes(), f"item {k}: rgb"
        if s.mode == IMG:
            assert ids == bytes([SENTINEL]) * len(ids)
            assert status[k] == 0
        else:
            assert want_ids.dtype == (np.int64 if s.mode == COL else np.uint8)
            assert ids == np.ascontiguousarray(want_ids).tobytes(), f"item {k}: ids"
            assert status[k] == (int(np.count_nonzero(want_ids == 128)) if s.mode == COL else 0)
    return res, status


def rgb(h, w, seed, c=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def colours(h, w, seed, c=3):
    a = prep2d_trees.label_colours(h, w, seed)[1]
    return a if c == 3 else np.concatenate([a, rgb(h, w, seed, 1)], -1)


def palette(seed=9):
    """the known colours in a shuffled 256-entry palette whose other entries are unknown colours"""
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    known = rng.permutation(256)[:len(prep2d_trees.COLOURS)]
    pal[known] = prep2d_trees.COLOURS
    return pal, known


def small_specs():
    """13 x 22 with the crop (8, 16) at the odd offsets (2, 3): every mode, bpp and factor"""
    box = (2, 3, 8, 16)
    pal, known = palette()
    idx = np.random.default_rng(1).choice(known, (13, 22)).astype(np.uint8)
    specs = []
    for k in (2, 4):
        specs += [Spec(rgb(13, 22, 2), IMG, box, k), Spec(rgb(13, 22, 3, 4), IMG, box, k), Spec(idx, IMG, box, k, pal),
                  Spec(prep2d_trees.label_ids(13, 22, 4), IDS, box, k),
                  Spec(colours(13, 22, 5), COL, box, k), Spec(colours(13, 22, 6, 4), COL, box, k), Spec(idx, COL, box, k, pal)]
    return specs


def test_small_shapes_every_mode_bpp_and_factor(dev):
    check(small_specs(), dev)


def test_clamped_taps_and_sizes_that_are_no_multiple_of_the_factor(dev):
    # 6 / 4 = 1.5 and 9 / 6 = 1.5 round to 2: the second tap of the last row / column is clamped to the CROP's edge, and
    # the pixels beyond the crop differ from it
    specs = []
    for mode, src in ((IMG, rgb(9, 9, 11)), (IMG, rgb(9, 9, 12, 4)), (COL, colours(9, 9, 13)), (IDS, prep2d_trees.label_ids(9, 9, 14))):
        specs += [Spec(src, mode, (1, 2, 6, 6), 4), Spec(src, mode, (0, 0, 9, 9), 6), Spec(src, mode, (2, 1, 7, 5), 2),
                  Spec(src, mode, (0, 0, 9, 9), 4), Spec(src, mode, (3, 0, 6, 9), 4), Spec(src, mode, (0, 0, 9, 9), 2)]
    check(specs, dev)


def test_pointers_off_their_alignment(dev):
    box = (2, 3, 8, 16)
    pal, known = palette()
    idx = np.random.default_rng(21).choice(known, (13, 22)).astype(np.uint8)
    specs = []
    for off in (1, 2, 3):
        specs += [Spec(rgb(13, 22, 22), IMG, box, 4, src_off=off, rgb_off=off), Spec(rgb(13, 22, 23, 4), IMG, box, 2, src_off=off),
                  Spec(idx, IMG, box, 4, pal, src_off=off), Spec(prep2d_trees.label_ids(13, 22, 24), IDS, box, 2, src_off=off, ids_off=off, rgb_off=off),
                  Spec(colours(13, 22, 25), COL, box, 2, src_off=off, rgb_off=off), Spec(colours(13, 22, 26, 4), COL, box, 2, src_off=off)]
    specs.append(Spec(colours(13, 22, 27), COL, box, 2, ids_off=8))      # int64 ids at 8 mod 16
    # the image's first and last bytes are taps: crop = the image
    specs += [Spec(rgb(8, 16, 28), IMG, (0, 0, 8, 16), 2, src_off=1), Spec(colours(8, 16, 29), COL, (0, 0, 8, 16), 2, src_off=3),
              Spec(rgb(2, 2, 30), IMG, (0, 0, 2, 2), 2, src_off=1), Spec(rgb(2, 2, 31, 4), IMG, (0, 0, 2, 2), 2, src_off=2)]
    check(specs, dev)


def test_an_item_is_the_same_bytes_alone_first_and_last(dev):
    # 30 x 101 output pixels: two work blocks, the boundary (pixel 2048) inside row 20
    big = [Spec(rgb(121, 405, 41), IMG, (0, 1, 120, 404), 4, src_off=1), Spec(colours(121, 405, 42), COL, (0, 1, 120, 404), 4),
           Spec(prep2d_trees.label_ids(121, 405, 43), IDS, (1, 0, 120, 404), 4)]
    others = small_specs()
    for item in big:
        alone, st0 = check([item], dev)
        first, st1 = check([item] + others, dev)
        last, st2 = check(others + [item], dev)
        assert alone[0] == first[0] == last[-1]
        assert st0[0] == st1[0] == st2[-1]


@pytest.mark.parametrize("mode", [IMG, IDS, COL])
def test_the_contracts_own_size(dev, mode):
    """1052 x 1914 -> crop (1024, 1912) at (14, 1) -> 256 x 478"""
    pal, known = palette()
    if mode == IMG:
        specs = [Spec(rgb(1052, 1914, 51), IMG, (14, 1, 1024, 1912), 4, src_off=1)]
    elif mode == IDS:
        specs = [Spec(prep2d_trees.label_ids(1052, 1914, 52), IDS, (14, 1, 1024, 1912), 4)]
    else:
        idx = np.random.default_rng(53).choice(known, (1052, 1914)).astype(np.uint8)
        specs = [Spec(idx, COL, (14, 1, 1024, 1912), 4, pal)]
    res, _ = check(specs, dev)
    assert len(res[0][0]) == 256 * 478 * 3


def test_status_counts_the_unknown_colours(dev):
    clean = colours(13, 22, 61)
    dirty = clean.copy()
    dirty[2:10:2, 3:19:2][np.random.default_rng(62).random((4, 8)) < 0.4] = (1, 2, 3)      # on the nearest grid of factor 2
    dirty[3, 4] = (9, 9, 9)                                                                    # off it
    pal, known = palette()
    idx = np.random.default_rng(63).integers(0, 256, (13, 22)).astype(np.uint8)                # unknown palette entries
    specs = [Spec(clean, COL, (2, 3, 8, 16), 2), Spec(dirty, COL, (2, 3, 8, 16), 2), Spec(idx, COL, (2, 3, 8, 16), 2, pal),
             Spec(rgb(13, 22, 64), IMG, (2, 3, 8, 16), 2)]
    _, status = check(specs, dev)
    assert status[0] == 0 and status[3] == 0 and status[1] > 0 and status[2] > 0
    assert status[1] == np.count_nonzero(specs[1].want()[1] == 128)


def test_refusals_leave_the_outputs_untouched(dev):
    pal, _ = palette()
    good, grey = rgb(13, 22, 71), prep2d_trees.label_ids(13, 22, 72)
    box = (2, 3, 8, 16)
    cases = [(Spec(good, IMG, (2, 7, 8, 16)), E_SHAPE), (Spec(good, IMG, (6, 3, 8, 16)), E_SHAPE), (Spec(good, IMG, (-1, 3, 8, 16)), E_SHAPE),
             (Spec(good, IMG, box, 3), E_SHAPE), (Spec(good, IMG, box, 0), E_SHAPE), (Spec(good, IMG, box, -2), E_SHAPE),
             (Spec(good, IMG, (2, 3, 1, 16), 4), E_SHAPE),                      # 1 / 4 rounds to an output of 0 rows
             (Spec(rgb(13, 22, 73, 2), IMG, box), E_DTYPE),                    # bpp 2
             (Spec(good, IMG, box, 4, pal), E_DTYPE),                          # a palette with bpp 3
             (Spec(grey, COL, box), E_DTYPE),                                  # bpp 1 without a palette
             (Spec(good, IDS, box), E_DTYPE), (Spec(good, 7, box), E_DTYPE)]
    for spec, code in cases:
        for batch in ([spec], small_specs()[:3] + [spec]):                      # alone, and behind items that are fine
            rc, res, status = run(batch, dev)
            assert rc == code, (rc, code)
            assert status == [-7] * len(batch)
            for r, i in res:
                assert r == bytes([SENTINEL]) * len(r) and i == bytes([SENTINEL]) * len(i)
    rc, res, status = run([Spec(grey, IDS, box)], dev, tables=False)           # a table the mode needs
    assert rc == E_NULL and status == [-7] and res[0][0] == bytes([SENTINEL]) * len(res[0][0])
    # H W bpp >= 2^31 is refused from the header alone (nothing of that size is allocated)
    import torch
    from values_amd import _lib
    from values_amd import preprocess2d as p2d
    lib = _lib.load()
    arr = (_lib.P2dItem * 1)()
    buf = torch.full((4096,), SENTINEL, dtype=torch.uint8, device=dev)
    arr[0].src = arr[0].out_rgb = arr[0].out_ids = buf.data_ptr()
    arr[0].H, arr[0].W, arr[0].bpp, arr[0].crop_h, arr[0].crop_w, arr[0].factor = 1 << 15, 1 << 14, 4, 8, 16, 4
    st = torch.full((1,), -7, dtype=torch.int32, device=dev)
    assert lib.vx_crop_resize_batched(arr, 1, p2d._device_tables(dev), st.data_ptr(), buf.data_ptr(), 4096, _lib.stream_ptr()) == E_SHAPE
    arr[0].src = None
    arr[0].H, arr[0].W = 13, 22
    assert lib.vx_crop_resize_batched(arr, 1, p2d._device_tables(dev), st.data_ptr(), buf.data_ptr(), 4096, _lib.stream_ptr()) == E_NULL
    torch.cuda.synchronize()
    assert st.item() == -7 and bool((buf == SENTINEL).all())


# ---------------------------------------------------------------------------------------------
# vx_png_encode_rgb

def _idat(png):
    import struct
    pos, out = 8, b""
    while pos < len(png):
        n, tag = struct.unpack(">I4s", png[pos:pos + 8])
        if tag == b"IDAT":
            out += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    return out


def test_png_encode_rgb(dev, tmp_path):
    import io
    import torch
    from PIL import Image
    from values_amd import image_io, images, results2d
    rng = np.random.default_rng(81)
    smooth = np.stack(np.broadcast_arrays(*np.ogrid[0:120, 0:100], 7), -1).astype(np.uint8)        # compressible
    imgs = [rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), rng.integers(0, 256, (3, 5, 3), dtype=np.uint8),
            rng.integers(0, 256, (120, 100, 3), dtype=np.uint8),                                      # 36120 scanline bytes: two chunks
            smooth, rng.integers(0, 256, (256, 478, 3), dtype=np.uint8)[:, :, :]]
    for batch in ([imgs[0]], [imgs[1]], [imgs[2]], imgs):                                             # alone and mixed
        files = results2d.png_encode_rgb([torch.from_numpy(a).to(dev) for a in batch])
        assert len(files) == len(batch)
        for k, (a, f) in enumerate(zip(batch, files)):
            h, w = a.shape[:2]
            im = Image.open(io.BytesIO(f))
            assert im.mode == "RGB" and im.size == (w, h)
            np.testing.assert_array_equal(np.asarray(im), a)
            path = tmp_path / f"e_{len(batch)}_{k}.png"
            path.write_bytes(f)
            np.testing.assert_array_equal(image_io.read_png(path), a)
            np.testing.assert_array_equal(images.load_png_device([path])[0].cpu().numpy(), a)
            raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, -1)], axis=1).tobytes()     # filter-0 scanlines
            assert zlib.decompress(_idat(f)) == raw
            assert len(f) <= 63 + len(raw) + 5 * (-(-len(raw) // 32768))
    # a file is the same bytes alone and in a batch
    assert results2d.png_encode_rgb([torch.from_numpy(imgs[3]).to(dev)])[0] == results2d.png_encode_rgb([torch.from_numpy(a).to(dev) for a in imgs])[3]
    # and it goes through the DEFLATE chunk kernel, not around it: a file of stored blocks alone is the scanline bytes plus
    # framing, so a file below the scanline bytes holds matches (how far below is the chunk kernel's business)
    assert len(results2d.png_encode_rgb([torch.from_numpy(imgs[3]).to(dev)])[0]) < 120 * (3 * 100 + 1)
    # the encoder of the masks through a table is what it was: the recorded bytes
    with open(writer_trees.GOLDEN) as f:
        golden = json.load(f)
    masks = [writer_trees.batch2d("m", 1, 1, H, W, 800 + i, True) for i, (H, W) in enumerate((writer_trees.SMALL, writer_trees.LARGE, (5, 3)))]
    files = results2d.png_encode([torch.from_numpy(m["pred_masks"][0, 0]).to(dev) for m in masks],
                                 [None if i == 1 else m["ignore_index_map"][0] for i, m in enumerate(masks)])
    for i, b in enumerate(files):
        assert hashlib.sha256(b).hexdigest() == golden[f"png_encode/{i}"]
    with pytest.raises(ValueError):
        results2d.png_encode_rgb([torch.zeros((4, 4), dtype=torch.uint8, device=dev)])


# ---------------------------------------------------------------------------------------------
# the data set on the device

def _files(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


@pytest.mark.parametrize("dataset", ["cityscapes", "gta"])
def test_dataset_device_route_equals_the_host_route(dev, tmp_path, capsys, dataset):
    from PIL import Image
    from values_amd import preprocess_dataset_2d
    kw = dict(crop=prep2d_trees.CROP, factor=prep2d_trees.FACTOR)
    cases = (prep2d_trees.cityscapes_tree if dataset == "cityscapes" else prep2d_trees.gta_tree)(tmp_path / "raw")
    done = sorted(cases)[1]
    for out in ("host", "device"):
        finished_case(tmp_path / out, done)
    assert preprocess_dataset_2d(tmp_path / "raw", tmp_path / "host", dataset, **kw) == 1
    capsys.readouterr()
    assert preprocess_dataset_2d(tmp_path / "raw", tmp_path / "device", dataset, device_io=True, batch=2, **kw) == 1
    assert "Different resolutions between image and mask for" in capsys.readouterr().out
    todo = {k: v for k, v in cases.items() if k != done}
    assert check_tree(tmp_path / "device", todo, dataset) == expected_files(todo, [done])
    assert untouched(tmp_path / "device", done)
    host, device = _files(tmp_path / "host" / "preprocessed"), _files(tmp_path / "device" / "preprocessed")
    assert sorted(host) == sorted(device)
    for name in host:
        if name.endswith(".npy"):
            assert host[name] == device[name], name
        elif done not in name:
            np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "host" / "preprocessed" / name)),
                                          np.asarray(Image.open(tmp_path / "device" / "preprocessed" / name)), err_msg=name)
    # a second run over the finished tree writes nothing
    stamp = lambda: {n: os.stat(tmp_path / "device" / "preprocessed" / n).st_mtime_ns for n in device}
    before = stamp()
    assert preprocess_dataset_2d(tmp_path / "raw", tmp_path / "device", dataset, device_io=True, **kw) == 1
    assert stamp() == before and _files(tmp_path / "device" / "preprocessed") == device
    # one batch for all, and one case per batch: the same files
    assert preprocess_dataset_2d(tmp_path / "raw", tmp_path / "device1", dataset, device_io=True, batch=1, **kw) == 1
    one = _files(tmp_path / "device1" / "preprocessed")
    assert sorted(one) == sorted(device)
    assert {n: b for n, b in one.items() if done not in n} == {n: b for n, b in device.items() if done not in n}


def test_dataset_device_route_raises_on_an_unknown_colour(dev, tmp_path):
    from values_amd import preprocess_dataset_2d
    prep2d_trees.gta_tree(tmp_path / "raw", unknown=True)
    with pytest.raises(AssertionError, match="Unknown color value in mask for image 00001.png!"):
        preprocess_dataset_2d(tmp_path / "raw", tmp_path / "out", "gta", device_io=True, crop=prep2d_trees.CROP, factor=prep2d_trees.FACTOR)
    with pytest.raises(ValueError):            # the sources are smaller than the contract's crop
        preprocess_dataset_2d(tmp_path / "raw", tmp_path / "out2", "gta", device_io=True)


def test_preprocess_images_device_and_the_tta_views(dev, tmp_path):
    import torch
    from values_amd import preprocess_images_device
    from values_amd import preprocess2d as p2d
    from values_amd.data import hflip_flags, tta_views_2d, tta_views_2d_device
    for dataset, tree in (("cityscapes", prep2d_trees.cityscapes_tree), ("gta", prep2d_trees.gta_tree)):
        cases = tree(tmp_path / dataset)
        todo = p2d.list_cases(tmp_path / dataset, tmp_path / "nowhere", dataset)
        todo = [c for c in todo if c[0] in cases]
        assert len(todo) == len(cases) == 3
        res = preprocess_images_device([c[2] for c in todo], [c[3] for c in todo], dataset, crop=prep2d_trees.CROP,
                                       factor=prep2d_trees.FACTOR, batch=2)
        for (image_id, _, _, _), (image, ids, colour) in zip(todo, res):
            want = p2d.preprocess_image(*cases[image_id], dataset, prep2d_trees.CROP, prep2d_trees.FACTOR)
            assert image.is_cuda and image.dtype == torch.uint8 and ids.dtype == (torch.uint8 if dataset == "cityscapes" else torch.int64)
            for got, w in zip((image, ids, colour), want):
                assert tuple(got.shape) == w.shape and got.is_contiguous()
                np.testing.assert_array_equal(got.cpu().numpy(), w)
        # the image goes to the TTA views as it is: a contiguous device tensor, no copy through the host
        image = res[0][0]
        mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        views, names = tta_views_2d_device(image, mean, std)
        host_views, host_names = tta_views_2d(image.cpu().numpy(), mean=mean, std=std)
        # (without noise fields both give the clean views in the noise slots; only the host function still names them)
        assert hflip_flags(names) == hflip_flags(host_names) and views.shape == (4, 1) + tuple(image.shape[:2]) + (4,)
        for g in range(4):
            np.testing.assert_array_equal(views[g, 0, :, :, :3].permute(2, 0, 1).cpu().numpy(), host_views[g])
    with pytest.raises(ValueError):
        bad = [c for c in p2d.list_cases(tmp_path / "gta", tmp_path / "nowhere", "gta") if c[0] == "00003"][0]
        preprocess_images_device([bad[2]], [bad[3]], "gta", crop=prep2d_trees.CROP)
