"""GPU: reading the 2D results tree on the device -- vx_png_unfilter through the C ABI against the images the streams
were built from (all five filters, band edges, odd pitches, unaligned buffers), its statuses, vx_rgb_to_trainid, the
device readers (images.load_png_device / load_tiff_device / ImageReader) against the host readers, and
DeviceExperimentDataloader / aggregate_uncertainties_device on a written tree against the host dataloader."""
import json
import os

import numpy as np
import pytest
import torch

from tests import png_build as pb
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = 3   # bytes between the items' outputs: odd offsets, and a write past an item's end shows


def _unfilter(cases, src_n=None):
    """cases: [(img (H, W, bpp), scanline bytes)] -> (statuses, [decoded (H, W, bpp) array]): one vx_png_unfilter call;
    the streams lie back to back in one device buffer and so do the outputs, GUARD bytes apart, so that sources and
    destinations start at every alignment.  src_n: per item an override of the stream size handed to the kernel."""
    from values_amd import images
    dev = torch.device("cuda")
    src = torch.from_numpy(np.frombuffer(b"".join(s for _, s in cases), dtype=np.uint8).copy()).to(dev)
    total = sum(img.size + GUARD for img, _ in cases)
    dst = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    entries, so, do, places = [], 0, 0, []
    for k, (img, s) in enumerate(cases):
        h, w, bpp = img.shape
        n = len(s) if src_n is None or src_n[k] is None else src_n[k]
        entries.append((src.data_ptr() + so, n, h, w, bpp, dst.data_ptr() + do))
        places.append((do, img.size))
        so += len(s)
        do += img.size + GUARD
    st = images.png_unfilter(entries, dev)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    for do, n in places:
        assert (host[do + n:do + n + GUARD] == 0xA5).all(), "a write beyond an item's output"
    return st, [host[do:do + n].reshape(img.shape) for (do, n), (img, _) in zip(places, cases)]


@pytest.mark.parametrize("bpp", pb.BPPS)
def test_unfilter_grid_bit_exact(bpp):
    cases = [(name, img, ft) for name, img, ft in pb.grid_cases() if img.shape[2] == bpp]
    assert len(cases) == 6 * 3 * 7
    st, outs = _unfilter([(img, pb.scanlines(img, ft)) for _, img, ft in cases])
    for (name, img, _), s, out in zip(cases, st, outs):
        assert s == 0, (name, s)
        bad = np.argwhere(out != img)
        assert bad.size == 0, (name, "first mismatch (y, x, c)", bad[0].tolist(), int(out[tuple(bad[0])]), int(img[tuple(bad[0])]))


def test_unfilter_mixed_batch_order_and_offsets():
    rng = np.random.default_rng(11)
    cases = []
    for k in range(300):
        h, w = ((8, 8), (5, 3))[k % 2]
        bpp = (1, 3, 4)[k % 3]
        img = rng.integers(0, 256, (h, w, bpp)).astype(np.uint8)
        cases.append((img, pb.scanlines(img, pb.filters("random", h, seed=k))))
    big = pb.content(130, 67, 3, seed=2)
    cases.insert(150, (big, pb.scanlines(big, pb.filters("random", 130, seed=9))))
    st, outs = _unfilter(cases)
    assert st == [0] * 301
    for k, ((img, _), out) in enumerate(zip(cases, outs)):
        assert np.array_equal(out, img), k


def test_unfilter_statuses_leave_the_other_items_alone():
    from values_amd import _lib
    img = pb.content(66, 9, 3)
    good = pb.scanlines(img, pb.filters("cyclic", 66))
    bad = bytearray(good)
    bad[65 * (1 + 27)] = 5                                # the last row's filter byte
    small = pb.content(3, 4, 1)
    s_small = pb.scanlines(small, pb.filters("paeth", 3))
    cases = [(img, good), (img, bytes(bad)), (small, s_small), (img, good), (small, s_small)]
    st, outs = _unfilter(cases, src_n=[None, None, len(s_small) - 1, None, None])
    assert st == [_lib.VX_PNG_OK, _lib.VX_PNG_BAD_FILTER, _lib.VX_PNG_BAD_SIZE, _lib.VX_PNG_OK, _lib.VX_PNG_OK]
    assert np.array_equal(outs[0], img) and np.array_equal(outs[3], img) and np.array_equal(outs[4], small)
    assert (outs[1] == 0xA5).all() and (outs[2] == 0xA5).all()     # refused items write nothing
    st, _ = _unfilter([(small, s_small)], src_n=[len(s_small) + 1])
    assert st == [_lib.VX_PNG_BAD_SIZE]


def test_filter0_copy_and_the_walk_agree():
    for bpp in pb.BPPS:
        img = pb.content(70, 67, bpp, seed=4)
        ft = pb.filters("none", 70)
        one = ft.copy()
        one[37] = 1                                        # one Sub row: the item takes the walk
        st, outs = _unfilter([(img, pb.scanlines(img, ft)), (img, pb.scanlines(img, one))])
        assert st == [0, 0]
        assert np.array_equal(outs[0], img) and np.array_equal(outs[1], outs[0])


def test_rgb_to_trainid_matches_the_host_form():
    from values_amd import gta
    rng = np.random.default_rng(3)
    cols = np.array(list(gta.COLOR2TRAINID) + [(1, 2, 3), (128, 64, 129), (142, 0, 0)], dtype=np.uint8)
    img = cols[rng.integers(0, len(cols), (37, 53))]                         # 1961 pixels: no multiple of 4
    want = gta.rgb_to_trainid_host(img)
    assert (want == gta.UNKNOWN).any() and len(np.unique(want)) > 20
    t = torch.from_numpy(img).cuda()
    got = gta.rgb_to_trainid(t)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy().astype(np.int64), want)
    flat = t.reshape(-1, 3)
    for skip in (1, 2, 3):                                                   # sources and outputs off the dword grid
        got = gta.rgb_to_trainid(flat[skip:])
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want.reshape(-1)[skip:]), skip
    tab = torch.tensor([[0x010203, 7], [0x8E0000, 9], [0x010203, 8]], dtype=torch.int32, device="cuda")
    got = gta.rgb_to_trainid(t, table=tab, default_id=200).cpu().numpy()     # of two entries with one key the later counts
    keys = gta.rgb_keys(img)
    assert np.array_equal(got, np.where(keys == 0x010203, 8, np.where(keys == 0x8E0000, 9, 200)).astype(np.uint8))


def test_load_png_device_matches_read_png(tmp_path):
    from values_amd import _lib, images
    from values_amd.image_io import read_png, write_png
    paths = []
    for k, (bpp, pat, n_idat) in enumerate(((3, "random", 3), (1, "paeth", 2), (4, "average", 5), (3, "none", 1))):
        img = pb.content(40 + k, 31, bpp, seed=k)
        p = tmp_path / f"f{k}.png"
        p.write_bytes(pb.png_bytes(pb.squeeze(img), pb.filters(pat, 40 + k, seed=k), n_idat=n_idat))
        paths.append(p)
    write_png(tmp_path / "own.png", pb.content(9, 7, 3))
    paths.append(tmp_path / "own.png")
    paths += [os.path.join(GOLDEN, "images2d", f"pil_{n}.png") for n in ("rgb", "grey", "rgba")]
    outs = images.load_png_device(paths)
    for p, t in zip(paths, outs):
        want = read_png(p)
        assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == want.shape, p
        assert np.array_equal(t.cpu().numpy(), want), p
    for n in ("rgb", "grey", "rgba"):
        assert np.array_equal(outs[5 + ("rgb", "grey", "rgba").index(n)].cpu().numpy(),
                              np.load(os.path.join(GOLDEN, "images2d", f"pil_{n}.npy")))
    # a broken file is named
    raw = bytearray(paths[0].read_bytes())
    raw[-30] ^= 0x55                                       # inside the last IDAT chunk's data
    (tmp_path / "broken.png").write_bytes(bytes(raw))
    with pytest.raises(_lib.VxError, match="broken.png"):
        images.load_png_device([paths[1], tmp_path / "broken.png"])


def test_load_tiff_device_and_image_reader_match_the_host_readers(tmp_path):
    from values_amd import images
    from values_amd.image_io import read_png, read_tiff_f32, write_tiff_f32
    rng = np.random.default_rng(8)
    paths = []
    for k, (endian, rps, comp) in enumerate((("<", None, 1), ("<", 4, 1), ("<", 5, 8), ("<", None, 32946), (">", 3, 8), (">", None, 1),
                                             ("<", 1, 8))):
        m = rng.random((21 + k, 13), dtype=np.float32)
        m[5:9] = 0.5
        p = tmp_path / f"m{k}.tif"
        p.write_bytes(pb.tiff_bytes(m, endian, rps, comp))
        paths.append(p)
    write_tiff_f32(tmp_path / "own.tiff", rng.random((6, 9), dtype=np.float32))
    paths.append(tmp_path / "own.tiff")
    for p, t in zip(paths, images.load_tiff_device(paths)):
        want = read_tiff_f32(p)
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == want.shape, p
        assert np.array_equal(t.cpu().numpy(), want), p
    pngs = []
    for k in range(5):
        img = pb.content(12 + k, 10, 3, seed=k)
        p = tmp_path / f"p{k}.png"
        p.write_bytes(pb.png_bytes(img, pb.filters("random", 12 + k, seed=k)))
        pngs.append(p)
    batches = [pngs[:2] + paths[:3], [], paths[3:] + pngs[2:]]
    with images.ImageReader(workers=2) as r:
        res = list(r.read(batches))
    assert [len(x) for x in res] == [5, 0, 8]
    for batch, out in zip(batches, res):
        for p, t in zip(batch, out):
            want = read_png(p) if str(p).endswith(".png") else read_tiff_f32(p)
            assert np.array_equal(t.cpu().numpy(), want), p


def test_written_2d_tree_read_back_on_the_device(tmp_path):
    from values_amd import results2d
    from values_amd.experiment import (DeviceExperimentDataloader, ExperimentDataloader, ExperimentVersion,
                                       aggregate_uncertainties, aggregate_uncertainties_device)
    rng = np.random.default_rng(5)
    ids, T, H, W = ["img_a", "img_b", "img_c"], 2, 20, 33
    pm = torch.from_numpy(rng.integers(0, 24, (3, T, H, W)).astype(np.uint8)).cuda()
    mm = torch.from_numpy(rng.integers(0, 24, (3, H, W)).astype(np.uint8)).cuda()
    names = ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")
    unc = {k: torch.from_numpy(rng.random((3, H, W), dtype=np.float32)).cuda() for k in names}
    types = ["predictive_uncertainty", "aleatoric_uncertainty", "epistemic_uncertainty"]
    aggs = {"patch_level": {"_target_": "values_amd.aggregation.patch_level_aggregation", "patch_size": 5},
            "image_level": {"_target_": "values_amd.aggregation.image_level_aggregation", "mean": True},
            "threshold": {"_target_": "values_amd.aggregation.threshold_aggregation", "threshold": 0.6}}
    for writer in ("device", "host"):
        ev = ExperimentVersion(base_path=tmp_path / writer, naming_scheme_version="seed{seed}", pred_model="Dropout",
                               image_ending=".png", unc_ending=".tif", unc_types=types, aggregations=None, n_reference_segs=1,
                               pred_seg_loading={"_target_": "evaluation.utils.gta.pred_seg_loading"}, seed=7)
        save_dir = str(ev.exp_path / "val")
        if writer == "device":
            results2d.save_images_device(save_dir, ids, pm, mm, unc)
        else:
            os.makedirs(os.path.join(save_dir, "pred_seg"))
            for b, iid in enumerate(ids):
                results2d.save_prediction(os.path.join(save_dir, "pred_seg"), iid, pm[b], mm[b])
                results2d.save_uncertainty(save_dir, iid, {k: v[b] for k, v in unc.items()})
        host, dev = ExperimentDataloader(ev, "val"), DeviceExperimentDataloader(ev, "val")
        assert host.image_ids == dev.image_ids == ids
        assert dev.prefetch(["img_b"]) == (T + 1) + 3
        for b, iid in enumerate(ids):
            for u, k in zip(types, names):
                t = dev.get_unc_map(iid, u)
                want = host.get_unc_map(iid, u)
                assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (W, H) == want.shape
                assert np.array_equal(t.cpu().numpy(), want) and np.array_equal(want, unc[k][b].cpu().numpy().T)
            hs, ds = host.get_pred_segs(iid), dev.get_pred_segs(iid)
            assert len(hs) == len(ds) == T + 1
            for a, t in zip(hs, ds):
                assert tuple(t.shape) == (W, H, 3) and np.array_equal(t.cpu().numpy(), a)
            mean = dev.get_mean_pred_seg(iid)                       # the hook, in its device form
            assert mean.is_cuda and mean.dtype == torch.int64 and tuple(mean.shape) == (H, W)
            assert np.array_equal(mean.cpu().numpy(), host.get_mean_pred_seg(iid))
            assert np.array_equal(mean.cpu().numpy(), mm[b].cpu().numpy().astype(np.int64))
        assert not dev._cache
        aggregate_uncertainties(host, aggs)
        want = {u: open(host.dataset_path / f"aggregated_{u}.json", "rb").read() for u in types}
        for u in types:
            os.remove(host.dataset_path / f"aggregated_{u}.json")
        aggregate_uncertainties_device(dev, aggs, batch=2)
        for u in types:
            got = open(dev.dataset_path / f"aggregated_{u}.json", "rb").read()
            assert got == want[u], (writer, u)
            assert sorted(json.loads(got)) == [f"{i}.tif" for i in ids]
