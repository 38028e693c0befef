"""GPU: the 3D test split on the device -- the three batched kernels of patches3d.hip (gather, per-patch accumulate,
case composite), the device loader against the host loader, and run_test_3d against the per-case route."""
import gzip
import json
import os

import numpy as np
import pytest
import torch

from tests import dataset3d_trees as trees

pytestmark = pytest.mark.gpu
P = trees.PATCH
RUN_CASES = ("c16", "c32", "c1632")           # one, two and two patches; float32, int16 and float64 files; z 16..23 of the last uncovered


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# gather

def test_gather_mixed_volumes_in_one_call():
    from values_amd.sliding import gather_patches_3d
    rng = np.random.default_rng(3)
    vols = [rng.standard_normal((5, 6, 7)) * 1e3 / 3,                                    # float64: rounds to nearest even
            rng.standard_normal((8, 8, 8)).astype(np.float32),
            rng.integers(-32768, 32767, size=(9, 4, 12), dtype=np.int16)]
    recs = [{"image": _t(v), "image_path": f"v{i}"} for i, v in enumerate(vols)]
    # rows that start off a 16-byte phase (odd z origins; the (5, 6, 7) rows have an odd pitch) and end at the volume's edge
    picks = [(0, (1, 2, 3)), (0, (0, 0, 0)), (1, (4, 4, 4)), (1, (3, 1, 2)), (2, (5, 0, 8)), (2, (0, 0, 1)), (2, (2, 0, 5))]
    patches = [(recs[i], tuple((o, o + 4) for o in org)) for i, org in picks]
    want = np.stack([vols[i][o[0]:o[0] + 4, o[1]:o[1] + 4, o[2]:o[2] + 4].astype(np.float32) for i, o in picks])[:, None]
    got = gather_patches_3d(patches, 4)
    assert got.shape == (7, 1, 4, 4, 4) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), want)
    assert (vols[0].astype(np.float32).astype(np.float64) != vols[0]).any()              # the float64 case really rounds
    for b, p in enumerate(patches):                                                      # each item alone: the same bits
        assert torch.equal(gather_patches_3d([p], 4)[0], got[b])
    # an out base off 16 bytes
    flat = torch.full((7 * 64 + 3,), -7.0, device="cuda")
    out = flat[1:1 + 7 * 64].view(7, 1, 4, 4, 4)
    assert out.data_ptr() % 16 == 4
    gather_patches_3d(patches, 4, out=out)
    assert torch.equal(out, got) and flat[0].item() == -7.0 and (flat[1 + 7 * 64:] == -7.0).all()


def test_gather_every_kind_and_ragged_rows():
    """all eight stored kinds; a patch row of 7 elements (one full quad and a ragged one)"""
    from values_amd import _lib
    from values_amd.dataset3d import _IMAGE_KIND
    lib = _lib.load()
    rng = np.random.default_rng(5)
    arrs = [rng.integers(0, 255, (7, 8, 9)).astype(np.uint8), rng.integers(-128, 127, (7, 8, 9)).astype(np.int8),
            rng.integers(0, 65535, (7, 8, 9)).astype(np.uint16), rng.integers(-32768, 32767, (7, 8, 9)).astype(np.int16),
            rng.integers(0, 2 ** 32 - 1, (7, 8, 9), dtype=np.uint32), rng.integers(-2 ** 31, 2 ** 31 - 1, (7, 8, 9)).astype(np.int32),
            rng.standard_normal((7, 8, 9)).astype(np.float32), rng.standard_normal((7, 8, 9)) / 3]
    ts = [_t(a) for a in arrs]
    P0, P1, P2 = 2, 3, 7
    items = (_lib.Gather3dItem * len(arrs))()
    for it, a, t in zip(items, arrs, ts):
        it.src, it.kind = t.data_ptr(), _IMAGE_KIND[a.dtype.name]
        for ax in range(3):
            it.dims[ax], it.origin[ax] = a.shape[ax], (5, 4, 2)[ax]
    out = torch.full((len(arrs), P0, P1, P2), np.nan, device="cuda")
    ws = _lib.workspace(out.device, int(lib.vx_gather_patches_3d_workspace_bytes(len(arrs))))
    _lib.check(lib.vx_gather_patches_3d(items, len(arrs), _lib.ptr(out), P0, P1, P2, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "gather")
    want = np.stack([a[5:7, 4:7, 2:9].astype(np.float32) for a in arrs])
    assert np.array_equal(out.cpu().numpy(), want)
    assert (arrs[4].astype(np.float32).astype(np.float64) != arrs[4]).any()              # uint32 -> float32 rounds too


# ---------------------------------------------------------------------------------------------------------------------
# accumulate

def _old_accumulate(logits, origins, ssum, count, overlap):
    from values_amd import _lib
    B, T, C = (int(v) for v in logits.shape[:3])
    Pn = int(logits.shape[-1])
    crop = torch.tensor(origins, dtype=torch.int32, device="cuda")
    X, Y, Z = (int(v) for v in count.shape)
    _lib.check(_lib.load().vx_softmax_accumulate(_lib.ptr(logits.contiguous()), B, T, C, Pn, Pn, Pn, _lib.ptr(crop), _lib.ptr(ssum),
                                                 _lib.ptr(count), X, Y, Z, int(overlap), _lib.stream_ptr()), "vx_softmax_accumulate")


@pytest.mark.parametrize("C", [2, 3, 8])
def test_accumulate_cases_equals_the_per_image_call(C):
    from values_amd.sliding import accumulate_cases
    T, Pn = 3, 4
    g = torch.Generator().manual_seed(C)
    logits = (torch.randn((5, T, C, Pn, Pn, Pn), generator=g) * 3).cuda()
    shapes = [(8, 4, 4), (4, 4, 9), (5, 6, 7)]
    # patch -> (image, origin): two disjoint crops of image 0, one of image 1 starting off a 16-byte phase, two of image 2
    # of which the second reaches past the image on every axis (its outside voxels are skipped one by one)
    where = [(0, (0, 0, 0)), (2, (0, 1, 1)), (1, (0, 0, 5)), (0, (4, 0, 0)), (2, (3, 4, 5))]
    new = [(torch.zeros((T, C) + s, device="cuda"), torch.zeros(s, device="cuda")) for s in shapes]
    old = [(torch.zeros((T, C) + s, device="cuda"), torch.zeros(s, device="cuda")) for s in shapes]
    # image 2's two crops (0..3, 1..4, 1..4) and (3.., 4.., 5..) share x = 3, y = 4 but no z: disjoint
    accumulate_cases(logits, [new[i] + (o,) for i, o in where], False)
    for i in range(3):
        idx = [b for b, (j, _) in enumerate(where) if j == i]
        _old_accumulate(logits[idx], [where[b][1] for b in idx], old[i][0], old[i][1], False)
    for i in range(3):
        assert torch.equal(new[i][0], old[i][0]) and torch.equal(new[i][1], old[i][1]), i
        assert new[i][1].max().item() == 1
    assert new[2][1].sum().item() == 64 + 2 * 2 * 2            # the crop past the image left its inside corner only
    assert (new[0][0].sum(1) - new[0][1][None]).abs().max().item() < 1e-5


def test_accumulate_cases_overlapping_crops_within_the_summation_bound():
    """|new - old| <= 2 (n - 1) n 2^-24 per voxel, n the voxel's count: n addends in [0, 1] and n - 1 float32 roundings of
    partial sums <= n put each route within (n - 1) n 2^-24 of the exact sum.  Counts are equal exactly."""
    from values_amd.sliding import accumulate_cases
    T, C, Pn = 3, 3, 4
    g = torch.Generator().manual_seed(11)
    origins = [(x, y, z) for z in (0, 2) for y in (0, 2) for x in (0, 1, 2)]        # 12 crops of a 6^3 image, count up to 12
    logits = (torch.randn((len(origins), T, C, Pn, Pn, Pn), generator=g) * 3).cuda()
    new = (torch.zeros((T, C, 6, 6, 6), device="cuda"), torch.zeros((6, 6, 6), device="cuda"))
    old = (torch.zeros((T, C, 6, 6, 6), device="cuda"), torch.zeros((6, 6, 6), device="cuda"))
    accumulate_cases(logits, [new + (o,) for o in origins], True)
    _old_accumulate(logits, origins, old[0], old[1], True)
    assert torch.equal(new[1], old[1]) and new[1].max().item() == 12
    n = new[1].double()
    bound = 2 * (n - 1) * n * 2.0 ** -24
    diff = (new[0].double() - old[0].double()).abs()
    print("overlap accumulate: max |new - old| =", diff.max().item(), "max bound", bound.max().item())
    assert (diff <= bound[None, None]).all()
    # the plain read-modify-write form refuses what it cannot do
    from values_amd import _lib
    with pytest.raises(_lib.VxError, match="overlapping"):
        accumulate_cases(logits, [new + (o,) for o in origins], False)


# ---------------------------------------------------------------------------------------------------------------------
# composite

def _records(names, raters=(0, 1, 2)):
    return [{"image_path": n + ".npy", "label_paths": [f"{n}_{r:02d}.npy" for r in raters], "image_id": n,
             "image": _t(trees.image(n)), "labels": [_t(trees.label(n, r)) for r in raters]} for n in names]


def _count_of(name):
    from values_amd import crop_indices
    shape, _, overlap = trees.CASES[name]
    crops = crop_indices(shape, P, overlap)
    cnt = np.zeros(shape, dtype=np.float32)
    for c in crops:
        cnt[tuple(slice(a, b) for a, b in c)] += 1
    return crops, cnt


def test_composite_equals_compose_case():
    from values_amd.dataset3d import compose_case, composite_device
    names = list(trees.CASES)
    recs = _records(names)                                   # raters stored as uint8, int32 and int64
    counts = [_t(_count_of(n)[1]) for n in names]
    out = composite_device(recs, counts)
    for n, o in zip(names, out):
        want = compose_case(trees.image(n), [trees.label(n, r) for r in range(3)], _count_of(n)[0])
        assert o["data"].dtype == torch.float64 and np.array_equal(o["data"].cpu().numpy(), want["data"]), n
        assert o["gt_seg"].dtype == torch.float64 and np.array_equal(o["gt_seg"].cpu().numpy(), want["gt_seg"]), n
        assert o["gt"].dtype == torch.uint8 and np.array_equal(o["gt"].cpu().numpy(), want["gt"]), n
    assert _count_of("c24")[1].max() == 8 and _count_of("c2416")[1].max() == 3 and _count_of("c1632")[1].min() == 0
    # a case alone gives the same bits; outputs may be left out
    alone = composite_device(recs[4:5], counts[4:5], want_gt_seg=False)
    assert set(alone[0]) == {"data", "gt"} and torch.equal(alone[0]["data"], out[4]["data"]) and torch.equal(alone[0]["gt"], out[4]["gt"])
    # a label 300 sets the status: the error names the rater files of that case
    bad = _records(["c16"], raters=(1,))
    bad[0]["labels"][0][3, 4, 5] = 300
    with pytest.raises(ValueError, match=r"c16_01\.npy: 1 labels outside 0\.\.255"):
        composite_device(recs[:1] + bad, [counts[0], counts[0]])


# ---------------------------------------------------------------------------------------------------------------------
# loaders

def _split(tmp_path, names=RUN_CASES, raters=(0, 1), overlap=1, layout="toy"):
    from values_amd.dataset3d import cases, get_val_test_data_samples
    base = trees.build_tree(tmp_path, layout, raters={n: list(raters) for n in trees.CASES}, names=names)
    return cases(get_val_test_data_samples(base, pattern=trees.PATTERN, num_raters=3, test=True, patch_size=P, patch_overlap=overlap,
                                           layout=layout))


def test_device_loader_equals_host_loader(tmp_path):
    from values_amd.dataset3d import DeviceTestLoader3D, HostTestLoader3D
    cs = _split(tmp_path, names=list(trees.CASES), raters=(0, 1, 2))
    host = list(HostTestLoader3D(cs, 2))
    for prefetch in (True, False):
        with DeviceTestLoader3D(cs, 2, prefetch=prefetch) as loader:
            dev = list(loader)
            assert len(loader) == 3
        assert [len(g) for g in dev] == [len(g) for g in host] == [2, 2, 1]
        for gd, gh in zip(dev, host):
            for d, h in zip(gd, gh):
                assert {k: v for k, v in d.items() if k not in ("image", "labels")} == {k: v for k, v in h.items() if k not in ("image", "labels")}
                assert d["image"].is_cuda and str(d["image"].dtype) == "torch." + str(h["image"].dtype)       # the stored dtype
                assert torch.equal(d["image"].cpu(), torch.from_numpy(h["image"]))
                assert len(d["labels"]) == 3
                for ld, lh in zip(d["labels"], h["labels"]):
                    assert str(ld.dtype) == "torch." + str(lh.dtype) and torch.equal(ld.cpu(), torch.from_numpy(lh))


def test_device_loader_refusals(tmp_path):
    from values_amd.dataset3d import DeviceTestLoader3D
    cs = _split(tmp_path, names=["c16"], raters=(0,))
    img, lab = cs[0]["image_path"], cs[0]["label_paths"][0]
    good_img, good_lab = np.load(img), np.load(lab)

    def refused(path, arr, word, **kw):
        np.save(path, arr, **kw)
        for prefetch in (True, False):
            with DeviceTestLoader3D(cs, 1, prefetch=prefetch) as loader:
                with pytest.raises(ValueError, match=word) as e:
                    list(loader)
            assert os.path.basename(path) in str(e.value)
        np.save(img, good_img)
        np.save(lab, good_lab)

    refused(img, np.asfortranarray(good_img), "C-order")
    refused(lab, np.asfortranarray(good_lab), "C-order")
    refused(img, np.array([[[None]]], dtype=object), "C-order|object", allow_pickle=True)
    refused(img, good_img[0], "3-D image")
    refused(img, good_img[None], "3-D image")
    refused(lab, good_lab[:, :, :8], "differs from its image")
    refused(img, good_img.astype(np.float16), "dtype")
    refused(img, good_img.astype(np.int64), "dtype")
    refused(img, good_img.astype(">f4"), "dtype")
    refused(lab, good_lab.astype(np.float32), "dtype")
    with DeviceTestLoader3D(cs, 1) as loader:                # the files are whole again
        (g,) = list(loader)
    assert torch.equal(g[0]["image"].cpu(), torch.from_numpy(good_img))
    with pytest.raises(ValueError):
        DeviceTestLoader3D(cs, 0)


# ---------------------------------------------------------------------------------------------------------------------
# run_test_3d

@pytest.fixture(scope="module")
def members():
    from tests.test_gpu_unet3d import make_model
    return [make_model(seed_tag=s, do_dropout=False) for s in range(2)]


@pytest.fixture(scope="module")
def dropout_model():
    from tests.test_gpu_unet3d import make_model
    return make_model(do_dropout=True)


def _tree(d):
    """{relative path: the file's bytes after gunzip}"""
    out = {}
    for root, _, fs in os.walk(d):
        for f in fs:
            p = os.path.join(root, f)
            raw = open(p, "rb").read()
            out[os.path.relpath(p, d)] = gzip.decompress(raw) if f.endswith(".gz") else raw
    return out


def _per_case_route(models, cs, save_dir, overlap=1, **kw):
    """what a user could write before run_test_3d: one image at a time"""
    from values_amd import predict_image_sliding, results
    from values_amd.dataset3d import compose_case
    from values_amd.metrics import process_metrics_3d
    metrics, outs = {}, {}
    for c in cs:
        img, labels = np.load(c["image_path"]), [np.load(p) for p in c["label_paths"]]
        out = predict_image_sliding(models, torch.from_numpy(img), patch_size=P, patch_overlap=overlap, patch_batch=8, **kw)
        comp = compose_case(img, labels, c["crops"])
        (m,) = process_metrics_3d({"mean_softmax": out["mean_softmax"][None], "argmax": out["pred_seg_mean"][None]},
                                  torch.from_numpy(comp["gt"].astype(np.uint8))[None], probs=out["softmax_sum"][None])
        metrics[c["image_id"]] = m
        maps = {k: out[k] for k in ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")}
        results.save_case_device(save_dir, c["image_id"], out["softmax_sum"], maps, data=comp["data"], gt_seg=comp["gt_seg"],
                                 num_predictions=out["num_predictions"])
        outs[c["image_id"]] = (out, comp)
    results.log_metrics(save_dir, metrics)
    return outs


def test_run_test_3d_deterministic_equals_the_per_case_route(tmp_path, members):
    from values_amd import run_test_3d
    from values_amd.dataset3d import DeviceTestLoader3D, HostTestLoader3D
    cs = _split(tmp_path)
    assert [len(c["crops"]) for c in cs] == [1, 2, 2] and [c["image_id"] for c in cs] == ["c16", "c1632", "c32"]
    ref_dir = str(tmp_path / "ref")
    _per_case_route(members, cs, ref_dir)
    want = _tree(ref_dir)
    assert len(want) == 3 * (1 + 2 + 3 * (1 + 2) + 3) + 1 and "metrics.json" in want
    runs = [("dev", 3, 32), ("dev", 3, 1), ("dev", 3, 3), ("dev", 1, 32), ("dev", 1, 3), ("host", 3, 3), ("host", 2, 32)]
    for kind, group_cases, patch_batch in runs:
        d = str(tmp_path / f"{kind}_{group_cases}_{patch_batch}")
        if kind == "dev":
            with DeviceTestLoader3D(cs, group_cases) as loader:
                res = run_test_3d(members, loader, d, patch_size=P, patch_batch=patch_batch)
        else:
            res = run_test_3d(members, HostTestLoader3D(cs, group_cases), d, patch_size=P, patch_batch=patch_batch)
        got = _tree(d)
        assert sorted(got) == sorted(want), (kind, group_cases, patch_batch)
        for k in want:
            if k != "metrics.json":
                assert got[k] == want[k], (kind, group_cases, patch_batch, k)
        assert json.loads(got["metrics.json"]) == json.loads(want["metrics.json"]), (kind, group_cases, patch_batch)
        assert list(res) == ["c16", "c1632", "c32"] and res == {k: v for k, v in json.loads(got["metrics.json"]).items() if k != "mean"}
    m = json.loads(want["metrics.json"])
    assert {"loss", "dice", "ged"} <= set(m["c16"]) and "mean" in m


def test_run_test_3d_mc_dropout_equals_the_restated_batching(tmp_path, dropout_model):
    from values_amd import predict_logits, run_test_3d
    from values_amd.dataset3d import DeviceTestLoader3D
    from values_amd.predict import derive_seed
    from values_amd.sliding import predict_split_3d
    cs = _split(tmp_path)
    kw = dict(n_pred=3, seeds=[7], patch_size=P, patch_batch=3)
    runs = []
    for i in range(2):
        with DeviceTestLoader3D(cs, 3) as loader:
            runs.append({c["image_id"]: (c["softmax_sum"].clone(), c["num_predictions"].clone(), {k: v.clone() for k, v in c["maps"].items()})
                         for c in predict_split_3d([dropout_model], loader, **kw)})
    for k in runs[0]:
        assert torch.equal(runs[0][k][0], runs[1][k][0]) and torch.equal(runs[0][k][1], runs[1][k][1]), k
        for name in runs[0][k][2]:
            assert torch.equal(runs[0][k][2][name], runs[1][k][2][name]), (k, name)
    # the batching, restated: the split's crop list in batches of three, batch k under derive_seed(7, 1, k), every patch
    # accumulated into its own image by the existing per-image call
    imgs = {c["image_id"]: np.load(c["image_path"]) for c in cs}
    patches = [(c["image_id"], crop) for c in cs for crop in c["crops"]]
    sums = {n: torch.zeros((3, 2) + imgs[n].shape, device="cuda") for n in imgs}
    cnts = {n: torch.zeros(imgs[n].shape, device="cuda") for n in imgs}
    for k, b0 in enumerate(range(0, len(patches), 3)):
        batch = patches[b0:b0 + 3]
        x = np.stack([imgs[n][tuple(slice(a, b) for a, b in crop)].astype(np.float32) for n, crop in batch])[:, None]
        logits = predict_logits([dropout_model], torch.from_numpy(x).cuda(), n_pred=3, seeds=[derive_seed(7, 1, k)])
        for n in imgs:
            idx = [i for i, (m, _) in enumerate(batch) if m == n]
            if idx:
                _old_accumulate(logits[idx], [[a for a, _ in batch[i][1]] for i in idx], sums[n], cnts[n], False)
    assert len(patches) == 5
    for n in imgs:
        assert torch.equal(runs[0][n][0], sums[n]) and torch.equal(runs[0][n][1], cnts[n]), n
    assert (sums["c32"][0] != sums["c32"][1]).any()                     # the passes differ: dropout was drawn
    # the T > 1 file set
    d = str(tmp_path / "mc")
    with DeviceTestLoader3D(cs, 3) as loader:
        run_test_3d([dropout_model], loader, d, **kw)
    got = _tree(d)
    for n in imgs:
        for sub in ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty"):
            assert os.path.join(sub, n + ".nii.gz") in got
        assert os.path.join("pred_seg", n + "_mean.nii.gz") in got and os.path.join("pred_prob", n + "_mean_02.nii.gz") in got
        assert os.path.join("pred_seg", n + "_03.nii.gz") in got and os.path.join("pred_prob", n + "_03_02.nii.gz") in got
    assert len(got) == 3 * (1 + 2 + 4 * (1 + 2) + 3) + 1


def test_run_test_3d_tta_does_not_depend_on_the_batching(tmp_path, members):
    from values_amd.dataset3d import DeviceTestLoader3D
    from values_amd.sliding import predict_split_3d
    cs = _split(tmp_path)
    runs = []
    for patch_batch, group_cases in ((2, 3), (32, 3), (2, 1)):
        with DeviceTestLoader3D(cs, group_cases) as loader:
            runs.append({c["image_id"]: c["softmax_sum"].clone() for c in
                         predict_split_3d(members[:1], loader, tta=True, noise_seed=5, patch_size=P, patch_batch=patch_batch)})
    for n in runs[0]:
        assert runs[0][n].shape[0] == 16
        assert torch.equal(runs[0][n], runs[1][n]) and torch.equal(runs[0][n], runs[2][n]), n
    assert (runs[0]["c16"][0] != runs[0]["c16"][8]).any()               # the noisy views differ from the plain ones


def test_run_test_3d_single_pass_writes_one_minus_max_softmax(tmp_path, members):
    from values_amd import nifti, run_test_3d
    from values_amd.dataset3d import DeviceTestLoader3D
    from values_amd.sliding import predict_split_3d
    cs = _split(tmp_path)
    d = str(tmp_path / "t1")
    with DeviceTestLoader3D(cs, 3) as loader:
        run_test_3d(members[:1], loader, d, patch_size=P)
    with DeviceTestLoader3D(cs, 3) as loader:
        sums = {c["image_id"]: (c["softmax_sum"].clone(), c["num_predictions"].clone()) for c in predict_split_3d(members[:1], loader, patch_size=P)}
    got = _tree(d)
    assert not [k for k in got if k.startswith(("aleatoric", "epistemic")) or "_mean" in k]
    assert not os.path.exists(os.path.join(d, "aleatoric_uncertainty")) and not os.path.exists(os.path.join(d, "epistemic_uncertainty"))
    assert len(got) == 3 * (1 + 2 + (1 + 2) + 1) + 1
    for n, (ssum, cnt) in sums.items():
        assert ssum.shape[0] == 1
        pe, _ = nifti.load(os.path.join(d, "pred_entropy", n + ".nii.gz"))
        prob = ssum[0] / cnt.clamp(min=1)
        want = (1 - prob.max(0).values).cpu().numpy()
        assert pe.dtype == np.float32 and np.array_equal(pe, want), n
    assert (nifti.load(os.path.join(d, "pred_entropy", "c1632.nii.gz"))[0][:, :, 16:] == 1).all()   # no patch: 1 - 0


def test_run_test_3d_overlapping_patches(tmp_path, members):
    from values_amd import nifti, run_test_3d
    from values_amd.dataset3d import DeviceTestLoader3D, compose_case
    from values_amd.sliding import predict_split_3d
    cs = _split(tmp_path, names=["c24"], overlap=0.5)
    assert len(cs) == 1 and len(cs[0]["crops"]) == 8
    ref = _per_case_route(members, cs, str(tmp_path / "ref"), overlap=0.5)["c24"][0]
    with DeviceTestLoader3D(cs, 1) as loader:
        (case,) = list(predict_split_3d(members, loader, patch_size=P, patch_overlap=0.5, patch_batch=3))
    cnt = case["num_predictions"]
    assert cnt.max().item() == 8 and torch.equal(cnt, ref["num_predictions"])
    n = cnt.double()
    bound = 2 * (n - 1) * n * 2.0 ** -24
    diff = (case["softmax_sum"].double() - ref["softmax_sum"].double()).abs()
    print("overlap 0.5: max |sum - per-case sum| =", diff.max().item(), "max bound", bound.max().item())
    assert (diff <= bound[None, None]).all()
    d = str(tmp_path / "run")
    with DeviceTestLoader3D(cs, 1) as loader:
        run_test_3d(members, loader, d, patch_size=P, patch_overlap=0.5, patch_batch=3)
    comp = compose_case(np.load(cs[0]["image_path"]), [np.load(p) for p in cs[0]["label_paths"]], cs[0]["crops"])
    data, _ = nifti.load(os.path.join(d, "input", "c24.nii.gz"))
    assert data.dtype == np.float64 and np.array_equal(data, comp["data"])
    for r in range(2):
        g, _ = nifti.load(os.path.join(d, "gt_seg", f"c24_{r:02d}.nii.gz"))
        assert g.dtype == np.float64 and np.array_equal(g, comp["gt_seg"][r])
    want, got = _tree(str(tmp_path / "ref")), _tree(d)
    for k in want:
        if k.startswith(("input", "gt_seg")):
            assert got[k] == want[k], k
