"""GPU: aggregation.aggregate_batch and the three per-image functions of values_amd.aggregation (a batch of one through the
same vx_aggregate_batched) against the host restatement of the documented summation order (tests/agg_restated.py).
Equality is exact (`==` on the result dicts).  Shapes are the smallest that reach every path of the box kernel: maps below
one tile, tiles cut in every axis, chunks along D, a single output element, 2D maps (no ring), float32 and float64 maps in
one call; the wide-range maps are the ones whose float64 sums depend on the order of the adds."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import agg_restated as ar

pytestmark = pytest.mark.gpu

A = "values_amd.aggregation."
REF = "evaluation.uncertainty_aggregation.aggregate_uncertainties."


def _patch(size, mean=False, target=A):
    return {"_target_": target + "patch_level_aggregation", "patch_size": size, "mean": mean}


def _image(mean=False):
    return {"_target_": A + "image_level_aggregation", "mean": mean}


def _thr(thr, mean=True):
    return {"_target_": A + "threshold_aggregation", "threshold": thr, "mean": mean}


def _per_image(images, aggs, **kw):
    from values_amd.io import instantiate
    kw = {"pred_model": None, "unc_type": None, **kw}
    return [{name: instantiate(dict(cfg), image=im, **kw) for name, cfg in aggs.items()} for im in images]


def _maps(shapes, seed, f64_every=3):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k, s in enumerate(shapes):
        m = torch.rand(s, generator=g, dtype=torch.float32)
        out.append(m.double() + 1e-9 if k % f64_every == 1 else m)   # (a float64 map that float32 does not hold exactly)
    return out


def test_box_shapes_match_per_image():
    from values_amd.aggregation import aggregate_batch
    groups = [
        # 3D maps both patches fit: below one tile, a cut tile in H and W, three chunks along D with cut tiles in every axis
        ([(7, 9, 11), (12, 10, 33), (19, 37, 70), (23, 37, 70)],
         {"p3": _patch(3), "p3m": _patch(3, True), "pt": _patch([5, 4, 10]), "ptm": _patch((5, 4, 10), True, REF)}),
        ([(5, 5, 5), (7, 9, 11)], {"p5": _patch(5), "p5m": _patch(5, True), "p3": _patch(3)}),       # one output element
        ([(12, 10, 33), (19, 37, 70), (23, 37, 70)], {"p10": _patch(10), "p10m": _patch(10, True)}),
        ([(13, 70), (150, 301)], {"p10": _patch(10), "p10m": _patch(10, True), "p1": _patch(1), "pt": _patch([3, 7])}),
        ([(6, 5), (13, 70)], {"p1": _patch(1), "p1m": _patch(1, True)}),
    ]
    for k, (shapes, aggs) in enumerate(groups):
        maps = [m.cuda() for m in _maps(shapes, seed=k)]
        got = aggregate_batch(maps, aggs)
        want = ar.restated(maps, aggs)
        assert got == want, (k, got, want)
        assert _per_image(maps, aggs) == want, k
        for g, m in zip(got, maps):
            for name, r in g.items():
                assert len(r["bounding_box"]) == m.dim() and all(type(v) is int for bb in r["bounding_box"] for v in bb)


@pytest.mark.parametrize("shape", [(8, 30, 100), (40, 150)])
def test_ties_and_the_isclose_quirk(shape):
    """a constant map: index zero; two equal maxima in different tiles, the C-order-first one in the LATER tile: it wins; a
    strict maximum later in C order with an earlier box sum inside 1e-8 + 1e-5 |max| of it: the earlier index is reported"""
    from values_amd.aggregation import aggregate_batch
    nd = len(shape)
    early = (2, 25, 10) if nd == 3 else (20, 140)     # its first box lies in tile (h 1, w 0) of 3D, (h 0, w 2) of 2D
    late = (4, 5, 90) if nd == 3 else (22, 10)        # ... in tile (h 0, w 1) of 3D, (h 0, w 0) of 2D: an earlier tile
    const = torch.full(shape, 0.25)
    tie = torch.zeros(shape)
    tie[early] = 1.0
    tie[late] = 1.0
    quirk = torch.zeros(shape)
    quirk[early] = 1.0
    quirk[late] = 1.0 + 5e-6
    maps = [const.cuda(), tie.cuda(), quirk.cuda(), quirk.double().cuda()]
    aggs = {"p3": _patch(3), "p3m": _patch(3, True)}
    got = aggregate_batch(maps, aggs)
    assert got == ar.restated(maps, aggs)
    assert _per_image(maps, aggs) == ar.restated(maps, aggs)
    assert got[0]["p3"]["bounding_box"] == [(0, 3)] * nd
    first = [(max(i - 2, 0), max(i - 2, 0) + 3) for i in early]
    assert got[1]["p3"]["bounding_box"] == first and got[1]["p3"]["max_score"] == 1.0
    assert got[2]["p3"]["bounding_box"] == first and got[2]["p3"]["max_score"] == float(np.float32(1.0 + 5e-6))


def test_sums_and_thresholds_match_per_image():
    from values_amd.aggregation import aggregate_batch
    shapes = [(1, 1), (8, 125), (32, 32), (25, 41), (11, 467)]        # n = 1, 1000, 1024, 1025, 5 * 1024 + 17
    maps = [m.cuda() for m in _maps(shapes, seed=7, f64_every=2)]
    assert [m.dtype for m in maps] == [torch.float32, torch.float64, torch.float32, torch.float64, torch.float32]
    equal = float(maps[4].flatten()[4000])
    # float64 values a fraction of a float32 ulp either side of the threshold: a float32 comparison counts all three
    near = torch.tensor([[0.3 - 1e-9, 0.3 + 1e-9, 0.3, 0.1]], dtype=torch.float64).cuda()
    maps.append(near)
    aggs = {"sum": _image(), "mean": _image(True), "none": _thr(2.0), "none_sum": _thr(2.0, False), "eq": _thr(equal),
            "eq_sum": _thr(equal, False), "t3": _thr(0.3, False), "t3m": _thr(0.3)}
    got = aggregate_batch(maps, aggs)
    assert got == ar.restated(maps, aggs)
    assert _per_image(maps, aggs) == ar.restated(maps, aggs)
    assert all(g["none"] == {"max_score": 0.0, "threshold": 2.0} for g in got)
    assert type(got[0]["mean"]) is float and got[0]["sum"] == {"max_score": float(maps[0].sum())}
    assert got[5]["t3"]["max_score"] == (0.3 + 1e-9) + 0.3 and got[5]["t3m"]["max_score"] == ((0.3 + 1e-9) + 0.3) / 2
    assert got[4]["eq_sum"]["max_score"] >= equal


def test_results_do_not_depend_on_the_batch(monkeypatch):
    from values_amd import _lib
    from values_amd.aggregation import aggregate_batch
    rng = np.random.default_rng(3)
    shapes = [tuple(int(v) for v in rng.integers(6, 30, 3)) for _ in range(35)]
    probe = _maps([(17, 21, 70)], seed=11)[0].numpy()
    others = [m.numpy() for m in _maps(shapes, seed=12)]
    aggs = {"p3": _patch(3), "p4m": _patch([4, 2, 5], True), "sum": _image(), "thr": _thr(0.5), "thr2": _thr(0.25, False)}
    alone = aggregate_batch([probe], aggs)
    assert alone == ar.restated([probe], aggs)
    assert _per_image([probe], aggs) == ar.restated([probe], aggs)
    batch = [probe] + others + [probe]
    assert len(batch) == 37
    full = aggregate_batch(batch, aggs)
    assert full[0] == alone[0] and full[-1] == alone[0]
    lib = _lib.load()
    calls = []
    real = lib.vx_aggregate_batched
    monkeypatch.setattr(lib, "vx_aggregate_batched", lambda *a: (calls.append(a[1]), real(*a))[1])
    chunked = aggregate_batch(batch, aggs, budget_bytes=200_000)
    assert len(calls) > 3 and sum(calls) == 37
    assert chunked == full


def test_wide_range_maps_pin_the_order_of_the_adds():
    """float32 values in [0, 1) have exact float64 sums in any order; these maps span 60 binades, and each one's own
    sensitivity is asserted on the host first (tests/test_aggregate_batched_cpu.py asserts the same without a device)"""
    from values_amd.aggregation import aggregate_batch
    for shape, patch, seed in ar.WIDE_BOX:
        m32, m64 = ar.wide_range(shape, seed), ar.wide_range(shape, seed, np.float64)
        full = len(shape) * [patch] if type(patch) == int else patch
        assert ar.box_max(m32, full)[0] != ar.box_max(m32, full, descending=True)[0]
        maps = [torch.from_numpy(m32).cuda(), torch.from_numpy(m64).cuda()]
        aggs = {"p": _patch(patch), "pm": _patch(patch, True)}
        want = ar.restated(maps, aggs)
        assert aggregate_batch(maps, aggs) == want, shape
        assert _per_image(maps, aggs) == want, shape
    for shape, dtype, seed, thr in ar.WIDE_SUMS:
        m = ar.wide_range(shape, seed, dtype)
        x = m.astype(np.float64)
        s, st, _ = ar.sums(m, thr)
        assert s != float(np.sum(x)) and st != float(np.sum(x[x >= thr]))
        maps = [torch.from_numpy(m).cuda()]
        aggs = {"sum": _image(), "mean": _image(True), "t": _thr(thr), "t_sum": _thr(thr, False)}
        want = ar.restated(maps, aggs)
        assert want[0]["sum"]["max_score"] == s and want[0]["t_sum"]["max_score"] == st
        assert aggregate_batch(maps, aggs) == want, shape
        assert _per_image(maps, aggs) == want, shape


def test_per_image_surface(tmp_path):
    """the three functions called directly: input kinds, patch_size spellings, ranks, what they raise"""
    from values_amd import _lib
    from values_amd.aggregation import image_level_aggregation, patch_level_aggregation, threshold_aggregation
    base = np.random.default_rng(9).random((9, 12, 14))
    inputs = [base, torch.from_numpy(base).half(), torch.from_numpy(base).float().cuda()]
    assert inputs[0].dtype == np.float64 and not inputs[1].is_cuda
    thr = np.float32(0.5)
    for im in inputs:
        for ps in (3, [3, 2, 4], (3, 2, 4), [np.int64(3), np.int64(2), np.int64(4)]):
            for mean in (False, True):
                got = patch_level_aggregation(im, ps, mean)
                assert got == ar.patch_level_aggregation(im, ps, mean), (type(im), ps, mean)
                assert type(got["max_score"]) is float and all(type(v) is int for bb in got["bounding_box"] for v in bb)
        assert patch_level_aggregation(im, patch_size=3, mean=True, pred_model="x", unc_type="y") == ar.patch_level_aggregation(im, 3, True)
        assert image_level_aggregation(im) == ar.image_level_aggregation(im)
        mean = image_level_aggregation(im, mean=True, unc_type="y")
        assert type(mean) is float and mean == ar.image_level_aggregation(im, mean=True)
        for mn in (True, False):
            got = threshold_aggregation(im, threshold=thr, mean=mn)
            assert got == ar.threshold_aggregation(im, thr, mn) and got["threshold"] is thr
    with pytest.raises(TypeError):
        patch_level_aggregation(base, np.int64(3))       # (not an `int` to the reference either: no expansion to the rank)
    for im in (np.random.default_rng(10).random(5000), torch.rand(2, 3, 5, 7).cuda()):      # _dhw: rank 1, rank 4
        assert image_level_aggregation(im) == ar.image_level_aggregation(im)
        assert image_level_aggregation(im, mean=True) == ar.image_level_aggregation(im, mean=True)
        assert threshold_aggregation(im, threshold=0.25) == ar.threshold_aggregation(im, 0.25)
    # what stays: the rank of a patch map, the two threshold exceptions
    with pytest.raises(ValueError, match="^patch_level_aggregation: 2D or 3D maps only$"):
        patch_level_aggregation(torch.rand(2, 3, 5, 7).cuda(), 2)
    with pytest.raises(Exception, match="^A threshold needs to be provided for threshold aggregation!$"):
        threshold_aggregation(base)
    (tmp_path / "thr.json").write_text(json.dumps({"Dropout": {"Mean predictive threshold": 0.5}}))
    with pytest.raises(Exception, match="^If you want to load the threshold from a json file, you have to provide the prediction "
                                        "model and the uncertainty type$"):
        threshold_aggregation(base, threshold_path=str(tmp_path / "thr.json"), pred_model="Dropout")
    got = threshold_aggregation(base, threshold_path=str(tmp_path / "thr.json"), pred_model="Dropout", unc_type="predictive_uncertainty")
    assert got == ar.threshold_aggregation(base, 0.5)
    # what changed with vx_version 810: all four are refusals of the one device path
    with pytest.raises(_lib.VxError, match=r"vx_aggregate_batched failed \(rc=-2\).*item 0: patch \(1,13,3\) of spec 0 must fit map \(1,12,14\)"):
        patch_level_aggregation(base[0], [13, 3])
    with pytest.raises(ValueError, match=r"patch_size \[3, 3\] for a map of rank 3"):
        patch_level_aggregation(base, [3, 3])
    with pytest.raises(_lib.VxError, match=r"rc=-2.*leaves no LDS tile"):
        patch_level_aggregation(torch.rand(210, 205).cuda(), 200)     # 200 * 200 floats of halo: more than 156 KB at a 1 x 1 tile
    for empty in (np.zeros((0, 5), np.float32), torch.zeros(3, 0, 2).cuda()):
        with pytest.raises(_lib.VxError, match=r"rc=-2.*item 0: map"):
            image_level_aggregation(empty)
        with pytest.raises(_lib.VxError, match=r"rc=-2.*item 0: map"):
            threshold_aggregation(empty, threshold=0.5)


def _lidc_tree(root, n=3):
    from values_amd.results import ResultsWriter, results_dir
    d = results_dir(str(root), "Dropout", "fold0_seed123", "id")
    with ResultsWriter(workers=2) as w:
        for i in range(n):
            g = torch.Generator(device="cuda").manual_seed(i)
            sm = torch.softmax(torch.randn(3, 2, 20, 24, 16, device="cuda", generator=g) * 3, 1)
            maps = {k: torch.rand(20, 24, 16, device="cuda", generator=g) * 0.5 for k in
                    ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")}
            gt = torch.rand(2, 20, 24, 16, generator=torch.Generator().manual_seed(i)) > 0.8
            w.submit(d, f"case{i}", softmax_pred=sm, maps=maps, data=sm[0, 0].cpu().numpy(), gt_seg=gt)
    return d


def _tree_check(ev, split, aggs, monkeypatch, n):
    from values_amd import aggregation
    from values_amd.experiment import (DeviceExperimentDataloader, ExperimentDataloader, aggregate_uncertainties,
                                       aggregate_uncertainties_device)
    host, dev = ExperimentDataloader(ev, split), DeviceExperimentDataloader(ev, split)
    aggregate_uncertainties(host, aggs)
    want = {u: open(host.dataset_path / f"aggregated_{u}.json", "rb").read() for u in ev.unc_types}
    for u in ev.unc_types:
        os.remove(host.dataset_path / f"aggregated_{u}.json")
    calls = []
    real = aggregation.aggregate_batch
    monkeypatch.setattr(aggregation, "aggregate_batch", lambda images, *a, **k: (calls.append(len(images)), real(images, *a, **k))[1])
    aggregate_uncertainties_device(dev, aggs, batch=2)
    assert len(calls) <= math.ceil(n / 2) * len(ev.unc_types) and sum(calls) == n * len(ev.unc_types)
    for u in ev.unc_types:
        assert open(host.dataset_path / f"aggregated_{u}.json", "rb").read() == want[u], u


def test_tree_3d_byte_equal_and_launch_economy(tmp_path, monkeypatch):
    from values_amd.experiment import ExperimentVersion
    _lidc_tree(tmp_path)
    thr_file = tmp_path / "thresholds.json"
    thr_file.write_text(json.dumps({"Dropout": {"Mean predictive threshold": 0.21, "Mean aleatoric threshold": 0.3,
                                                "Mean epistemic threshold": 0.4}}))
    ev = ExperimentVersion(base_path=tmp_path, naming_scheme_version="fold{fold}_seed{seed}", pred_model="Dropout",
                           image_ending=".nii.gz", unc_ending=".nii.gz",
                           unc_types=["predictive_uncertainty", "aleatoric_uncertainty", "epistemic_uncertainty"],
                           aggregations=None, n_reference_segs=2, fold=0, seed=123)
    aggs = {"patch_level": _patch(5, target=REF), "image_level": _image(True), "threshold": _thr(0.2),
            "threshold_file": {"_target_": A + "threshold_aggregation", "threshold_path": str(thr_file)}}
    _tree_check(ev, "id", aggs, monkeypatch, 3)


def test_tree_2d_tiff_byte_equal_and_launch_economy(tmp_path, monkeypatch):
    from values_amd import results2d
    from values_amd.experiment import ExperimentVersion
    rng = np.random.default_rng(5)
    ids, T, H, W = ["img_a", "img_b", "img_c"], 2, 20, 33
    pm = torch.from_numpy(rng.integers(0, 24, (3, T, H, W)).astype(np.uint8)).cuda()
    mm = torch.from_numpy(rng.integers(0, 24, (3, H, W)).astype(np.uint8)).cuda()
    names = ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")
    unc = {k: torch.from_numpy(rng.random((3, H, W), dtype=np.float32)).cuda() for k in names}
    ev = ExperimentVersion(base_path=tmp_path, naming_scheme_version="seed{seed}", pred_model="Dropout", image_ending=".png",
                           unc_ending=".tif", unc_types=["predictive_uncertainty", "aleatoric_uncertainty", "epistemic_uncertainty"],
                           aggregations=None, n_reference_segs=1, seed=7)
    results2d.save_images_device(str(ev.exp_path / "val"), ids, pm, mm, unc)
    aggs = {"patch_level": _patch(5), "patch_mean": _patch([4, 7], True), "image_level": _image(True), "threshold": _thr(0.6)}
    _tree_check(ev, "val", aggs, monkeypatch, 3)


def test_errors(monkeypatch, tmp_path):
    import ctypes as C
    from values_amd import _lib
    from values_amd.aggregation import aggregate_batch, threshold_aggregation
    lib = _lib.load()
    maps = [torch.rand(6, 7, 8).cuda(), torch.rand(4, 9, 9).cuda()]
    with pytest.raises(_lib.VxError, match="image 1"):
        aggregate_batch(maps, {"p": _patch(5)})
    # the library's own refusals, before any launch
    items = (_lib.AggItem * 2)(*[_lib.AggItem(m.data_ptr(), _lib.VX_F32, *m.shape) for m in maps])
    spec = (_lib.AggSpec * 9)(*[_lib.AggSpec(_lib.VX_AGG_PATCH, 5, 5, 5, 0.0)] * 9)
    out = torch.empty((2, 9, 4), dtype=torch.float64, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    assert lib.vx_aggregate_batched(items, 2, spec, 1, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()) == -2
    assert b"item 1" in lib.vx_last_error_string()
    assert lib.vx_aggregate_workspace_bytes(items, 2, spec, 1) == 0
    spec[0] = _lib.AggSpec(_lib.VX_AGG_IMAGE, 1, 1, 1, 0.0)
    assert lib.vx_aggregate_batched(items, 2, spec, 9, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()) == -2
    with pytest.raises(_lib.VxError, match="rc=-2"):
        aggregate_batch(maps, {f"t{k}": _thr(0.1 * k) for k in range(9)})
    # an empty list: no launch
    monkeypatch.setattr(lib, "vx_aggregate_batched", lambda *a: pytest.fail("launched for an empty list"))
    assert aggregate_batch([], {"p": _patch(5)}) == []
    monkeypatch.undo()
    # the threshold that cannot be resolved: threshold_aggregation's own two exceptions
    (tmp_path / "thr.json").write_text(json.dumps({"Dropout": {}}))
    for cfg, kw in (({}, {}), ({"threshold_path": str(tmp_path / "thr.json")}, {"pred_model": "Dropout"})):
        with pytest.raises(Exception) as want:
            threshold_aggregation(maps[0], **cfg, **kw)
        with pytest.raises(Exception) as got:
            aggregate_batch(maps, {"t": {"_target_": A + "threshold_aggregation", **cfg}}, **kw)
        assert type(got.value) is type(want.value) is Exception and str(got.value) == str(want.value)


def test_case_maps_against_the_oracle():
    """the reference's own arithmetic (oracle/aggregation_oracle.py) on a 3D and a 2D map: the sums within rel 1e-6, the
    bounding box exactly (the tolerances tests/test_gpu_results.py uses for the per-image functions)"""
    from oracle import aggregation_oracle as ao
    from values_amd.aggregation import aggregate_batch
    for shape, patch in (((19, 37, 70), 10), ((150, 301), 10)):
        m = _maps([shape], seed=21)[0]
        got = aggregate_batch([m.cuda()], {"p": _patch(patch), "i": _image(), "t": _thr(0.5)})[0]
        ref = m.double().numpy()         # (the same values: the oracle's own sums then carry no float32 rounding)
        want = ao.patch_level_aggregation(ref, patch)
        assert got["p"]["bounding_box"] == [tuple(int(v) for v in bb) for bb in want["bounding_box"]]
        assert got["p"]["max_score"] == pytest.approx(want["max_score"], rel=1e-6)
        assert got["i"]["max_score"] == pytest.approx(ao.image_level_aggregation(ref)["max_score"], rel=1e-6)
        assert got["t"]["max_score"] == pytest.approx(ao.threshold_aggregation(ref, threshold=0.5)["max_score"], rel=1e-6)
