"""GPU: the batched evaluation scores (values_amd/csrc/evalmetrics.hip, evalmetrics.ncc_batch /
sigmoid_calibration_batch / calc_ace_batch and the *_device drivers) against the per-image functions and a host
restatement of the documented association: every number equal with `==`, every JSON file byte for byte.  The sizes sit
where the shared association could break (one element, one short of a wave row, exactly / one more than one element per
thread of the 512 x 256 grid, several rounds of the grid)."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests.em_inputs import ncc_sums_restated, platt_items, rater_label_cases
from tests.helpers import load_npz

pytestmark = pytest.mark.gpu

NCC_SIZES = (1, 2, 255, 131072, 131073, 300001)


@pytest.fixture(scope="module")
def ncc_pairs():
    rng = np.random.default_rng(17)
    dts = ((np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64))
    pairs = []
    for k, n in enumerate(NCC_SIZES):
        dg, dp = dts[k % 4]
        g = rng.random(n).astype(dg)
        pairs.append((g, (0.6 * g + 0.4 * rng.random(n)).astype(dp)))
    pairs.append((np.full(255, 0.25, dtype=np.float32), rng.random(255)))          # a constant map: the host path gives nan
    single = [ncc_sums_restated(g, p) for g, p in pairs]
    return pairs, single


def test_ncc_batch_equals_compute_ncc(ncc_pairs):
    from values_amd.evalmetrics import _ncc_sums_batch, compute_ncc, ncc_batch
    pairs, single = ncc_pairs
    gts, preds = [g for g, _ in pairs], [p for _, p in pairs]
    rows = _ncc_sums_batch(gts, preds)
    for i, ((n, row), want) in enumerate(zip(rows, single)):
        assert n == len(gts[i]) and np.array_equal(np.array(row), np.array(want), equal_nan=True), (i, row, want)
    # one element: compute_ncc divides by n - 1 = 0 in Python floats and raises; so does the batch that holds such a pair
    with pytest.raises(ZeroDivisionError):
        compute_ncc(*pairs[0])
    with pytest.raises(ZeroDivisionError):
        ncc_batch(gts, preds)
    got = ncc_batch(gts[1:], preds[1:])
    want = [compute_ncc(g, p) for g, p in pairs[1:]]
    assert len(got) == len(want) and all(type(v) is np.float64 for v in got)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b, equal_nan=True), (i, a, b)
    assert np.isnan(got[-1]) and abs(abs(got[0]) - 0.5) < 1e-12 and all(0.5 < v < 1.0 for v in got[1:-1])   # (two elements: +-1/2)
    assert ncc_batch([], []) == []
    with pytest.raises(ValueError, match="pair 1"):
        ncc_batch([gts[1], gts[2]], [preds[1], preds[3]])
    # device tensors are taken where they lie, host and device inputs mix
    dev_got = ncc_batch([torch.from_numpy(g).cuda() for g in gts[1:4]], [preds[1], torch.from_numpy(preds[2]).cuda(), preds[3]])
    assert dev_got == got[:3]


def test_ncc_item_does_not_depend_on_its_batch_mates(ncc_pairs):
    from values_amd.evalmetrics import _ncc_sums_batch
    pairs, single = ncc_pairs
    for k in (0, 3, 5):
        g, p = pairs[k]
        others = [pairs[j] for j in (1, 2, 6)]
        alone = _ncc_sums_batch([g], [p])[0][1]
        first = _ncc_sums_batch([g] + [o[0] for o in others], [p] + [o[1] for o in others])[0][1]
        last = _ncc_sums_batch([o[0] for o in others] + [g], [o[1] for o in others] + [p])[-1][1]
        assert alone == first == last == single[k], k


def test_rater_variance_and_rater_stack_ncc():
    from values_amd.evalmetrics import compute_ncc, ncc_batch, rater_variance
    rng = np.random.default_rng(23)
    stacks, preds = [], []
    for labels in rater_label_cases():
        want = np.var(labels, axis=0)
        got = rater_variance(labels)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == labels.shape[1:]
        assert np.array_equal(got.cpu().numpy(), want), labels.shape
        assert np.array_equal(rater_variance(torch.from_numpy(labels.astype(np.uint8)).cuda()).cpu().numpy(), want)
        stacks.append(labels if len(stacks) % 2 else torch.from_numpy(labels.astype(np.uint8)).cuda())
        preds.append((want + 0.3 * rng.random(want.shape)).astype(np.float32 if len(preds) % 2 else np.float64))
    got = ncc_batch(stacks, preds)
    for labels, p, v in zip(rater_label_cases(), preds, got):
        with np.errstate(divide="ignore", invalid="ignore"):
            want = compute_ncc(np.var(labels, axis=0), p)
        assert np.array_equal(v, want, equal_nan=True), (labels.shape, v, want)        # (one rater: a zero map, nan)
    assert sum(np.isnan(v) for v in got) == 2 and all(v > 0.5 for v in got[2:])


def _rater_case(rng, R, nvox, dtype):
    pred = rng.integers(0, 3, nvox).astype(np.int32)
    ref = np.where(rng.random((R, nvox)) < 0.7, pred[None], rng.integers(0, 3, (R, nvox))).astype(np.int32)
    unc = (0.6 * (ref != pred[None]).mean(0) + 0.4 * rng.random(nvox)).astype(dtype)
    return ref, pred, unc


@pytest.mark.parametrize("ignore", [None, 2])
def test_platt_sums_and_bins_batched_equal_the_per_image_calls(ignore):
    """pins batch independence: an item's 8 + 63 numbers are the same bits alone, first, last, and among other parameters
    (the per-image functions are a batch of one through the same entry point, so this compares the kernel with itself).
    The VALUES are pinned in tests/test_gpu_evalmetrics_matrix.py, against the long double reference of tests/em_ref.py"""
    from values_amd import _lib, evalmetrics as vm
    lib = _lib.load()
    rng = np.random.default_rng(29)
    cases = [_rater_case(rng, R, nvox, np.float32 if (R + nvox) % 2 else np.float64) for R in (1, 4) for nvox in (1, 257, 131073)]
    big = [1, 2, 4, 5]                                               # the items of more than one voxel
    assert all((cases[i][0] == 2).any() for i in big)                # the ignored label occurs
    xs = [vm._RaterInputs(*c, ignore) for c in cases]
    params = [(-1.5 - 0.5 * i, 0.25 * i - 0.5, 0.9 - 0.01 * i, 0.05 + 0.01 * i) for i in range(len(xs))]
    got = np.array(vm._platt_sums_batch(xs, params))
    want = np.array([vm._platt_sums(x, *p) for x, p in zip(xs, params)])
    assert got.shape == (6, 8) and np.array_equal(got, want), (got, want)
    assert (want[big, 0] > 0).all() and len({tuple(r) for r in want[big].tolist()}) == 4
    # an item alone, and in another position with other parameters around it
    assert vm._platt_sums_batch([xs[5]], [params[5]]) == [want[5].tolist()]
    assert vm._platt_sums_batch([xs[5], xs[1]], [params[5], params[0]])[0] == want[5].tolist()

    dev, st = xs[0].dev, _lib.stream_ptr()
    edges = (C.c_double * 21)(*np.linspace(0.0, 1.0 + 1e-8, 21).tolist())
    ign = -1 if ignore is None else ignore
    single = torch.empty((len(xs), 63), dtype=torch.float64, device=dev)
    for i, (x, p) in enumerate(zip(xs, params)):               # every item as a call of its own
        one = vm._em_items([x])
        ws = _lib.workspace(dev, lib.vx_calib_batched_workspace_bytes(one, 1))
        _lib.check(lib.vx_calib_bins_batched(one, 1, (C.c_double * 2)(p[0], p[1]), edges, ign, _lib.ptr(single[i]), _lib.ptr(ws),
                                             ws.numel(), st), "vx_calib_bins_batched")
    items = vm._em_items(xs)
    ab = (C.c_double * 12)(*[v for p in params for v in p[:2]])
    ws = _lib.workspace(dev, lib.vx_calib_batched_workspace_bytes(items, len(xs)))
    out = torch.empty((len(xs), 63), dtype=torch.float64, device=dev)
    _lib.check(lib.vx_calib_bins_batched(items, len(xs), ab, edges, ign, _lib.ptr(out), _lib.ptr(ws), ws.numel(), st),
               "vx_calib_bins_batched")
    got, want = out.cpu().numpy(), single.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(want[:, 42:].sum(1), np.array(vm._platt_sums_batch(xs, params))[:, 0])    # every valid voxel in a bin
    assert (np.count_nonzero(want[4:, 42:], axis=1) >= 3).all()
    # the two counts are exact: numpy's number of valid rater-voxels and of correct ones; every correct one is in a bin
    sums = np.array(vm._platt_sums_batch(xs, params))
    valid = [np.ones_like(ref, dtype=bool) if ignore is None else ref != ignore for ref, _, _ in cases]
    assert np.array_equal(sums[:, 0], np.array([float(v.sum()) for v in valid]))
    assert np.array_equal(sums[:, 1], np.array([float((v & (ref == pred[None])).sum()) for v, (ref, pred, _) in zip(valid, cases)]))
    assert np.array_equal(got[:, 21:42].sum(1), sums[:, 1])


@pytest.fixture(scope="module")
def fit_cases():
    """the images of tests/em_inputs.platt_items as one-rater volumes, and the reference fixture's image"""
    cases = []
    for k, (unc, correct) in enumerate(platt_items()):
        pred = np.ones(len(unc), dtype=np.int32)
        ref = np.where(correct, 1, 0).astype(np.int32)[None]
        cases.append((ref, pred, unc.astype(np.float32) if k in (1, 3) else unc))
    g = load_npz("evalmetrics_kat.npz")
    cases.append((g["ace_ref"], g["ace_pred"], g["ace_unc"]))
    return cases


def test_lockstep_fit_and_ace_equal_the_per_image_functions(fit_cases, monkeypatch):
    from values_amd import evalmetrics as vm
    refs, preds, uncs = [c[0] for c in fit_cases], [c[1] for c in fit_cases], [c[2] for c in fit_cases]
    # the per-image path: its controller, fed by the per-image entry point
    single = []
    for r, p, u in fit_cases:
        x = vm._RaterInputs(r, p, u)
        single.append(vm._platt_fit_one(lambda A, B, tp, tn, x=x: vm._platt_sums(x, A, B, tp, tn)))
    want = [vm.sigmoid_calibration(r, p, u) for r, p, u in fit_cases]
    assert want == [f.result for f in single]
    lengths = [len(f.visited) for f in single]
    assert len(set(lengths)) >= 4, lengths                                        # they finish in different rounds
    assert [v[0] for v in single[0].visited] == ["counts", "start"]               # done in the first round
    for f in single[4:6]:
        assert min(v[3] for v in f.visited) < 1.0 and any(v[0] == "line_search" for v in f.visited)   # halved steps
    calls = []
    real = vm._platt_sums_batch
    monkeypatch.setattr(vm, "_platt_sums_batch", lambda xs, params: (calls.append(len(xs)), real(xs, params))[1])
    got = vm.sigmoid_calibration_batch(refs, preds, uncs)
    monkeypatch.undo()
    assert got == want, (got, want)
    # one device call per round, over the unfinished items only
    assert calls == [sum(n > k for n in lengths) for k in range(max(lengths))], (calls, lengths)
    # the fixture's image against the reference's optimum, with the tolerance of test_gpu_evalmetrics.py
    g = load_npz("evalmetrics_kat.npz")
    a, b = got[-1]
    assert abs(a - float(g["ace_all_a"])) < 2e-3 * abs(a) and abs(b - float(g["ace_all_b"])) < 2e-3 * abs(b), (a, b)
    got2 = vm.sigmoid_calibration_batch(refs[-1:], preds[-1:], uncs[-1:], ignore_value=2)
    assert got2 == [vm.sigmoid_calibration(refs[-1], preds[-1], uncs[-1], ignore_value=2)]
    assert vm.sigmoid_calibration_batch(refs[1:3], preds[1:3], uncs[1:3], max_iter=1) == \
        [vm.sigmoid_calibration(r, p, u, max_iter=1) for r, p, u in fit_cases[1:3]]

    a, b = float(g["ace_all_a"]), float(g["ace_all_b"])
    aces = vm.calc_ace_batch(refs, preds, uncs, a, b)
    want_ace = [vm.calc_ace(r, p, u, a, b) for r, p, u in fit_cases]
    assert aces == want_ace and all(type(v) is np.float64 for v in aces)
    assert abs(aces[-1] - float(g["ace_all"])) < 1e-13
    stats = vm.calib_stats_batch(refs, preds, uncs, a, b)
    for (d, w, k), (r, p, u) in zip(stats, fit_cases):
        d1, w1, k1 = vm.calib_stats(r, p, u, a, b)
        assert k == k1 and np.array_equal(d, d1) and np.array_equal(w, w1)
    # the single-label quirk comes from the shared host helper
    allcorrect = np.repeat(preds[-1][None], 2, 0)
    assert vm.calc_ace_batch([allcorrect, refs[-1]], [preds[-1]] * 2, [uncs[-1]] * 2, 2.0, -1.0, ignore_value=2) == \
        [vm.calc_ace(allcorrect, preds[-1], uncs[-1], 2.0, -1.0, ignore_value=2), vm.calc_ace(refs[-1], preds[-1], uncs[-1], 2.0, -1.0, ignore_value=2)]
    with pytest.raises(ValueError, match="no valid voxel"):
        vm.calc_ace_batch([np.full((1, 5), 2)], [np.zeros(5, dtype=np.int64)], [np.zeros(5)], 1.0, 0.0, ignore_value=2)
    with pytest.raises(ValueError, match="item 1"):
        vm.sigmoid_calibration_batch([refs[1], np.full((1, 5), 2)], [preds[1], np.zeros(5, dtype=np.int64)], [uncs[1], np.zeros(5)],
                                     ignore_value=2)


# --------------------------------------------------------------------------------------------------------- drivers
FILES = ("ambiguity_modeling.json", "platt_scale_params.json", "calibration.json")


def _json_bytes(ev, split):
    d = ev.exp_path / split
    return [open(p, "rb").read() for p in (d / FILES[0], ev.exp_path / FILES[1], d / FILES[2])]


class _Spy:
    """records what the scoring code moves to the host (.cpu() / .tolist() of a device tensor called from evalmetrics.py)
    and what _RaterInputs is given and keeps"""

    def __init__(self, monkeypatch):
        import sys
        from values_amd import evalmetrics as vm
        self.copies, self.inputs = [], []
        for name in ("cpu", "tolist"):
            real = getattr(torch.Tensor, name)

            def spy(t, *a, _real=real, **k):
                if t.is_cuda and sys._getframe(1).f_code.co_filename.endswith("evalmetrics.py"):
                    self.copies.append(t.numel())
                return _real(t, *a, **k)
            monkeypatch.setattr(torch.Tensor, name, spy)
        init = vm._RaterInputs.__init__

        def spy_init(x, ref, pred, unc, ignore_value=None):
            init(x, ref, pred, unc, ignore_value)
            self.inputs.append((vm._on_device(ref), vm._on_device(pred), vm._on_device(unc), x.ref.is_cuda and x.pred.is_cuda and x.unc.is_cuda))
        monkeypatch.setattr(vm._RaterInputs, "__init__", spy_init)


def test_device_drivers_write_the_host_drivers_files_3d(tmp_path, monkeypatch):
    from values_amd import evalmetrics as vm, nifti
    from values_amd.experiment import DeviceExperimentDataloader, ExperimentDataloader, ExperimentVersion
    rng = np.random.default_rng(31)
    types = ["predictive_uncertainty", "aleatoric_uncertainty"]
    mk = lambda base: ExperimentVersion(base_path=base, naming_scheme_version="fold{fold}", pred_model="Dropout", image_ending=".nii.gz",
                                        unc_ending=".nii.gz", unc_types=types, aggregations=None, n_reference_segs=3, fold=0)
    ev = mk(tmp_path / "host")
    S = (16, 16, 16)
    for split in ("val", "test"):
        d = ev.exp_path / split
        for sub in ("pred_seg", "pred_entropy", "aleatoric_uncertainty", "gt_seg"):
            (d / sub).mkdir(parents=True)
        for i in range(3):
            iid = f"case{i}"
            base = (rng.random(S) < 0.4).astype(np.uint8)
            segs = np.array([base ^ (rng.random(S) < 0.1 * (r + i)) for r in range(3)]).astype(np.uint8)
            segs = (segs * (1 + (rng.random(S) < 0.1))).astype(np.uint8)                      # labels 0, 1, 2
            pred = base.copy()
            pred[rng.random(S) < 0.15] ^= 1
            nifti.save(pred, d / "pred_seg" / f"{iid}_mean.nii.gz")
            for k, sub in enumerate(("pred_entropy", "aleatoric_uncertainty")):
                unc = ((0.5 + 0.2 * k) * segs.var(0) + (0.2 + 0.3 * i) * rng.random(S)).astype(np.float32)
                nifti.save(unc, d / sub / f"{iid}.nii.gz")
            for r in range(3):
                nifti.save(segs[r], d / "gt_seg" / f"{iid}_{r:02d}.nii.gz")
    shutil.copytree(tmp_path / "host", tmp_path / "dev")
    shutil.copytree(tmp_path / "host", tmp_path / "plain")
    for ign in (None, 2):
        host = ExperimentDataloader(ev, "test")
        vm.ambiguity_modeling(host)
        vm.calibration(host, ignore_value=ign)
        want = _json_bytes(ev, "test")
        assert set(json.loads(want[0])) == {"mean", "case0", "case1", "case2"} and json.loads(want[1]).keys() == set(types)

        evd = mk(tmp_path / "dev")
        dev = DeviceExperimentDataloader(evd, "test")
        with monkeypatch.context() as m:
            spy = _Spy(m)
            am = vm.ambiguity_modeling_device(dev, batch=2)
            cal = vm.calibration_device(dev, ignore_value=ign, batch=2)
        assert _json_bytes(evd, "test") == want, ign
        assert am == json.loads(want[0]) and cal == json.loads(want[2])
        # nothing but the sums of a chunk (5, 8 or 63 numbers per image) came back; every scored tensor lay on the device
        assert spy.copies and max(spy.copies) <= 2 * 63, spy.copies
        assert spy.inputs and all(all(flags) for flags in spy.inputs), spy.inputs
        assert not dev._cache

        evp = mk(tmp_path / "plain")                                  # a plain loader: its arrays go up once
        plain = ExperimentDataloader(evp, "test")
        vm.ambiguity_modeling_device(plain, batch=32)
        vm.calibration_device(plain, ignore_value=ign, batch=32)
        assert _json_bytes(evp, "test") == want, ign
        for e in (ev, evd, evp):
            os.remove(e.exp_path / FILES[1])
    # the ground-truth map of the file branch on the device
    for i in host.image_ids:
        t = dev.get_gt_unc_map_device(i)
        assert t.is_cuda and t.dtype == torch.float64 and np.array_equal(t.cpu().numpy(), host.get_gt_unc_map(i))


def test_device_drivers_write_the_host_drivers_files_2d(tmp_path, monkeypatch):
    """a 2D tree: colour PNG predictions through the GTA hook ((H, W)), TIFF maps ((W, H): the axis swap), reference
    segmentations from a datamodule, the ground-truth map from the GTA hook"""
    from values_amd import evalmetrics as vm, results2d
    from values_amd.experiment import DeviceExperimentDataloader, ExperimentDataloader, ExperimentVersion
    rng = np.random.default_rng(37)
    ids, T, H, W = ["img_a", "img_b", "img_c"], 2, 20, 33
    types = ["predictive_uncertainty", "aleatoric_uncertainty"]
    classes = np.array([0, 1, 8, 11, 13, 5], dtype=np.uint8)
    mk = lambda base: ExperimentVersion(
        base_path=base, naming_scheme_version="seed{seed}", pred_model="Dropout", image_ending=".png", unc_ending=".tif",
        unc_types=types, aggregations=None, n_reference_segs=2, seed=7,
        datamodule_config={"_target_": "tests.em_inputs.StubDataModule", "root": str(tmp_path / "labels")},
        pred_seg_loading={"_target_": "evaluation.utils.gta.pred_seg_loading"},
        gt_unc_map_loading={"_target_": "evaluation.utils.gta.gt_unc_map"})
    ev = mk(tmp_path / "host")
    for split in ("val", "test"):
        label = classes[rng.integers(0, len(classes), (3, H, W))]
        segs = np.stack([np.where(rng.random((3, H, W)) < 0.8, label, classes[rng.integers(0, len(classes), (3, H, W))]) for _ in range(2)], 1)
        mean = np.where(rng.random((3, H, W)) < 0.75, label, classes[rng.integers(0, len(classes), (3, H, W))]).astype(np.uint8)
        os.makedirs(tmp_path / "labels" / split)
        for b, iid in enumerate(ids):
            np.save(tmp_path / "labels" / split / f"{iid}.npy", label[b].astype(np.int64))
            np.save(tmp_path / "labels" / split / f"{iid}_seg.npy", segs[b].astype(np.int64))
        wrong = (segs != mean[:, None]).mean(1)
        switch = 0.5 * np.isin(label, [0, 1, 8, 11, 13])
        unc = {k: torch.from_numpy((s * wrong + switch + 0.3 * rng.random((3, H, W))).astype(np.float32)).cuda()
               for k, s in (("pred_entropy", 0.7), ("aleatoric_uncertainty", 0.4), ("epistemic_uncertainty", 0.2))}
        pm = torch.from_numpy(mean[:, None].repeat(T, 1)).cuda()
        results2d.save_images_device(str(ev.exp_path / split), ids, pm, torch.from_numpy(mean).cuda(), unc)
    shutil.copytree(tmp_path / "host", tmp_path / "dev")
    host = ExperimentDataloader(ev, "test")
    assert host.image_ids == ids and host.get_reference_segs("img_a").shape == (2, H, W)
    assert host.get_unc_map("img_a", types[0]).shape == (W, H) and host.get_mean_pred_seg("img_a").shape == (H, W)
    vm.ambiguity_modeling(host)
    vm.calibration(host)
    want = _json_bytes(ev, "test")
    evd = mk(tmp_path / "dev")
    dev = DeviceExperimentDataloader(evd, "test")
    with monkeypatch.context() as m:
        spy = _Spy(m)
        vm.ambiguity_modeling_device(dev, batch=2)
        vm.calibration_device(dev, batch=2)
    assert _json_bytes(evd, "test") == want
    assert spy.copies and max(spy.copies) <= 2 * 63, spy.copies
    # (the reference segmentations of this tree come from the datamodule on the host and go up once per chunk)
    assert spy.inputs and all(all(flags) for flags in spy.inputs), spy.inputs
    assert 0.0 < json.loads(want[0])["mean"][types[0]]["metrics"]["ncc"] < 1.0


def test_batched_refusals_name_the_item():
    from values_amd import _lib, evalmetrics as vm
    lib = _lib.load()
    dev = vm._dev()
    m = torch.zeros(300, dtype=torch.float32, device=dev)
    lab = torch.zeros((2, 300), dtype=torch.int32, device=dev)
    out = torch.empty(8 * 63, dtype=torch.float64, device=dev)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=dev)
    F32, st = _lib.VX_F32, _lib.stream_ptr()
    ncc = lambda **k: _lib.NccItem(**{**dict(gt=m.data_ptr(), pred=m.data_ptr(), n_gt=300, n_pred=300, gt_dtype=F32, pred_dtype=F32, gt_R=0), **k})
    em = lambda **k: _lib.EmItem(**{**dict(unc=m.data_ptr(), ref=lab.data_ptr(), pred=lab.data_ptr(), nvox=300, dtype=F32, R=2), **k})
    par = (C.c_double * 16)(*([0.0, 0.0, 0.5, 0.5] * 4))
    edges = (C.c_double * 21)(*np.linspace(0.0, 1.0 + 1e-8, 21).tolist())
    calls = {"ncc": (lambda items, n: lib.vx_ncc_batched(items, n, _lib.ptr(out), _lib.ptr(ws), ws.numel(), st), _lib.NccItem, ncc),
             "platt": (lambda items, n: lib.vx_platt_sums_batched(items, n, par, -1, _lib.ptr(out), _lib.ptr(ws), ws.numel(), st), _lib.EmItem, em),
             "bins": (lambda items, n: lib.vx_calib_bins_batched(items, n, par, edges, -1, _lib.ptr(out), _lib.ptr(ws), ws.numel(), st),
                      _lib.EmItem, em)}
    bad = {"ncc": [(dict(gt=None), -1), (dict(pred_dtype=9), -3), (dict(n_pred=299), -2), (dict(gt_R=-1), -2)],
           "platt": [(dict(unc=None), -1), (dict(R=0), -2), (dict(dtype=9), -3)],
           "bins": [(dict(unc=None), -1), (dict(R=0), -2), (dict(dtype=9), -3)]}
    for name, (call, T, make) in calls.items():
        good = (T * 3)(make(), make(), make())
        for n in (0, 4097):
            assert call(good, n) == -2 and b"n_items" in lib.vx_last_error_string()
        for kw, code in bad[name]:
            items = (T * 3)(make(), make(), make(**kw))
            assert call(items, 3) == code, (name, kw, lib.vx_last_error_string())
            assert b"item 2" in lib.vx_last_error_string()
            with pytest.raises(_lib.VxError, match="item 2"):
                _lib.check(call(items, 3), name)
        assert call(good, 3) == 0                                    # the same call with nothing wrong in it runs
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="do not fit together"):
        vm.calc_ace_batch([lab.view(2, 20, 15)], [lab[0].view(20, 15)], [m.view(20, 15)[:, :14]], 1.0, 0.0)
