"""GPU: the batched threshold search -- thresholds.count_nonzero_batch (vx_count_nonzero_batched) against np.count_nonzero,
thresholds.quantile_segments (vx_select_segments) against np.quantile of the concatenated float32 data, compared with ==,
and the drivers get_foreground_quantile_device / find_threshold(device_io=True) on a written 3D and a written 2D results
tree against the host paths (the two JSON files byte for byte).  The oracle is numpy on the host."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TYPES = ["predictive_uncertainty", "aleatoric_uncertainty", "epistemic_uncertainty"]


def _offset_view(a, skip):
    """a device copy of the numpy array `a` that starts `skip` elements into its buffer"""
    buf = torch.empty(a.size + skip, dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
    buf[skip:] = torch.from_numpy(a.reshape(-1)).cuda()
    return buf[skip:].reshape(a.shape)


# ---------------------------------------------------------------------------------------------------------------------
# counts

def _count_array(dtype, n, rng):
    if dtype == np.bool_:
        return rng.random(n) < 0.4
    if np.issubdtype(dtype, np.integer):
        bits = np.dtype(dtype).itemsize * 8
        # a non-zero element may have any ONE byte set: the top byte alone, the low byte alone
        a = (rng.integers(1, 256, n).astype(np.uint64) << (8 * rng.integers(0, bits // 8, n)).astype(np.uint64)).astype(dtype)
        a[rng.random(n) < 0.5] = 0
        return a
    a = rng.standard_normal(n).astype(dtype)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, np.finfo(dtype).tiny / 4, -np.finfo(dtype).smallest_subnormal, 2.0],
                       dtype=dtype)
    idx = rng.random(n) < 0.6
    a[idx] = special[rng.integers(0, len(special), int(idx.sum()))]
    return a


def test_count_nonzero_batch_matches_numpy():
    from values_amd.thresholds import count_nonzero_batch
    rng = np.random.default_rng(21)
    arrays, tensors = [], []
    for dtype in (np.bool_, np.uint8, np.int16, np.int32, np.int64, np.float32, np.float64):
        for n in (0, 1, 63, 64, 65, 70001):
            a = _count_array(dtype, n, rng)
            arrays.append(a)
            tensors.append(torch.from_numpy(a).cuda())
    for skip in (1, 3):                                    # uint8 views that start at byte offsets 1 and 3 of a buffer
        a = _count_array(np.uint8, 5003, rng)
        arrays.append(a)
        tensors.append(_offset_view(a, skip))
    rgb = _count_array(np.uint8, 29 * 41 * 3, rng).reshape(29, 41, 3)
    arrays.append(rgb.swapaxes(0, 1))                      # what the 2D reader returns: a transposed (H, W, 3) view
    tensors.append(torch.from_numpy(rgb).cuda().transpose(0, 1))
    strided = _count_array(np.int32, 300, rng).reshape(10, 30)
    arrays.append(strided[:, ::3])                         # not a dense block: made contiguous
    tensors.append(torch.from_numpy(strided).cuda()[:, ::3])
    assert not tensors[-2].is_contiguous() and not tensors[-1].is_contiguous()
    want = [int(np.count_nonzero(a)) for a in arrays]
    assert count_nonzero_batch(tensors) == want
    assert any(w not in (0, a.size) for w, a in zip(want, arrays))
    # the special values alone
    f = np.array([-0.0, 0.0, np.nan, -np.nan, np.inf, 1e-45, -0.0, 0.0], dtype=np.float32)
    d = np.array([-0.0, 5e-324, np.nan, 0.0, 2.0, -np.inf, -0.0], dtype=np.float64)
    assert count_nonzero_batch([torch.from_numpy(f).cuda(), torch.from_numpy(d).cuda()]) == [4, 4]


def test_count_nonzero_batch_many_small_items():
    """3 000 items of 7 elements: more work blocks than the grid has workgroups, every block another item"""
    from values_amd.thresholds import count_nonzero_batch
    rng = np.random.default_rng(22)
    a = (rng.random((3000, 7)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (3000, 7)).astype(np.uint8)
    t = torch.from_numpy(a).cuda()
    assert count_nonzero_batch([t[i] for i in range(3000)]) == np.count_nonzero(a, axis=1).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# selection

def _check(segments, qs, tensors=None):
    """quantile_segments over device copies of the numpy `segments` == np.quantile of their float32 concatenation, and
    == thresholds.quantile of the concatenated device tensor"""
    from values_amd.thresholds import quantile, quantile_segments
    if tensors is None:
        tensors = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in segments]
    flat = np.concatenate([np.asarray(s).reshape(-1) for s in segments]).astype(np.float32)
    joined = torch.from_numpy(flat).cuda()
    for q in qs:
        want = float(np.quantile(flat.astype(np.float64), q))
        got = quantile_segments(tensors, q)
        assert got == want, (q, got, want)
        assert got == quantile(joined, q), q


def test_quantile_segments_small_and_tied():
    _check([np.array([3.25], dtype=np.float32)], (0.0, 0.3, 1.0))
    same = np.full(1000, 0.7, dtype=np.float32)
    _check([same[:1], same[1:64], same[64:]], (0.0, 0.5, 0.999, 1.0))
    gap = np.array([0.0] * 10 + [1.0] * 10, dtype=np.float32)
    _check([gap[:7], gap[7:]], (0.5,))                     # order statistics 9 and 10 straddle the gap: the minimum-above pass runs
    _check([gap[:7], gap[7:]], (0.25,))                    # both inside the zeros: an equal key remains
    _check([gap[::-1].copy()], (0.5, 9 / 19, 10 / 19, 0.0, 1.0))


def test_quantile_segments_normal_variates_in_odd_segments():
    rng = np.random.default_rng(31)
    x = rng.standard_normal(100003).astype(np.float32)
    x[x == 0] = 1.0                                        # no -0.0 / +0.0 pair in the data
    cuts = np.cumsum([0, 64, 0, 65, 257, 30001, 50000])   # seven segments, one empty, the rest to the last
    segments = [x[a:b] for a, b in zip(cuts, list(cuts[1:]) + [len(x)])]
    assert len(segments) == 7 and [len(s) for s in segments[:4]] == [64, 0, 65, 257]
    tensors = [_offset_view(s, skip) for s, skip in zip(segments, (1, 0, 3, 2, 1, 5, 7))]
    assert all(t.data_ptr() % 16 for t in (tensors[0], tensors[2], tensors[3]))
    _check(segments, (0.0, 1e-7, 0.5, 0.97, 0.999, 1.0), tensors)


def test_quantile_segments_sweeps_and_many_segments():
    rng = np.random.default_rng(32)
    x = (rng.random(600000, dtype=np.float32) * 0.5).astype(np.float32)
    x[rng.random(600000) < 0.3] = 0.0                      # an uncertainty map: a third of it exactly zero
    _check([x[:250000].reshape(500, 500), x[250000:]], (0.1, 0.31, 0.9, 0.99999))
    # 2 500 segments of 37 elements: more work blocks than the grid has workgroups
    y = rng.standard_normal((2500, 37)).astype(np.float32)
    t = torch.from_numpy(y).cuda()
    _check(list(y), (0.2, 0.977), [t[i] for i in range(2500)])
    # transposed views of dense blocks, as the 2D readers return them
    z = rng.random((6, 24, 37), dtype=np.float32)
    tz = torch.from_numpy(z).cuda()
    _check(list(z), (0.4, 0.93), [tz[i].transpose(0, 1) for i in range(6)])


def test_quantile_segments_digits_inf_and_mixed_dtypes():
    rng = np.random.default_rng(33)
    one = np.float32(1.0)
    ulps = (one + np.arange(1000, dtype=np.float32) * np.spacing(one)).astype(np.float32)   # keys differ in the lowest digit only
    rng.shuffle(ulps)
    _check([ulps[:300], ulps[300:]], (0.0, 0.123, 0.5, 0.9995, 1.0))
    pows = np.concatenate([2.0 ** np.arange(-100, 100), -(2.0 ** np.arange(-100, 100))]).astype(np.float32)   # ... the highest only
    rng.shuffle(pows)
    _check([pows], (0.0, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0))
    x = rng.standard_normal(5000).astype(np.float32)
    x[x == 0] = 1.0
    x[:3], x[3:5] = np.inf, -np.inf
    rng.shuffle(x)
    # (ranks 0, 1 are -inf and 4997 .. 4999 +inf: the quantiles below interpolate between finite neighbours of them, since
    # numpy's own interpolation of an infinite pair is nan and nan compares unequal to itself)
    _check([x[:77], x[77:]], (0.0005, 0.3, 0.5, 0.9993))
    # float64 segments whose values no float32 holds: the cast on load decides the order statistics
    d = 1.0 + rng.random(4001) * 1e-6
    assert (d.astype(np.float32).astype(np.float64) != d).mean() > 0.9
    f = (1.0 + rng.random(3000) * 1e-6).astype(np.float32)
    tensors = [torch.from_numpy(d[:1500]).cuda(), torch.from_numpy(f).cuda(), _offset_view(d[1500:], 1)]
    assert tensors[0].dtype == torch.float64 and tensors[2].data_ptr() % 16 == 8
    _check([d[:1500], f, d[1500:]], (0.0, 0.1, 0.5, 0.77, 1.0), tensors)


def test_quantile_segments_nan_gives_nan():
    from values_amd.thresholds import quantile_segments
    rng = np.random.default_rng(34)
    x = rng.random(9000, dtype=np.float32)
    y = x.copy()
    y[8111] = np.nan
    clean, dirty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    assert np.isnan(quantile_segments([clean[:4000], dirty[4000:]], 0.5))
    assert np.isnan(quantile_segments([dirty.to(torch.float64)], 0.0))
    assert quantile_segments([clean[:4000], clean[4000:]], 0.5) == float(np.quantile(x.astype(np.float64), 0.5))


# ---------------------------------------------------------------------------------------------------------------------
# drivers

def _drivers_match_host(host, dev, tmp_path, loader):
    """get_foreground_quantile_device == get_foreground_quantile as a list; quantile_analysis.json and
    threshold_analysis.json of the device path == the host path's, byte for byte"""
    from values_amd import thresholds
    qh = thresholds.get_foreground_quantile(host)
    qd = thresholds.get_foreground_quantile_device(dev, batch=4)
    assert qd == qh
    (values,) = qh[host.exp_version.pred_model].values()
    assert len(values) == sum(len(host.get_pred_seg_paths(i)) for i in host.image_ids) and 0 < min(values) and max(values) < 1
    paths = thresholds.threshold_images_paths(host)
    out = {}
    for name, q, kw in (("host", qh, {"loader": loader}), ("device", qd, {"device_io": True, "batch": 4})):
        d = tmp_path / name
        os.makedirs(d)
        thresholds.save_foreground_quantiles(q, d)
        thresholds.find_threshold(paths, d, d, **kw)
        out[name] = [open(d / f, "rb").read() for f in ("quantile_analysis.json", "threshold_analysis.json")]
    assert out["device"] == out["host"]
    assert b"Mean epistemic threshold" in out["device"][1]


def test_drivers_3d_tree_match_host(tmp_path):
    from values_amd.experiment import DeviceExperimentDataloader, ExperimentDataloader, ExperimentVersion
    from values_amd.results import ResultsWriter, results_dir
    d = results_dir(str(tmp_path), "Dropout", "fold0_seed123", "id")
    with ResultsWriter(workers=2) as w:
        for i in range(5):
            g = torch.Generator(device="cuda").manual_seed(i)
            sm = torch.softmax(torch.randn(3, 2, 16, 16, 16, device="cuda", generator=g) * 3, 1)
            maps = {k: torch.rand(16, 16, 16, device="cuda", generator=g) * 0.5
                    for k in ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")}
            w.submit(d, f"case{i}", softmax_pred=sm, maps=maps)
    ev = ExperimentVersion(base_path=tmp_path, naming_scheme_version="fold{fold}_seed{seed}", pred_model="Dropout",
                           image_ending=".nii.gz", unc_ending=".nii.gz", unc_types=TYPES, aggregations=None,
                           n_reference_segs=1, fold=0, seed=123)
    host, dev = ExperimentDataloader(ev, "id"), DeviceExperimentDataloader(ev, "id")
    assert len(host.image_ids) == 5
    _drivers_match_host(host, dev, tmp_path, None)


def test_drivers_2d_tree_match_host(tmp_path):
    """PNG masks and TIFF maps: find_threshold(device_io=True) could not read this tree before it went through the
    readers of experiment._read_batches_device"""
    from values_amd import results2d
    from values_amd.experiment import DeviceExperimentDataloader, ExperimentDataloader, ExperimentVersion, _load_file
    rng = np.random.default_rng(5)
    ids, T, H, W = [f"img_{c}" for c in "abcdef"], 2, 24, 37
    pm = torch.from_numpy(rng.integers(0, 24, (6, T, H, W)).astype(np.uint8)).cuda()
    mm = torch.from_numpy(rng.integers(0, 24, (6, H, W)).astype(np.uint8)).cuda()
    unc = {k: torch.from_numpy(rng.random((6, H, W), dtype=np.float32)).cuda()
           for k in ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")}
    ev = ExperimentVersion(base_path=tmp_path, naming_scheme_version="seed{seed}", pred_model="Dropout", image_ending=".png",
                           unc_ending=".tif", unc_types=TYPES, aggregations=None, n_reference_segs=1, seed=7)
    results2d.save_images_device(str(ev.exp_path / "val"), ids, pm, mm, unc,
                                 ignore_index_map=torch.from_numpy((rng.random((6, H, W)) < 0.3).astype(np.uint8)).cuda())
    host, dev = ExperimentDataloader(ev, "val"), DeviceExperimentDataloader(ev, "val")
    assert host.image_ids == ids
    _drivers_match_host(host, dev, tmp_path, _load_file)
