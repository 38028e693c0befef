"""GPU: per-case test metrics of the 3D path for a whole step (calculate_metrics, test_3D.py:537-575): the sums of
vx_soft_metric_sums_batched, and process_metrics_3d against the oracle and against the per-case functions."""
import json

import numpy as np
import pytest
import torch

from tests.metrics3d_ref import formula_case, np_soft_sums

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -7.0
U = 2.0 ** -53

# The device's logf and numpy's float32 log are two implementations: where they round a term to different neighbours the log
# component moves by up to one float32 ulp of that term, and the component is bounded by nvox 2^-23 max|log p| on top of the
# reordering bound.  test_sums_match_numpy prints, per shape, the error and by how much it exceeds the reordering bound alone
# (excess <= 0: the allowance was not needed); set this to False where a run shows it is never needed.
LOGF_LAST_ULP = True


def span_of_one_workgroup():
    """the launcher's partition rule, read off its workspace query: the largest nvox one workgroup takes"""
    from values_amd import _lib
    ws = _lib.load().vx_soft_metric_batched_workspace_bytes
    one = ws(1, 1, 1, 1)
    lo, hi = 1, 1 << 24
    assert ws(1, 1, 1, hi) > one
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ws(1, 1, 1, mid) == one else (lo, mid)
    return lo


def make_inputs(rng, B, C, R, nvox):
    """float32 softmax probabilities (B, C, nvox); labels (B, R, nvox) with a few values >= C and 255 among them"""
    z = rng.standard_normal((B, C, nvox)) * 2.5
    e = np.exp(z - z.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True)).astype(np.float32)
    g = rng.integers(0, C, (B, R, nvox)).astype(np.uint8)
    junk = rng.random((B, R, nvox))
    g[junk < 0.06] = C
    g[junk < 0.04] = 255
    g[junk < 0.02] = min(C + 7, 254)
    return p, g


def device_sums(p, g):
    """vx_soft_metric_sums_batched through the C ABI; sentinel-filled guard regions behind the sums and behind the workspace"""
    from values_amd import _lib
    lib = _lib.load()
    B, C, nvox = p.shape
    R = g.shape[1]
    pd, gd = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    n = B * R * (3 * C + 1)
    out = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    nws = int(lib.vx_soft_metric_batched_workspace_bytes(B, C, R, nvox))
    assert nws > 0 and nws % 8 == 0
    ws = torch.full((nws // 8 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    _lib.check(lib.vx_soft_metric_sums_batched(pd.data_ptr(), gd.data_ptr(), B, C, R, nvox, out.data_ptr(), ws.data_ptr(),
                                               _lib.stream_ptr()), "vx_soft_metric_sums_batched")
    host = out.cpu().numpy()
    assert (host[n:] == SENTINEL).all(), "guard region behind sums was written"
    assert (ws[nws // 8:] == SENTINEL).all().item(), "guard region behind the workspace was written"
    return host[:n].reshape(B, R, 3 * C + 1)


def one_image_sums(p, g):
    """vx_soft_metric_sums on one image: p (C, nvox), g (R, nvox)"""
    from values_amd import _lib
    lib = _lib.load()
    C, nvox = p.shape
    R = g.shape[0]
    pd, gd = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    out = torch.empty((R, 3 * C + 1), dtype=torch.float64, device="cuda")
    ws = torch.empty(max(int(lib.vx_soft_metric_workspace_bytes(C, R)), 8), dtype=torch.uint8, device="cuda")
    _lib.check(lib.vx_soft_metric_sums(pd.data_ptr(), gd.data_ptr(), C, R, nvox, out.data_ptr(), ws.data_ptr(), _lib.stream_ptr()),
               "vx_soft_metric_sums")
    return out.cpu().numpy()


SHAPES = [(1, 1, 1, 1), (3, 2, 4, 63), (2, 3, 1, 64), (2, 8, 2, 65), (1, 32, 3, 257), (2, 2, 4, 315)]


def all_shapes():
    span = span_of_one_workgroup()
    # the smallest image of two workgroups (its second holds one voxel: a ragged tail), and one of three workgroups whose
    # size is a multiple of 4 (the 16-byte loads) with a tail that fills neither a workgroup nor a wave
    return SHAPES + [(2, 2, 4, span + 1), (2, 3, 5, 2 * span + 1028)]


def test_sums_match_numpy():
    """integer component exact; float components within the float64 reordering bound 4 nvox 2^-53 sum|term|; the log
    component within that bound plus the last-ulp allowance nvox 2^-23 max|log p| (LOGF_LAST_ULP above; the largest excess
    over the reordering bound alone is printed per shape)."""
    for B, C, R, nvox in all_shapes():
        rng = np.random.default_rng(1000 * B + 100 * C + 10 * R + nvox)
        p, g = make_inputs(rng, B, C, R, nvox)
        assert (g >= C).any() or nvox < 16
        want, mag = np_soft_sums(p, g)
        got = device_sums(p, g)
        assert got.dtype == np.float64 and got.shape == want.shape
        cnt = [3 * c + 1 for c in range(C)]
        flt = [k for k in range(3 * C) if k % 3 != 1]
        assert np.array_equal(got[..., cnt], want[..., cnt]), (B, C, R, nvox)
        bound = 4 * nvox * U * mag
        err = np.abs(got - want)
        assert (err[..., flt] <= bound[..., flt]).all(), (B, C, R, nvox, float((err - bound)[..., flt].max()))
        maxlog = float(np.abs(np.log(p)).max())
        excess = float((err[..., 3 * C] - bound[..., 3 * C]).max())
        print(f"B={B} C={C} R={R} nvox={nvox}: log component err {err[..., 3 * C].max():.3e}, reordering bound "
              f"{bound[..., 3 * C].max():.3e}, excess {excess:.3e}, last-ulp allowance {nvox * 2.0 ** -23 * maxlog:.3e}")
        allow = bound[..., 3 * C] + (nvox * 2.0 ** -23 * maxlog if LOGF_LAST_ULP else 0.0)
        assert (err[..., 3 * C] <= allow).all(), (B, C, R, nvox, excess)
        # sum p_c does not depend on the rater: one value, replicated
        assert (got[:, :, 2:3 * C:3] == got[:, :1, 2:3 * C:3]).all()


def test_sums_do_not_depend_on_the_batch_and_repeat_bit_for_bit():
    span = span_of_one_workgroup()
    for C, R, nvox in ((2, 4, 315), (3, 2, 2 * span + 1028), (2, 5, span + 1)):
        rng = np.random.default_rng(nvox + R)
        p, g = make_inputs(rng, 3, C, R, nvox)
        got = device_sums(p, g)
        assert np.array_equal(got, device_sums(p, g))                      # two consecutive calls
        for b in range(3):
            assert np.array_equal(got[b], device_sums(p[b:b + 1], g[b:b + 1])[0]), (C, R, nvox, b)


def test_sums_against_the_one_image_kernel():
    """same terms (device logf on both sides), another order: integer component equal, float components within the
    reordering bound of two float64 sums"""
    span = span_of_one_workgroup()
    for B, C, R, nvox in ((3, 2, 4, 315), (2, 8, 2, 65), (2, 3, 5, 2 * span + 1028)):
        rng = np.random.default_rng(7 * nvox + C)
        p, g = make_inputs(rng, B, C, R, nvox)
        _, mag = np_soft_sums(p, g)
        got = device_sums(p, g)
        for b in range(B):
            one = one_image_sums(p[b], g[b])
            cnt = [3 * c + 1 for c in range(C)]
            assert np.array_equal(got[b][:, cnt], one[:, cnt]), (B, C, R, nvox, b)
            assert (np.abs(got[b] - one) <= 4 * nvox * U * mag[b]).all(), (B, C, R, nvox, b)


def test_wrapper_flattens_space_and_takes_integer_labels():
    from values_amd.metrics import soft_metric_sums_batched
    rng = np.random.default_rng(5)
    p, g = make_inputs(rng, 2, 3, 2, 5 * 6 * 7)
    got = soft_metric_sums_batched(torch.from_numpy(p.reshape(2, 3, 5, 6, 7)).cuda(),
                                   torch.from_numpy(g.reshape(2, 2, 5, 6, 7).astype(np.int64)).cuda())
    assert np.array_equal(got, device_sums(p, g))
    with pytest.raises(ValueError):
        soft_metric_sums_batched(torch.zeros(2, 3, 8).cuda(), torch.zeros(1, 2, 8).cuda())


def _step(C, T, R, shape, B=3, tag=0):
    """B different cases of one step: probs (B, T, C, *shape) float32, gt (B, R, *shape) int64, and uncertainty_maps' dict"""
    from values_amd.uncertainty import uncertainty_maps
    cases = [formula_case(C, T, R, shape, tag + 10 * b) for b in range(B)]
    sm = np.stack([c[0] for c in cases])
    gt = np.stack([c[1] for c in cases])
    out = uncertainty_maps(torch.from_numpy(sm).cuda(), from_logits=False, want_sample_argmax=True)
    return sm, gt, out


def _per_case(out, probs, gt, b, ged):
    from values_amd.metrics import calculate_ged, calculate_test_metrics
    m = calculate_test_metrics(out["mean_softmax"][b:b + 1], torch.from_numpy(gt[b]).cuda())
    if ged:
        m.update(calculate_ged(torch.from_numpy(probs[b]).cuda(), torch.from_numpy(gt[b]).cuda(), pred_masks=out["sample_argmax"][b]))
    return m


def _assert_equals_per_case(got, want):
    assert list(got) == list(want)
    for k in want:
        if k == "loss":
            assert abs(got[k] - want[k]) < 1e-12, k
        else:
            assert got[k] == want[k], k                       # ratios of the same integers


@pytest.mark.parametrize("C,T,R,shape", [(2, 5, 4, (12, 10, 8)), (3, 4, 3, (9, 7, 5)), (2, 1, 1, (4, 4, 4))])
def test_process_metrics_3d_matches_oracle_and_the_per_case_path(C, T, R, shape):
    """tolerances of tests/test_gpu_results.py::test_metrics_match_oracle: loss 1e-5, dice 1e-7, GED keys 1e-6"""
    from oracle import metrics_oracle as mo
    from values_amd.metrics import process_metrics_3d
    sm, gt, out = _step(C, T, R, shape)
    got = process_metrics_3d(out, torch.from_numpy(gt).cuda())
    assert isinstance(got, list) and len(got) == 3
    ged = R > 1 or T > 1
    for b in range(3):
        mean = sm[b].mean(0, keepdims=True)
        ref = mo.calculate_test_metrics(mean.astype(np.float64), gt[b])
        if ged:
            ref.update(mo.calculate_ged(sm[b], gt[b]))
        print(b, got[b], ref)
        assert set(got[b]) == set(ref)
        for k in ref:
            assert abs(got[b][k] - ref[k]) < {"loss": 1e-5, "dice": 1e-7}.get(k, 1e-6), (b, k)
        _assert_equals_per_case(got[b], _per_case(out, sm, gt, b, ged))
    assert len({m["dice"] for m in got}) == 3 or shape == (4, 4, 4)           # different cases: the batch order is checked
    # host ground truth; the sample arg-maxes handed in, taken from probs, or unknown (loss and dice only)
    bare = {k: out[k] for k in ("mean_softmax", "argmax")}
    assert process_metrics_3d(bare, gt, sample_argmax=out["sample_argmax"]) == got
    assert process_metrics_3d(bare, gt, probs=torch.from_numpy(sm).cuda()) == got
    assert process_metrics_3d({"mean_softmax": out["mean_softmax"]}, gt) == [{k: m[k] for k in ("loss", "dice")} for m in got]
    # predict_uncertainty's names for the two masks
    named = {"mean_softmax": out["mean_softmax"], "pred_seg_mean": out["argmax"], "pred_seg": out["sample_argmax"]}
    assert process_metrics_3d(named, gt) == got


def test_edge_cases_all_background_single_prediction_and_the_fallback():
    from oracle import metrics_oracle as mo
    from values_amd.metrics import process_metrics_3d
    from values_amd.uncertainty import uncertainty_maps
    shape = (6, 6, 6)
    # predictions and raters all background (every Dice 0 / 0 -> 0); second case: one rater with some foreground
    sm = np.zeros((2, 3, 2) + shape, np.float32); sm[:, :, 0] = 0.9; sm[:, :, 1] = 0.1
    gt = np.zeros((2, 2) + shape, np.int64)
    gt[1, 0, :3] = 1
    out = uncertainty_maps(torch.from_numpy(sm).cuda(), from_logits=False, want_sample_argmax=True)
    got = process_metrics_3d(out, gt)
    for b in range(2):
        ref = mo.calculate_ged(sm[b], gt[b])
        assert {k: got[b][k] for k in ref} == pytest.approx(ref)
        assert got[b]["dice"] == 0.0
        _assert_equals_per_case(got[b], _per_case(out, sm, gt, b, True))
    assert got[0]["ged"] == pytest.approx(0.0)                              # 2*1 - 1 - 1
    # T = 1, R = 1: no GED keys
    sm1, gt1, out1 = _step(2, 1, 1, (4, 5, 6), B=2, tag=3)
    got = process_metrics_3d(out1, gt1)
    assert [list(m) for m in got] == [["loss", "dice"]] * 2
    for b in range(2):
        _assert_equals_per_case(got[b], _per_case(out1, sm1, gt1, b, False))
    # 1 + T + R = 33 masks: the documented per-case fallback, same results
    smf, gtf, outf = _step(2, 28, 4, (4, 5, 6), B=2, tag=5)
    got = process_metrics_3d(outf, gtf)
    for b in range(2):
        want = _per_case(outf, smf, gtf, b, True)
        assert "max dice rater 3" in want and got[b] == want


def test_metrics_json_end_to_end(tmp_path):
    """process_metrics_3d(image_ids) -> results.log_metrics -> metrics.json -> evalmetrics.get_dice / get_risk"""
    from values_amd import evalmetrics
    from values_amd.metrics import process_metrics_3d
    from values_amd.results import log_metrics
    sm, gt, out = _step(2, 3, 2, (6, 7, 5), tag=40)
    ids = ["case_c", "case_a", "case_b"]
    metrics = process_metrics_3d(out, gt, image_ids=ids)
    assert list(metrics) == ids and [metrics[i] for i in ids] == process_metrics_3d(out, gt)
    log_metrics(str(tmp_path), metrics)
    f = tmp_path / "metrics.json"
    on_disk = json.load(open(f))
    assert set(on_disk) == set(ids) | {"mean"}
    assert on_disk["mean"]["ged"] == pytest.approx(float(np.mean([metrics[i]["ged"] for i in ids])), abs=1e-15)
    for i in ids:
        assert on_disk[i] == metrics[i]
        assert evalmetrics.get_dice(i, f) == metrics[i]["dice"]
        assert evalmetrics.get_risk(i, f) == 1 - metrics[i]["dice"]
    assert len({metrics[i]["dice"] for i in ids}) == 3
    with pytest.raises(ValueError, match="image ids"):
        process_metrics_3d(out, gt, image_ids=ids[:2])
