"""CPU: tests/reduce_ref.py, the float64 restatement the GPU reduction tests compare with, against the reference's own
recorded outputs (unc_kat.npz, accum_24.npz)."""
import numpy as np
import pytest

from tests import reduce_ref as rr
from tests.formula import formula_tensor
from tests.helpers import load_npz

KEYS = (("pred_entropy", "pred_entropy"), ("expected_entropy", "aleatoric_uncertainty"),
        ("mutual_information", "epistemic_uncertainty"))


@pytest.mark.parametrize("case", ["hand", "r3d", "r2d", "ex"])
def test_plain_maps_equal_the_reference_fixture(case):
    g = load_npz("unc_kat.npz")
    x = g[f"{case}_in"]
    T, C = x.shape[:2]
    m = rr.maps(x.reshape(1, T, C, -1), from_logits=False)
    for mine, theirs in KEYS:
        want = g[f"{case}_{theirs}"]
        np.testing.assert_allclose(m[mine][0].reshape(want.shape), want, atol=2e-6, rtol=0)
        assert not np.isnan(m[mine]).any()
    mean = x.astype(np.float64).mean(0).reshape(C, -1)
    np.testing.assert_allclose(m["mean_softmax"][0], mean, atol=1e-12)
    np.testing.assert_array_equal(m["argmax"][0], mean.argmax(0))
    np.testing.assert_array_equal(m["sample_argmax"][0], x.reshape(T, C, -1).argmax(1))
    np.testing.assert_allclose(m["variance"][0], x.astype(np.float64).reshape(T, C, -1).var(0).mean(0), atol=1e-15)


def _accum_inputs():
    from oracle.predict_oracle import crop_indices
    size, patch, T = 24, 16, 3
    crops = crop_indices((size,) * 3, patch, 0.5)
    fake = np.abs(formula_tensor((len(crops), T, 2, patch, patch, patch), tag=55, scale=1.0))
    fake = fake / fake.sum(axis=2, keepdims=True)
    return np.log(fake), [(c[0][0], c[1][0], c[2][0]) for c in crops], (size,) * 3     # softmax(log p) == p


def test_accumulate_equals_the_reference_concat_data():
    g = load_npz("accum_24.npz")
    logits, crops, shape = _accum_inputs()
    sums, counts = rr.accumulate(logits, crops, shape)
    np.testing.assert_allclose(sums, g["softmax_sum"], atol=2e-6, rtol=0)
    np.testing.assert_array_equal(counts, g["num_predictions"][0])
    np.testing.assert_allclose(sums / np.clip(counts, 1, None), g["normalised"], atol=1e-6, rtol=0)
    assert counts.max() == 8 and counts.min() == 1


def test_accumulate_drops_patch_voxels_outside_the_image():
    logits = formula_tensor((2, 1, 2, 3, 4, 5), 61, scale=2.0)
    sums, counts = rr.accumulate(logits, [(0, 0, 0), (2, 3, 4)], (4, 5, 6))
    want = np.zeros((4, 5, 6))
    want[:3, :4, :5] += 1
    want[2:, 3:, 4:] += 1
    np.testing.assert_array_equal(counts, want)
    np.testing.assert_allclose(sums.sum(1)[0], want, atol=1e-12)        # every addend is a softmax


def test_out_count_maps_equal_the_fixture_maps_divided_by_the_clipped_count():
    """quirk D10 as the reference has it: calculate_uncertainty on the un-normalised sums, the maps divided by
    clip(count, 1) when they are saved"""
    g = load_npz("accum_24.npz")
    x = g["softmax_sum"]
    cnt = g["num_predictions"][0]
    m = rr.maps(x.reshape((1,) + x.shape[:2] + (-1,)), from_logits=False, out_count=cnt.reshape(1, -1))
    cl = np.clip(cnt, 1, None)
    for mine, theirs in KEYS:
        np.testing.assert_allclose(m[mine][0].reshape(cnt.shape), g[f"unc_{theirs}"] / cl, atol=2e-6, rtol=0)
    np.testing.assert_allclose(m["mean_softmax"][0].reshape(x.shape[1:]), x.astype(np.float64).mean(0) / cl, atol=1e-12)
    np.testing.assert_allclose(m["variance"][0].reshape(cnt.shape), x.astype(np.float64).var(0).mean(0) / cl ** 2, atol=1e-12)
    # in_count: the same maps as the plain maps of the normalised sums
    n = rr.maps(x.reshape((1,) + x.shape[:2] + (-1,)), from_logits=False, in_count=cnt.reshape(1, -1))
    p = rr.maps((x.astype(np.float64) / cl).reshape((1,) + x.shape[:2] + (-1,)), from_logits=False)
    for k in n:
        np.testing.assert_array_equal(n[k], p[k])


def test_masked_class_logits_give_finite_maps():
    """a class logit of -inf is p = 0 exactly; the reference skips its NaN product (test_3D.py:503-504)"""
    x = np.array([-np.inf, 0.0, 1.0]).reshape(1, 1, 3, 1)
    m = rr.maps(x, from_logits=True)
    assert abs(m["pred_entropy"][0, 0] - 0.5822031) < 1e-6 and abs(m["expected_entropy"][0, 0] - 0.5822031) < 1e-6
    assert m["mutual_information"][0, 0] == 0
    assert rr.clear_mean(m["mean_softmax"]).all() and rr.clear_sample(x, True).all()


def test_float32_gaps_of_the_reference_are_the_constants_of_the_gpu_test():
    """the tolerance rule of tests/test_gpu_reduce.py: its GAP_* constants are the largest difference between this
    reference in float64 and with the input and every accumulator rounded to float32, over that test's own inputs"""
    from tests import test_gpu_reduce as tg
    gap = {"count_maps": 0.0, "count_mean": 0.0, "variance": 0.0, "plain_maps": 0.0, "plain_mean": 0.0}
    excluded = 0.0
    for from_logits, extras, nvox, T, C in tg.EXTRAS_CASES:
        x, kw, cnt = tg.extras_case(from_logits, extras, nvox, T, C, np.float32)
        a, b = rr.maps(x, from_logits, **kw), rr.maps(x, from_logits, dtype=np.float32, **kw)
        g = "count" if (not from_logits or extras != "var") else "plain"
        gap[g + "_maps"] = max([gap[g + "_maps"]] + [float(np.abs(a[k] - b[k]).max()) for k in tg.MAPS])
        gap[g + "_mean"] = max(gap[g + "_mean"], float(np.abs(a["mean_softmax"] - b["mean_softmax"]).max()))
        gap["variance"] = max(gap["variance"], float(np.abs(a["variance"] - b["variance"]).max()))
        clear = rr.clear_mean(a["mean_softmax"]) | ((cnt == 0) & (not from_logits))
        excluded = max(excluded, 1.0 - float(clear.mean()))
    for name, const in (("count_maps", tg.GAP_COUNT_MAPS), ("count_mean", tg.GAP_COUNT_MEAN), ("variance", tg.GAP_VARIANCE)):
        assert gap[name] <= const <= 1.05 * gap[name], (name, gap[name], const)
    # paths without counts: the oracle's own float32 gap stays an order below the 5e-6 / 2e-6 held there
    assert gap["plain_maps"] < 1e-6 and gap["plain_mean"] < 2e-7
    assert tg.COUNT_MAPS == max(5e-6, 4 * tg.GAP_COUNT_MAPS) and tg.VARIANCE == max(5e-6, 4 * tg.GAP_VARIANCE)
    assert tg.COUNT_MEAN == max(5e-6, 4 * tg.GAP_COUNT_MEAN)
    assert excluded <= 0.001 < tg.ARGMAX_EXCLUDED
