"""CPU: tests/noise_ref.py, the restatement tests/test_gpu_noise.py compares vx_noise_view_3d and vx_tta_views_2d_gen with:
moments, ranges and independence of what it generates, independence of chunking, the float32 gap of the 3D view on the GPU
module's inputs, and the share of 2D elements that sit on a truncation step.  The restatement is deterministic: the
statistical bounds are five-sigma bounds of the estimators, fixed numbers for fixed seeds, and cannot flake."""
import numpy as np
import pytest

from tests import noise_ref as nr
from tests import sample_ref as sr

SEEDS = (0, 5, 1234)


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


# ---- 1. moments and range -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_generated_field_has_the_moments_of_a_standard_normal(seed):
    n = 1 << 20
    z = nr.view3d(np.zeros((1, n), np.float32), seed, index0=4, lo=1.0, hi=1.0)[0].reshape(-1)      # sigma = 1: the field itself
    np.testing.assert_array_equal(z, sr.gauss(seed, np.arange(n), 4))
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.std() - 1) < 5 / np.sqrt(2 * n)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("lo,hi", [(0.0, 0.1), (10.0, 50.0)])
def test_scales_lie_in_the_range_of_their_law_and_the_variance_is_uniform(seed, lo, hi):
    n = 4096
    slots = np.arange(n)
    flo, fhi = float(np.float32(lo)), float(np.float32(hi))
    s0, s1 = nr.scales(seed, slots, lo, hi, 0), nr.scales(seed, slots, lo, hi, 1)
    assert (s0 >= np.sqrt(flo)).all() and (s0 < np.sqrt(fhi)).all()
    assert (s1 >= flo).all() and (s1 < fhi).all()
    var = nr.variances(seed, slots, lo, hi)
    np.testing.assert_array_equal(s1, var)
    np.testing.assert_allclose(s0 * s0, var, rtol=1e-15, atol=0)
    # U(lo, hi): standard deviation (hi - lo) / sqrt(12), standard error of the mean of n draws / sqrt(n)
    assert abs(var.mean() - (flo + fhi) / 2) < 5 * (fhi - flo) / np.sqrt(12 * n)
    assert len(np.unique(var)) > n - 8          # (24-bit uniforms: a repeat among 4096 draws has probability 0.4)
    # a degenerate range gives the one value, whatever the uniform
    np.testing.assert_array_equal(nr.variances(seed, slots, 0.05, 0.05), np.full(n, float(np.float32(0.05))))


# ---- 2. independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_neighbouring_slots_and_the_two_slots_of_an_image_are_uncorrelated(seed):
    n = 1 << 16
    for g in (0, 7, 100):
        a, b = sr.gauss(seed, np.arange(n), g), sr.gauss(seed, np.arange(n), g + 1)
        assert abs(_corr(a, b)) < 5 / np.sqrt(n), g
    H, W = 128, 171
    f = nr.field2d(seed, 3, 2, H, W)
    m = H * W * 3
    assert f.shape == (2, 2, H, W, 3)
    for b in range(2):
        assert abs(_corr(f[b, 0].reshape(-1), f[b, 1].reshape(-1))) < 5 / np.sqrt(m)
    assert abs(_corr(f[0, 1].reshape(-1), f[1, 0].reshape(-1))) < 5 / np.sqrt(m)
    # element (y, x, c) of slot k of image b is element (y * W + x) * 3 + c of stream (image0 + b) * 2 + k
    assert f[1, 1, 5, 7, 2] == sr.gauss(seed, (5 * W + 7) * 3 + 2, (3 + 1) * 2 + 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_scale_stream_shares_nothing_with_the_element_streams(seed):
    n = 1 << 16
    slots = np.arange(n)
    u = sr.uniforms(nr.scale_seed(seed), 0, slots)[1]               # the uniform behind var of every slot
    e0 = sr.gauss(seed, 0, slots)                                   # element 0 of the same slots
    assert abs(_corr(u, e0)) < 5 / np.sqrt(n)
    assert abs(_corr(u, sr.uniforms(seed, 0, slots)[1])) < 5 / np.sqrt(n)
    assert not np.isin(sr.stream_key(nr.scale_seed(seed), slots), sr.stream_key(seed, slots)).any()
    assert nr.SCALE_XOR != sr.W_XOR
    assert not np.isin(sr.stream_key(nr.scale_seed(seed), slots), sr.stream_key(seed ^ sr.W_XOR, slots)).any()


# ---- 3. chunking ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", [0, 1])
def test_a_view_does_not_depend_on_how_the_volumes_are_chunked(law):
    x = nr.volumes(5, 2)
    for dtype in (np.float64, np.float32):
        whole, sg = nr.view3d(x, 9, 0, 0.0, 0.1, law, dtype=dtype)
        a, sa = nr.view3d(x[:2], 9, 0, 0.0, 0.1, law, dtype=dtype)
        b, sb = nr.view3d(x[2:], 9, 2, 0.0, 0.1, law, dtype=dtype)
        np.testing.assert_array_equal(whole, np.concatenate([a, b]))
        np.testing.assert_array_equal(sg, np.concatenate([sa, sb]))
    shifted, _ = nr.view3d(x[2:], 9, 0, 0.0, 0.1, law)
    assert not np.array_equal(shifted, whole[2:])


# ---- 4. the float32 gap the 3D bound is built on ----------------------------------------------------------------------------
def test_float32_gap_of_the_3d_view_is_the_constant_of_the_gpu_test():
    gap = 0.0
    for name, ref in nr.reference_matrix_3d():
        (a, sa), (b, sb) = ref(np.float64), ref(np.float32)
        assert a.dtype == np.float64 and b.dtype == np.float32 and sb.dtype == np.float32, name
        gap = max(gap, float(np.abs(a - b).max()), float(np.abs(sa - sb).max()))
    print(f"GAP_NOISE3D {gap:.3e}")
    assert gap <= nr.GAP_NOISE3D <= 1.05 * gap, (gap, nr.GAP_NOISE3D)


def test_3d_inputs_reach_every_case_the_issue_names():
    assert len(nr.CASES_3D) == 2 * 2 * 3 * 2 * 2
    assert nr.PER_BIG > 16384 * 256 and nr.NVOX % 256 != 0 and nr.NVOX % 2 == 1
    x = nr.volumes(3, 2)
    out, sg = nr.view3d(x, 5, 0, 0.0, 0.1, 0)
    assert 0.05 < np.abs(out - x).max() < 0.1 ** 0.5 * 6 and len(np.unique(sg)) == 3


# ---- 5. the 2D exclusion set --------------------------------------------------------------------------------------------------
def test_the_2d_exclusion_set_is_a_sliver_of_every_noisy_view():
    assert nr.CONTRACT_GENERATED == min(1e-4, 4 * 3.41e-7)
    from tests import test_gpu_sample as tg
    assert nr.CONTRACT_GENERATED == tg.CONTRACT["generated"]
    assert nr.DELTA == np.sqrt(50.0) * nr.CONTRACT_GENERATED + 2.0 ** -16 and 2 * nr.DELTA < 6e-5
    img = nr.images_2d()
    assert img.min() == 0 and img.max() == 255
    for image0 in nr.IMAGE0_2D:
        noise = nr.noise2d(nr.SEED_2D, image0, nr.B2, nr.H2, nr.W2, *nr.VAR_LIMIT)
        for codes in (nr.CODES_REF4, nr.CODES_8):
            for code in codes:
                if not code & 32:
                    continue
                for b in range(nr.B2):
                    pre = nr.noisy_view_pre(img[b], noise[b, (code >> 4) & 1], code)
                    share = nr.excluded(pre).mean()
                    assert share <= nr.EXCLUDED_SHARE_MAX, (image0, code, b, share)
                    clipped = ((pre < 0) | (pre > 255)).mean()
                    assert 0 < clipped < 0.2, "the inputs reach both clip ends"
