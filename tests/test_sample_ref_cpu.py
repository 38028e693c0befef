"""CPU: tests/sample_ref.py, the restatement the GPU sampling tests compare with -- against the oracle, the reference's
recorded SSN samples (ssn_16.npz) and the aleatoric formula; its float32 gaps on the inputs of tests/test_gpu_sample.py;
and the properties of the Gaussian generator it restates (vx_gauss, accumulate.hip).  The restatement is deterministic,
so the statistical bounds below are fixed numbers for fixed seeds: nothing here can flake."""
import numpy as np
import pytest

from tests import sample_ref as sr
from tests.formula import formula_tensor
from tests.helpers import load_npz

SEEDS = (0, 3, 5, 1234)
SLOTS, LEN = 64, 8192


# ---- parity with the reference ---------------------------------------------------------------------------------------
def test_ssn_equals_the_oracle_rsample_at_batch_three():
    from oracle.ssn_oracle import lowrank_rsample
    N, S, C, R, nvox = 3, 2, 2, 3, 37
    E = C * nvox
    loc, logd = formula_tensor((N, E), 11, 4.0), formula_tensor((N, E), 12, 2.0)
    fac = formula_tensor((N, R, E), 13, 1.0)                        # [n][r][c*nvox + v]: head channel r*C + c
    ew, ed = formula_tensor((S, N, R), 14, 1.7), formula_tensor((S, N, E), 15, 1.7)
    head = np.concatenate([loc.reshape(N, C, nvox), logd.reshape(N, C, nvox), fac.reshape(N, R * C, nvox)], axis=1)
    eps = float(np.float32(1e-5))
    got = sr.ssn(head, ew, ed, 0, N, S, C, R, nvox, 1e-5)
    want = lowrank_rsample(loc, np.exp(logd) + eps, fac.transpose(0, 2, 1), ew, ed)          # (S, N, E)
    np.testing.assert_allclose(got.reshape(N, S, E).transpose(1, 0, 2), want, rtol=0, atol=1e-13)
    # a transposed (s, n) stride of either normal does not survive this batch
    assert np.abs(sr.ssn(head, ew.transpose(1, 0, 2).reshape(S, N, R), ed, 0, N, S, C, R, nvox, 1e-5) - got).max() > 0.1


def test_ssn_reproduces_the_reference_fixture():
    g = load_npz("ssn_16.npz")
    NC, R, vox = 2, 10, 16 ** 3
    S = g["samples"].shape[0]
    loc, diag, fac = g["loc"].astype(np.float64), g["cov_diag"].astype(np.float64), g["cov_factor"].astype(np.float64)
    head = np.concatenate([loc.reshape(1, NC, vox), np.log(diag - 1e-5).reshape(1, NC, vox),
                           fac[0].T.reshape(1, R * NC, vox)], axis=1)
    got = sr.ssn(head, g["eps_w"], g["eps_d"], 0, 1, S, NC, R, vox, 1e-5)
    # 2e-6: the bound test_oracle_golden.test_ssn_oracle_matches_reference holds the oracle to on this fixture
    np.testing.assert_allclose(got.reshape(1, S, -1).transpose(1, 0, 2), g["samples"], rtol=0, atol=2e-6)


def test_aleatoric_equals_the_reference_formula():
    """test_3D.py:458-469: output = mu + exp(s / 2) * eps"""
    N, T, C, nvox = 2, 3, 2, 41
    mu, s = formula_tensor((N, C, nvox), 21, 4.0), formula_tensor((N, C, nvox), 22, 2.0)
    eps = formula_tensor((N, T, C, nvox), 23, 1.7)
    out, sigma = sr.aleatoric(np.concatenate([mu, s], 1), eps, 0, N, T, C, nvox)
    np.testing.assert_allclose(out, mu[:, None] + np.exp(s[:, None] / 2) * eps, rtol=0, atol=1e-14)
    np.testing.assert_allclose(sigma, np.exp(s / 2), rtol=0, atol=1e-15)


def test_ssn2d_is_the_3d_formula_in_two_steps():
    """comb + add_diag on channels-last inputs = the planar rsample (bilinear interpolation left out: factor 1)"""
    B, pix, S, C, R = 2, 13, 3, 3, 2
    mean, fac = formula_tensor((B * pix, 5), 31, 4.0), formula_tensor((B * pix, 8), 32, 1.0)
    ew, ed = formula_tensor((S, B, R), 33, 1.7), formula_tensor((S, B, C * pix), 34, 1.7)
    comb, expm = sr.ssn2d_lowres(mean, 5, fac, 8, ew, 0, B, pix, S, C, R)
    np.testing.assert_allclose(expm, np.exp(mean[:, :C]), rtol=0, atol=1e-13)
    planar = comb.reshape(S, B, pix, C).transpose(1, 0, 3, 2).reshape(B, S, C * pix)             # [b][s][c][p]
    diag = expm.reshape(B, pix, C).transpose(0, 2, 1).reshape(B, C * pix)
    got = sr.ssn2d_add_diag(planar, diag, ed, 0, S, B, C * pix, 1e-5)
    head = np.concatenate([mean[:, :C].reshape(B, pix, C).transpose(0, 2, 1), mean[:, :C].reshape(B, pix, C).transpose(0, 2, 1),
                           fac[:, :R * C].reshape(B, pix, R * C).transpose(0, 2, 1)], axis=1)
    np.testing.assert_allclose(got.reshape(B, S, C, pix), sr.ssn(head, ew, ed, 0, B, S, C, R, pix, 1e-5), rtol=0, atol=1e-13)


def test_generated_normals_fill_the_documented_slots():
    N, T, S, C, R, nvox, seed = 2, 3, 2, 2, 3, 5, 9
    out, _ = sr.aleatoric(np.zeros((N, 2 * C, nvox)), None, seed, N, T, C, nvox)
    for n, t, c, v in ((0, 0, 0, 0), (1, 2, 1, 4), (1, 0, 0, 3)):
        assert out[n, t, c, v] == sr.gauss(seed, c * nvox + v, n * T + t)
    head = np.zeros((N, (2 + R) * C, nvox))
    head[:, 2 * C:] = formula_tensor((N, R * C, nvox), 41, 1.0)
    got = sr.ssn(head, None, None, seed, N, S, C, R, nvox, 0.0)
    for n, s, c, v in ((0, 0, 0, 0), (1, 1, 1, 4), (1, 0, 1, 2)):
        low = sum(head[n, 2 * C + k * C + c, v] * sr.gauss(seed ^ 0x5bd1e995, k, n * S + s) for k in range(R))
        assert abs(got[n, s, c, v] - (low + sr.gauss(seed, c * nvox + v, n * S + s))) < 1e-14
    # the hash in plain Python integers, beside the masked uint64 arithmetic of the restatement
    def mix(h):
        h ^= h >> 16
        h = h * 0x7feb352d & 0xFFFFFFFF
        h ^= h >> 15
        h = h * 0x846ca68b & 0xFFFFFFFF
        return h ^ h >> 16
    for sd, a, b in ((0, 0, 0), (5, 1, 1), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (1234, 2 * 1029 - 1, 11)):
        h1 = mix(a * 0x9E3779B1 & 0xFFFFFFFF ^ mix(sd ^ (b * 0x85EBCA6B + 0x165667B1 & 0xFFFFFFFF)))
        h2 = mix(h1 ^ 0x27D4EB2F ^ (a * 0xC2B2AE35 & 0xFFFFFFFF))
        assert tuple(int(w) for w in sr.gauss_words(sd, a, b)) == (h1, h2)
    assert int(sr.mix32(0)) == 0 and int(sr.stream_key(0, 0)) == 0x165667B1


def test_pack_and_colorize_restatements():
    x = formula_tensor((2, 3, 2, 3, 4), 51, 1.0)
    out = sr.pack_input_cl8(x, 4, 2, None, [0, 1, 6, 7])
    assert out.shape == (4, 2, 3, 4, 8) and (out[..., 3:] == 0).all()
    np.testing.assert_array_equal(out[0, ..., :3], np.moveaxis(x[0], 0, -1))
    np.testing.assert_array_equal(out[1, ..., :3], np.moveaxis(x[0][:, ::-1], 0, -1))
    np.testing.assert_array_equal(out[2, ..., :3], np.moveaxis(x[1][:, :, ::-1, ::-1], 0, -1))
    np.testing.assert_array_equal(out[3, ..., :3], np.moveaxis(x[1][:, ::-1, ::-1, ::-1], 0, -1))
    np.testing.assert_array_equal(sr.pack_input_cl8(x, 3, 1, [1, 1, 0], None)[2, ..., :3], np.moveaxis(x[0], 0, -1))
    lut = np.arange(768, dtype=np.uint8).reshape(256, 3)
    rgb = sr.colorize(np.array([0, 7, 255], np.uint8), np.array([0, 1, 0], np.uint8), lut, 9)
    np.testing.assert_array_equal(rgb, lut[[0, 9, 255]])
    np.testing.assert_array_equal(sr.colorize(np.array([7], np.uint8), None, lut, 9), lut[[7]])


# ---- the float32 gaps the GPU module's bounds are built on ---------------------------------------------------------------
def test_float32_gaps_of_the_restatement_are_the_constants_of_the_gpu_test():
    """tests/test_gpu_sample.py: GAP[group] is the largest difference between the restatement in float64 and in its
    float32 form over that module's own inputs, to two digits; CONTRACT = min(1e-4, 4 x GAP)"""
    from tests import test_gpu_sample as tg
    gap = {k: 0.0 for k in tg.GAP}
    for group, name, rel, ref in tg.reference_matrix():
        a, b = ref(np.float64), ref(np.float32)
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert y.dtype == np.float32 and x.dtype == np.float64, name
            gap[group] = max(gap[group], tg.deviation(y, x, rel))
    print("gaps", {k: f"{v:.3e}" for k, v in gap.items()})
    for k, const in tg.GAP.items():
        assert gap[k] <= const <= 1.05 * gap[k], (k, gap[k], const)
        assert tg.CONTRACT[k] == min(1e-4, 4 * const)
        assert tg.REG[k] == min(tg.CONTRACT[k], 5 * tg.OBS[k])


def test_gpu_inputs_reach_the_magnitudes_the_fixtures_have():
    from tests import test_gpu_sample as tg
    mu_s, eps = tg.aleatoric_case(2, 5)
    assert 7.0 < np.abs(sr.aleatoric(mu_s, eps, 0, 3, 5, 2, tg.NVOX)[0]).max() < 12.0
    head, ew, ed = tg.ssn_case(3, 2, 2, 10)
    assert 7.0 < np.abs(sr.ssn(head, ew, ed, 0, 3, 2, 2, 10, tg.NVOX, 1e-5)).max() < 16.0
    assert len(np.unique(ew)) == ew.size and len(np.unique(ed[:, :, 0, 0])) == 6


# ---- the generator --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def streams():
    """seed -> (64, 8192) float64: the first 8192 elements of slots 0..63"""
    out = {s: sr.gauss(s, np.arange(LEN)[None, :], np.arange(SLOTS)[:, None]) for s in SEEDS + tuple(s + 1 for s in SEEDS)}
    for v in out.values():
        v.setflags(write=False)
    return out


def _corr(a, b):
    a, b = a - a.mean(-1, keepdims=True), b - b.mean(-1, keepdims=True)
    return (a * b).sum(-1) / np.sqrt((a * a).sum(-1) * (b * b).sum(-1))


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_moments_and_stream_independence(streams, seed):
    """z-score bounds: a standard normal sample of n values has mean ~ N(0, 1/n), variance ~ N(1, 2/n), fourth moment
    ~ N(3, 96/n); the correlation of two independent streams of m values ~ N(0, 1/m)"""
    z = streams[seed]
    n = z.size
    assert abs(z.mean()) < 4 / np.sqrt(n)
    assert abs(z.var() - 1) < 4 * np.sqrt(2 / n)
    assert abs((z ** 4).mean() - 3) < 4 * np.sqrt(96 / n)
    c = np.corrcoef(z)
    pairs = np.abs(c[np.triu_indices(SLOTS, 1)])
    assert pairs.size == 2016 and pairs.max() < 5 / np.sqrt(LEN), pairs.max()
    # successive draws of LowRankNormal (seed * 7919 + draws) use seeds s and s + 1: their streams are unrelated too
    nxt = streams[seed + 1]
    cross = np.abs(np.corrcoef(z, nxt)[:SLOTS, SLOTS:])
    assert cross.shape == (SLOTS, SLOTS) and cross.max() < 5 / np.sqrt(LEN), cross.max()


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_has_no_serial_correlation(seed):
    """lag 1, and lag nvox: element c*nvox + v and (c+1)*nvox + v are the same voxel of neighbouring classes"""
    nvox = 4096
    z = sr.gauss(seed, np.arange(2 * nvox)[None, :], np.arange(8)[:, None])
    n = z[:, :-1].size
    assert abs(_corr(z[:, :-1].reshape(-1), z[:, 1:].reshape(-1))) < 5 / np.sqrt(n)
    n = z[:, :nvox].size
    assert abs(_corr(z[:, :nvox].reshape(-1), z[:, nvox:].reshape(-1))) < 5 / np.sqrt(n)
    for lag_nvox in (1029, 16 ** 3):            # the class stride of the GPU tests and of the 16^3 fixtures
        y = sr.gauss(seed, np.arange(2 * lag_nvox)[None, :], np.arange(8)[:, None])
        assert abs(_corr(y[:, :lag_nvox].reshape(-1), y[:, lag_nvox:].reshape(-1))) < 5 / np.sqrt(8 * lag_nvox)


@pytest.mark.parametrize("seed", SEEDS)
def test_eps_w_streams_share_nothing_with_eps_d_streams(streams, seed):
    R = 10
    w = sr.gauss(seed ^ sr.W_XOR, np.arange(R)[None, :], np.arange(SLOTS)[:, None])
    d = streams[seed][:, :R]
    assert not np.isin(w, d).any()
    slots = np.arange(SLOTS)
    assert not np.isin(sr.stream_key(seed ^ sr.W_XOR, slots), sr.stream_key(seed, slots)).any()


def test_stream_keys_of_the_default_seeds_do_not_collide():
    """a stream is keyed by ONE word, seed ^ (slot * 0x85EBCA6B + 0x165667B1): two (seed, slot) pairs with the same word
    are the same stream.  Seeds 1234..1238 (the default member seeds of predict._predict_logits_aleatoric), their
    ^ 0x5bd1e995 partners (eps_w), slots below 4096."""
    seeds = [s for m in range(1234, 1239) for s in (m, m ^ sr.W_XOR)]
    keys = np.concatenate([sr.stream_key(s, np.arange(4096)) for s in seeds])
    assert keys.size == 10 * 4096 and len(np.unique(keys)) == keys.size
    assert len(np.unique(sr.mix32(keys))) == keys.size           # (vx_mix32 is a bijection)


def test_uniforms_keep_the_logarithm_finite_and_bound_the_normals(streams):
    for seed in SEEDS:
        u1, u2 = sr.uniforms(seed, np.arange(LEN)[None, :], np.arange(SLOTS)[:, None])
        assert u1.min() >= 2.0 ** -24 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
        assert np.isfinite(streams[seed]).all() and np.abs(streams[seed]).max() <= np.sqrt(48 * np.log(2))
    # the extreme words: h1 >> 8 = 0 gives the largest radius, h1 >> 8 = 2^24 - 1 gives u1 = 1 and z = 0
    for dtype in (np.float64, np.float32):
        assert np.isfinite(np.sqrt(dtype(-2) * np.log(dtype(2.0 ** -24))))
    assert np.array_equal(sr.uniforms(0, 0, 0)[0].astype(np.float32).astype(np.float64), sr.uniforms(0, 0, 0)[0])
