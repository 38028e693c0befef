"""CPU: pins tests/ops2d_ref.py (the host restatement the GPU matrix of tests/test_gpu_ops2d.py compares the 2D kernels
with) to torch's float64 / float32 operations and to oracle/hrnet_oracle.py, and checks the conditions on the GPU
matrix's inputs under which its contracts are derivable."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hrnet_oracle
from tests import ops2d_ref as R
from tests.formula import formula_tensor


def _cl(t):
    """NCHW torch -> channels-last numpy"""
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("src,dst", [((8, 15), (16, 30)), ((8, 15), (32, 60)), ((8, 15), (64, 120)), ((16, 30), (8, 15)),
                                     ((7, 9), (14, 18)), ((6, 10), (3, 5))])
def test_f64_twin_equals_f_interpolate_at_dyadic_ratios(src, dst):
    """ratios 1/2, 1/4, 1/8 (HRNet's upsamples) and 2 (downscale): the float32 source coordinates are exact there, so the
    float64 twin IS F.interpolate(float64) up to the rounding of its four products and three sums"""
    x = R.f32_tensor((2, *src, 8), 301, scale=2.0)
    got = R.affine_gather_f64(x, out_hw=dst)
    ref = _cl(F.interpolate(_nchw(x).double(), size=dst, mode="bilinear", align_corners=False))
    bound = 4 * 2.0 ** -52 * R.corner_abs_sum(x, dst)
    assert got.shape == ref.shape and (np.abs(got - ref) <= bound).all(), np.abs(got - ref).max()
    # ... and the float32 restatement is the float64 twin rounded a few times
    g32 = R.affine_gather_f32(x, out_hw=dst)
    assert g32.dtype == np.float32 and (np.abs(g32 - got) <= 4 * 2.0 ** -24 * R.corner_abs_sum(x, dst)).all()


@pytest.mark.parametrize("src,dst", [((64, 120), (256, 478)), ((5, 7), (9, 20))])
def test_f32_restatement_matches_f_interpolate_at_non_dyadic_ratios(src, dst):
    """ratios 120/478 and 7/20: ATen's CPU kernel (index / weight tables) and the float32 closed form differ by ~1e-5 in
    the interpolation weight -- the bound of test_bilinear_matches_f_interpolate"""
    x = R.f32_tensor((2, *src, 8), 231)
    ref = _cl(F.interpolate(_nchw(x), size=dst, mode="bilinear", align_corners=False)).astype(np.float64)
    assert np.abs(R.affine_gather_f32(x, out_hw=dst).astype(np.float64) - ref).max() < 2e-5
    assert np.abs(R.affine_gather_f64(x, out_hw=dst) - ref).max() < 2e-5


def test_bil_coord_edges():
    for n_in, n_out in ((8, 64), (16, 8), (7, 20), (120, 478), (1, 5)):
        i0, i1, l1 = R.bil_coord_f32(np.arange(n_out), n_in, n_out)
        assert i0.min() == 0 and i1.max() == n_in - 1 and (i1 - i0 <= 1).all() and (i1 >= i0).all()
        assert (l1 >= 0).all() and (l1 < 1).all() and l1.dtype == np.float32
        assert l1[0] == 0 or n_in > n_out          # upsampling: the first output sits before the first source centre
        assert (i1[i0 == n_in - 1] == n_in - 1).all()


def test_bn_scale_shift_exact_is_batch_norm_training():
    """x * scale + shift with (scale, shift) from partials that are exact sums rounded ONCE to float32, against
    F.batch_norm(training=True) in float64 and the oracle's _bn.  The rounding of (sum, sumsq) moves the mean by 2^-24 |mu|
    and the variance by 2^-24 (var + mu^2); with the offsets below mu^2 / var <= 0.75 + sampling, so rstd moves by about
    2^-24 and the result by no more than 2 x 2^-24 (|x scale| + |mu scale|); beta takes the sign of -mu, which makes |shift| =
    |beta| + |mu scale| -- the bound 8 x 2^-24 (|x scale| + |shift|) has a factor 4 to spare (float32's eps differs from 1e-5
    by 2.5e-8 of itself: 4e-13 of rstd)."""
    n, h, w, c = 3, 9, 13, 20
    off = 0.5 * formula_tensor((c,), 312)
    x = (formula_tensor((n, h, w, c), 311) + off).astype(np.float32)
    gamma = (1 + formula_tensor((c,), 313, 0.3)).astype(np.float32)
    beta = (-np.sign(off) * np.abs(formula_tensor((c,), 314, 0.2))).astype(np.float32)
    tiles = np.array_split(x.astype(np.float64).reshape(-1, c), 4)           # four "tiles" of 88, 88, 88, 87 pixels
    part = np.stack([np.stack([t.sum(0), (t * t).sum(0)], -1) for t in tiles]).astype(np.float32)
    scale, shift = R.bn_scale_shift_exact(part, n * h * w, R.EPS32, gamma, beta)
    mu = x.astype(np.float64).mean((0, 1, 2))
    assert (np.sign(shift) == np.sign(beta)).all() and (mu * mu / x.astype(np.float64).var((0, 1, 2)) <= 1.5).all()
    got = x.astype(np.float64) * scale + shift
    bound = 8 * 2.0 ** -24 * (np.abs(x.astype(np.float64) * scale) + np.abs(shift))
    xt, g, b = _nchw(x).double(), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double()
    ref = _cl(F.batch_norm(xt, None, None, g, b, training=True, eps=1e-5))
    assert (np.abs(got - ref) <= bound).all(), (np.abs(got - ref) / bound).max()
    ora = _cl(hrnet_oracle._bn(xt, {"bn.weight": g, "bn.bias": b}, "bn"))
    assert (np.abs(got - ora) <= bound).all()
    # null gamma / beta mean 1 / 0
    s1, h1 = R.bn_scale_shift_exact(part, n * h * w)
    ref1 = _cl(F.batch_norm(xt, None, None, None, None, training=True, eps=1e-5))
    got1 = x.astype(np.float64) * s1 + h1
    assert (np.abs(got1 - ref1) <= 8 * 2.0 ** -24 * (np.abs(x * s1) + np.abs(h1))).all()
    # grouped form: rows of [G][cpitch], nobody's columns are NaN
    sg, hg = R.bn_scale_shift_exact_groups(np.concatenate([part, part[::-1] * np.float32(0.5)]), 2, 36, n * h * w, R.EPS32, gamma, beta)
    assert sg.shape == (2, 36) and np.array_equal(sg[0, :c], scale) and np.array_equal(hg[0, :c], shift)
    assert np.isnan(sg[:, c:]).all() and np.isnan(hg[:, c:]).all() and not np.array_equal(sg[1, :c], scale)


def test_bn_variance_clamp_cases():
    """the two degenerate inputs of the GPU matrix: var == 0 exactly, and a sumsq partial rounded DOWN so that q / n < mu^2"""
    part, count = R.clamp_partials()
    n = count
    p = part.astype(np.float64).sum(0)
    mu = p[:, 0] / n
    assert p[0, 1] / n - mu[0] * mu[0] == 0.0               # constant 0.5, power-of-two count: exact sums
    assert p[1, 1] / n - mu[1] * mu[1] < 0.0                # rounded-down sumsq: negative before the clamp
    scale, shift = R.bn_scale_shift_exact(part, n, R.EPS32, np.array([1.5, 0.75], np.float32), None)
    want = np.array([1.5, 0.75]) / np.sqrt(float(R.EPS32))
    assert np.isfinite(scale).all() and np.isfinite(shift).all() and (np.abs(scale - want) <= 2.0 ** -50 * want).all()


def test_fuse_twin_equals_the_oracle_module_fuse_step():
    """HighResolutionModule's SUM fusion of branch 0 out of three (hrnet_oracle._module with no blocks): y = x0 +
    up2(bn(conv1x1(x1))) + up4(bn(conv1x1(x2))), relu.  The twin takes the raw 1x1 outputs with BN folded to scale / shift
    AFTER the resize (interpolation weights sum to 1).  Float64 on O(10) values with some twenty operations per element:
    20 x 10 x 2^-52 = 5e-14; the bound is 1e-12."""
    n, chans, hw = 2, (4, 8, 12), (8, 12)
    xs = [torch.from_numpy(formula_tensor((n, c, hw[0] >> i, hw[1] >> i), 320 + i, 2.0)) for i, c in enumerate(chans)]
    sd = {}
    for i in range(3):
        for j in range(3):
            if j > i:
                sd[f"m.fuse_layers.{i}.{j}.0.weight"] = torch.from_numpy(formula_tensor((chans[i], chans[j], 1, 1), 330 + 3 * i + j, 0.5))
                sd[f"m.fuse_layers.{i}.{j}.1.weight"] = torch.from_numpy(1 + formula_tensor((chans[i],), 340 + 3 * i + j, 0.3))
                sd[f"m.fuse_layers.{i}.{j}.1.bias"] = torch.from_numpy(formula_tensor((chans[i],), 350 + 3 * i + j, 0.2))
            elif j < i:
                for k in range(i - j):
                    co = chans[i] if k == i - j - 1 else chans[j]
                    sd[f"m.fuse_layers.{i}.{j}.{k}.0.weight"] = torch.from_numpy(formula_tensor((co, chans[j], 3, 3), 360 + 9 * i + 3 * j + k, 0.2))
                    sd[f"m.fuse_layers.{i}.{j}.{k}.1.weight"] = torch.ones(co, dtype=torch.float64)
                    sd[f"m.fuse_layers.{i}.{j}.{k}.1.bias"] = torch.zeros(co, dtype=torch.float64)
    ref = _cl(hrnet_oracle._module(xs, sd, "m", 3, [0, 0, 0], "BASIC")[0])
    terms = [(_cl(xs[0]), None, None)]
    for j in (1, 2):
        t = F.conv2d(xs[j], sd[f"m.fuse_layers.0.{j}.0.weight"])
        mu, var = t.mean((0, 2, 3)), t.var((0, 2, 3), unbiased=False)
        scale = sd[f"m.fuse_layers.0.{j}.1.weight"] / torch.sqrt(var + 1e-5)
        terms.append((_cl(t), scale.numpy(), (sd[f"m.fuse_layers.0.{j}.1.bias"] - mu * scale).numpy()))
    got = R.fuse_sum_f64(terms, hw, relu=True)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 and ref.max() > 1.0
    assert np.abs(R.fuse_sum_f64(terms, hw) - R.fuse_sum_f64(terms, hw, relu=True)).max() > 0.1      # relu acts on this input


def test_fusion_input_is_order_sensitive():
    """the float32 sum of the GPU matrix's fusion input depends on the term order: a kernel that adds its terms in another
    order cannot pass the `==` there"""
    terms, hw = R.order_sensitive_terms()
    fwd, rev = R.fuse_sum_f32(terms, hw), R.fuse_sum_f32(terms, hw, reverse=True)
    assert fwd.dtype == np.float32 and (fwd != rev).mean() > 0.05
    assert np.abs(R.fuse_sum_f64(terms, hw) - R.fuse_sum_f64(terms, hw, reverse=True)).max() < 1e-9   # ... only by rounding


@pytest.mark.parametrize("case", R.finalize_cases(), ids=R.finalize_case_id)
def test_finalize_inputs_meet_the_one_ulp_condition(case):
    """mean^2 / var <= 1e4 on every channel of every vx_bn_finalize input of the GPU matrix: var = q/n - mu^2 then loses at
    most log2(1e4) = 14 of float64's 53 bits, and another float64 summation order (ntiles x 2^-53 relative on s and q)
    moves scale / shift by ntiles x 2^-53 x 1e4 < 2^-29 of themselves: far below half a float32 ulp."""
    part, count = R.finalize_partials(case.ntiles, case.C, case.tag, case.G)
    assert part.shape == (case.G * case.ntiles, case.C, 2) and part.dtype == np.float32
    p = part.astype(np.float64).reshape(case.G, case.ntiles, case.C, 2).sum(1)
    mu = p[..., 0] / count
    var = p[..., 1] / count - mu * mu
    assert (var > 0).all() and (mu * mu / var <= 1e4).all()
    if case.G > 1:                                       # groups differ visibly
        sc, sh = R.bn_scale_shift_exact_groups(part, case.G, case.cpitch, count)
        for g in range(1, case.G):
            assert (np.abs(sh[g, :case.C] - sh[0, :case.C]) > 1e-3).mean() > 0.5


def test_hash_keep_mask_layout():
    m = R.hash_keep_mask(123, 3, 2, 100)
    a, b = R._np_key(123, 3, 1)
    w = R._np_words(int(a), int(b), 4)
    assert m.shape == (2, 100) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}
    assert all(int(m[1, e]) == (int(w[e // 32]) >> (e % 32)) & 1 for e in range(100))
    assert not np.array_equal(m[0], m[1]) and 0.3 < m.mean() < 0.7


def test_bilinear_nchw_slots_and_flips():
    x = R.f32_tensor((3, 4, 6, 5), 371)
    out = R.bilinear_nchw_f64(x, (8, 12), slots=4, dst=[2, 0, 3], flip=[0, 1, 3], fill=-77.0)
    ref = F.interpolate(_nchw(x).double(), size=(8, 12), mode="bilinear", align_corners=False).numpy()
    assert np.abs(out[2] - ref[0]).max() < 1e-14 and np.abs(out[0] - ref[1][:, :, ::-1]).max() < 1e-14
    assert np.abs(out[3] - ref[2][:, ::-1, ::-1]).max() < 1e-14 and (out[1] == -77.0).all()


def test_conv2d_prologue_case_table_names_the_listed_instances():
    """static: the case table of the GPU matrix names every split-fp16 instance the prologue has to run on, and chunked layers
    with resident and with re-staged weights (the GPU test asserts that the named instance is the one that ran)"""
    from tests.test_gpu_ops2d import K, PROLOGUE_CASES
    names = {p[9] for p in PROLOGUE_CASES}
    for want in (K % (3, 1, 1, 1, 0), K % (3, 1, 2, 2, 0), K % (3, 1, 3, 3, 0), K % (3, 2, 3, 1, 0), K % (1, 1, 1, 4, 0), K % (1, 1, 2, 4, 0),
                 K % (1, 1, 3, 4, 0), K % (1, 1, 5, 4, 0), K % (3, 1, 1, 1, 1), K % (3, 1, 2, 1, 3), K % (3, 2, 3, 1, 3), K % (3, 2, 1, 1, 1)):
        assert want in names, want
    assert {(p[10] > 1, p[11]) for p in PROLOGUE_CASES} >= {(True, 0), (True, 1), (False, 0)}


def test_logits_pitch_keeps_the_softmax_upsample_on_a_vector_instance():
    from values_amd.hrnet import _softmax_pitch
    for c in range(1, 41):
        p, q = _softmax_pitch(c), (c + 3) // 4
        assert p % 4 == 0 and p >= 4 * q
        if q <= 8:
            assert p == 4 * min(Q for Q in (1, 2, 5, 8) if Q >= q)
        else:
            assert p == 4 * q
    assert _softmax_pitch(19) == 20 and _softmax_pitch(5) == 8 and _softmax_pitch(2) == 4
