"""CPU: the restatement of the 2D SSN head's validation reduction (tests/valstep2d_ref.py) pinned two ways.

(a) To torch at test time.  The reference route (HighResolutionNet.hrnet_ssn + forward_ssn(val=True)) interpolates the mean,
exp(mean) + epsilon and the FACTOR to full resolution with F.interpolate(bilinear, align_corners=False), samples
LowRankMultivariateNormal.rsample there (its normals captured) and runs cross_entropy / logsumexp / arg-max over the samples.
The restatement combines at low resolution and interpolates once per sample -- the same real number (interpolation is linear),
float32 roundings apart.  K_ULP: the worst deviation between the two routes' samples, in ulp32 of the pixel's largest
|logit|, measured on this matrix on the CPU (x86-64, torch's CPU kernels): 48 (C = 2, R = 0), 64 (C = 2, R = 3), 6 (C = 19,
R = 0), 4 (C = 19, R = 3) -- with two classes both logits of a pixel can be small beside the terms they were added from;
the worst, doubled: K_ULP = 128.  The test asserts the premise (measured deviation <= K_ULP / 2) before it uses the bound.
    loss:  |d| <= max_{b,s} sum_v 2 K_ULP ulp32(max_c |y|)          (log-softmax: slope <= 2)
                  + sum_bound(nvox + C, max_{b,s} sum_v |lsm_t|)       (torch's float32 summation, test_valstep_ref_cpu)
    Dice:  one float32 ulp (the reference rounds the S values through float32), on inputs whose top-two gap exceeds K_ULP
           ulp32 (asserted), so no arg-max depends on the route.

(b) To tests/golden/valstep2d_kat.npz (tools/gen_golden_valstep2d.py): the reference's own HighResolutionNet.hrnet_ssn on a
formula feature map, ignore_index 0 and 255, full rank and mean_only -- the same loss bound; the Dice, which the reference
averages in a float32 tensor of S values, within f32_mean_bound(S).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import valstep2d_ref as v2
from tests import valstep_ref as vr
from tests.helpers import load_npz
from tests.test_valstep_ref_cpu import sum_bound, torch_ssn, ulp1

F32 = np.float32
K_ULP = 128


def torch_samples(mean, fac, eps_w, eps_d, C, R, H, W, epsilon):
    """hrnet_ssn's distribution from the low-resolution head (channels-last numpy, as valstep2d_ref takes it) and its
    rsample with the given normals -> (B, S, C, H * W) float32"""
    import torch.distributions.lowrank_multivariate_normal as lrm
    B, S = mean.shape[0], eps_d.shape[0]
    up = lambda t: F.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)   # noqa: E731
    m = torch.from_numpy(np.ascontiguousarray(mean[..., :C])).permute(0, 3, 1, 2).contiguous()
    loc = up(m).reshape(B, -1)
    cov_diag = up(m.exp() + epsilon).reshape(B, -1)
    if R:
        f = torch.from_numpy(np.ascontiguousarray(fac[..., :R * C])).permute(0, 3, 1, 2).contiguous()
        cov_factor = up(f).view(B, R, C, -1).flatten(2, 3).transpose(1, 2)
        ew = torch.from_numpy(np.asarray(eps_w, F32))
    else:
        cov_factor = torch.zeros([*cov_diag.shape, 1])     # the reference's mean_only factor (rank columns of zeros)
        ew = torch.zeros((S, B, 1))
    ed = torch.from_numpy(np.asarray(eps_d, F32)).reshape(S, B, -1)
    dist = torch.distributions.LowRankMultivariateNormal(loc=loc, cov_factor=cov_factor, cov_diag=cov_diag)
    drawn = [ew, ed]
    orig = lrm._standard_normal

    def fake(shape, dtype, device):
        t = drawn.pop(0)
        assert tuple(shape) == tuple(t.shape), (shape, t.shape)
        return t.to(dtype)

    lrm._standard_normal = fake
    try:
        smp = dist.rsample([S])
    finally:
        lrm._standard_normal = orig
    return smp.view(S, B, C, H * W).transpose(0, 1).contiguous().numpy()


def check_against(y, dmag, y_t, lab, C, ig, want_loss, want_dice, name, nvox, dice_tol=None):
    dev = float((np.abs(y.astype(np.float64) - y_t.astype(np.float64)).max(2) / vr.ulp32(np.abs(y).max(2))).max()) if y_t is not None else None
    if dev is not None:
        assert dev <= K_ULP / 2, (name, "the routes' samples are further apart than K_ULP assumes", dev)
    assert vr.top_two_gap_ok(y, n_ulp=K_ULP), (name, "a top-two gap within K_ULP ulp32")
    ce_ig = vr.ce_ignore_label(ig)
    ss, smag, sallow, ts = v2.np_val_ssn2d_sums(y, dmag, lab, ce_ig)
    loss, dice = vr.ssn_loss_dice_from_sums(ss, ts, C, ig)
    _, take, _ = vr._label_masks(lab, C, ce_ig)
    route = max(float((2 * K_ULP * vr.ulp32(np.abs(y[b, s]).max(0)))[take[b]].sum()) for b in range(y.shape[0]) for s in range(y.shape[1]))
    tol = route + sum_bound(nvox + C, smag[:, :, 0].max())
    print(f"valstep2d ref {name}: sample deviation {dev} ulp32; loss {loss:.9g} want {want_loss:.9g} d {abs(loss - want_loss):.3e} tol {tol:.3e}; "
          f"dice d {abs(dice - want_dice):.2e}")
    assert abs(loss - want_loss) <= tol, (name, loss, want_loss, tol)
    assert abs(dice - want_dice) <= (ulp1(dice) if dice_tol is None else dice_tol(dice)), (name, dice, want_dice)


@pytest.mark.parametrize("C", [2, 19])
@pytest.mark.parametrize("R", [0, 3])
@pytest.mark.parametrize("ig", [0, 255])
def test_restatement_against_the_reference_route_in_torch(C, R, ig):
    B, S, h0, w0, H, W = 2, 3, 5, 7, 19, 27
    rng = np.random.default_rng(400 + 10 * C + R)
    mean, fac, ew, ed, y, dmag = v2.case(rng, B, S, C, R, h0, w0, H, W, tie=False, min_gap_ulp=K_ULP)
    lab = vr.place_labels(rng, B, H * W, C, ig if ig else None)
    y_t = torch_samples(mean, fac, ew, ed, C, R, H, W, 1e-5)
    want = torch_ssn(y_t, lab, ig)
    am = y_t.argmax(2)                                                                   # (B, S, nvox)
    dice = np.array([vr.micro_dice([((am[:, s] == c) & (lab == c)).sum() for c in range(C)], [(am[:, s] == c).sum() for c in range(C)],
                                   [(lab == c).sum() for c in range(C)], C, ig) for s in range(S)], F32).mean(dtype=F32)
    check_against(y, dmag, y_t, lab, C, ig, want, float(dice), f"torch C={C} R={R} ig={ig}", H * W)


def f32_mean_bound(S):
    """the fixture's Dice is the reference's: S values, each rounded to float32, added in a float32 tensor and divided by S.
    The values are >= 0, so every partial sum is at most the total T: the S roundings of the values move it by <= 2^-24 T, the
    S - 1 additions by <= 2^-24 T each, the division by <= 2^-24 T / S  ->  (S + 1) 2^-24 of the mean"""
    return lambda dice: (S + 1) * 2.0 ** -24 * dice


def fixture_case(g, mean_only):
    """the stored head, channels-last, and the restatement's samples with the stored normals"""
    from tests.formula import formula_tensor
    B, C = g["mean_lo"].shape[:2]
    R = 0 if mean_only else g["factor_lo"].shape[1] // C
    H, W = (int(v) for v in g["size"])
    S = int(g["n_samples"])
    mean = np.ascontiguousarray(g["mean_lo"].transpose(0, 2, 3, 1))
    fac = np.ascontiguousarray(g["factor_lo"].transpose(0, 2, 3, 1)) if R else None
    eps_d = formula_tensor((S, B, C * H * W), tag=int(g["eps_d_tag"]), scale=1.7).astype(F32)
    y, dmag = v2.samples(mean, fac, g["eps_w"], eps_d, C, R, H, W, float(g["epsilon"]))
    return mean, fac, g["eps_w"], eps_d, y, dmag, (B, S, C, R, H, W)


@pytest.mark.parametrize("ig", [0, 255])
@pytest.mark.parametrize("mean_only", [False, True])
def test_restatement_reproduces_the_golden_numbers(ig, mean_only):
    g = load_npz("valstep2d_kat.npz")
    _, _, _, _, y, dmag, (B, S, C, R, H, W) = fixture_case(g, mean_only)
    name = "ssn_mean_only" if mean_only else "ssn"
    lab = g[f"seg_{ig}"].reshape(B, H * W)
    assert (lab == 255).any() == (ig == 255)
    check_against(y, dmag, None, lab, C, ig, float(g[f"{name}_loss_{ig}"]), float(g[f"{name}_dice_{ig}"]), f"golden {name} ig={ig}", H * W,
                  dice_tol=f32_mean_bound(S))


def test_interpolation_is_torchs_and_the_coordinates_have_their_edges():
    rng = np.random.default_rng(5)
    for (h0, w0), (H, W) in (((1, 1), (1, 1)), ((1, 1), (3, 5)), ((2, 3), (8, 12)), ((5, 7), (19, 27)), ((16, 24), (64, 96))):
        x = rng.standard_normal((2, h0, w0, 3)).astype(F32)
        want = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
        got = v2.interp(x, H, W)
        assert got.shape == want.shape and np.abs(got - want).max() <= 4 * np.spacing(F32(np.abs(x).max()))
        i0, i1, l1 = v2.bil_coord(np.arange(H), h0, H)
        assert i0.min() == 0 and i1.max() == h0 - 1 and (l1 >= 0).all() and (l1 < 1).all() and ((i1 - i0) <= 1).all()
    # a source of one pixel: both indices are 0 but the weight l = s - 0 is not (the clamp is on the index), so the pixel is
    # rebuilt from h * p + l * p -- a copy only at equal sizes, where every l is 0
    x = rng.standard_normal((1, 1, 1, 4)).astype(F32)
    assert (v2.interp(x, 1, 1) == x).all()
    assert v2.bil_coord(np.arange(3), 1, 3)[2].max() > 0
    assert np.abs(v2.interp(x, 3, 5) - x).max() <= 4 * np.spacing(F32(np.abs(x).max()))
