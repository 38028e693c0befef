"""CPU: the restatement of the validation step (tests/valstep_ref.py) against the recorded reference numbers
(tests/golden/valstep_kat.npz, tools/gen_golden_valstep.py) and against torch's CPU ops at test time; the host arithmetic
of values_amd.validation against the restatement's, its nan and ignore_index-quirk cases; the input builder's tie rule.

Bounds.  torch sums float32 terms: a float32 sum of n terms of magnitude mag is within (n + 4) * 2^-24 * mag of the exact
one (the 4: the roundings of the handful of operations that form a term).  A loss is a mean of such terms (and, with
SoftDice, a ratio of such sums of magnitude <= 1, taken twice): (n + 4) * 2^-24 * (mean |log term| + 2).  The SSN loss is
a logsumexp (slope <= 1) of sums of n log terms: (n + 4) * 2^-24 * max_s sum |lsm_t|.  Where the float32 samples were
formed by another expression order than torch's the restatement's own allowance for that is added (2 ulp32 per voxel).
Dice values are ratios of integers, exact in float64: one float32 ulp where the reference rounds them through float32.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import sample_ref as sr
from tests import valstep_ref as vr
from tests.helpers import load_npz

F32 = np.float32


def ulp1(v):
    return float(np.spacing(F32(abs(v))))


def sum_bound(n, mag_mean):
    return (n + 4) * 2.0 ** -24 * mag_mean


def soft_dice_torch(p, target):
    """SoftDiceLoss() with torch ops: one-hot by scatter, sums over the spatial axes, smooth 1e-5 in both places"""
    oh = torch.zeros_like(p).scatter_(1, target.unsqueeze(1), 1)
    ax = tuple(range(2, p.dim()))
    return (-((2 * (p * oh).sum(ax) + 1e-5) / ((p + oh).sum(ax) + 1e-5))).mean()


def torch_plain(logits, target, ig):
    x, t = torch.from_numpy(logits), torch.from_numpy(target.astype(np.int64))
    if ig != 0:
        return float(F.cross_entropy(x, t, ignore_index=ig))
    return float(soft_dice_torch(F.softmax(x, 1), t) + F.cross_entropy(x, t))


def torch_aleatoric(samples, target):
    y, t = torch.from_numpy(samples), torch.from_numpy(target.astype(np.int64))       # (B, T, C, nvox)
    lavg = torch.logsumexp(F.log_softmax(y, dim=2), 1) - math.log(y.shape[1])
    return float(soft_dice_torch(torch.exp(lavg), t) + F.nll_loss(lavg, t)), torch.argmax(torch.exp(lavg), 1).numpy()


def torch_ssn(samples, target, ig):
    y, t = torch.from_numpy(samples), torch.from_numpy(target.astype(np.int64))       # (B, S, C, nvox)
    B, S, C, nvox = y.shape
    flat = y.transpose(0, 1).reshape(S * B, C, nvox)
    tt = t[None].expand(S, B, nvox).reshape(S * B, nvox)
    ce = F.cross_entropy(flat, tt, ignore_index=ig, reduction="none") if ig != 0 else F.cross_entropy(flat, tt, reduction="none")
    return float(-torch.mean(torch.logsumexp((-ce).view(S, B, nvox).sum(-1), 0) - math.log(S)))


def golden_samples(g, rank):
    B, C = g["logits"].shape[:2]
    nvox = int(np.prod(g["logits"].shape[2:]))
    S, R = g["eps_w"].shape[0], g["eps_w"].shape[2]
    head = g["head"].reshape(B, -1, nvox)
    if rank == 0:
        head = head[:, :2 * C]
    return sr.ssn(head, g["eps_w"] if rank else None, g["eps_d"], 0, B, S, C, rank, nvox, float(g["epsilon"]), dtype=F32)


# ---- the restatement against the recorded reference numbers ----------------------------------------------------------------------
@pytest.mark.parametrize("ig", [0, 1])
def test_restatement_reproduces_the_golden_numbers(ig):
    g = load_npz("valstep_kat.npz")
    B, C = g["logits"].shape[:2]
    nvox = int(np.prod(g["logits"].shape[2:]))
    n = B * nvox
    seg = g["seg"].reshape(B, nvox)
    ce_ig = vr.ce_ignore_label(ig)
    # deterministic
    sums, mag, _ = vr.np_val_sums(g["logits"].reshape(B, C, nvox), seg, ce_ig)
    loss, dice = vr.loss_dice_from_sums(sums, C, nvox, ig)
    tol = sum_bound(n, mag[:, 5 * C].sum() / max(sums[:, 5 * C + 1].sum(), 1) + 2)
    print(f"plain ig={ig}: loss {loss:.9g} golden {g[f'plain_loss_{ig}']:.9g} d {abs(loss - g[f'plain_loss_{ig}']):.2e} tol {tol:.2e}")
    assert abs(loss - float(g[f"plain_loss_{ig}"])) <= tol
    assert abs(dice - float(g[f"plain_dice_{ig}"])) <= ulp1(dice)
    # aleatoric
    T = g["eps_aleatoric"].shape[1]
    smp, _ = sr.aleatoric(g["mu_s"].reshape(B, 2 * C, nvox), g["eps_aleatoric"].reshape(B, T, C, nvox), 0, B, T, C, nvox, dtype=F32)
    sums, mag, allow = vr.np_val_aleatoric_sums(smp.astype(F32), seg, -1, numpy_samples=True)
    loss, dice = vr.loss_dice_from_sums(sums, C, nvox, ig, aleatoric=True)
    tol = sum_bound(n, mag[:, 5 * C].sum() / n + 2) + allow[:, 5 * C].sum() / n
    print(f"aleatoric ig={ig}: loss {loss:.9g} golden {g[f'aleatoric_loss_{ig}']:.9g} tol {tol:.2e}")
    assert abs(loss - float(g[f"aleatoric_loss_{ig}"])) <= tol
    assert abs(dice - float(g[f"aleatoric_dice_{ig}"])) <= ulp1(dice)
    # SSN, full rank and mean_only
    for name, rank in (("ssn", g["eps_w"].shape[2]), ("ssn_mean_only", 0)):
        smp = golden_samples(g, rank).astype(F32)
        ss, smag, sallow, ts = vr.np_val_ssn_sums(smp, seg, ce_ig, numpy_samples=True)
        loss, dice = vr.ssn_loss_dice_from_sums(ss, ts, C, ig)
        tol = sum_bound(nvox, smag[:, :, 0].max()) + sallow[:, :, 0].max()
        print(f"{name} ig={ig}: loss {loss:.9g} golden {g[f'{name}_loss_{ig}']:.9g} tol {tol:.2e}")
        assert abs(loss - float(g[f"{name}_loss_{ig}"])) <= tol
        assert abs(dice - float(g[f"{name}_dice_{ig}"])) <= ulp1(dice)


# ---- the restatement against torch at test time ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,nvox,ig", [(2, 63, 0), (3, 120, 1), (8, 257, 255), (19, 40, 0), (2, 1, 0)])
def test_plain_restatement_against_torch(C, nvox, ig):
    rng = np.random.default_rng(100 + C + nvox)
    B = 2
    y = vr.separated_logits(rng, (B, C, nvox))
    lab = vr.place_labels(rng, B, nvox, C, ig if ig else None)
    sums, mag, _ = vr.np_val_sums(y, lab, vr.ce_ignore_label(ig))
    loss, dice = vr.loss_dice_from_sums(sums, C, nvox, ig)
    want = torch_plain(y, lab, ig)
    tol = sum_bound(B * nvox, mag[:, 5 * C].sum() / max(sums[:, 5 * C + 1].sum(), 1) + 2)
    print(f"plain C={C} nvox={nvox} ig={ig}: {loss:.9g} torch {want:.9g} d {abs(loss - want):.2e} tol {tol:.2e}")
    assert abs(loss - want) <= tol
    # the counts against numpy's own arg-max
    am = y.argmax(1)
    for c in range(C):
        assert sums[:, 5 * c + 4].sum() == (am == c).sum() and sums[:, 5 * c + 3].sum() == ((am == c) & (lab == c)).sum()
        assert sums[:, 5 * c + 1].sum() == (lab == c).sum()


@pytest.mark.parametrize("C,T,nvox", [(2, 1, 63), (2, 10, 120), (8, 32, 65)])
def test_aleatoric_restatement_against_torch(C, T, nvox):
    rng = np.random.default_rng(200 + C + T)
    B = 2
    smp = vr.separated_logits(rng, (B, T, C, nvox))
    lab = vr.place_labels(rng, B, nvox, C, None)
    sums, mag, _ = vr.np_val_aleatoric_sums(smp, lab, -1)
    loss, _ = vr.loss_dice_from_sums(sums, C, nvox, 0, aleatoric=True)
    want, am = torch_aleatoric(smp, lab)
    # torch's float32 chain: log_softmax, logsumexp over T, then the mean: (T + C) more float32 operations per term
    tol = sum_bound(B * nvox + T + C, mag[:, 5 * C].sum() / (B * nvox) + 2)
    print(f"aleatoric C={C} T={T} nvox={nvox}: {loss:.9g} torch {want:.9g} d {abs(loss - want):.2e} tol {tol:.2e}")
    assert abs(loss - want) <= tol
    agree = sum(sums[:, 5 * c + 4].sum() == (am == c).sum() for c in range(C))
    assert agree == C


@pytest.mark.parametrize("C,S,nvox,ig", [(2, 1, 63, 0), (2, 10, 120, 1), (8, 32, 65, 255)])
def test_ssn_restatement_against_torch(C, S, nvox, ig):
    rng = np.random.default_rng(300 + C + S)
    B = 3
    smp = vr.separated_logits(rng, (B, S, C, nvox))
    lab = vr.place_labels(rng, B, nvox, C, ig if ig else None)
    ss, smag, _, ts = vr.np_val_ssn_sums(smp, lab, vr.ce_ignore_label(ig))
    loss, _ = vr.ssn_loss_dice_from_sums(ss, ts, C, ig)
    want = torch_ssn(smp, lab, ig)
    tol = sum_bound(nvox + C, smag[:, :, 0].max())
    print(f"ssn C={C} S={S} nvox={nvox} ig={ig}: {loss:.9g} torch {want:.9g} d {abs(loss - want):.2e} tol {tol:.2e}")
    assert abs(loss - want) <= tol
    am = smp.argmax(2)
    for c in range(C):
        assert (ss[:, :, 1 + C + c] == (am == c).sum(-1)).all()
        assert (ss[:, :, 1 + c] == ((am == c) & (lab[:, None] == c)).sum(-1)).all()
        assert (ts[:, c] == (lab == c).sum(-1)).all()
    assert ts[:, C].sum() == ((lab < C) & (lab != vr.ce_ignore_label(ig))).sum() and ts[:, C + 1].sum() == 0


# ---- host arithmetic ---------------------------------------------------------------------------------------------------------------
def test_host_arithmetic_of_the_package_is_the_restatement():
    from values_amd import validation as va
    rng = np.random.default_rng(7)
    B, C, S, nvox = 3, 3, 5, 50
    y = vr.separated_logits(rng, (B, C, nvox))
    lab = vr.place_labels(rng, B, nvox, C, 1)
    for ig in (0, 1, 2):
        sums, _, _ = vr.np_val_sums(y, lab, vr.ce_ignore_label(ig))
        assert va.ce_ignore_label(ig) == vr.ce_ignore_label(ig)
        for al in (False, True):
            a, b = va.loss_dice_from_sums(sums, C, ig, aleatoric=al), vr.loss_dice_from_sums(sums, C, nvox, ig, aleatoric=al)
            assert np.allclose(a, b, rtol=1e-15, atol=0), (ig, al, a, b)
        smp = vr.separated_logits(rng, (B, S, C, nvox))
        ss, _, _, ts = vr.np_val_ssn_sums(smp, lab, vr.ce_ignore_label(ig))
        a, b = va.ssn_loss_dice_from_sums(ss, ts, C, ig), vr.ssn_loss_dice_from_sums(ss, ts, C, ig)
        assert np.allclose(a, b, rtol=1e-15, atol=0), (ig, a, b)


def test_quirk_ignore_index_zero_ignores_nothing_and_adds_soft_dice():
    """ignore_index == 0: label 0 takes its log term and the loss is SoftDice + CE; ignore_index == 1: CE over the voxels
    whose label is not 1, alone; the Dice deletes column ignore_index either way"""
    rng = np.random.default_rng(11)
    C, nvox = 2, 30
    y = vr.separated_logits(rng, (1, C, nvox))
    lab = vr.place_labels(rng, 1, nvox, C, None)
    s0, _, _ = vr.np_val_sums(y, lab, vr.ce_ignore_label(0))
    s1, _, _ = vr.np_val_sums(y, lab, vr.ce_ignore_label(1))
    assert s0[0, 5 * C + 1] == nvox and s1[0, 5 * C + 1] == (lab != 1).sum() < nvox
    l0, d0 = vr.loss_dice_from_sums(s0, C, nvox, 0)
    l1, d1 = vr.loss_dice_from_sums(s1, C, nvox, 1)
    assert abs(l0 - torch_plain(y, lab, 0)) < 1e-5 and abs(l1 - torch_plain(y, lab, 1)) < 1e-5
    am = y[0].argmax(0)
    for ig, d in ((0, d0), (1, d1)):
        k = 1 - ig                                            # the class that is left
        tp, fp, fn = ((am == k) & (lab[0] == k)).sum(), ((am == k) & (lab[0] != k)).sum(), ((am != k) & (lab[0] == k)).sum()
        assert d == 2.0 * tp / (2 * tp + fp + fn)


def test_all_ignored_batch_is_nan_as_in_torch():
    from values_amd import validation as va
    rng = np.random.default_rng(12)
    C, nvox = 2, 20
    y = vr.separated_logits(rng, (2, C, nvox))
    lab = np.ones((2, nvox), np.uint8)
    sums, _, _ = vr.np_val_sums(y, lab, 1)
    assert sums[:, 5 * C + 1].sum() == 0
    assert math.isnan(vr.loss_dice_from_sums(sums, C, nvox, 1)[0]) and math.isnan(va.loss_dice_from_sums(sums, C, 1)[0])
    assert math.isnan(torch_plain(y, lab, 1))
    # the SSN loss of an all-ignored batch: every log term is 0, logsumexp_s 0 - log S = 0
    smp = vr.separated_logits(rng, (2, 4, C, nvox))
    ss, _, _, ts = vr.np_val_ssn_sums(smp, lab, 1)
    assert vr.ssn_loss_dice_from_sums(ss, ts, C, 1)[0] == 0.0 == torch_ssn(smp, lab, 1)


def test_invalid_labels_are_counted_not_summed():
    rng = np.random.default_rng(13)
    C, nvox = 3, 40
    y = vr.separated_logits(rng, (2, C, nvox))
    lab = vr.place_labels(rng, 2, nvox, C, 255, invalid=True)
    sums, _, _ = vr.np_val_sums(y, lab, 255)
    assert sums[0, 5 * C + 2] == 0 and sums[1, 5 * C + 2] == 1
    assert sums[:, 5 * C + 1].sum() == (lab < C).sum()


# ---- the builder ---------------------------------------------------------------------------------------------------------------------
def test_builder_tie_condition():
    one = F32(1.0)
    near = np.array([[one], [one + F32(np.spacing(one)) * 3]], F32)       # 3 ulps apart: too close to call
    far = np.array([[one], [one + F32(np.spacing(one)) * 9]], F32)
    tie = np.array([[one], [one]], F32)
    assert not vr.top_two_gap_ok(near) and vr.top_two_gap_ok(far) and vr.top_two_gap_ok(tie)
    rng = np.random.default_rng(3)
    y = vr.separated_logits(rng, (2, 4, 9), tie_at=((1,), 5))
    assert (y[1, :, 5] == y[1, 0, 5]).all()
    a, lsm, _, _ = vr.log_softmax64(y)
    assert a[1, 5] == 0 and np.allclose(lsm[1, :, 5], -math.log(4))
