"""GPU: the validation step's fused reductions (valstep.hip) against their float64 restatement (tests/valstep_ref.py),
and the drivers of values_amd.validation.

Integer slots (class counts, arg-max counts, valid / invalid counts) are ==.  A float slot is within
valstep_ref.float_bound: n * 2^-52 * mag for the order of the float64 additions, the per-term allowance for the device's
double exp / log (ULP_DEV and its source are in valstep_ref.py) and, where the float32 samples were formed in numpy and
not by the device's own sample kernel, sum_v 2 ulp32(max_c |y_c|).  The input builders assert on the CPU that every
sample's top-two logit gap is wider than 4 float32 ulps (or an intended exact tie), so the arg-max counts cannot depend
on whose float32 expression formed the sample.
"""
import numpy as np
import pytest
import torch

from tests import valstep_ref as vr
from tests.helpers import load_npz
from values_amd import _lib
from values_amd import validation as va

pytestmark = pytest.mark.gpu
F32 = np.float32
NVOX = (1, 63, 120, 257, 4097)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def check_row(got, want, mag, allow, n, C, name):
    """a (B, 5C + 3) result against the restatement: integer slots ==, float slots within the bound"""
    ints = vr.int_slots(C)
    flt = [k for k in range(5 * C + 3) if k not in ints]
    assert np.array_equal(got[:, ints], want[:, ints]), (name, "integer slots", got[:, ints], want[:, ints])
    bound = vr.float_bound(n, mag[:, flt], allow[:, flt])
    d = np.abs(got[:, flt] - want[:, flt])
    worst = float((d / np.maximum(bound, 1e-300)).max())
    print(f"valstep {name}: max |d| {d.max():.3e}, worst d / bound {worst:.3f}")
    assert (d <= bound).all(), (name, d.max(), worst)


def check_ssn(got_ss, got_ts, want, n, C, name):
    ss, smag, sallow, ts = want
    assert np.array_equal(got_ts, ts), (name, "target sums", got_ts, ts)
    assert np.array_equal(got_ss[:, :, 1:], ss[:, :, 1:]), (name, "arg-max counts")
    bound = vr.float_bound(n, smag[:, :, 0], sallow[:, :, 0])
    d = np.abs(got_ss[:, :, 0] - ss[:, :, 0])
    worst = float((d / np.maximum(bound, 1e-300)).max())
    print(f"valstep {name}: max |d| {d.max():.3e}, worst d / bound {worst:.3f}")
    assert (d <= bound).all(), (name, d.max(), worst)


# ---- a. the deterministic kernel ------------------------------------------------------------------------------------------------------
PLAIN = [(B, C, nvox, ig) for k, nvox in enumerate(NVOX) for B, C, ig in
         [((1, 3)[k % 2], (2, 8, 19)[k % 3], (-1, 0, 255)[k % 3]), ((3, 1)[k % 2], (8, 19, 2)[k % 3], (0, 255, -1)[k % 3]),
          (3, (19, 2, 8)[k % 3], (255, -1, 0)[k % 3])]]


@pytest.mark.parametrize("B,C,nvox,ig", PLAIN)
def test_plain_kernel_against_restatement(B, C, nvox, ig):
    rng = np.random.default_rng(1000 + 7 * nvox + C + B)
    y = vr.separated_logits(rng, (B, C, nvox), tie_at=((0,), nvox // 3))
    lab = vr.place_labels(rng, B, nvox, C, ig)
    got = va.val_sums(dev(y), dev(lab), ig)
    want, mag, allow = vr.np_val_sums(y, lab, ig)
    check_row(got, want, mag, allow, nvox, C, f"plain B={B} C={C} nvox={nvox} ig={ig}")
    # the tie voxel went to class 0
    assert vr.log_softmax64(y[0])[0][nvox // 3] == 0


# ---- b. the aleatoric kernel, injected normals --------------------------------------------------------------------------------------
ALEATORIC = [(1, 2, 1, 1, -1), (3, 8, 10, 63, 0), (1, 8, 32, 120, 255), (3, 2, 32, 257, 0), (3, 2, 10, 4097, 255), (1, 8, 1, 4097, -1),
             (3, 8, 32, 63, -1), (1, 2, 10, 120, 0)]


@pytest.mark.parametrize("B,C,T,nvox,ig", ALEATORIC)
def test_aleatoric_kernel_against_restatement(B, C, T, nvox, ig):
    rng = np.random.default_rng(2000 + 7 * nvox + C + T)
    mu_s, eps, y = vr.aleatoric_case(rng, B, T, C, nvox)
    lab = vr.place_labels(rng, B, nvox, C, ig)
    got = va.val_sums_aleatoric(dev(mu_s), dev(lab), T, dev(eps), 0, 0, ig)
    want, mag, allow = vr.np_val_aleatoric_sums(y, lab, ig, numpy_samples=True)
    check_row(got, want, mag, allow, nvox, C, f"aleatoric B={B} C={C} T={T} nvox={nvox} ig={ig}")


# ---- c. the SSN kernel, injected normals ----------------------------------------------------------------------------------------------
SSN = [(1, 2, 1, 0, 1, -1), (3, 8, 10, 3, 63, 0), (1, 8, 32, 10, 120, 255), (3, 2, 32, 3, 257, 0), (3, 2, 10, 10, 4097, 255),
       (1, 8, 1, 0, 4097, -1), (3, 8, 32, 0, 63, -1), (1, 2, 10, 10, 120, 0), (3, 8, 10, 10, 257, 255), (1, 2, 1, 3, 63, 0)]


@pytest.mark.parametrize("B,C,S,R,nvox,ig", SSN)
def test_ssn_kernel_against_restatement(B, C, S, R, nvox, ig):
    rng = np.random.default_rng(3000 + 7 * nvox + C + S + R)
    head, ew, ed, y = vr.ssn_case(rng, B, S, C, R, nvox)
    lab = vr.place_labels(rng, B, nvox, C, ig)
    ss, ts = va.val_sums_ssn(dev(head), dev(lab), C, R, S, dev(ew), dev(ed), 0, 0, 1e-5, ig)
    check_ssn(ss, ts, vr.np_val_ssn_sums(y, lab, ig, numpy_samples=True), nvox, C, f"ssn B={B} C={C} S={S} R={R} nvox={nvox} ig={ig}")


# ---- d. generated normals: the fused result against the restatement on the samples the sample kernels write ----------------------
def device_aleatoric_samples(mu_s, seed, B, T, C, nvox):
    out = torch.empty((B, T, C, nvox), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().vx_aleatoric_sample(mu_s.data_ptr(), None, seed, B, T, C, nvox, out.data_ptr(), None, _lib.stream_ptr()),
               "vx_aleatoric_sample")
    return out.cpu().numpy()


def device_ssn_samples(head, seed, B, S, C, R, nvox, epsilon=1e-5):
    out = torch.empty((B, S, C, nvox), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().vx_ssn_sample(head.data_ptr(), None, None, seed, B, S, C, R, nvox, epsilon, out.data_ptr(), _lib.stream_ptr()),
               "vx_ssn_sample")
    return out.cpu().numpy()


@pytest.mark.parametrize("B,C,T,nvox,seed", [(3, 2, 10, 4097, 77), (1, 8, 32, 257, 0xDEADBEEF)])
def test_aleatoric_generated_is_the_sample_kernels_stream(B, C, T, nvox, seed):
    rng = np.random.default_rng(4000 + nvox)
    mu_s, _, _ = vr.aleatoric_case(rng, B, T, C, nvox, tie=False)
    lab = vr.place_labels(rng, B, nvox, C, 0)
    m = dev(mu_s)
    got = va.val_sums_aleatoric(m, dev(lab), T, None, seed, 0, 0)
    want, mag, allow = vr.np_val_aleatoric_sums(device_aleatoric_samples(m, seed, B, T, C, nvox), lab, 0)
    check_row(got, want, mag, allow, nvox, C, f"aleatoric generated B={B} C={C} T={T} nvox={nvox}")


@pytest.mark.parametrize("B,C,S,R,nvox,seed", [(3, 2, 10, 10, 4097, 78), (1, 8, 32, 3, 257, 0xDEADBEEF), (2, 2, 10, 0, 120, 5)])
def test_ssn_generated_is_the_sample_kernels_stream(B, C, S, R, nvox, seed):
    rng = np.random.default_rng(5000 + nvox)
    head, _, _, _ = vr.ssn_case(rng, B, S, C, R, nvox, tie=False)
    lab = vr.place_labels(rng, B, nvox, C, 0)
    h = dev(head)
    ss, ts = va.val_sums_ssn(h, dev(lab), C, R, S, None, None, seed, 0, 1e-5, 0)
    check_ssn(ss, ts, vr.np_val_ssn_sums(device_ssn_samples(h, seed, B, S, C, R, nvox), lab, 0), nvox, C,
              f"ssn generated B={B} C={C} S={S} R={R} nvox={nvox}")


# ---- e. an item alone is bit-equal to the same item among batch mates -------------------------------------------------------------------
def test_item_alone_is_bit_equal_to_its_row_in_a_batch():
    rng = np.random.default_rng(6000)
    B, C, S, R, T, nvox, k, seed = 3, 2, 10, 3, 10, 2500, 2, 99
    lab = vr.place_labels(rng, B, nvox, C, 0)
    g = dev(lab)
    y = dev(vr.separated_logits(rng, (B, C, nvox)))
    assert np.array_equal(va.val_sums(y, g, 0)[k], va.val_sums(y[k:k + 1], g[k:k + 1], 0)[0])
    mu_s, eps, _ = vr.aleatoric_case(rng, B, T, C, nvox)
    m, e = dev(mu_s), dev(eps)
    assert np.array_equal(va.val_sums_aleatoric(m, g, T, e, 0, 0, 0)[k], va.val_sums_aleatoric(m[k:k + 1], g[k:k + 1], T, e[k:k + 1], 0, 0, 0)[0])
    # generated: the streams are keyed by item0 + b, so the item alone draws its own with item0 = k
    assert np.array_equal(va.val_sums_aleatoric(m, g, T, None, seed, 0, 0)[k], va.val_sums_aleatoric(m[k:k + 1], g[k:k + 1], T, None, seed, k, 0)[0])
    assert not np.array_equal(va.val_sums_aleatoric(m, g, T, None, seed, 0, 0)[k], va.val_sums_aleatoric(m[k:k + 1], g[k:k + 1], T, None, seed, 0, 0)[0])
    head, ew, ed, _ = vr.ssn_case(rng, B, S, C, R, nvox)
    h, w, d = dev(head), dev(ew), dev(ed)
    for inj in (True, False):
        full = va.val_sums_ssn(h, g, C, R, S, w if inj else None, d if inj else None, seed, 0, 1e-5, 0)
        one = va.val_sums_ssn(h[k:k + 1], g[k:k + 1], C, R, S, w[:, k:k + 1] if inj else None, d[:, k:k + 1] if inj else None, seed,
                              0 if inj else k, 1e-5, 0)
        assert np.array_equal(full[0][k], one[0][0]) and np.array_equal(full[1][k], one[1][0]), inj
    # ... and a chunked batch: items 1.. with item0 = 1 are rows 1.. of the whole
    full = va.val_sums_ssn(h, g, C, R, S, None, None, seed, 0, 1e-5, 0)
    tail = va.val_sums_ssn(h[1:], g[1:], C, R, S, None, None, seed, 1, 1e-5, 0)
    assert np.array_equal(full[0][1:], tail[0])


# ---- f. invalid labels -------------------------------------------------------------------------------------------------------------------
def test_invalid_label_is_counted_and_raises():
    rng = np.random.default_rng(7000)
    B, C, S, R, T, nvox = 2, 2, 3, 2, 3, 130
    lab = vr.place_labels(rng, B, nvox, C, 255, invalid=True)
    g = dev(lab)
    y = dev(vr.separated_logits(rng, (B, C, nvox)))
    got = va.val_sums(y, g, 255, raise_invalid=False)
    assert got[0, 5 * C + 2] == 0 and got[1, 5 * C + 2] == 1 and got[:, 5 * C + 1].sum() == (lab < C).sum()
    with pytest.raises(ValueError):
        va.val_sums(y, g, 255)
    mu_s, eps, _ = vr.aleatoric_case(rng, B, T, C, nvox)
    assert va.val_sums_aleatoric(dev(mu_s), g, T, dev(eps), 0, 0, 255, raise_invalid=False)[1, 5 * C + 2] == 1
    with pytest.raises(ValueError):
        va.val_sums_aleatoric(dev(mu_s), g, T, dev(eps), 0, 0, 255)
    head, ew, ed, _ = vr.ssn_case(rng, B, S, C, R, nvox)
    assert va.val_sums_ssn(dev(head), g, C, R, S, dev(ew), dev(ed), 0, 0, 1e-5, 255, raise_invalid=False)[1][1, C + 1] == 1
    with pytest.raises(ValueError):
        va.val_sums_ssn(dev(head), g, C, R, S, dev(ew), dev(ed), 0, 0, 1e-5, 255)
    # a label that no uint8 holds is invalid too, not wrapped into a class
    wide = torch.from_numpy(lab.astype(np.int64)).cuda()
    wide[0, 1] = 256 + 1
    assert va.val_sums(y, wide, 255, raise_invalid=False)[0, 5 * C + 2] == 1


# ---- g. validation_step on the golden inputs ------------------------------------------------------------------------------------------------
class _Logits:
    def __init__(self, out, **attrs):
        self.out = out
        self.__dict__.update(attrs)

    def __call__(self, x, **kw):
        return self.out


def _golden_ssn_model(g):
    from values_amd import SsnUNet3D
    from values_amd.ssn import LowRankNormal
    C, R = g["logits"].shape[1], g["eps_w"].shape[2]
    head = dev(g["head"])

    class Fixed(SsnUNet3D):
        def forward(self, x, mean_only=False, **kw):
            h = head[:, :2 * C].contiguous() if mean_only else head
            return LowRankNormal(h, C, 0 if mean_only else R, float(g["epsilon"]), 0)

    return Fixed(num_classes=C, rank=R)


@pytest.mark.parametrize("ig", [0, 1])
def test_validation_step_reproduces_the_golden_numbers(ig):
    """the bounds of tests/test_valstep_ref_cpu.py (float32 summation of the reference, one float32 ulp for a Dice)"""
    from tests.test_valstep_ref_cpu import golden_samples, sum_bound, ulp1
    g = load_npz("valstep_kat.npz")
    B, C = g["logits"].shape[:2]
    nvox = int(np.prod(g["logits"].shape[2:]))
    seg, x = dev(g["seg"]), torch.zeros((B, 1) + g["logits"].shape[2:], device="cuda")
    T, S = g["eps_aleatoric"].shape[1], g["eps_w"].shape[0]
    mean_lt = 4.0   # mean |log term| of these inputs is below 2 (the recorded losses); + 2 for the SoftDice share

    def close(res, name, tol):
        dl, dd = abs(res["validation/val_loss"] - float(g[f"{name}_loss_{ig}"])), abs(res["validation/val_dice"] - float(g[f"{name}_dice_{ig}"]))
        print(f"valstep golden {name} ig={ig}: loss {res['validation/val_loss']:.9g} d {dl:.2e} (tol {tol:.2e}), dice d {dd:.2e}")
        assert dl <= tol and dd <= ulp1(res["validation/val_dice"]), (name, res)

    close(va.validation_step(_Logits(dev(g["logits"])), x, seg, ignore_index=ig), "plain", sum_bound(B * nvox, mean_lt))
    mu_s = dev(g["mu_s"])
    al = _Logits(tuple(mu_s.split(C, 1)), aleatoric_loss=True)
    close(va.validation_step(al, x, seg, n_aleatoric_samples=T, ignore_index=ig, eps=dev(g["eps_aleatoric"])), "aleatoric",
          sum_bound(B * nvox, mean_lt))
    model = _golden_ssn_model(g)
    eps = (dev(g["eps_w"]), dev(g["eps_d"]))
    for name, rank in (("ssn", g["eps_w"].shape[2]), ("ssn_mean_only", 0)):
        _, smag, sallow, _ = vr.np_val_ssn_sums(golden_samples(g, rank).astype(F32), g["seg"].reshape(B, nvox), vr.ce_ignore_label(ig),
                                                numpy_samples=True)
        close(va.validation_step(model, x, seg, n_aleatoric_samples=S, ignore_index=ig, eps=eps, mean_only=rank == 0), name,
              sum_bound(nvox, smag[:, :, 0].max()) + sallow[:, :, 0].max())
    with pytest.raises(NotImplementedError):
        va.validation_step(_Logits(dev(g["logits"]), ssn=True), x, seg)


# ---- h. the drivers on the three 3D model kinds, 16^3 -------------------------------------------------------------------------------------
def _capture(model):
    seen = []
    orig = model.forward

    def fwd(*a, **kw):
        out = orig(*a, **kw)
        seen.append(out)
        return out

    model.forward = fwd
    return seen


def _loss_tol(sums, mag, allow, n, C):
    """what the float bounds of the slots allow the loss to move by: the log-term mean, and each SoftDice ratio by twice
    the relative movement of its sums"""
    b = vr.float_bound(n, mag, allow)
    nval = max(sums[:, 5 * C + 1].sum(), 1)
    soft = max(2 * (b[:, 5 * c] + b[:, 5 * c + 2]).max() / (sums[:, 5 * c + 2] + sums[:, 5 * c + 1] + 1e-5).min() for c in range(C))
    return b[:, 5 * C].sum() / nval + soft


def test_drivers_equal_the_materialised_route():
    from tests.formula import formula_ssn_state_dict, formula_unet3d_state_dict, formula_volume
    from values_amd import SsnUNet3D, UNet3D
    NC, R, size, B, S, seed = 2, 10, 16, 2, 10, 4321
    nvox = size ** 3
    x = torch.from_numpy(np.concatenate([formula_volume((1, 1, size, size, size), tag=t) for t in (7, 8)], 0)).float().cuda()
    rng = np.random.default_rng(8000)
    lab = vr.place_labels(rng, B, nvox, NC, None)
    seg = dev(lab.reshape(B, 1, size, size, size))
    for ig in (0, 1):
        ce_ig = vr.ce_ignore_label(ig)
        # plain
        m = UNet3D(num_classes=NC)
        m.load_state_dict({k: torch.from_numpy(v).float() for k, v in formula_unet3d_state_dict().items()})
        m = m.cuda()
        seen = _capture(m)
        res = va.validation_step(m, x, seg, ignore_index=ig)
        sums, mag, allow = vr.np_val_sums(seen[-1].float().cpu().numpy().reshape(B, NC, nvox), lab, ce_ig)
        loss, dice = vr.loss_dice_from_sums(sums, NC, nvox, ig)
        tol = _loss_tol(sums, mag, allow, nvox, NC) if ig == 0 else vr.float_bound(nvox, mag, allow)[:, 5 * NC].sum() / sums[:, 5 * NC + 1].sum()
        print(f"valstep driver plain ig={ig}: {res} d {abs(res['validation/val_loss'] - loss):.2e} tol {tol:.2e}")
        assert abs(res["validation/val_loss"] - loss) <= tol and res["validation/val_dice"] == dice
        # aleatoric
        m = UNet3D(num_classes=NC, aleatoric_loss=True)
        m.load_state_dict({k: torch.from_numpy(v).float() for k, v in formula_unet3d_state_dict(seed_tag=4, aleatoric_loss=True).items()})
        m = m.cuda()
        seen = _capture(m)
        res = va.validation_step(m, x, seg, n_aleatoric_samples=S, ignore_index=ig, seed=seed)
        mu_s = torch.cat(seen[-1], 1).float().reshape(B, 2 * NC, nvox).contiguous()
        sums, mag, allow = vr.np_val_aleatoric_sums(device_aleatoric_samples(mu_s, seed, B, S, NC, nvox), lab, -1)
        loss, dice = vr.loss_dice_from_sums(sums, NC, nvox, ig, aleatoric=True)
        tol = _loss_tol(sums, mag, allow, nvox, NC)
        print(f"valstep driver aleatoric ig={ig}: {res} d {abs(res['validation/val_loss'] - loss):.2e} tol {tol:.2e}")
        assert abs(res["validation/val_loss"] - loss) <= tol and res["validation/val_dice"] == dice
        # SSN, full rank and mean_only
        m = SsnUNet3D(num_classes=NC, rank=R)
        m.load_state_dict({k: torch.from_numpy(v).float() for k, v in formula_ssn_state_dict(NC, R).items()}, strict=True)
        m = m.cuda()
        seen = _capture(m)
        for mean_only in (False, True):
            res = va.validation_step(m, x, seg, n_aleatoric_samples=S, ignore_index=ig, seed=seed, mean_only=mean_only)
            dist = seen[-1]
            smp = device_ssn_samples(dist.head.reshape(B, -1, nvox), seed, B, S, NC, dist.rank, nvox, float(dist.epsilon))
            ss, smag, sallow, ts = vr.np_val_ssn_sums(smp, lab, ce_ig)
            loss, dice = vr.ssn_loss_dice_from_sums(ss, ts, NC, ig)
            tol = vr.float_bound(nvox, smag[:, :, 0], sallow[:, :, 0]).max()
            print(f"valstep driver ssn mean_only={mean_only} ig={ig}: {res} d {abs(res['validation/val_loss'] - loss):.2e} tol {tol:.2e}")
            assert abs(res["validation/val_loss"] - loss) <= tol and abs(res["validation/val_dice"] - dice) <= 1e-15


# ---- i. epoch means -------------------------------------------------------------------------------------------------------------------------
def test_validate_weights_the_epoch_means_by_batch_size():
    rng = np.random.default_rng(9000)
    C, nvox = 3, 200
    batches, models = [], []
    for B in (1, 2):
        y = dev(vr.separated_logits(rng, (B, C, nvox)))
        batches.append({"data": torch.zeros((B, 1, nvox), device="cuda"), "seg": dev(vr.place_labels(rng, B, nvox, C, None)), "out": y})

    class ByBatch:
        def __call__(self, x, **kw):
            return next(b["out"] for b in batches if b["data"].shape[0] == x.shape[0])

    res = va.validate(ByBatch(), batches)
    per = [va.validation_step(ByBatch(), b["data"], b["seg"]) for b in batches]
    assert res["batches"] == per and len(per) == 2 and per[0] != per[1]
    for k in ("validation/val_loss", "validation/val_dice"):
        assert res[k] == (1 * per[0][k] + 2 * per[1][k]) / 3
