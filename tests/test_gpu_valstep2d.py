"""GPU: the 2D SSN head's fused validation reduction (vx_val_ssn2d_sums_batched, valstep.hip) against its restatement
(tests/valstep2d_ref.py) and against the materialised route (LowRankNormal2D.sample_images + the float64 sums of
tests/valstep_ref.py), and the drivers of values_amd.validation over an SSN HighResolutionNet.

Integer slots are ==.  The log-term slot is within valstep_ref.float_bound: against numpy-formed samples with the
numpy-samples allowance plus the diagonal term's (valstep2d_ref's docstring derives it: the device's expf and sqrtf enter
sd * eps_d); against the samples sample_images wrote -- the very values the kernel forms -- with the sharper device-formed
bound, which has no float32 allowance at all.
"""
import numpy as np
import pytest
import torch

from tests import valstep2d_ref as v2
from tests import valstep_ref as vr
from tests.helpers import load_npz
from values_amd import validation as va

pytestmark = pytest.mark.gpu
F32 = np.float32
GEOM = {"1": (1, 1, 1, 1), "1up": (1, 1, 3, 5), "x4": (2, 3, 8, 12), "odd": (5, 7, 19, 27), "64x96": (16, 24, 64, 96)}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def make_dist(mean, fac, C, R, H, W, epsilon=1e-5, seed=0):
    from values_amd.hrnet import LowRankNormal2D
    return LowRankNormal2D.from_lowres(dev(mean), dev(fac) if R else None, C, R, epsilon, (H, W), seed)


def check_ssn(got_ss, got_ts, want, n, name):
    ss, smag, sallow, ts = want
    assert np.array_equal(got_ts, ts), (name, "target sums", got_ts, ts)
    assert np.array_equal(got_ss[:, :, 1:], ss[:, :, 1:]), (name, "arg-max counts")
    bound = vr.float_bound(n, smag[:, :, 0], sallow[:, :, 0])
    d = np.abs(got_ss[:, :, 0] - ss[:, :, 0])
    worst = float((d / np.maximum(bound, 1e-300)).max())
    print(f"valstep2d {name}: max |d| {d.max():.3e}, worst d / bound {worst:.3f}")
    assert (d <= bound).all(), (name, d.max(), worst)
    return worst


# ---- 1. the kernel against the restatement, numpy-formed samples, injected normals -------------------------------------------------
# B, S, C, R, geometry, ignore_label: every geometry, B, C (2, 4, 19: register instances; 5, 32: the two-sweep form), S, R and
# ignore_label value at least once; 513 pixels ("odd") is two full spans plus one pixel
MATRIX = [(1, 1, 2, 0, "1", -1), (3, 10, 4, 3, "1up", 0), (1, 32, 19, 10, "x4", 255), (3, 10, 32, 3, "odd", 0),
          (3, 10, 19, 10, "64x96", 255), (1, 1, 32, 0, "x4", -1), (3, 32, 2, 10, "odd", 255), (1, 10, 4, 0, "64x96", -1),
          (3, 1, 19, 3, "odd", 0), (1, 10, 5, 3, "odd", 255), (3, 32, 19, 0, "1up", -1), (1, 10, 2, 10, "64x96", 0)]


@pytest.mark.parametrize("B,S,C,R,geom,ig", MATRIX)
def test_kernel_against_restatement(B, S, C, R, geom, ig):
    h0, w0, H, W = GEOM[geom]
    nvox = H * W
    rng = np.random.default_rng(1000 + 7 * nvox + 3 * C + S + R)
    # the head's own pitches: the mean at round4 / round16 of C, the factor at round16 of R C -- both above what is used
    pm, pf = (C + 15) // 16 * 16 + (4 if C % 16 == 0 else 0), (R * C + 15) // 16 * 16 + 16
    mean, fac, ew, ed, y, dmag = v2.case(rng, B, S, C, R, h0, w0, H, W, pm=pm, pf=pf, tie=nvox >= 3)
    assert pm > C
    lab = vr.place_labels(rng, B, nvox, C, ig)
    dist = make_dist(mean, fac, C, R, H, W)
    ss, ts = va.val_sums_ssn2d(dist, dev(lab), S, dev(ew) if R else None, dev(ed), 0, 0, ig)
    check_ssn(ss, ts, v2.np_val_ssn2d_sums(y, dmag, lab, ig), nvox, f"restatement B={B} S={S} C={C} R={R} {geom} ig={ig}")
    if nvox >= 3:   # the tie pixel went to class 0 in every sample
        assert (vr.log_softmax64(y[0])[0][:, nvox // 3] == 0).all()


# ---- 2. the bit-level tie to the existing route -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,C,R,geom,ig", [(2, 10, 19, 10, "64x96", 255), (3, 3, 32, 3, "odd", 0), (1, 10, 4, 0, "x4", -1),
                                             (2, 32, 2, 10, "1up", 0)])
@pytest.mark.parametrize("injected", [True, False])
def test_fused_sums_are_the_sums_of_the_samples_sample_images_writes(B, S, C, R, geom, ig, injected):
    h0, w0, H, W = GEOM[geom]
    nvox = H * W
    rng = np.random.default_rng(2000 + nvox + C)
    mean, fac, ew, ed, _, _ = v2.case(rng, B, S, C, R, h0, w0, H, W, tie=False)
    lab = vr.place_labels(rng, B, nvox, C, ig)
    seed = 0xDEADBEEF if C == 19 else 77
    dist = make_dist(mean, fac, C, R, H, W)
    kw = dict(eps_w=dev(ew) if R else None, eps_d=dev(ed)) if injected else {}
    smp = dist.sample_images(S, seed=seed, **kw).cpu().numpy().reshape(B, S, C, nvox)
    ss, ts = va.val_sums_ssn2d(dist, dev(lab), S, kw.get("eps_w"), kw.get("eps_d"), seed, 0, ig)
    worst = check_ssn(ss, ts, vr.np_val_ssn_sums(smp, lab, ig, numpy_samples=False), nvox,
                      f"device samples B={B} S={S} C={C} R={R} {geom} ig={ig} injected={injected}")
    # seed=None draws the distribution's next seed, as sample_images does: the two routes meet there too
    if not injected:
        d1, d2 = make_dist(mean, fac, C, R, H, W, seed=5), make_dist(mean, fac, C, R, H, W, seed=5)
        smp = d1.sample_images(S).cpu().numpy().reshape(B, S, C, nvox)
        ss2, ts2 = va.val_sums_ssn2d(d2, dev(lab), S, ignore_label=ig)
        check_ssn(ss2, ts2, vr.np_val_ssn_sums(smp, lab, ig, numpy_samples=False), nvox, "device samples, the distribution's seed")


# ---- 3. an item alone is bit-equal to its row in a batch -----------------------------------------------------------------------------
@pytest.mark.parametrize("C", [19, 5])
def test_item_alone_is_bit_equal_to_its_row_in_a_batch(C):
    rng = np.random.default_rng(3000 + C)
    B, S, R, k, seed = 3, 10, 3, 2, 99
    h0, w0, H, W = GEOM["odd"]
    nvox = H * W
    mean, fac, ew, ed, _, _ = v2.case(rng, B, S, C, R, h0, w0, H, W, tie=False)
    lab = vr.place_labels(rng, B, nvox, C, 0)
    g, w, d = dev(lab), dev(ew), dev(ed)
    whole = make_dist(mean, fac, C, R, H, W)
    one = make_dist(mean[k:k + 1], fac[k:k + 1], C, R, H, W)
    tail = make_dist(mean[1:], fac[1:], C, R, H, W)
    for inj in (True, False):
        full = va.val_sums_ssn2d(whole, g, S, w if inj else None, d if inj else None, seed, 0, 0)
        alone = va.val_sums_ssn2d(one, g[k:k + 1], S, w[:, k:k + 1] if inj else None, d[:, k:k + 1] if inj else None, seed, 0 if inj else k, 0)
        assert np.array_equal(full[0][k], alone[0][0]) and np.array_equal(full[1][k], alone[1][0]), inj
        rest = va.val_sums_ssn2d(tail, g[1:], S, w[:, 1:] if inj else None, d[:, 1:] if inj else None, seed, 0 if inj else 1, 0)
        assert np.array_equal(full[0][1:], rest[0]) and np.array_equal(full[1][1:], rest[1]), inj
    # the generated streams ARE keyed by the item: with item0 = 0 the item alone draws item 0's
    assert not np.array_equal(va.val_sums_ssn2d(whole, g, S, None, None, seed, 0, 0)[0][k],
                              va.val_sums_ssn2d(one, g[k:k + 1], S, None, None, seed, 0, 0)[0][0])


# ---- 4. invalid labels -----------------------------------------------------------------------------------------------------------------
def test_invalid_label_is_counted_and_raises():
    rng = np.random.default_rng(4000)
    B, S, C, R = 2, 3, 4, 2
    h0, w0, H, W = GEOM["x4"]
    nvox = H * W
    mean, fac, ew, ed, _, _ = v2.case(rng, B, S, C, R, h0, w0, H, W, tie=False)
    lab = vr.place_labels(rng, B, nvox, C, 255, invalid=True)
    dist = make_dist(mean, fac, C, R, H, W)
    ss, ts = va.val_sums_ssn2d(dist, dev(lab), S, dev(ew), dev(ed), 0, 0, 255, raise_invalid=False)
    assert ts[0, C + 1] == 0 and ts[1, C + 1] == 1 and ts[:, C].sum() == (lab < C).sum()
    with pytest.raises(ValueError):
        va.val_sums_ssn2d(dist, dev(lab), S, dev(ew), dev(ed), 0, 0, 255)
    wide = torch.from_numpy(lab.astype(np.int64)).cuda()
    wide[0, 1] = 256 + 1                  # no uint8 holds it: invalid, not wrapped into class 1
    assert va.val_sums_ssn2d(dist, wide, S, dev(ew), dev(ed), 0, 0, 255, raise_invalid=False)[1][0, C + 1] == 1


# ---- 5. validation_step and validate ------------------------------------------------------------------------------------------------------
class _Fixed:
    """a model whose SSN head is the fixture's"""
    ssn = True

    def __init__(self, g):
        self.g = g

    def __call__(self, x, mean_only=False, **kw):
        g = self.g
        C = g["mean_lo"].shape[1]
        R = 0 if mean_only else g["factor_lo"].shape[1] // C
        return make_dist(g["mean_lo"].transpose(0, 2, 3, 1), g["factor_lo"].transpose(0, 2, 3, 1), C, R, *(int(v) for v in g["size"]),
                         epsilon=float(g["epsilon"]))


@pytest.mark.parametrize("ig", [0, 255])
@pytest.mark.parametrize("mean_only", [False, True])
def test_validation_step_reproduces_the_golden_numbers(ig, mean_only):
    """the bounds of tests/test_valstep2d_ref_cpu.py"""
    from tests.test_valstep2d_ref_cpu import K_ULP, f32_mean_bound, fixture_case, sum_bound
    g = load_npz("valstep2d_kat.npz")
    _, _, ew, ed, y, dmag, (B, S, C, R, H, W) = fixture_case(g, mean_only)
    name = "ssn_mean_only" if mean_only else "ssn"
    lab = g[f"seg_{ig}"].reshape(B, H * W)
    ce_ig = vr.ce_ignore_label(ig)
    res = va.validation_step(_Fixed(g), torch.zeros((B, 3, H, W), device="cuda"), dev(g[f"seg_{ig}"]), n_aleatoric_samples=S, ignore_index=ig,
                             mean_only=mean_only, eps=(dev(ew), dev(ed)))
    _, smag, sallow, _ = v2.np_val_ssn2d_sums(y, dmag, lab, ce_ig)
    _, take, _ = vr._label_masks(lab, C, ce_ig)
    route = max(float((2 * K_ULP * vr.ulp32(np.abs(y[b, s]).max(0)))[take[b]].sum()) for b in range(B) for s in range(S))
    tol = route + sum_bound(H * W + C, smag[:, :, 0].max()) + vr.float_bound(H * W, smag[:, :, 0], sallow[:, :, 0]).max()
    dl = abs(res["validation/val_loss"] - float(g[f"{name}_loss_{ig}"]))
    dd = abs(res["validation/val_dice"] - float(g[f"{name}_dice_{ig}"]))
    print(f"valstep2d golden {name} ig={ig}: loss {res['validation/val_loss']:.9g} d {dl:.2e} (tol {tol:.2e}), dice d {dd:.2e}")
    assert dl <= tol and dd <= f32_mean_bound(S)(res["validation/val_dice"]), (name, res)


def _ssn_hrnet():
    import json
    from tests.formula import formula_state_dict_from_shapes
    from tests.test_gpu_hrnet import small_cfg
    from values_amd.hrnet import HighResolutionNet
    shapes = json.loads(bytes(load_npz("hrnet_ssn.npz")["shapes_json"]).decode())
    cfg = small_cfg(False)
    cfg["MODEL"].update({"SSN": True, "SSN_RANK": 10, "SSN_EPS": 1e-5})
    m = HighResolutionNet(cfg)
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in formula_state_dict_from_shapes(shapes).items()}, strict=False)
    return m.cuda()


def _capture(model):
    seen = []
    orig = model.forward

    def fwd(*a, **kw):
        out = orig(*a, **kw)
        seen.append(out)
        return out

    model.forward = fwd
    return seen


def test_drivers_on_the_ssn_hrnet_equal_the_materialised_route():
    from tests.formula import formula_tensor
    m = _ssn_hrnet()
    seen = _capture(m)
    C, S, seed, H, W = 4, 10, 4321, 64, 96
    nvox = H * W
    xs = [torch.from_numpy(formula_tensor((b, 3, H, W), tag=83 + b, scale=1.5)).float().cuda() for b in (2, 1)]
    rng = np.random.default_rng(5000)
    labs = [vr.place_labels(rng, int(x.shape[0]), nvox, C, 255) for x in xs]
    for ig in (0, 255):
        lab = labs[0] if ig else np.where(labs[0] == 255, 1, labs[0]).astype(np.uint8)   # ignore_index 0: CE ignores nothing
        ce_ig = vr.ce_ignore_label(ig)
        for mean_only in (False, True):
            res = va.validation_step(m, xs[0], dev(lab.reshape(2, 1, H, W)), n_aleatoric_samples=S, ignore_index=ig, seed=seed,
                                     mean_only=mean_only)
            dist = seen[-1]
            assert dist.rank == (0 if mean_only else 10)
            smp = dist.sample_images(S, seed=seed).cpu().numpy().reshape(2, S, C, nvox)
            ss, smag, sallow, ts = vr.np_val_ssn_sums(smp, lab, ce_ig)
            loss, dice = vr.ssn_loss_dice_from_sums(ss, ts, C, ig)
            tol = vr.float_bound(nvox, smag[:, :, 0], sallow[:, :, 0]).max()
            print(f"valstep2d driver mean_only={mean_only} ig={ig}: {res} d {abs(res['validation/val_loss'] - loss):.2e} tol {tol:.2e}")
            assert abs(res["validation/val_loss"] - loss) <= tol and res["validation/val_dice"] == dice
    # validate: Lightning's on_epoch means over two unequal batches, weighted by batch size
    batches = [(x, dev(l.reshape(-1, 1, H, W))) for x, l in zip(xs, labs)]
    out = va.validate(m, batches, n_aleatoric_samples=3, ignore_index=255, seed=seed)
    per = [va.validation_step(m, x, s, n_aleatoric_samples=3, ignore_index=255, seed=seed) for x, s in batches]
    assert out["batches"] == per and len(per) == 2 and per[0] != per[1]
    for k in ("validation/val_loss", "validation/val_dice"):
        assert out[k] == (2 * per[0][k] + 1 * per[1][k]) / 3
