"""GPU: the drivers that draw the TTA noise views on the device from a seed (noise_seed): predict_logits / predict_uncertainty,
predict_image_sliding, GraphedPredictor, ensemble_uncertainty_sharded and tta_views_2d_device.  The smallest UNet3D of the
driver tests (16^3 patches, no dropout), so that every difference between two runs is a difference of the noise views."""
import os

import numpy as np
import pytest
import torch

from tests.formula import formula_tensor, formula_volume
from tests.test_dist_cpu import _run_world2

pytestmark = pytest.mark.gpu

SEED = 4711


def _volumes(V, tag=60, size=16):
    return torch.from_numpy(np.concatenate([formula_volume((1, 1, size, size, size), tag=tag + i) for i in range(V)], 0)).float().cuda()


@pytest.fixture(scope="module")
def model():
    from tests.test_gpu_unet3d import make_model
    return make_model(do_dropout=False)


@pytest.mark.parametrize("V,n_streams", [(3, 1), (3, 2), (8, 2)])
def test_predict_logits_noise_seed_is_the_view_of_noise_view_device(model, V, n_streams):
    """(8 volumes on two streams: the smallest TTA batch predict_logits splits into chunks -- each chunk draws its own
    volumes' streams)"""
    from values_amd import noise_view_device, predict_logits
    from values_amd.predict import _volume_chunks
    x = _volumes(V)
    view, sigma = noise_view_device(x, SEED, return_sigma=True)
    assert len(_volume_chunks(V, n_streams, False, 16)[0]) == (2 if V == 8 else 1)
    assert (sigma > 0).all() and (sigma < 0.1 ** 0.5).all() and len(torch.unique(sigma)) == V
    a = predict_logits([model], x, tta=True, noise_seed=SEED, n_streams=n_streams)
    b = predict_logits([model], x, tta=True, x_noise=view, n_streams=n_streams)
    assert tuple(a.shape) == (V, 16, 2, 16, 16, 16)
    assert torch.equal(a, b)
    assert not torch.equal(a[:, :8], a[:, 8:])
    # index0 shifts the streams; the other sigma law gives another view
    c = predict_logits([model], x[1:], tta=True, noise_seed=SEED, noise_index0=1, n_streams=1)
    assert torch.equal(c, a[1:])
    d = predict_logits([model], x, tta=True, noise_seed=SEED, sigma_law="var", n_streams=1)
    assert torch.equal(d[:, :8], a[:, :8]) and not torch.equal(d[:, 8:], a[:, 8:])
    assert torch.equal(d, predict_logits([model], x, tta=True, x_noise=noise_view_device(x, SEED, sigma_law="var"), n_streams=1))


def test_noise_view_device_arguments(model):
    from values_amd import noise_view_device
    x = _volumes(3)
    out = torch.empty_like(x)
    assert noise_view_device(x, SEED, out=out) is out
    assert torch.equal(out, noise_view_device(x, SEED))
    word = torch.tensor([5], dtype=torch.int32, device="cuda")
    assert torch.equal(noise_view_device(x, SEED, seed_dev=word), noise_view_device(x, SEED + 5))
    v, s = noise_view_device(x, SEED, variance=(0.04, 0.04), return_sigma=True)
    assert torch.allclose(s, torch.full((3,), 0.2, device="cuda"), atol=1e-6)
    with pytest.raises(ValueError):
        noise_view_device(x, SEED, sigma_law="std")
    with pytest.raises(ValueError):
        noise_view_device(x, SEED, out=torch.empty((2, 1, 16, 16, 16), device="cuda"))
    from values_amd._lib import VxError
    with pytest.raises(VxError):
        noise_view_device(x, SEED, variance=(0.2, 0.1))


def test_predict_uncertainty_repeats_with_the_seed_and_changes_with_it(model):
    from values_amd import predict_uncertainty
    x = _volumes(3)
    a = predict_uncertainty([model], x, tta=True, noise_seed=SEED)
    b = predict_uncertainty([model], x, tta=True, noise_seed=SEED)
    c = predict_uncertainty([model], x, tta=True, noise_seed=SEED + 1)
    for k in ("logits", "pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty", "mean_softmax", "pred_seg_mean"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["logits"], c["logits"]) and not torch.equal(a["pred_entropy"], c["pred_entropy"])
    assert torch.equal(a["logits"][:, :8], c["logits"][:, :8])
    # batch size does not matter: volume 2 alone, told its global index
    d = predict_uncertainty([model], x[2:], tta=True, noise_seed=SEED, noise_index0=2)
    assert torch.equal(d["logits"][0], a["logits"][2])


def test_sliding_window_noise_does_not_depend_on_the_patch_batch(model):
    from values_amd import noise_view_device, predict_image_sliding
    img = torch.from_numpy(formula_volume((1, 1, 24, 24, 24), tag=81)[0, 0]).float().cuda()
    kw = dict(patch_size=16, patch_overlap=0.5, tta=True, noise_seed=SEED)
    a = predict_image_sliding([model], img, patch_batch=8, **kw)
    b = predict_image_sliding([model], img, patch_batch=3, **kw)
    assert float(a["num_predictions"].max()) == 8.0          # 2 x 2 x 2 overlapping patches
    # (overlapping patches accumulate through float atomics, whose order is not fixed: the comparison is on a non-overlapping
    # crop list below; here the sums agree to rounding)
    assert (a["softmax_sum"] - b["softmax_sum"]).abs().max().item() < 1e-5
    # the default patch_overlap = 1 (one patch on this image, no atomics): bit for bit
    one, two = (predict_image_sliding([model], img, patch_size=16, tta=True, noise_seed=SEED, patch_batch=pb) for pb in (8, 1))
    for k in one:
        assert torch.equal(one[k], two[k]), k
    img32 = torch.from_numpy(formula_volume((1, 1, 32, 32, 32), tag=82)[0, 0]).float().cuda()
    kw = dict(patch_size=16, patch_overlap=1, tta=True, noise_seed=SEED)
    c = predict_image_sliding([model], img32, patch_batch=8, **kw)
    d = predict_image_sliding([model], img32, patch_batch=3, **kw)
    for k in ("softmax_sum", "pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty", "mean_softmax", "pred_seg_mean"):
        assert torch.equal(c[k], d[k]), k
    e = predict_image_sliding([model], img32, patch_batch=8, **dict(kw, noise_seed=SEED + 1))
    assert not torch.equal(c["softmax_sum"], e["softmax_sum"])
    # noise_fn keeps working, and with the device draw of the same slots it is the same run
    starts = iter(range(0, 8, 3))
    f = predict_image_sliding([model], img32, patch_size=16, patch_overlap=1, tta=True, patch_batch=3,
                              noise_fn=lambda x: noise_view_device(x, SEED, index0=next(starts)))
    assert torch.equal(f["softmax_sum"], d["softmax_sum"])
    with pytest.raises(ValueError):
        predict_image_sliding([model], img32, noise_fn=lambda x: x, **kw)


def test_sliding_window_on_a_24_cubed_image_is_bit_equal_for_two_block_sizes(model):
    """24^3, patch 16, overlap 0.5: eight overlapping patches.  The softmax sums of overlapping patches go through float
    atomics, so the bit-for-bit comparison is made where the order of additions is fixed: on the logits the two block sizes
    hand to the accumulation, patch by patch."""
    from values_amd import predict_logits
    from values_amd.predict import crop_indices
    img = torch.from_numpy(formula_volume((1, 1, 24, 24, 24), tag=81)[0, 0]).float().cuda()
    crops = crop_indices((24, 24, 24), 16, 0.5)
    assert len(crops) == 8

    def run(block):
        parts = []
        for b0 in range(0, len(crops), block):
            x = torch.stack([img[c[0][0]:c[0][1], c[1][0]:c[1][1], c[2][0]:c[2][1]] for c in crops[b0:b0 + block]]).unsqueeze(1)
            parts.append(predict_logits([model], x, tta=True, noise_seed=SEED, noise_index0=b0))
        return torch.cat(parts)
    assert torch.equal(run(8), run(3))


def test_graphed_predictor_captures_the_noise_draw(model):
    from values_amd import GraphedPredictor, predict_uncertainty
    x = _volumes(2, tag=90)
    gp = GraphedPredictor([model], tuple(x.shape), tta=True, noise_seed=SEED)
    a = {k: v.clone() for k, v in gp(x, seed=7).items()}
    b = {k: v.clone() for k, v in gp(x, seed=7).items()}
    c = {k: v.clone() for k, v in gp(x, seed=8).items()}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["logits"][:, :8], c["logits"][:, :8]), "the clean views moved with the seed word"
    assert not torch.equal(a["logits"][:, 8:], c["logits"][:, 8:])
    for v in range(2):
        for k in range(8, 16):
            assert not torch.equal(a["logits"][v, k], c["logits"][v, k]), (v, k)
    # the replay's word is ADDED to the seed: the eager call with seed + 7
    e = predict_uncertainty([model], x, tta=True, noise_seed=SEED + 7)
    assert torch.equal(a["logits"], e["logits"])


def test_tta_views_2d_device_generates_the_noisy_views(model):
    from tests import noise_ref as nr
    from values_amd.data import TTA_8_VIEW_CODES, tta_views_2d_device
    img = torch.from_numpy(nr.images_2d())
    views, names, sigma = tta_views_2d_device(img, nr.MEAN, nr.STD, noise_seed=SEED, return_sigma=True)
    assert tuple(views.shape) == (4, nr.B2, nr.H2, nr.W2, 4) and tuple(sigma.shape) == (nr.B2, 2)
    assert names == [[], ["HorizontalFlip"], ["GaussNoise"], ["HorizontalFlip", "GaussNoise"]]
    assert (sigma >= 10 ** 0.5).all() and (sigma < 50 ** 0.5).all()
    unflipped = [views[0], views[1].flip(2), views[2], views[3].flip(2)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert torch.equal(unflipped[i], unflipped[j]) == ((i, j) == (0, 1)), (i, j)
            assert not torch.equal(views[i], views[j])
    again, _ = tta_views_2d_device(img, nr.MEAN, nr.STD, noise_seed=SEED)
    assert torch.equal(again, views)
    # without a seed: today's output (the noisy views degenerate to the clean ones), and no sigma
    plain, names0, none = tta_views_2d_device(img, nr.MEAN, nr.STD, return_sigma=True)
    assert none is None and names0 == [[], ["HorizontalFlip"], [], ["HorizontalFlip"]]
    assert torch.equal(plain[0], views[0]) and torch.equal(plain[1], views[1])
    assert torch.equal(plain[2], plain[0]) and torch.equal(plain[3], plain[1])
    # a supplied field wins for its slot
    n0 = torch.from_numpy(formula_tensor(tuple(img.shape), 3240, 9.0).astype(np.float32))
    mixed, _ = tta_views_2d_device(img, nr.MEAN, nr.STD, noise=n0, noise_seed=SEED)
    given, _ = tta_views_2d_device(img, nr.MEAN, nr.STD, noise=n0, noise_flipped=torch.zeros_like(n0))
    assert torch.equal(mixed[2], given[2]) and torch.equal(mixed[3], views[3]) and not torch.equal(mixed[2], views[2])
    # the eight views: one generated draw, flipped four ways; image_index0 names the images
    eight, _ = tta_views_2d_device(img, nr.MEAN, nr.STD, noise_seed=SEED, view_codes=TTA_8_VIEW_CODES)
    assert torch.equal(eight[4], views[2])
    assert torch.equal(eight[5], eight[4].flip(2)) and torch.equal(eight[6], eight[4].flip(1)) and torch.equal(eight[7], eight[4].flip(1, 2))
    second, _ = tta_views_2d_device(img[1], nr.MEAN, nr.STD, noise_seed=SEED, image_index0=1)
    assert torch.equal(second[:, 0], views[:, 1])


def _worker_sharded_noise(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from tests.test_gpu_unet3d import KEYS, make_model
        from values_amd import predict_uncertainty
        from values_amd.dist import ensemble_uncertainty_sharded
        models = [make_model(seed_tag=s, do_dropout=False) for s in range(3)]      # 3 members on 2 ranks: volume blocks [0, 2), [2, 3)
        x = _volumes(3, tag=70)
        sh = ensemble_uncertainty_sharded(models, x, world=world, rank=rank, tta=True, noise_seed=SEED)
        ok = True
        if rank == 0:
            one = ensemble_uncertainty_sharded(models, x, world=1, rank=0, tta=True, noise_seed=SEED)
            other = ensemble_uncertainty_sharded(models, x, world=1, rank=0, tta=True, noise_seed=SEED + 1)
            full = predict_uncertainty(models, x, tta=True, noise_seed=SEED)
            for ref in (one, full):
                ok = ok and all((sh[k] - ref[k]).abs().max().item() < 2e-6 for k in KEYS + ("mean_softmax",))
                ok = ok and torch.equal(sh["pred_seg_mean"], ref["pred_seg_mean"])
            ok = ok and (one["pred_entropy"] - other["pred_entropy"]).abs().max().item() > 1e-4     # the seed matters
        else:
            ok = sh is None
        torch.cuda.synchronize()
        q.put(bool(ok))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sharded_ensemble_with_a_noise_seed_equals_the_one_rank_result():
    assert all(_run_world2(_worker_sharded_noise))
