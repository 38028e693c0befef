"""GPU: values_amd.HighResolutionNet (HIP) vs the golden fixture produced by the imported reference class (float32,
training-mode BatchNorm, DROPOUT_FINAL masks injected) and vs the float64 oracle.

Tolerance (BASELINE.json north_star): uncertainty maps within 1e-4 abs of the reference; logits within 1e-4 too, or --
where the reference's own float32 evaluation sits further than that from a float64 evaluation of the same network
(the deep W18 fixture: 1.3e-4, recorded in the fixture) -- within twice that gap."""
import json

import numpy as np
import pytest
import torch

from tests.helpers import load_npz
from tests.formula import HRNET_SMALL_EXTRA, formula_state_dict_from_shapes, formula_tensor

pytestmark = pytest.mark.gpu
KEYS = ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")
MAP_TOL = 1e-4
LOGIT_TOL = 1e-4


def small_cfg(dropout_final=True, ncls=4):
    extra = dict(HRNET_SMALL_EXTRA, DROPOUT_FINAL=dropout_final)
    return {"MODEL": {"EXTRA": extra, "ALIGN_CORNERS": False, "INPUT_CHANNELS": 3, "PRETRAINED": False},
            "DATASET": {"NUM_CLASSES": ncls}}


def fixture():
    g = load_npz("hrnet_small.npz")
    shapes = json.loads(bytes(g["shapes_json"]).decode())
    sd = {k: torch.from_numpy(v).float() for k, v in formula_state_dict_from_shapes(shapes).items()}
    return g, shapes, sd


def masks_of(g, t):
    out = []
    for i in range(4):
        shape = tuple(int(v) for v in g[f"maskshape_{i}"])
        out.append(torch.from_numpy(np.unpackbits(g[f"mask_{t}_{i}"])[:int(np.prod(shape))].astype(bool).reshape(shape)))
    return out


def make(dropout_final=True):
    from values_amd.hrnet import HighResolutionNet
    g, shapes, sd = fixture()
    m = HighResolutionNet(small_cfg(dropout_final))
    ours = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert ours == {k: tuple(v) for k, v in shapes.items()}          # identical state-dict names and shapes
    missing = m.load_state_dict(sd, strict=False)                    # buffers (running stats) keep their defaults
    assert not missing.unexpected_keys
    assert all(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in missing.missing_keys)
    return m.cuda(), g, sd


def test_hrnet_golden_no_dropout():
    from oracle.hrnet_oracle import hrnet_forward
    m, g, sd = make(dropout_final=False)
    x = torch.from_numpy(g["input"]).cuda()
    y = m(x)
    assert y.shape == (2, 4, 64, 96)
    err_ref = np.abs(y.cpu().numpy() - g["logits_nodrop"]).max()
    with torch.no_grad():
        y64 = hrnet_forward(dict(HRNET_SMALL_EXTRA, DROPOUT_FINAL=False), {k: v.double() for k, v in sd.items()},
                            torch.from_numpy(g["input"]).double()).numpy()
    err_o = np.abs(y.cpu().numpy() - y64).max()
    ref_o = np.abs(g["logits_nodrop"] - y64).max()
    print(f"max|d| hip-vs-reference(f32) {err_ref:.2e}, hip-vs-oracle(f64) {err_o:.2e}, reference(f32)-vs-oracle(f64) {ref_o:.2e}")
    assert err_o < max(2 * ref_o, LOGIT_TOL)
    assert err_ref < LOGIT_TOL


def test_hrnet_golden_mc_dropout_final_and_maps():
    from values_amd import uncertainty_maps
    m, g, sd = make(dropout_final=True)
    x = torch.from_numpy(g["input"]).cuda()
    T = g["logits"].shape[0]
    lg = m.forward_samples(x, T, dropout_masks=[masks_of(g, t) for t in range(T)])
    assert lg.shape == (T, 2, 4, 64, 96)
    err = np.abs(lg.cpu().numpy() - g["logits"]).max()
    assert err < LOGIT_TOL, err
    # process_output (test_2D.py:205-248): per image, (T, C+1, H, W) softmax with a zero channel -> calculate_uncertainty
    sm = torch.softmax(lg, dim=2)
    sm1 = torch.cat([sm, torch.zeros(T, 2, 1, 64, 96, device="cuda")], dim=2)
    for b in range(2):
        u = uncertainty_maps(sm1[:, b].unsqueeze(0).contiguous())
        for k, kk in zip(KEYS, ("pred_entropy", "expected_entropy", "mutual_information")):
            d = np.abs(u[kk][0].cpu().numpy() - g[f"{k}_{b}"]).max()
            assert d < MAP_TOL, (k, d)
    # the same maps from the REFERENCE's logits: isolates the reduction (must hold the 1e-4 of the north star)
    smr = torch.softmax(torch.from_numpy(g["logits"]).cuda(), dim=2)
    smr1 = torch.cat([smr, torch.zeros(T, 2, 1, 64, 96, device="cuda")], dim=2)
    for b in range(2):
        u = uncertainty_maps(smr1[:, b].unsqueeze(0).contiguous())
        for k, kk in zip(KEYS, ("pred_entropy", "expected_entropy", "mutual_information")):
            assert np.abs(u[kk][0].cpu().numpy() - g[f"{k}_{b}"]).max() < 1e-5


def test_hrnet_hash_dropout_and_properties():
    m, g, sd = make(dropout_final=True)
    x = torch.from_numpy(g["input"]).cuda()
    a = m.forward_samples(x, 3, seeds=[1, 2, 3])
    b = m.forward_samples(x, 3, seeds=[1, 2, 3])
    assert torch.equal(a, b)                       # deterministic, no atomics
    assert not torch.equal(a[0], a[1])             # samples differ
    # batch statistics: an image's logits DO depend on its batch mates (training-mode BN)
    single = m.forward_samples(x[:1], 1, seeds=[1])
    assert (single[0, 0] - a[0, 0]).abs().max().item() > 1e-3
    # un-flip of a HorizontalFlip view
    xf = torch.flip(x, [-1])
    yf = m.forward_samples(xf, 1, seeds=[5], hflip_back=True)
    yn = m.forward_samples(xf, 1, seeds=[5])
    assert torch.equal(yf, torch.flip(yn, [-1]))
    with pytest.raises(NotImplementedError):   # unsupported variants raise instead of falling back
        from values_amd.hrnet import HighResolutionNet
        cfg = small_cfg()
        cfg["MODEL"]["ALIGN_CORNERS"] = True
        HighResolutionNet(cfg)


def test_predict_2d_driver_mc_and_tta_vs_oracle():
    """Tester.predict_cases ordering (test_2D.py:283-317) + process_output maps, against the float64 oracle."""
    from oracle import uncertainty_oracle as uo
    from oracle.hrnet_oracle import hrnet_forward
    from values_amd.predict2d import predict_logits_2d, process_output_2d
    m, g, sd = make(dropout_final=True)
    sd64 = {k: v.double() for k, v in sd.items()}
    x = torch.from_numpy(g["input"])
    T = 3
    masks = [masks_of(g, t) for t in range(T)]
    lg = predict_logits_2d([m], x.cuda(), n_pred=T, dropout_masks=[masks])
    assert lg.shape == (2, T, 4, 64, 96)
    np.testing.assert_allclose(lg.permute(1, 0, 2, 3, 4).cpu().numpy(), g["logits"], atol=LOGIT_TOL)
    out = process_output_2d(lg)
    for b in range(2):
        for k in KEYS:
            assert np.abs(out[k][b].cpu().numpy() - g[f"{k}_{b}"]).max() < MAP_TOL
    sm_ref = torch.softmax(torch.from_numpy(g["logits"]), 2).permute(1, 0, 2, 3, 4).numpy()
    assert np.abs(out["softmax_pred"].cpu().numpy() - sm_ref).max() < MAP_TOL
    # TTA: 4 views (identity, hflip, noisy, hflip+noisy): flip views are un-flipped; dropout off in this model
    m2, _, _ = make(dropout_final=False)
    noise = torch.from_numpy(formula_tensor((2, 3, 64, 96), tag=82, scale=0.1)).float()
    views = [x, torch.flip(x, [-1]), x + noise, torch.flip(x + noise, [-1])]
    flags = [False, True, False, True]
    lg = predict_logits_2d([m2], [v.cuda() for v in views], tta=True, hflip_views=flags)
    extra = dict(HRNET_SMALL_EXTRA, DROPOUT_FINAL=False)
    with torch.no_grad():
        for vi, (v, fl) in enumerate(zip(views, flags)):
            y = hrnet_forward(extra, sd64, v.double())
            if fl:
                y = torch.flip(y, [-1])
            assert np.abs(lg[:, vi].cpu().numpy() - y.numpy()).max() < LOGIT_TOL, vi
    out = process_output_2d(lg)
    ref = uo.calculate_uncertainty(uo.softmax(lg[0].double().cpu().numpy(), axis=1))
    for k in KEYS:
        assert np.abs(out[k][0].cpu().numpy() - ref[k]).max() < 1e-5
    # single prediction -> 1 - max softmax
    one = process_output_2d(lg[:, :1].contiguous())
    p = torch.softmax(lg[:, 0].double(), 1)
    assert (one["pred_entropy"].double() - (1 - p.max(1)[0])).abs().max().item() < 1e-6
    assert "epistemic_uncertainty" not in one


def test_hrnet_ssn_head_matches_reference_fixture():
    """HighResolutionNet with the SSN head (hrnet_config_ssn.yaml keys; hrnet_module.py:430-453, 559-595): state-dict
    names, mean, samples with the reference's captured normals (test_2D.py:285-299), and the generated diagonal noise"""
    from tests.formula import formula_tensor
    from values_amd.hrnet import HighResolutionNet
    g = load_npz("hrnet_ssn.npz")
    shapes = json.loads(bytes(g["shapes_json"]).decode())
    sd = {k: torch.from_numpy(v).float() for k, v in formula_state_dict_from_shapes(shapes).items()}
    cfg = small_cfg(False)
    cfg["MODEL"].update({"SSN": True, "SSN_RANK": 10, "SSN_EPS": 1e-5})
    m = HighResolutionNet(cfg)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
    m.load_state_dict(sd, strict=False)
    m = m.cuda()
    x = torch.from_numpy(g["input"]).cuda()
    dist = m(x)
    assert np.abs(dist.mean.cpu().numpy() - g["loc"]).max() < 1e-4
    S, B = g["samples"].shape[:2]
    eps_d = torch.from_numpy(formula_tensor(g["samples"].shape, tag=int(g["eps_d_tag"]), scale=1.7).astype(np.float32))
    smp = dist.sample([S], eps_w=torch.from_numpy(g["eps_w"]), eps_d=eps_d)
    assert tuple(smp.shape) == g["samples"].shape
    err = np.abs(smp.cpu().numpy() - g["samples"])
    assert err.max() < 5e-4, err.max()          # samples reach |9|; float32 backbone + exp() of the head
    assert np.abs(err).mean() < 2e-5
    # generated normals: unit variance of the diagonal part (rank-0 distribution)
    d0 = m(x, mean_only=True)
    z = d0.sample_images(16, seed=3)                                   # (B, 16, C, H, W)
    mean = d0.mean.reshape(B, 1, 4, 64, 96)
    zz = ((z - mean) / torch.from_numpy(g["cov_diag"]).cuda().reshape(B, 1, 4, 64, 96).sqrt()).reshape(-1)
    assert abs(zz.mean().item()) < 0.01 and abs(zz.var().item() - 1.0) < 0.01


def test_hrnet_w18_widths_match_reference_fixture():
    """HRNet-W18 widths (18/36/72/144, 270 concatenated, 5 classes): the zero-padded round16(C) layout of the HIP
    path gives the reference's logits, with DROPOUT_FINAL masks and without"""
    from tests.formula import HRNET_W18S_EXTRA
    from values_amd.hrnet import HighResolutionNet
    g = load_npz("hrnet_w18s.npz")
    shapes = json.loads(bytes(g["shapes_json"]).decode())
    sd = {k: torch.from_numpy(v).float() for k, v in formula_state_dict_from_shapes(shapes).items()}
    x = torch.from_numpy(g["input"]).cuda()
    for dropout_final in (True, False):
        cfg = {"MODEL": {"EXTRA": dict(HRNET_W18S_EXTRA, DROPOUT_FINAL=dropout_final), "ALIGN_CORNERS": False, "INPUT_CHANNELS": 3},
               "DATASET": {"NUM_CLASSES": 5}}
        m = HighResolutionNet(cfg)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
        m.load_state_dict(sd, strict=False)
        m = m.cuda()
        if dropout_final:
            masks = []
            for t in range(2):
                per = []
                for i in range(4):
                    shape = tuple(int(v) for v in g[f"maskshape_{i}"])
                    per.append(torch.from_numpy(np.unpackbits(g[f"mask_{t}_{i}"])[:int(np.prod(shape))].astype(bool).reshape(shape)))
                masks.append(per)
            y = m.forward_samples(x, 2, dropout_masks=masks).cpu().numpy()
            assert np.abs(y - g["logits"]).max() < 5e-5, np.abs(y - g["logits"]).max()
        else:
            y = m(x).cpu().numpy()
            assert np.abs(y - g["logits_nodrop"]).max() < 5e-5
            # the persistent zero-padded buffers: their tails are still zero after forwards, and a second geometry REPLACES
            # a layer's buffer instead of adding one (the cache grew without bound)
            assert m.zero_tails_intact()
            n_buf = len(m._zcache)
            y2 = m(torch.cat([x, x], 0)[:, :, :x.shape[2] // 2 * 2 - 32]).cpu().numpy()      # another batch size and height
            assert np.isfinite(y2).all() and len(m._zcache) == n_buf and m.zero_tails_intact()
            y3 = m(x).cpu().numpy()
            assert np.array_equal(y3, y)


def _w18_full(ncls=19):
    from values_amd.hrnet_configs import hrnet_w18_extra
    from values_amd.hrnet import HighResolutionNet
    g = load_npz("hrnet_w18_256x478.npz")
    shapes = json.loads(bytes(g["shapes_json"]).decode())
    cfg = {"MODEL": {"EXTRA": hrnet_w18_extra(False), "ALIGN_CORNERS": False, "INPUT_CHANNELS": 3},
           "DATASET": {"NUM_CLASSES": ncls}}
    m = HighResolutionNet(cfg)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
    sd = {k: torch.from_numpy(v).float() for k, v in formula_state_dict_from_shapes(shapes).items()}
    m.load_state_dict(sd, strict=False)
    return m.cuda(), g


def _check_view(y, g, tag, tol):
    """y (C, H, W) against a fixture view: the stride-(4, 6) sub-grid and the row / column sums over the whole map"""
    assert np.abs(y[:, ::4, ::6] - g[f"{tag}_sub"]).max() < tol, (tag, np.abs(y[:, ::4, ::6] - g[f"{tag}_sub"]).max())
    assert np.abs(y.astype(np.float64).sum(2) - g[f"{tag}_rowsum"]).max() < tol * y.shape[2] ** 0.5 * 4, tag
    assert np.abs(y.astype(np.float64).sum(1) - g[f"{tag}_colsum"]).max() < tol * y.shape[1] ** 0.5 * 4, tag


def test_config_C4_w18_full_layout_at_256x478_matches_reference_fixture():
    """BASELINE config 4's network as worded -- the full HRNet-W18 layout, 19 classes -- at the size of the reference's test
    images (256 x 478), one image per batch (training-mode BatchNorm over that image, as a TTA forward
    runs): logits against the imported reference class (float32) and its float64 run, the HorizontalFlip view
    un-flipped as test_2D.py:304-309 does and the VerticalFlip view of the 8-view extension.  The reference's own
    float32-vs-float64 gap on this 300-layer net is 1.3e-4 (in the fixture): logits are held to twice that."""
    from values_amd.predict2d import predict_logits_2d, process_output_2d, tta_views_8
    m, g = _w18_full()
    x = torch.from_numpy(formula_tensor((1, 3, 256, 478), tag=int(g["input_tag"]), scale=float(g["input_scale"]))).float().cuda()
    gap = float(g["ref_f32_f64_gap"])
    tol = max(LOGIT_TOL, 2 * gap)
    y = m(x)[0].cpu().numpy()
    assert y.shape == (19, 256, 478)
    _check_view(y, g, "logits", tol)
    _check_view(y, g, "logits64", tol)
    e32 = np.abs(y[:, ::4, ::6] - g["logits_sub"]).max()
    e64 = np.abs(y[:, ::4, ::6] - g["logits64_sub"]).max()
    print(f"W18 256x478: max|d| vs reference f32 {e32:.2e}, vs reference f64 {e64:.2e}; reference f32-vs-f64 {gap:.2e}")
    assert e64 < 2 * gap                      # no further from float64 than the reference itself (x2)
    views, hf, vf = tta_views_8(x, x)         # noise-free: the noisy half repeats the clean one
    lg = predict_logits_2d([m], views, tta=True, hflip_views=hf, vflip_views=vf)
    assert lg.shape == (1, 8, 19, 256, 478)
    l8 = lg[0].cpu().numpy()
    _check_view(l8[0], g, "logits", tol)
    _check_view(l8[1], g, "logits_hflip", tol)
    _check_view(l8[2], g, "logits_vflip", tol)
    assert np.array_equal(l8[:4], l8[4:])
    # maps of the 4 distinct views against the reduction of the REFERENCE's logits where the fixture has them (sub-grid)
    from oracle import uncertainty_oracle as uo
    out = process_output_2d(lg[:, :3].contiguous())
    ref_l = np.stack([g["logits_sub"], g["logits_hflip_sub"], g["logits_vflip_sub"]]).astype(np.float64)
    ref = uo.calculate_uncertainty(uo.softmax(ref_l, axis=1))
    for k in KEYS:
        d = np.abs(out[k][0].cpu().numpy()[::4, ::6] - ref[k]).max()
        assert d < MAP_TOL, (k, d)


def test_config_C4_w18_8_view_tta_at_1024x512_properties():
    """Config 4 as worded, full size: HRNet-W18, one 1024 x 512 image, 8 TTA views ({id, H, V, HV} x {clean, noisy}).
    No reference run exists at this size, so: every view equals its stand-alone forward un-flipped by
    torch.flip, reruns are bit-identical, the maps obey their bounds and MI = PE - EE."""
    from values_amd.predict2d import predict_logits_2d, process_output_2d, tta_views_8
    m, _ = _w18_full()
    x = torch.from_numpy(formula_tensor((1, 3, 512, 1024), tag=88, scale=1.5)).float().cuda()
    noisy = x + torch.from_numpy(formula_tensor((1, 3, 512, 1024), tag=89, scale=0.1)).float().cuda()
    views, hf, vf = tta_views_8(x, noisy)
    lg = predict_logits_2d([m], views, tta=True, hflip_views=hf, vflip_views=vf)
    lg2 = predict_logits_2d([m], views, tta=True, hflip_views=hf, vflip_views=vf)
    assert lg.shape == (1, 8, 19, 512, 1024) and torch.equal(lg, lg2)
    assert torch.isfinite(lg).all()
    for vi in (0, 1, 2, 3, 6):
        alone = m(views[vi])
        dims = ([-1] if hf[vi] else []) + ([-2] if vf[vi] else [])
        alone = torch.flip(alone, dims) if dims else alone
        assert torch.equal(lg[:, vi], alone), vi
    assert (lg[:, 0] - lg[:, 3]).abs().max().item() > 1e-3      # strided convs are not flip-equivariant: the views differ
    out = process_output_2d(lg)
    pe, ee, mi = out["pred_entropy"], out["aleatoric_uncertainty"], out["epistemic_uncertainty"]
    assert pe.min().item() >= 0 and pe.max().item() <= float(np.log(19)) + 1e-5
    assert ee.min().item() >= 0 and mi.min().item() > -1e-5
    assert (mi - (pe - ee)).abs().max().item() < 1e-6
    assert (out["mean_softmax"].sum(1) - 1).abs().max().item() < 1e-5
    assert torch.equal(out["pred_seg"], out["mean_softmax"].argmax(1).to(torch.uint8)) or \
        (out["pred_seg"] != out["mean_softmax"].argmax(1).to(torch.uint8)).float().mean().item() < 1e-5


def test_batched_tta_views_equal_one_forward_per_view():
    """predict_logits_2d(batch_views=True): the TTA views as ONE batch with BatchNorm statistics per view
    (vx_bn_finalize_groups, vx_affine_args.group_images) give the bits of one forward per view (test_2D.py:299-311) --
    W18 widths (zero-padded channels, persistent padded buffers) and the small W48-style net, 4 and 8 views, batch 2."""
    from tests.formula import HRNET_W18S_EXTRA
    from values_amd.hrnet import HighResolutionNet
    from values_amd.predict2d import predict_logits_2d, tta_views_8
    g = load_npz("hrnet_w18s.npz")
    shapes = json.loads(bytes(g["shapes_json"]).decode())
    sd = {k: torch.from_numpy(v).float() for k, v in formula_state_dict_from_shapes(shapes).items()}
    cfg = {"MODEL": {"EXTRA": dict(HRNET_W18S_EXTRA, DROPOUT_FINAL=False), "ALIGN_CORNERS": False, "INPUT_CHANNELS": 3},
           "DATASET": {"NUM_CLASSES": 5}}
    m = HighResolutionNet(cfg)
    m.load_state_dict(sd, strict=False)
    m = m.cuda()
    x = torch.from_numpy(g["input"]).cuda()
    noisy = x + torch.from_numpy(formula_tensor(tuple(x.shape), tag=83, scale=0.1)).float().cuda()
    views, hf, vf = tta_views_8(x, noisy)
    for nv in (8, 4):
        a = predict_logits_2d([m], views[:nv], tta=True, hflip_views=hf[:nv], vflip_views=vf[:nv], batch_views=True)
        b = predict_logits_2d([m], views[:nv], tta=True, hflip_views=hf[:nv], vflip_views=vf[:nv], batch_views=False)
        assert a.shape == (2, nv, 5, 64, 96) and torch.equal(a, b), nv
        a2 = predict_logits_2d([m], views[:nv], tta=True, hflip_views=hf[:nv], vflip_views=vf[:nv], batch_views=True)
        assert torch.equal(a, a2)          # the persistent padded buffers are clean on reuse
    m2, gg, _ = make(dropout_final=False)
    x2 = torch.from_numpy(gg["input"]).cuda()
    v2, h2, w2 = tta_views_8(x2, x2 * 1.02)
    assert torch.equal(predict_logits_2d([m2], v2, tta=True, hflip_views=h2, vflip_views=w2, batch_views=True),
                       predict_logits_2d([m2], v2, tta=True, hflip_views=h2, vflip_views=w2, batch_views=False))


def test_tta_views_2d_on_device_is_the_dataset_branch_bit_for_bit():
    """Row a17 (cityscapes_dataset.py:76-99): vx_tta_views_2d -- uint8 HWC image (+ the two noise fields, which are inputs:
    albumentations' generator is third-party) -> the four normalised views in ONE launch, flips as index arithmetic,
    channels-last at the stem's pitch.  The KERNEL is compared with oracle/tta2d_oracle.py (the branch restated over
    albumentations 1.3.0's published Normalize / HorizontalFlip / GaussNoise arithmetic; the library is absent, so the row
    stays "parity unpinned") bit for bit: batches of images, both ends of the uint8 clip, a missing field (the view
    degenerates to the clean one), the 8-view set of config C4; the product's host function gives the same bits; and fed
    to the network through NhwcViews the device-built views give the bits of the host-built ones."""
    from oracle import tta2d_oracle
    from values_amd.data import TTA_2D_VIEW_CODES, hflip_flags, tta_views_2d, tta_views_2d_device, tta_views_8_device
    from values_amd.predict2d import NhwcViews, predict_logits_2d, tta_views_8
    rng = np.random.default_rng(5)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    B, H, W = 3, 37, 50
    imgs = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    imgs[0, :4] = 0; imgs[0, 4:8] = 255                       # the clip's two ends are reached
    n0 = (rng.standard_normal((B, H, W, 3)) * 30).astype(np.float32)
    n1 = (rng.standard_normal((B, H, W, 3)) * 30).astype(np.float32)
    dv, names = tta_views_2d_device(torch.from_numpy(imgs), mean, std, noise=n0, noise_flipped=n1)
    assert dv.shape == (4, B, H, W, 4) and dv.dtype == torch.float32
    got = dv.cpu().numpy()
    assert (got[..., 3] == 0).all()
    for b in range(B):
        ref, tr = tta2d_oracle.tta_branch(imgs[b], mean, std, n0[b], n1[b])          # the oracle, not product code
        host, tr_h = tta_views_2d(imgs[b], mean, std, noise=n0[b], noise_flipped=n1[b])
        assert tr == tr_h == names
        assert hflip_flags(tr) == hflip_flags(names) == [False, True, False, True]
        for g in range(4):
            np.testing.assert_array_equal(got[g, b, :, :, :3].transpose(2, 0, 1), ref[g], err_msg=f"view {g} image {b}")
            np.testing.assert_array_equal(host[g], ref[g], err_msg=f"host view {g} image {b}")
    assert (got[2] != got[0]).any() and (got[3] != got[1]).any()
    # a single (H, W, 3) image, no flipped-noise field: view 3 falls back to the clean flip, exactly as in the oracle
    dv1, _ = tta_views_2d_device(imgs[1], mean, std, noise=n0[1])
    ref, _ = tta2d_oracle.tta_branch(imgs[1], mean, std, n0[1], None)
    for g in range(4):
        np.testing.assert_array_equal(dv1[g, 0, :, :, :3].cpu().numpy().transpose(2, 0, 1), ref[g])
    assert TTA_2D_VIEW_CODES == [0, 1, 4, 21]
    # float source: the 8 views of config C4 = torch.flip of the clean / noisy tensors, laid out channels-last
    m2, gg, _ = make(dropout_final=False)
    x = torch.from_numpy(gg["input"]).cuda()
    noisy = x * 1.02 + 0.01
    views, hf, vf = tta_views_8(x, noisy)
    d8, hf2, vf2 = tta_views_8_device(x, noisy)
    o8, ohf, ovf = tta2d_oracle.tta_views_8(x.cpu().numpy(), noisy.cpu().numpy())
    assert hf2 == hf == ohf and vf2 == vf == ovf
    for g in range(8):
        np.testing.assert_array_equal(d8[g][..., :3].permute(0, 3, 1, 2).cpu().numpy(), o8[g], err_msg=f"view {g}")
        assert torch.equal(d8[g][..., :3].permute(0, 3, 1, 2), views[g]), g
    # ... and through the network: one batched forward of the device-built views = the host-built ones, bit for bit
    a = predict_logits_2d([m2], NhwcViews(d8, hf2, vf2), tta=True)
    b = predict_logits_2d([m2], views, tta=True, hflip_views=hf, vflip_views=vf)
    assert torch.equal(a, b)
    with pytest.raises(_lib_mod().VxError):
        tta_views_2d_device(torch.from_numpy(imgs), mean, std, view_codes=[0, 99])


def _lib_mod():
    from values_amd import _lib
    return _lib


def test_multi_term_fusion_pass_gives_the_bits_of_the_term_by_term_chain(monkeypatch):
    """vx_fuse_sum (round 4): all terms of a HighResolutionModule output (hrnet_module.py:316-333) summed in ONE pass, in the
    reference's order, against the chain of vx_affine_gather passes it replaces -- bit for bit, W18 widths (padded channels,
    4 branches, upsampled and strided terms), batched view groups included."""
    from values_amd.predict2d import predict_logits_2d, tta_views_8
    m, _ = _w18_full()
    x = torch.from_numpy(formula_tensor((2, 3, 128, 192), tag=188, scale=1.5)).float().cuda()
    views, hf, vf = tta_views_8(x, x * 1.01 + 0.02)
    a = m(x)
    av = predict_logits_2d([m], views[:4], tta=True, hflip_views=hf[:4], vflip_views=vf[:4])
    monkeypatch.setenv("VX_HRNET_NO_MULTIFUSE", "1")
    b = m(x)
    bv = predict_logits_2d([m], views[:4], tta=True, hflip_views=hf[:4], vflip_views=vf[:4])
    assert torch.equal(a, b) and torch.equal(av, bv)
    assert torch.isfinite(a).all()


def test_graphed_predictor_2d_replays_the_eager_bits():
    """GraphedPredictor2D: predict_logits_2d + process_output_2d captured into one hipGraph (branches on side streams
    inside the capture) -- the replay gives the eager path's bits, for new inputs too; wrong shapes are refused."""
    from tests.formula import HRNET_W18S_EXTRA
    from values_amd.hrnet import HighResolutionNet
    from values_amd.predict2d import GraphedPredictor2D, predict_logits_2d, process_output_2d, tta_views_8
    g = load_npz("hrnet_w18s.npz")
    shapes = json.loads(bytes(g["shapes_json"]).decode())
    sd = {k: torch.from_numpy(v).float() for k, v in formula_state_dict_from_shapes(shapes).items()}
    cfg = {"MODEL": {"EXTRA": dict(HRNET_W18S_EXTRA, DROPOUT_FINAL=False), "ALIGN_CORNERS": False, "INPUT_CHANNELS": 3},
           "DATASET": {"NUM_CLASSES": 5}}
    m = HighResolutionNet(cfg)
    m.load_state_dict(sd, strict=False)
    m = m.cuda()
    x = torch.from_numpy(g["input"]).cuda()
    noisy = x + torch.from_numpy(formula_tensor(tuple(x.shape), tag=83, scale=0.1)).float().cuda()
    views, hf, vf = tta_views_8(x, noisy)
    gp = GraphedPredictor2D([m], views, tta=True, hflip_views=hf, vflip_views=vf)
    gp2 = GraphedPredictor2D([m], views, tta=True, hflip_views=hf, vflip_views=vf, keep_logits=False)
    for scale in (1.0, 0.7, 1.0):
        vs = [v * scale for v in views]
        out = gp(vs)
        lg = predict_logits_2d([m], vs, tta=True, hflip_views=hf, vflip_views=vf)
        ref = process_output_2d(lg)
        torch.cuda.synchronize()
        assert torch.equal(gp.logits, lg), scale
        # keep_logits=False: every view's softmax in its upsampling pass (vx_bilinear_softmax_nchw) -- no full-resolution
        # logits in the graph, the same bits in every output
        out2 = gp2(vs)
        assert gp2.logits is None
        for k in ref:
            assert torch.equal(out2[k], ref[k]), (k, scale)
        for k in ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty", "mean_softmax", "pred_seg"):
            assert torch.equal(out[k], ref[k]), (k, scale)
    with pytest.raises(ValueError):
        gp(views[:4])
    # a DROPOUT_FINAL member without explicit seeds is refused (the seeds are baked into the graph)
    m3, gg, _ = make(dropout_final=True)
    with pytest.raises(ValueError):
        GraphedPredictor2D([m3], torch.from_numpy(gg["input"]).cuda(), n_pred=2)


@pytest.mark.parametrize("ncls,pitch,inst", [(12, 20, 5), (21, 32, 8)])
def test_logits_of_12_and_21_classes_travel_at_the_pitch_of_a_vector_softmax_instance(ncls, pitch, inst):
    """Class counts whose round4(C) pitch holds fewer channel quads than the softmax-upsample instance that covers them: the
    head writes its logits at pitch 20 / 32 (hrnet._softmax_pitch), vx_bilinear_softmax_nchw stays on vec<5> / vec<8>, the
    probabilities are the class softmax of the logits path (which reads the same padded tensor) and the logits match the
    float64 oracle as for every other class count."""
    from oracle.hrnet_oracle import hrnet_forward
    from values_amd import _lib
    from values_amd.hrnet import HighResolutionNet, _softmax_pitch
    from values_amd.predict2d import predict_logits_2d
    assert _softmax_pitch(ncls) == pitch
    m = HighResolutionNet(small_cfg(dropout_final=False, ncls=ncls))
    sd = formula_state_dict_from_shapes({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in sd.items()}, strict=False)
    m = m.cuda()
    x = torch.from_numpy(formula_tensor((2, 3, 64, 96), tag=97)).float().cuda()
    lg = predict_logits_2d([m], x)
    pr = predict_logits_2d([m], x, softmax=True)
    torch.cuda.synchronize()
    assert _lib.load().vx_last_kernel_name().decode() == f"bilinear_softmax_nchw_vec_kernel<{inst}>"
    assert lg.shape == pr.shape and lg.shape[2] == ncls
    assert (pr - torch.softmax(lg.double(), 2)).abs().max().item() < 1e-6
    with torch.no_grad():
        y64 = hrnet_forward(dict(HRNET_SMALL_EXTRA, DROPOUT_FINAL=False), {k: torch.from_numpy(v).double() for k, v in sd.items()},
                            x.double().cpu())
    assert (lg[:, 0].double().cpu() - y64).abs().max().item() < LOGIT_TOL
