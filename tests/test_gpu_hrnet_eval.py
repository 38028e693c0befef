"""GPU: values_amd.HighResolutionNet in eval mode (running-statistics BatchNorm in the conv epilogue) against the fixtures
the reference class produced with model.eval() (tools/gen_golden_hrnet_eval.py): formula weights, running statistics
calibrated over two batches, 2 x 3 x 64 x 96 inputs, the small layout (widths 16 .. 128) and the W18 widths (18 .. 144, 270
concatenated: padded channel tails pass through the epilogue).

Tolerance: the rule of test_config_C4_w18_full_layout_at_256x478_matches_reference_fixture -- against the reference's float32
logits max(1e-4, 2 gap), against its float64 logits 2 gap, gap = the reference's own float32-vs-float64 distance, read from the
fixture."""
import copy
import json

import numpy as np
import pytest
import torch

from tests.helpers import load_npz
from tests.formula import HRNET_SMALL_EXTRA, HRNET_W18S_EXTRA, formula_state_dict_from_shapes

pytestmark = pytest.mark.gpu
LAYOUTS = {"small": ("hrnet_eval_small.npz", HRNET_SMALL_EXTRA), "w18s": ("hrnet_eval_w18s.npz", HRNET_W18S_EXTRA)}
_cache = {}


def fixture(layout):
    if layout not in _cache:        # loaded once, shared, never written
        _cache[layout] = load_npz(LAYOUTS[layout][0])
    return _cache[layout]


def make(layout, dropout_final=False, ssn=False, eval_mode=True, stats=True):
    from values_amd.hrnet import HighResolutionNet
    g = fixture(layout)
    extra = dict(copy.deepcopy(LAYOUTS[layout][1]), DROPOUT_FINAL=dropout_final)
    model_cfg = {"EXTRA": extra, "ALIGN_CORNERS": False, "INPUT_CHANNELS": 3, "PRETRAINED": False}
    if ssn:
        model_cfg.update(SSN=True, SSN_RANK=10, SSN_EPS=1e-5)
    m = HighResolutionNet({"MODEL": model_cfg, "DATASET": {"NUM_CLASSES": 4}})
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    if not ssn:
        assert shapes == {k: tuple(v) for k, v in json.loads(bytes(g["shapes_json"]).decode()).items()}
    sd = {k: torch.from_numpy(v).float() for k, v in formula_state_dict_from_shapes(shapes).items()}
    if stats:
        for k in shapes:
            if k.endswith(("running_mean", "running_var")):
                # (the SSN factor head's BatchNorm is not in the fixture: it takes the mean head's statistics)
                sd[k] = torch.from_numpy(g[k.replace("cov_factor_conv", "last_layer")])
    missing = m.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys
    assert all(k.endswith("num_batches_tracked") or not stats for k in missing.missing_keys)
    m = m.cuda()
    return m.eval() if eval_mode else m


def x_of(layout):
    return torch.from_numpy(fixture(layout)["input"]).cuda()


def masks_of(g):
    out = []
    for i in range(4):
        shape = tuple(int(v) for v in g[f"maskshape_{i}"])
        out.append(torch.from_numpy(np.unpackbits(g[f"mask_0_{i}"])[:int(np.prod(shape))].astype(bool).reshape(shape)))
    return out


def check_rule(y, ref32, ref64_minus32, gap, what):
    y = y.astype(np.float64)
    d32 = np.abs(y - ref32.astype(np.float64)).max()
    d64 = np.abs(y - (ref32.astype(np.float64) + ref64_minus32.astype(np.float64))).max()
    print(f"{what}: max|d| vs reference f32 {d32:.3e} (bound {max(1e-4, 2 * gap):.3e}), vs reference f64 {d64:.3e} "
          f"(bound {2 * gap:.3e}); reference f32-vs-f64 gap {gap:.3e}")
    assert d32 <= max(1e-4, 2 * gap), (what, d32)
    assert d64 <= 2 * gap, (what, d64)


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_eval_logits_match_the_reference_in_eval_mode(layout):
    g = fixture(layout)
    m = make(layout)
    y = m(x_of(layout))
    assert y.shape == (2, 4, 64, 96)
    check_rule(y.cpu().numpy(), g["logits_eval"], g["logits_eval64_minus32"], float(g["ref_f32_f64_gap"]), f"eval logits ({layout})")


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_fused_epilogue_and_unfused_route_give_the_same_bits(layout, monkeypatch):
    m = make(layout)
    x = x_of(layout)
    monkeypatch.delenv("VX_HRNET_NO_FOLD", raising=False)
    fused = m(x).clone()
    monkeypatch.setenv("VX_HRNET_NO_FOLD", "1")
    unfused = m(x).clone()
    assert torch.equal(fused, unfused)
    monkeypatch.setenv("VX_HRNET_NO_MULTIFUSE", "1")      # ... and the term-by-term SUM fusion
    assert torch.equal(m(x), fused)


def test_fused_and_unfused_ssn_head(monkeypatch):
    m = make("small", ssn=True)
    x = x_of("small")
    monkeypatch.delenv("VX_HRNET_NO_FOLD", raising=False)
    fused = m.forward_ssn(x).mean.clone()
    assert fused.shape == (2, 4 * 64 * 96) and bool(torch.isfinite(fused).all())
    monkeypatch.setenv("VX_HRNET_NO_FOLD", "1")
    assert torch.equal(m.forward_ssn(x).mean, fused)
    # the mean head is the plain model's last_layer on the same backbone and statistics
    monkeypatch.delenv("VX_HRNET_NO_FOLD", raising=False)
    assert torch.equal(fused.view(2, 4, 64, 96), make("small")(x))


# 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_eval_logits_do_not_depend_on_the_batch(layout):
    from values_amd.predict2d import predict_logits_2d
    m = make(layout)
    x = x_of(layout)
    x3 = torch.cat([x, torch.flip(x[1:], [-2])], 0)
    alone = m(x[:1]).clone()
    assert torch.equal(m(x3)[0], alone[0])
    # ... nor on the other view of a batched TTA forward (two statistics groups in train mode; none here)
    lg = predict_logits_2d([m], [x[:1], x[1:]], tta=True, hflip_views=[False, False])
    assert lg.shape == (1, 2, 4, 64, 96)
    assert torch.equal(lg[0, 0], alone[0])
    assert torch.equal(lg[0, 1], m(x[1:])[0])


# 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_dropout_final_stays_live_in_eval_mode(layout):
    g = fixture(layout)
    m = make(layout, dropout_final=True)
    x = x_of(layout)
    y = m.forward_samples(x, 1, dropout_masks=[masks_of(g)])[0]
    check_rule(y.cpu().numpy(), g["logits_drop"], g["logits_drop64_minus32"], float(g["ref_drop_f32_f64_gap"]),
               f"DROPOUT_FINAL pass in eval mode ({layout})")
    a = m.forward_samples(x, 3, seeds=[11, 12, 13])
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2]) and not torch.equal(a[0], a[2])
    for t, seed in enumerate((11, 12, 13)):
        assert torch.equal(m.forward_samples(x, 1, seeds=[seed])[0], a[t])


# 5 ------------------------------------------------------------------------------------------------------------------
def test_eval_leaves_nothing_behind_in_train_mode_and_follows_load_state_dict():
    x = x_of("w18s")
    fresh = make("w18s", eval_mode=False)(x).clone()        # never in eval mode
    m = make("w18s")
    ev = m(x).clone()
    m.train()
    assert torch.equal(m(x), fresh)
    assert not torch.equal(ev, fresh)
    m.eval()
    assert torch.equal(m(x), ev)
    sd = {k: (v * 1.5 if k.endswith("running_var") else v + 0.25) for k, v in m.state_dict().items()
          if k.endswith(("running_mean", "running_var"))}
    m.load_state_dict(sd, strict=False)
    moved = m(x).clone()
    assert (moved - ev).abs().max().item() > 1e-3           # the table was rebuilt from the new statistics
    m.train()
    assert torch.equal(m(x), fresh)                         # train mode never reads them


# 6 ------------------------------------------------------------------------------------------------------------------
def test_graphed_predictor_replays_the_eager_bits_in_eval_mode():
    from values_amd.predict2d import GraphedPredictor2D, predict_logits_2d, process_output_2d
    m = make("w18s")
    x = x_of("w18s")
    hf = [False, True]      # two TTA views (one forward of two groups; T = 2: every map of process_output_2d is capturable)

    def views(t):
        return [t, torch.flip(t, [-1])]

    eager = predict_logits_2d([m], views(x), tta=True, hflip_views=hf).clone()
    ref = process_output_2d(eager)
    gp = GraphedPredictor2D([m], views(x), tta=True, hflip_views=hf)
    gp(views(torch.flip(x, [-2])))      # another input first: the graph computes, it does not remember
    torch.cuda.synchronize()
    assert not torch.equal(gp.logits, eager)
    out = gp(views(x))
    torch.cuda.synchronize()
    assert torch.equal(gp.logits, eager)
    assert torch.equal(out["pred_entropy"], ref["pred_entropy"])
    assert torch.equal(predict_logits_2d([m], views(x), tta=True, hflip_views=hf), eager)     # eager still works beside the graph


# 7 ------------------------------------------------------------------------------------------------------------------
def test_zero_tails_survive_the_eval_forward(monkeypatch):
    m = make("w18s")
    x = x_of("w18s")
    monkeypatch.delenv("VX_HRNET_NO_FOLD", raising=False)
    m(x)
    assert m._zreal and m.zero_tails_intact()
    monkeypatch.setenv("VX_HRNET_NO_FOLD", "1")
    m(x)
    assert m.zero_tails_intact()
