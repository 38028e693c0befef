"""Generate tests/golden/valstep2d_kat.npz: a tiny 2D SSN head and the reference-dtype (float32) validation/val_loss and
validation/val_dice of forward_ssn(val=True) over it, for ignore_index 0 and 255, full rank and mean_only.

    python tools/gen_golden_valstep2d.py --reference <checkout of the reference>

The reference's HighResolutionNet is IMPORTED in the small SSN configuration (the one tools/gen_golden.py:gen_hrnet_ssn
builds: 4 classes, rank 10, epsilon 1e-5, formula weights) and its hrnet_ssn is called on a formula feature map of
16 x 24, upsampled to 64 x 96.  Stored: what its two head convolutions return at 16 x 24 (the low-resolution mean and
factor that the package's reduction starts from), the labels, the normals that LowRankMultivariateNormal.rsample drew
(captured: eps_w as data, eps_d as a formula tag) and the numbers of forward_ssn(val=True)'s operations in its order on
the samples of that distribution.  torchmetrics is absent here: val_dice is its micro / global definition from per-class
counts (the ignore_index column deleted, 2 tp / (2 tp + fp + fn); a pixel labelled 255 is in no class) written with torch
ops -- parity with the package itself stays unpinned, as for every Dice of this project.  With ignore_index == 0 the
reference calls the cross-entropy WITHOUT ignore_index, so that run's labels are all classes; the ignore_index == 255 run
has 255 on a tenth of the pixels.  The fixture is data only.
"""
import argparse
import copy
import importlib.abc
import importlib.machinery
import math
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, C, R, S = 2, 4, 10, 3
LO, HI = (16, 24), (64, 96)
EPSILON = 1e-5
IGNORE = (0, 255)
EPS_TAG = 9300
MOCK_ROOTS = ("hydra", "omegaconf", "torchmetrics", "batchgenerators", "medpy", "pytorch_lightning", "torchvision", "cv2",
              "albumentations", "jsbeautifier", "pydantic_settings", "SimpleITK")


class _MockFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in MOCK_ROOTS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = MagicMock(name=spec.name)
        m.__path__ = []
        m.__spec__ = spec
        return m

    def exec_module(self, module):
        pass


class _Cfg(dict):
    def __getattr__(self, k):
        v = self[k]
        return _Cfg(v) if isinstance(v, dict) else v


def micro_dice(pred, target, ignore_index):
    tp = fp = fn = 0
    for c in range(C):
        if c == ignore_index:
            continue
        p, t = pred == c, target == c
        tp, fp, fn = tp + int((p & t).sum()), fp + int((p & ~t).sum()), fn + int((~p & t).sum())
    den = 2 * tp + fp + fn
    return torch.tensor(0.0) if den == 0 else torch.tensor(2.0 * tp).float() / torch.tensor(float(den))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "valstep2d_kat.npz"))
    args = ap.parse_args()
    sys.meta_path.insert(0, _MockFinder())
    sys.path.insert(0, args.reference)
    sys.path.insert(0, os.path.join(args.reference, "uncertainty_modeling"))
    import torch.distributions.lowrank_multivariate_normal as lrm
    import uncertainty_modeling.models.hrnet_module as ref_hr
    from tests.formula import HRNET_SMALL_EXTRA, formula_state_dict_from_shapes, formula_tensor

    extra = copy.deepcopy(HRNET_SMALL_EXTRA)
    extra["DROPOUT_FINAL"] = False
    cfg = _Cfg({"MODEL": {"EXTRA": extra, "ALIGN_CORNERS": False, "INPUT_CHANNELS": 3, "PRETRAINED": False,
                          "SSN": True, "SSN_RANK": R, "SSN_EPS": EPSILON},
                "DATASET": {"NUM_CLASSES": C}})
    model = ref_hr.HighResolutionNet(cfg)
    full = model.state_dict()
    for k, v in formula_state_dict_from_shapes({k: tuple(v.shape) for k, v in full.items()}).items():
        full[k] = torch.from_numpy(v).float()
    model.load_state_dict(full)
    model.eval()
    torch.set_grad_enabled(False)
    cin = model.last_layer[0].in_channels
    feat = torch.from_numpy(formula_tensor((B, cin) + LO, tag=91, scale=1.0)).float()
    mean_lo, fac_lo = model.last_layer(feat), model.cov_factor_conv(feat)

    g = torch.Generator().manual_seed(21)
    seg0 = torch.randint(0, C, (B, 1) + HI, generator=g)
    seg255 = seg0.clone()
    seg255[torch.rand(seg0.shape, generator=g) < 0.1] = 255
    out = {"mean_lo": mean_lo.numpy(), "factor_lo": fac_lo.numpy(), "seg_0": seg0.numpy().astype(np.uint8),
           "seg_255": seg255.numpy().astype(np.uint8), "epsilon": np.float32(EPSILON), "eps_d_tag": np.array(EPS_TAG),
           "n_samples": np.array(S), "size": np.array(HI), "ignore_index": np.array(IGNORE, dtype=np.int64)}

    eps_w = torch.from_numpy(formula_tensor((S, B, R), tag=EPS_TAG + 1, scale=1.7)).float()
    eps_d = torch.from_numpy(formula_tensor((S, B, C * HI[0] * HI[1]), tag=EPS_TAG, scale=1.7)).float()
    out["eps_w"] = eps_w.numpy()

    def fake_normal(shape, dtype, device):
        t = eps_w if tuple(shape) == tuple(eps_w.shape) else eps_d
        assert tuple(shape) == tuple(t.shape), shape
        return t.to(dtype)

    orig = lrm._standard_normal
    lrm._standard_normal = fake_normal
    try:
        for name, mean_only in (("ssn", False), ("ssn_mean_only", True)):
            dist = model.hrnet_ssn(feat, HI, mean_only)
            assert isinstance(dist, torch.distributions.LowRankMultivariateNormal)
            samples = dist.rsample([S]).view([S, B, C, *HI])
            for ig, seg in ((0, seg0), (255, seg255)):
                target = seg.long().squeeze(1)
                vd = torch.zeros([S])
                for i, lab in enumerate(torch.argmax(samples, dim=2)):
                    vd[i] = micro_dice(lab, target, ig)
                tt = target.unsqueeze(1)
                tt = tt.expand((S,) + tt.shape).reshape(S * B, -1)
                flat = samples.reshape(S * B, C, -1)
                ce = F.cross_entropy(flat, tt, ignore_index=ig, reduction="none") if ig != 0 else F.cross_entropy(flat, tt, reduction="none")
                ll = torch.mean(torch.logsumexp(torch.sum(-ce.view(S, B, -1), dim=-1), dim=0) - math.log(S))
                out[f"{name}_loss_{ig}"] = (-ll).numpy()
                out[f"{name}_dice_{ig}"] = torch.mean(vd).numpy()
    finally:
        lrm._standard_normal = orig
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes;", {k: float(v) for k, v in out.items() if "loss" in k or "dice" in k})


if __name__ == "__main__":
    main()
