#!/usr/bin/env python3
"""Generate the eval-mode HRNet fixtures (target `hrnet_eval`) by IMPORTING the reference class, like the other HRNet
targets of tools/gen_golden.py (whose import mocks, config object and output directory this tool reuses).

    python tools/gen_golden_hrnet_eval.py      # writes tests/golden/hrnet_eval_small.npz and hrnet_eval_w18s.npz

Recipe (the same for both layouts): formula weights (tests.formula, not stored); running statistics CALIBRATED as a
real checkpoint gets them -- the reference module in train mode with momentum=None (cumulative average) over two
calibration batches that are not the test input -- then .eval().  Stored: the input, every BatchNorm's running_mean /
running_var under its state-dict name, the reference's eval logits in float32 and float64 (the latter as a float32
residual against the former) with their gap, the gap between its train-mode and eval-mode logits on the same input,
and one DROPOUT_FINAL pass with the captured masks (float32, and float64 with the same masks, again as a residual).
"""
from __future__ import annotations

import copy
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden as gg  # noqa: E402  (installs the import mocks and the reference's path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tests.formula import HRNET_SMALL_EXTRA, HRNET_W18S_EXTRA, formula_state_dict_from_shapes, formula_tensor  # noqa: E402

SIZE = (2, 3, 64, 96)


def _cfg(extra, ncls):
    return gg._Cfg({"MODEL": {"EXTRA": extra, "ALIGN_CORNERS": False, "INPUT_CHANNELS": 3, "PRETRAINED": False},
                    "DATASET": {"NUM_CLASSES": ncls}})


def gen_hrnet_eval(extra_src, ncls, tag, fname):
    import uncertainty_modeling.models.hrnet_module as ref_hr
    torch.set_grad_enabled(False)
    extra = copy.deepcopy(extra_src)
    extra["DROPOUT_FINAL"] = False
    model = ref_hr.HighResolutionNet(_cfg(extra, ncls))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    full = model.state_dict()
    for k, v in formula_state_dict_from_shapes(shapes).items():
        full[k] = torch.from_numpy(v).float()
    model.load_state_dict(full)
    # calibration: cumulative-average running statistics over two batches that are not the test input
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = None
    for k in range(2):
        model.forward(torch.from_numpy(formula_tensor(SIZE, tag=tag + 100 + k, scale=1.5)).float())
    full = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.from_numpy(formula_tensor(SIZE, tag=tag, scale=1.5)).float()
    out = {"input": x.numpy(),
           "shapes_json": np.frombuffer(json.dumps({k: list(v) for k, v in shapes.items()}).encode(), dtype=np.uint8)}
    for k, v in full.items():
        if k.endswith(("running_mean", "running_var")):
            out[k] = v.numpy().copy()
    # train-mode logits on the test input (a copy: the forward moves the running statistics)
    mt = copy.deepcopy(model).train()
    y_train = mt.forward(x).numpy().copy()
    model.eval()
    y32 = model.forward(x).numpy().copy()
    m64 = ref_hr.HighResolutionNet(_cfg(extra, ncls)).double()
    m64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in full.items()})
    m64.eval()
    y64 = m64.forward(x.double()).numpy().copy()
    # float64 results travel as float32 residuals against the float32 logits (float64(logits) + float64(residual)
    # restores them to ~1e-12; the full float64 arrays would put a fixture past the size limit of a committed file)
    out["logits_eval"] = y32
    out["logits_eval64_minus32"] = (y64 - y32.astype(np.float64)).astype(np.float32)
    out["ref_f32_f64_gap"] = np.array(np.abs(y32 - y64).max())
    out["train_eval_gap"] = np.array(np.abs(y_train - y32).max())
    # one DROPOUT_FINAL pass in eval mode (F.dropout(training=True) stays live, hrnet_module.py:642-646), masks captured
    extra_d = copy.deepcopy(extra_src)
    extra_d["DROPOUT_FINAL"] = True
    masks = []
    orig = F.dropout

    def spy(inp, p=0.5, training=True, inplace=False):
        o = orig(inp, p, training, inplace)
        masks.append(((o != 0) | (inp == 0)).clone())
        return o

    torch.manual_seed(tag)
    ref_hr.F.dropout = spy
    try:
        md, md64 = ref_hr.HighResolutionNet(_cfg(extra_d, ncls)), ref_hr.HighResolutionNet(_cfg(extra_d, ncls)).double()
        md.load_state_dict(full)
        md.eval()
        out["logits_drop"] = md.forward(x).numpy().copy()
        keep = [m.clone() for m in masks]
    finally:
        ref_hr.F.dropout = orig
    for i, m in enumerate(keep):
        out[f"mask_0_{i}"] = np.packbits(m.numpy().astype(np.uint8).ravel())
        out[f"maskshape_{i}"] = np.array(m.shape)
    # the same pass in float64 with the SAME masks: the reference's own float32-vs-float64 gap of the dropout pass
    it = iter(keep)
    ref_hr.F.dropout = lambda inp, p=0.5, training=True, inplace=False: inp * next(it).to(inp.dtype) * 2.0
    try:
        md64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in full.items()})
        md64.eval()
        y_d64 = md64.forward(x.double()).numpy()
    finally:
        ref_hr.F.dropout = orig
    out["logits_drop64_minus32"] = (y_d64 - out["logits_drop"].astype(np.float64)).astype(np.float32)
    out["ref_drop_f32_f64_gap"] = np.array(np.abs(out["logits_drop"] - y_d64).max())
    torch.set_grad_enabled(True)
    path = os.path.join(gg.OUT, fname)
    np.savez_compressed(path, **out)
    rv = np.concatenate([v.ravel() for k, v in out.items() if k.endswith("running_var")])
    print(fname, y32.shape, os.path.getsize(path) / 1e6, "MB; logit range", float(y32.min()), float(y32.max()),
          "f32-vs-f64 gap", float(out["ref_f32_f64_gap"]), "drop gap", float(out["ref_drop_f32_f64_gap"]),
          "train-vs-eval gap", float(out["train_eval_gap"]), "running_var range", float(rv.min()), float(rv.max()))


if __name__ == "__main__":
    gen_hrnet_eval(HRNET_SMALL_EXTRA, 4, 91, "hrnet_eval_small.npz")
    gen_hrnet_eval(HRNET_W18S_EXTRA, 4, 93, "hrnet_eval_w18s.npz")
