"""CPU: the eval-mode HRNet fixtures (tools/gen_golden_hrnet_eval.py) are what the GPU tests need them to be, and the ABI
of the running-statistics path is in place."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.helpers import load_npz

FIXTURES = ("hrnet_eval_small.npz", "hrnet_eval_w18s.npz")


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_separates_eval_from_train(name):
    g = load_npz(name)
    assert g["input"].shape == (2, 3, 64, 96) and g["input"].dtype == np.float32
    assert g["logits_eval"].shape == g["logits_eval64_minus32"].shape == g["logits_drop"].shape == (2, 4, 64, 96)
    gap = float(g["ref_f32_f64_gap"])
    # the float64 logits travel as a float32 residual against the float32 ones: the stored gap is the residual's maximum
    assert abs(float(np.abs(g["logits_eval64_minus32"]).max()) - gap) <= 1e-6 * gap
    assert 0 < gap < 1e-3
    # a forward that ignores .eval() (batch statistics) cannot pass the golden test: the reference's own train-mode logits
    # sit at least 100 tolerances away from its eval-mode logits
    assert float(g["train_eval_gap"]) >= 100 * max(1e-4, 2 * gap)
    means = [v for k, v in g.items() if k.endswith("running_mean")]
    variances = [v for k, v in g.items() if k.endswith("running_var")]
    assert len(means) == len(variances) > 20
    assert all(bool((v > 0).all()) for v in variances)
    assert not all(bool((m == 0).all()) for m in means)
    assert any(bool((np.abs(v - 1) > 1e-3).any()) for v in variances)       # calibrated, not the defaults
    for i in range(4):
        shape = tuple(int(v) for v in g[f"maskshape_{i}"])
        assert g[f"mask_0_{i}"].size * 8 >= int(np.prod(shape))
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", name)) < (1 << 20)


def test_w18s_fixture_has_padded_widths():
    g = load_npz("hrnet_eval_w18s.npz")
    widths = {v.shape[0] for k, v in g.items() if k.endswith("running_var")}
    assert {18, 36, 72, 144, 270} <= widths


def test_abi_of_the_running_statistics_path():
    from values_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "values_amd.h")).read()
    assert re.search(r"\bint\s+vx_bn_running_affine\s*\(", header)
    assert "vx_bn_running_affine" in _lib.SIGNATURES
    body = re.search(r"typedef struct vx_conv2d_args \{(.*?)\} vx_conv2d_args;", header, re.S).group(1)
    names = [n for n, _ in _lib.Conv2dArgs._fields_]
    new = ["out_scale", "out_shift", "out_add", "out_add_pitch", "out_act"]
    assert names[-5:] == new                                   # appended: a caller's zero-initialised struct keeps today's path
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)           # declarations only
    pos = [re.search(r"\b%s\s*[;,]" % n, body).start() for n in ("in_relu",) + tuple(new)]
    assert pos == sorted(pos)
    a = _lib.Conv2dArgs()
    assert a.out_scale is None and a.out_shift is None and a.out_add is None and a.out_add_pitch == 0
    assert a.out_act == _lib.VX_ACT_NONE == 0
    it = re.search(r"typedef struct vx_bn_affine_item \{(.*?)\} vx_bn_affine_item;", header, re.S).group(1)
    for n, _ in _lib.BnAffineItem._fields_:
        assert re.search(r"\b%s\b" % n, it), n
    assert ctypes.sizeof(_lib.BnAffineItem) == 6 * ctypes.sizeof(ctypes.c_void_p) + 8
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.load().vx_version() >= 850
