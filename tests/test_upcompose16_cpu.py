"""CPU: the algebra of the composed level-1 up-convolution (values_amd/csrc/upcompose16.h, the function the device pack kernel
evaluates), compiled into a stand-alone host program under AddressSanitizer + UBSan, against a float64 torch restatement -- and
the restatement itself against conv3d(conv_transpose3d(coarse)) on a grid that holds every border class."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.formula import formula_tensor
from tests.upcompose16_ref import apply_composed, formula_weights, weff_btab
from tests.helpers import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables():
    w1, uw, ub = formula_weights()
    return (w1, uw, ub) + weff_btab(w1, uw, ub)


def test_host_function_matches_the_float64_restatement(tables, tmp_path):
    w1, uw, ub, weff, btab = tables
    exe = str(tmp_path / "upcompose16_host")
    build_host_program(os.path.join(ROOT, "tests", "upcompose16_host.cpp"), exe)
    blob = tmp_path / "w.bin"
    np.concatenate([w1.numpy().ravel(), uw.numpy().ravel(), ub.numpy().ravel()]).astype(np.float32).tofile(blob)
    lines = subprocess.check_output([exe, str(blob)]).decode().split("\n")
    vals = np.array([float(v) for v in lines[:8 * 8 * 32 * 16 + 27 * 16]])
    assert lines[len(vals)] == "floats %d" % (8 * 8 * 2 * 64 * 8 // 2 + 27 * 16)
    got_w = vals[:8 * 8 * 32 * 16].reshape(8, 8, 32, 16)
    got_b = vals[8 * 8 * 32 * 16:].reshape(3, 3, 3, 16)
    for got, want in ((got_w, weff.numpy()), (got_b, btab.numpy())):
        scale = np.abs(want).max()
        assert scale > 0.05
        err = np.abs(got - want).max()
        print("max |host - torch| =", err, "at scale", scale)
        assert err <= 1e-12 * scale


def test_composed_tables_rebuild_the_two_stage_result(tables):
    """conv3d(conv_transpose3d(coarse) + up_b, padding = 1) on a fine grid of 4 x 8 x 32: every voxel is a border voxel in z,
    y and x have first / interior / last"""
    w1, uw, ub, weff, btab = tables
    coarse = torch.from_numpy(formula_tensor((2, 32, 2, 4, 16), 915, scale=1.3)).double()
    up = F.conv_transpose3d(coarse, uw.double(), ub.double(), stride=2)
    want = F.conv3d(up, w1.double()[:, :16].contiguous(), None, padding=1)
    got = apply_composed(coarse, weff, btab)
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print("max |composed - two-stage| =", err, "at |out| up to", scale)
    assert scale > 1.0 and err <= 1e-12 * scale
