"""CPU: the binding and the argument checks of vx_soft_metric_sums_batched, and the host arithmetic behind
values_amd.metrics.process_metrics_3d (calculate_metrics of test_3D.py:537-575) on reductions built in numpy."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.metrics3d_ref import formula_case, np_counts, np_soft_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(2, 5, 4, (12, 10, 8)), (3, 4, 3, (9, 7, 5)), (2, 1, 1, (4, 4, 4))]


def test_soft_metric_sums_batched_is_bound():
    """one argtype per parameter of the header's prototypes"""
    from values_amd import _lib
    c = ctypes
    assert _lib.SIGNATURES["vx_soft_metric_sums_batched"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_int64,
                                                                        c.c_void_p, c.c_void_p, c.c_void_p])
    assert _lib.SIGNATURES["vx_soft_metric_batched_workspace_bytes"] == (c.c_int64, [c.c_int, c.c_int, c.c_int, c.c_int64])
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "values_amd.h")).read(), flags=re.S)
    for name, res in (("vx_soft_metric_sums_batched", "int"), ("vx_soft_metric_batched_workspace_bytes", "int64_t")):
        proto = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (res, name), src)
        assert proto and len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.load(), name)
    # the one-image entry points are as they were
    assert _lib.SIGNATURES["vx_soft_metric_sums"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int64, c.c_void_p,
                                                                c.c_void_p, c.c_void_p])
    assert _lib.SIGNATURES["vx_soft_metric_workspace_bytes"] == (c.c_int64, [c.c_int, c.c_int])


BAD_SHAPES = [(0, 2, 2, 64), (1, 0, 2, 64), (1, 33, 2, 64), (1, 2, 0, 64), (1, 2, 32, 64), (1, 2, 2, 0), (1, 2, 2, -5),
              (1, 2, 2, (1 << 39) + 1), (-1, 2, 2, 64)]


def test_soft_metric_sums_batched_refuses_bad_arguments_without_a_gpu():
    """argument errors come back before anything touches a device (the pointers are never dereferenced)"""
    from values_amd import _lib
    lib = _lib.load()
    assert lib.vx_version() >= 750
    dummy = 0x10000
    for B, C, R, nvox in BAD_SHAPES:
        assert lib.vx_soft_metric_sums_batched(dummy, dummy, B, C, R, nvox, dummy, dummy, None) == -2, (B, C, R, nvox)   # VX_E_SHAPE
        assert lib.vx_last_error_string().decode().startswith("vx_soft_metric_sums_batched:")
    for k in range(4):                                                                                              # VX_E_NULL
        ptrs = [dummy] * 4
        ptrs[k] = None
        assert lib.vx_soft_metric_sums_batched(ptrs[0], ptrs[1], 1, 2, 2, 64, ptrs[2], ptrs[3], None) == -1, k
        assert lib.vx_last_error_string().decode().startswith("vx_soft_metric_sums_batched:")


def test_workspace_bytes_follow_the_partition_of_one_image():
    from values_amd import _lib
    ws = _lib.load().vx_soft_metric_batched_workspace_bytes
    for B, C, R, nvox in BAD_SHAPES:
        assert ws(B, C, R, nvox) == 0, (B, C, R, nvox)
    for C, R in ((1, 1), (2, 4), (32, 31)):
        row = R * (3 * C + 1) * 8                                  # one workgroup's partial sums
        last = 0
        for nvox in (1, 63, 64, 4096, 4097, 64 ** 3, 100 ** 3 + 1, 1 << 39):
            one = ws(1, C, R, nvox)
            assert one >= row and one % row == 0 and one >= last   # whole partials; never fewer for a larger image
            last = one
            for B in (2, 3, 32):
                assert ws(B, C, R, nvox) == B * one, (B, C, R, nvox)
    assert ws(1, 2, 4, 1) == ws(1, 2, 4, 64)                        # a small image is one workgroup's
    assert ws(1, 2, 4, 1 << 30) > ws(1, 2, 4, 1 << 20) > ws(1, 2, 4, 1 << 10)


def _reductions(C, T, R, shape, tag):
    """sums (1, R, 3C + 1) and the counts (1, 1 + T' + R, ., C) of [mean arg-max, T' sample arg-maxes, raters] in numpy, T' = T
    when the GED is due and 0 otherwise; plus the case itself"""
    from values_amd.metrics import _ged_due
    sm, gt = formula_case(C, T, R, shape, tag)
    mean = sm.mean(0)
    nvox = int(np.prod(shape))
    sums, _ = np_soft_sums(mean.reshape(1, C, nvox), gt.reshape(1, R, nvox))
    stack = [mean.argmax(0)[None]] + ([sm.argmax(1)] if _ged_due(T, R) else []) + [gt]
    I = np_counts(np.concatenate(stack, 0).reshape(1, -1, nvox), C)
    return sm, gt, mean, nvox, sums, I


@pytest.mark.parametrize("C,T,R,shape", CASES)
def test_host_arithmetic_matches_the_oracle(C, T, R, shape):
    """loss against the oracle's SoftDiceLoss + NLLLoss with the float32 log the kernel takes (1e-9: float64 sums in another
    order) and against its calculate_test_metrics as it stands (float64 log: 1e-5, the project's loss tolerance);
    dice and the GED keys 1e-12 (ratios of the same integers)"""
    from oracle import metrics_oracle as mo
    from values_amd.metrics import _metrics_3d_from_reductions, _test_metrics_from_sums
    sm, gt, mean, nvox, sums, I = _reductions(C, T, R, shape, 0)
    got = _metrics_3d_from_reductions(sums, I, C, nvox, T, R)
    assert len(got) == 1
    got = got[0]
    mean64 = mean[None].astype(np.float64)
    log32 = np.log(mean[None].astype(np.float32)).astype(np.float64)
    loss32 = float(np.mean([mo.soft_dice_loss(mean64, gt[r][None]) + mo.nll_loss(log32, gt[r][None]) for r in range(R)]))
    ref = mo.calculate_test_metrics(mean64, gt)
    print("loss", got["loss"], loss32, ref["loss"], "dice", got["dice"], ref["dice"])
    assert abs(got["loss"] - loss32) < 1e-9
    assert abs(got["loss"] - ref["loss"]) < 1e-5
    assert abs(got["dice"] - ref["dice"]) < 1e-12
    ged = mo.calculate_ged(sm, gt, ignore_index=0, ged_only=False)
    if R > 1 or T > 1:
        assert set(got) == {"loss", "dice"} | set(ged)
        for k in ged:
            assert abs(got[k] - ged[k]) < 1e-12, k
    else:
        assert list(got) == ["loss", "dice"]
    # the per-image helper on the same rows: rater rows named, or the default layout [arg-max, raters]
    G = list(range(I.shape[1] - R, I.shape[1]))
    assert _test_metrics_from_sums(sums[0], I[0], C, nvox, 0, G) == {"loss": got["loss"], "dice": got["dice"]}
    keep = [0] + G
    assert _test_metrics_from_sums(sums[0], I[0][np.ix_(keep, keep)], C, nvox) == {"loss": got["loss"], "dice": got["dice"]}


@pytest.mark.parametrize("T,R,keys", [(1, 1, False), (None, 1, False), (None, 3, False), (1, 2, True), (2, 1, True), (3, 2, True)])
def test_key_set_follows_the_reference_condition(T, R, keys):
    """GED keys when R > 1 or T > 1 (test_3D.py:554); without per-sample masks (T unknown) loss and dice only"""
    from values_amd.metrics import _ged_due, _metrics_3d_from_reductions
    C, shape = 2, (4, 5, 3)
    sm, gt = formula_case(C, T or 1, R, shape, 7)
    nvox = int(np.prod(shape))
    mean = sm.mean(0)
    sums, _ = np_soft_sums(mean.reshape(1, C, nvox), gt.reshape(1, R, nvox))
    assert _ged_due(T, R) == keys
    stack = [mean.argmax(0)[None]] + ([sm.argmax(1)] if keys else []) + [gt]
    I = np_counts(np.concatenate(stack, 0).reshape(1, -1, nvox), C)
    got = _metrics_3d_from_reductions(sums, I, C, nvox, T, R)[0]
    want = ["loss", "dice"]
    if keys:
        want += ["ged"] + (["max dice rater {}".format(r) for r in range(R)] + ["max dice pred"] if R > 1 else [])
    assert list(got) == want
