"""CPU: the host half of the batched evaluation scores (values_amd/evalmetrics.py, csrc/evalmetrics.hip): the ABI
structs against the C header, the workspace queries and the refusals that happen before any device call, and the
lock-step Platt controller driven by a numpy stand-in for the device sums.  No device call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, DTYPE, WORKSPACE = -1, -2, -3, -4


def test_item_struct_sizes_match_c(tmp_path):
    from values_amd import _lib
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "values_amd.h"
int main(void){printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(vx_em_item), sizeof(vx_ncc_item), offsetof(vx_em_item, nvox),
 offsetof(vx_em_item, R), offsetof(vx_ncc_item, n_pred), offsetof(vx_ncc_item, gt_R), VX_EM_MAX_ITEMS); return 0;}
'''
    (tmp_path / "s.c").write_text(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got == [ctypes.sizeof(_lib.EmItem), ctypes.sizeof(_lib.NccItem), _lib.EmItem.nvox.offset, _lib.EmItem.R.offset,
                   _lib.NccItem.n_pred.offset, _lib.NccItem.gt_R.offset, _lib.VX_EM_MAX_ITEMS]


def _err():
    from values_amd import _lib
    return _lib.load().vx_last_error_string()


def test_rater_workspace_queries_and_refusals_need_no_device():
    from values_amd import _lib
    lib = _lib.load()
    P = 0x1000                                   # never dereferenced: every call below ends in a host-side check
    item = lambda nvox=1000, R=2, dtype=_lib.VX_F32, unc=P, ref=P, pred=P: _lib.EmItem(unc, ref, pred, nvox, dtype, R)
    arr = lambda *its: (_lib.EmItem * len(its))(*its)
    good = arr(item(), item(64 ** 3, 4, _lib.VX_F64), item(1, 1))
    params = (ctypes.c_double * 12)(*([0.0, 0.0, 0.5, 0.5] * 3))
    edges = (ctypes.c_double * 21)(*np.linspace(0.0, 1.0 + 1e-8, 21).tolist())
    out = ctypes.c_void_p(P)
    # 512 partial rows of K doubles per item behind a descriptor table of at most 128 bytes per item
    for query, K in ((lib.vx_platt_batched_workspace_bytes, 8), (lib.vx_calib_batched_workspace_bytes, 63)):
        for n in (1, 3):
            ws = query(good, n)
            assert n * 512 * K * 8 < ws <= n * 512 * K * 8 + 128 * n + 256, (K, n, ws)
        assert query(good, 0) == 0 and query(good, 4097) == 0 and query(None, 1) == 0

    def platt(items, n, ws_bytes=1 << 30, par=params):
        return lib.vx_platt_sums_batched(items, n, par, -1, out, out, ws_bytes, None)

    def bins(items, n, ws_bytes=1 << 30):
        return lib.vx_calib_bins_batched(items, n, params, edges, -1, out, out, ws_bytes, None)
    for call, query in ((platt, lib.vx_platt_batched_workspace_bytes), (bins, lib.vx_calib_batched_workspace_bytes)):
        for n in (0, 4097):
            assert call(good, n) == SHAPE and b"n_items" in _err()
        for bad, code in ((item(unc=None), NULL), (item(ref=None), NULL), (item(pred=None), NULL), (item(R=0), SHAPE),
                          (item(nvox=0), SHAPE), (item(dtype=7), DTYPE), (item(R=3, nvox=2 ** 62), SHAPE)):
            items = arr(item(), bad, item())
            assert query(items, 3) == 0
            assert call(items, 3) == code, (code, _err())
            assert b"item 1" in _err()
        assert call(None, 1) == NULL
        assert call(good, 3, 16) == WORKSPACE and b"workspace needs" in _err()
    assert platt(good, 3, par=None) == NULL
    assert lib.vx_calib_bins_batched(good, 3, params, None, -1, out, out, 1 << 30, None) == NULL
    assert lib.vx_platt_sums_batched(good, 3, params, -1, None, out, 1 << 30, None) == NULL


def test_ncc_workspace_query_and_refusals_need_no_device():
    from values_amd import _lib
    lib = _lib.load()
    P = 0x1000
    F32, F64 = _lib.VX_F32, _lib.VX_F64
    item = lambda n=1000, n_pred=None, gd=F32, pd=F64, R=0, gt=P, pred=P: _lib.NccItem(gt, pred, n, n if n_pred is None else n_pred,
                                                                                       gd, pd, R, 0)
    arr = lambda *its: (_lib.NccItem * len(its))(*its)
    good = arr(item(), item(300001, R=4, gd=99), item(1))          # (the dtype of a rater stack is not read)
    out = ctypes.c_void_p(P)
    for n in (1, 3):
        ws = lib.vx_ncc_batched_workspace_bytes(good, n)
        assert n * 512 * 3 * 8 < ws <= n * 512 * 3 * 8 + 128 * n + 256
    call = lambda items, n, ws_bytes=1 << 30: lib.vx_ncc_batched(items, n, out, out, ws_bytes, None)
    for n in (0, 4097):
        assert lib.vx_ncc_batched_workspace_bytes(good, n) == 0
        assert call(good, n) == SHAPE and b"n_items" in _err()
    for bad, code, text in ((item(gt=None), NULL, b"null map"), (item(pred=None), NULL, b"null map"), (item(gd=5), DTYPE, b"dtypes"),
                            (item(pd=-1), DTYPE, b"dtypes"), (item(R=-1), SHAPE, b"gt_R"), (item(n=0), SHAPE, b"empty"),
                            (item(n=100, n_pred=101), SHAPE, b"different size"), (item(n=2 ** 62, R=3), SHAPE, b"gt_R")):
        items = arr(item(), item(), bad)
        assert lib.vx_ncc_batched_workspace_bytes(items, 3) == 0
        assert call(items, 3) == code, (code, _err())
        assert b"item 2" in _err() and text in _err(), _err()
    assert call(good, 3, 64) == WORKSPACE
    assert lib.vx_ncc_batched(good, 3, None, out, 1 << 30, None) == NULL
    assert lib.vx_rater_variance(None, 2, 10, out, None) == NULL and lib.vx_rater_variance(out, 0, 10, out, None) == SHAPE
    assert lib.vx_rater_variance(out, 2, 0, out, None) == SHAPE


# ----------------------------------------------------------------------------------------------- lock-step controller
def test_lockstep_controller_visits_the_per_image_sequence():
    from tests.em_inputs import platt_items, platt_sums_numpy
    from values_amd.evalmetrics import _platt_fit_lockstep, _platt_fit_one
    items = platt_items()
    single = [_platt_fit_one(lambda A, B, tp, tn, u=u, c=c: platt_sums_numpy(u, c, A, B, tp, tn)) for u, c in items]
    rounds = []

    def evaluate(indices, requests):
        rounds.append(list(indices))
        return [platt_sums_numpy(*items[i], *req) for i, req in zip(indices, requests)]
    batch = _platt_fit_lockstep(len(items), evaluate)
    for i, (one, many) in enumerate(zip(single, batch)):
        assert many.visited == one.visited, i                 # the same (phase, A, B, t) at every evaluation
        assert many.result == one.result and many.iters == one.iters
    # every round holds exactly the unfinished items, each item once; an item takes part in len(visited) rounds
    assert rounds[0] == list(range(len(items)))
    for i, one in enumerate(single):
        assert [i in r for r in rounds] == [k < len(one.visited) for k in range(len(rounds))]
    assert len(rounds) == max(len(f.visited) for f in single)
    lengths = [len(f.visited) for f in single]
    assert len(set(lengths)) >= 4, lengths                    # they finish in different rounds
    # item 0 is done after the start point; the heavy-tailed items need halved steps
    assert [v[0] for v in single[0].visited] == ["counts", "start"] and single[0].iters == 0
    for f in single[4:]:
        assert any(v[0] == "line_search" for v in f.visited) and min(v[3] for v in f.visited) < 1.0
    for f in single[1:4]:
        assert all(v[0] != "line_search" for v in f.visited) and f.iters >= 2
    # max_iter bounds the accepted steps in both controllers alike
    capped = _platt_fit_lockstep(len(items), evaluate, max_iter=2)
    for i, (u, c) in enumerate(items):
        one = _platt_fit_one(lambda A, B, tp, tn: platt_sums_numpy(u, c, A, B, tp, tn), max_iter=2)
        assert capped[i].visited == one.visited and one.iters <= 2
    with pytest.raises(ValueError, match="item 1"):
        _platt_fit_lockstep(2, lambda idx, req: [[1.0, 1.0] + [0.0] * 6, [0.0] * 8][:len(idx)])


def test_rater_variance_restated_in_kernel_order_is_numpys():
    """em_rater_var (evalmetrics.hip) adds the raters in index order, divides by R, adds the squared deviations in index
    order, divides by R, all in float64 with no fused multiply-add: restated in numpy, that is np.var(labels, axis=0) bit
    for bit on the cases the GPU test uses, for every label dtype a results tree holds"""
    from tests.em_inputs import rater_label_cases, rater_variance_restated
    for labels in rater_label_cases():
        for dt in (np.uint8, np.int16, np.int32, np.int64):
            lab = labels.astype(dt)
            want = np.var(lab, axis=0)
            assert want.dtype == np.float64
            assert np.array_equal(rater_variance_restated(lab), want), (labels.shape, dt)
    assert np.var(rater_label_cases()[-1], axis=0).max() > 0


def _wave_sum_scalar(x):
    """one wave's share of the documented association, one Python float at a time: lane i holds 0.0 + x[i] (lanes past the
    end hold 0.0), the shuffle-down tree, then the three idle waves and the 511 idle block rows, each 0.0"""
    lanes = [0.0] * 64
    for i, v in enumerate(x):
        lanes[i] = 0.0 + float(v)
    for off in (32, 16, 8, 4, 2, 1):
        new = list(lanes)
        for lane in range(64):
            new[lane] = lanes[lane] + lanes[lane + off if lane + off < 64 else lane]   # (__shfl_down past the wave: own value)
        lanes = new
    block = 0.0
    for w in range(4):
        block += lanes[0] if w == 0 else 0.0
    total = 0.0
    for b in range(512):
        total += block if b == 0 else 0.0
    return total


def test_ncc_sums_restated_follows_the_documented_association():
    """tests/em_inputs.ncc_sums_restated, the host reference of the GPU test's `==` on the five NCC sums: numpy's own sums
    to 1e-12 relative at a size below one wave row and at one element more than the grid has threads, and for at most 64
    elements the explicit scalar loop over one wave's lanes, bit for bit"""
    from tests.em_inputs import ncc_sums_restated
    rng = np.random.default_rng(41)
    for n, dg, dp in ((255, np.float32, np.float64), (131073, np.float64, np.float32)):
        g = rng.random(n).astype(dg)
        p = (0.6 * g + 0.4 * rng.random(n)).astype(dp)
        got = ncc_sums_restated(g, p)
        g64, p64 = g.astype(np.float64), p.astype(np.float64)
        da, db = g64 - g64.sum() / n, p64 - p64.sum() / n
        want = [g64.sum(), p64.sum(), (da * da).sum(), (db * db).sum(), (da * db).sum()]
        assert len(got) == 5 and all(type(v) is float for v in got)
        for k, (a, b) in enumerate(zip(got, want)):
            assert abs(a - b) <= 1e-12 * abs(b), (n, k, a, b)
    for n in (1, 2, 37, 64):
        g = rng.random(n).astype(np.float32)
        p = rng.normal(size=n)
        got = ncc_sums_restated(g, p)
        g64, p64 = [float(v) for v in g], [float(v) for v in p]
        sg, sp = _wave_sum_scalar(g64), _wave_sum_scalar(p64)
        da, db = [v - sg / n for v in g64], [v - sp / n for v in p64]
        want = [sg, sp, _wave_sum_scalar([a * a for a in da]), _wave_sum_scalar([b * b for b in db]),
                _wave_sum_scalar([a * b for a, b in zip(da, db)])]
        assert got == want, (n, got, want)
