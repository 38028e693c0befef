"""CPU: the host half of values_amd.aggregation: the ABI structs against the C header, spec building from aggregation
configs, result-dict assembly from a hand-written device array; the host restatement of the device's summation order
(tests/agg_restated.py) against the oracle, and the inputs that can tell one order from another.  No device call."""
import builtins
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = "values_amd.aggregation."


def test_agg_struct_sizes_and_constants_match_c(tmp_path):
    from values_amd import _lib
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "values_amd.h"
int main(void){printf("%zu %zu %zu %zu %d %d %d\n", sizeof(vx_agg_item), sizeof(vx_agg_spec), offsetof(vx_agg_item, H),
 offsetof(vx_agg_spec, thr), VX_AGG_IMAGE, VX_AGG_THRESHOLD, VX_AGG_PATCH); return 0;}
'''
    (tmp_path / "s.c").write_text(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got == [ctypes.sizeof(_lib.AggItem), ctypes.sizeof(_lib.AggSpec), _lib.AggItem.H.offset, _lib.AggSpec.thr.offset,
                   _lib.VX_AGG_IMAGE, _lib.VX_AGG_THRESHOLD, _lib.VX_AGG_PATCH]


def test_plan_resolves_both_spellings_and_routes_foreign_targets():
    from values_amd import _lib
    from values_amd.aggregation import _plan, _specs_for
    ref = "evaluation.uncertainty_aggregation.aggregate_uncertainties."
    short = "uncertainty_aggregation.aggregate_uncertainties."
    aggs = {"a": {"_target_": ref + "patch_level_aggregation", "patch_size": 4},
            "b": {"_target_": A + "patch_level_aggregation", "patch_size": [2, 3], "mean": True},
            "c": {"_target_": short + "image_level_aggregation", "mean": True},
            "d": {"_target_": A + "threshold_aggregation", "threshold": 0.5},
            "e": {"_target_": ref + "threshold_aggregation", "threshold": 0.5, "mean": False},
            "f": {"_target_": "oracle.aggregation_oracle.image_level_aggregation"},
            "g": {"_target_": A + "patch_level_aggregation", "patch_size": 4, "mean": True, "_partial_": True}}
    plan = _plan(aggs, pred_model="Dropout", unc_type="aleatoric_uncertainty")
    assert [(n, k) for n, k, _ in plan] == [("a", "patch"), ("b", "patch"), ("c", "image"), ("d", "threshold"), ("e", "threshold"),
                                            ("f", "foreign"), ("g", "patch")]
    assert plan[5][2] == aggs["f"] and plan[3][2] == {"threshold": 0.5, "mean": True}
    # an int patch expands to the map's rank; equal device specs are shared (a, g; d, e)
    specs, index = _specs_for(plan, 2)
    P, I, T = _lib.VX_AGG_PATCH, _lib.VX_AGG_IMAGE, _lib.VX_AGG_THRESHOLD
    assert specs == [(P, 1, 4, 4, 0.0), (P, 1, 2, 3, 0.0), (I, 1, 1, 1, 0.0), (T, 1, 1, 1, 0.5)]
    assert index == [0, 1, 2, 3, 3, None, 0]
    specs3, _ = _specs_for([plan[0]], 3)
    assert specs3 == [(P, 4, 4, 4, 0.0)]
    with pytest.raises(ValueError):
        _specs_for(plan, 3)                 # the two-element patch of "b" on a 3D map
    with pytest.raises(ValueError):
        _specs_for([plan[0]], 4)


def test_threshold_file_is_opened_once_per_batch(tmp_path, monkeypatch):
    from values_amd.aggregation import _plan
    path = tmp_path / "thr.json"
    path.write_text(json.dumps({"Dropout": {"Mean aleatoric threshold": 0.125, "Mean epistemic threshold": 0.5}}))
    opened = []
    real = builtins.open
    monkeypatch.setattr(builtins, "open", lambda f, *a, **k: (opened.append(str(f)), real(f, *a, **k))[1])
    aggs = {"t": {"_target_": A + "threshold_aggregation", "threshold_path": str(path)},
            "t_sum": {"_target_": A + "threshold_aggregation", "threshold_path": str(path), "mean": False},
            "fixed": {"_target_": A + "threshold_aggregation", "threshold": 3}}
    plan = _plan(aggs, pred_model="Dropout", unc_type="aleatoric_uncertainty")
    assert opened.count(str(path)) == 1
    assert [p["threshold"] for _, _, p in plan] == [0.125, 0.125, 3] and [p["mean"] for _, _, p in plan] == [True, False, True]
    monkeypatch.undo()
    for kw, text in (({}, "prediction model"), ({"pred_model": "Dropout", "unc_type": None}, "prediction model")):
        with pytest.raises(Exception, match=text):
            _plan({"t": aggs["t"]}, **kw)
    with pytest.raises(Exception, match="A threshold needs to be provided"):
        _plan({"t": {"_target_": A + "threshold_aggregation"}})
    with pytest.raises(TypeError):
        _plan({"t": {"_target_": A + "threshold_aggregation", "threshold": 1, "patch_size": 3}})


def test_result_dicts_from_a_hand_written_out_array():
    from values_amd.aggregation import _assemble, _plan, _specs_for
    aggs = {"patch": {"_target_": A + "patch_level_aggregation", "patch_size": 2},
            "patch_mean": {"_target_": A + "patch_level_aggregation", "patch_size": 2, "mean": True},
            "sum": {"_target_": A + "image_level_aggregation"},
            "mean": {"_target_": A + "image_level_aggregation", "mean": True},
            "thr": {"_target_": A + "threshold_aggregation", "threshold": 7},
            "thr_sum": {"_target_": A + "threshold_aggregation", "threshold": 7, "mean": False},
            "other": {"_target_": "oracle.aggregation_oracle.image_level_aggregation"}}
    plan = _plan(aggs)
    for shape, box in (((4, 5, 6), [(1, 3), (2, 4), (3, 5)]), ((5, 6), [(2, 4), (3, 5)])):
        specs, index = _specs_for(plan, len(shape))
        assert len(specs) == 3
        rows = [[10.0, 1.0, 2.0, 3.0], [30.0, 0.0, 0.0, 0.0], [9.0, 4.0, 0.0, 0.0]]      # PATCH, IMAGE, THRESHOLD
        n = 120 if len(shape) == 3 else 30
        got = _assemble(plan, index, rows, shape)
        assert got == {"patch": {"max_score": 10.0, "bounding_box": box},
                       "patch_mean": {"max_score": 10.0 / 2 ** len(shape), "bounding_box": box},
                       "sum": {"max_score": 30.0}, "mean": 30.0 / n,
                       "thr": {"max_score": 2.25, "threshold": 7}, "thr_sum": {"max_score": 9.0, "threshold": 7}, "other": None}
        assert list(got) == list(aggs) and type(got["mean"]) is float
        assert all(type(v) is int for bb in got["patch"]["bounding_box"] for v in bb)
        rows[2] = [0.0, 0.0, 0.0, 0.0]                                                    # nothing at or above the threshold
        assert _assemble(plan, index, rows, shape)["thr"] == {"max_score": 0.0, "threshold": 7}


def test_workspace_query_and_refusals_need_no_device():
    from values_amd import _lib
    lib = _lib.load()
    assert lib.vx_version() >= 810
    item = lambda d, h, w: _lib.AggItem(0x1000, _lib.VX_F32, d, h, w)
    items = (_lib.AggItem * 2)(item(64, 64, 64), item(1, 1024, 512))
    sums = (_lib.AggSpec * 2)(_lib.AggSpec(_lib.VX_AGG_IMAGE, 1, 1, 1, 0.0), _lib.AggSpec(_lib.VX_AGG_THRESHOLD, 1, 1, 1, 0.5))
    patch = (_lib.AggSpec * 1)(_lib.AggSpec(_lib.VX_AGG_PATCH, 1, 10, 10, 0.0))
    small = lib.vx_aggregate_workspace_bytes(items, 2, sums, 2)
    assert 0 < small <= 1024
    # O(tiles): far below the 8 bytes per map element the stored box sums would take
    ws = lib.vx_aggregate_workspace_bytes(items, 2, patch, 1)
    assert small < ws < (64 ** 3 + 1024 * 512) * 8 // 100
    big = (_lib.AggSpec * 1)(_lib.AggSpec(_lib.VX_AGG_PATCH, 1, 600, 10, 0.0))
    assert lib.vx_aggregate_workspace_bytes(items, 2, big, 1) == 0                   # does not fit item 0
    assert lib.vx_aggregate_workspace_bytes(items, 0, sums, 2) == 0 and lib.vx_aggregate_workspace_bytes(items, 2, sums, 9) == 0
    out = ctypes.c_void_p(0x1000)
    assert lib.vx_aggregate_batched(items, 2, big, 1, out, out, 1 << 20, None) == -2
    assert b"item 0" in lib.vx_last_error_string()
    assert lib.vx_aggregate_batched(items, 2, sums, 9, out, out, 1 << 20, None) == -2
    assert lib.vx_aggregate_batched(items, 4097, sums, 2, out, out, 1 << 20, None) == -2
    assert lib.vx_aggregate_batched(items, 2, patch, 1, out, out, 16, None) == -4     # VX_E_WORKSPACE
    huge = (_lib.AggSpec * 1)(_lib.AggSpec(_lib.VX_AGG_PATCH, 1, 512, 512, 0.0))     # no LDS tile holds this halo
    assert lib.vx_aggregate_batched((_lib.AggItem * 1)(item(1, 1024, 512)), 1, huge, 1, out, out, 1 << 20, None) == -2


def test_restatement_matches_the_oracle_on_exact_inputs():
    """float32 values in [0, 1) widened to float64: every box sum is exact in any order, so the bounding boxes must be the
    oracle's exactly.  max_score and the sums within rel 1e-12: all summands are positive and no path has more than
    ceil(n / 1024) + 22 sequential adds, so either side's error is below 1e-14 relative for n <= 49210 (the largest map
    here); the float64 maps of the sums (m + 1e-9) are not exact, the bound covers them."""
    from oracle import aggregation_oracle as ao
    from tests import agg_restated as ar
    rng = np.random.default_rng(0)
    cases = [((7, 9, 11), 3), ((7, 9, 11), 5), ((5, 5, 5), 5), ((12, 10, 33), [5, 4, 10]), ((12, 10, 33), 10), ((19, 37, 70), 3),
             ((19, 37, 70), [5, 4, 10]), ((19, 37, 70), 10), ((13, 70), 10), ((13, 70), [3, 7]), ((13, 70), 1), ((6, 5), 1),
             ((150, 301), 10), ((150, 301), [3, 7])]
    for shape, patch in cases:
        m = rng.random(shape, dtype=np.float32)
        for mean in (False, True):
            got = ar.patch_level_aggregation(m, patch, mean)
            want = ao.patch_level_aggregation(m.astype(np.float64), patch, mean)
            assert got["bounding_box"] == [tuple(int(v) for v in bb) for bb in want["bounding_box"]], (shape, patch)
            assert got["max_score"] == pytest.approx(want["max_score"], rel=1e-12)
            assert all(type(v) is int for bb in got["bounding_box"] for v in bb) and type(got["max_score"]) is float
    for shape in ((1, 1), (8, 125), (32, 32), (25, 41), (11, 467), (19, 37, 70)):
        m32 = rng.random(shape, dtype=np.float32)
        for m in (m32, m32.astype(np.float64) + 1e-9):
            ref = m.astype(np.float64)
            assert ar.image_level_aggregation(m)["max_score"] == pytest.approx(ao.image_level_aggregation(ref)["max_score"], rel=1e-12)
            mean = ar.image_level_aggregation(m, mean=True)
            assert type(mean) is float and mean == pytest.approx(ao.image_level_aggregation(ref, mean=True), rel=1e-12)
            for thr, mn in ((0.5, True), (0.5, False), (2.0, True)):
                got, want = ar.threshold_aggregation(m, thr, mn), ao.threshold_aggregation(ref, threshold=thr, mean=mn)
                assert got["threshold"] == thr and got["max_score"] == pytest.approx(float(want["max_score"]), rel=1e-12)


def test_wide_range_inputs_see_the_order_of_the_adds():
    """the conditions the GPU tests rely on: with these maps a kernel that added in another order would not pass `==`"""
    from tests import agg_restated as ar
    ranks = set()
    for shape, patch, seed in ar.WIDE_BOX:
        m = ar.wide_range(shape, seed)
        patch = len(shape) * [patch] if type(patch) == int else patch
        up, down = ar.box_sums(m, patch), ar.box_sums(m, patch, descending=True)
        assert np.mean(up != down) > 0.25, (shape, float(np.mean(up != down)))
        assert ar.box_max(m, patch)[0] != ar.box_max(m, patch, descending=True)[0], shape
        ranks.add(len(shape))
    assert ranks == {2, 3}
    dtypes = set()
    for shape, dtype, seed, thr in ar.WIDE_SUMS:
        m = ar.wide_range(shape, seed, dtype)
        x = m.astype(np.float64)
        s, st, ct = ar.sums(m, thr)
        assert s != float(np.sum(x)) and st != float(np.sum(x[x >= thr])), shape
        assert ct == float(np.count_nonzero(x >= thr)) and 0 < ct < x.size
        dtypes.add(m.dtype)
    assert dtypes == {np.dtype(np.float32), np.dtype(np.float64)}


def test_threshold_is_resolved_before_any_device_call(tmp_path):
    """threshold_aggregation's two exceptions, in its order of checks (the file is opened before the names are asked for)"""
    from values_amd.aggregation import threshold_aggregation
    m = np.zeros((2, 2), np.float32)
    with pytest.raises(Exception, match="^A threshold needs to be provided for threshold aggregation!$") as e:
        threshold_aggregation(m)
    assert type(e.value) is Exception
    (tmp_path / "thr.json").write_text(json.dumps({"Dropout": {}}))
    with pytest.raises(Exception, match="^If you want to load the threshold from a json file, you have to provide the prediction "
                                        "model and the uncertainty type$") as e:
        threshold_aggregation(m, threshold_path=str(tmp_path / "thr.json"), pred_model="Dropout")
    assert type(e.value) is Exception
    with pytest.raises(FileNotFoundError):
        threshold_aggregation(m, threshold_path=str(tmp_path / "none.json"))
