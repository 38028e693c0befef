"""CPU: the host half of aggregation.aggregate_batch: the ABI structs against the C header, spec building from aggregation
configs, result-dict assembly from a hand-written device array.  No device call."""
import builtins
import ctypes
import json
import os
import subprocess

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
