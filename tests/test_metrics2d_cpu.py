"""CPU: the 2D metrics.json writer (Tester.save_results_dict, test_2D.py:258-271), read back by values_amd.evalmetrics, and
the binding of vx_mask_agreement_batched."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RESULTS = {
    "frankfurt_000000_000294": {"dataset": "cityscapes", "metrics": {"dice": 0.5, "ged": 0.25}},
    "frankfurt_000000_000576": {"dataset": "cityscapes", "metrics": {"dice": 0.75, "ged": 0.5}},
    "00042": {"dataset": "gta", "metrics": {"dice": 1.0, "ged": 0.0}},
}


def test_save_results_dict_writes_the_reference_layout(tmp_path):
    from values_amd.results2d import save_results_dict
    given = json.loads(json.dumps(RESULTS))
    full = save_results_dict(str(tmp_path), given)
    want = {
        "frankfurt_000000_000294": {"dataset": "cityscapes", "metrics": {"dice": 0.5, "ged": 0.25}},
        "frankfurt_000000_000576": {"dataset": "cityscapes", "metrics": {"dice": 0.75, "ged": 0.5}},
        "00042": {"dataset": "gta", "metrics": {"dice": 1.0, "ged": 0.0}},
        "mean": {"metrics": {"dice": 0.75, "ged": 0.25}},
    }
    text = (tmp_path / "metrics.json").read_text()
    assert json.loads(text) == want and full == want
    assert list(json.loads(text)) == list(want)                   # images in the order given, "mean" last
    assert text == json.dumps(want, indent=2)                     # indent=2, as json.dump(self.results_dict, f, indent=2)
    assert given == RESULTS                                       # the caller's dict is not touched


def test_save_results_dict_round_trip_through_evalmetrics(tmp_path):
    from values_amd import evalmetrics
    from values_amd.results2d import save_results_dict
    save_results_dict(str(tmp_path / "val"), RESULTS)
    f = tmp_path / "val" / "metrics.json"
    for iid, e in RESULTS.items():
        assert evalmetrics.get_dice(iid, f) == e["metrics"]["dice"]
        assert evalmetrics.get_risk(iid, f) == 1 - e["metrics"]["dice"]
    # the `path/id.ext` style keys _metric_entry resolves: a tree whose metrics were keyed by file name
    keyed = {f"leftImg8bit/val/{iid}.png": e for iid, e in RESULTS.items()}
    save_results_dict(str(tmp_path / "keyed"), keyed)
    f = tmp_path / "keyed" / "metrics.json"
    for iid, e in RESULTS.items():
        assert evalmetrics.get_dice(iid, f) == e["metrics"]["dice"]
        assert evalmetrics.get_risk(iid, f) == 1 - e["metrics"]["dice"]


def test_save_results_dict_without_images(tmp_path):
    from values_amd.results2d import save_results_dict
    assert save_results_dict(str(tmp_path), {}) == {"mean": {"metrics": {}}}
    assert json.loads((tmp_path / "metrics.json").read_text()) == {"mean": {"metrics": {}}}


def test_mask_agreement_batched_is_bound():
    """one argtype per parameter of the header's prototype: masks, B, M, C, nvox, remap_from, counts, stream"""
    from values_amd import _lib
    res, args = _lib.SIGNATURES["vx_mask_agreement_batched"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                    ctypes.c_void_p]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "values_amd.h")).read(), flags=re.S)
    proto = re.search(r"\bint\s+vx_mask_agreement_batched\s*\(([^)]*)\)\s*;", src)
    assert proto and len(proto.group(1).split(",")) == len(args)
    # the one-image entry point is as it was
    assert _lib.SIGNATURES["vx_mask_agreement"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                                   ctypes.c_void_p, ctypes.c_void_p])


def test_mask_agreement_batched_refuses_bad_arguments_without_a_gpu():
    """argument errors come back before anything touches a device (the pointers are never dereferenced)"""
    from values_amd import _lib
    lib = _lib.load()
    assert lib.vx_version() >= 740
    dummy = 0x10000
    for B, M, C, nvox in ((0, 2, 2, 64), (1, 33, 2, 64), (1, 0, 2, 64), (1, 2, 33, 64), (1, 2, 0, 64), (1, 2, 2, -1),
                          (1, 2, 2, (1 << 39) + 1)):
        assert lib.vx_mask_agreement_batched(dummy, B, M, C, nvox, -1, dummy, None) == -2, (B, M, C, nvox)   # VX_E_SHAPE
        assert lib.vx_last_error_string().decode().startswith("vx_mask_agreement_batched:")
    assert lib.vx_mask_agreement_batched(dummy, 1, 2, 2, 64, -1, None, None) == -1                           # VX_E_NULL
    assert "vx_mask_agreement_batched" in lib.vx_last_error_string().decode()
