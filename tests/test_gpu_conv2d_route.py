"""GPU: the kernel instance every vx_conv2d launch takes is the recorded one (tests/golden/conv2d_routes.json) -- whole HRNet
forwards in training and eval mode under every switch that moves a 2D launch, and single layers at the smallest shapes where the
tile and chunk geometry can go wrong, where the name after the real launch must also be the dry run's."""
import json
import os

import pytest

from tests import conv2d_route_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", rc.GOLDEN)))


@pytest.mark.parametrize("case", rc.FORWARD_CASES, ids=[c[0] for c in rc.FORWARD_CASES])
def test_forward_launches_the_recorded_kernels(case, golden, vxcfg):
    cid, mode, cfg = case
    vxcfg.set(conv_fp32=0, c2s_no_wide=0, c2s_no_oct=0)
    vxcfg.set(**cfg)
    names, _ = rc.forward_run(rc.forward_model(mode), rc.forward_input())
    assert names == golden["forward"][cid]


@pytest.mark.parametrize("group", sorted({c["id"].rsplit(":", 3)[0] for c in rc.LAYER_CASES}))
def test_layer_launch_takes_the_route_the_dry_run_names(group, golden, vxcfg):
    """group = configuration and kernel size / stride"""
    from values_amd import _lib
    lib = _lib.load()
    for case in (c for c in rc.LAYER_CASES if c["id"].rsplit(":", 3)[0] == group):
        vxcfg.set(conv_fp32=0, c2s_no_wide=0, c2s_no_oct=0)
        vxcfg.set(**case["cfg"])
        buf = rc.LayerBuffers(lib, case)
        code, dry, geo, _ = rc.dry_run(lib, rc.layer_args(lib, case, buf.ptr))
        assert code == 0, (case["id"], lib.vx_last_error_string())
        assert [dry] + list(geo) == golden["layers"][case["id"]] and buf.launch() == dry, case["id"]
