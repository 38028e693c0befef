"""GPU: the kernel instance every 3x3x3 launch takes is the recorded one (tests/golden/conv3d_routes.json) -- whole forwards under
every data-flow switch, and single layers at the smallest shapes where each family's geometry can go wrong, where the name after
the real launch must also be the dry run's."""
import json
import os

import pytest

from tests import conv3d_route_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", rc.GOLDEN)))


@pytest.mark.parametrize("case", rc.FORWARD_CASES, ids=[c[0] for c in rc.FORWARD_CASES])
def test_forward_launches_the_recorded_kernels(case, golden, vxcfg):
    cid, shape, kw, cfg = case
    vxcfg.set(**cfg)
    rows = rc.forward_rows(rc.forward_model(kw), rc.forward_input(shape))
    assert rows == golden["forward"][cid]


@pytest.mark.parametrize("family", sorted({c["id"].split(":")[0] for c in rc.LAYER_CASES}))
def test_layer_launch_takes_the_route_the_dry_run_names(family, golden, vxcfg):
    from values_amd import _lib
    lib = _lib.load()
    for case in (c for c in rc.LAYER_CASES if c["id"].startswith(family + ":")):
        vxcfg.set(conv_fp32=case["cfg"].get("conv_fp32", 0))
        buf = rc.LayerBuffers(lib, case)
        code, dry = rc.dry_run(lib, rc.layer_args(lib, case, buf.ptr))
        assert code == 0, (case["id"], lib.vx_last_error_string())
        assert buf.launch() == dry == golden["layers"][case["id"]], case["id"]
