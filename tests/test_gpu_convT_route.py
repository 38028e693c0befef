"""GPU: the kernel every vx_convT_k2s2 launch takes is the recorded one (tests/golden/convT_routes.json) -- single launches into
correctly sized buffers at the smallest shapes where each rule of the route can go wrong; the name after the real launch must be the
dry run's and the golden's, the dry run's grid the golden's.  Only valid cases are launched: refused arguments are exercised through
the dry run and the host program (tests/test_convT_route_cpu.py)."""
import json
import os

import pytest

from tests import convT_route_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", rc.GOLDEN)))


@pytest.mark.parametrize("group", rc.GROUPS)
def test_launch_takes_the_route_the_dry_run_names(group, golden, vxcfg):
    from values_amd import _lib
    lib = _lib.load()
    for case in (c for c in rc.LAYER_CASES if c["id"].split(":")[0] == group):
        vxcfg.set(conv_fp32=0)
        vxcfg.set(**case["cfg"])
        buf = rc.LayerBuffers(lib, case)
        code, dry, gx, gy = rc.dry_run(lib, rc.layer_args(case, buf.ptr))
        assert code == 0, (case["id"], lib.vx_last_error_string())
        assert [dry, gx, gy] == golden["layers"][case["id"]] and buf.launch() == dry, case["id"]
