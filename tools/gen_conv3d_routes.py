#!/usr/bin/env python3
"""Records tests/golden/conv3d_routes.json: which kernel instance every 3x3x3 launch of the cases in tests/conv3d_route_cases.py
takes.  Run once on the GPU against the build whose routing is the reference:

    VX_LIB_PATH=values_amd/libvalues_amd_base.so python tools/gen_conv3d_routes.py [out.json]

(a) "forward": the label|kernel list of bench.profiled_forward per forward case; (b) "layers": the kernel name after a real
launch with correctly sized buffers per single-layer case."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from tests import conv3d_route_cases as rc
from values_amd import _lib

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", rc.GOLDEN)
lib = _lib.load()
golden = {"library": os.path.basename(_lib.LIB_PATH), "version": lib.vx_version(), "forward": {}, "layers": {}}
for cid, shape, kw, cfg in rc.FORWARD_CASES:
    with _lib.config(**cfg):
        golden["forward"][cid] = rc.forward_rows(rc.forward_model(kw), rc.forward_input(shape))
    print(cid, len(golden["forward"][cid]), flush=True)
for case in rc.LAYER_CASES:
    with _lib.config(**case["cfg"]):
        golden["layers"][case["id"]] = rc.LayerBuffers(lib, case).launch()
    print(case["id"], golden["layers"][case["id"]], flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
json.dump(golden, open(out_path, "w"), indent=0, sort_keys=True)
print("wrote", out_path, len(golden["forward"]), "forwards", len(golden["layers"]), "layers")
