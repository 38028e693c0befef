#!/usr/bin/env python3
"""Records tests/golden/convT_routes.json: which kernel every vx_convT_k2s2 launch of the cases in tests/convT_route_cases.py takes,
and with what grid.  Run once on the GPU against the build whose routing is the reference:

    VX_LIB_PATH=values_amd/libvalues_amd_base.so python tools/gen_convT_routes.py [out.json]

Per case: the kernel name after a real launch with correctly sized buffers, plus grid_x / grid_y.

The reference build (the parent of the commit that introduced convT_route.h) reports the name only.  Its grid is restated here from
its launchers (convtranspose.hip: launch_convT_mfma, launch_convT_s16 and the two launches at the end of vx_convT_k2s2).  The
restatement is used at recording time only; the tests compare the recorded numbers with vx_convT_k2s2_route.

Cases added after the route had its dry run are recorded without a GPU:

    python tools/gen_convT_routes.py --add [golden.json]

keeps every entry of the file as it is and adds the cases it lacks from vx_convT_k2s2_route of the current library (names and
grids; the restated grid must agree).  tests/test_gpu_convT_route.py and tests/test_gpu_convT_matrix.py then hold the real launches
to those names."""
import json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from tests import convT_route_cases as rc
from values_amd import _lib


def restated_grid(name, case):
    """(grid_x, grid_y) the parent's launchers derive for the kernel `name`"""
    n, d, h, w = case["vol"]
    nvox, cout = n * d * h * w, case["cout"]
    m = re.fullmatch(r"convT_k2s2_(mfma|s16)_kernel<(\d+),(\d+),(true|false)>", name)
    if m:
        groups = (cout // 2) // int(m.group(3))
        cap = -(-(512 if m.group(1) == "s16" else 256 * 32) // groups)
        return min(-(-(-(-nvox // 16)) // 4), cap), groups
    if name == "convT_k2s2_rows_kernel":
        return min(-(-(n * d * h * (2 * w) * (cout // 4)) // 256), 4096), 4
    assert name == "convT_k2s2_kernel", name
    return min(-(-nvox // 256), 8192), 4 * (cout // 8)


def write(golden, out_path):
    with open(out_path, "w") as f:          # one line per case
        d = golden["layers"]
        head = ",\n".join(f"{json.dumps(k)}: {json.dumps(golden[k])}" for k in sorted(golden) if k != "layers")
        f.write("{\n%s,\n\"layers\": {\n%s\n}\n}\n" % (head, ",\n".join(f"{json.dumps(k)}: {json.dumps(d[k])}" for k in sorted(d))))
    print("wrote", out_path, len(d), "layers,", len({v[0] for v in d.values()}), "kernels")


def add_dry(path):
    lib = _lib.load()
    golden = json.load(open(path))
    added = []
    for case in rc.LAYER_CASES:
        if case["id"] in golden["layers"]:
            continue
        with _lib.config(conv_fp32=0, **case["cfg"]):
            code, name, gx, gy = rc.dry_run(lib, rc.layer_args(case, rc.dummy_ptr))
        assert code == 0 and (gx, gy) == restated_grid(name, case), (case["id"], code, name, gx, gy)
        golden["layers"][case["id"]] = [name, gx, gy]
        added.append(case["id"])
    golden["provenance_added"] = ("groups bound, rowsnd, stride: names and grids from vx_convT_k2s2_route (dry run, version %d), equal to "
                                  "restated_grid; real launches are held to them by tests/test_gpu_convT_route.py" % lib.vx_version())
    write(golden, path)
    print("added", len(added))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--add":
        add_dry(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", rc.GOLDEN))
        sys.exit(0)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", rc.GOLDEN)
    lib = _lib.load()
    golden = {"library": os.path.basename(_lib.LIB_PATH), "version": lib.vx_version(),
              "provenance": "names: vx_last_kernel_name() after real launches of this library; grid_x / grid_y: "
                            "tools/gen_convT_routes.py restated_grid (this library has no dry run)",
              "layers": {}}
    for case in rc.LAYER_CASES:
        with _lib.config(**case["cfg"]):
            name = rc.LayerBuffers(lib, case).launch()
        golden["layers"][case["id"]] = [name] + list(restated_grid(name, case))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    write(golden, out_path)
