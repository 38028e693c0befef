#!/usr/bin/env python3
"""Records tests/golden/conv2d_routes.json: which kernel instance every vx_conv2d launch of the cases in tests/conv2d_route_cases.py
takes, and with what launch geometry.  Run once on the GPU against the build whose routing is the reference:

    VX_LIB_PATH=values_amd/libvalues_amd_base.so python tools/gen_conv2d_routes.py [out.json]

(a) "forward": the kernel names of one HighResolutionNet forward per forward case, in launch order; (b) "layers": per single-layer
case the kernel name after a real launch with correctly sized buffers, plus nchunks / w_all / grid_x / grid_y.

The reference build (the parent of the commit that introduced conv2d_route.h) reports the instance name only.  Its launch geometry
is restated here from its launchers (conv2d_s16.hip: vx_conv2d_s16 and launch_c2s; conv2d_mfma.hip: vx_conv2d and launch_c2) -- the
restatement tests/test_gpu_ops2d.py carried as c2s_lds / c2s_workgroups until the library grew its dry run, extended by the
epilogue table of the EPI instances and by the fp32 launcher.  It is used at recording time only; the tests compare the recorded
numbers with vx_conv2d_route."""
import json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from tests import conv2d_route_cases as rc
from values_amd import _lib

LDS = 160 * 1024


def restated_geometry(name, cin_pad, cout, total_tiles):
    """(nchunks, w_all, grid_x, grid_y) the parent's launchers derive for the instance `name`"""
    fam, par = re.fullmatch(r"conv2d_(s16|mfma)_kernel<([\d,]+)>", name).groups()
    p = [int(v) for v in par.split(",")]
    ks, s, nt, nsub = p[:4]
    hx = hy = 15 * s + ks
    npp = -(-hx // s) * -(-hy // s)
    plane = rc.r16(s * s * npp)
    if fam == "s16":
        oct_, epi = p[5], len(p) == 7
        nchunks = 1 if oct_ or (ks == 3 and nsub > 1) else -(-(cin_pad // 16) // nsub)
        img_h = (oct_ or 2 * nsub) * plane * 8
        nstep = ((9 * oct_ + 3) // 4 if oct_ else 5 * nsub) if ks == 3 else nsub // 2
        tabc = rc.r16(oct_ * 8) if oct_ else nsub * 16
        wch = nstep * nt * 2 * 64 * 8 * 2
        rest = img_h * 4 + 8 * nt * 16 * 2 * 4 + 2 * tabc * 4 + (2 * nt * 16 * 4 if epi else 0)
        w_all = int(nchunks > 1 and rest + nchunks * wch <= LDS)
        lds, cap = rest + (nchunks if w_all else 1) * wch, 2
    else:
        nchunks, w_all = -(-(cin_pad // 16) // nsub), 0
        lds, cap = (nsub * 4 * plane * 4 + nsub * ks * ks * nt * 64 * 4 + 8 * nt * 16 * 2) * 4, 4
    per_cu = min(cap, max(1, LDS // lds))
    ygroups = -(-cout // (16 * nt))
    return nchunks, w_all, min(-(-256 * per_cu // ygroups), total_tiles), ygroups


if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", rc.GOLDEN)
    lib = _lib.load()
    golden = {"library": os.path.basename(_lib.LIB_PATH), "version": lib.vx_version(),
              "provenance": "names: vx_last_kernel_name() after real launches of this library; nchunks / w_all / grid_x / grid_y: "
                            "tools/gen_conv2d_routes.py restated_geometry (this library has no dry run)",
              "forward": {}, "layers": {}}
    for cid, mode, cfg in rc.FORWARD_CASES:
        with _lib.config(**cfg):
            golden["forward"][cid] = rc.forward_run(rc.forward_model(mode), rc.forward_input())[0]
        print(cid, len(golden["forward"][cid]), flush=True)
    for case in rc.LAYER_CASES:
        with _lib.config(**case["cfg"]):
            name = rc.LayerBuffers(lib, case).launch()
            tiles = rc.LAYER_N * lib.vx_conv2d_tiles(case["h"], case["w"], case["ks"], case["s"])
        golden["layers"][case["id"]] = [name] + list(restated_geometry(name, rc.r16(case["cin"]), case["cout"], tiles))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:          # one line per case
        rows = lambda d: "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(d[k])}" for k in sorted(d)) + "\n}"
        head = ",\n".join(f"{json.dumps(k)}: {json.dumps(golden[k])}" for k in ("library", "provenance", "version"))
        f.write("{\n%s,\n\"forward\": %s,\n\"layers\": %s\n}\n" % (head, rows(golden["forward"]), rows(golden["layers"])))
    print("wrote", out_path, len(golden["forward"]), "forwards", len(golden["layers"]), "layers,",
          len({v[0] for v in golden["layers"].values()}), "instances")
