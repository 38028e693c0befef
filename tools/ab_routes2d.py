#!/usr/bin/env python3
"""One-time A/B for the 2D path (the sibling of tools/ab_routes.py): are two builds of the library bit-identical on the cases of
tests/conv2d_route_cases.py?  Both are loaded RTLD_LOCAL into one process; every case runs base, base again (is the case
deterministic?), then new, on the same inputs.  Compared: single layers -- kernel name, output tensor, statistics partials;
forwards -- kernel names and logits.  Exit status 1 on any difference.

    python tools/ab_routes2d.py [--base values_amd/libvalues_amd_base.so] [--new values_amd/libvalues_amd.so]

--queries instead (no GPU): vx_conv2d_family, vx_conv2d_packed_floats and vx_conv2d_tiles of the two builds over a grid of
(Cin, Cout, KS, S, H, W, configuration).
--refusals instead (a machine WITHOUT a GPU only: the base build has no dry run, so its vx_conv2d is called with dummy pointers and an
accepted call must end in the runtime's "no device" error): code and message of base vx_conv2d against new vx_conv2d_route over
single fields and field pairs of a handful of layers under every configuration.
--hosttime instead: the host time of one eager (uncaptured) forward of the `small` HRNet -- the call that issues every launch,
returning before the GPU has finished; the GPU idle at its start -- alternating base / new rounds of 20 calls in this process."""
import argparse, ctypes as C, itertools, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from tests import conv2d_route_cases as rc
from values_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--base", default=os.path.join(ROOT, "values_amd", "libvalues_amd_base.so"))
ap.add_argument("--new", default=os.path.join(ROOT, "values_amd", "libvalues_amd.so"))
ap.add_argument("--hosttime", action="store_true")
ap.add_argument("--queries", action="store_true")
ap.add_argument("--refusals", action="store_true")
args = ap.parse_args()


def open_lib(path):
    lib = C.CDLL(path, mode=os.RTLD_LOCAL)
    for name, (res, at) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name); fn.restype = res; fn.argtypes = at
    return lib


libs = {"base": open_lib(args.base), "new": open_lib(args.new)}


def use(lib):
    _lib._lib = lib     # what values_amd's own code (models, _lib.config) calls from here on


def same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


if args.queries:
    chans = (-8, 0, 1, 3, 8, 9, 16, 17, 18, 24, 25, 32, 36, 48, 64, 72, 80, 144, 256, 270, 720, 1 << 20)
    dims = (-7, 0, 1, 5, 7, 15, 16, 17, 31, 32, 33, 112, 256, 478, 1024, 1 << 20)
    points = bad = 0
    for cfg in ({}, dict(conv_fp32=1), dict(conv_fp32=2), dict(c2s_no_wide=1), dict(c2s_no_oct=1), dict(c2s_no_wide=1, c2s_no_oct=1)):
        got = {}
        for which in libs:
            use(libs[which])
            with _lib.config(**cfg):
                lib = libs[which]
                got[which] = [(lib.vx_conv2d_family(ci, co, ks), lib.vx_conv2d_packed_floats(ci, co, ks))
                              for ci, co, ks in itertools.product(chans, chans, (-1, 0, 1, 2, 3, 5))]
                got[which] += [lib.vx_conv2d_tiles(h, w, ks, s) for h, w, ks, s in itertools.product(dims, dims, (1, 3), (1, 2, 3, -1))]
        points += len(got["base"])
        bad += sum(x != y for x, y in zip(got["base"], got["new"]))
    print(f"host queries: {points} points, {bad} differ base against new")
    sys.exit(1 if bad else 0)

if args.refusals:
    assert not torch.cuda.is_available(), "--refusals calls the base build's vx_conv2d with dummy pointers: CPU machines only"
    mods = [("in_", None), ("w_packed", None), ("out", None), ("bias", None), ("bias", 0x30004), ("in_", 0x10004), ("out", 0x40008),
            ("w_packed", 0x2000c), ("N", 0), ("N", -1), ("H", 0), ("W", -1), ("H", 1 << 14), ("W", 1 << 16), ("Cin", 0), ("Cin", 12),
            ("Cin", 16), ("Cin", 32), ("Cin", 48), ("Cout", -8), ("Cout", 0), ("Cout", 20), ("KS", 5), ("KS", 1), ("KS", 3), ("S", 2),
            ("S", 3), ("S", 0), ("w_family", 0), ("w_family", 3), ("w_family", 11), ("w_family", 111), ("w_family", 211), ("w_family", 311),
            ("w_family", 312), ("w_family", 15), ("w_family", -112), ("in_pitch", 0), ("in_pitch", 4), ("in_pitch", 16), ("in_pitch", 20),
            ("in_pitch", 22), ("in_pitch", 1 << 20), ("out_pitch", 12), ("out_pitch", 18), ("out_pitch", 1 << 22), ("out_coff", 4),
            ("out_coff", 2), ("out_coff", -4), ("in_scale", 0x90000), ("in_shift", 0xa0000), ("in_cpitch", 16), ("in_cpitch", 17),
            ("in_cpitch", 1), ("in_cpitch", 1000), ("in_group_images", -1), ("in_group_images", 3), ("out_scale", 0x60000), ("out_scale", None),
            ("out_shift", 0x70000), ("out_shift", None), ("stats_partial", None), ("stats_partial", 0x50000), ("out_add", 0x80000),
            ("out_add", 0x80004), ("out_add", None), ("out_add_pitch", 12), ("out_add_pitch", 18), ("out_add_pitch", 1 << 22),
            ("out_add_pitch", 64), ("out_act", 0), ("out_act", 1), ("out_act", 2), ("out_act", -1)]
    layers = [dict(ks=3, s=1, h=16, w=16, cin=32, cout=16, epi=0), dict(ks=3, s=1, h=16, w=16, cin=32, cout=16, epi=1),
              dict(ks=3, s=2, h=17, w=31, cin=18, cout=36, epi=0), dict(ks=3, s=1, h=20, w=33, cin=3, cout=64, epi=1),
              dict(ks=1, s=1, h=9, w=21, cin=256, cout=72, epi=0), dict(ks=1, s=1, h=9, w=21, cin=720, cout=48, epi=1)]
    calls = refused = bad = 0
    for cfg in ({}, dict(conv_fp32=1), dict(c2s_no_wide=1), dict(c2s_no_oct=1)):
        for layer in layers:
            for i, j in itertools.combinations(range(-1, len(mods)), 2):
                res = []
                for which in ("base", "new"):
                    use(libs[which])
                    with _lib.config(**cfg):
                        a = rc.layer_args(libs[which], layer, rc.dummy_ptr)
                        for k in (i, j):
                            if k >= 0:
                                setattr(a, *mods[k])
                        if which == "base":
                            code = libs[which].vx_conv2d(C.byref(a), None)
                        else:
                            code = libs[which].vx_conv2d_route(C.byref(a), None, 0, None)
                        res.append((code, libs[which].vx_last_error_string()) if code < 0 else (0, b""))   # (> 0: accepted, no device)
                calls += 1; refused += res[0][0] < 0; bad += res[0] != res[1]
                if res[0] != res[1] and bad <= 10:
                    print(cfg, layer, mods[i] if i >= 0 else None, mods[j], res)
    print(f"refusals: {calls} calls, {refused} refused by base, {bad} differ base against new (code or message)")
    sys.exit(1 if bad else 0)

if args.hosttime:
    import statistics, time
    models, med = {}, {"base": [], "new": []}
    for which in libs:
        use(libs[which])
        models[which] = rc.forward_model("train")
    x = rc.forward_input()
    for which in libs:
        use(libs[which])
        for i in range(5):
            models[which](x)
        torch.cuda.synchronize()
    for rnd in range(12):
        for which in (("base", "new") if rnd % 2 == 0 else ("new", "base")):
            use(libs[which])
            ts = []
            for i in range(20):
                t0 = time.perf_counter()
                models[which](x)
                ts.append((time.perf_counter() - t0) * 1e6)
                torch.cuda.synchronize()
            med[which].append(statistics.median(ts))
    for which in libs:
        print(f"{which}: host time per eager small-HRNet forward (2 x 3 x 64 x 96), median of 20 calls per round, us: " +
              " ".join(f"{t:.1f}" for t in med[which]) + f"  | median {statistics.median(med[which]):.1f}  min {min(med[which]):.1f}  max {max(med[which]):.1f}")
    sys.exit(0)

bad = nondet = 0
for case in rc.LAYER_CASES:
    res = []
    for which in ("base", "base", "new"):
        use(libs[which])
        with _lib.config(**case["cfg"]):
            buf = rc.LayerBuffers(libs[which], case)
            name = buf.launch()
        res.append((name, (buf.out.clone(), buf.stats.clone())))
    det = same(res[0][1], res[1][1]); eq = same(res[0][1], res[2][1]) and res[0][0] == res[2][0]
    nondet += not det; bad += not eq
    if not (det and eq):
        print(f"layer {case['id']:44s} {res[2][0]:40s} base==base {det}  base==new {eq}", flush=True)
for cid, mode, cfg in rc.FORWARD_CASES:
    res = []
    for which in ("base", "base", "new"):
        use(libs[which])
        with _lib.config(**cfg):
            names, y = rc.forward_run(rc.forward_model(mode), rc.forward_input())
        res.append((names, [y.clone()]))
    det = same(res[0][1], res[1][1]); eq = same(res[0][1], res[2][1]) and res[0][0] == res[2][0]
    nondet += not det; bad += not eq
    print(f"forward {cid:20s} {len(res[2][0])} launches  base==base {det}  base==new {eq}", flush=True)
print(f"{len(rc.LAYER_CASES)} layers, {len(rc.FORWARD_CASES)} forwards: {nondet} differ base against base, {bad} differ base against new")
sys.exit(1 if bad else 0)
