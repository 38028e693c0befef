#!/usr/bin/env python3
"""One-time A/B for vx_convT_k2s2 (the sibling of tools/ab_routes.py and tools/ab_routes2d.py): are two builds of the library
bit-identical on the cases of tests/convT_route_cases.py?  Both are loaded RTLD_LOCAL into one process; every case runs base, base
again (is the case deterministic?), then new, on the same inputs.  Compared: kernel name, output tensor, range word.  Exit status 1
on any difference.

    python tools/ab_routesT.py [--base values_amd/libvalues_amd_base.so] [--new values_amd/libvalues_amd.so]

--refusals instead (a machine WITHOUT a GPU only: the base build has no dry run, so its vx_convT_k2s2 is called with dummy pointers
and an accepted call must end in the runtime's "no device" error): code and message of base vx_convT_k2s2 against new
vx_convT_k2s2_route over single fields and field pairs of a handful of layers under both configurations, and
vx_convT_k2s2_packed_floats over a grid of channels.
--launchtime instead: per-launch times of the forward's four up-convolutions (T = 10 samples of a 64^3 volume), alternating base /
new rounds in this process.  (Host time of a whole eager forward: tools/ab_routes.py --hosttime.)"""
import argparse, ctypes as C, itertools, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from tests import convT_route_cases as rc
from values_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--base", default=os.path.join(ROOT, "values_amd", "libvalues_amd_base.so"))
ap.add_argument("--new", default=os.path.join(ROOT, "values_amd", "libvalues_amd.so"))
ap.add_argument("--refusals", action="store_true")
ap.add_argument("--launchtime", action="store_true")
args = ap.parse_args()


def open_lib(path):
    lib = C.CDLL(path, mode=os.RTLD_LOCAL)
    for name, (res, at) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name); fn.restype = res; fn.argtypes = at
    return lib


libs = {"base": open_lib(args.base), "new": open_lib(args.new)}


def use(lib):
    _lib._lib = lib     # what _lib.config calls from here on


if args.refusals:
    assert not torch.cuda.is_available(), "--refusals calls the base build's vx_convT_k2s2 with dummy pointers: CPU machines only"
    big = 0x7fffffff
    mods = [("in_", None), ("w_packed", None), ("bias", None), ("out", None), ("N", 0), ("N", -1), ("N", 3), ("N", 1 << 20), ("D", 0),
            ("D", 1), ("D", 1 << 20), ("D", big), ("H", -7), ("H", 65536), ("H", big), ("W", 0), ("W", 1 << 30), ("W", 3), ("W", 65535), ("W", 65536), ("W", 1 << 20),
            ("Cin", 0), ("Cin", -8), ("Cin", 6), ("Cin", 12), ("Cin", 16), ("Cin", 32), ("Cin", 64), ("Cin", 128), ("Cin", 256),
            ("Cout", 0), ("Cout", -8), ("Cout", 4), ("Cout", 8), ("Cout", 24), ("Cout", 64), ("Cout", 136), ("Cout", 1 << 20),
            ("in_pitch", 0), ("in_pitch", 8), ("in_pitch", 130), ("in_pitch", 256), ("in_pitch", big - 3), ("out_pitch", 0),
            ("out_pitch", 18), ("out_pitch", 256), ("out_pitch", big - 3), ("out_coff", 4), ("out_coff", 2), ("out_coff", -4),
            ("out_coff", 1 << 20), ("out_coff", big - 3), ("out_xblk", 1), ("out_xblk", 2), ("out_xblk", 3), ("out_xblk", 4), ("out_xblk", -1), ("out_half", 1),
            ("out_half", 2), ("act", 1), ("act", 2), ("act", 7), ("drop_mode", 1), ("drop_mode", 2), ("drop_mode", 3),
            ("drop_mask", 0x50000), ("range_flag", None)]
    layers = [rc._case("ab", ci, co, vol) for ci, co, vol in ((16, 8, (2, 4, 4, 4)), (32, 16, (1, 3, 5, 7)), (64, 32, (2, 4, 4, 4)),
                                                             (128, 64, (2, 3, 5, 6)), (8, 8, (2, 2, 2, 2)), (16, 8, (1, 1, 1, 65536)))]
    # the refusals convT_route.h added where the base build's own arithmetic overflowed and it went on (DESIGN.md lists them)
    listed = (b"vx_convT_k2s2: N * 2 D must stay below 2^31", b"vx_convT_k2s2: sample too large",
              b"vx_convT_k2s2: pitches/offsets must be multiples of 4 floats")
    calls = refused = bad = new = 0
    for cfg in ({}, dict(conv_fp32=1)):
        for layer in layers:
            for i, j in itertools.combinations(range(-1, len(mods)), 2):
                res = []
                for which in ("base", "new"):
                    use(libs[which])
                    with _lib.config(**cfg):
                        a = rc.layer_args(layer, rc.dummy_ptr)
                        for k in (i, j):
                            if k >= 0:
                                setattr(a, *mods[k])
                        if which == "base":
                            code = libs[which].vx_convT_k2s2(C.byref(a), None)
                        else:
                            code = libs[which].vx_convT_k2s2_route(C.byref(a), None, 0, None)
                        res.append((code, libs[which].vx_last_error_string()) if code < 0 else (0, b""))   # (> 0: accepted, no device)
                calls += 1; refused += res[0][0] < 0
                # (the wrapped out_coff + Cout let the base build go on to its LATER checks: it may have refused with one of those)
                later = res[1][1] == listed[2] and res[0][1] in (b"vx_convT_k2s2: mask mode without mask", listed[1])
                if res[1][1] in listed and (res[0] == (0, b"") or later):
                    new += 1
                    continue
                bad += res[0] != res[1]
                if res[0] != res[1]:
                    print(cfg, layer["id"], mods[i] if i >= 0 else None, mods[j], res)
    chans = (-8, 0, 2, 4, 8, 12, 16, 24, 32, 64, 128, 136, 256, 1 << 20)
    q = [(ci, co) for ci in chans for co in chans if libs["base"].vx_convT_k2s2_packed_floats(ci, co) != libs["new"].vx_convT_k2s2_packed_floats(ci, co)]
    print(f"refusals: {calls} calls, {refused} refused by base, {new} refused by new alone with a listed message, {bad} differ otherwise "
          f"(code or message); packed size: {len(chans) ** 2} points, {len(q)} differ")
    sys.exit(1 if bad or q else 0)

if args.launchtime:
    dev, s, T = torch.device("cuda", 0), _lib.stream_ptr(), 10
    for name, cin, cout, e, act in (("center.4 128->64 4^3 relu", 128, 64, 4, _lib.VX_ACT_RELU), ("upscale4 64->32 8^3", 64, 32, 8, 0),
                                    ("upscale3 32->16 16^3", 32, 16, 16, 0), ("upscale2 16->8 32^3", 16, 8, 32, 0)):
        case = rc._case("time", cin, cout, (T, e, e, e), act=act)
        times, names = {"base": [], "new": []}, {}
        bufs = {w: rc.LayerBuffers(libs[w], case) for w in libs}
        for rnd in range(13):
            for which in (("base", "new") if rnd % 2 == 0 else ("new", "base")):
                lib, a = libs[which], rc.layer_args(case, bufs[which].ptr)
                _lib.check(lib.vx_convT_k2s2(C.byref(a), s), "convT")
                names[which] = lib.vx_last_kernel_name().decode()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(50):
                    lib.vx_convT_k2s2(C.byref(a), s)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[which].append(e0.elapsed_time(e1) / 50 * 1e3)
        for which in libs:
            t = times[which]
            print(f"{name:28s} {which:4s} {names[which]:36s} us per launch, 12 rounds of 50: " + " ".join(f"{v:.2f}" for v in t) +
                  f"  | median {statistics.median(t):.2f}  min {min(t):.2f}  max {max(t):.2f}", flush=True)
    sys.exit(0)

bad = nondet = 0
for case in rc.LAYER_CASES:
    res = []
    for which in ("base", "base", "new"):
        use(libs[which])
        with _lib.config(**case["cfg"]):
            buf = rc.LayerBuffers(libs[which], case)
            name = buf.launch()
        res.append((name, buf.out.view(torch.int32).clone(), buf.range.clone()))
    det = all(torch.equal(x, y) for x, y in zip(res[0][1:], res[1][1:]))
    eq = all(torch.equal(x, y) for x, y in zip(res[0][1:], res[2][1:])) and res[0][0] == res[2][0]
    nondet += not det; bad += not eq
    if not (det and eq):
        print(f"layer {case['id']:44s} {res[2][0]:40s} base==base {det}  base==new {eq}", flush=True)
print(f"{len(rc.LAYER_CASES)} layers: {nondet} differ base against base, {bad} differ base against new")
sys.exit(1 if bad else 0)
