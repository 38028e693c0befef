#!/usr/bin/env python3
"""One-time A/B: are two builds of the library bit-identical on the cases of tests/conv3d_route_cases.py?  Both are loaded
RTLD_LOCAL into one process (as tools/ab_layers.py); every case runs base, base again (is the case deterministic?), then new,
on the same inputs.  Compared: single layers -- output tensor, statistics partials, range flag; forwards -- logits and the
uncertainty maps of predict_uncertainty.  Exit status 1 on any difference.

    python tools/ab_routes.py [--base values_amd/libvalues_amd_base.so] [--new values_amd/libvalues_amd.so]

--hosttime instead: the host time of one eager (uncaptured) T = 10 forward at 64^3 -- the call that issues every launch, returning
before the GPU has finished; the GPU idle at its start -- alternating base / new rounds of 20 calls in this one process.
--stream3d-refusals instead (a machine WITHOUT a GPU only: the entry points are called with dummy pointers and an accepted call must
end in the runtime's "no device" error): code and message of the ten entry points of norm_apply.hip, base against new, over single
fields and field pairs of a handful of layers and over grids of the small passes' arguments.  They must be equal except for the
refusals values_amd/csrc/stream3d_route.h added where the base build's own arithmetic wrapped, each of which is
checked against the wrap it closes; the new build's dry run must agree with its entry point."""
import argparse, ctypes as C, itertools, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from tests import conv3d_route_cases as rc
from values_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--base", default=os.path.join(ROOT, "values_amd", "libvalues_amd_base.so"))
ap.add_argument("--new", default=os.path.join(ROOT, "values_amd", "libvalues_amd.so"))
ap.add_argument("--hosttime", action="store_true")
ap.add_argument("--stream3d-refusals", action="store_true")
args = ap.parse_args()


def open_lib(path):
    lib = C.CDLL(path, mode=os.RTLD_LOCAL)
    for name, (res, at) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name); fn.restype = res; fn.argtypes = at
    return lib


libs = {"base": open_lib(args.base), "new": open_lib(args.new)}


def use(lib):
    _lib._lib = lib     # what values_amd's own code (models, predict_uncertainty, _lib.config) calls from here on


def same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


if args.stream3d_refusals:
    assert not torch.cuda.is_available(), "--stream3d-refusals calls launching entry points with dummy pointers: CPU machines only"
    big, P = 0x7fffffff, 0x10000
    calls = refused = bad = new = 0

    def result(lib, code):
        return (code, lib.vx_last_error_string()) if code < 0 else (0, b"")      # (> 0: accepted, no device)

    def compare(what, call, wrapped):
        """call(lib) -> code, on both builds; wrapped: {message prefix of a listed refusal: did the base build's arithmetic wrap here?}"""
        global calls, refused, bad, new
        res = [result(libs[w], call(libs[w])) for w in ("base", "new")]
        calls += 1; refused += res[0][0] < 0
        if res[0] == res[1]:
            return
        hit = [k for k in wrapped if res[1][1].startswith(k)]
        if hit and wrapped[hit[0]]:
            new += 1
            return
        bad += 1
        print(what, res)

    # ---- vx_norm_act_drop_pool, _bcast, _stats ----
    mods = [("x", None), ("out", None), ("pool_out", None), ("pool_out", 0x50000), ("mean", None), ("rstd", None), ("N", 0), ("N", -1), ("N", 4), ("N", 65535),
            ("N", 65536), ("N", 131070), ("N", 1 << 20), ("N", big), ("D", 0), ("D", 1), ("D", 3), ("D", 1 << 16), ("D", 1 << 20), ("D", big), ("H", -7), ("H", 5),
            ("H", 65536), ("H", big), ("W", 0), ("W", 3), ("W", 65536), ("W", 1 << 27), ("W", 1 << 28), ("W", big - 1), ("C", 0), ("C", -4), ("C", 6), ("C", 4),
            ("C", 12), ("C", 132), ("C", 516), ("C", big - 3), ("x_pitch", 0), ("x_pitch", 10), ("x_pitch", 1 << 20), ("x_pitch", big - 3), ("out_pitch", 0),
            ("out_pitch", 10), ("out_pitch", 1 << 20), ("out_pitch", big - 3), ("out_coff", 2), ("out_coff", 4), ("out_coff", -4), ("out_coff", big - 3),
            ("out_coff", -(1 << 31)), ("pool_pitch", 0), ("pool_pitch", 6), ("pool_pitch", 1 << 20), ("pool_pitch", big - 3), ("out_xblk", 1), ("out_xblk", 2),
            ("out_xblk", 3), ("out_xblk", 4), ("out_xblk", -1), ("out_half", 1), ("out_half", 2), ("x_xblk", 1), ("x_xblk", 2), ("x_xblk", 3), ("x_xblk", 4),
            ("x_half", 1), ("x_half", 2), ("act", 2), ("act", 7), ("drop_mode", 1), ("drop_mode", 2), ("drop_mask", 0x80000), ("range_flag", 0x60000)]
    layers = [(2, 4, 4, 4, 8, 0), (2, 4, 4, 4, 8, 1), (3, 3, 5, 7, 12, 0), (2, 2, 6, 10, 128, 1), (2, 2, 2, 4, 256, 1), (6, 1, 1, 21, 16, 0), (1, 72, 57, 341, 12, 0),
              (65535, 1, 1, 1, 4, 0), (66000, 1, 1, 70, 16, 0)]
    st = _lib.StatSrc(); st.stats_partial = 0x70000; st.tiles = 5; st.eps = 1e-5; st.count = 100
    for (n, d, h, w, c, pool), form in itertools.product(layers, ("plain", "bcast2", "bcast3", "stats")):
        for i, j in itertools.combinations(range(-1, len(mods)), 2):
            a = _lib.NormArgs()
            a.x, a.out, a.x_pitch, a.out_pitch = P, 0x40000, c, c
            if form != "stats":
                a.mean, a.rstd = 0x20000, 0x30000
            if pool:
                a.pool_out, a.pool_pitch = 0x50000, c
            a.N, a.D, a.H, a.W, a.C, a.act = n, d, h, w, c, 1
            for k in (i, j):
                if k >= 0:
                    setattr(a, *mods[k])
            rep = {"bcast2": 2, "bcast3": 3}.get(form, 1)
            fan = rep > 1 and not a.pool_out
            wrapped = {b"vx_norm_act_drop_pool: pitches/offsets": a.out_coff + a.C >= 1 << 31, b"vx_norm_act_drop_pool: sample too large": a.D * a.H * a.W * a.C >= 1 << 63,
                       b"vx_norm_act_drop_pool: the plane index": (a.N // rep if fan else a.N) * a.D >= 1 << 31}
            if form == "stats":
                call = lambda lib: lib.vx_norm_act_drop_pool_stats(C.byref(a), C.byref(st), None)
            elif form == "plain":
                call = lambda lib: lib.vx_norm_act_drop_pool(C.byref(a), None)
            else:
                call = lambda lib: lib.vx_norm_act_drop_pool_bcast(C.byref(a), rep, None)
            compare((form, (n, d, h, w, c, pool), mods[i] if i >= 0 else None, mods[j]), call, wrapped)
            dry = result(libs["new"], libs["new"].vx_norm_act_drop_pool_route(C.byref(a), rep, C.byref(st) if form == "stats" else None, None, 0, None))
            if dry != result(libs["new"], call(libs["new"])):
                bad += 1
                print("dry run differs from its entry point", form, (n, d, h, w, c, pool), mods[i] if i >= 0 else None, mods[j], dry)
    # ---- the small passes over grids ----
    Ns = (-1, 0, 1, 3, 65535, 65536, 1 << 20, big)
    sizes = (-1, 0, 1, 5, 129, 70001, (1 << 28) - 1, 1 << 28, (1 << 30) - 1, 1 << 30, (1 << 32) - 4, 1 << 32, 1 << 33, 1 << 61, 1 << 62, (1 << 63) - 1)
    ptrs = (None, P, P + 4)
    for n, v, p, q in itertools.product(Ns, sizes, ptrs, ptrs):
        for c in (-4, 0, 8, 516, 1 << 20, big - 3):
            compare(("finalize", n, c, v, p), lambda lib: lib.vx_instnorm_finalize(p, n, 3, c, v, 1e-5, P, q, None), {b"vx_instnorm_finalize: N * C": n * c >= 1 << 31})
        compare(("split", n, v, p, q), lambda lib: lib.vx_prenorm_split(p, q, P, n, v, 1.0, None), {})
        compare(("split_stats", n, v, p), lambda lib: lib.vx_prenorm_split_stats(p, C.byref(st) if q else None, n, v, 1.0, None), {})
        compare(("hash_mask", n, v, p), lambda lib: lib.vx_drop_hash_mask(1, 2, n, v, p, None), {})
        for pitch in (-8, 0, 4, 8, 10, 16, 18, big - 3):
            compare(("finish", n, v, p, q, pitch), lambda lib: lib.vx_pool_finish(p, P, P, P, q, pitch, n, v, 1, None), {})
            for dp in (-7, 0, 1, 6, 65536, big):
                w = {b"vx_pool_finish_z: empty": dp * v >= 1 << 63, b"vx_pool_finish_z_stats: empty": dp * v >= 1 << 63}
                compare(("finish_z", n, dp, v, p, q, pitch), lambda lib: lib.vx_pool_finish_z(p, P, P, P, q, pitch, n, dp, v, 1, None), w)
                compare(("finish_z_stats", n, dp, v, p, q, pitch), lambda lib: lib.vx_pool_finish_z_stats(p, P, C.byref(st), q, pitch, n, dp, v, 1, None), w)
    print(f"stream3d refusals: {calls} calls, {refused} refused by base, {new} refused by new alone with a listed message where base's arithmetic wrapped, "
          f"{bad} differ otherwise (code or message)")
    sys.exit(1 if bad else 0)

if args.hosttime:
    import statistics, time
    x = rc.forward_input((64, 64, 64))
    models, outs, med = {}, {}, {"base": [], "new": []}
    for which in libs:
        use(libs[which])
        models[which] = rc.forward_model({})
        outs[which] = torch.empty((10, 2, 64, 64, 64), device=x.device)
        for i in range(5):
            models[which](x, n_samples=10, seed=i, out=outs[which])
        torch.cuda.synchronize()
    for rnd in range(12):
        for which in (("base", "new") if rnd % 2 == 0 else ("new", "base")):
            use(libs[which])
            ts = []
            for i in range(20):
                t0 = time.perf_counter()
                models[which](x, n_samples=10, seed=i, out=outs[which])
                ts.append((time.perf_counter() - t0) * 1e6)
                torch.cuda.synchronize()
            med[which].append(statistics.median(ts))
    for which in libs:
        print(f"{which}: host time per eager T=10 64^3 forward, median of 20 calls per round, us: " + " ".join(f"{t:.1f}" for t in med[which]) +
              f"  | median {statistics.median(med[which]):.1f}  min {min(med[which]):.1f}  max {max(med[which]):.1f}")
    sys.exit(0)

bad = nondet = 0
for case in rc.LAYER_CASES:
    res = []
    for which in ("base", "base", "new"):
        use(libs[which])
        with _lib.config(**case["cfg"]):
            buf = rc.LayerBuffers(libs[which], case)
            name = buf.launch()
        res.append((name, (buf.out.clone(), buf.stats.clone(), buf.range_flag.clone())))
    det = same(res[0][1], res[1][1]); eq = same(res[0][1], res[2][1]) and res[0][0] == res[2][0]
    nondet += not det; bad += not eq
    print(f"layer {case['id']:44s} {res[2][0]:48s} base==base {det}  base==new {eq}", flush=True)
for cid, shape, kw, cfg in rc.FORWARD_CASES:
    from values_amd import predict_uncertainty
    res = []
    for which in ("base", "base", "new"):
        use(libs[which])
        with _lib.config(**cfg):
            model, x = rc.forward_model(kw), rc.forward_input(shape)
            if kw.get("do_dropout", True):
                out = predict_uncertainty([model], x, n_pred=rc.FORWARD_T, seeds=[rc.FORWARD_SEED])
            else:
                out = predict_uncertainty([model], x, n_pred=1)
            torch.cuda.synchronize()
        res.append([out[k].clone() for k in ("logits", "pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")])
    det = same(res[0], res[1]); eq = same(res[0], res[2])
    nondet += not det; bad += not eq
    print(f"forward {cid:32s} base==base {det}  base==new {eq}", flush=True)
print(f"{len(rc.LAYER_CASES)} layers, {len(rc.FORWARD_CASES)} forwards: {nondet} differ base against base, {bad} differ base against new")
sys.exit(1 if bad else 0)
