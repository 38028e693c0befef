#!/usr/bin/env python3
"""One-time A/B: are two builds of the library bit-identical on the cases of tests/conv3d_route_cases.py?  Both are loaded
RTLD_LOCAL into one process (as tools/ab_layers.py); every case runs base, base again (is the case deterministic?), then new,
on the same inputs.  Compared: single layers -- output tensor, statistics partials, range flag; forwards -- logits and the
uncertainty maps of predict_uncertainty.  Exit status 1 on any difference.

    python tools/ab_routes.py [--base values_amd/libvalues_amd_base.so] [--new values_amd/libvalues_amd.so]

--hosttime instead: the host time of one eager (uncaptured) T = 10 forward at 64^3 -- the call that issues every launch, returning
before the GPU has finished; the GPU idle at its start -- alternating base / new rounds of 20 calls in this one process."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from tests import conv3d_route_cases as rc
from values_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--base", default=os.path.join(ROOT, "values_amd", "libvalues_amd_base.so"))
ap.add_argument("--new", default=os.path.join(ROOT, "values_amd", "libvalues_amd.so"))
ap.add_argument("--hosttime", action="store_true")
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
