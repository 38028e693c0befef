#!/usr/bin/env python3
"""Cases per second of a 3D test split, three routes in one process:

    a        the per-case route of the functions that existed before run_test_3d: host np.load, predict_image_sliding,
             process_metrics_3d on one case, ResultsWriter
    b        run_test_3d over the host loader
    c1/8/32  run_test_3d over the device loader at patch_batch 1 / 8 / 32

on N toy-shaped cases of 64^3 (one 64^3 patch each at the shipped patch_overlap 1), T = 10 MC-dropout passes, two raters.
Every route is warmed up once, then the routes alternate for --repeats rounds; a time is a host clock around a run that
ends with the writer closed and a device synchronise.  Then the stages of routes a and c32 alone (reading, the forwards at
batch 1 and 32, each route without its writer), and the three kernels of patches3d.hip alone: device-event time
per call and GB/s against the bytes they must move (computed from the shapes below), as a share of the 6.3 TB/s a
streaming kernel reaches on an MI355X and of the 8 TB/s peak.  Prints one JSON line per result.

    python tools/bench_test3d.py [--cases 32] [--repeats 5] [--passes 10]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, R = 64, 2
HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12


def build_tree(root, n):
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, "imagesTs"))
    os.makedirs(os.path.join(root, "labelsTs"))
    for i in range(n):
        img = rng.standard_normal((S, S, S)).astype(np.float32)
        np.save(os.path.join(root, "imagesTs", f"case{i:03d}.npy"), img)
        for r in range(R):
            np.save(os.path.join(root, "labelsTs", f"case{i:03d}_{r:02d}.npy"), (img > 0.2 * (r + 1)).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--passes", type=int, default=10)
    args = ap.parse_args()
    import torch
    from values_amd import UNet3D, _lib, predict_image_sliding, predict_logits, results, run_test_3d
    from values_amd.predict import derive_seed
    from values_amd.dataset3d import DeviceTestLoader3D, HostTestLoader3D, cases, composite_device, get_val_test_data_samples
    from values_amd.metrics import process_metrics_3d
    from values_amd.sliding import accumulate_cases, gather_patches_3d, predict_split_3d
    _lib.require_gpu()
    torch.manual_seed(0)
    model = UNet3D(num_classes=2, do_dropout=True).cuda()
    T, N = args.passes, args.cases
    tmp = tempfile.mkdtemp(prefix="bench_test3d_")
    try:
        build_tree(tmp, N)
        cs = cases(get_val_test_data_samples(tmp, num_raters=R, test=True, patch_size=S))
        assert len(cs) == N and all(len(c["crops"]) == 1 for c in cs)
        kw = dict(n_pred=T, seeds=[1], patch_size=S)

        def route_a(d):
            metrics = {}
            with results.ResultsWriter() as w:
                for c in cs:
                    img, labels = np.load(c["image_path"]), np.stack([np.load(p) for p in c["label_paths"]])
                    out = predict_image_sliding([model], torch.from_numpy(img), patch_batch=8, **kw)
                    (metrics[c["image_id"]],) = process_metrics_3d({"mean_softmax": out["mean_softmax"][None], "argmax": out["pred_seg_mean"][None]},
                                                                   torch.from_numpy(labels)[None], probs=out["softmax_sum"][None])
                    maps = {k: out[k] for k in ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")}
                    w.submit(d, c["image_id"], out["softmax_sum"], maps, data=img, gt_seg=labels, num_predictions=out["num_predictions"])
            results.log_metrics(d, metrics)

        def route_b(d):
            run_test_3d([model], HostTestLoader3D(cs, 32), d, patch_batch=32, **kw)

        def route_c(pb):
            def run(d):
                with DeviceTestLoader3D(cs, max(pb, 8)) as loader:
                    run_test_3d([model], loader, d, patch_batch=pb, **kw)
            return run

        routes = [("a", route_a), ("b", route_b), ("c1", route_c(1)), ("c8", route_c(8)), ("c32", route_c(32))]
        times = {name: [] for name, _ in routes}
        for rep in range(args.repeats + 1):           # round 0 warms every route up
            for name, fn in routes:
                d = os.path.join(tmp, f"out_{name}")
                shutil.rmtree(d, ignore_errors=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(d)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
        base = float(np.median(times["a"]))
        for name, _ in routes:
            t = np.array(times[name])
            print(json.dumps({"route": name, "cases": N, "passes": T, "repeats": len(t), "cases_per_s_median": N / float(np.median(t)),
                              "cases_per_s_min": N / float(t.max()), "cases_per_s_max": N / float(t.min()),
                              "seconds_median": float(np.median(t)), "speedup_vs_a": base / float(np.median(t))}), flush=True)

        # per-stage times of routes a and c32: reading, the forwards alone, everything but the writer
        def read_host(_):
            for c in cs:
                np.load(c["image_path"])
                for p in c["label_paths"]:
                    np.load(p)

        def read_device(_):
            with DeviceTestLoader3D(cs, 32) as loader:
                for _g in loader:
                    pass

        xs = torch.randn((N, 1, S, S, S), device="cuda")

        def forwards(batch):
            def run(_):
                for k, b0 in enumerate(range(0, N, batch)):
                    predict_logits([model], xs[b0:b0 + batch], n_pred=T, seeds=[derive_seed(1, 1, k)])
            return run

        def a_no_writer(_):
            for c in cs:
                img, labels = np.load(c["image_path"]), np.stack([np.load(p) for p in c["label_paths"]])
                out = predict_image_sliding([model], torch.from_numpy(img), patch_batch=8, **kw)
                process_metrics_3d({"mean_softmax": out["mean_softmax"][None], "argmax": out["pred_seg_mean"][None]},
                                   torch.from_numpy(labels)[None], probs=out["softmax_sum"][None])

        def c32_no_writer(_):
            with DeviceTestLoader3D(cs, 32) as loader:
                for _case in predict_split_3d([model], loader, patch_batch=32, **kw):
                    pass

        stages = [("read: np.load of every file", read_host), ("read: device loader alone", read_device),
                  ("forwards alone, batch 1", forwards(1)), ("forwards alone, batch 32", forwards(32)),
                  ("route a without the writer", a_no_writer), ("route c32 without the writer", c32_no_writer)]
        stimes = {name: [] for name, _ in stages}
        for rep in range(args.repeats + 1):
            for name, fn in stages:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(None)
                torch.cuda.synchronize()
                if rep:
                    stimes[name].append(time.perf_counter() - t0)
        for name, _ in stages:
            t = np.array(stimes[name])
            print(json.dumps({"stage": name, "cases": N, "ms_median": 1e3 * float(np.median(t)), "ms_min": 1e3 * float(t.min()),
                              "ms_max": 1e3 * float(t.max())}), flush=True)

        # the three kernels alone, at the shapes of a full forward batch of this split
        B, C = min(32, N), 2
        with DeviceTestLoader3D(cs[:B], B) as loader:
            (group,) = list(loader)
        patches = [(c, c["crops"][0]) for c in group]
        x = torch.empty((B, 1, S, S, S), device="cuda")
        logits = torch.randn((B, T, C, S, S, S), device="cuda")
        flat = _lib.zeros((B * (T * C + 1) * S ** 3,), torch.float32, "cuda")
        ssum = flat[:B * T * C * S ** 3].view(B, T, C, S, S, S)
        cnt = flat[B * T * C * S ** 3:].view(B, S, S, S)
        dests = [(ssum[b], cnt[b], (0, 0, 0)) for b in range(B)]
        ones = [torch.ones((S, S, S), device="cuda") for _ in range(B)]
        vox = B * S ** 3
        kernels = [("vx_gather_patches_3d", lambda: gather_patches_3d(patches, S, out=x), vox * (4 + 4)),
                   ("vx_softmax_accumulate_cases", lambda: accumulate_cases(logits, dests, False), vox * (T * C * 4 * 3 + 8)),
                   ("vx_case_composite", lambda: composite_device(group, ones), vox * (4 + 4 + 8 + R * (1 + 8 + 1)))]
        for name, fn, nbytes in kernels:
            for _ in range(3):
                fn()
            ms = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            rate = nbytes / (med * 1e-3)
            print(json.dumps({"kernel": name, "batch": B, "bytes": nbytes, "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                              "GB_per_s": rate / 1e9, "share_of_6.3TBs": rate / HBM_ACHIEVABLE, "share_of_8TBs_peak": rate / HBM_PEAK,
                              "note": "device events around the whole call: table upload and, for the composite, its allocations and status read included"}),
                  flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
