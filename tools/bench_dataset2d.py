"""Measure the 2D test split's loader (values_amd.dataset2d) at the reference's image size: 256 x 478, B = 12, R = 5.

    python tools/bench_dataset2d.py [--images 48] [--iters 200]

Prints one JSON line:
  kernel_ms        GPU time of one vx_label_switch_batched call (int64 labels, raters + variance) between events: the median
                   of `iters` timed calls after 20 warm-up calls, and the min / max beside it
  kernel_gbs       (8 B in + (R + 4) B out) per pixel over that median
  refs_only_ms / refs_only_gbs   the loader's call: raters only, 8 + R bytes per pixel
  big_kernel_ms / big_kernel_gbs the first call at B = 192 (the call's memset, table upload and launch weigh 16 times less)
  host_s_per_image, device_s_per_image, device_prefetch_s_per_image
                   wall time per image of a pass over a temporary tree of `images` images: the host mirror's loader, the
                   device loader reading each batch's files when it is asked for, and the device loader reading batch i + 1
                   while batch i is on the device (median of 3 passes each, after one warm-up pass; files in the page cache)
"""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from values_amd import _lib, dataset2d as d2  # noqa: E402

H, W, B, R = 256, 478, 12, 5
IDS = np.array([0, 1, 2, 5, 8, 11, 13, 255])


def kernel_times(variance, iters, B=B):
    rng = np.random.default_rng(0)
    labs = [torch.from_numpy(IDS[rng.integers(0, len(IDS), size=(H, W))]).cuda() for _ in range(B)]
    refs = torch.empty((B, R, H, W), dtype=torch.uint8, device="cuda")
    var = torch.empty((B, W, H), dtype=torch.float32, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    arr = (_lib.LswitchItem * B)()
    for b in range(B):
        it = arr[b]
        it.labels, it.refs, it.H, it.W, it.kind, it.index = labs[b].data_ptr(), refs[b].data_ptr(), H, W, _lib.VX_COUNT_B8, b
        if variance:
            it.variance = var[b].data_ptr()
    for _ in range(20):
        d2.label_switch_call(arr, B, R, status, 1)
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d2.label_switch_call(arr, B, R, status, 1)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert status.cpu().tolist() == [0] * B
    return statistics.median(ms), min(ms), max(ms)


def make_tree(root, n):
    rng = np.random.default_rng(1)
    d = os.path.join(root, "OriginalData", "preprocessed")
    for kind in ("images", "labels"):
        os.makedirs(os.path.join(d, kind))
        os.makedirs(os.path.join(root, "CityScapesOriginalData", "preprocessed", kind))
    keys = []
    for i in range(n):
        np.save(os.path.join(d, "images", f"{i:05d}.npy"), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
        np.save(os.path.join(d, "labels", f"{i:05d}.npy"), IDS[rng.integers(0, len(IDS), size=(H, W))])
        keys.append((f"{i:05d}.npy", "gta"))
    empty = np.empty((0, 2), dtype="<U16")
    with open(os.path.join(root, "splits.pkl"), "wb") as f:
        pickle.dump([{"train": [], "val": [], "id_test": keys, "ood_test": [], "id_unlabeled_pool": empty, "ood_unlabeled_pool": empty}], f)
    return os.path.join(root, "splits.pkl")


def per_image(make_loader, n):
    times = []
    for p in range(4):
        loader = make_loader()
        t0 = time.perf_counter()
        for batch in loader:
            pass
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / n)
        if hasattr(loader, "close"):
            loader.close()
    return statistics.median(times[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    _lib.require_gpu()
    px = B * H * W
    full, full_lo, full_hi = kernel_times(True, args.iters)
    ro, ro_lo, ro_hi = kernel_times(False, args.iters)
    out = {"shape": [B, R, H, W], "kernel_ms": full, "kernel_ms_min": full_lo, "kernel_ms_max": full_hi,
           "kernel_gbs": px * (8 + R + 4) / full / 1e6, "refs_only_ms": ro, "refs_only_ms_min": ro_lo, "refs_only_ms_max": ro_hi,
           "refs_only_gbs": px * (8 + R) / ro / 1e6}
    big, big_lo, _ = kernel_times(True, args.iters, 16 * B)      # the same maps, 16 batches in one call: the launch costs fade
    out.update({"big_batch": 16 * B, "big_kernel_ms": big, "big_kernel_ms_min": big_lo, "big_kernel_gbs": 16 * px * (8 + R + 4) / big / 1e6})
    with tempfile.TemporaryDirectory() as root:
        splits = make_tree(root, args.images)
        tr = d2.TestTransforms2D(n_reference_samples=R)
        ds = d2.CityscapesTestSet(splits, root, split="id_test", transforms=tr, seed=1)
        out["images"] = len(ds)
        out["host_s_per_image"] = per_image(lambda: d2.HostTestLoader2D(ds, B), len(ds))
        out["device_s_per_image"] = per_image(lambda: d2.DeviceTestLoader2D(ds, B, seed=1, prefetch=False), len(ds))
        out["device_prefetch_s_per_image"] = per_image(lambda: d2.DeviceTestLoader2D(ds, B, seed=1, prefetch=True), len(ds))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
