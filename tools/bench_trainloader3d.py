#!/usr/bin/env python3
"""The 3D train loader at the reference's shapes: batches/s and samples/s of the host loader (HostLoader3D, one process)
against the device loader (DeviceLoader3D; cache cold: cache_bytes=0, every batch reads and uploads its files again while
the previous one is in use; cache warm: all payloads resident), and the time of a vx_train_patches_3d call by device
events (table upload, memset and launch, calls back to back) with the GB/s its traffic gives.  Needs a GPU; nothing falls
back.

A seeded data set is generated under --dir (default: a temporary directory): --cases float64 volumes of --size^3 with three
uint8 raters, the toy layout's preprocessed tree.  Every loader runs the same order (one seed); a timed window lasts at least --seconds (whole
epochs of --batches batches) and ends in a device synchronise; the three loaders' windows alternate; each figure is the
median of --repeats windows and the spread (min .. max) is printed beside it.

    python tools/bench_trainloader3d.py [--cases 32] [--size 80] [--batch 16] [--patch 64] [--batches 16] [--seconds 0.5]
                                        [--repeats 5] [--kernel-only] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from values_amd import _lib  # noqa: E402
from values_amd import datamodule3d as dm  # noqa: E402


def make_tree(root, cases, size):
    base = os.path.join(root, "preprocessed")
    os.makedirs(os.path.join(base, "imagesTr"))
    os.makedirs(os.path.join(base, "labelsTr"))
    rs = np.random.RandomState(0)
    for c in range(cases):
        np.save(os.path.join(base, "imagesTr", f"{c:03d}.npy"), rs.standard_normal((size,) * 3))
        for r in range(3):
            np.save(os.path.join(base, "labelsTr", f"{c:03d}_{r:02d}.npy"), (rs.random_sample((size,) * 3) < 0.1 * (r + 1)).astype(np.uint8))
    return base


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def window(loader, seconds, sync):
    """whole epochs of the loader until `seconds` have passed -> (batches/s, samples/s, batches)"""
    t0 = time.perf_counter()
    n = k = 0
    while time.perf_counter() - t0 < seconds:
        for batch in loader:
            n += 1
            k += len(batch["image_paths"])
    if sync:
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return n / dt, k / dt, n


def bench_loaders(samples, args, augment):
    kw = dict(batch_size=args.batch, patch_size=args.patch, training=True, augment=augment, num_workers=1, seed=1,
              batches_per_epoch=args.batches)
    host = dm.HostLoader3D(samples, **kw)
    rates = {"host": [], "device_cold": [], "device_warm": []}
    with dm.DeviceLoader3D(samples, cache_bytes=0, **kw) as cold, dm.DeviceLoader3D(samples, cache_bytes=None, **kw) as warm:
        for _ in range(4 * max(1, len(samples) // args.batch)):       # warm-up: code objects, pinned buffers, every payload resident
            list(cold), list(warm)
        list(host)
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            rates["host"].append(window(host, args.seconds, False))
            rates["device_cold"].append(window(cold, args.seconds, True))
            rates["device_warm"].append(window(warm, args.seconds, True))
        resident = (len(warm.cache.entries), warm.cache.bytes)
    out = {k: {"batches_per_s": spread([r[0] for r in v]), "samples_per_s": spread([r[1] for r in v]), "batches_per_window": [r[2] for r in v]}
           for k, v in rates.items()}
    out["warm_cache"] = {"files": resident[0], "bytes": resident[1]}
    return out


def bench_kernel(args, noise):
    """vx_train_patches_3d alone, batch x patch^3 from resident float64 volumes with uint8 labels, device events"""
    lib = _lib.load()
    B, P, S = args.batch, args.patch, args.size
    g = torch.Generator(device="cuda").manual_seed(0)
    images = [torch.randn((S, S, S), dtype=torch.float64, device="cuda", generator=g) for _ in range(B)]
    labels = [(torch.rand((S, S, S), device="cuda", generator=g) < 0.2).to(torch.uint8) for _ in range(B)]
    items = (_lib.Train3dItem * B)()
    rs = np.random.RandomState(0)
    for i, it in enumerate(items):
        it.image, it.image_kind, it.label, it.label_kind = images[i].data_ptr(), _lib.VX_PREP_F64, labels[i].data_ptr(), _lib.VX_COUNT_B1
        for a in range(3):
            it.dims[a], it.origin[a] = S, int(rs.randint(0, S - P + 1))
        it.flags, it.index = int(rs.randint(0, 8)) | (8 if noise else 0), i
    data = torch.empty((B, 1, P, P, P), dtype=torch.float32, device="cuda")
    seg = torch.empty((B, 1, P, P, P), dtype=torch.float32, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    ws = _lib.workspace(data.device, int(lib.vx_train_patches_3d_workspace_bytes(B)))

    def call():
        _lib.check(lib.vx_train_patches_3d(items, B, P, P, P, _lib.ptr(data), _lib.ptr(seg), 0, 1, None, 0.0, 0.1, 0, None, _lib.ptr(status),
                                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "vx_train_patches_3d")
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    times, calls = [], 2000
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / calls)
    nbytes = B * P ** 3 * (8 + 4 + 1 + 4)          # float64 image + float32 data + uint8 label + float32 seg
    ms = spread(times)                              # (per call: table upload, memset and launch)
    return {"ms_per_call": ms, "calls_per_window": calls, "bytes_per_call": nbytes,
            "GB_per_s_at_median": nbytes / (ms["median"] * 1e-3) / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=32)
    ap.add_argument("--size", type=int, default=80)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true", help="skip the loaders (a run under a kernel tracer)")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    result = {"config": vars(args), "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory(dir=args.dir) as td:
        if not args.kernel_only:
            base = make_tree(td, args.cases, args.size)
            samples = dm.get_train_data_samples(base, "*.npy", None, 3)
            for augment in (False, True):
                result[f"loaders_augment_{'on' if augment else 'off'}"] = bench_loaders(samples, args, augment)
    for noise in (False, True):
        result[f"kernel_noise_{'on' if noise else 'off'}"] = bench_kernel(args, noise)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
