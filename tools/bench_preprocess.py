"""The 3D preprocessing step (values_amd.preprocess) on synthetic raw data sets the tool writes itself with nifti.save, host
mirror against the device route, in one process:

  toy    8 volumes of 128^3 int16, one uint8 rater each
  lidc   64 crops of (40, 40, 24) float32, one uint8 rater each

One JSON line per case:

  host_s_per_case, device_s_per_case   wall clock of preprocess_dataset(device_io=False / True) over the case count: files
                                       read, .npy files written, final synchronise included (min of --wall-reps runs of the
                                       device route; the host mirror runs once)
  stats_ms, pad_ms                     GPU time of ONE vx_volume_stats_batched / vx_zscore_pad_batched call over the whole
                                       data set resident on the device (volumes and labels in one batch), device events
                                       around the call, [min, max] of --reps repetitions after one warm-up
  stats_gbs, pad_gbs                   the bytes the kernel must move over its min time: statistics = two reads of every
                                       source; normalise-and-pad = one read of every source and one write of every padded
                                       output
  roofline_ms                          those bytes / 8 TB/s, per kernel

  python tools/bench_preprocess.py [--cases toy,lidc] [--reps 5] [--wall-reps 2] [--skip-host] [--root DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"toy": (8, (128, 128, 128), "int16"), "lidc": (64, (40, 40, 24), "float32")}


def write_raw(root, count, shape, dtype):
    import numpy as np
    from values_amd import nifti
    os.makedirs(os.path.join(root, "images"))
    os.makedirs(os.path.join(root, "labels"))
    rng = np.random.default_rng(0)
    for i in range(count):
        base = rng.standard_normal(shape) * 300 + 40
        nifti.save(base.astype(dtype), os.path.join(root, "images", f"case_{i:03d}.nii.gz"))
        nifti.save((base > 400).astype(np.uint8), os.path.join(root, "labels", f"case_{i:03d}_00.nii.gz"))


def wall(fn, reps):
    import torch
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def kernel_times(root, count, reps):
    """the two calls alone over the whole data set on the device -> (stats [min, max] ms, pad [min, max] ms, bytes)"""
    import torch
    from values_amd import nifti
    from values_amd import preprocess as pp
    images = [t for t, _ in nifti.load_device([os.path.join(root, "images", f"case_{i:03d}.nii.gz") for i in range(count)])]
    labels = [[t for t, _ in nifti.load_device([os.path.join(root, "labels", f"case_{i:03d}_00.nii.gz")])] for i in range(count)]
    srcs, arr, outs, arena, _, _ = pp._plan_batch(images, labels, 64, 1.0, None)
    dev = arena.device
    stats = torch.empty((len(srcs), 4), dtype=torch.float64, device=dev)
    src_bytes = sum(t.numel() * t.element_size() for t in srcs)
    out_bytes = sum(t.numel() * t.element_size() for t in outs)
    st, pd = [], []
    for rep in range(reps + 1):            # the first repetition warms both calls up
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        pp._stats_call(srcs, stats, dev)
        e[1].record()
        pp._pad_call(arr, len(srcs), stats, dev)
        e[2].record()
        torch.cuda.synchronize()
        if rep:
            st.append(e[0].elapsed_time(e[1]))
            pd.append(e[1].elapsed_time(e[2]))
    return [min(st), max(st)], [min(pd), max(pd)], src_bytes, out_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="toy,lidc")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wall-reps", type=int, default=2)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--root", default=None)
    args = ap.parse_args()
    import torch
    from values_amd import preprocess_dataset
    assert torch.cuda.is_available(), "bench_preprocess.py needs a GPU"
    for case in args.cases.split(","):
        count, shape, dtype = CASES[case]
        with tempfile.TemporaryDirectory(dir=args.root) as d:
            root = os.path.join(d, "raw")
            write_raw(root, count, shape, dtype)
            line = {"case": case, "count": count, "shape": list(shape), "dtype": dtype}
            if not args.skip_host:
                line["host_s_per_case"] = wall(lambda: preprocess_dataset(root, os.path.join(d, "host"), 1), 1) / count
            preprocess_dataset(root, os.path.join(d, "warm"), 1, device_io=True)
            line["device_s_per_case"] = wall(lambda: preprocess_dataset(root, os.path.join(d, "dev"), 1, device_io=True), args.wall_reps) / count
            st, pd, src_bytes, out_bytes = kernel_times(root, count, args.reps)
            line.update(stats_ms=st, pad_ms=pd, stats_bytes=2 * src_bytes, pad_bytes=src_bytes + out_bytes)
            line["stats_gbs"] = 2 * src_bytes / (st[0] * 1e-3) / 1e9 if st[0] > 0 else None
            line["pad_gbs"] = (src_bytes + out_bytes) / (pd[0] * 1e-3) / 1e9 if pd[0] > 0 else None
            line["roofline_ms"] = {"stats": 2 * src_bytes / 8e12 * 1e3, "pad": (src_bytes + out_bytes) / 8e12 * 1e3}
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
