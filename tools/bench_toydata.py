"""The toy data set generator (values_amd.toydata): host mirror, scipy baseline and device route in one process, one run.

Cases: 128^3 and 256^3, sigma 8, 5 raters, gray object, blur, segmentations and noise on.  One JSON line per case:

  mirror_s_per_case    wall clock of generate_toy_dataset(device_io=False) per sample.  The mirror restates scipy's filter
                       tap by tap in numpy and is slow by construction (--mirror-samples samples, 0 skips it)
  scipy_s_per_case     the baseline that matters, where scipy imports: the same steps with scipy.ndimage.gaussian_filter in
                       the blur's place -- embed, filter, np.quantile thresholds, np.where, np.random noise, nifti.save --
                       per sample (null without scipy)
  device_s_per_case    wall clock of generate_toy_dataset(device_io=True) per sample, files written, final synchronise
                       included, after one warm-up data set (min of --wall-reps runs)
  kernel_ms            GPU time of every call alone on a resident sample, device events, [min, max] of --reps repetitions
                       after one warm-up: embed, blur0 / blur1 / blur2, count, order_stats, segment, noise
  blur_gbs             16 bytes per voxel over each blur pass's min time; copy_fraction: against the 6.29 TB/s copy rate
                       DESIGN records
  order_stats_reads    reads of the data the one vx_order_stats_f64 call makes

  python tools/bench_toydata.py [--sizes 128,256] [--samples 2] [--mirror-samples 1] [--reps 5] [--wall-reps 2] [--root DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12   # the float4 copy rate DESIGN records for the MI355X, bytes / s
SIGMA, RATERS = 8, 5


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


def scipy_dataset(save, size, samples):
    """the host steps with scipy's filter -> seconds per sample, or None without scipy"""
    try:
        from scipy.ndimage import gaussian_filter
    except ImportError:
        return None
    import numpy as np
    from values_amd import nifti
    from values_amd import toydata as td
    os.makedirs(os.path.join(save, "segmentation"))
    plan = td.plan_samples(td.sphere_object, samples, size, object_gray=True, seed=22)
    np.random.seed(22)
    t0 = time.perf_counter()
    for i, item in enumerate(plan):
        image = gaussian_filter(td.embed(item), sigma=SIGMA)
        for r, seg in enumerate(td.segment(image, td.rater_thresholds(image, RATERS))):
            nifti.save(seg.transpose(2, 1, 0), os.path.join(save, "segmentation", f"{i:04d}_{r:02d}.nii.gz"))
        nifti.save(td.add_noise(image, 0.5).transpose(2, 1, 0), os.path.join(save, f"{i:04d}.nii.gz"))
    return (time.perf_counter() - t0) / samples


def kernel_times(size, reps):
    import numpy as np
    import torch
    from values_amd import toydata as td
    item = td.plan_samples(td.sphere_object, 1, size, object_gray=True, seed=22)[0]
    w, radius = td.gaussian_weights(SIGMA)
    wd = torch.from_numpy(w).cuda()
    names = ["embed", "blur0", "blur1", "blur2", "count", "order_stats", "segment", "noise"]
    times = {k: [] for k in names}
    reads = None
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        return out, (e0, e1)

    for rep in range(reps + 1):            # the first repetition warms every call up
        ev = {}
        image, ev["embed"] = timed(lambda: td.embed_device(item))
        a, ev["blur0"] = timed(lambda: td.blur_axis_device(image, 0, wd, radius))
        b, ev["blur1"] = timed(lambda: td.blur_axis_device(a, 1, wd, radius))
        c, ev["blur2"] = timed(lambda: td.blur_axis_device(b, 2, wd, radius, out=a))
        count, ev["count"] = timed(lambda: td.count_ge_device(c, 0.1))
        n = c.numel()
        perc = td._perc_thresholds(RATERS) * (int(count.cpu()[0]) / n)     # (the downloads lie between the timed spans)
        ks = [int(np.floor(float(q) * (n - 1))) for q in 1 - perc]
        (stats, _, reads), ev["order_stats"] = timed(lambda: td.order_stats_device(c, ks))
        thr = [float(v) for v in stats[:, 0].cpu()]
        _, ev["segment"] = timed(lambda: td.segment_device(c, thr))
        _, ev["noise"] = timed(lambda: td.add_noise_device(c, 22, 0))
        torch.cuda.synchronize()
        if rep:
            for k in names:
                times[k].append(ev[k][0].elapsed_time(ev[k][1]))
    return {k: [min(v), max(v)] for k, v in times.items()}, reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--mirror-samples", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wall-reps", type=int, default=2)
    ap.add_argument("--root", default=None)
    args = ap.parse_args()
    import torch
    from values_amd import generate_toy_dataset
    from values_amd.toydata import sphere_object
    assert torch.cuda.is_available(), "bench_toydata.py needs a GPU"
    for size in [int(s) for s in args.sizes.split(",")]:
        kw = dict(image_size=size, gauss_sigma=SIGMA, object_gray=True, blur=True, noise=True, segmentation=True, n_raters=RATERS, seed=22)
        line = {"size": size, "sigma": SIGMA, "raters": RATERS, "samples": args.samples, "device": torch.cuda.get_device_name(0)}
        with tempfile.TemporaryDirectory(dir=args.root) as d:
            line["mirror_s_per_case"] = None
            if args.mirror_samples:
                t0 = time.perf_counter()
                generate_toy_dataset(os.path.join(d, "mirror"), sphere_object, n_samples=args.mirror_samples, **kw)
                line["mirror_s_per_case"] = (time.perf_counter() - t0) / args.mirror_samples
            line["scipy_s_per_case"] = scipy_dataset(os.path.join(d, "scipy"), size, args.samples)
            generate_toy_dataset(os.path.join(d, "warm"), sphere_object, n_samples=1, device_io=True, **kw)
            runs = iter(range(args.wall_reps))
            line["device_s_per_case"] = wall(lambda: generate_toy_dataset(os.path.join(d, f"dev{next(runs)}"), sphere_object,
                                                                          n_samples=args.samples, device_io=True, **kw),
                                             args.wall_reps) / args.samples
            line["device_files_bytes"] = sum(os.path.getsize(os.path.join(p, f)) for p, _, fs in os.walk(os.path.join(d, "dev0")) for f in fs)
        km, reads = kernel_times(size, args.reps)
        line["kernel_ms"] = km
        nbytes = 16 * size ** 3
        line["blur_gbs"] = {k: nbytes / (km[k][0] * 1e-3) / 1e9 for k in ("blur0", "blur1", "blur2")}
        line["copy_fraction"] = {k: v * 1e9 / COPY_RATE for k, v in line["blur_gbs"].items()}
        line["order_stats_reads"] = reads
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
