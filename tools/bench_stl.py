"""The mesh voxeliser (values_amd.stl): host mirror against the device route in one process, one run.

Per resolution (ballSphere.stl, 960 triangles), one JSON line:

  mirror_ms            wall clock of stl.voxelize per object, [min, median, max] of --reps runs after one warm-up
  device_ms            wall clock of stl.voxelize_device per object (upload cached, the odd_columns download and its
                       synchronise included), [min, median, max]
  kernel_ms            device time of one vx_voxelize_meshes call (the counter's zeroing and the one kernel): events around 50
                       calls back to back, over 50, [min, median, max] of --reps such spans; enqueue_ms is the host's time
                       to issue one call, which must be the smaller for the span to be device time
  listed_per_column    triangles a column meets in its workgroup's LDS lists after the tile culling (computed on the host
                       from the plan's tiles, rows of 64 columns), against 960 without culling; boxed_per_column: those whose own xy box
                       holds the column, which alone reach the edge functions
  out_gbs              4 bytes per voxel over the kernel's min time: the volume is written once
  equal                device volume == mirror volume, odd_columns both 0

and one line for a Case_1-shaped data set (64^3, sigma 2, 3 raters, --samples samples, ballSphere.stl): seconds per
sample on the host route and on the device route, files written, [min, median, max] of --wall-reps runs after one
warm-up data set each.  The host route's blur restates scipy's tap by tap and dominates it: object_ms_host /
object_ms_device give the voxeliser's share from the same plan.

  python tools/bench_stl.py [--resolutions 32,64,128] [--reps 10] [--samples 20] [--wall-reps 3] [--mesh PATH] [--root DIR]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TILE_X, TILE_Y = 64, 1     # voxel_plan.h
LAUNCHES = 50


def spread(v):
    return [min(v), statistics.median(v), max(v)]


def culling(tris, resolution):
    """-> (triangles listed per column, triangles whose box holds the column, per column): the kernel's two culling steps"""
    import numpy as np
    from values_amd import stl
    origin, h, dims = stl.voxel_grid([tris], resolution)
    cx, cy = stl.sample_points(origin[0], h, dims[0]), stl.sample_points(origin[1], h, dims[1])
    t = tris.astype(np.float64)
    keep = np.array([stl.triangle_setup(tri) is not None for tri in t])
    x0, x1, y0, y1 = t[keep, :, 0].min(1), t[keep, :, 0].max(1), t[keep, :, 1].min(1), t[keep, :, 1].max(1)
    listed = 0
    for j in range(0, len(cy), TILE_Y):
        for i in range(0, len(cx), TILE_X):
            xs, ys = cx[i:i + TILE_X], cy[j:j + TILE_Y]
            n = int(((x0 <= xs[-1]) & (x1 >= xs[0]) & (y0 <= ys[-1]) & (y1 >= ys[0])).sum())
            listed += n * len(xs) * len(ys)
    in_x = (cx[None, :] >= x0[:, None]) & (cx[None, :] <= x1[:, None])
    in_y = (cy[None, :] >= y0[:, None]) & (cy[None, :] <= y1[:, None])
    boxed = int((in_x.sum(1) * in_y.sum(1)).sum())
    columns = len(cx) * len(cy)
    return listed / columns, boxed / columns


def bench_objects(tris, resolutions, reps):
    import numpy as np
    import torch
    from values_amd import stl
    obj = stl.MeshObject([tris])
    for r in resolutions:
        want, want_odd = stl.voxelize_info([tris], r)                       # warm-up of the mirror
        mirror = []
        for _ in range(reps):
            t0 = time.perf_counter()
            stl.voxelize([tris], r)
            mirror.append((time.perf_counter() - t0) * 1e3)
        got = stl.voxelize_device(obj, r)                                    # warm-up: upload, code object
        torch.cuda.synchronize()
        device, kernel = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            stl.voxelize_device(obj, r)
            torch.cuda.synchronize()
            device.append((time.perf_counter() - t0) * 1e3)
        out, odd = torch.empty_like(got), torch.empty(1, dtype=torch.int64, device=got.device)
        for _ in range(reps):
            # LAUNCHES calls back to back between two events: the host prepares a call faster than the device runs it, so
            # the span is device time and its LAUNCHES-th part the time of one call
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(LAUNCHES):
                stl.voxelize_device_info(obj, r, out=out, odd=odd)
            e1.record()
            torch.cuda.synchronize()
            kernel.append(e0.elapsed_time(e1) / LAUNCHES)
        t0 = time.perf_counter()
        for _ in range(LAUNCHES):
            stl.voxelize_device_info(obj, r, out=out, odd=odd)
        enqueue_ms = (time.perf_counter() - t0) * 1e3 / LAUNCHES
        torch.cuda.synchronize()
        listed, boxed = culling(tris, r)
        line = {"mesh_triangles": len(tris), "resolution": r, "shape": list(want.shape), "reps": reps,
                "device": torch.cuda.get_device_name(0), "mirror_ms": spread(mirror), "device_ms": spread(device),
                "kernel_ms": spread(kernel), "enqueue_ms": enqueue_ms, "listed_per_column": listed, "boxed_per_column": boxed,
                "out_gbs": want.size * 4 / (min(kernel) * 1e-3) / 1e9,
                "equal": bool(np.array_equal(got.cpu().numpy(), want) and np.array_equal(out.cpu().numpy(), want)
                              and want_odd == 0 and int(odd.cpu()[0]) == 0)}
        print(json.dumps(line), flush=True)


def bench_dataset(mesh, samples, wall_reps, root):
    import numpy as np
    import torch
    from values_amd import generate_toy_dataset
    from values_amd import stl, toydata
    kw = dict(n_samples=samples, image_size=(64, 64, 64), min_object_ratio=5, max_object_ratio=2, gauss_sigma=2, blur=True,
              segmentation=True, n_raters=3, seed=16, input_files=[os.path.basename(mesh)])
    line = {"dataset": "Case_1-shaped", "samples": samples, "wall_reps": wall_reps, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory(dir=root) as d:
        for route, device_io in (("host", False), ("device", True)):
            fn = stl.mesh_object([mesh], device_io=device_io)
            generate_toy_dataset(os.path.join(d, f"{route}_warm"), fn, device_io=device_io, **dict(kw, n_samples=1))
            times = []
            for k in range(wall_reps):
                t0 = time.perf_counter()
                generate_toy_dataset(os.path.join(d, f"{route}{k}"), fn, device_io=device_io, **kw)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) / samples)
            line[f"{route}_s_per_sample"] = spread(times)
            # the voxeliser's share: the same resolutions, objects only
            shapes = [item["object"].shape[0] for item in toydata.plan_samples(lambda r: np.ones((r, r, r), np.float32), samples,
                                                                               (64, 64, 64), 5, 2, seed=16)]
            t0 = time.perf_counter()
            for r in shapes:
                fn(r)
            torch.cuda.synchronize()
            line[f"object_ms_{route}"] = (time.perf_counter() - t0) * 1e3 / samples
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", default="32,64,128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--wall-reps", type=int, default=3)
    ap.add_argument("--mesh", default=os.path.join(ROOT, "tests", "golden", "stl", "ballSphere.stl"))
    ap.add_argument("--root", default=None)
    args = ap.parse_args()
    import torch
    from values_amd import stl
    assert torch.cuda.is_available(), "bench_stl.py needs a GPU"
    tris = stl.read_stl(args.mesh)
    bench_objects(tris, [int(r) for r in args.resolutions.split(",")], args.reps)
    if args.samples:
        bench_dataset(args.mesh, args.samples, args.wall_reps, args.root)


if __name__ == "__main__":
    main()
