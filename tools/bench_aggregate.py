"""Map -> scalar aggregations of a split (values_amd.aggregation): the per-image loop (the three functions per map through
io.instantiate, each a vx_aggregate_batched call of one map and one spec) against one aggregate_batch call, on the same
device-resident float32 maps, in one process.  Patch size 10 (--patch), one threshold, the image-level mean.  One JSON line
per case:

  case                    "3d": 32 maps of 64^3;  "2d": 32 maps of 1024 x 512
  loop_ms_per_map         host clock around the per-image loop over the 32 maps, final synchronise included, / 32
  batch_ms_per_map        the same around one aggregate_batch call
  loop_gpu_ms_per_map     device events around the same loops (the per-image loop blocks on its copies, so its device
  batch_gpu_ms_per_map    time includes the gaps the host leaves)
  kernels_ms_per_map      device events around vx_aggregate_batched alone (descriptor upload + its launches)
  loop_launches_per_map   launches of the library per map, counted from the launcher: the patch call 3 (two box passes
                          and the finish), the image-level and the threshold call 1 each (the sums kernel)
  batch_launches_per_map  4 per call / maps per call
  loop_round_trips_per_map  blocking device -> host copies per map: one per call, 1 + 1 + 1;  the batched call: 1 per call
  loop_workspace_bytes    what the loop's largest call asks of the shared grow-only workspace (_lib.workspace: 64 KiB at
                          the least, allocated once): vx_aggregate_workspace_bytes of one map and the patch spec
  batch_workspace_bytes   vx_aggregate_workspace_bytes for the whole batch
  speedup                 loop_ms_per_map / batch_ms_per_map

The results of the two paths are compared with `==` before anything is timed.

  python tools/bench_aggregate.py [--iters 10] [--maps 32] [--patch 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--maps", type=int, default=32)
    ap.add_argument("--patch", type=int, default=10)
    a = ap.parse_args()
    import torch

    from values_amd import _lib, aggregation
    from values_amd.io import instantiate
    _lib.require_gpu()
    lib = _lib.load()
    B = a.maps
    aggs = {"patch_level": {"_target_": "values_amd.aggregation.patch_level_aggregation", "patch_size": a.patch},
            "image_level": {"_target_": "values_amd.aggregation.image_level_aggregation", "mean": True},
            "threshold": {"_target_": "values_amd.aggregation.threshold_aggregation", "threshold": 0.5}}

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters, e0.elapsed_time(e1) / iters

    for case, shape in (("3d", (64, 64, 64)), ("2d", (1024, 512))):
        g = torch.Generator(device="cuda").manual_seed(len(shape))
        maps = [torch.rand(shape, device="cuda", generator=g, dtype=torch.float32) for _ in range(B)]

        def loop():
            return [{name: instantiate(dict(cfg), image=m, pred_model=None, unc_type=None) for name, cfg in aggs.items()}
                    for m in maps]

        def batch():
            return aggregation.aggregate_batch(maps, aggs)
        assert batch() == loop(), f"{case}: batched and per-image results differ"

        plan = aggregation._plan(aggs)
        specs, _ = aggregation._specs_for(plan, len(shape))
        items = (_lib.AggItem * B)(*[aggregation._item(m.data_ptr(), False, shape) for m in maps])
        sp = aggregation._spec_array(specs)
        ws_bytes = int(lib.vx_aggregate_workspace_bytes(items, B, sp, len(specs)))
        patch_spec = aggregation._spec_array([s for s in specs if s[0] == _lib.VX_AGG_PATCH])
        loop_ws_bytes = int(lib.vx_aggregate_workspace_bytes(items, 1, patch_spec, 1))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        out = torch.empty((B, len(specs), 4), dtype=torch.float64, device="cuda")
        st = _lib.stream_ptr()

        def kernels():
            _lib.check(lib.vx_aggregate_batched(items, B, sp, len(specs), _lib.ptr(out), _lib.ptr(ws), ws_bytes, st),
                       "vx_aggregate_batched")
        loop_ms, loop_gpu = timed(loop, max(2, a.iters // 3))
        batch_ms, batch_gpu = timed(batch, a.iters)
        _, kern_gpu = timed(kernels, a.iters)
        print(json.dumps({
            "case": case, "maps": B, "shape": list(shape), "patch": a.patch,
            "loop_ms_per_map": round(loop_ms / B, 4), "batch_ms_per_map": round(batch_ms / B, 4),
            "loop_gpu_ms_per_map": round(loop_gpu / B, 4), "batch_gpu_ms_per_map": round(batch_gpu / B, 4),
            "kernels_ms_per_map": round(kern_gpu / B, 4),
            "loop_launches_per_map": 5, "batch_launches_per_map": round(4 / B, 3),
            "loop_round_trips_per_map": 3, "batch_round_trips_per_map": round(1 / B, 3),
            "loop_workspace_bytes": loop_ws_bytes, "batch_workspace_bytes": ws_bytes,
            "speedup": round(loop_ms / batch_ms, 2)}), flush=True)


if __name__ == "__main__":
    main()
