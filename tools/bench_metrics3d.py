"""Per-case test metrics of a 3D inference step (values_amd.metrics.process_metrics_3d): B = 32 volumes of 64^3, C = 2 classes,
T = 10 predictions, R = 1 and R = 4 raters.  One JSON line per R:

  soft_ms                 device events around vx_soft_metric_sums_batched (its two launches) over mean_softmax (B, C, nvox) + gt
  soft_gbps               float32 probabilities + uint8 labels read / soft_ms
  counts_ms               device events around vx_mask_agreement_batched over the stacked (B, 1 + T + R, nvox) masks
  soft_loop_ms            device events around B calls of vx_soft_metric_sums, the one-image kernel (same data)
  metrics_ms              host clock around process_metrics_3d (two launches' worth of device work, two copies, the ratios
                          on the host), the arg-max masks handed in as uncertainty_maps returns them
  loop_ms                 host clock around the per-case path it replaces: calculate_test_metrics + calculate_ged (with the
                          sample arg-maxes handed in) for each of the B cases
  host_ratios_ms          host clock around the ratio arithmetic alone (the same numpy counts and sums, no device work)
  speedup                 loop_ms / metrics_ms
  share_of_step           metrics_ms / --step-ms (the 3D step the metrics follow: 32 volumes at the README's volumes/s)

Hard Dice and the GED keys of the two paths are asserted equal, the loss within 1e-12.  Label maps are blobs (a thresholded
smooth field per case; every prediction and rater its own threshold), as a lesion segmentation looks to the kernels.

  python tools/bench_metrics3d.py [--iters 20] [--step-ms 8.2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_step(torch, B, T, R, C, S, seed):
    """probs (B, T, C, S, S, S) float32 softmax and gt (B, R, S, S, S) uint8: a smooth random field per case, every
    prediction a sigmoid of it around its own threshold, every rater a cut at its own threshold"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    coarse = torch.randn((B, 1, S // 8, S // 8, S // 8), device="cuda", generator=g)
    field = torch.nn.functional.interpolate(coarse, size=(S, S, S), mode="trilinear", align_corners=False)
    thr = 0.8 + 0.2 * torch.randn((B, T, 1, 1, 1), device="cuda", generator=g)
    fg = torch.sigmoid(4.0 * (field - thr) + 0.3 * torch.randn((B, T, S, S, S), device="cuda", generator=g))
    probs = torch.stack([1.0 - fg] + [fg / (C - 1)] * (C - 1), 2).to(torch.float32).contiguous()
    rthr = 0.8 + 0.2 * torch.randn((B, R, 1, 1, 1), device="cuda", generator=g)
    gt = (field > rthr).to(torch.uint8).contiguous()
    return probs, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-ms", type=float, default=8.2)
    a = ap.parse_args()
    import torch

    from values_amd import _lib
    from values_amd.metrics import (_metrics_3d_from_reductions, calculate_ged, calculate_test_metrics, mask_agreement_batched,
                                    process_metrics_3d, soft_metric_sums_batched)
    from values_amd.uncertainty import uncertainty_maps
    _lib.require_gpu()
    lib = _lib.load()
    B, T, C, S = 32, 10, 2, 64
    nvox = S ** 3
    st = _lib.stream_ptr()

    def events(fn, iters):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def clock(fn, iters):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    for R in (1, 4):
        probs, gt = make_step(torch, B, T, R, C, S, seed=100 + R)
        out = uncertainty_maps(probs, from_logits=False, want_sample_argmax=True)
        mean, am, sa = out["mean_softmax"], out["argmax"], out["sample_argmax"]
        M = 1 + T + R
        res = {"B": B, "S": S, "C": C, "T": T, "R": R, "foreground": round(float(gt.float().mean()), 4)}

        p = mean.reshape(B, C, nvox)
        g8 = gt.reshape(B, R, nvox)
        sums = torch.empty((B, R, 3 * C + 1), dtype=torch.float64, device="cuda")
        ws = torch.empty(int(lib.vx_soft_metric_batched_workspace_bytes(B, C, R, nvox)), dtype=torch.uint8, device="cuda")

        def soft():
            _lib.check(lib.vx_soft_metric_sums_batched(p.data_ptr(), g8.data_ptr(), B, C, R, nvox, sums.data_ptr(), ws.data_ptr(), st),
                       "vx_soft_metric_sums_batched")
        res["soft_ms"] = round(events(soft, a.iters), 4)
        res["soft_gbps"] = round(B * nvox * (4 * C + R) / res["soft_ms"] / 1e6, 1)

        stack = torch.cat([am.reshape(B, 1, nvox), sa.reshape(B, T, nvox), g8], 1).contiguous()
        counts = torch.empty((B, M, M, C), dtype=torch.int64, device="cuda")

        def count():
            _lib.check(lib.vx_mask_agreement_batched(stack.data_ptr(), B, M, C, nvox, -1, counts.data_ptr(), st),
                       "vx_mask_agreement_batched")
        res["counts_ms"] = round(events(count, a.iters), 4)

        sums1 = torch.empty_like(sums)
        ws1 = torch.empty(max(int(lib.vx_soft_metric_workspace_bytes(C, R)), 8), dtype=torch.uint8, device="cuda")

        def soft_loop():
            for b in range(B):
                _lib.check(lib.vx_soft_metric_sums(p[b].data_ptr(), g8[b].data_ptr(), C, R, nvox, sums1[b].data_ptr(), ws1.data_ptr(), st),
                           "vx_soft_metric_sums")
        res["soft_loop_ms"] = round(events(soft_loop, max(2, a.iters // 4)), 4)
        assert torch.equal(sums[..., 1:3 * C:3], sums1[..., 1:3 * C:3]), "batched and one-image label counts differ"
        assert torch.allclose(sums, sums1, rtol=2e-10, atol=0.0), "batched and one-image sums differ"   # 4 n 2^-53: two float64 orders

        def batched():
            return process_metrics_3d(out, gt)

        def loop():
            ms = []
            for b in range(B):
                m = calculate_test_metrics(mean[b:b + 1], gt[b])
                m.update(calculate_ged(probs[b], gt[b], pred_masks=sa[b]))
                ms.append(m)
            return ms
        res["metrics_ms"] = round(clock(batched, a.iters), 3)
        res["loop_ms"] = round(clock(loop, max(2, a.iters // 4)), 3)
        sn, In = soft_metric_sums_batched(mean, gt), mask_agreement_batched(stack, C)
        t0 = time.perf_counter()
        for _ in range(a.iters):
            _metrics_3d_from_reductions(sn, In, C, nvox, T, R)
        res["host_ratios_ms"] = round((time.perf_counter() - t0) * 1e3 / a.iters, 3)
        res["speedup"] = round(res["loop_ms"] / res["metrics_ms"], 2)
        res["share_of_step"] = round(res["metrics_ms"] / a.step_ms, 3)
        got, want = batched(), loop()
        for b in range(B):
            assert list(got[b]) == list(want[b]), b
            for k in want[b]:
                if k == "loss":
                    assert abs(got[b][k] - want[b][k]) < 1e-12, (b, k)
                else:
                    assert got[b][k] == want[b][k], (b, k, got[b][k], want[b][k])
        res["mean_dice"] = round(sum(m["dice"] for m in got) / B, 4)
        res["mean_ged"] = round(sum(m["ged"] for m in got) / B, 4)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
