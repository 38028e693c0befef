"""Per-image test metrics of a 2D inference step (values_amd.metrics.process_metrics_2d): B = 8 images, T = 8 predictions,
R = 1 rater, 19 classes + the appended ignore class, at 1024 x 512 (config C4's step) and 256 x 478 (the reference's size).
One JSON line per size and label content:

  batched_ms              device events around vx_mask_agreement_batched over the stacked (B, 1 + T + R, H W) masks
  labels_gbps             uint8 labels read / batched_ms
  metrics_ms              host clock around process_metrics_2d (stack, launch, one copy, the ratios on the host) with the
                          per-sample arg-max masks handed in, as the results writer's caller has them
  metrics_argmax_ms       the same without them (one more uncertainty pass over softmax_pred)
  fold8_batched_ms        the same masks with labels folded mod 8 (C = 8): one batched launch ...
  fold8_loop_ms           ... against B launches of vx_mask_agreement; the counts are asserted bit-equal
  share_of_step           metrics_ms / --step-ms (the 2D step the metrics follow: 8 images at the README's images/s)

content "blocks": label maps in 32 x 32 blocks, every mask a copy with a tenth of its 8 x 8 cells redrawn (what a
segmentation looks like to the kernel: a 64-pixel run holds one to three classes); "noise": every pixel drawn on its own
(no segmentation looks like it: ~19 classes per run, the kernel's worst case).

  python tools/bench_metrics2d.py [--iters 20] [--step-ms 51]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_masks(torch, B, M, H, W, C, content, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if content == "noise":
        m = torch.randint(0, C, (B, M, H, W), device="cuda", generator=g, dtype=torch.uint8)
    else:
        def up(t, f):
            return t.repeat_interleave(f, -2).repeat_interleave(f, -1)[..., :H, :W]
        base = up(torch.randint(0, C, (B, 1, (H + 31) // 32, (W + 31) // 32), device="cuda", generator=g, dtype=torch.uint8), 32)
        cells = ((H + 7) // 8, (W + 7) // 8)
        redraw = up(torch.rand((B, M) + cells, device="cuda", generator=g) < 0.1, 8)
        other = up(torch.randint(0, C, (B, M) + cells, device="cuda", generator=g, dtype=torch.uint8), 8)
        m = torch.where(redraw, other, base.expand(B, M, H, W))
    # the rater (last mask) carries the ignore label on ~3 % of its 8 x 8 cells
    ign = torch.rand((B, (H + 7) // 8, (W + 7) // 8), device="cuda", generator=g) < 0.03
    m[:, -1][ign.repeat_interleave(8, -2).repeat_interleave(8, -1)[:, :H, :W]] = 255
    return m.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-ms", type=float, default=51.0)
    a = ap.parse_args()
    import numpy as np
    import torch

    from values_amd import _lib
    from values_amd.metrics import mask_agreement_batched, process_metrics_2d
    _lib.require_gpu()
    lib = _lib.load()
    B, T, R, C = 8, 8, 1, 19
    M, Ce = 1 + T + R, C + 1

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

    for H, W in ((1024, 512), (256, 478)):
        for content in ("blocks", "noise"):
            m = make_masks(torch, B, M, H, W, C, content, seed=H + len(content))
            nvox = H * W
            out = torch.empty((B, M, M, Ce), dtype=torch.int64, device="cuda")
            st = _lib.stream_ptr()

            def batched(mm=m, cc=Ce, oo=out, remap=255):
                _lib.check(lib.vx_mask_agreement_batched(mm.data_ptr(), B, M, cc, nvox, remap, oo.data_ptr(), st),
                           "vx_mask_agreement_batched")
            res = {"H": H, "W": W, "B": B, "T": T, "R": R, "classes": Ce, "content": content}
            res["batched_ms"] = round(events(batched, a.iters), 4)
            res["labels_gbps"] = round(B * M * nvox / res["batched_ms"] / 1e6, 1)
            # the whole metrics step: softmax_pred whose arg-max masks are m[:, 1 : 1 + T]; pred_seg = m[:, 0]
            probs = torch.full((B, T, C, H, W), 0.1 / (C - 1), dtype=torch.float32, device="cuda")
            probs.scatter_(2, m[:, 1:1 + T].unsqueeze(2).long(), 0.9)
            o = {"softmax_pred": probs, "pred_seg": m[:, 0]}
            gt, sa = m[:, 1 + T:], m[:, 1:1 + T]
            res["metrics_ms"] = round(clock(lambda: process_metrics_2d(o, gt, sample_argmax=sa), a.iters), 3)
            res["metrics_argmax_ms"] = round(clock(lambda: process_metrics_2d(o, gt), max(2, a.iters // 4)), 3)
            res["share_of_step"] = round(res["metrics_ms"] / a.step_ms, 4)
            del probs, o
            # C <= 8: one batched launch against B launches of the one-image kernel, same counts
            f8 = (m % 8).contiguous()
            o8 = torch.empty((B, M, M, 8), dtype=torch.int64, device="cuda")
            l8 = torch.empty((B, M, M, 8), dtype=torch.int64, device="cuda")

            def loop():
                for b in range(B):
                    _lib.check(lib.vx_mask_agreement(f8[b].data_ptr(), M, 8, nvox, l8[b].data_ptr(), st), "vx_mask_agreement")
            res["fold8_batched_ms"] = round(events(lambda: batched(f8, 8, o8, -1), a.iters), 4)
            res["fold8_loop_ms"] = round(events(loop, a.iters), 4)
            assert torch.equal(o8, l8), "batched and one-image counts differ"
            assert np.array_equal(mask_agreement_batched(m, Ce, 255), out.cpu().numpy())
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
