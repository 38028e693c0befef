"""The 2D SSN head's validation reduction at the shipped shape: 256 x 478 images, head at 64 x 120, C = 19, R = 10, S = 10,
B = 4, with injected and with generated normals.  One JSON line per normals kind, both routes in one process, alternating:

  fused_ms      values_amd.validation.val_sums_ssn2d: vx_val_ssn2d_sums_batched (three launches) and the read-back of its
                (B, S, 1 + 2C) and (B, C + 2) float64 sums
  fused_dev_ms  device events around vx_val_ssn2d_sums_batched alone (no read-back)
  mat_ms        the route the package offered before: LowRankNormal2D.sample_images(S) (vx_ssn2d_lowres, S + 1 upsamples,
                vx_ssn2d_add_diag: S x B x C x H x W float32 written) and validation.val_sums on each of the S samples, with its
                read-back of (B, 5C + 3) sums per sample
  mat_dev_ms    device events around the same work through the C entry points, one read-back-free call per sample
  ratio         mat_ms / fused_ms;  ratio_dev: mat_dev_ms / fused_dev_ms
  median of --rounds alternating rounds with min / max next to it; host-clock times end in a device synchronise.

The two routes' numbers are compared on the spot: log-term sums within 1e-12 relative (both are float64 sums of the same
float32 samples, ordered differently), arg-max and target counts equal.

  python tools/bench_valstep2d.py [--rounds 5] [--min-window-ms 300] [--batch 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-window-ms", type=float, default=300.0)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, nargs=2, default=(256, 478))
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--rank", type=int, default=10)
    a = ap.parse_args()
    import numpy as np
    import torch

    from values_amd import _lib
    from values_amd import validation as va
    from values_amd.hrnet import LowRankNormal2D
    _lib.require_gpu()
    lib = _lib.load()
    st = _lib.stream_ptr()
    B, C, R, S, (H, W), seed = a.batch, a.classes, a.rank, a.samples, a.size, 1234
    h0, w0 = ((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2     # two stride-2 3x3 convs with padding 1
    nvox = H * W
    g = torch.Generator(device="cuda").manual_seed(7)
    pm, pf = (C + 3) // 4 * 4, (R * C + 15) // 16 * 16
    mean = torch.zeros((B, h0, w0, pm), device="cuda")
    mean[..., :C] = torch.randn((B, h0, w0, C), device="cuda", generator=g) * 1.5
    fac = torch.zeros((B, h0, w0, pf), device="cuda")
    fac[..., :R * C] = torch.randn((B, h0, w0, R * C), device="cuda", generator=g) * 0.2
    labels = torch.randint(0, C, (B, nvox), device="cuda", generator=g).to(torch.uint8)
    labels[torch.rand((B, nvox), device="cuda", generator=g) < 0.1] = 255
    dist = LowRankNormal2D.from_lowres(mean, fac, C, R, 1e-5, (H, W))
    ss = torch.empty((B, S, 1 + 2 * C), dtype=torch.float64, device="cuda")
    ts = torch.empty((B, C + 2), dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.vx_val_ssn2d_sums_workspace_bytes(B, S, C, h0, w0, H, W)), dtype=torch.uint8, device="cuda")
    sums = torch.empty((S, B, 5 * C + 3), dtype=torch.float64, device="cuda")
    ws1 = torch.empty(int(lib.vx_val_sums_workspace_bytes(B, C, nvox)), dtype=torch.uint8, device="cuda")

    def host(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for kind in ("injected", "generated"):
        ew = torch.randn((S, B, R), device="cuda", generator=g) if kind == "injected" else None
        ed = torch.randn((S, B, C * nvox), device="cuda", generator=g) if kind == "injected" else None

        def fused():
            return va.val_sums_ssn2d(dist, labels, S, ew, ed, seed, 0, 255)

        def fused_dev():
            _lib.check(lib.vx_val_ssn2d_sums_batched(mean.data_ptr(), pm, fac.data_ptr(), pf, _lib.ptr(ew), _lib.ptr(ed), seed, 0, labels.data_ptr(),
                                                     B, S, C, R, h0, w0, H, W, 1e-5, 255, ss.data_ptr(), ts.data_ptr(), ws.data_ptr(), ws.numel(),
                                                     st), "fused")

        def mat():
            smp = dist.sample_images(S, ew, ed, seed)
            return [va.val_sums(smp[:, s], labels, 255) for s in range(S)]

        def mat_dev():
            smp = dist.sample_images(S, ew, ed, seed)
            for s in range(S):
                x = smp[:, s].contiguous()
                _lib.check(lib.vx_val_sums_batched(x.data_ptr(), labels.data_ptr(), B, C, nvox, 255, sums[s].data_ptr(), ws1.data_ptr(),
                                                   ws1.numel(), st), "vx_val_sums_batched")

        routes = (("fused", fused, host), ("fused_dev", fused_dev, events), ("mat", mat, host), ("mat_dev", mat_dev, events))
        for _, fn, _ in routes:          # warm up: code objects, torch's allocator, the shared workspace
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        iters = {n: max(5, int(a.min_window_ms / max(timer(fn, 3), 1e-3))) for n, fn, timer in routes}
        ms = {n: [] for n, _, _ in routes}
        for _ in range(a.rounds):
            for n, fn, timer in routes:
                ms[n].append(timer(fn, iters[n]))
        # the two routes' numbers
        f_ss, f_ts = fused()
        rows = np.stack(mat(), 1)                                            # (B, S, 5C + 3)
        cls = rows[:, :, :5 * C].reshape(B, S, C, 5)
        rel = float(np.abs(f_ss[:, :, 0] - rows[:, :, 5 * C]).max() / np.abs(rows[:, :, 5 * C]).max())
        same = bool(np.array_equal(f_ss[:, :, 1:1 + C], cls[..., 3]) and np.array_equal(f_ss[:, :, 1 + C:], cls[..., 4])
                    and np.array_equal(f_ts[:, :C], cls[:, 0, :, 1]) and np.array_equal(f_ts[:, C], rows[:, 0, 5 * C + 1]))
        assert rel < 1e-12 and same, (kind, rel, same)
        med = {n: statistics.median(v) for n, v in ms.items()}
        res = {"kind": kind, "B": B, "size": [H, W], "lowres": [h0, w0], "C": C, "R": R, "S": S}
        for n in ms:
            res[n + "_ms"] = round(med[n], 4)
            res[n + "_ms_min_max"] = [round(min(ms[n]), 4), round(max(ms[n]), 4)]
        res.update({"ratio": round(med["mat"] / med["fused"], 2), "ratio_dev": round(med["mat_dev"] / med["fused_dev"], 2),
                    "samples_mb_per_image": round(S * C * nvox * 4 / 1e6, 1), "iters": iters, "rounds": a.rounds, "ll_rel_diff": rel})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
