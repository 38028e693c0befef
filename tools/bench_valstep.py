"""The validation step's reductions at the reference's defaults: 64^3 patches, C = 2, SSN (S = 10, R = 10) and the aleatoric
head (T = 10), B in {1, 8}, generated normals.  One JSON line per (kind, B), both routes in one process, alternating:

  fused_ms      device events around the fused call (vx_val_ssn_sums_batched / vx_val_aleatoric_sums_batched: two launches)
  fused_gbps    head + labels read once / fused_ms           (the traffic the algorithm needs)
  hbm_floor_ms  the same bytes at --hbm-tbps (default 6.3, what a streaming kernel reaches on an MI355X)
  mat_ms        device events around the materialised route built from entry points that predate the fused ones:
                vx_ssn_sample / vx_aleatoric_sample, then torch log_softmax / gather / sum / argmax (and, aleatoric,
                logsumexp / exp and the soft sums) on the device, float32
  mat_gbps      the bytes THAT route moves at the least (head read, samples written and read twice) / mat_ms
  ratio         mat_ms / fused_ms
  median of --rounds alternating rounds; min / max are kept next to it.

The two routes' numbers are compared (float32 route against float64 sums: 1e-4 relative on the log terms, arg-max
counts within 2 voxels per sample -- the float32 route resolves near-ties differently).

  python tools/bench_valstep.py [--rounds 5] [--min-window-ms 300]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-window-ms", type=float, default=300.0)
    ap.add_argument("--hbm-tbps", type=float, default=6.3)
    ap.add_argument("--size", type=int, default=64)
    a = ap.parse_args()
    import torch

    from values_amd import _lib
    _lib.require_gpu()
    lib = _lib.load()
    st = _lib.stream_ptr()
    C, S, R, T, size, seed = 2, 10, 10, 10, a.size, 1234
    nvox = size ** 3

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def measure(fused, mat):
        for fn in (fused, mat):      # warm up: code objects, torch's allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        iters = {}
        for name, fn in (("fused", fused), ("mat", mat)):
            iters[name] = max(10, int(a.min_window_ms / max(events(fn, 5), 1e-3)))
        ms = {"fused": [], "mat": []}
        for _ in range(a.rounds):
            ms["fused"].append(events(fused, iters["fused"]))
            ms["mat"].append(events(mat, iters["mat"]))
        return ms, iters

    for kind in ("ssn", "aleatoric"):
        for B in (1, 8):
            g = torch.Generator(device="cuda").manual_seed(10 * B + len(kind))
            labels = (torch.rand((B, nvox), device="cuda", generator=g) < 0.2).to(torch.uint8)
            lab64 = labels.long()
            if kind == "ssn":
                planes = (2 + R) * C
                head = torch.cat([torch.randn((B, C, nvox), device="cuda", generator=g) * 2.0,
                                  torch.randn((B, C, nvox), device="cuda", generator=g) * 0.5 - 2.0,
                                  torch.randn((B, R * C, nvox), device="cuda", generator=g) * 0.2], 1).contiguous()
                ss = torch.empty((B, S, 1 + 2 * C), dtype=torch.float64, device="cuda")
                ts = torch.empty((B, C + 2), dtype=torch.float64, device="cuda")
                ws = torch.empty(int(lib.vx_val_ssn_sums_workspace_bytes(B, S, C, nvox)), dtype=torch.uint8, device="cuda")
                smp = torch.empty((B, S, C, nvox), dtype=torch.float32, device="cuda")
                n_s = S

                def fused():
                    _lib.check(lib.vx_val_ssn_sums_batched(head.data_ptr(), None, None, seed, 0, labels.data_ptr(), B, S, C, R, nvox, 1e-5,
                                                           -1, ss.data_ptr(), ts.data_ptr(), ws.data_ptr(), ws.numel(), st), "fused ssn")

                def mat():
                    _lib.check(lib.vx_ssn_sample(head.data_ptr(), None, None, seed, B, S, C, R, nvox, 1e-5, smp.data_ptr(), st), "vx_ssn_sample")
                    ls = torch.log_softmax(smp, 2)
                    ll = ls.gather(2, lab64[:, None, None, :].expand(B, S, 1, nvox)).sum((2, 3))
                    am = smp.argmax(2)
                    pred = torch.stack([(am == c).sum(-1) for c in range(C)], -1)
                    tp = torch.stack([((am == c) & (lab64[:, None] == c)).sum(-1) for c in range(C)], -1)
                    return ll, tp, pred
            else:
                planes = 2 * C
                head = torch.cat([torch.randn((B, C, nvox), device="cuda", generator=g) * 2.0,
                                  torch.randn((B, C, nvox), device="cuda", generator=g) * 0.5 - 2.0], 1).contiguous()
                sums = torch.empty((B, 5 * C + 3), dtype=torch.float64, device="cuda")
                ws = torch.empty(int(lib.vx_val_aleatoric_sums_workspace_bytes(B, C, nvox)), dtype=torch.uint8, device="cuda")
                smp = torch.empty((B, T, C, nvox), dtype=torch.float32, device="cuda")
                onehot = torch.nn.functional.one_hot(lab64, C).permute(0, 2, 1).float()
                n_s = T

                def fused():
                    _lib.check(lib.vx_val_aleatoric_sums_batched(head.data_ptr(), None, seed, 0, labels.data_ptr(), B, T, C, nvox, -1,
                                                                 sums.data_ptr(), ws.data_ptr(), ws.numel(), st), "fused aleatoric")

                def mat():
                    _lib.check(lib.vx_aleatoric_sample(head.data_ptr(), None, seed, B, T, C, nvox, smp.data_ptr(), None, st),
                               "vx_aleatoric_sample")
                    lavg = torch.logsumexp(torch.log_softmax(smp, 2), 1) - math.log(T)
                    p = torch.exp(lavg)
                    ll = lavg.gather(1, lab64[:, None, :]).sum((1, 2))
                    am = p.argmax(1)
                    pred = torch.stack([(am == c).sum(-1) for c in range(C)], -1)
                    tp = torch.stack([((am == c) & (lab64 == c)).sum(-1) for c in range(C)], -1)
                    return ll, tp, pred, (p * onehot).sum(-1), p.sum(-1)

            ms, iters = measure(fused, mat)
            # the two routes' numbers
            fused()
            ref = mat()
            torch.cuda.synchronize()
            if kind == "ssn":
                got_ll, got_tp, got_pred = ss[:, :, 0], ss[:, :, 1:1 + C], ss[:, :, 1 + C:]
            else:
                row = sums[:, :5 * C].reshape(B, C, 5)
                got_ll, got_tp, got_pred = sums[:, 5 * C], row[:, :, 3], row[:, :, 4]
            rel = float(((got_ll - ref[0].double()).abs() / ref[0].double().abs()).max())
            dcount = float(max((got_tp - ref[1].double()).abs().max(), (got_pred - ref[2].double()).abs().max()))
            assert rel < 1e-4 and dcount <= 2, (kind, B, rel, dcount)
            need = B * nvox * (4 * planes + 1)
            moved = B * nvox * (4 * planes + 1 + 3 * 4 * n_s * C)
            fm, mm = statistics.median(ms["fused"]), statistics.median(ms["mat"])
            res = {"kind": kind, "B": B, "size": size, "C": C, "S" if kind == "ssn" else "T": n_s, "fused_ms": round(fm, 4),
                   "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)], "fused_gbps": round(need / fm / 1e6, 1),
                   "hbm_floor_ms": round(need / (a.hbm_tbps * 1e9), 4), "mat_ms": round(mm, 4),
                   "mat_ms_min_max": [round(min(ms["mat"]), 4), round(max(ms["mat"]), 4)], "mat_gbps": round(moved / mm / 1e6, 1),
                   "ratio": round(mm / fm, 2), "iters": iters, "rounds": a.rounds, "ll_rel_diff": rel, "count_diff": dcount}
            if kind == "ssn":
                res["R"] = R
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
