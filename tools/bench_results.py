"""Results-writer benchmark: N LIDC-shaped cases (64^3, T = 10, C = 2, the three maps, the input, 0 or 4 raters) written
to a temporary directory by the host writer (results.save_case), by the device writer (results.save_case_device) and by
the pipelined ResultsWriter, in one process on the same inputs.  Prints one JSON line:

  host_s_per_case, device_s_per_case, speedup          end to end, files on disk
  writer_cases_per_s                                   ResultsWriter over the N cases (close() included)
  gpu_payload_ms, gpu_encode_ms (per case)             device events around vx_nifti_payload / vx_gzip_encode
  encode_gbps                                          payload bytes / encode time
  host_bytes, device_bytes, bytes_ratio                compressed tree sizes (host: zlib level 1)

  python tools/bench_results.py --cases 4 [--raters 4]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tree_bytes(d):
    return sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(d) for f in fs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=4)
    ap.add_argument("--raters", type=int, default=0, choices=(0, 4))
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--workers", type=int, default=4)
    a = ap.parse_args()
    import torch

    from tests.formula import formula_volume
    from values_amd.results import ResultsWriter, save_case, save_case_device
    from values_amd import _lib
    _lib.require_gpu()
    S, T, C = a.size, a.T, 2
    cases = []
    for i in range(a.cases):
        g = torch.Generator(device="cuda").manual_seed(100 + i)
        logits = torch.randn(T, C, S, S, S, device="cuda", generator=g) * 4
        logits[:, 1, : S // 2] -= 12   # a background half: saturated probabilities, like a real case
        sm = torch.softmax(logits, 1)
        maps = {k: torch.rand(S, S, S, device="cuda", generator=g) * 0.1 for k in
                ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")}
        img = torch.from_numpy(formula_volume((S, S, S), tag=i))
        gt = (torch.rand(a.raters, S, S, S, generator=torch.Generator().manual_seed(i)) > 0.97) if a.raters else None
        cases.append(dict(softmax_pred=sm, maps=maps, data=img, gt_seg=gt))
    root = tempfile.mkdtemp(prefix="bench_results_")
    try:
        # warm-up of every shape on the device path
        save_case_device(os.path.join(root, "warm"), "w", **cases[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, kw in enumerate(cases):
            save_case(os.path.join(root, "host"), f"c{i}", **kw)
        t_host = (time.perf_counter() - t0) / a.cases
        timing = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, kw in enumerate(cases):
            save_case_device(os.path.join(root, "dev"), f"c{i}", _timing=timing, **kw)
        t_dev = (time.perf_counter() - t0) / a.cases
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with ResultsWriter(workers=a.workers) as w:
            for i, kw in enumerate(cases):
                w.submit(os.path.join(root, "pipe"), f"c{i}", **kw)
        t_pipe = time.perf_counter() - t0
        hb, db = tree_bytes(os.path.join(root, "host")), tree_bytes(os.path.join(root, "dev"))
        enc_ms = timing["encode_ms"] / a.cases
        res = {"metric": "results_writer", "cases": a.cases, "size": S, "T": T, "C": C, "raters": a.raters,
               "files_per_case": sum(len(fs) for _, _, fs in os.walk(os.path.join(root, "dev"))) // a.cases,
               "host_s_per_case": round(t_host, 4), "device_s_per_case": round(t_dev, 4),
               "speedup": round(t_host / t_dev, 2), "writer_cases_per_s": round(a.cases / t_pipe, 2),
               "gpu_payload_ms": round(timing["payload_ms"] / a.cases, 3), "gpu_encode_ms": round(enc_ms, 3),
               "payload_mb_per_case": round(timing["payload_bytes"] / a.cases / 1e6, 2),
               "encode_gbps": round(timing["payload_bytes"] / a.cases / (enc_ms * 1e-3) / 1e9, 2),
               "host_bytes": hb, "device_bytes": db, "bytes_ratio": round(db / hb, 4)}
        print(json.dumps(res))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
