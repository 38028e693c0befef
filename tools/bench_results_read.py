"""Results-reader benchmark: N LIDC-shaped cases (64^3, T = 10, C = 2, the three maps, the input; as
tools/bench_results.py) written to a temporary directory by ResultsWriter (or, with --host-writer, by the host writer
save_case: zlib level 1), then read back in one process:

  host_s_per_case                        nifti.load over every file of a case, one after another
  device_s_per_case, reader_s_per_case   nifti.load_device / nifti.NiftiReader, --per-call cases per call
  *_gbps                                 decoded payload bytes / time
  gpu_inflate_ms, gpu_decode_ms          device events around vx_inflate / vx_nifti_decode, per case
  agg_host_s, agg_device_s, agg_same     aggregate_uncertainties vs aggregate_uncertainties_device on the tree (the JSON
                                         files compared byte for byte)

  python tools/bench_results_read.py --cases 8 --per-call 8 [--host-writer]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=8)
    ap.add_argument("--per-call", type=int, default=8)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--host-writer", action="store_true")
    a = ap.parse_args()
    import torch

    from tests.formula import formula_volume
    from values_amd import _lib, nifti
    from values_amd.experiment import (DeviceExperimentDataloader, ExperimentDataloader, ExperimentVersion,
                                       aggregate_uncertainties, aggregate_uncertainties_device)
    from values_amd.results import ResultsWriter, results_dir, save_case
    _lib.require_gpu()
    S, T, C = a.size, a.T, 2
    root = tempfile.mkdtemp(prefix="bench_results_read_")
    try:
        d = results_dir(root, "Dropout", "fold0_seed123", "id")
        w = None if a.host_writer else ResultsWriter(workers=4)
        for i in range(a.cases):
            g = torch.Generator(device="cuda").manual_seed(100 + i)
            logits = torch.randn(T, C, S, S, S, device="cuda", generator=g) * 4
            logits[:, 1, : S // 2] -= 12
            sm = torch.softmax(logits, 1)
            maps = {k: torch.rand(S, S, S, device="cuda", generator=g) * 0.1 for k in
                    ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")}
            kw = dict(softmax_pred=sm, maps=maps, data=torch.from_numpy(formula_volume((S, S, S), tag=i)))
            if w is None:
                save_case(d, f"c{i}", **kw)
            else:
                w.submit(d, f"c{i}", **kw)
        if w is not None:
            w.close()
        files = {}
        for r, _, fs in os.walk(d):
            for f in fs:
                if f.endswith(".nii.gz"):
                    files.setdefault(f.split("_")[0].split(".")[0], []).append(os.path.join(r, f))
        cases = [sorted(files[f"c{i}"]) for i in range(a.cases)]
        n_files = sum(len(c) for c in cases)
        batches = [sum(cases[i:i + a.per_call], []) for i in range(0, a.cases, a.per_call)]
        # warm-up: every shape, the pool, the pinned buffer
        nifti.load_device(batches[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        payload = 0
        for c in cases:
            for p in c:
                arr, _ = nifti.load(p)
                payload += arr.nbytes + 352
        t_host = (time.perf_counter() - t0) / a.cases
        timing = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in batches:
            nifti.load_device(b, _timing=timing)
        torch.cuda.synchronize()
        t_dev = (time.perf_counter() - t0) / a.cases
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with nifti.NiftiReader() as r:
            for _ in r.read(batches):
                pass
        torch.cuda.synchronize()
        t_rd = (time.perf_counter() - t0) / a.cases
        # aggregation over the tree
        ev = ExperimentVersion(base_path=root, naming_scheme_version="fold{fold}_seed{seed}", pred_model="Dropout",
                               image_ending=".nii.gz", unc_ending=".nii.gz",
                               unc_types=["predictive_uncertainty", "aleatoric_uncertainty", "epistemic_uncertainty"],
                               aggregations=None, n_reference_segs=0, fold=0, seed=123)
        aggs = {"patch_level": {"_target_": "values_amd.aggregation.patch_level_aggregation", "patch_size": 10},
                "image_level": {"_target_": "values_amd.aggregation.image_level_aggregation", "mean": True},
                "threshold": {"_target_": "values_amd.aggregation.threshold_aggregation", "threshold": 0.05}}
        hdl, ddl = ExperimentDataloader(ev, "id"), DeviceExperimentDataloader(ev, "id")
        t0 = time.perf_counter()
        aggregate_uncertainties(hdl, aggs)
        t_agg_h = time.perf_counter() - t0
        want = {u: open(hdl.dataset_path / f"aggregated_{u}.json", "rb").read() for u in ev.unc_types}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aggregate_uncertainties_device(ddl, aggs, batch=max(1, 3 * a.per_call))
        torch.cuda.synchronize()
        t_agg_d = time.perf_counter() - t0
        same = all(open(hdl.dataset_path / f"aggregated_{u}.json", "rb").read() == want[u] for u in ev.unc_types)
        gb = payload / a.cases / 1e9
        res = {"metric": "results_reader", "cases": a.cases, "per_call": a.per_call, "size": S, "T": T,
               "writer": "host" if a.host_writer else "device", "files_per_case": n_files // a.cases,
               "payload_mb_per_case": round(payload / a.cases / 1e6, 2),
               "host_s_per_case": round(t_host, 4), "device_s_per_case": round(t_dev, 4),
               "reader_s_per_case": round(t_rd, 4), "speedup": round(t_host / t_dev, 2),
               "reader_speedup": round(t_host / t_rd, 2),
               "host_gbps": round(gb / t_host, 3), "device_gbps": round(gb / t_dev, 3), "reader_gbps": round(gb / t_rd, 3),
               "gpu_inflate_ms": round(timing["inflate_ms"] / a.cases, 3),
               "gpu_decode_ms": round(timing["decode_ms"] / a.cases, 3),
               "agg_host_s": round(t_agg_h, 4), "agg_device_s": round(t_agg_d, 4), "agg_same": same}
        print(json.dumps(res))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
