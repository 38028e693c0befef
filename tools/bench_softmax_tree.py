"""Softmax-tree benchmark: N cases (size^3, C classes, T = 1: the plain Softmax model) written to a temporary directory
by ResultsWriter, copied, and the tree's pred_entropy/ set up on each copy by the host ExperimentDataloader and by
DeviceExperimentDataloader, in one process:

  host_s_per_image, device_s_per_image, *_images_per_s   constructing the dataloader (a warm-up copy is built first)
  same                                                   the two pred_entropy/ trees hold the same decoded bytes
  kernel_ms, kernel_gbps      one vx_one_minus_msr_batched call over --per-call images (device events around --iters calls of
                              the entry point back to back, tables built once), over (C + 1) * n * esize bytes per image;
                              call_ms: the same through uncertainty.one_minus_msr_batch (with its Python per image)
  reader_inflate_ms, reader_decode_ms, encoder_payload_ms, encoder_gzip_ms   device events, per image
  step2d_ms, step2d_parent_ms   process_output_2d(T = 1) at B = 8 (19 classes, --h x --w) against the same step with the
                                B launches of vx_one_minus_msr it made before; step2d_same: equal bits

  python tools/bench_softmax_tree.py --cases 16 --per-call 16
"""
import argparse
import gzip
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
    ap.add_argument("--cases", type=int, default=16)
    ap.add_argument("--per-call", type=int, default=16)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--h", type=int, default=512)
    ap.add_argument("--w", type=int, default=1024)
    a = ap.parse_args()
    import torch

    from values_amd import _lib, nifti, uncertainty
    from values_amd.experiment import DeviceExperimentDataloader, ExperimentDataloader, ExperimentVersion
    from values_amd.predict2d import process_output_2d
    from values_amd.results import ResultsWriter, results_dir, save_maps_device
    _lib.require_gpu()
    lib = _lib.load()
    S, C = a.size, a.classes
    root = tempfile.mkdtemp(prefix="bench_softmax_tree_")

    def version(base):
        return ExperimentVersion(base_path=base, naming_scheme_version="fold{fold}", pred_model="Softmax", image_ending=".nii.gz",
                                 unc_ending=".nii.gz", unc_types=["predictive_uncertainty"], aggregations=None,
                                 n_reference_segs=0, n_classes=C, fold=0)

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    try:
        d = results_dir(os.path.join(root, "src"), "Softmax", "fold0", "id")
        with ResultsWriter(workers=4) as w:
            for i in range(a.cases):
                g = torch.Generator(device="cuda").manual_seed(100 + i)
                logits = torch.randn(1, C, S, S, S, device="cuda", generator=g) * 4
                logits[:, 1:, : S // 2] -= 12
                w.submit(d, f"c{i}", torch.softmax(logits, 1))
        for name in ("warm_host", "warm_dev", "host", "dev"):
            shutil.copytree(os.path.join(root, "src"), os.path.join(root, name))
        DeviceExperimentDataloader.softmax_chunk = a.per_call
        ExperimentDataloader(version(os.path.join(root, "warm_host")), "id")
        DeviceExperimentDataloader(version(os.path.join(root, "warm_dev")), "id")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hdl = ExperimentDataloader(version(os.path.join(root, "host")), "id")
        torch.cuda.synchronize()
        t_host = (time.perf_counter() - t0) / a.cases
        t0 = time.perf_counter()
        ddl = DeviceExperimentDataloader(version(os.path.join(root, "dev")), "id")
        torch.cuda.synchronize()
        t_dev = (time.perf_counter() - t0) / a.cases
        same = all(gzip.decompress(open(hdl.dataset_path / "pred_entropy" / n, "rb").read())
                   == gzip.decompress(open(ddl.dataset_path / "pred_entropy" / n, "rb").read())
                   for n in sorted(os.listdir(hdl.dataset_path / "pred_entropy")))
        # the pieces: reader, kernel, encoder over one chunk
        ids = ddl.image_ids[:a.per_call]
        files = [p for i in ids for p in ddl._prob_paths(i)]
        nifti.load_device(files)
        rt = {}
        planes = [t for t, _ in nifti.load_device(files, _timing=rt)]
        images = [planes[k * C:(k + 1) * C] for k in range(len(ids))]
        call_ms = timed(lambda: uncertainty.one_minus_msr_batch(images), a.iters)
        maps = uncertainty.one_minus_msr_batch(images)
        k_bytes = sum((C + 1) * m.numel() * m.element_size() for m in maps)
        # the kernel alone: the entry point called back to back with tables built once (no Python per image in the loop)
        dt = _lib.VX_F64 if maps[0].dtype == torch.float64 else _lib.VX_F32
        items, table, n_planes = uncertainty.msr_tables([(m.data_ptr(), m.numel(), dt, [p.data_ptr() for p in ps])
                                                         for m, ps in zip(maps, images)])
        ws = _lib.workspace(maps[0].device, int(lib.vx_one_minus_msr_batched_workspace_bytes(len(maps), n_planes)))
        k_ms = timed(lambda: _lib.check(lib.vx_one_minus_msr_batched(items, len(maps), table, n_planes, _lib.ptr(ws), ws.numel(),
                                                                     _lib.stream_ptr()), "vx_one_minus_msr_batched"), a.iters)
        out_dir = os.path.join(root, "enc")
        os.makedirs(out_dir)
        paths = [os.path.join(out_dir, f"{i}.nii.gz") for i in ids]
        save_maps_device(paths, maps)
        et = {}
        save_maps_device(paths, maps, _timing=et)
        # the 2D step: T = 1, B = 8
        B, C2 = 8, 19
        probs = torch.softmax(torch.randn(B, 1, C2, a.h, a.w, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)), 2)

        def parent_step():
            m = uncertainty.uncertainty_maps(probs, from_logits=False)
            msr = torch.empty((B, a.h, a.w), dtype=torch.float32, device=probs.device)
            for b in range(B):
                _lib.check(lib.vx_one_minus_msr(_lib.ptr(probs[b, 0]), _lib.VX_F32, C2, a.h * a.w, _lib.ptr(msr[b]), _lib.stream_ptr()),
                           "vx_one_minus_msr")
            return msr
        step_same = torch.equal(process_output_2d(None, probs=probs)["pred_entropy"].view(torch.int32), parent_step().view(torch.int32))
        s_new, s_old = [], []
        for _ in range(3):      # alternating: other work shares the machine
            s_new.append(timed(lambda: process_output_2d(None, probs=probs), a.iters))
            s_old.append(timed(parent_step, a.iters))
        n = len(ids)
        res = {"metric": "softmax_tree", "cases": a.cases, "per_call": a.per_call, "size": S, "classes": C,
               "host_s_per_image": round(t_host, 5), "device_s_per_image": round(t_dev, 5),
               "host_images_per_s": round(1 / t_host, 2), "device_images_per_s": round(1 / t_dev, 2),
               "speedup": round(t_host / t_dev, 2), "same": same,
               "call_ms": round(call_ms, 4), "kernel_ms": round(k_ms, 4), "kernel_gbps": round(k_bytes / (k_ms * 1e-3) / 1e9, 1), "kernel_mb": round(k_bytes / 1e6, 2),
               "reader_inflate_ms": round(rt["inflate_ms"] / n, 4), "reader_decode_ms": round(rt["decode_ms"] / n, 4),
               "encoder_payload_ms": round(et["payload_ms"] / n, 4), "encoder_gzip_ms": round(et["encode_ms"] / n, 4),
               "step2d_shape": [B, 1, C2, a.h, a.w], "step2d_ms": round(min(s_new), 4), "step2d_parent_ms": round(min(s_old), 4),
               "step2d_ms_all": [round(v, 4) for v in s_new], "step2d_parent_ms_all": [round(v, 4) for v in s_old],
               "step2d_same": step_same}
        print(json.dumps(res))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
