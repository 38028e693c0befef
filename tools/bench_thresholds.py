"""The threshold task of the evaluation stage (values_amd.thresholds) on a synthetic split written with the project's own
writers -- "3d": .nii.gz maps and masks (results.ResultsWriter), "2d": TIFF maps and PNG masks
(results2d.save_images_device) -- in three legs, in one process:

  host      ExperimentDataloader + get_foreground_quantile, find_threshold(loader=experiment._load_file)
  single    the single-array forms: DeviceExperimentDataloader + get_foreground_quantile (thresholds.count_nonzero per mask:
            one vx_count_nonzero_batched call of one item and one host copy each), and for the thresholds the maps read on
            the device, cast to float32, joined with torch.cat and handed to thresholds.quantile (one vx_select_segments
            call over the one joined array), restated over experiment._read_batches_device for every kind of file.
  new       get_foreground_quantile_device (one count_nonzero_batch call per reader batch) and
            find_threshold(device_io=True) (one quantile_segments call per uncertainty type over the tensors as read)

The three legs must write the same quantile_analysis.json and threshold_analysis.json (compared before anything is
reported).  One JSON line per (case, leg):

  quantile_wall_s, threshold_wall_s   host clock around the two drivers, files read from disk, final synchronise included
                                      (min and max of --wall-reps runs; the host leg runs once)
and one JSON line per case with the device calls alone, on masks / maps already resident on the device:
  count_ms, select_ms                 {"single": [min, max], "new": [min, max]} of --reps repetitions, device events around
                                      all count calls of the split's masks / the quantile of ONE uncertainty type
  count_ratio, select_ratio           single min / new min (above 1: the batched path is faster)
  launches_per_type                   kernel launches and other stream operations of one uncertainty type's quantile,
                                      counted from the launchers: single = per-map cast / gather copies + cat + what new
                                      takes; new = memset + table upload + 8 kernels
  count_launches                      single: one launch, one memset, one table upload and one host copy per mask; new: the
                                      same per batch
  extra_bytes                         peak device bytes allocated during one uncertainty type's quantile beyond the maps
                                      themselves (torch's allocator statistics; the workspace is allocated inside)

  python tools/bench_thresholds.py [--cases 3d,2d] [--images-3d 64] [--size-3d 64] [--images-2d 512] [--hw 256 478]
                                   [--masks 2] [--batch 32] [--reps 5] [--wall-reps 3] [--skip-host] [--root DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TYPES = ["predictive_uncertainty", "aleatoric_uncertainty", "epistemic_uncertainty"]
NAMES = ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")


def write_3d(root, images, size, masks):
    import torch
    from values_amd.results import ResultsWriter, results_dir
    d = results_dir(root, "Dropout", "fold0_seed1", "val")
    with ResultsWriter(workers=4) as w:
        for i in range(images):
            g = torch.Generator(device="cuda").manual_seed(i)
            logits = torch.randn(masks, 2, size, size, size, device="cuda", generator=g) * 3
            logits[:, 0] += 6                                  # a small foreground: the quantile lies high, as in a real split
            sm = torch.softmax(logits, 1)
            maps = {}
            for k in NAMES:      # an uncertainty map: zero over most of the volume
                m = torch.rand(size, size, size, device="cuda", generator=g)
                maps[k] = torch.where(m > 0.6, (m - 0.6) * 1.5, torch.zeros_like(m))
            w.submit(d, f"case{i:04d}", softmax_pred=sm, maps=maps)
    return dict(naming_scheme_version="fold{fold}_seed{seed}", image_ending=".nii.gz", unc_ending=".nii.gz", fold=0, seed=1)


def write_2d(root, images, hw, masks, chunk=32):
    import torch
    from values_amd import results2d
    d = os.path.join(root, "Dropout", "test_results", "seed1", "val")
    g = torch.Generator(device="cuda").manual_seed(2)
    for b0 in range(0, images, chunk):
        n = min(chunk, images - b0)
        ids = [f"img{b0 + i:05d}" for i in range(n)]
        pm = torch.randint(0, 24, (n, masks) + hw, device="cuda", generator=g, dtype=torch.uint8)
        mm = torch.randint(0, 24, (n,) + hw, device="cuda", generator=g, dtype=torch.uint8)
        unc = {}
        for k in NAMES:
            m = torch.rand((n,) + hw, device="cuda", generator=g)
            unc[k] = torch.where(m > 0.2, (m - 0.2) * 0.6, torch.zeros_like(m))
        results2d.save_images_device(d, ids, pm, mm, unc)
    return dict(naming_scheme_version="seed{seed}", image_ending=".png", unc_ending=".tif", seed=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="3d,2d")
    ap.add_argument("--images-3d", type=int, default=64)
    ap.add_argument("--size-3d", type=int, default=64)
    ap.add_argument("--images-2d", type=int, default=512)
    ap.add_argument("--hw", type=int, nargs=2, default=(256, 478))
    ap.add_argument("--masks", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wall-reps", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--root", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from values_amd import _lib, thresholds as th
    from values_amd.experiment import (DeviceExperimentDataloader, ExperimentDataloader, ExperimentVersion, _load_file,
                                       _read_batches_device)
    _lib.require_gpu()

    def wall(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return out, [round(min(ts), 4), round(max(ts), 4)]

    def events(fn, reps):
        fn()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return [round(min(ms), 4), round(max(ms), 4)]

    def single_find_threshold(paths, qdir, out_dir):
        """find_threshold over the single-array form, for every kind of file: cast, torch.cat, thresholds.quantile"""
        flat = {(pm, unc): p for pm, vs in paths.items() for v in vs.values() for unc, p in v.items()}
        with open(os.path.join(qdir, "quantile_analysis.json")) as f:
            qs = json.load(f)
        td = {}
        for (pm, unc), ps in flat.items():
            maps = torch.cat([t.reshape(-1).to(torch.float32) for _, t in _read_batches_device(ps, a.batch)])
            td.setdefault(pm, {})[f"Mean {unc.split('_')[0]} threshold"] = th.quantile(maps, qs[pm])
        td["Mean"] = {f"Mean {k} threshold": float(np.mean([v[f"Mean {k} threshold"] for v in td.values()]))
                      for k in ("aleatoric", "epistemic", "predictive")}      # (find_threshold's order; no Softmax model here)
        with open(os.path.join(out_dir, "threshold_analysis.json"), "w") as f:
            json.dump(td, f, indent=2)

    with tempfile.TemporaryDirectory(dir=a.root) as tmp:
        for case in a.cases.split(","):
            root = os.path.join(tmp, case)
            if case == "3d":
                kw = write_3d(root, a.images_3d, a.size_3d, a.masks)
                shape, images = [a.size_3d] * 3, a.images_3d
            else:
                kw = write_2d(root, a.images_2d, tuple(a.hw), a.masks)
                shape, images = list(a.hw), a.images_2d
            torch.cuda.synchronize()
            ev = ExperimentVersion(base_path=root, pred_model="Dropout", unc_types=TYPES, aggregations=None, n_reference_segs=1, **kw)
            host, dev = ExperimentDataloader(ev, "val"), DeviceExperimentDataloader(ev, "val")
            paths = th.threshold_images_paths(host)
            legs = {"host": (lambda: th.get_foreground_quantile(host), lambda d: th.find_threshold(paths, d, d, loader=_load_file)),
                    "single": (lambda: th.get_foreground_quantile(dev), lambda d: single_find_threshold(paths, d, d)),
                    "new": (lambda: th.get_foreground_quantile_device(dev, batch=a.batch),
                            lambda d: th.find_threshold(paths, d, d, device_io=True, batch=a.batch))}
            if a.skip_host:
                del legs["host"]
            files, lines = {}, []
            for leg, (quant, thr) in legs.items():
                d = os.path.join(tmp, f"{case}_{leg}")
                os.makedirs(d)
                reps = 1 if leg == "host" else a.wall_reps
                q, tq = wall(quant, reps)
                th.save_foreground_quantiles(q, d)
                _, tt = wall(lambda: thr(d), reps)
                files[leg] = [open(os.path.join(d, f), "rb").read() for f in ("quantile_analysis.json", "threshold_analysis.json")]
                lines.append({"case": case, "leg": leg, "images": images, "shape": shape, "masks_per_image": a.masks + 1,
                              "quantile_wall_s": tq, "threshold_wall_s": tt})
            # the legs' own "Mean" entry: the single-array restatement has one pred model, as find_threshold has here
            assert all(f == files["new"] for f in files.values()), f"{case}: the legs wrote different files"
            for line in lines:
                print(json.dumps(line), flush=True)

            # the device calls alone, on resident tensors
            mask_paths = [str(p) for i in host.image_ids for p in host.get_pred_seg_paths(i)]
            masks = [t for _, t in _read_batches_device(mask_paths, a.batch)]
            maps = [t for _, t in _read_batches_device(paths["Dropout"][ev.version_name][TYPES[0]], a.batch)]
            q = json.loads(files["new"][0])["Dropout"]
            single_count = lambda: [th.count_nonzero(m) for m in masks]
            new_count = lambda: [c for i in range(0, len(masks), a.batch) for c in th.count_nonzero_batch(masks[i:i + a.batch])]
            single_select = lambda: th.quantile(torch.cat([t.reshape(-1).to(torch.float32) for t in maps]), q)
            new_select = lambda: th.quantile_segments(maps, q)
            assert single_count() == new_count() and single_select() == new_select(), f"{case}: the device calls differ"
            extra = {}
            for name, fn in (("single", single_select), ("new", new_select)):
                _lib._ws.clear()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fn()
                torch.cuda.synchronize()
                extra[name] = int(torch.cuda.max_memory_allocated() - base)
            cm = {"single": events(single_count, a.reps), "new": events(new_count, a.reps)}
            sm = {"single": events(single_select, a.reps), "new": events(new_select, a.reps)}
            copies = sum(1 for t in maps if not (t.is_contiguous() and t.dtype == torch.float32))
            batches = -(-len(masks) // a.batch)
            print(json.dumps({
                "case": case, "leg": "device calls", "masks": len(masks), "maps_per_type": len(maps), "map_dtype": str(maps[0].dtype),
                "map_bytes_per_type": sum(t.numel() * t.element_size() for t in maps),
                "count_ms": cm, "count_ratio": round(cm["single"][0] / cm["new"][0], 2),
                "select_ms": sm, "select_ratio": round(sm["single"][0] / sm["new"][0], 2),
                "launches_per_type": {"single": copies + 1 + 10, "new": 10},
                "count_launches": {"single": {"launches": len(masks), "memsets": len(masks), "table_uploads": len(masks), "host_copies": len(masks)},
                                   "new": {"launches": batches, "memsets": batches, "table_uploads": batches, "host_copies": batches}},
                "extra_bytes": extra}), flush=True)


if __name__ == "__main__":
    main()
