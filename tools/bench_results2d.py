"""2D results-writer benchmark: batches of street-scene-like arg-max masks (N TTA views + the mean) and three float32
uncertainty maps per image, written to a temporary directory by the host writer (results2d.save_prediction +
save_uncertainty per image), by the device writer (results2d.save_images_device) and by the pipelined ResultsWriter2D, in
one process on the same inputs.  Prints one JSON line with one entry per shape:

  host_s_per_image, device_s_per_image, writer_s_per_image    end to end, files on disk
  host_images_per_s, device_images_per_s, writer_images_per_s
  gpu_encode_ms_per_image                                     device events around vx_png_encode
  png_gbps                                                    PNG scanline bytes / encode time
  png_bytes_ratio                                             compressed PNG bytes, device / host (zlib level 3)
  tiff                                                        per TIFF leg ("none": uncompressed, the default writer;
                                                              "lzw_p1" / "lzw_p2" / "lzw_p3" with --tiff lzw), the legs
                                                              run alternately --reps times on the same inputs:
    tiff_bytes, raw_map_bytes, tiff_ratio                       strip bytes written / float32 map bytes
    gpu_predict_ms, gpu_encode_ms, gpu_pack_ms (per image)      device events around vx_tiff_predict / vx_tiff_lzw_encode /
                                                                vx_tiff_lzw_pack
    device_s_per_image, writer_s_per_image                      save_images_device / ResultsWriter2D, best of the reps
    read_s_per_map                                              images.load_tiff_device over the leg's written maps

--maps rand: uniform random maps (the worst case of a compressor); --maps hrnet: the three maps process_output_2d makes of
a randomly initialised HRNet-W18 (seed 123, as bench.py's config 4) over 8 TTA views of Gaussian images, for the
512 x 1024 shape alone.

  python tools/bench_results2d.py [--batches 4] [--workers 4] [--tiff lzw --tiff-predictor 1 2 3] [--maps hrnet]
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

SHAPES = [  # (H, W, N views, B images per batch)
    (512, 1024, 8, 8),
    (256, 478, 4, 12),    # the reference's HRNet-W48 test shape
    (1024, 2048, 8, 2),
]
UNC = ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")


def png_bytes(d):
    return sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(d) for f in fs if f.endswith(".png"))


def hrnet_maps(B, H, W, batches):
    """per batch the three uncertainty maps of B images: HRNet-W18 with random weights (seed 123) over the 8 TTA views of
    Gaussian images, through predict_logits_2d and process_output_2d"""
    import torch

    from values_amd.data import tta_views_8_device
    from values_amd.hrnet import HighResolutionNet
    from values_amd.hrnet_configs import hrnet_w18_extra
    from values_amd.predict2d import NhwcViews, predict_logits_2d, process_output_2d
    cfg = {"MODEL": {"EXTRA": hrnet_w18_extra(False), "ALIGN_CORNERS": False, "INPUT_CHANNELS": 3}, "DATASET": {"NUM_CLASSES": 19}}
    torch.manual_seed(123)
    model = HighResolutionNet(cfg).cuda()
    out = []
    for k in range(batches):
        g = torch.Generator(device="cpu").manual_seed(123 + k)
        x = torch.randn((B, 3, H, W), generator=g).cuda()
        noisy = x + 0.05 * torch.randn((B, 3, H, W), generator=g).cuda()
        d8, hf, vf = tta_views_8_device(x, noisy)
        res = process_output_2d(None, probs=predict_logits_2d([model], NhwcViews(d8, hf, vf), tta=True, softmax=True))
        out.append({u: res[u].detach().float().reshape(B, H, W).clone() for u in UNC})
    del model
    torch.cuda.empty_cache()
    return out


def tiff_legs(root, tag, data, B, batches, workers, predictors, reps):
    """the TIFF legs of one shape, alternately, `reps` times: -> {leg: figures}"""
    import torch

    from values_amd import images
    from values_amd.results2d import ResultsWriter2D, save_images_device
    legs = [("none", {})] + [(f"lzw_p{p}", {"tiff": "lzw", "tiff_predictor": p}) for p in predictors]
    for name, kw in legs:                                      # first-call costs of every leg's buffers
        save_images_device(os.path.join(root, tag, "warm_" + name), *data[0], **kw)
    out = {name: {"device_s_per_image": [], "writer_s_per_image": []} for name, _ in legs}
    for rep in range(reps):
        for name, kw in legs:
            timing = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for d in data:
                save_images_device(os.path.join(root, tag, "t_" + name), *d, _timing=timing, **kw)
            out[name]["device_s_per_image"].append((time.perf_counter() - t0) / (B * batches))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with ResultsWriter2D(workers=workers, **kw) as w:
                for d in data:
                    w.submit(os.path.join(root, tag, "tp_" + name), *d)
            out[name]["writer_s_per_image"].append((time.perf_counter() - t0) / (B * batches))
            out[name]["timing"] = timing
    res = {}
    for name, _ in legs:
        t = out[name]["timing"]
        paths = [os.path.join(root, tag, "t_" + name, u, f) for u in UNC for f in sorted(os.listdir(os.path.join(root, tag, "t_" + name, u)))]
        images.load_tiff_device(paths[:8])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        images.load_tiff_device(paths)
        torch.cuda.synchronize()
        t_read = (time.perf_counter() - t0) / len(paths)
        res[name] = {"tiff_bytes": t["tiff_bytes"], "raw_map_bytes": t["tiff_raw_bytes"],
                     "tiff_ratio": round(t["tiff_bytes"] / t["tiff_raw_bytes"], 4),
                     "gpu_predict_ms": round(t.get("tiff_predict_ms", 0.0) / (B * batches), 4),
                     "gpu_encode_ms": round(t.get("tiff_encode_ms", 0.0) / (B * batches), 4),
                     "gpu_pack_ms": round(t.get("tiff_pack_ms", 0.0) / (B * batches), 4),
                     "device_s_per_image": round(min(out[name]["device_s_per_image"]), 5),
                     "writer_s_per_image": round(min(out[name]["writer_s_per_image"]), 5),
                     "device_s_per_image_all": [round(v, 5) for v in out[name]["device_s_per_image"]],
                     "writer_s_per_image_all": [round(v, 5) for v in out[name]["writer_s_per_image"]],
                     "read_s_per_map": round(t_read, 6)}
    return res


def run_shape(root, H, W, N, B, batches, workers, predictors=(), reps=3, maps=None):
    import torch

    from tests.test_gpu_results2d_device import blocky_masks
    from values_amd.results2d import ResultsWriter2D, save_images_device, save_prediction, save_uncertainty
    data = []
    for k in range(batches):
        g = torch.Generator(device="cuda").manual_seed(k)
        pm = torch.from_numpy(blocky_masks(B, N, H, W, seed=k)).cuda()
        unc = maps[k] if maps is not None else {u: torch.rand(B, H, W, device="cuda", generator=g) * 0.5 for u in UNC}
        data.append(([f"img{k}_{b}" for b in range(B)], pm, pm[:, 0].clone(), unc))
    tag = f"{H}x{W}"
    save_images_device(os.path.join(root, "warm"), *data[0])   # first-call costs: buffers, LDS attribute, pinned memory
    torch.cuda.synchronize()
    # host: one batch (the slow leg)
    ids, pm, mean, unc = data[0]
    hd = os.path.join(root, tag, "host")
    os.makedirs(os.path.join(hd, "pred_seg"))
    t0 = time.perf_counter()
    for b, iid in enumerate(ids):
        save_prediction(os.path.join(hd, "pred_seg"), iid, pm[b], mean[b])
        save_uncertainty(hd, iid, {u: v[b] for u, v in unc.items()})
    t_host = (time.perf_counter() - t0) / B
    timing = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for d in data:
        save_images_device(os.path.join(root, tag, "dev"), *d, _timing=timing)
    t_dev = (time.perf_counter() - t0) / (B * batches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with ResultsWriter2D(workers=workers) as w:
        for d in data:
            w.submit(os.path.join(root, tag, "pipe"), *d)
    t_pipe = (time.perf_counter() - t0) / (B * batches)
    # device bytes of the host's batch only
    dev_png = sum(os.path.getsize(os.path.join(root, tag, "dev", "pred_seg", f))
                  for f in os.listdir(os.path.join(root, tag, "dev", "pred_seg")) if f.startswith("img0_"))
    enc_ms = timing["encode_ms"] / (B * batches)
    tiff = tiff_legs(root, tag, data, B, batches, workers, predictors, reps) if predictors else None
    return {"H": H, "W": W, "views": N, "B": B, "batches": batches, "files_per_image": N + 1 + len(UNC),
            "host_s_per_image": round(t_host, 5), "device_s_per_image": round(t_dev, 5),
            "writer_s_per_image": round(t_pipe, 5), "host_images_per_s": round(1 / t_host, 1),
            "device_images_per_s": round(1 / t_dev, 1), "writer_images_per_s": round(1 / t_pipe, 1),
            "gpu_encode_ms_per_image": round(enc_ms, 3),
            "png_gbps": round(timing["raw_bytes"] / (timing["encode_ms"] * 1e-3) / 1e9, 2),
            "png_bytes_ratio": round(dev_png / png_bytes(hd), 4), "maps": "hrnet" if maps is not None else "rand",
            "tiff_raw_map_bytes": timing["tiff_raw_bytes"], "tiff_bytes": timing["tiff_bytes"], "tiff": tiff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--tiff", choices=("none", "lzw"), default="none")
    ap.add_argument("--tiff-predictor", type=int, nargs="+", choices=(1, 2, 3), default=[3])
    ap.add_argument("--reps", type=int, default=3, help="repetitions of the alternating TIFF legs")
    ap.add_argument("--maps", choices=("rand", "hrnet"), default="rand")
    a = ap.parse_args()
    from values_amd import _lib
    _lib.require_gpu()
    root = tempfile.mkdtemp(prefix="bench_results2d_")
    predictors = a.tiff_predictor if a.tiff == "lzw" else ()
    try:
        if a.maps == "hrnet":
            H, W, N, B = SHAPES[0]
            res = [run_shape(root, H, W, N, B, a.batches, a.workers, predictors, a.reps, hrnet_maps(B, H, W, a.batches))]
        else:
            res = [run_shape(root, H, W, N, B, a.batches, a.workers, predictors, a.reps) for H, W, N, B in SHAPES]
        print(json.dumps({"metric": "results_writer_2d", "shapes": res}))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
