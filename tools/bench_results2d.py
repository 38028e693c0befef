"""2D results-writer benchmark: batches of street-scene-like arg-max masks (N TTA views + the mean) and three float32
uncertainty maps per image, written to a temporary directory by the host writer (results2d.save_prediction +
save_uncertainty per image), by the device writer (results2d.save_images_device) and by the pipelined ResultsWriter2D, in
one process on the same inputs.  Prints one JSON line with one entry per shape:

  host_s_per_image, device_s_per_image, writer_s_per_image    end to end, files on disk
  host_images_per_s, device_images_per_s, writer_images_per_s
  gpu_encode_ms_per_image                                     device events around vx_png_encode
  png_gbps                                                    PNG scanline bytes / encode time
  png_bytes_ratio                                             compressed PNG bytes, device / host (zlib level 3)

  python tools/bench_results2d.py [--batches 4] [--workers 4]
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


def run_shape(root, H, W, N, B, batches, workers):
    import torch

    from tests.test_gpu_results2d_device import blocky_masks
    from values_amd.results2d import ResultsWriter2D, save_images_device, save_prediction, save_uncertainty
    data = []
    for k in range(batches):
        g = torch.Generator(device="cuda").manual_seed(k)
        pm = torch.from_numpy(blocky_masks(B, N, H, W, seed=k)).cuda()
        unc = {u: torch.rand(B, H, W, device="cuda", generator=g) * 0.5 for u in UNC}
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
    return {"H": H, "W": W, "views": N, "B": B, "batches": batches, "files_per_image": N + 1 + len(UNC),
            "host_s_per_image": round(t_host, 5), "device_s_per_image": round(t_dev, 5),
            "writer_s_per_image": round(t_pipe, 5), "host_images_per_s": round(1 / t_host, 1),
            "device_images_per_s": round(1 / t_dev, 1), "writer_images_per_s": round(1 / t_pipe, 1),
            "gpu_encode_ms_per_image": round(enc_ms, 3),
            "png_gbps": round(timing["raw_bytes"] / (timing["encode_ms"] * 1e-3) / 1e9, 2),
            "png_bytes_ratio": round(dev_png / png_bytes(hd), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--workers", type=int, default=4)
    a = ap.parse_args()
    from values_amd import _lib
    _lib.require_gpu()
    root = tempfile.mkdtemp(prefix="bench_results2d_")
    try:
        res = [run_shape(root, H, W, N, B, a.batches, a.workers) for H, W, N, B in SHAPES]
        print(json.dumps({"metric": "results_writer_2d", "shapes": res}))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
