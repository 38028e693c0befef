"""The 2D preprocessing step (values_amd.preprocess2d) on synthetic raw data sets the tool writes itself, host mirror
against the device route, in one process:

  cityscapes   1024 x 2048 RGB images with grey label-id files, the Cityscapes folder layout
  gta          1052 x 1914 RGB images with 8-bit palette label files, the GTA5 folder layout

One JSON line per data set:

  host_s_per_image, device_s_per_image   wall clock of preprocess_dataset_2d(device_io=False / True) over the case count:
                                         files read, four files per case written, final synchronise included (the device
                                         route: min of --wall-reps runs into fresh directories after one warm-up run; the
                                         host mirror runs once); device_images_per_s is the inverse
  stage_ms_per_batch                     GPU time per batch of --batch cases between device events around each stage of
                                         the device route, over all batches of the last run: inflate (vx_inflate),
                                         unfilter (vx_png_unfilter), crop_resize (vx_crop_resize_batched), png_encode
                                         (vx_png_encode_rgb); bound_by names the largest
  crop_resize_ms                         one vx_crop_resize_batched call (table upload, status memset, kernel) over a
                                         decoded batch resident on the device: device events around 20 calls issued back
                                         to back, over 20; [min, max] of --reps such windows after one warm-up
  tap_bytes, row_bytes                   what that call must move: tap_bytes = the source bytes of the taps (4 per output
                                         pixel and channel for the linear mode, 1 pixel for the nearest modes) plus every
                                         output byte; row_bytes = the source rows those taps lie in, read in full (two of
                                         every four rows for the image, one of four for the labels), plus the outputs
  crop_resize_gbs                        tap_bytes and row_bytes over the call's min time
  roofline_ms                            both byte counts over 8 TB/s

  python tools/bench_preprocess2d.py [--datasets cityscapes,gta] [--count 16] [--batch 8] [--distinct N] [--reps 10]
                                     [--wall-reps 2] [--skip-host] [--root DIR]
"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cityscapes": (1024, 2048), "gta": (1052, 1914)}
CALLS = 20   # vx_crop_resize_batched calls per timed window


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_palette_png(path, idx, palette):
    """an 8-bit palette PNG (colour type 3), filter 0 on every row -- image_io.write_png with a PLTE chunk"""
    import numpy as np
    h, w = idx.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), idx], axis=1).tobytes()
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 3, 0, 0, 0)))
        f.write(_chunk(b"PLTE", np.ascontiguousarray(palette, np.uint8).tobytes()) + _chunk(b"IDAT", zlib.compress(raw, 3)) + _chunk(b"IEND", b""))


def write_raw(root, dataset, count, distinct=None):
    """photo-like images (smooth ramps with sensor noise) and label maps of rectangular regions; beyond the first
    `distinct` cases a case is a copy of an earlier one's files (the timing does not care, the generation does)"""
    import shutil

    import numpy as np
    from values_amd import gta
    from values_amd.image_io import write_png
    h, w = SHAPES[dataset]
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:h, 0:w]
    colours = np.array(list(gta.COLOR2TRAINID), dtype=np.uint8)
    if dataset == "cityscapes":
        image_dir = os.path.join(root, "images", "leftImg8bit", "train", "city")
        label_dir = os.path.join(root, "labels", "gtFine", "train", "city")
        os.makedirs(os.path.join(root, "images", "leftImg8bit", "val"))
    else:
        image_dir, label_dir = os.path.join(root, "images"), os.path.join(root, "labels")
    os.makedirs(image_dir)
    os.makedirs(label_dir)
    def names(i):
        if dataset == "cityscapes":
            return (os.path.join(image_dir, f"city_{i:06d}_000019_leftImg8bit.png"), os.path.join(label_dir, f"city_{i:06d}_000019_gtFine_labelIds.png"))
        return os.path.join(image_dir, f"{i + 1:05d}.png"), os.path.join(label_dir, f"{i + 1:05d}.png")
    distinct = count if distinct is None else max(1, min(distinct, count))
    for i in range(distinct):
        base = np.stack([(xx // 3 + yy // 5 + 40 * c + 17 * i) % 256 for c in range(3)], -1)
        image = np.clip(base + rng.integers(-6, 7, base.shape), 0, 255).astype(np.uint8)
        regions = rng.integers(0, 34 if dataset == "cityscapes" else len(colours), (h // 64 + 1, w // 64 + 1)).astype(np.uint8)
        labels = np.ascontiguousarray(regions.repeat(64, 0).repeat(64, 1)[:h, :w])
        write_png(names(i)[0], image)
        if dataset == "cityscapes":
            write_png(names(i)[1], labels)
        else:
            write_palette_png(names(i)[1], labels, colours)
    for i in range(distinct, count):
        for src, dst in zip(names(i % distinct), names(i)):
            shutil.copyfile(src, dst)


def kernel_times(root, dataset, batch, reps):
    """one vx_crop_resize_batched call over the first batch, decoded and resident -> ([min, max] ms, tap bytes, row bytes)"""
    import torch
    from values_amd import preprocess2d as p2d
    cases = p2d.list_cases(root, os.path.join(root, "nowhere"), dataset)[:batch]
    with p2d.Preprocess2DReader() as reader:
        decoded = next(iter(reader.read([[(c[2], c[3]) for c in cases]])))
    dev = decoded[0][0].device
    tap = row = 0
    for img, lab, _, _ in decoded:
        _, _, ch, cw = p2d.center_crop_box(int(img.shape[0]), int(img.shape[1]))
        oh, ow = p2d.out_size(ch, 4), p2d.out_size(cw, 4)
        ibpp, lbpp = int(img.shape[2]), (1 if lab.dim() == 2 else int(lab.shape[2]))
        out = oh * ow * (3 + 3 + (1 if dataset == "cityscapes" else 8))
        tap += oh * ow * (4 * ibpp + lbpp) + out
        row += oh * cw * (2 * ibpp + lbpp) + out
    arr, arena, outs, _, pal_dev = p2d._plan_batch(decoded, dataset, p2d.CROP, p2d.FACTOR, dev)
    status = torch.empty(2 * len(decoded), dtype=torch.int32, device=dev)
    ms = []
    for rep in range(reps + 1):            # the first repetition warms the call up
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        for _ in range(CALLS):             # back to back: the window is the device's time once the queue is ahead of it
            p2d._crop_resize_call(arr, 2 * len(decoded), status, dev)
        e[1].record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e[0].elapsed_time(e[1]) / CALLS)
    assert not status.cpu().any()
    return [min(ms), max(ms)], tap, row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="cityscapes,gta")
    ap.add_argument("--count", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--distinct", type=int, default=None, help="generate this many cases, the rest are copies of them")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--wall-reps", type=int, default=2)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--root", default=None)
    args = ap.parse_args()
    import torch
    from values_amd import preprocess_dataset_2d
    assert torch.cuda.is_available(), "bench_preprocess2d.py needs a GPU"
    for dataset in args.datasets.split(","):
        with tempfile.TemporaryDirectory(dir=args.root) as d:
            root = os.path.join(d, "raw")
            write_raw(root, dataset, args.count, args.distinct)
            line = {"dataset": dataset, "count": args.count, "batch": args.batch, "shape": list(SHAPES[dataset])}
            if not args.skip_host:
                t0 = time.perf_counter()
                assert preprocess_dataset_2d(root, os.path.join(d, "host"), dataset) == 0
                line["host_s_per_image"] = (time.perf_counter() - t0) / args.count
            preprocess_dataset_2d(root, os.path.join(d, "warm"), dataset, device_io=True, batch=args.batch)
            best, timing = None, {}
            for rep in range(args.wall_reps):
                timing = {}
                t0 = time.perf_counter()
                preprocess_dataset_2d(root, os.path.join(d, f"dev{rep}"), dataset, device_io=True, batch=args.batch, _timing=timing)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            line["device_s_per_image"] = best / args.count
            line["device_images_per_s"] = args.count / best
            n_batches = -(-args.count // args.batch)
            stages = {k[:-3]: timing.get(k, 0.0) / n_batches for k in ("inflate_ms", "unfilter_ms", "crop_resize_ms", "png_encode_ms")}
            line["stage_ms_per_batch"] = stages
            line["bound_by"] = max(stages, key=stages.get)
            ms, tap, row = kernel_times(root, dataset, args.batch, args.reps)
            line.update(crop_resize_ms=ms, tap_bytes=tap, row_bytes=row)
            line["crop_resize_gbs"] = {"tap": tap / (ms[0] * 1e-3) / 1e9, "row": row / (ms[0] * 1e-3) / 1e9} if ms[0] > 0 else None
            line["roofline_ms"] = {"tap": tap / 8e12 * 1e3, "row": row / 8e12 * 1e3}
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
