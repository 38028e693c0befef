"""2D results-reader benchmark: 256 x 478 files of the 2D tree (coloured label masks as PNG in three encodings -- filter 0 on
every row as this project writes them, all-Sub as OpenCV writes a mask, all-Paeth -- and float32 maps as TIFF, uncompressed
as this project writes them, in Deflate strips of 32 rows, and as libtiff writes them -- LZW in one-row strips with
predictor 1 and predictor 3), read back in one process:

  host_s_per_file                         image_io.read_png / read_tiff_f32, one file after another
  device_s_per_file, reader_s_per_file    images.load_png_device / load_tiff_device in one call of `batch` files,
                                          images.ImageReader over the same files in 4 batches (batch / 4 files each)
  gpu_inflate_ms, gpu_unfilter_ms         device events around vx_inflate / vx_png_unfilter, for the whole batch
  gpu_lzw_ms, gpu_unpredict_ms, lzw_gbps  (LZW legs) device events around vx_tiff_lzw / vx_tiff_unpredict for the whole
                                          batch, and decoded payload per second of the two together
  host_reader                             (LZW legs) what host_s_per_file timed: "pil_libtiff" = PIL with libtiff on one
                                          core plus the upload of the array, else "read_tiff_f32" (this project's
                                          Python reference reader) plus the upload

--unique distinct files per encoding are written; a batch cycles through them (the page cache serves every read, on
both sides).  One JSON line per (encoding, batch size).

The LZW files are written by libtiff through PIL where PIL has it, else by the test encoder (tests/lzw_build.py).

  python tools/bench_results2d_read.py [--batches 16 256 2048] [--unique 64] [--encodings tiff tiff_lzw_p1 tiff_lzw_p3]
  python tools/bench_results2d_read.py --H 1024 --W 2048 --unique 4 --batches 8 32 --encodings tiff tiff_lzw_p1 tiff_lzw_p3
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


def _masks(n, H, W, rng):
    """blocky label masks: a few dozen rectangles of the 24 classes over a background, as a segmentation looks"""
    import numpy as np
    out = np.zeros((n, H, W), dtype=np.uint8)
    for m in out:
        m[:] = rng.integers(0, 24)
        for _ in range(40):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            m[y:y + int(rng.integers(8, 90)), x:x + int(rng.integers(8, 160))] = rng.integers(0, 24)
    return out


ENCODINGS = ("png_none", "png_sub", "png_paeth", "tiff", "tiff_deflate", "tiff_lzw_p1", "tiff_lzw_p3")


def _pil_libtiff():
    """PIL's Image module where PIL is there and built with libtiff, else None"""
    try:
        from PIL import Image, features
        return Image if features.check("libtiff") else None
    except ImportError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256, 2048])
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--W", type=int, default=478)
    ap.add_argument("--encodings", nargs="+", default=list(ENCODINGS), choices=ENCODINGS)
    a = ap.parse_args()
    import numpy as np
    import torch

    from tests import lzw_build as lb
    from tests import png_build as pb
    from values_amd import _lib, images, results2d
    from values_amd.image_io import read_png, read_tiff_f32, write_tiff_f32
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    H, W = a.H, a.W
    root = tempfile.mkdtemp(prefix="bench_results2d_read_")
    try:
        rgb = results2d._lut()[_masks(a.unique, H, W, rng)] if any(e.startswith("png") for e in a.encodings) else None
        maps = (rng.random((a.unique, H, W), dtype=np.float32) * 0.7).round(3).astype(np.float32)
        maps[:, : H // 3] = 0.0
        files = {}
        for enc, pat in (("png_none", "none"), ("png_sub", "sub"), ("png_paeth", "paeth")):
            if enc not in a.encodings:
                continue
            files[enc] = []
            for k in range(a.unique):
                p = os.path.join(root, f"{enc}_{k}.png")
                with open(p, "wb") as f:
                    f.write(pb.png_bytes(rgb[k], pb.filters(pat, H), level=3))
                files[enc].append(p)
        Image = _pil_libtiff()
        for enc in ("tiff", "tiff_deflate", "tiff_lzw_p1", "tiff_lzw_p3"):
            if enc not in a.encodings:
                continue
            files[enc] = []
            for k in range(a.unique):
                p = os.path.join(root, f"{enc}_{k}.tif")
                if enc == "tiff":
                    write_tiff_f32(p, maps[k])
                elif enc == "tiff_deflate":
                    with open(p, "wb") as f:
                        f.write(pb.tiff_bytes(maps[k], "<", 32, 8))
                elif Image is not None:      # libtiff's writer: LZW, one row per strip
                    Image.fromarray(maps[k]).save(p, compression="tiff_lzw", tiffinfo={317: int(enc[-1]), 278: 1})
                else:
                    with open(p, "wb") as f:
                        f.write(lb.tiff_lzw_bytes(maps[k], "<", 1, int(enc[-1])))
                files[enc].append(p)

        def pil_read(p):
            return torch.from_numpy(np.array(Image.open(p))).cuda()

        def ref_read(p):
            return torch.from_numpy(read_tiff_f32(p)).cuda()

        for enc, paths in files.items():
            png, lzw = enc.startswith("png"), enc.startswith("tiff_lzw")
            host_read = read_png if png else read_tiff_f32
            if lzw:                           # the host path a user has today: libtiff on one core, then the upload
                host_read = pil_read if Image is not None else ref_read
            dev_read = images.load_png_device if png else images.load_tiff_device
            n_host = 2 if enc == "png_paeth" or (lzw and Image is None) else min(16, len(paths))
            host_read(paths[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in paths[:n_host]:
                host_read(p)
            torch.cuda.synchronize()
            t_host = (time.perf_counter() - t0) / n_host
            dev_read(paths[:16])                           # warm-up: the pool, the pinned buffer, the kernels
            torch.cuda.synchronize()
            for n in a.batches:
                batch = [paths[i % len(paths)] for i in range(n)]
                dev_read(batch)                            # the buffers of this size
                torch.cuda.synchronize()
                timing = {}
                t0 = time.perf_counter()
                out = dev_read(batch, _timing=timing)
                torch.cuda.synchronize()
                t_dev = (time.perf_counter() - t0) / n
                del out
                q = max(n // 4, 1)
                t0 = time.perf_counter()
                with images.ImageReader() as r:
                    for _ in r.read([batch[i:i + q] for i in range(0, n, q)]):
                        pass
                torch.cuda.synchronize()
                t_rd = (time.perf_counter() - t0) / n
                extra = {}
                if lzw:
                    # five more calls: the median of the device times and their spread
                    reps = [timing]
                    for _ in range(4):
                        reps.append({})
                        dev_read(batch, _timing=reps[-1])
                    lz = sorted(r.get("lzw_ms", 0.0) for r in reps)
                    up = sorted(r.get("unpredict_ms", 0.0) for r in reps)
                    ms = lz[2] + up[2]
                    extra = {"gpu_lzw_ms": round(lz[2], 3), "gpu_lzw_ms_min_max": [round(lz[0], 3), round(lz[-1], 3)],
                             "gpu_unpredict_ms": round(up[2], 3), "gpu_unpredict_ms_min_max": [round(up[0], 3), round(up[-1], 3)],
                             "lzw_gbps": round(timing["payload_bytes"] / ms / 1e6, 2) if ms > 0 else None,
                             "host_reader": "pil_libtiff" if Image is not None else "read_tiff_f32",
                             "writer": "libtiff" if Image is not None else "lzw_build"}
                print(json.dumps({"metric": "results2d_reader", "encoding": enc, "batch": n, "H": H, "W": W, **extra,
                                  "file_kb": round(sum(os.path.getsize(p) for p in paths) / len(paths) / 1e3, 1),
                                  "host_s_per_file": round(t_host, 6), "device_s_per_file": round(t_dev, 6),
                                  "reader_s_per_file": round(t_rd, 6), "speedup": round(t_host / t_dev, 2),
                                  "reader_speedup": round(t_host / t_rd, 2),
                                  "gpu_inflate_ms": None if lzw else round(timing.get("inflate_ms", 0.0), 3),
                                  "gpu_unfilter_ms": round(timing["unfilter_ms"], 3) if png else None}), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
