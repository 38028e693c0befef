"""Times the TTA noise-view kernels with device events: vx_noise_view_3d on a batch of 64^3 volumes beside
the ATen draw it replaces (values_amd.predict.gaussian_noise_view), and vx_tta_views_2d_gen on a batch of uint8 images
beside vx_tta_views_2d fed two uploaded float32 fields.  Bytes are the algorithm's (shapes), not counters:
  3D: 8 B per element;  2D: 3 B read + 16 B written per output pixel (+ 12 B per noisy pixel whose field is supplied).
Usage: python tools/bench_noise.py [--volumes 32] [--size 64] [--images 4] [--height 512] [--width 1024] [--reps 200]
For kernel times: rocprofv3 --kernel-trace --stats -- python tools/bench_noise.py --reps 20"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup=10):
    """ms per call: device events around `reps` back-to-back calls, after a warm-up"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=32)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    from values_amd import _lib
    from values_amd.data import TTA_2D_VIEW_CODES, tta_views_2d_device
    from values_amd.predict import gaussian_noise_view, noise_view_device
    _lib.require_gpu()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((a.volumes, 1, a.size, a.size, a.size), device="cuda", generator=g)
    out = torch.empty_like(x)
    n = x.numel()
    for name, fn in (("vx_noise_view_3d", lambda: noise_view_device(x, 7, out=out)),
                     ("gaussian_noise_view (ATen)", lambda: gaussian_noise_view(x))):
        ms = timed(fn, a.reps)
        print(f"{name}: {a.volumes} x {a.size}^3 = {n} elements, {ms * 1e3:.1f} us per call, "
              f"{8 * n / ms / 1e9:.2f} TB/s of the 8 B per element")
    img = torch.randint(0, 256, (a.images, a.height, a.width, 3), device="cuda", dtype=torch.uint8, generator=g)
    n0 = torch.randn((a.images, a.height, a.width, 3), device="cuda", generator=g) * 5
    n1 = torch.randn((a.images, a.height, a.width, 3), device="cuda", generator=g) * 5
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    pix = a.images * a.height * a.width
    G = len(TTA_2D_VIEW_CODES)
    for name, fn, extra in (("vx_tta_views_2d_gen (2 of 4 views generated)", lambda: tta_views_2d_device(img, mean, std, noise_seed=7), 0),
                            ("vx_tta_views_2d (2 of 4 views, supplied fields)",
                             lambda: tta_views_2d_device(img, mean, std, noise=n0, noise_flipped=n1), 12 * 2 * pix),
                            ("vx_tta_views_2d (no noise: 4 clean views)", lambda: tta_views_2d_device(img, mean, std), 0)):
        ms = timed(fn, a.reps)
        nbytes = 19 * G * pix + extra
        print(f"{name}: {a.images} x {a.height} x {a.width}, {G} views, {ms * 1e3:.1f} us per call (host wrapper included), "
              f"{nbytes / ms / 1e9:.2f} TB/s of {nbytes / 1e6:.0f} MB")


if __name__ == "__main__":
    main()
