"""An independent numpy restatement of what cv2.resize computes on uint8 images when it shrinks by an integer factor k
(fx = fy = 1 / k), shared by tests/test_preprocess2d_cpu.py and tests/test_gpu_preprocess2d.py.  Written from OpenCV's
published algorithm (modules/imgproc/src/resize.cpp), not from values_amd.preprocess2d: the GENERAL two-pass fixed-point
bilinear, of which the mirror's four-tap average is the special case of an even k.

    output size     saturate_cast<int>(size * fx): round half to even on the exact quotient
    INTER_LINEAR    source coordinate f = (d + 0.5) * k - 0.5, s = floor(f), weight w = f - s; coefficients
                    round((1 - w) * 2048), round(w * 2048).  Horizontally a tap left of the image gives (s, w) = (0, 0),
                    one at or beyond the last column (size - 1, 0); vertically the rows s and s + 1 are clipped into the
                    image and the weights stay.  Rows are summed in int32 (HResizeLinear), then
                    (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2   (VResizeLinear, uint8)
    INTER_NEAREST   source pixel min(floor(d * k), size - 1)

cv2 itself is absent, so this is the derivation the mirror is held to, not an observation of OpenCV.
"""
from fractions import Fraction

import numpy as np

ONE = 2048   # INTER_RESIZE_COEF_SCALE: 11 bits


def out_size(size, k):
    return round(Fraction(size, k))   # Python rounds a Fraction half to even


def _taps(size, n_out, k, zero_at_borders):
    s0, s1, a0, a1 = [], [], [], []
    for d in range(n_out):
        f = (d + 0.5) * k - 0.5
        s = int(np.floor(f))
        w = f - s
        if zero_at_borders:
            if s < 0:
                s, w = 0, 0.0
            if s >= size - 1:
                s, w = size - 1, 0.0
        s0.append(min(max(s, 0), size - 1))
        s1.append(min(max(s + 1, 0), size - 1))
        a0.append(int(np.rint((1.0 - w) * ONE)))
        a1.append(int(np.rint(w * ONE)))
    return np.array(s0), np.array(s1), np.array(a0, np.int64), np.array(a1, np.int64)


def resize_linear_fixed(img, k):
    a = np.asarray(img)
    assert a.dtype == np.uint8
    squeeze = a.ndim == 2
    a = a[..., None] if squeeze else a
    h, w = a.shape[:2]
    oh, ow = out_size(h, k), out_size(w, k)
    x0, x1, ax0, ax1 = _taps(w, ow, k, True)
    y0, y1, by0, by1 = _taps(h, oh, k, False)
    s = a.astype(np.int64)
    rows = s[:, x0] * ax0[None, :, None] + s[:, x1] * ax1[None, :, None]          # (h, ow, c), the int buffer
    top = (by0[:, None, None] * (rows[y0] >> 4)) >> 16
    bot = (by1[:, None, None] * (rows[y1] >> 4)) >> 16
    out = (top + bot + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    out = out.astype(np.uint8)
    return out[..., 0] if squeeze else out


def resize_nearest_ref(img, k):
    a = np.asarray(img)
    h, w = a.shape[:2]
    ys = [min(int(np.floor(d * k)), h - 1) for d in range(out_size(h, k))]
    xs = [min(int(np.floor(d * k)), w - 1) for d in range(out_size(w, k))]
    return a[np.array(ys, np.int64)][:, np.array(xs, np.int64)]
