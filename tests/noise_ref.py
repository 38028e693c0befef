"""Restatement of the TTA noise-view kernels (numpy only, no GPU, nothing from values_amd): vx_noise_view_3d (noise.hip)
and the generated fields of vx_tta_views_2d_gen (tta2d.hip), built on the generator restated in tests/sample_ref.py, plus
the inputs tests/test_gpu_noise.py runs them on (tests/test_noise_ref_cpu.py measures the float32 gap and the 2D exclusion
set on the same arrays).

dtype=np.float64 is the reference; dtype=np.float32 rounds the inputs and every intermediate to float32 (sample_ref's
convention) and is used only to measure what float32 arithmetic alone costs.  The seed arguments are the EFFECTIVE seed
(seed + the device word, modulo 2^32).
"""
from __future__ import annotations

import numpy as np

from tests.formula import formula_tensor
from tests.sample_ref import _f, gauss, stream_key, uniforms

SCALE_XOR = 0x3C6EF372          # the scale of slot g comes from element 0 of stream g of seed ^ SCALE_XOR (u2 word)
F32 = np.float32


def scale_seed(seed):
    return (int(seed) ^ SCALE_XOR) & 0xFFFFFFFF


def variances(seed, slots, lo, hi, dtype=np.float64):
    """var[slot] = lo + (hi - lo) * u2, u2 in [0, 1) the second uniform of element 0 of stream `slot` of seed ^ SCALE_XOR;
    lo / hi are float32 values (the ABI takes floats)"""
    u2 = uniforms(scale_seed(seed), 0, np.asarray(slots))[1].astype(dtype)
    lo, hi = dtype(F32(lo)), dtype(F32(hi))
    return (lo + ((hi - lo) * u2).astype(dtype)).astype(dtype)


def scales(seed, slots, lo, hi, sigma_law=0, dtype=np.float64):
    """sigma[slot]: sqrt(var) (sigma_law 0) or var (sigma_law 1)"""
    var = variances(seed, slots, lo, hi, dtype)
    return var if sigma_law else _f(np.sqrt, var, dtype)


def view3d(x, seed, index0=0, lo=0.0, hi=0.1, sigma_law=0, dtype=np.float64):
    """x [V][per] -> (x[v][r] + sigma_g * gauss(seed, r, g), sigma [V]),  g = index0 + v"""
    x = np.asarray(x)
    V = x.shape[0]
    xf = x.reshape(V, -1).astype(dtype)
    g = index0 + np.arange(V)
    sg = scales(seed, g, lo, hi, sigma_law, dtype)
    e = gauss(seed, np.arange(xf.shape[1])[None, :], g[:, None], dtype)
    return (xf + (sg[:, None] * e).astype(dtype)).astype(dtype).reshape(x.shape), sg


def field2d(seed, image0, B, H, W, dtype=np.float64):
    """unit normals [B][2][H][W][3]: element (y * W + x) * 3 + c of stream (image0 + b) * 2 + k"""
    slot = (image0 + np.arange(B))[:, None] * 2 + np.arange(2)[None, :]
    return gauss(seed, np.arange(H * W * 3)[None, None, :], slot[:, :, None], dtype).reshape(B, 2, H, W, 3)


def scales2d(seed, image0, B, lo=10.0, hi=50.0, dtype=np.float64):
    """sqrt(var) [B][2]"""
    slot = (image0 + np.arange(B))[:, None] * 2 + np.arange(2)[None, :]
    return scales(seed, slot, lo, hi, 0, dtype)


def noise2d(seed, image0, B, H, W, lo=10.0, hi=50.0):
    """the additive fields sigma * n in float64, [B][2][H][W][3] (slot k on axis 1)"""
    return scales2d(seed, image0, B, lo, hi)[:, :, None, None, None] * field2d(seed, image0, B, H, W)


def pre_truncation(img, field):
    """img [H][W][3] uint8 (already flipped if the view is), field [H][W][3] float64 -> img + field, float64: what the
    view clips to 0..255 and truncates"""
    return np.asarray(img).astype(np.float64) + field


# ---- the GPU module's inputs ------------------------------------------------------------------------------------------
NVOX = 1029                     # per channel: odd, five blocks of 256 with a ragged last one
SEEDS = (0, 5, 0xFFFFFFFF)
VARIANCES = ((0.0, 0.1), (0.05, 0.05))
PER_BIG = (1 << 22) + 517       # one volume: past 16384 x 256 threads, a second trip of the grid-stride loop
CASES_3D = [(C_, index0, seed, law, var) for C_ in (1, 2) for index0 in (0, 7) for seed in SEEDS for law in (0, 1)
            for var in VARIANCES]
BIG_3D = dict(seed=11, index0=3, law=0, var=(0.0, 0.1))
GAP_NOISE3D = 3.34e-7           # test_noise_ref_cpu.py recomputes it; includes the scales


def volumes(V, C_, nvox=NVOX, tag=3100):
    """(V, C, nvox) float32 of magnitude < 3 (z-scored intensities)"""
    return formula_tensor((V, C_, nvox), tag + 10 * C_ + V, scale=3.0).astype(F32)


def big_volume():
    return formula_tensor((1, 1, PER_BIG), 3190, scale=3.0).astype(F32)


def reference_matrix_3d():
    """every float comparison of the 3D GPU tests as (name, ref): ref(dtype) -> (view, sigma)"""
    for C_, index0, seed, law, var in CASES_3D:
        x = volumes(3, C_)
        yield (f"C{C_} index0={index0} seed={seed} law={law} var={var}",
               lambda dtype, a=(x, seed, index0, var[0], var[1], law): view3d(*a, dtype=dtype))
    b = BIG_3D
    yield ("second trip", lambda dtype, a=(big_volume(), b["seed"], b["index0"], b["var"][0], b["var"][1], b["law"]):
           view3d(*a, dtype=dtype))
    x = volumes(3, 2, tag=3150)
    yield ("second half of [orig | noisy]", lambda dtype, a=(x, 21, 0, 0.0, 0.1, 0): view3d(*a, dtype=dtype))


# 2D
B2, H2, W2 = 2, 23, 37
SEED_2D = 77
IMAGE0_2D = (0, 3)
VAR_LIMIT = (10.0, 50.0)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
CODES_REF4 = [0, 1, 4 | 32, 1 | 4 | 16 | 32]                                   # the reference's four views, noisy ones generated
CODES_8 = [c | 32 if c & 4 else c for c in [0, 1, 2, 3, 4 | 8, 5 | 8, 6 | 8, 7 | 8]]   # TTA_8_VIEW_CODES with bit 5
CONTRACT_GENERATED = min(1e-4, 4 * 3.41e-7)      # tests/test_gpu_sample.py: CONTRACT["generated"], the generator's contract bound
DELTA = float(np.sqrt(VAR_LIMIT[1])) * CONTRACT_GENERATED + 2.0 ** -16
EXCLUDED_SHARE_MAX = 1e-3


def images_2d():
    """(B, H, W, 3) uint8 covering 0..255 (values near both clip ends included)"""
    return ((formula_tensor((B2, H2, W2, 3), 3200, 1.0) + 1.0) * 127.999).astype(np.uint8)


def flip_of(code, a):
    """the array a [H][W][...] under the flips of a view code (bit 0 horizontal, bit 1 vertical)"""
    if code & 1:
        a = a[:, ::-1]
    if code & 2:
        a = a[::-1]
    return a


def noisy_view_pre(img, field, code):
    """float64 pre-truncation values of a noisy view in VIEW coordinates: img [H][W][3] uint8, field [H][W][3] the slot's
    additive field.  bit 3: the field travels with the image (flip of the noisy image); else it is indexed at the view's pixel"""
    if code & 8:
        return flip_of(code, pre_truncation(img, field))
    return pre_truncation(flip_of(code, img), field)


def excluded(pre):
    """elements whose pre-truncation value lies within DELTA of a truncation step: the uint8 value may fall on either side"""
    k = np.rint(pre)
    return (np.abs(pre - k) <= DELTA) & (k >= 1) & (k <= 255)      # (truncation steps at 1..255: below 1 everything is 0)
