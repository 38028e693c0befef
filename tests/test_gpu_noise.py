"""GPU: the TTA noise-view kernels through the C ABI -- vx_noise_view_3d (noise.hip) and vx_tta_views_2d_gen (tta2d.hip) --
against the restatement in tests/noise_ref.py, which also holds this module's inputs (tests/test_noise_ref_cpu.py measures
the float32 gap and the 2D exclusion set on them).

Every output lives in a buffer with GUARD sentinel elements before and after it (tests/test_gpu_sample.py: _Out).

3D bounds (the convention of tests/test_gpu_sample.py): GAP_NOISE3D is the largest float64 vs float32-rounded difference
of the restated view and its scales over this module's inputs; CONTRACT = min(1e-4, 4 x GAP_NOISE3D) -- the factor 4
covers the device's logf / sqrtf / cospif forms against numpy's; OBS is the largest deviation measured on an MI355X over
this module, REG = min(CONTRACT, 5 x OBS) a regression bound asserted beside the contract bound.  sigma_out is held to the
same rule.  Chunking, the device seed word and the refusals are exact.

2D: uint8 truncation is discontinuous, so an element whose float64 pre-truncation value lies within noise_ref.DELTA of a
truncation step may come out one uint8 step off (noise_ref.excluded; at most 1e-3 of a view, expected 5e-5); every other
element of a noisy view is bit-equal to values_amd.data.tta_views_2d fed the restated field.  Clean views are bit-equal
to vx_tta_views_2d.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import noise_ref as nr
from tests.formula import formula_tensor
from tests.test_gpu_sample import _Out, _dev, deviation
from values_amd import _lib

pytestmark = pytest.mark.gpu

CONTRACT = min(1e-4, 4 * nr.GAP_NOISE3D)
OBS = {"view": 2.93e-7, "sigma": 1.54e-8}          # measured on an MI355X over this module (the 2D scales: 2.9e-7)
REG = {k: min(CONTRACT, 5 * v) for k, v in OBS.items()}
F32 = np.float32
# the (B, 2) scales of the 2D entry: var = lo + (hi - lo) * u < 50 carries two float32 roundings, together at most one ulp of
# [32, 64) = 2^-18, which sqrt divides by 2 * sigma >= 2 * sqrt(10); the square root below 8 (ulp 2^-21) adds half an ulp of
# rounding and at most one ulp of the device's sqrtf
SIGMA2D_TOL = 2.0 ** -18 / (2 * 10.0 ** 0.5) + 1.5 * 2.0 ** -21
OK, E_NULL, E_SHAPE, E_DTYPE = 0, -1, -2, -3


def _close(got, want, group, name):
    assert not np.isnan(got).any(), f"{name}: NaN"
    err = deviation(got, want)
    print(f"deviation noise3d {group} {name} {err:.3e}")
    assert err <= CONTRACT, f"{name}: {err:.3e} > contract {CONTRACT:.1e}"
    assert err <= REG[group], f"{name}: {err:.3e} > regression bound {REG[group]:.1e}"


def _seed_word(k):
    """a device word holding the 32-bit value k (int32 storage, as GraphedPredictor's seed word), or None"""
    return None if k is None else torch.from_numpy(np.array([k], dtype=np.uint32).view(np.int32)).cuda()


def _view3d(x, seed, index0, var, law, want_sigma=True, seed_word=None):
    """vx_noise_view_3d on x (V, ...) -> (view, sigma or None)"""
    V = x.shape[0]
    per = int(np.prod(x.shape[1:]))
    out = _Out(x.shape)
    sig = _Out((V,)) if want_sigma else None
    hold = (_dev(x), _seed_word(seed_word))
    _lib.check(_lib.load().vx_noise_view_3d(_lib.ptr(hold[0]), out.p, V, per, seed, _lib.ptr(hold[1]), index0, var[0], var[1],
                                            law, sig.p if sig else None, _lib.stream_ptr()), "vx_noise_view_3d")
    return out.get(), (sig.get() if sig else None)


# ---- 3D: against the float64 restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,index0,seed,law,var", nr.CASES_3D)
def test_noise_view_3d_against_float64(Cc, index0, seed, law, var):
    x = nr.volumes(3, Cc)
    want, want_sigma = nr.view3d(x, seed, index0, var[0], var[1], law)
    got, sigma = _view3d(x, seed, index0, var, law)
    name = f"C{Cc} index0={index0} seed={seed} law={law} var={var}"
    _close(got, want, "view", name)
    _close(sigma, want_sigma, "sigma", name + " sigma")
    alone, _ = _view3d(x, seed, index0, var, law, want_sigma=False)
    assert np.array_equal(alone, got), "out depends on whether sigma is requested"
    lo, hi = float(F32(var[0])), float(F32(var[1]))
    bounds = (np.sqrt(lo), np.sqrt(hi)) if law == 0 else (lo, hi)
    assert (sigma >= bounds[0] - CONTRACT).all() and (sigma <= bounds[1] + CONTRACT).all()
    if hi > lo:
        assert len(np.unique(sigma)) == 3 and np.abs(got - x).max() > 0.01
    assert not np.array_equal(got[0], got[1] - x[1] + x[0])          # the volumes carry different fields


def test_noise_view_3d_second_trip_of_the_grid_stride_loop():
    b = nr.BIG_3D
    x = nr.big_volume()
    assert x.size > 16384 * 256
    want, want_sigma = nr.view3d(x, b["seed"], b["index0"], b["var"][0], b["var"][1], b["law"])
    got, sigma = _view3d(x, b["seed"], b["index0"], b["var"], b["law"])
    for part, sl in (("head", slice(0, 1024)), ("tail", slice(-1024, None))):
        e = deviation(got[..., sl], want[..., sl])
        assert e <= CONTRACT, f"second trip [{part}]: {e:.3e}"
    _close(got, want, "view", "second trip")
    _close(sigma, want_sigma, "sigma", "second trip sigma")


def test_noise_view_3d_writes_the_second_half_of_an_orig_noisy_buffer():
    x = nr.volumes(3, 2, tag=3150)
    V, per = 3, x[0].size
    want, _ = nr.view3d(x, 21, 0, 0.0, 0.1, 0)
    buf = _Out((2 * V,) + x.shape[1:], data=np.concatenate([x, np.full_like(x, -77.0)]))
    first = buf.view[:V * per]
    second = buf.view[V * per:]
    _lib.check(_lib.load().vx_noise_view_3d(_lib.ptr(first), _lib.ptr(second), V, per, 21, None, 0, 0.0, 0.1, 0, None,
                                            _lib.stream_ptr()), "vx_noise_view_3d")
    got = buf.get()
    assert np.array_equal(got[:V], x), "the original half changed"
    _close(got[V:], want, "view", "second half of [orig | noisy]")


# ---- 3D: exact properties ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", [0, 1])
def test_noise_view_3d_chunks_are_the_whole_call_bit_for_bit(law):
    x = nr.volumes(5, 2)
    whole, sg = _view3d(x, 9, 0, (0.0, 0.1), law)
    a, sa = _view3d(x[:2], 9, 0, (0.0, 0.1), law)
    b, sb = _view3d(x[2:], 9, 2, (0.0, 0.1), law)
    assert np.array_equal(whole, np.concatenate([a, b]))
    assert np.array_equal(sg, np.concatenate([sa, sb]))
    shifted, _ = _view3d(x[2:], 9, 0, (0.0, 0.1), law)
    assert not np.array_equal(shifted, whole[2:])


@pytest.mark.parametrize("seed,word", [(5, 3), (0xFFFFFFFF, 2), (7, 0xFFFFFFF0)])
def test_noise_view_3d_device_seed_word_is_added_to_the_seed(seed, word):
    x = nr.volumes(3, 1)
    a, sa = _view3d(x, seed, 1, (0.0, 0.1), 0, seed_word=word)
    b, sb = _view3d(x, (seed + word) & 0xFFFFFFFF, 1, (0.0, 0.1), 0)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    c, _ = _view3d(x, seed, 1, (0.0, 0.1), 0)
    assert not np.array_equal(a, c)


def test_noise_view_3d_refusals_return_before_any_launch():
    lib = _lib.load()
    st = _lib.stream_ptr()
    src = torch.zeros(4096, device="cuda")
    out = _Out((256,))
    s, o = _lib.ptr(src), out.p
    calls = {
        "per = 2^32": (lib.vx_noise_view_3d(s, o, 1, 1 << 32, 0, None, 0, 0.0, 0.1, 0, None, st), E_SHAPE),
        "V = 0": (lib.vx_noise_view_3d(s, o, 0, 16, 0, None, 0, 0.0, 0.1, 0, None, st), E_SHAPE),
        "per < 0": (lib.vx_noise_view_3d(s, o, 1, -1, 0, None, 0, 0.0, 0.1, 0, None, st), E_SHAPE),
        "null x": (lib.vx_noise_view_3d(None, o, 1, 16, 0, None, 0, 0.0, 0.1, 0, None, st), E_NULL),
        "null out": (lib.vx_noise_view_3d(s, None, 1, 16, 0, None, 0, 0.0, 0.1, 0, None, st), E_NULL),
        "hi < lo": (lib.vx_noise_view_3d(s, o, 1, 16, 0, None, 0, 0.2, 0.1, 0, None, st), E_SHAPE),
        "lo < 0": (lib.vx_noise_view_3d(s, o, 1, 16, 0, None, 0, -0.01, 0.1, 0, None, st), E_SHAPE),
        "lo NaN": (lib.vx_noise_view_3d(s, o, 1, 16, 0, None, 0, float("nan"), 0.1, 0, None, st), E_SHAPE),
        "hi inf": (lib.vx_noise_view_3d(s, o, 1, 16, 0, None, 0, 0.0, float("inf"), 0, None, st), E_SHAPE),
        "sigma_law 2": (lib.vx_noise_view_3d(s, o, 1, 16, 0, None, 0, 0.0, 0.1, 2, None, st), E_DTYPE),
        "sigma_law -1": (lib.vx_noise_view_3d(s, o, 1, 16, 0, None, 0, 0.0, 0.1, -1, None, st), E_DTYPE),
        "index0 < 0": (lib.vx_noise_view_3d(s, o, 1, 16, 0, None, -1, 0.0, 0.1, 0, None, st), E_SHAPE),
        "index0 + V > 2^32": (lib.vx_noise_view_3d(s, o, 2, 16, 0, None, (1 << 32) - 1, 0.0, 0.1, 0, None, st), E_SHAPE),
        "per = 0": (lib.vx_noise_view_3d(s, o, 1, 0, 0, None, 0, 0.0, 0.1, 0, None, st), OK),
    }
    for name, (rc, want) in calls.items():
        assert rc == want, f"{name}: rc = {rc}, expected {want}"
    assert out.untouched(), "a refused call wrote to its output"
    assert b"vx_noise_view_3d" in lib.vx_last_error_string()
    # the last admissible slot
    one = _Out((16,))
    _lib.check(lib.vx_noise_view_3d(s, one.p, 1, 16, 3, None, (1 << 32) - 1, 1.0, 1.0, 0, None, st), "vx_noise_view_3d")
    np.testing.assert_allclose(one.get(), nr.view3d(np.zeros((1, 16), F32), 3, (1 << 32) - 1, 1.0, 1.0)[0][0], atol=CONTRACT)


# ---- 2D -------------------------------------------------------------------------------------------------------------------
def _c3(v):
    return (C.c_float * 3)(*[float(t) for t in v])


def _views_gen(img, codes, seed, image0, noise0=None, noise1=None, want_sigma=True, seed_word=None, var_limit=nr.VAR_LIMIT):
    """vx_tta_views_2d_gen on img (B, H, W, 3) u8 -> (views (G, B, H, W, 4), sigma (B, 2) or None)"""
    B, H, W, _ = img.shape
    out = _Out((len(codes), B, H, W, 4))
    sig = _Out((B, 2)) if want_sigma else None
    hold = (_dev(img, np.uint8), _dev(noise0), _dev(noise1), _seed_word(seed_word))
    vc = (C.c_int32 * len(codes))(*codes)
    vl = (C.c_float * 2)(*var_limit)
    _lib.check(_lib.load().vx_tta_views_2d_gen(_lib.ptr(hold[0]), 1, _lib.ptr(hold[1]), _lib.ptr(hold[2]), _c3(nr.MEAN), _c3(nr.STD),
                                               255.0, B, H, W, len(codes), vc, seed, _lib.ptr(hold[3]), image0, vl,
                                               sig.p if sig else None, out.p, _lib.stream_ptr()), "vx_tta_views_2d_gen")
    return out.get(), (sig.get() if sig else None)


def _views_plain(img, codes, noise0=None, noise1=None, src_u8=1):
    B, H, W = (img.shape[0], img.shape[1], img.shape[2]) if src_u8 else (img.shape[0], img.shape[2], img.shape[3])
    out = _Out((len(codes), B, H, W, 4))
    hold = (_dev(img, np.uint8 if src_u8 else F32), _dev(noise0), _dev(noise1))
    vc = (C.c_int32 * len(codes))(*codes)
    rc = _lib.load().vx_tta_views_2d(_lib.ptr(hold[0]), src_u8, _lib.ptr(hold[1]), _lib.ptr(hold[2]),
                                     _c3(nr.MEAN) if src_u8 else None, _c3(nr.STD) if src_u8 else None, 255.0 if src_u8 else 0.0,
                                     B, H, W, len(codes), vc, out.p, _lib.stream_ptr())
    return rc, out


def _host_noisy_view(img_b, field, code):
    """the noisy view of one image through values_amd.data.tta_views_2d fed the restated field -> (H, W, 3) float32"""
    from values_amd.data import tta_views_2d
    if code & 8:      # flip of the noisy image
        v = tta_views_2d(img_b, nr.MEAN, nr.STD, noise=field)[0][2]                      # Noise(img), CHW
        return nr.flip_of(code, v.transpose(1, 2, 0))
    v = tta_views_2d(np.ascontiguousarray(nr.flip_of(code, img_b)), nr.MEAN, nr.STD, noise=field)[0][2]
    return v.transpose(1, 2, 0)


def _check_noisy(got, img, noise, codes, tag):
    """got (G, B, H, W, 4); every generated view against the host function, element by element"""
    step = (F32(1.0) / (np.asarray(nr.STD, F32) * F32(255.0))).astype(np.float64)        # one uint8 step after Normalize
    for g, code in enumerate(codes):
        if not code & 32:
            continue
        for b in range(img.shape[0]):
            field = noise[b, (code >> 4) & 1]
            want = _host_noisy_view(img[b], field, code)
            ex = nr.excluded(nr.noisy_view_pre(img[b], field, code))
            share = ex.mean()
            print(f"excluded share {tag} code {code} image {b}: {share:.2e}")
            assert share <= nr.EXCLUDED_SHARE_MAX
            have = got[g, b, :, :, :3]
            assert (got[g, b, :, :, 3] == 0).all()
            assert np.array_equal(have[~ex], want[~ex]), f"{tag} code {code} image {b}: outside the exclusion set"
            d = np.abs(have.astype(np.float64) - want.astype(np.float64))
            # (one step is inv_c = 1 / (std_c * 255) up to the float32 rounding of two normalised values below 4: 2 x 2^-22)
            assert (d <= step[None, None, :] + 2.0 ** -21)[ex].all(), f"{tag} code {code} image {b}: exclusion set, more than one step"


@pytest.mark.parametrize("image0", nr.IMAGE0_2D)
@pytest.mark.parametrize("which", ["ref4", "eight"])
def test_tta_views_2d_gen_noisy_views_are_the_host_function_on_the_restated_field(which, image0):
    img = nr.images_2d()
    codes = nr.CODES_REF4 if which == "ref4" else nr.CODES_8
    noise = nr.noise2d(nr.SEED_2D, image0, nr.B2, nr.H2, nr.W2, *nr.VAR_LIMIT)
    got, sigma = _views_gen(img, codes, nr.SEED_2D, image0)
    # clean views: bit-equal to vx_tta_views_2d
    rc, plain = _views_plain(img, [c for c in codes if not c & 4])
    assert rc == OK
    assert np.array_equal(got[[g for g, c in enumerate(codes) if not c & 4]], plain.get())
    _check_noisy(got, img, noise, codes, f"{which} image0={image0}")
    want_sigma = nr.scales2d(nr.SEED_2D, image0, nr.B2, *nr.VAR_LIMIT)
    err = deviation(sigma, want_sigma)
    print(f"deviation noise2d sigma {which} image0={image0} {err:.3e}")
    assert err <= SIGMA2D_TOL
    assert len(np.unique(sigma)) == 2 * nr.B2
    alone, _ = _views_gen(img, codes, nr.SEED_2D, image0, want_sigma=False)
    assert np.array_equal(alone, got)
    if which == "ref4":       # the two slots of one image differ: views 2 and 3 un-flipped carry different fields
        for b in range(nr.B2):
            assert not np.array_equal(got[2, b], got[3, b, :, ::-1])
            assert np.mean(got[2, b] != got[0, b]) > 0.5
    else:                     # bit 3: exact flips of the slot-0 noisy view
        base = got[4]
        assert np.array_equal(got[5], base[:, :, ::-1]) and np.array_equal(got[6], base[:, ::-1])
        assert np.array_equal(got[7], base[:, ::-1, ::-1])
    if image0 == 3:           # image 3 + b of this call is image b of a call with image0 = 3 + b: batching does not matter
        single, _ = _views_gen(img[1:], codes, nr.SEED_2D, 4)
        assert np.array_equal(single[:, 0], got[:, 1])


def test_tta_views_2d_gen_mixes_supplied_and_generated_fields_and_adds_the_seed_word():
    img = nr.images_2d()
    supplied = (formula_tensor((nr.B2, nr.H2, nr.W2, 3), 3210, 9.0)).astype(F32)
    codes = [0, 1, 4, 1 | 4 | 16 | 32]                    # slot 0 supplied, slot 1 generated
    noise = nr.noise2d(nr.SEED_2D, 0, nr.B2, nr.H2, nr.W2, *nr.VAR_LIMIT)
    got, _ = _views_gen(img, codes, nr.SEED_2D, 0, noise0=supplied)
    rc, plain = _views_plain(img, [0, 1, 4], noise0=supplied)
    assert rc == OK and np.array_equal(got[:3], plain.get())
    _check_noisy(got, img, noise, codes, "mixed")
    # a supplied field in the other slot, generated slot 0
    codes = [4 | 32, 1 | 4 | 16]
    got, _ = _views_gen(img, codes, nr.SEED_2D, 0, noise1=supplied)
    rc, plain = _views_plain(img, [1 | 4 | 16], noise1=supplied)
    assert rc == OK and np.array_equal(got[1:], plain.get())
    _check_noisy(got, img, noise, codes, "mixed, slot 1 supplied")
    # seed word k with seed s = seed s + k
    a, sa = _views_gen(img, nr.CODES_REF4, 70, 0, seed_word=7)
    b, sb = _views_gen(img, nr.CODES_REF4, 77, 0)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    c, _ = _views_gen(img, nr.CODES_REF4, 70, 0)
    assert not np.array_equal(a, c)


def test_tta_views_2d_gen_refusals_and_the_unchanged_plain_entry():
    lib = _lib.load()
    st = _lib.stream_ptr()
    img = nr.images_2d()
    B, H, W = nr.B2, nr.H2, nr.W2
    d_img = _dev(img, np.uint8)
    f32src = torch.zeros((B, 3, H, W), device="cuda")
    out = _Out((4, B, H, W, 4))
    vl = (C.c_float * 2)(*nr.VAR_LIMIT)

    def gen(codes, src=d_img, src_u8=1, var=vl, image0=0, n0=None, outp=None):
        vc = (C.c_int32 * len(codes))(*codes)
        return lib.vx_tta_views_2d_gen(_lib.ptr(src), src_u8, _lib.ptr(n0), None, _c3(nr.MEAN), _c3(nr.STD), 255.0, B, H, W,
                                       len(codes), vc, 1, None, image0, var, None, outp or out.p, st)
    calls = {
        "bit 5 with the f32 source": (gen([0, 4 | 32], src=f32src, src_u8=0, n0=f32src), E_DTYPE),
        "code 64": (gen([0, 64]), E_DTYPE),
        "code -1": (gen([-1]), E_DTYPE),
        "bit 5 without bit 2": (gen([32]), E_DTYPE),
        "noisy, not generated, no field": (gen([4]), E_NULL),
        "null var_limit": (gen([4 | 32], var=None), E_NULL),
        "var hi < lo": (gen([4 | 32], var=(C.c_float * 2)(50.0, 10.0)), E_SHAPE),
        "var lo < 0": (gen([4 | 32], var=(C.c_float * 2)(-1.0, 10.0)), E_SHAPE),
        "image0 < 0": (gen([4 | 32], image0=-1), E_SHAPE),
        "(image0 + B) * 2 > 2^32": (gen([4 | 32], image0=(1 << 31) - 1), E_SHAPE),
        "misaligned out": (gen([4 | 32], outp=C.c_void_p(out.p.value + 4)), -5),
    }
    for name, (rc, want) in calls.items():
        assert rc == want, f"{name}: rc = {rc}, expected {want}"
    assert out.untouched(), "a refused call wrote to its output"
    # vx_tta_views_2d keeps its refusals: bit 5 (and anything above 31) is not its to take
    for code in (32, 4 | 32, 63, 64):
        rc, o = _views_plain(img, [0, code])
        assert rc == E_DTYPE and o.untouched(), code
    rc, o = _views_plain(img, [4])
    assert rc == E_NULL and o.untouched()
    # ... and every code it accepts gives the same output through either entry, u8 and f32 source
    n0 = formula_tensor((B, H, W, 3), 3220, 9.0).astype(F32)
    n1 = formula_tensor((B, H, W, 3), 3221, 9.0).astype(F32)
    from values_amd.data import tta_views_2d
    for lo in (0, 16):
        codes = list(range(lo, lo + 16))
        rc, plain = _views_plain(img, codes, n0, n1)
        assert rc == OK
        via_gen, _ = _views_gen(img, codes, 1, 0, noise0=n0, noise1=n1, want_sigma=False)
        assert np.array_equal(plain.get(), via_gen), "a code without bit 5 behaves differently through the new entry"
    host, _ = tta_views_2d(img[0], nr.MEAN, nr.STD, noise=n0[0], noise_flipped=n1[0])           # today's outputs
    rc, plain = _views_plain(img, [0, 1, 4, 1 | 4 | 16], n0, n1)
    assert rc == OK
    for g in range(4):
        assert np.array_equal(plain.get()[g, 0, :, :, :3], host[g].transpose(1, 2, 0)), g
    xf = formula_tensor((B, 3, H, W), 3230, 2.0).astype(F32)
    xn = formula_tensor((B, 3, H, W), 3231, 2.0).astype(F32)
    rc, o = _views_plain(xf, list(range(8)), noise0=xn, src_u8=0)
    assert rc == OK
    got = o.get()
    for code in range(8):
        want = (xn if code & 4 else xf).transpose(0, 2, 3, 1)                 # (B, H, W, 3)
        want = want[:, :, ::-1] if code & 1 else want
        want = want[:, ::-1] if code & 2 else want
        assert np.array_equal(got[code, ..., :3], want), code
