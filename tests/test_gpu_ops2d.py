"""GPU: the kernel-level matrix of the 2D (HRNet) streaming kernels and of vx_conv2d's input prologue, through the C ABI,
against tests/ops2d_ref.py -- the host restatement that tests/test_ops2d_ref_cpu.py pins to torch and the oracle.

Contracts ("Kernel-level contracts of the 2D path"):
  vx_bn_finalize[_groups]          scale / shift within 1 float32 ulp of the exactly summed float64 formula
  vx_affine_gather, vx_fuse_sum,
  vx_bilinear_nchw                 `==` the float32 restatement (the library is built without contraction)
  vx_bilinear_softmax_nchw         `==` vx_bilinear_nchw + vx_softmax_planar, 1e-6 of the float64 twin
  vx_conv2d with the prologue      equal bits to vx_affine_gather + vx_conv2d, 3e-5 x max(1, max|activated input|) of float64
Every output buffer starts as a sentinel; what a call must not write is checked to still hold it."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from values_amd import _lib
from tests import ops2d_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77.0
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -5


def r4(c):
    return (c + 3) // 4 * 4


def r16(c):
    return (c + 15) // 16 * 16


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pitched(x, pitch, pad=0.0):
    """channels-last numpy [..., C] -> device [..., pitch] float32 with `pad` in the channels [C, pitch)"""
    out = np.full(x.shape[:-1] + (pitch,), pad, dtype=np.float32)
    out[..., :x.shape[-1]] = x
    return to_dev(out)


def assert_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~(got == ref)
    if bad.any():
        d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, max |d| = {np.nanmax(d):.3e}, first at {tuple(np.argwhere(bad)[0])}")


def assert_window(full, ref, coff, what=""):
    """full [..., pitch]: channels [coff, coff + C) equal ref, every other channel still holds the sentinel"""
    c = ref.shape[-1]
    assert (full[..., :coff] == SENT).all() and (full[..., coff + c:] == SENT).all(), f"{what}: wrote outside [out_coff, out_coff + C)"
    assert_bits(full[..., coff:coff + c], ref, what)


# =====================================================================================================================
# vx_bn_finalize / vx_bn_finalize_groups
def run_finalize(part, count, c, g, cpitch, gamma, beta, grouped, ntiles=None, rc=0, eps=1e-5):
    lib = _lib.load()
    pd = to_dev(part)
    ntiles = part.shape[0] // max(g, 1) if ntiles is None else ntiles
    scale = torch.full((max(g, 1), max(cpitch, 1)), SENT, dtype=torch.float32, device=DEV)
    shift = torch.full_like(scale, SENT)
    gd, bd = (None if t is None else to_dev(t) for t in (gamma, beta))
    if grouped:
        got = lib.vx_bn_finalize_groups(_lib.ptr(pd), ntiles, g, c, cpitch, count, eps, _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(scale),
                                        _lib.ptr(shift), _lib.stream_ptr())
    else:
        got = lib.vx_bn_finalize(_lib.ptr(pd), ntiles, c, count, eps, _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(scale), _lib.ptr(shift),
                                 _lib.stream_ptr())
    assert got == rc, (got, lib.vx_last_error_string())
    torch.cuda.synchronize()
    return scale.cpu().numpy(), shift.cpu().numpy()


def assert_one_ulp(got, ref64, what):
    err = np.abs(got.astype(np.float64) - ref64)
    ulp = R.ulp32(ref64)
    assert np.isfinite(got).all() and (err <= ulp).all(), f"{what}: {np.max(err / ulp):.3f} ulp"
    return float(np.max(err / ulp))


@pytest.mark.parametrize("case", R.finalize_cases(), ids=R.finalize_case_id)
def test_bn_finalize_within_one_ulp_of_exact_sums(case):
    """ntiles around the 64-lane wave and the 256-thread stride, one to 720 channels, null and non-null gamma / beta; the grouped
    form with cpitch == C and cpitch > C (columns [C, cpitch) keep their sentinel) on partials that differ per group"""
    part, count = R.finalize_partials(case.ntiles, case.C, case.tag, case.G)
    gamma, beta = R.f32_tensor((case.C,), case.tag + 2, 0.3, 1.0), R.f32_tensor((case.C,), case.tag + 3, 0.2)
    sums = R.exact_sums(part.reshape(case.G, case.ntiles, case.C, 2))
    worst = 0.0
    for use_g, use_b in itertools.product((True, False), (True, False)):
        ga, be = gamma if use_g else None, beta if use_b else None
        sc, sh = run_finalize(part, count, case.C, case.G, case.cpitch, ga, be, case.grouped)
        for g in range(case.G):
            rs, rh = R.bn_scale_shift_from_sums(sums[g, :, 0], sums[g, :, 1], count, R.EPS32, ga, be)
            worst = max(worst, assert_one_ulp(sc[g, :case.C], rs, f"scale, group {g}, gamma {use_g}"))
            worst = max(worst, assert_one_ulp(sh[g, :case.C], rh, f"shift, group {g}, gamma {use_g}, beta {use_b}"))
        assert (sc[:, case.C:] == SENT).all() and (sh[:, case.C:] == SENT).all()
    print(f"bn_finalize {R.finalize_case_id(case)}: worst {worst:.3f} ulp")


def test_bn_finalize_variance_clamp():
    """var == 0 exactly (a constant channel, exact sums) and var < 0 before the clamp (a sumsq partial rounded down): finite, and
    gamma / sqrt(eps32) within 1 ulp"""
    part, count = R.clamp_partials()
    gamma, beta = np.array([1.5, 0.75], np.float32), np.array([0.25, -0.5], np.float32)
    rs, rh = R.bn_scale_shift_exact(part, count, R.EPS32, gamma, beta)
    for grouped in (False, True):
        sc, sh = run_finalize(part, count, 2, 1, 2, gamma, beta, grouped)
        assert_one_ulp(sc[0], rs, "scale")
        assert_one_ulp(sh[0], rh, "shift")
        assert_one_ulp(sc[0], gamma.astype(np.float64) / np.sqrt(float(R.EPS32)), "gamma / sqrt(eps)")


def test_bn_finalize_refusals():
    part, count = R.finalize_partials(4, 8, 77)
    for kw in (dict(ntiles=0), dict(c=0), dict(count=0), dict(ntiles=-1), dict(c=-3), dict(count=-5)):
        for grouped in (False, True):
            sc, sh = run_finalize(part, kw.get("count", count), kw.get("c", 8), 1, 8, None, None, grouped, ntiles=kw.get("ntiles", 4), rc=E_SHAPE)
            assert (sc == SENT).all() and (sh == SENT).all()
    sc, sh = run_finalize(part, count, 8, 1, 4, None, None, True, ntiles=4, rc=E_SHAPE)          # cpitch < C
    assert (sc == SENT).all() and (sh == SENT).all()
    sc, sh = run_finalize(part, count, 8, 0, 8, None, None, True, ntiles=4, rc=E_SHAPE)          # no group
    assert (sc == SENT).all()


# =====================================================================================================================
# vx_affine_gather
def group_rows(t, n, group_images):
    """scale / shift for the device: grouped rows [G][C] travel in a buffer of N rows whose rows beyond G hold 1000 -- a kernel
    that took row n instead of row n / group_images would read defined, visibly wrong values"""
    t = np.asarray(t, dtype=np.float32)
    if group_images <= 0 or t.ndim != 2 or t.shape[0] >= n:
        return t
    return np.concatenate([t, np.full((n - t.shape[0], t.shape[1]), 1000.0, dtype=np.float32)])


def run_affine(x, *, out_hw=None, x_pitch=None, x_pad=0.0, scale=None, shift=None, add=None, add_pitch=None, add_pad=0.0,
               alias=False, relu=False, act=None, out_pitch=None, out_coff=0, group_images=0, drop=None, rc=0, C_override=None):
    """x, add: channels-last numpy of REAL channels.  drop: ("mask", uint8 [N][H][W][C] numpy or device tensor) |
    ("mask-null",) | ("hash", seed, layer).  Returns the whole output buffer [N][OH][OW][out_pitch] (numpy)."""
    lib = _lib.load()
    n, h, w, c = x.shape
    oh, ow = out_hw or (h, w)
    xd = pitched(x, x_pitch or c, x_pad)
    out_pitch = out_pitch or c
    out = torch.full((n, oh, ow, out_pitch), SENT, dtype=torch.float32, device=DEV)
    a = _lib.AffineArgs()
    a.x = xd.data_ptr(); a.x_pitch = xd.shape[-1]
    keep = [xd]
    for name, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            keep.append(to_dev(group_rows(t, n, group_images)))
            setattr(a, name, keep[-1].data_ptr())
    if add is not None:
        if alias:
            out[..., out_coff:out_coff + c] = to_dev(add)
            a.add = out.data_ptr() + 4 * out_coff; a.add_pitch = out_pitch
        else:
            # (the buffer is as long as one of the output's pitch, the tail holding 1000: a kernel that stepped through `add` with
            # out_pitch would read defined, visibly wrong values)
            ad = pitched(add, add_pitch or c, add_pad)
            keep.append(torch.full((n * oh * ow * max(ad.shape[-1], out_pitch),), 1000.0, dtype=torch.float32, device=DEV))
            keep[-1][:ad.numel()] = ad.reshape(-1)
            a.add = keep[-1].data_ptr(); a.add_pitch = ad.shape[-1]
    a.out = out.data_ptr(); a.out_pitch = out_pitch; a.out_coff = out_coff
    a.N, a.H, a.W, a.C, a.OH, a.OW = n, h, w, C_override or c, oh, ow
    a.act = act if act is not None else (_lib.VX_ACT_RELU if relu else _lib.VX_ACT_NONE)
    a.group_images = group_images
    if drop is not None:
        if drop[0] == "hash":
            a.drop_mode, a.drop_seed, a.drop_layer = _lib.VX_DROP_HASH, drop[1], drop[2]
        else:
            a.drop_mode = _lib.VX_DROP_MASK
            if drop[0] == "mask":
                keep.append(drop[1] if torch.is_tensor(drop[1]) else to_dev(np.asarray(drop[1], dtype=np.uint8)))
                a.drop_mask = keep[-1].data_ptr()
    before = out.clone()
    got = lib.vx_affine_gather(C.byref(a), _lib.stream_ptr())
    assert got == rc, (got, lib.vx_last_error_string())
    torch.cuda.synchronize()
    if rc != 0:
        assert torch.equal(out, before)
    return out.cpu().numpy()


def _row_lengths(c):
    """OW whose row of OW * C / 4 pieces is shorter than a 256-thread block, ends at (or next to) its edge, passes it by one
    (or as little as C / 4 allows), and spans more than two blocks without filling the last"""
    c4 = c // 4
    ows = {max(1, 100 // c4), 256 // c4, 256 // c4 + 1, -(-257 // c4), 600 // c4 + 1}
    if c4 == 1:
        assert {256, 257} <= ows
    return sorted(ows)


AFFINE_BASE = [(c, ow) for c in (4, 8, 20, 36, 720) for ow in _row_lengths(c)]


@pytest.mark.parametrize("c,ow", AFFINE_BASE, ids=[f"C{c}-OW{ow}-row{ow * c // 4}" for c, ow in AFFINE_BASE])
def test_affine_gather_base_matrix(c, ow):
    """every channel-quad count the index decode meets (C / 4 = 1, a power of two, 5, 9, 180) at row lengths on both sides of
    the 256-thread block; scale, add and relu on and off; identity and a 2x upsample; pitches above C with an offset into
    the output; `add` aliasing `out`.  N = 3 and two or more rows, so the image and row block indices count."""
    n, oh = 3, 4
    rowp = ow * c // 4
    assert (rowp + 255) // 256 >= 1
    x_id = R.f32_tensor((n, oh, ow, c), 601, 2.0)
    x_up = R.f32_tensor((n, oh // 2, (ow + 1) // 2, c), 602, 2.0)
    scale, shift = R.f32_tensor((c,), 603, 0.5, 1.0), R.f32_tensor((c,), 604, 0.5)
    add = R.f32_tensor((n, oh, ow, c), 605, 2.0)
    # every combination of: identity / 2x upsample, scale, relu, no add / an add tensor of its own / `add` aliasing `out`,
    # pitches equal to C / all above C and all different (x C + 4, add C + 8, out C + 20 at offset 8)
    for resize, use_scale, relu, add_mode, wide in itertools.product((False, True), (False, True), (False, True),
                                                                     (None, "separate", "alias"), (False, True)):
        x = x_up if resize else x_id
        kw = dict(out_hw=(oh, ow), relu=relu, add=None if add_mode is None else add)
        if use_scale:
            kw.update(scale=scale, shift=shift)
        ref = R.affine_gather_f32(x, **kw)
        if wide:
            kw.update(x_pitch=c + 4, out_pitch=c + 20, out_coff=8)
            if add_mode == "separate":
                kw.update(add_pitch=c + 8)
        full = run_affine(x, alias=add_mode == "alias", **kw)
        assert_window(full, ref, kw.get("out_coff", 0), f"resize={resize} scale={use_scale} relu={relu} add={add_mode} wide={wide}")


@pytest.mark.parametrize("src,dst", [((8, 15), (16, 30)), ((8, 15), (32, 60)), ((8, 15), (64, 120)), ((16, 30), (8, 15)),
                                     ((5, 7), (9, 20)), ((64, 120), (256, 478))],
                         ids=["up2", "up4", "up8", "down2", "5x7-9x20", "64x120-256x478"])
def test_affine_gather_resize(src, dst):
    """the bilinear gather at HRNet's ratios, a downscale and two non-dyadic sizes, plain and with scale + add + relu; the
    first and last row and column on their own, so that an edge clamp error is named"""
    x = R.f32_tensor((2, *src, 8), 611, 2.0)
    add = R.f32_tensor((2, *dst, 8), 612)
    scale, shift = R.f32_tensor((8,), 613, 0.5, 1.0), R.f32_tensor((8,), 614, 0.5)
    for kw in (dict(), dict(scale=scale, shift=shift, add=add, relu=True)):
        ref = R.affine_gather_f32(x, out_hw=dst, **kw)
        got = run_affine(x, out_hw=dst, **kw)
        assert_bits(got[:, 0], ref[:, 0], "first row")
        assert_bits(got[:, -1], ref[:, -1], "last row")
        assert_bits(got[:, :, 0], ref[:, :, 0], "first column")
        assert_bits(got[:, :, -1], ref[:, :, -1], "last column")
        assert_bits(got, ref, "interior")


@pytest.mark.parametrize("gi", [1, 2])
def test_affine_gather_group_images(gi):
    """N = 4 images in groups of gi: image n takes row n / gi of scale / shift [G][C], rows that differ per group"""
    n, c = 4, 20
    g = n // gi
    scale = R.f32_tensor((g, c), 621, 0.2, 1.0) * (1 + np.arange(g, dtype=np.float32))[:, None]
    shift = R.f32_tensor((g, c), 622, 0.2) + np.arange(g, dtype=np.float32)[:, None]
    for src, dst in (((6, 9), (6, 9)), ((3, 5), (6, 10))):
        x = R.f32_tensor((n, *src, c), 623)
        ref = R.affine_gather_f32(x, out_hw=dst, scale=scale, shift=shift, relu=True, group_images=gi)
        assert_bits(run_affine(x, out_hw=dst, scale=scale, shift=shift, relu=True, group_images=gi), ref, f"{src}->{dst}")
        one_row = R.affine_gather_f32(x, out_hw=dst, scale=scale[0], shift=shift[0], relu=True)
        assert g == 1 or (one_row[gi:] != ref[gi:]).mean() > 0.5          # the groups' rows matter


def device_hash_mask(seed, layer, n, elems):
    lib = _lib.load()
    m = torch.full((n, elems), 7, dtype=torch.uint8, device=DEV)
    _lib.check(lib.vx_drop_hash_mask(seed, layer, n, elems, _lib.ptr(m), _lib.stream_ptr()), "vx_drop_hash_mask")
    return m


@pytest.mark.parametrize("seed,layer", [(123, 0), (123, 3), (0x9E3779B9, 0), (0x9E3779B9, 3)])
def test_affine_gather_hash_dropout_is_the_exported_mask(seed, layer):
    """VX_DROP_HASH == VX_DROP_MASK with vx_drop_hash_mask's mask == the host generator's mask; C = 20: 32-element keep-words
    straddle pixels; three samples with different streams; identity and 2x upsample into a concat window"""
    n, h, w, c = 3, 6, 9, 20
    x = R.f32_tensor((n, h, w, c), 631, 2.0)
    md = device_hash_mask(seed, layer, n, h * w * c)
    host = R.hash_keep_mask(seed, layer, n, h * w * c)
    assert np.array_equal(md.cpu().numpy(), host)
    assert not np.array_equal(host[0], host[1]) and not np.array_equal(host[1], host[2])
    keep = host.reshape(n, h, w, c)
    for dst in ((h, w), (2 * h, 2 * w)):
        kw = dict(out_hw=dst, x_pitch=c + 4, out_pitch=c + 12, out_coff=4)
        ref = R.affine_gather_f32(x, out_hw=dst, keep=keep)
        hashed = run_affine(x, drop=("hash", seed, layer), **kw)
        masked = run_affine(x, drop=("mask", md), **kw)
        assert np.array_equal(hashed, masked)
        assert_window(hashed, ref, 4, f"hash dropout {dst}")
        assert (ref == 0).mean() > 0.05 and (ref != 0).mean() > 0.3


def test_affine_gather_does_not_read_padding_channels():
    """NaN in the channels [C, x_pitch) of x and [C, add_pitch) of add does not reach the output"""
    x, add = R.f32_tensor((2, 5, 7, 20), 641), R.f32_tensor((2, 10, 14, 20), 642)
    scale, shift = R.f32_tensor((20,), 643, 0.5, 1.0), R.f32_tensor((20,), 644, 0.5)
    ref = R.affine_gather_f32(x, out_hw=(10, 14), scale=scale, shift=shift, add=add, relu=True)
    full = run_affine(x, out_hw=(10, 14), scale=scale, shift=shift, add=add, relu=True, x_pitch=28, x_pad=np.nan, add_pitch=24,
                      add_pad=np.nan, out_pitch=24)
    assert np.isfinite(full).all()
    assert_window(full, ref, 0, "NaN padding")


def test_affine_gather_refusals():
    x = R.f32_tensor((1, 4, 4, 8), 651)
    s = R.f32_tensor((8,), 652)
    run_affine(x, C_override=6, rc=E_SHAPE)                               # C % 4
    run_affine(x, x_pitch=10, rc=E_ALIGN)                                 # misaligned pitches / offset
    run_affine(x, out_pitch=14, rc=E_ALIGN)
    run_affine(x, out_pitch=16, out_coff=2, rc=E_ALIGN)
    run_affine(x, out_pitch=12, out_coff=8, rc=E_ALIGN)                   # the window passes the pitch
    run_affine(x, add=x, add_pitch=10, rc=E_ALIGN)
    run_affine(x, scale=s, rc=E_NULL)                                     # scale without shift, shift without scale
    run_affine(x, shift=s, rc=E_NULL)
    run_affine(x, drop=("mask-null",), rc=E_NULL)                         # mask mode without a mask
    run_affine(x, act=_lib.VX_ACT_LRELU, rc=E_DTYPE)                      # act is none or relu
    run_affine(x, act=7, rc=E_DTYPE)


# =====================================================================================================================
# vx_fuse_sum
def run_fuse(terms, out_hw, c, *, relu=False, out_pitch=None, group_images=0, pitches=None, nterms=None, rc=0, null_x=None):
    """terms: [(x numpy [N][H][W][C], scale, shift)]; pitches: per-term x_pitch.  Returns the whole output buffer."""
    lib = _lib.load()
    n = terms[0][0].shape[0]
    out_pitch = out_pitch or c
    out = torch.full((n, *out_hw, out_pitch), SENT, dtype=torch.float32, device=DEV)
    a = _lib.FuseArgs()
    keep = []
    for t, (x, sc, sh) in enumerate(terms):
        xd = pitched(x, pitches[t] if pitches else c)
        keep.append(xd)
        a.term[t].x = None if null_x == t else xd.data_ptr()
        a.term[t].x_pitch, a.term[t].H, a.term[t].W = xd.shape[-1], x.shape[1], x.shape[2]
        for name, v in (("scale", sc), ("shift", sh)):
            if v is not None:
                keep.append(to_dev(group_rows(v, n, group_images)))
                setattr(a.term[t], name, keep[-1].data_ptr())
    a.nterms = len(terms) if nterms is None else nterms
    a.out = out.data_ptr(); a.out_pitch = out_pitch
    a.N, a.OH, a.OW, a.C = n, out_hw[0], out_hw[1], c
    a.act = _lib.VX_ACT_RELU if relu else _lib.VX_ACT_NONE
    a.group_images = group_images
    got = lib.vx_fuse_sum(C.byref(a), _lib.stream_ptr())
    assert got == rc, (got, lib.vx_last_error_string())
    torch.cuda.synchronize()
    full = out.cpu().numpy()
    if rc != 0:
        assert (full == SENT).all()
    return full


def run_chain(terms, out_hw, c, *, relu=False, group_images=0):
    """the chain of vx_affine_gather passes vx_fuse_sum replaces: the first term written, the others accumulated in place"""
    acc = None
    for t, (x, sc, sh) in enumerate(terms):
        last = t == len(terms) - 1
        full = run_affine(x, out_hw=out_hw, scale=sc, shift=sh, add=acc, alias=acc is not None, relu=relu and last, group_images=group_images)
        acc = full
    return acc


def fuse_terms(n, c, out_hw, nterms, idpos, tag, groups=0):
    """nterms terms with the identity term (null scale, output resolution) at position idpos, the others 2x, 4x, 8x upsampled"""
    terms, k = [], 0
    for t in range(nterms):
        if t == idpos:
            terms.append((R.f32_tensor((n, *out_hw, c), tag + t, 2.0), None, None))
            continue
        f = (2, 4, 8)[k]
        k += 1
        shape = (groups, c) if groups else (c,)
        sc, sh = R.f32_tensor(shape, tag + 10 + t, 0.5, 1.0), R.f32_tensor(shape, tag + 20 + t, 0.5)
        if groups:
            sc, sh = sc * (1 + np.arange(groups, dtype=np.float32))[:, None], sh + np.arange(groups, dtype=np.float32)[:, None]
        terms.append((R.f32_tensor((n, out_hw[0] // f, out_hw[1] // f, c), tag + t, 2.0), sc, sh))
    return terms


FUSE_CASES = [(nt, ip, c) for nt in (1, 2, 3, 4) for ip in range(nt) for c in (4, 20, 36)]


@pytest.mark.parametrize("nterms,idpos,c", FUSE_CASES, ids=[f"T{nt}-id{ip}-C{c}" for nt, ip, c in FUSE_CASES])
def test_fuse_sum_equals_restatement_and_chain(nterms, idpos, c):
    """1 .. 4 terms with the identity term in every position, the others resized by 2, 4 and 8; relu on and off; per-term
    pitches above C and an output pitch above C: `==` the float32 restatement and `==` the chained vx_affine_gather passes"""
    n, out_hw = 2, (16, 24)
    terms = fuse_terms(n, c, out_hw, nterms, idpos, 700 + 40 * nterms + 7 * idpos)
    for relu in (False, True):
        ref = R.fuse_sum_f32(terms, out_hw, relu=relu)
        full = run_fuse(terms, out_hw, c, relu=relu, out_pitch=c + 8, pitches=[c + 4 * (t + 1) for t in range(nterms)])
        assert_window(full, ref, 0, f"relu={relu}")
        assert_bits(run_chain(terms, out_hw, c, relu=relu), ref, f"chain, relu={relu}")
        assert_bits(run_fuse(terms, out_hw, c, relu=relu), ref, f"pitch == C, relu={relu}")


def test_fuse_sum_all_terms_scaled_and_no_identity():
    """terms that all carry scale / shift, one of them at output resolution (a scaled identity-size term)"""
    n, c, out_hw = 2, 20, (8, 12)
    terms = fuse_terms(n, c, out_hw, 3, 9, 760)
    terms.append((R.f32_tensor((n, *out_hw, c), 765), R.f32_tensor((c,), 766, 0.5, 1.0), R.f32_tensor((c,), 767, 0.5)))
    ref = R.fuse_sum_f32(terms, out_hw, relu=True)
    assert_bits(run_fuse(terms, out_hw, c, relu=True), ref, "fuse")
    assert_bits(run_chain(terms, out_hw, c, relu=True), ref, "chain")
    one = fuse_terms(n, c, out_hw, 1, 9, 768)                 # a single resized term
    assert_bits(run_fuse(one, out_hw, c), R.fuse_sum_f32(one, out_hw), "one resized term")


@pytest.mark.parametrize("gi", [1, 2])
def test_fuse_sum_group_images(gi):
    n, c, out_hw = 4, 20, (8, 16)
    terms = fuse_terms(n, c, out_hw, 3, 1, 770, groups=n // gi)
    ref = R.fuse_sum_f32(terms, out_hw, relu=True, group_images=gi)
    assert_bits(run_fuse(terms, out_hw, c, relu=True, group_images=gi), ref, "fuse")
    assert_bits(run_chain(terms, out_hw, c, relu=True, group_images=gi), ref, "chain")


def test_fuse_sum_adds_in_term_order():
    """the input whose float32 sum depends on the order (tests/test_ops2d_ref_cpu.py shows it does)"""
    terms, hw = R.order_sensitive_terms()
    c = terms[0][0].shape[-1]
    ref = R.fuse_sum_f32(terms, hw)
    assert (ref != R.fuse_sum_f32(terms, hw, reverse=True)).mean() > 0.05
    assert_bits(run_fuse(terms, hw, c), ref, "fuse")
    assert_bits(run_chain(terms, hw, c), ref, "chain")


def test_fuse_sum_refusals():
    n, c, hw = 1, 8, (4, 4)
    terms = fuse_terms(n, c, hw, 4, 0, 780)
    run_fuse(terms, hw, c, nterms=0, rc=E_SHAPE)
    run_fuse(terms, hw, c, nterms=5, rc=E_SHAPE)
    run_fuse(terms, hw, c, null_x=2, rc=E_SHAPE)
    run_fuse([terms[0], (terms[1][0], terms[1][1], None)], hw, c, rc=E_NULL)       # scale without shift
    run_fuse([terms[0], (terms[1][0], None, terms[1][2])], hw, c, rc=E_NULL)


# =====================================================================================================================
# vx_bilinear_nchw / vx_bilinear_softmax_nchw
def run_bilinear(x, out_hw, *, pitch=None, pad=0.0, dst=None, flip=None, slots=None, softmax=False, offset_floats=0):
    """x [N][H][W][C] numpy -> (out device tensor [slots][C][OH][OW], kernel name).  offset_floats: the input starts that many
    floats into its allocation (a pointer that is not 16-byte aligned)."""
    lib = _lib.load()
    n, h, w, c = x.shape
    pitch = pitch or r4(c)
    buf = torch.zeros(n * h * w * pitch + 8, dtype=torch.float32, device=DEV)
    xd = buf[offset_floats:offset_floats + n * h * w * pitch].view(n, h, w, pitch)
    xd.copy_(pitched(x, pitch, pad))
    assert xd.data_ptr() == buf.data_ptr() + 4 * offset_floats
    slots = slots or n
    out = torch.full((slots, c, *out_hw), SENT, dtype=torch.float32, device=DEV)
    dd = None if dst is None else torch.tensor(dst, dtype=torch.int32, device=DEV)
    fd = None if flip is None else torch.tensor(flip, dtype=torch.int32, device=DEV)
    fn = lib.vx_bilinear_softmax_nchw if softmax else lib.vx_bilinear_nchw
    _lib.check(fn(C.c_void_p(xd.data_ptr()), pitch, n, h, w, c, out_hw[0], out_hw[1], _lib.ptr(out), _lib.ptr(dd), _lib.ptr(fd),
                  _lib.stream_ptr()), fn.__name__)
    name = lib.vx_last_kernel_name().decode() if softmax else ""
    torch.cuda.synchronize()
    return out, name


def softmax_planar(lg):
    lib = _lib.load()
    two = torch.empty_like(lg)
    _lib.check(lib.vx_softmax_planar(_lib.ptr(lg), lg.shape[0], lg.shape[1], lg.shape[2] * lg.shape[3], _lib.ptr(two), _lib.stream_ptr()),
               "softmax_planar")
    torch.cuda.synchronize()
    return two


@pytest.mark.parametrize("src,dst", [((16, 30), (64, 120)), ((5, 7), (9, 20)), ((32, 60), (128, 239))], ids=["x4", "5x7-9x20", "32x60-128x239"])
@pytest.mark.parametrize("c", [1, 5, 19])
def test_bilinear_nchw_logits_equal_restatement(c, src, dst):
    """all four un-flip codes, permuted slots with one unused, `==` the float32 restatement.  (Finite inputs: like ATen's
    bilinear, the kernel turns 0 * inf into NaN.)"""
    x = R.f32_tensor((4, *src, c), 801, 3.0)
    dsts, flips = [4, 0, 3, 1], [0, 1, 2, 3]
    out, _ = run_bilinear(x, dst, dst=dsts, flip=flips, slots=5)
    ref = R.bilinear_nchw_f32(x, dst, dst=dsts, flip=flips, slots=5, fill=SENT)
    got = out.cpu().numpy()
    for i, s in enumerate(dsts):
        assert_bits(got[s], ref[s], f"image {i} (flip {flips[i]}) in slot {s}")
    assert (got[2] == SENT).all()
    # the flips are not no-ops on this input
    plain = R.bilinear_nchw_f32(x, dst, dst=dsts, slots=5, fill=SENT)
    assert all((plain[dsts[i]] != ref[dsts[i]]).mean() > 0.5 for i in (1, 2, 3))


SOFTMAX_INSTANCES = {1: "vec_kernel<1>", 3: "vec_kernel<1>", 4: "vec_kernel<1>", 5: "vec_kernel<2>", 8: "vec_kernel<2>",
                     9: "kernel", 12: "kernel", 13: "kernel", 16: "kernel", 17: "vec_kernel<5>", 20: "vec_kernel<5>",
                     21: "kernel", 24: "kernel", 28: "kernel", 29: "vec_kernel<8>", 32: "vec_kernel<8>", 33: "kernel"}
assert len(set(SOFTMAX_INSTANCES.values())) == 5


@pytest.mark.parametrize("c", list(SOFTMAX_INSTANCES), ids=[f"C{c}-bilinear_softmax_nchw_{k}" for c, k in SOFTMAX_INSTANCES.items()])
def test_bilinear_softmax_every_class_count_and_instance(c):
    """every channel-quad count 1 .. 8 at pitch round4(C), and 33 classes: the instance the id names ran (a vec<Q> instance
    only where the pixel holds Q quads: C = 9 .. 16 and 21 .. 28 take the scalar kernel); probabilities `==` vx_bilinear_nchw +
    vx_softmax_planar and within 1e-6 of the float64 twin; slots, both un-flips"""
    x = R.f32_tensor((3, 8, 15, c), 811, 3.0)
    dst, dsts, flips = (32, 60), [2, 0, 3], [0, 1, 3]
    pr, name = run_bilinear(x, dst, dst=dsts, flip=flips, slots=4, softmax=True)
    assert name == "bilinear_softmax_nchw_" + SOFTMAX_INSTANCES[c]
    lg, _ = run_bilinear(x, dst, dst=dsts, flip=flips, slots=4)
    two = softmax_planar(lg)
    for s in dsts:
        assert torch.equal(pr[s], two[s]), s
    assert (pr[1] == SENT).all()
    twin = R.softmax_f64(R.bilinear_nchw_f64(x, dst, dst=dsts, flip=flips, slots=4, fill=0.0), axis=1)
    err = np.abs(pr.cpu().numpy().astype(np.float64) - twin)[dsts].max()
    print(f"bilinear_softmax C={c} {name}: max |p - float64| = {err:.3e}")
    assert err < 1e-6, err
    assert_bits(lg.cpu().numpy()[dsts], R.bilinear_nchw_f32(x, dst, dst=dsts, flip=flips, slots=4, fill=SENT)[dsts], "logits")


def test_bilinear_softmax_scalar_fallback_below_33_classes():
    """C = 19 at pitch 19 (no multiple of 4) and at pitch 20 from a pointer 4 bytes off a 16-byte boundary: the scalar kernel,
    the bits of the vector instance on the same values"""
    x = R.f32_tensor((2, 8, 15, 19), 821, 3.0)
    dst = (32, 60)
    vec, name = run_bilinear(x, dst, softmax=True)
    assert name == "bilinear_softmax_nchw_vec_kernel<5>"
    for kw in (dict(pitch=19), dict(pitch=20, offset_floats=1), dict(pitch=23, offset_floats=3)):
        got, name = run_bilinear(x, dst, softmax=True, **kw)
        assert name == "bilinear_softmax_nchw_kernel", kw
        assert torch.equal(got, vec), kw
        lg, _ = run_bilinear(x, dst, **kw)
        assert_bits(lg.cpu().numpy(), R.bilinear_nchw_f32(x, dst), f"logits {kw}")


@pytest.mark.parametrize("c,pitch,inst", [(9, 20, 5), (12, 20, 5), (16, 20, 5), (21, 32, 8), (28, 32, 8)])
def test_bilinear_softmax_padded_pitch_keeps_the_vector_instance(c, pitch, inst):
    """the class counts whose pitch round4(C) holds fewer quads than the instance that covers them: with the pitch padded to
    20 / 32 (what HighResolutionNet does for its logits, whatever the pad lanes hold) the vec instance runs, with the scalar
    kernel's bits"""
    x = R.f32_tensor((2, 8, 15, c), 825, 3.0)
    scalar, n0 = run_bilinear(x, (32, 60), softmax=True)
    vec, n1 = run_bilinear(x, (32, 60), pitch=pitch, pad=np.nan, softmax=True)
    assert n0 == "bilinear_softmax_nchw_kernel" and n1 == f"bilinear_softmax_nchw_vec_kernel<{inst}>"
    assert torch.equal(scalar, vec)


@pytest.mark.parametrize("c,pitch", [(19, 20), (5, 8), (1, 4), (29, 32), (9, 12), (3, 8)])
def test_bilinear_softmax_pad_lanes_are_not_used(c, pitch):
    """NaN in the pad lanes [C, pitch): every output finite and unchanged"""
    x = R.f32_tensor((2, 8, 15, c), 831, 3.0)
    clean, n0 = run_bilinear(x, (32, 60), pitch=pitch, softmax=True)
    dirty, n1 = run_bilinear(x, (32, 60), pitch=pitch, pad=np.nan, softmax=True)
    assert n0 == n1 and torch.isfinite(dirty).all() and torch.equal(clean, dirty)
    lg, _ = run_bilinear(x, (32, 60), pitch=pitch, pad=np.nan)
    assert torch.isfinite(lg).all()


def test_bilinear_second_grid_stride_trip():
    """N = 5, 256^2 -> 1024^2, two classes: 5 242 880 output pixels for the 16384 x 256 threads the launchers start at most"""
    n, c, src, dst = 5, 2, (256, 256), (1024, 1024)
    assert n * dst[0] * dst[1] > 16384 * 256
    x = R.f32_tensor((n, *src, c), 841, 3.0)
    flips = [0, 1, 2, 3, 0]
    lg, _ = run_bilinear(x, dst, flip=flips)
    pr, name = run_bilinear(x, dst, flip=flips, softmax=True)
    assert name == "bilinear_softmax_nchw_vec_kernel<1>"
    lg, pr = lg.cpu().numpy(), pr.cpu().numpy()
    for i in range(n):                                   # (one image at a time: the host arrays stay small)
        assert_bits(lg[i], R.bilinear_nchw_f32(x[i:i + 1], dst, flip=flips[i:i + 1])[0], f"logits, image {i}")
        twin = R.softmax_f64(R.bilinear_nchw_f64(x[i:i + 1], dst, flip=flips[i:i + 1]), axis=1)[0]
        assert np.abs(pr[i] - twin).max() < 1e-6, i


# =====================================================================================================================
# vx_conv2d with the input prologue (split-fp16 kernels)
def run_conv2d(xd, cin_real, wt, ks, s, *, out_pitch=None, pre=None, fill=0.0, rc=0, args_hook=None):
    """xd: device [N][H][W][in_pitch]; wt: torch (Cout, cin_real, ks, ks) float32 on the host.  pre: dict(scale, shift, cpitch,
    gi, relu) of device tensors / ints.  Returns (out [N][OH][OW][out_pitch], stats [N * tiles][Cout][2], kernel name)."""
    lib = _lib.load()
    n, h, w, in_pitch = xd.shape
    cout = wt.shape[0]
    wd = wt.contiguous().to(DEV)
    wp = torch.empty(lib.vx_conv2d_packed_floats(cin_real, cout, ks), dtype=torch.float32, device=DEV)
    _lib.check(lib.vx_pack_conv2d(_lib.ptr(wd), _lib.ptr(wp), cin_real, cout, ks, _lib.stream_ptr()), "pack2d")
    oh, ow = (h + 2 * (ks // 2) - ks) // s + 1, (w + 2 * (ks // 2) - ks) // s + 1
    out_pitch = out_pitch or r4(cout)
    out = torch.full((n, oh, ow, out_pitch), fill, dtype=torch.float32, device=DEV)
    st = torch.full((n * lib.vx_conv2d_tiles(h, w, ks, s), cout, 2), fill, dtype=torch.float32, device=DEV)
    a = _lib.Conv2dArgs()
    a.w_family = lib.vx_conv2d_family(cin_real, cout, ks)
    a.in_ = xd.data_ptr(); a.in_pitch = in_pitch; a.w_packed = wp.data_ptr()
    a.out = out.data_ptr(); a.out_pitch = out_pitch; a.out_coff = 0
    a.N, a.H, a.W, a.Cin, a.Cout, a.KS, a.S = n, h, w, r16(cin_real), cout, ks, s
    a.stats_partial = st.data_ptr()
    if pre is not None:
        a.in_scale = None if pre.get("scale") is None else pre["scale"].data_ptr()
        a.in_shift = None if pre.get("shift") is None else pre["shift"].data_ptr()
        a.in_cpitch, a.in_group_images, a.in_relu = pre["cpitch"], pre["gi"], int(pre["relu"])
    if args_hook:
        args_hook(a)
    got = lib.vx_conv2d(C.byref(a), _lib.stream_ptr())
    if got > 0:                                          # a HIP error code, not a refusal: not an ordinary test failure
        raise _lib.VxError(f"vx_conv2d: HIP error {got}: {lib.vx_last_error_string()}")
    assert got == rc, (got, lib.vx_last_error_string())
    name = lib.vx_last_kernel_name().decode()
    torch.cuda.synchronize()
    return out, st, name


def affine_dev(xd, c, scale, shift, relu, gi):
    """vx_affine_gather on device tensors: the activated tensor at the pitch of xd (c == the pitch: every channel written)"""
    lib = _lib.load()
    n, h, w, pitch = xd.shape
    assert c == pitch
    out = torch.full_like(xd, SENT)
    a = _lib.AffineArgs()
    a.x = xd.data_ptr(); a.x_pitch = pitch; a.scale = scale.data_ptr(); a.shift = shift.data_ptr()
    a.out = out.data_ptr(); a.out_pitch = pitch
    a.N, a.H, a.W, a.C, a.OH, a.OW = n, h, w, c, h, w
    a.act = _lib.VX_ACT_RELU if relu else _lib.VX_ACT_NONE
    a.group_images = gi
    _lib.check(lib.vx_affine_gather(C.byref(a), _lib.stream_ptr()), "affine")
    torch.cuda.synchronize()
    return out


def conv2d_dry_run(a):
    """vx_conv2d_route of the arguments `a`: (kernel name, nchunks, w_all, grid_x) of the launch they make"""
    lib = _lib.load()
    buf, info = C.create_string_buffer(128), _lib.Conv2dRouteInfo()
    _lib.check(lib.vx_conv2d_route(C.byref(a), buf, len(buf), C.byref(info)), "vx_conv2d_route")
    return buf.value.decode(), info.nchunks, info.w_all, info.grid_x


def prologue_case(cin, cout, ks, s, n, h, w, *, narrow=False, gi=0, relu=True, cpitch_extra=0, tag=900, name=None, nchunks=None,
                  w_all=None, multi_item=False, report=None):
    """conv -> BN -> ReLU -> conv as in BasicBlock: a first vx_conv2d (16 -> cin, 3x3) leaves raw output and statistics
    partials, vx_bn_finalize_groups folds them with gamma / beta that make shift > 0 on most channels, and the layer under test
    runs (a) with the prologue on the raw tensor and (b) without it on vx_affine_gather's activated tensor."""
    lib = _lib.load()
    c0 = 16
    in_pitch = r4(cin) if narrow else r16(cin)
    cpitch = in_pitch + cpitch_extra
    assert not (gi and cpitch_extra)                     # (vx_affine_gather's group rows are C apart)
    x0 = R.f32_tensor((n, h, w, c0), tag)
    groups = n // gi if gi else 1
    if gi:                                               # groups that differ strongly: amplitude 1 + g, offset g / 2
        assert n % gi == 0
        gidx = (np.arange(n) // gi).astype(np.float32)[:, None, None, None]
        x0 = (x0 * (1 + gidx) + 0.5 * gidx).astype(np.float32)
    w1 = torch.from_numpy(R.f32_tensor((cin, c0, 3, 3), tag + 1, (1.0 / (9 * c0)) ** 0.5))
    y1, st1, _ = run_conv2d(to_dev(x0), c0, w1, 3, 1, out_pitch=in_pitch)          # pad channels [cin, in_pitch) hold zeros
    tpi = lib.vx_conv2d_tiles(h, w, 3, 1)
    gamma, beta = to_dev(R.f32_tensor((cin,), tag + 2, 0.3, 1.0)), to_dev(R.f32_tensor((cin,), tag + 3, 0.3, 0.6))
    # (n rows: a pass that took row n instead of row n / in_group_images would still read inside the buffer)
    scale = torch.zeros((n, cpitch), dtype=torch.float32, device=DEV)
    shift = torch.zeros_like(scale)
    per = gi or n
    _lib.check(lib.vx_bn_finalize_groups(_lib.ptr(st1), per * tpi, groups, cin, cpitch, per * h * w, 1e-5, _lib.ptr(gamma), _lib.ptr(beta),
                                         _lib.ptr(scale), _lib.ptr(shift), _lib.stream_ptr()), "bn_finalize_groups")
    w2 = torch.from_numpy(R.f32_tensor((cout, cin, ks, ks), tag + 4, (1.0 / (ks * ks * cin)) ** 0.5))
    pre = dict(scale=scale, shift=shift, cpitch=cpitch, gi=gi, relu=relu)
    out_pitch = r4(cout) + 8
    route = []                                           # the dry run of the very arguments the launch below takes
    fused, stf, kname = run_conv2d(y1, cin, w2, ks, s, out_pitch=out_pitch, pre=pre, fill=SENT, args_hook=lambda a: route.append(conv2d_dry_run(a)))
    if name is not None:
        assert kname == name, kname
    total_tiles = n * lib.vx_conv2d_tiles(h, w, ks, s)
    dry_name, got_chunks, got_w_all, wgs = route[0]
    assert dry_name == kname, (dry_name, kname)
    if nchunks is not None:
        assert (got_chunks, got_w_all) == (nchunks, w_all), (got_chunks, got_w_all)
    if multi_item:                                       # more tiles than workgroups: persistent workgroups take several
        assert total_tiles > wgs and total_tiles > 512, (total_tiles, wgs)
    # (b) the two passes
    act = affine_dev(y1, in_pitch, scale[:, :in_pitch].contiguous(), shift[:, :in_pitch].contiguous(), relu, gi)
    two, st2, kname2 = run_conv2d(act, cin, w2, ks, s, out_pitch=out_pitch, fill=SENT)
    assert kname2 == kname
    assert torch.equal(fused, two), f"output: {(fused != two).sum().item()} elements differ from the two-pass form"
    assert torch.equal(stf, st2), "statistics partials differ from the two-pass form"
    assert (fused[..., r4(cout):] == SENT).all()
    # the restated activated tensor and its float64 convolution
    sc, sh = scale.cpu().numpy()[:groups, :cin], shift.cpu().numpy()[:groups, :cin]
    assert (sh > 0).mean() > 0.5 and (scale[:, cin:] == 0).all() and (shift[:, cin:] == 0).all()
    y1h = y1.cpu().numpy()
    assert (y1h[..., cin:] == 0).all()
    act_ref = R.affine_gather_f32(y1h[..., :cin], scale=sc if gi else sc[0], shift=sh if gi else sh[0], relu=relu, group_images=gi)
    acth = act.cpu().numpy()
    assert_bits(acth[..., :cin], act_ref, "vx_affine_gather vs its restatement")
    assert (acth[..., cin:] == 0).all()
    at = torch.from_numpy(act_ref).permute(0, 3, 1, 2).double()
    ref = F.conv2d(at, w2.double(), stride=s, padding=ks // 2)
    got = fused[..., :cout].permute(0, 3, 1, 2).cpu().double()
    mag = max(1.0, float(np.abs(act_ref).max()))
    bound = 3e-5 * mag
    err = (got - ref).abs()
    ring = max(err[:, :, 0].max().item(), err[:, :, -1].max().item(), err[:, :, :, 0].max().item(), err[:, :, :, -1].max().item())
    print(f"prologue {kname} {cin}->{cout} k{ks}s{s} n{n} {h}x{w}: max err {err.max().item():.3e} (border ring {ring:.3e}), bound {bound:.3e}")
    assert ring <= bound, f"border ring: {ring:.3e} > {bound:.3e}"
    assert err.max().item() <= bound, f"{err.max().item():.3e} > {bound:.3e}"
    ssum = stf.double().sum(0).cpu()
    np.testing.assert_allclose(ssum[:, 0].numpy(), ref.sum((0, 2, 3)).numpy(), rtol=1e-4, atol=2e-3)
    np.testing.assert_allclose(ssum[:, 1].numpy(), (ref * ref).sum((0, 2, 3)).numpy(), rtol=1e-4, atol=2e-3)
    if ks == 3:
        # the test can tell: padding with the activated value of a zero input (act(shift)) instead of zero moves the border
        # ring by far more than the bound
        padv = torch.from_numpy(np.maximum(sh, 0) if relu else sh).double()[np.arange(n) // gi if gi else np.zeros(n, dtype=np.int64)]
        wrong = padv[:, :, None, None].expand(n, cin, h + 2, w + 2).clone()
        wrong[:, :, 1:-1, 1:-1] = at
        d = (F.conv2d(wrong, w2.double(), stride=s) - ref).abs()
        assert d[:, :, 0].max().item() > 20 * bound and d[:, :, :, 0].max().item() > 20 * bound
    if report is not None:
        report.append((kname, err.max().item() / mag))
    return kname


K = "conv2d_s16_kernel<%d,%d,%d,%d,16,%d>"
# (cin, cout, ks, s, n, h, w, options, configuration, instance, chunks, weights resident)
PROLOGUE_CASES = [
    # 3x3 stride 1: one, two, three sub-blocks per item; several chunks with resident and with re-staged weights
    (16, 16, 3, 1, 2, 20, 33, {}, {}, K % (3, 1, 1, 1, 0), 1, 0),
    (32, 32, 3, 1, 2, 17, 21, {}, {}, K % (3, 1, 2, 2, 0), 1, 0),
    (48, 48, 3, 1, 2, 20, 33, {}, {}, K % (3, 1, 3, 3, 0), 1, 0),
    (64, 16, 3, 1, 2, 20, 33, {}, {}, K % (3, 1, 1, 1, 0), 4, 1),
    (80, 48, 3, 1, 2, 9, 35, {}, {}, K % (3, 1, 3, 1, 0), 5, 0),
    (32, 32, 3, 1, 2, 17, 21, {}, {"c2s_no_wide": 1}, K % (3, 1, 2, 1, 0), 2, 1),
    (48, 36, 3, 1, 2, 17, 21, {}, {"c2s_no_wide": 1}, K % (3, 1, 3, 1, 0), 3, 1),
    # 3x3 stride 2, odd H and W
    (32, 36, 3, 2, 2, 17, 31, {}, {}, K % (3, 2, 3, 1, 0), 2, 1),
    (64, 48, 3, 2, 2, 17, 31, {}, {}, K % (3, 2, 3, 1, 0), 4, 0),
    (16, 18, 3, 2, 2, 33, 19, {}, {}, K % (3, 2, 2, 1, 0), 1, 0),
    # 1x1: one chunk, four, twelve; row tiles 1, 2, 3, 5
    (64, 16, 1, 1, 2, 20, 33, {}, {}, K % (1, 1, 1, 4, 0), 1, 0),
    (256, 72, 1, 1, 2, 9, 21, {}, {}, K % (1, 1, 5, 4, 0), 4, 1),
    (720, 72, 1, 1, 2, 9, 21, {}, {}, K % (1, 1, 5, 4, 0), 12, 0),
    (256, 32, 1, 1, 2, 9, 21, {}, {}, K % (1, 1, 2, 4, 0), 4, 1),
    (720, 48, 1, 1, 1, 9, 21, {}, {}, K % (1, 1, 3, 4, 0), 12, 0),
    (720, 16, 1, 1, 1, 9, 21, {}, {}, K % (1, 1, 1, 4, 0), 12, 1),
    # both octet families (8 real channels; 18 at pitch 20), stride 1 and 2, and the same layers without them
    (8, 16, 3, 1, 2, 20, 33, {"narrow": True}, {}, K % (3, 1, 1, 1, 1), 1, 0),
    (18, 18, 3, 1, 2, 20, 33, {"narrow": True}, {}, K % (3, 1, 2, 1, 3), 1, 0),
    (18, 36, 3, 2, 2, 17, 31, {"narrow": True}, {}, K % (3, 2, 3, 1, 3), 1, 0),
    (8, 16, 3, 2, 2, 17, 31, {"narrow": True}, {}, K % (3, 2, 1, 1, 1), 1, 0),
    (8, 16, 3, 1, 2, 20, 33, {"narrow": True}, {"c2s_no_oct": 1}, K % (3, 1, 1, 1, 0), 1, 0),
    (18, 18, 3, 1, 2, 20, 33, {"narrow": True}, {"c2s_no_oct": 1}, K % (3, 1, 2, 2, 0), 1, 0),
    (18, 18, 3, 1, 2, 20, 33, {"narrow": True}, {"c2s_no_wide": 1}, K % (3, 1, 2, 1, 3), 1, 0),
    (8, 16, 3, 1, 2, 20, 33, {"narrow": True}, {"c2s_no_wide": 1}, K % (3, 1, 1, 1, 1), 1, 0),
    (18, 18, 3, 1, 2, 20, 33, {"narrow": True}, {"c2s_no_oct": 1, "c2s_no_wide": 1}, K % (3, 1, 2, 1, 0), 2, 1),
    (18, 36, 3, 2, 2, 17, 31, {"narrow": True}, {"c2s_no_oct": 1}, K % (3, 2, 3, 1, 0), 2, 1),
    # a single tile smaller than the tile; no ReLU; scale / shift rows longer than the pitch; statistics groups
    (16, 16, 3, 1, 2, 5, 7, {}, {}, K % (3, 1, 1, 1, 0), 1, 0),
    (64, 16, 1, 1, 2, 5, 7, {}, {}, K % (1, 1, 1, 4, 0), 1, 0),
    (16, 16, 3, 1, 2, 20, 33, {"relu": False}, {}, K % (3, 1, 1, 1, 0), 1, 0),
    (256, 32, 1, 1, 2, 9, 21, {"relu": False}, {}, K % (1, 1, 2, 4, 0), 4, 1),
    (18, 18, 3, 1, 2, 20, 33, {"narrow": True, "cpitch_extra": 16}, {}, K % (3, 1, 2, 1, 3), 1, 0),
    (64, 16, 3, 1, 4, 20, 33, {"gi": 2}, {}, K % (3, 1, 1, 1, 0), 4, 1),
    (18, 18, 3, 1, 4, 20, 33, {"narrow": True, "gi": 1}, {}, K % (3, 1, 2, 1, 3), 1, 0),
    # persistent workgroups with several items whose consecutive items change statistics group: one chunk, several chunks
    (16, 16, 3, 1, 12, 112, 112, {"gi": 3, "multi_item": True}, {}, K % (3, 1, 1, 1, 0), 1, 0),
    (64, 16, 3, 1, 12, 112, 112, {"gi": 3, "multi_item": True}, {}, K % (3, 1, 1, 1, 0), 4, 1),
]


def _prologue_id(p):
    cin, cout, ks, s, n, h, w, opt, cfg, name, nchunks, w_all = p
    extra = "".join(f"-{k}{'' if v is True else v}" for k, v in {**opt, **cfg}.items())
    return f"{cin}to{cout}-k{ks}s{s}-n{n}-{h}x{w}{extra}-{name.replace('conv2d_s16_kernel', '')}-chunks{nchunks}-wall{w_all}"


@pytest.mark.parametrize("p", PROLOGUE_CASES, ids=[_prologue_id(p) for p in PROLOGUE_CASES])
def test_conv2d_prologue_equals_two_passes_and_float64(p, vxcfg):
    cin, cout, ks, s, n, h, w, opt, cfg, name, nchunks, w_all = p
    vxcfg.set(conv_fp32=0, c2s_no_oct=0, c2s_no_wide=0)
    if cfg:
        vxcfg.set(**cfg)
    prologue_case(cin, cout, ks, s, n, h, w, name=name, nchunks=nchunks, w_all=w_all, tag=900 + 10 * PROLOGUE_CASES.index(p), **opt)


def test_conv2d_prologue_refusals(vxcfg):
    """each refusal: the error code, and output and statistics untouched"""
    vxcfg.set(conv_fp32=0)
    xd = to_dev(R.f32_tensor((1, 8, 8, 32), 991))
    wt = torch.from_numpy(R.f32_tensor((16, 32, 3, 3), 992, 0.05))
    sc, sh = torch.ones((1, 32), device=DEV), torch.zeros((1, 32), device=DEV)

    def refused(pre, rc):
        out, st, _ = run_conv2d(xd, 32, wt, 3, 1, pre=pre, fill=SENT, rc=rc)
        assert (out == SENT).all() and (st == SENT).all()

    refused(dict(scale=sc, shift=None, cpitch=32, gi=0, relu=1), E_NULL)
    refused(dict(scale=None, shift=sh, cpitch=32, gi=0, relu=1), E_NULL)
    refused(dict(scale=sc, shift=sh, cpitch=16, gi=0, relu=1), E_SHAPE)            # in_cpitch < Cin - 15
    refused(dict(scale=sc, shift=sh, cpitch=32, gi=-1, relu=1), E_SHAPE)
    out, st, _ = run_conv2d(xd, 32, wt, 3, 1, pre=dict(scale=sc, shift=sh, cpitch=17, gi=0, relu=1), fill=SENT)   # 17 = Cin - 15: accepted
    assert (out[..., :16] != SENT).all()
    vxcfg.set(conv_fp32=1)                                                         # (weights packed for the fp32 family)
    refused(dict(scale=sc, shift=sh, cpitch=32, gi=0, relu=1), E_SHAPE)
    out, _, _ = run_conv2d(xd, 32, wt, 3, 1, fill=SENT)                            # ... which runs the layer without a prologue
    assert (out[..., :16] != SENT).all()


def test_fuzz_conv2d_prologue_fixed_seed_slice(vxcfg):
    """tools/fuzz_conv2d.py, kind `pre`, for a fixed seed: random layers through the prologue against the two-pass form and the
    float64 oracle"""
    vxcfg.set(conv_fp32=0, c2s_no_oct=0, c2s_no_wide=0)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("vx_fuzz_conv2d", os.path.join(root, "tools", "fuzz_conv2d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cases, bad, names = mod.run_pre_cases(24, 2026)
    assert bad == 0 and cases == 24
    assert len(names) >= 6, names
