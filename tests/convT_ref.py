"""A plain float64 restatement of a whole vx_convT_k2s2 launch: the up-convolution, the activation, the dropout and the two output
layouts, with the error bound a correct kernel must meet.  numpy / torch only; nothing is imported from the library (the case
dictionaries are those of tests/convT_route_cases.py).  Every function takes CPU or device tensors and computes where they live.

    expected()            E (float64, NCDHW), the keep mask and S = sum_ci |w| |x| per output element
    offsets()             the flat float offset of every NCDHW output element inside the launch's buffer: the set the launch may write
    tolerance()           per element, derived below
    emulate_fp32/_split   what a correct kernel of either arithmetic computes, for tests/test_convT_ref_cpu.py
    compare()             the worst |got - E| / tol and the first element beyond it

The bound.  u = 2^-24 is the unit roundoff of float32, S the sum of the absolute exact products of an output element.

  fp32 families (mfma, rows, generic): the bias is the accumulator's first value, Cin products are added to it in some order (fmaf or
      the matrix instruction: one rounding per addition at most), the LeakyReLU multiply rounds once more.  The classical bound of a
      recursive sum in any order is n u times the sum of the absolute terms for n roundings; with one spare rounding

          tol32 = (Cin + 2) u (S + |b|)

  s16 family (convT_k2s2_s16_kernel): both operands are split as v = hi + lo / 2048 + e, hi = fp16(v), lo = fp16(2048 (v - hi))
      (vx_split4 in s16_common.h for the activations, the same two statements for the weights in convtranspose.hip; v - hi and its
      scaling are exact in float32, tests/conv_lattice.split restates them).  With h = 2^-11, the unit roundoff of fp16:
          |v - hi| <= h |v|,   |lo / 2048| <= h (1 + h) |v|,   |e| <= h^2 |v|            (normal fp16 range)
      Below 2^-14 fp16 is a fixed grid of spacing 2^-24, so there |e| <= 2^-25 / 2048 = 2^-36 instead: |e| <= h^2 |v| + 2^-36.
      The kernel forms  hi_x hi_w + (lo_x hi_w + hi_x lo_w) / 2048  and drops
          x w - that = lo_x lo_w / 2048^2 + e_x w + (x - e_x) e_w
                    <= |x| |w| h^2 ((1 + h)^2 + 1 + (1 + h^2)) + 2^-36 (|w| + |x| (1 + h^2))
                    <= 3 (1 + 2^-10) 2^-22 |x| |w| + 2^-34         for |x|, |w| <= 2 (asserted where the inputs are made).
      Its three kinds of products are exact in the matrix instruction; they are accumulated in float32: the main sum (bias first, Cin
      products of size <= (1 + h)^2 |x| |w|), the cross sum (2 Cin products of size <= h (1 + h)^2 |x| |w|, error <= 2 Cin u 2 h (1 + h)^2
      S), one fmaf that combines them and the activation multiply: (Cin + 2) u (1 + h)^2 (S + |b|) + Cin u 2^-9 (1 + h)^2 S, which is
      below (1 + 2^-8) tol32.  This is the structure tests/conv_lattice.py proves for its `lo` flavour (there the sums are exact and
      3 u (|M| + |X| / 2048 + |b|) remains for the combine, the bias and a spare); here the sums round as well.  Altogether

          tol16 = (1 + 2^-8) (tol32 + 3 * 2^-22 S) + Cin 2^-34

  ReLU and LeakyReLU are 1-Lipschitz: the bound passes through them.  Dropout multiplies by exactly 2 or 0: a kept element has twice
  the tolerance, a dropped one tolerance 0 -- got == 0, and -0.0 is equal to 0.

Not derived: how the matrix instructions round INSIDE one instruction (four or 32 products per accumulator update).  The bound assumes
no step is worse than a correctly rounded float32 addition."""
import numpy as np
import torch

from tests.ops2d_ref import hash_keep_mask

ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2
DROP_NONE, DROP_HASH, DROP_MASK = 0, 1, 2
DROP_SEED, DROP_LAYER = 77, 3                 # what tests/convT_route_cases.layer_args passes
SLOPE = float(np.float32(0.01))               # the kernels' 0.01f, as the double it is
U24, U11 = 2.0 ** -24, 2.0 ** -11
SENTINEL = -77.0
FP32_FAMILIES = ("mfma", "rows", "generic")


def family_of(kernel_name):
    """'mfma' | 's16' | 'rows' | 'generic' from the name vx_last_kernel_name() / the dry run reports"""
    for f in ("mfma", "s16", "rows"):
        if kernel_name.startswith("convT_k2s2_%s_kernel" % f):
            return f
    assert kernel_name == "convT_k2s2_kernel", kernel_name
    return "generic"


def _act(v, act):
    if act == ACT_RELU:
        return torch.clamp_min(v, 0.0)
    if act == ACT_LRELU:
        return torch.maximum(v, SLOPE * v)
    return v


def keep_mask(case, n_samples, mask=None, seed_dev=0, sample0=0, drop_seed=DROP_SEED, device="cpu"):
    """bool (n_samples, Cout, 2D, 2H, 2W): the elements the dropout keeps, for samples sample0 .. of the launch"""
    _, d, h, w = case["vol"]
    co = case["cout"]
    if case["drop"] == DROP_NONE:
        return torch.ones((n_samples, co, 2 * d, 2 * h, 2 * w), dtype=torch.bool, device=device)
    if case["drop"] == DROP_HASH:
        # one stream per sample of the LAUNCH: the key takes the sample's index, the element index is ((oz OH + oy) OW + ox) Cout + co
        seed = (int(drop_seed) + int(seed_dev)) % (1 << 32)
        k = hash_keep_mask(seed, DROP_LAYER, sample0 + n_samples, 8 * d * h * w * co)[sample0:]
        k = torch.from_numpy(k.reshape(n_samples, 2 * d, 2 * h, 2 * w, co)).to(device)
    else:
        k = mask[sample0:sample0 + n_samples].to(device)       # [N][2D][2H][2W][Cout], as the launch reads it
    return (k != 0).permute(0, 4, 1, 2, 3)


def expected(case, x, w, b, mask=None, seed_dev=0, sample0=0, drop_seed=DROP_SEED):
    """x [n][D][H][W][Cin] (samples sample0 .. sample0 + n of the launch), w (Cin, Cout, 2, 2, 2), b (Cout), mask [N][2D][2H][2W][Cout]
    or None -> (E, keep, S): float64 / bool / float64, each (n, Cout, 2D, 2H, 2W), on x's device"""
    x, w, b = x.double(), w.double().to(x.device), b.double().to(x.device)
    n, d, h, wd, _ = x.shape
    assert (d, h, wd) == tuple(case["vol"][1:]) and w.shape == (case["cin"], case["cout"], 2, 2, 2)
    shape = (n, case["cout"], 2 * d, 2 * h, 2 * wd)
    # out[n, co, 2z + dz, 2y + dy, 2x + dx] = b[co] + sum_ci x[n, z, y, x, ci] w[ci, co, dz, dy, dx]
    E = torch.einsum("nzyxi,iopqr->nozpyqxr", x, w).reshape(shape) + b.view(1, -1, 1, 1, 1)
    S = torch.einsum("nzyxi,iopqr->nozpyqxr", x.abs(), w.abs()).reshape(shape)
    E = _act(E, case["act"])
    keep = keep_mask(case, n, mask, seed_dev, sample0, drop_seed, x.device)
    if case["drop"] != DROP_NONE:
        E = torch.where(keep, 2.0 * E, torch.zeros_like(E))
    return E, keep, S


def tolerance(case, S, b, family, keep=None):
    """per element, see the module docstring; keep: the keep mask of a launch with dropout"""
    cin = case["cin"]
    tol = (cin + 2) * U24 * (S + b.double().to(S.device).abs().view(1, -1, 1, 1, 1))
    if family == "s16":
        tol = (1.0 + 2.0 ** -8) * (tol + 3.0 * 2.0 ** -22 * S) + cin * 2.0 ** -34
    else:
        assert family in FP32_FAMILIES, family
    if case["drop"] != DROP_NONE:
        tol = torch.where(keep, 2.0 * tol, torch.zeros_like(tol))
    return tol


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
def buffer_floats(case):
    """floats of the buffer the launch writes into"""
    n, d, h, w = case["vol"]
    return n * 8 * d * h * w * (2 * case["cout"] if case["xblk"] else case["cout"] + case["out_extra"])


def plain_offsets(vol, cout, pitch, coff, n0=0, n1=None, device="cpu"):
    """[N][2D][2H][2W][pitch], channels [coff, coff + cout): int64 (n1 - n0, cout, 2D, 2H, 2W)"""
    n, d, h, w = vol
    n1 = n if n1 is None else n1
    ar = lambda k, pos: torch.arange(k, dtype=torch.int64, device=device).view([-1 if i == pos else 1 for i in range(5)])
    nn, co, oz, oy, ox = ar(n1 - n0, 0) + n0, ar(cout, 1), ar(2 * d, 2), ar(2 * h, 3), ar(2 * w, 4)
    return (((nn * (2 * d) + oz) * (2 * h) + oy) * (2 * w) + ox) * pitch + coff + co


def concat_offsets(vol, cout, xb, half, n0=0, n1=None, device="cpu"):
    """[N][2D][2H][2W / xb][2][xb][cout], half `half`: int64 (n1 - n0, cout, 2D, 2H, 2W)"""
    n, d, h, w = vol
    n1 = n if n1 is None else n1
    assert xb in (1, 2, 4) and (2 * w) % xb == 0 and half in (0, 1)
    ar = lambda k, pos: torch.arange(k, dtype=torch.int64, device=device).view([-1 if i == pos else 1 for i in range(5)])
    nn, co, oz, oy, ox = ar(n1 - n0, 0) + n0, ar(cout, 1), ar(2 * d, 2), ar(2 * h, 3), ar(2 * w, 4)
    row = (nn * (2 * d) + oz) * (2 * h) + oy
    return (((row * ((2 * w) // xb) + ox // xb) * 2 + half) * xb + ox % xb) * cout + co


def offsets(case, n0=0, n1=None, device="cpu"):
    """the case's layout: where element (n, co, oz, oy, ox) of samples n0 .. n1 lies in the buffer -- the set the launch may write"""
    if case["xblk"]:
        return concat_offsets(case["vol"], case["cout"], case["xblk"], case["half"], n0, n1, device)
    return plain_offsets(case["vol"], case["cout"], case["cout"] + case["out_extra"], case["out_coff"], n0, n1, device)


def scatter(case, values, buf=None):
    """values (N, Cout, 2D, 2H, 2W) written through the case's layout into a flat buffer prefilled with the sentinel"""
    if buf is None:
        buf = torch.full((buffer_floats(case),), SENTINEL, dtype=values.dtype, device=values.device)
    buf[offsets(case, device=values.device).reshape(-1)] = values.reshape(-1)
    return buf


def gather(case, buf, n0=0, n1=None):
    return buf.reshape(-1)[offsets(case, n0, n1, buf.device)]


# ---- comparison -------------------------------------------------------------------------------------------------------------------
def compare(got, E, tol):
    """(worst |got - E| / tol, index of the first element beyond its tolerance or None).  Where tol == 0 the element must equal E
    (ratio inf otherwise); a NaN is beyond any tolerance"""
    inf = float("inf")
    err = (got.double() - E).abs()
    bad = ~(err <= tol)
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, inf)))
    ratio = float(r.nan_to_num(nan=inf, posinf=inf).max())
    first = tuple(int(v) for v in bad.nonzero()[0]) if bool(bad.any()) else None
    return ratio, first


def describe(case, first, got, E, tol, n0=0):
    """the failure message: the element, its input voxel and the column tile of 16 input voxels the tile kernels handle it in"""
    n, co, oz, oy, ox = first
    _, d, h, w = case["vol"]
    v = (((n + n0) * d + oz // 2) * h + oy // 2) * w + ox // 2
    return "%s: first bad (n, co, oz, oy, ox) = %s: got %.9g want %.9g tol %.3g; input voxel (n, z, y, x) = %s = flat %d, column tile %d" % (
        case["id"], (n + n0, co, oz, oy, ox), float(got[first]), float(E[first]), float(tol[first]), (n + n0, oz // 2, oy // 2, ox // 2), v, v // 16)


# ---- emulations: what a correct kernel computes (CPU) -----------------------------------------------------------------------------
def _f32(t):
    return t.float().double()


def _prods(x, w, ci, out=None):
    """the products of channel ci, (n, Cout, D, 2, H, 2, W, 2) float64 (a view of the NCDHW shape), exact for float32 / fp16 operands"""
    n, d, h, wd, _ = x.shape
    return torch.mul(x[..., ci].reshape(n, 1, d, 1, h, 1, wd, 1), w[ci].reshape(1, -1, 1, 2, 1, 2, 1, 2), out=out)


def _epilogue32(case, acc, keep):
    """the kernels' epilogue on float32 values held as doubles"""
    if case["act"] == ACT_RELU:
        acc = torch.clamp_min(acc, 0.0)
    elif case["act"] == ACT_LRELU:
        acc = torch.maximum(acc, _f32(SLOPE * acc))
    if case["drop"] != DROP_NONE:
        acc = torch.where(keep, 2.0 * acc, torch.zeros_like(acc))
    return acc


def emulate_fp32(case, x, w, b, keep):
    """sequential float32 fmaf over ci from the bias (the product is exact in float64; the sum is rounded to float64, then to float32)"""
    x, w = x.double(), w.double()
    n, d, h, wd, _ = x.shape
    acc = b.double().view(1, -1, 1, 1, 1, 1, 1, 1).expand(n, -1, d, 2, h, 2, wd, 2).clone()
    tmp = torch.empty_like(acc)
    for ci in range(case["cin"]):
        _prods(x, w, ci, tmp).add_(acc)
        acc.copy_(tmp.float())
    acc = acc.view(n, -1, 2 * d, 2 * h, 2 * wd)
    return _epilogue32(case, acc, keep)


def split16(v):
    """v (float32 values) -> (hi, lo) as doubles, the statements of vx_split4 / the weight split: hi = fp16(v), lo = fp16((v - hi) 2048)"""
    v = v.float()
    hi = v.half()
    lo = ((v - hi.float()) * 2048.0).half()
    return hi.double(), lo.double()


def emulate_split(case, x, w, b, keep):
    """the split-fp16 kernel: hi / lo exactly as it forms them, products in float64, the main and the cross accumulator rounded to
    float32 once per 32 channels and operand pair (one matrix instruction each), then fmaf(cross, 1 / 2048, main)"""
    hx, lx = split16(x)
    hw, lw = split16(torch.clamp(w.float(), -65504.0, 65504.0))
    n, d, h, wd, _ = x.shape
    main = b.double().view(1, -1, 1, 1, 1, 1, 1, 1).expand(n, -1, d, 2, h, 2, wd, 2).clone()
    cross = torch.zeros_like(main)
    for q in range(0, case["cin"], 32):
        hh, hl, lh = (sum(_prods(a, c, ci) for ci in range(q, q + 32)) for a, c in ((hx, hw), (lx, hw), (hx, lw)))
        main = _f32(main + hh)
        cross = _f32(_f32(cross + hl) + lh)
    main, cross = (t.view(n, -1, 2 * d, 2 * h, 2 * wd) for t in (main, cross))
    return _epilogue32(case, _f32(cross / 2048.0 + main), keep)
