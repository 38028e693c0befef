"""CPU: pins tests/ops3d_ref.py, the host restatement the GPU matrix of the 3D streaming kernels (tests/test_gpu_stream3d.py)
compares with -- its float64 twins against torch and the oracle's contract block, the pool-finish identity the header claims,
the split round trip, the derived conditioning bounds, and the exactness range of the launcher's multiply-high index decode."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ops3d_ref as R
from tests.formula import formula_tensor


def _cl(t):            # NCDHW torch -> channels-last numpy
    return t.permute(0, 2, 3, 4, 1).contiguous().numpy()


def _nc(a):            # channels-last numpy -> NCDHW torch
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 4, 1, 2, 3).contiguous()


def _x(shape, tag, scale=3.0, off=1.5):
    return (formula_tensor(shape, tag, scale) + off).astype(np.float32)


def _keep(shape, tag):
    return (formula_tensor(shape, tag) > 0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_LRELU, R.ACT_RELU])
@pytest.mark.parametrize("drop", [False, True])
def test_float64_twins_match_torch(act, drop):
    shape = (3, 4, 6, 10, 8)
    x = _x(shape, 11)
    keep = _keep(shape, 12) if drop else None
    mu, var, rstd = R.instnorm_two_pass(x)
    got = R.norm_act_drop_f64(x, mu, rstd, act, keep)
    t = F.instance_norm(_nc(x).double(), eps=float(np.float32(1e-5)))
    t = {R.ACT_NONE: lambda v: v, R.ACT_LRELU: lambda v: F.leaky_relu(v, 0.01), R.ACT_RELU: F.relu}[act](t)
    if drop:
        t = t * _nc(keep).double() * 2.0
    assert np.abs(got - _cl(t)).max() < 1e-13
    assert np.abs(R.maxpool2_f64(got) - _cl(F.max_pool3d(t, 2, 2))).max() < 1e-13
    assert np.array_equal(R.maxpool2_f32(got.astype(np.float32)), _cl(F.max_pool3d(_nc(got.astype(np.float32)), 2, 2)))


def test_statistics_from_exact_partials_are_the_two_pass_statistics():
    x = _x((2, 4096, 8), 21).reshape(2, 16, 16, 16, 8)
    part, count = R.ideal_partials(x, 37)
    assert count == 4096 and part.shape == (2, 37, 8, 2)
    mu, rstd, mu32, rs32 = R.instnorm_from_partials(part, count)
    mu2, var2, rstd2 = R.instnorm_two_pass(x)
    assert np.abs(mu - mu2).max() < 1e-6 and np.abs(rstd / rstd2 - 1).max() < 1e-6
    assert mu32.dtype == np.float32 and np.array_equal(mu32, mu.astype(np.float32)) and np.array_equal(rs32, rstd.astype(np.float32))
    # a negative computed variance clamps (ops2d_ref.clamp_partials, channel 1)
    from tests.ops2d_ref import clamp_partials
    cp, n = clamp_partials()
    _, r, _, _ = R.instnorm_from_partials(cp[None], n)
    assert np.all(r == 1.0 / np.sqrt(float(np.float32(1e-5))))


def test_contract_block_of_the_oracle_states_the_same_sequence():
    """oracle/unet3d_oracle.py's _contract: conv -> InstanceNorm -> LeakyReLU -> Dropout, and max_pool3d after it as
    unet3d_forward applies it: the restatement on the conv's raw output gives the same (the oracle's eps is the double 1e-5, the
    kernels' the float32 one: 3e-13 of eps apart)"""
    from oracle.unet3d_oracle import _contract
    g = lambda s, tag, sc=1.0: torch.from_numpy(formula_tensor(s, tag, sc))            # noqa: E731
    sd = {"b.0.weight": g((8, 4, 3, 3, 3), 31, 0.2), "b.0.bias": g((8,), 32, 0.3)}
    x = g((2, 4, 4, 6, 8), 35)
    m = g((2, 8, 4, 6, 8), 36) > 0
    for masks in ({"b": m}, None):
        ref = _contract(x, sd, "b", masks, 0.5)
        raw = F.conv3d(x, sd["b.0.weight"], sd["b.0.bias"], padding=1)
        mu, _, rstd = R.instnorm_two_pass(_cl(raw))
        got = R.norm_act_drop_f64(_cl(raw), mu, rstd, R.ACT_LRELU, None if masks is None else _cl(m.double()))
        assert np.abs(got - _cl(ref)).max() < 1e-11
        assert np.abs(R.maxpool2_f64(got) - _cl(F.max_pool3d(ref, 2, 2))).max() < 1e-11


def test_conv1x1_f64_matches_einsum_and_flip():
    n, f, c, d, h, w = 4, 8, 3, 3, 5, 7
    x, wt, b = _x((n, d, h, w, f), 41), _x((c, f), 42, 1.0, 0.0), _x((c,), 43, 1.0, 0.0)
    dst, flip = [3, 0, 5, 2], [0, 1, 6, 7]
    out, mag = R.conv1x1_f64(x, wt, b, dst=dst, flip=flip, slots=6)
    ref = torch.einsum("nfdhw,cf->ncdhw", _nc(x).double(), torch.from_numpy(wt).double()) + torch.from_numpy(b).double().view(1, -1, 1, 1, 1)
    for i in range(n):
        dims = [1 + k for k in range(3) if flip[i] >> k & 1]
        r = torch.flip(ref[i], dims) if dims else ref[i]
        assert np.abs(out[dst[i]] - r.numpy()).max() < 1e-13
        assert np.all(mag[dst[i]] >= np.abs(out[dst[i]]) - 1e-13)
    assert np.isnan(out[1]).all() and np.isnan(out[4]).all()


def test_concat_buffer_helpers_round_trip_and_agree_with_the_kernel_tests():
    x = _x((2, 2, 3, 8, 4), 51)
    for xb in (1, 2, 4):
        for half in (0, 1):
            buf = R.to_xblk(x, half, xb, -77.0)
            assert np.array_equal(R.from_xblk(buf, half), x) and np.all(R.from_xblk(buf, 1 - half) == -77.0)
    # the torch helper the conv tests use builds the same buffer
    up, skip = _nc(x), _nc(x + 1)
    u = _cl(up).reshape(2, 2, 3, 2, 1, 4, 4)
    k = _cl(skip).reshape(2, 2, 3, 2, 1, 4, 4)
    cat = np.concatenate([u, k], 4)
    assert np.array_equal(R.from_xblk(cat, 0), x) and np.array_equal(R.from_xblk(cat, 1), x + 1)
    assert np.array_equal(R.to_xblk(x + 1, 1, 4, 0.0)[:, :, :, :, 1], cat[:, :, :, :, 1])


# ---------------------------------------------------------------------------------------------------------------------
def _forced_keep(shape, tag):
    """hash keep-mask with window (0,0,0) of every sample all dropped, window (0,0,1) none dropped"""
    n, d, h, w, c = shape
    keep = R.hash_keep_mask(tag, 3, n, d * h * w * c).reshape(shape).copy()
    keep[:, 0:2, 0:2, 0:2] = 0
    keep[:, 0:2, 0:2, 2:4] = 1
    return keep


@pytest.mark.parametrize("layout,c", [(1, 8), (2, 16)])
@pytest.mark.parametrize("scale2", [True, False])
def test_pool_finish_identity(layout, c, scale2):
    """the header's claim, on the restatement: finishing the window maxima and flags IS pooling the normalised tensor"""
    shape = (3, 4, 6, 8, c)
    x = _x(shape, 61 + c, 3.0, 0.5)
    keep = _forced_keep(shape, 17)
    # a negative maximum beside one dropped element: window (1, 1, 1) of sample 0 all far below the mean, one element dropped
    x[0, 2:4, 2:4, 2:4] = -9.0 + 0.01 * x[0, 2:4, 2:4, 2:4]
    keep[0, 2:4, 2:4, 2:4] = 1
    keep[0, 2, 2, 2] = 0
    mu, _, rstd = R.instnorm_two_pass(x)
    mu32, rs32 = mu.astype(np.float32), rstd.astype(np.float32)
    want = R.maxpool2_f32(R.norm_act_drop_f32(x, mu32, rs32, R.ACT_LRELU, keep, scale2))
    raw, flags = R.pool_windows(x, keep, layout)
    got = (R.pool_finish_f32 if layout == 1 else R.pool_finish_z_f32)(raw, flags, mu32, rs32, scale2)
    assert np.array_equal(got, want)
    assert np.all(got[:, 0, 0, 0] == 0) and np.all(want[0, 1, 1, 1] == 0)        # all dropped; the max(., 0) branch
    assert np.all(np.isneginf(raw[:, 0, 0, 0])) and (flags[:, 0, 0, 1] == 0).all() and (flags[:, 0, 0, 0] == 15).all()
    assert (R.norm_act_drop_f32(x, mu32, rs32)[0, 2:4, 2:4, 2:4] < 0).all()
    # no dropout at all: flags 0 everywhere
    raw, flags = R.pool_windows(x, np.ones(shape, np.uint8), layout)
    got = (R.pool_finish_f32 if layout == 1 else R.pool_finish_z_f32)(raw, flags, mu32, rs32, False)
    assert not flags.any() and np.array_equal(got, R.maxpool2_f32(R.norm_act_drop_f32(x, mu32, rs32)))


@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_split_round_trip(scale):
    n, nvox = 3, 257
    x = _x((n, nvox, 8), 71, 2.0, 0.3)
    mu, _, rstd = R.instnorm_two_pass(x)
    mu32, rs32 = mu.astype(np.float32), rstd.astype(np.float32)
    R.plant_split_values(x, mu32, rs32, scale)                  # +-0, underflowing lo, either side of hi's tie (ops3d_ref)
    x[0, 7, 7] = np.float32(mu32[0, 7] + np.float32(70000.0) / (rs32[0, 7] * np.float32(scale)))          # past fp16: hi = inf
    t = R.prenorm_split_t_f32(x, mu32, rs32, scale)
    halves = R.prenorm_split_f32(x, mu32, rs32, scale)
    assert halves.dtype == np.float16 and halves.shape == (n, nvox, 2, 2, 4)
    back = R.unsplit(halves).reshape(n, nvox, 8)
    fin = np.isfinite(halves.astype(np.float64)).all((-1, -2)).repeat(4).reshape(n, nvox, 8)
    # hi + lo / 2048 == t up to the rounding of lo: half an fp16 ulp of the scaled residual, |res| * 2048 <= 2^-11 |t| * 2048 = |t|,
    # i.e. 2^-11 relative of the residual = 2^-22 |t|; a lo in fp16's subnormal range keeps 2^-25 absolute, scaled by 2^-11
    tol = 2.0 ** -22 * np.abs(t.astype(np.float64)) + 2.0 ** -36
    assert (np.abs(back - t.astype(np.float64))[fin] <= tol[fin]).all()
    assert not fin[0, 7, 7] and fin.sum() == fin.size - 4             # 70000 is past fp16: hi = inf (the range_flag's business)
    # the hand-written unsplit of tests/test_gpu_kernels.py::test_prenorm_split_and_pool_finish_z_with_their_own_statistics
    hl = torch.from_numpy(halves.view(np.float32).copy()).contiguous().view(torch.float16).view(n, nvox, 2, 2, 4).float()
    theirs = (hl[..., 0, :] + hl[..., 1, :] / 2048.0).numpy().reshape(n, nvox, 8)
    assert np.array_equal(theirs[fin], back.astype(np.float32)[fin])


# ---------------------------------------------------------------------------------------------------------------------
COND_NVOX, COND_TILES = 4096, 37


def _cond_case(kind, value):
    if kind == "ratio":
        return R.conditioned((2, COND_NVOX, 4), 81, (value,))
    return np.full((2, COND_NVOX, 4), np.float32(value), dtype=np.float32)


@pytest.mark.parametrize("kind,value", [("ratio", r) for r in R.MU_OVER_SIGMA] + [("const", c) for c in R.CONSTANTS])
def test_conditioning_bounds_hold_for_ideal_partials(kind, value):
    """|d mu| <= u A and |d var| <= u (sigma^2 + mu^2) + 2 |mu| u A + (u A)^2 (tests/ops3d_ref.py), against the float64 two-pass
    statistics; partials = exact tile sums rounded once to float32"""
    x = _cond_case(kind, value)
    part, count = R.ideal_partials(x, COND_TILES)
    mu, var, _ = R.instnorm_two_pass(x)
    sums = R.exact_sums(part)
    mu_p = sums[..., 0] / count
    var_p = sums[..., 1] / count - mu_p * mu_p                        # unclamped: the bound is on the formula
    dmu, dvar = R.stat_bounds(part, count, mu, var)
    print(f"{kind} {value}: |dmu| {np.abs(mu_p - mu).max():.3e} <= {dmu.max():.3e}; |dvar| {np.abs(var_p - var).max():.3e} <= {dvar.max():.3e}")
    assert (np.abs(mu_p - mu) <= dmu).all()
    assert (np.abs(var_p - var) <= dvar).all()
    if kind == "ratio" and value > 0:
        assert np.allclose(np.abs(mu) / np.sqrt(var), value, rtol=0.05)
    # and propagated: the float32 restatement fed the correctly rounded statistics stays inside y_bound
    if kind == "const" or value <= 300:
        _, _, mu32, rs32 = R.instnorm_from_partials(part, count)
        y32 = R.norm_act_drop_f32(x, mu32, rs32, R.ACT_NONE)
        _, _, rstd = R.instnorm_two_pass(x)
        y64 = R.norm_act_drop_f64(x, mu, rstd, R.ACT_NONE)
        yb = R.y_bound(x, part, count)
        dev = np.abs(y32 - y64)
        print(f"   |dy| {dev.max():.3e} <= bound {yb.max():.3e}")
        assert (dev <= yb).all()


def test_y_bound_shows_where_the_formula_leaves_the_contract():
    """The derived bound guarantees the 1e-4 map contract at |mu| / sigma = 10 and no longer at 30 (1.5e-4; ideal partials measure
    1.5e-5 there); at 300 the FORMULA itself, evaluated exactly on ideal partials, is 8e-4 from the two-pass result: outside."""
    def case(ratio):
        x = R.conditioned((1, COND_NVOX, 4), 81, (ratio,))
        part, count = R.ideal_partials(x, COND_TILES)
        mu, rstd, _, _ = R.instnorm_from_partials(part, count)
        mu2, _, rstd2 = R.instnorm_two_pass(x)
        dev = np.abs(R.norm_act_drop_f64(x, mu, rstd, R.ACT_NONE) - R.norm_act_drop_f64(x, mu2, rstd2, R.ACT_NONE)).max()
        return R.y_bound(x, part, count).max(), dev
    assert case(10.0)[0] < 1e-4
    b30, d30 = case(30.0)
    assert b30 > 1e-4 and d30 < 1e-4
    b300, d300 = case(300.0)
    assert d300 > 1e-4 and d300 <= b300


# ---------------------------------------------------------------------------------------------------------------------
def _matrix_divisors():
    """every divisor the GPU matrix decodes with: (PW, C4, RH) of each case of ops3d_ref.norm_cases(), of the grid-stride and
    decode-limit launches of tests/test_gpu_stream3d.py"""
    div = set()
    for c in R.norm_cases():
        _, pool, _ = R.INSTANCES[c.inst]
        div.update(R.decode_divisors(pool, c.inst.startswith("wide"), c.C, *c.shape[1:])[0])
    L = R.DECODE_LIMIT
    div.update(R.decode_divisors(False, False, L["C"], L["D"], L["H"], L["W"])[0])
    for pool, wide, c, d, h, w in R.TRIP_SHAPES:
        div.update(R.decode_divisors(pool, wide, c, d, h, w)[0])
    return sorted(div)


def test_matrix_covers_every_option_with_every_instance():
    cases = R.norm_cases()
    assert len(cases) <= 150
    for inst, (entry, pool, _) in R.INSTANCES.items():
        mine = [c for c in cases if c.inst == inst]
        assert {c.act for c in mine} == {0, 1, 2} and {c.drop for c in mine} == {0, 1, 2}
        assert {(c.act, c.drop) for c in mine} == {(a, d) for a in range(3) for d in range(3)}
        want_c = R.C_WIDE if inst.startswith("wide") else R.C_SHUFFLE if pool else R.C_NOPOOL
        assert {c.C for c in mine} == set(want_c)
        lay = {c.layout for c in mine}
        assert {"dense", "x_pitch", "out_pitch"} <= lay and {f"out_xblk{xb}_{h}" for xb in (1, 2, 4) for h in (0, 1)} <= lay
        shapes = {c.shape[1:] for c in mine}
        assert {s[1:] for s in (R.POOL_SHAPES if pool else R.NOPOOL_SHAPES)} <= shapes
        assert all(c.shape[0] >= 3 for c in mine if c.drop == 1)
        if pool:
            assert "pool_pitch" in lay
            xin = [R.parse_layout(c.layout) for c in mine if c.layout.startswith("x_xblk")]
            assert {(d["x_xblk"], d["x_half"]) for d in xin} == {(xb, h) for xb in (1, 2, 4) for h in (0, 1)}
            assert {d["pool_only"] for d in xin} == {False, True}
        if inst == "fanout":
            assert {c.repeat for c in mine} == {2, 5}
    assert {c.C // 4 for c in cases if c.inst == "pool"} == {1, 2, 4, 8, 16, 32}


def test_magic_division_is_exact_below_the_launchers_limit_and_not_beyond():
    fails_past = 0
    divisors = _matrix_divisors()
    assert 1 in divisors and 1023 in divisors and 57 in divisors and 3 in divisors
    for d in divisors:
        top = ((1 << 32) - 1) // d                                   # the largest i with i * d < 2^32
        i = np.unique(np.concatenate([np.arange(0, min(top, 4096) + 1), np.arange(max(top - 70000, 0), top + 1),
                                      np.linspace(0, top, 5001).astype(np.int64)])).astype(np.uint64)
        assert i[-1] == top
        assert np.array_equal(R.magic_div(i, d), i // np.uint64(d)), d
        if d > 1:
            j = np.arange(top + 1, min(top + 1 + 4 * 70000, (1 << 32) - 1), dtype=np.uint64)
            fails_past += int((R.magic_div(j, d) != j // np.uint64(d)).any())
    assert fails_past > 0          # the property does end near the limit: the launcher's refusal carries weight
