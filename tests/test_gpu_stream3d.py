"""GPU: the 3D streaming kernels between the convolutions (norm_apply.hip, conv1x1.hip) through the C ABI, against the host
restatement tests/ops3d_ref.py (pinned on the CPU by tests/test_ops3d_ref_cpu.py).

Outputs are compared two ways: np.array_equal with the *_f32 restatement fed the device's own mean / rstd (the library is built
without contraction and none of these expressions could contract: the restatement defines the bits; +0 and -0 compare equal), and
float64 through ops3d_ref.y_bound computed from the statistics partials.  Tolerances are bit equality, one float32 ulp, a bound
computed by ops3d_ref from the inputs, or the project's 1e-4 contract; nothing else.

Instances launched and name-checked (vx_last_kernel_name):
    norm_act_drop_pool_kernel<false,false>, <true,false>, <true,true>         test_norm_matrix[plain- / pool- / wide-...]
    norm_act_drop_pool_kernel<..,true> (the three _stats forms)               test_norm_matrix[plain_stats- / pool_stats- / wide_stats-...]
    norm_act_drop_fanout_kernel                                               test_norm_matrix[fanout-...], test_grid_stride_trips[fanout]
    instnorm_finalize_kernel                                                  test_statistics
    pool_finish_kernel, pool_finish_z_kernel<false|true>                      test_pool_finish_is_pooling_the_normalised_tensor
    prenorm_split_kernel<false|true>                                          test_prenorm_split
    conv1x1_ncdhw_kernel<8|16|32>                                             test_conv1x1"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import ops3d_ref as R
from tests.formula import formula_tensor
from values_amd import _lib

pytestmark = pytest.mark.gpu

SENT = -77.0
OTHER = 12345.0            # the other half of a concat INPUT: read by mistake it cannot pass
E_SHAPE, E_ALIGN = -2, -5
EPS = 1e-5


def dev():
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _kernel():
    return _lib.load().vx_last_kernel_name().decode()


def _x(shape, tag, scale=3.0, off=1.5):
    return (formula_tensor(shape, tag, scale) + off).astype(np.float32)


def _stat_src(part_d, tiles, count, mo, ro):
    st = _lib.StatSrc()
    st.stats_partial = part_d.data_ptr(); st.tiles = tiles; st.eps = EPS; st.count = count
    st.mean_out = mo.data_ptr() if mo is not None else None
    st.rstd_out = ro.data_ptr() if ro is not None else None
    return st


def _ulp_ok(got32, ref64):
    return np.abs(got32.astype(np.float64) - ref64) <= R.ulp32(ref64)


# ---------------------------------------------------------------------------------------------------------------------
def launch_norm(x, *, entry="plain", repeat=1, mean=None, rstd=None, part=None, count=None, act=1, drop=0, keep=None, seed=0,
                layer=0, seed_dev=None, pool=False, lay=None, range_flag=False, expect_rc=0):
    """x [Ns][D][H][W][C] float32 numpy -> namespace(out [N][D][H][W][C] or None, pool, kernel, mean, rstd, flag): builds every
    buffer with sentinels around the real channels, launches, and checks that the sentinels survived"""
    lib = _lib.load()
    lay = dict(R.parse_layout("dense"), **(lay or {}))
    ns, d, h, w, c = x.shape
    n = ns * repeat
    keep_alive = []
    a = _lib.NormArgs()
    if lay["x_xblk"]:
        xd = _d(R.to_xblk(x, lay["x_half"], lay["x_xblk"], OTHER))
        a.x_xblk, a.x_half, a.x_pitch = lay["x_xblk"], lay["x_half"], 0
    else:
        xp = c + lay["x_pad"]
        xb = np.full((ns, d, h, w, xp), 7.0, dtype=np.float32)           # garbage pad channels must be ignored
        xb[..., :c] = x
        xd = _d(xb); a.x_pitch = xp
    a.x = xd.data_ptr()
    a.N, a.D, a.H, a.W, a.C = n, d, h, w, c
    a.act, a.drop_mode, a.drop_seed, a.drop_layer = act, drop, seed, layer
    if mean is not None:
        md, rd = _d(mean), _d(rstd); keep_alive += [md, rd]
        a.mean, a.rstd = md.data_ptr(), rd.data_ptr()
    if drop == _lib.VX_DROP_MASK:
        kd = _d(np.asarray(keep, dtype=np.uint8).reshape(n, d, h, w, c)); keep_alive.append(kd)
        a.drop_mask = kd.data_ptr()
    if seed_dev is not None:
        sd = torch.tensor([seed_dev], dtype=torch.int32, device=dev()); keep_alive.append(sd)
        a.seed_dev = sd.data_ptr()
    out = None
    if not lay["pool_only"]:
        if lay["out_xblk"]:
            xb_ = lay["out_xblk"]
            out = torch.full((n, d, h, w // xb_, 2, xb_, c), SENT, dtype=torch.float32, device=dev())
            a.out_xblk, a.out_half = xb_, lay["out_half"]
        else:
            op, oc = (2 * c, c) if lay["out_pitch2"] else (c, 0)
            out = torch.full((n, d, h, w, op), SENT, dtype=torch.float32, device=dev())
            a.out_pitch, a.out_coff = op, oc
        a.out = out.data_ptr()
    pl = None
    if pool:
        pp = c + lay["pool_pad"]
        pl = torch.full((n, d // 2, h // 2, w // 2, pp), SENT, dtype=torch.float32, device=dev())
        a.pool_out, a.pool_pitch = pl.data_ptr(), pp
    flag = None
    if range_flag:
        flag = torch.zeros(1, dtype=torch.int32, device=dev())
        a.range_flag = flag.data_ptr()
    mo = ro = None
    if entry == "stats":
        pd = _d(part); keep_alive.append(pd)
        mo = torch.full((ns, c), SENT, dtype=torch.float32, device=dev()); ro = torch.full_like(mo, SENT)
        st = _stat_src(pd, part.shape[1], count, mo, ro)
        rc = lib.vx_norm_act_drop_pool_stats(C.byref(a), C.byref(st), _lib.stream_ptr())
    elif entry == "bcast":
        rc = lib.vx_norm_act_drop_pool_bcast(C.byref(a), repeat, _lib.stream_ptr())
    else:
        assert repeat == 1
        rc = lib.vx_norm_act_drop_pool(C.byref(a), _lib.stream_ptr())
    assert rc == expect_rc, (rc, lib.vx_last_error_string())
    # the dry run, given the arguments just launched: the same code, and the name of the kernel that ran
    dry_name = C.create_string_buffer(96)
    dry = lib.vx_norm_act_drop_pool_route(C.byref(a), repeat, C.byref(st) if entry == "stats" else None, dry_name, len(dry_name), None)
    assert dry == rc, (dry, rc, lib.vx_last_error_string())
    if rc != 0:
        return None
    name = _kernel()
    assert dry_name.value.decode() == name
    torch.cuda.synchronize()
    res = SimpleNamespace()
    res.kernel = name
    res.out = res.pool = None
    if out is not None:
        o = out.cpu().numpy()
        if lay["out_xblk"]:
            res.out = R.from_xblk(o, lay["out_half"])
            assert (R.from_xblk(o, 1 - lay["out_half"]) == SENT).all(), "the other half of the concat buffer was written"
        else:
            res.out = o[..., a.out_coff:a.out_coff + c]
            assert (o[..., :a.out_coff] == SENT).all() and (o[..., a.out_coff + c:] == SENT).all(), "pitch gap written"
    if pl is not None:
        p = pl.cpu().numpy()
        res.pool = p[..., :c]
        assert (p[..., c:] == SENT).all(), "pool pitch gap written"
    res.mean = mo.cpu().numpy() if mo is not None else mean
    res.rstd = ro.cpu().numpy() if ro is not None else rstd
    res.flag = int(flag.cpu().numpy().view(np.uint32)[0]) if flag is not None else None
    return res


def device_hash_mask(seed, layer, n, per):
    m = torch.full((n, per), 9, dtype=torch.uint8, device=dev())
    _lib.check(_lib.load().vx_drop_hash_mask(seed, layer, n, per, _lib.ptr(m), _lib.stream_ptr()), "vx_drop_hash_mask")
    torch.cuda.synchronize()
    return m.cpu().numpy()


def norm_case_body(inst, c, shape, act, drop, layout, tiles, repeat):
    """one case of the matrix (also what tools/fuzz_misc.py draws): launch, name check, bits against the float32 restatement
    fed the device's statistics, float64 against ops3d_ref.y_bound, statistics against the correctly rounded ones"""
    entry, pool, kname = R.INSTANCES[inst]
    ns, d, h, w = shape
    n = ns * repeat
    tag = 1000 + 7 * c + 13 * d + h + 3 * w
    x = _x((ns, d, h, w, c), tag)
    count = d * h * w
    part, _ = R.ideal_partials(x, tiles)
    mu64, rs64, mu32, rs32 = R.instnorm_from_partials(part, count)
    seed, layer = 77 + c, 5
    keep = None
    if drop == _lib.VX_DROP_HASH:
        keep = R.hash_keep_mask(seed, layer, n, count * c).reshape(n, d, h, w, c)
        assert np.array_equal(device_hash_mask(seed, layer, n, count * c), keep.reshape(n, -1))
    elif drop == _lib.VX_DROP_MASK:
        keep = (formula_tensor((n, d, h, w, c), tag + 1) > 0).astype(np.uint8)
    kw = dict(entry=entry, repeat=repeat, act=act, drop=drop, keep=keep, seed=seed, layer=layer, pool=pool, lay=R.parse_layout(layout))
    if entry == "stats":
        r = launch_norm(x, part=part, count=count, **kw)
        assert _ulp_ok(r.mean, mu64).all() and _ulp_ok(r.rstd, rs64).all()
    else:
        r = launch_norm(x, mean=mu32, rstd=rs32, **kw)
    assert r.kernel == kname, r.kernel
    rep = lambda t: np.repeat(t, repeat, 0)                    # noqa: E731
    y32 = R.norm_act_drop_f32(rep(x), rep(r.mean), rep(r.rstd), act, keep)
    mu2, _, rstd2 = R.instnorm_two_pass(x)
    y64 = R.norm_act_drop_f64(rep(x), rep(mu2), rep(rstd2), act, keep)
    yn = R.norm_act_drop_f64(rep(x), rep(mu2), rep(rstd2), R.ACT_NONE)
    bound = R.out_bound(rep(R.y_bound(x, part, count)), yn, act, 2.0 if keep is not None else 1.0)
    if r.out is not None:
        assert np.array_equal(r.out, y32)
        assert (np.abs(r.out - y64) <= bound).all()
    else:
        assert R.parse_layout(layout)["pool_only"]
    if pool:
        assert np.array_equal(r.pool, R.maxpool2_f32(y32))
        assert (np.abs(r.pool - R.maxpool2_f64(y64)) <= R.maxpool2_f64(bound)).all()
    return r


@pytest.mark.parametrize("case", R.norm_cases(), ids=R.norm_case_id)
def test_norm_matrix(case):
    norm_case_body(*case)


# ---------------------------------------------------------------------------------------------------------------------
def _plain_args(c, shape, pool):
    n, d, h, w = shape
    x = _x((n, d, h, w, c), 31)
    part, cnt = R.ideal_partials(x, 1)
    _, _, mu32, rs32 = R.instnorm_from_partials(part, cnt)
    return x, mu32, rs32


@pytest.mark.parametrize("c", R.POOL_REFUSED_C)
def test_pooling_refuses_channel_counts_the_shuffle_cannot_pair(c):
    x, mu, rs = _plain_args(c, (2, 2, 2, 4), True)
    assert launch_norm(x, mean=mu, rstd=rs, pool=True, expect_rc=E_SHAPE) is None
    r = launch_norm(x, mean=mu, rstd=rs, pool=False)               # the same C without pooling runs
    assert r.kernel == "norm_act_drop_pool_kernel<false,false>" and np.array_equal(r.out, R.norm_act_drop_f32(x, mu, rs))


def test_concat_input_goes_with_pooling_and_no_broadcast():
    x, mu, rs = _plain_args(8, (2, 2, 2, 4), True)
    lay = dict(x_xblk=2, x_half=1)
    assert launch_norm(x, mean=mu, rstd=rs, pool=False, lay=lay, expect_rc=E_SHAPE) is None
    assert launch_norm(x, entry="bcast", repeat=2, mean=mu, rstd=rs, pool=True, lay=lay, expect_rc=E_SHAPE) is None
    x6, mu6, rs6 = _plain_args(8, (2, 2, 2, 6), True)
    assert launch_norm(x6, mean=mu6, rstd=rs6, pool=True, lay=dict(x_xblk=3, x_half=0), expect_rc=E_SHAPE) is None     # xb in {1, 2, 4}
    x516 = _x((1, 2, 2, 2, 516), 32)
    part, cnt = R.ideal_partials(x516, 2)
    assert launch_norm(x516, entry="stats", part=part, count=cnt, pool=True, expect_rc=E_SHAPE) is None      # C <= 512


def test_broadcast_with_pooling_reads_sample_n_over_repeat():
    """vx_norm_act_drop_pool_bcast with pool_out keeps the per-sample kernel: output sample n reads source n / x_repeat"""
    x, mu, rs = _plain_args(16, (2, 2, 4, 6), True)
    rep = 3
    keep = R.hash_keep_mask(9, 2, 2 * rep, x[0].size).reshape((2 * rep,) + x.shape[1:])
    r = launch_norm(x, entry="bcast", repeat=rep, mean=mu, rstd=rs, drop=_lib.VX_DROP_HASH, seed=9, layer=2, pool=True)
    assert r.kernel == "norm_act_drop_pool_kernel<true,false>"
    y = R.norm_act_drop_f32(np.repeat(x, rep, 0), np.repeat(mu, rep, 0), np.repeat(rs, rep, 0), R.ACT_LRELU, keep)
    assert np.array_equal(r.out, y) and np.array_equal(r.pool, R.maxpool2_f32(y))


def test_seed_comes_from_the_device_word():
    """seed_dev is ADDED to drop_seed: the keep-bits are those of the sum, not of drop_seed alone"""
    x, mu, rs = _plain_args(8, (3, 2, 2, 4), True)
    r = launch_norm(x, mean=mu, rstd=rs, drop=_lib.VX_DROP_HASH, seed=1000, seed_dev=234, layer=4, pool=True)
    keep = R.hash_keep_mask(1234, 4, 3, x[0].size).reshape(x.shape)
    wrong = R.hash_keep_mask(1000, 4, 3, x[0].size).reshape(x.shape)
    assert not np.array_equal(keep, wrong)
    y = R.norm_act_drop_f32(x, mu, rs, R.ACT_LRELU, keep)
    assert np.array_equal(r.out, y) and np.array_equal(r.pool, R.maxpool2_f32(y))


@pytest.mark.parametrize("inst", ["plain", "pool", "fanout"])
def test_range_word_without_normalisation(inst):
    """mean == rstd == NULL: y = Dropout(act(x)).  range_flag stays 0 for an in-range input; one element at 4.0e4 reports a value
    >= 32768: the per-sample kernels the largest |stored value| (the dropout's 2 included where the element is kept), the
    fan-out kernel twice the activation whatever the masks say, as its comment states"""
    entry, pool, kname = R.INSTANCES[inst]
    rep = 2 if inst == "fanout" else 1
    x = _x((2, 2, 2, 4, 8), 41)
    n = 2 * rep
    keep = (formula_tensor((n,) + x.shape[1:], 42) > 0).astype(np.uint8)
    kw = dict(entry=entry, repeat=rep, act=R.ACT_LRELU, drop=_lib.VX_DROP_MASK, keep=keep, pool=pool, range_flag=True)
    r = launch_norm(x, **kw)
    assert r.kernel == kname and r.flag == 0
    y = R.norm_act_drop_f32(np.repeat(x, rep, 0), None, None, R.ACT_LRELU, keep)
    assert np.array_equal(r.out, y)
    x[1, 1, 0, 2, 5] = 4.0e4
    keep[:, 1, 0, 2, 5] = 0                                   # dropped in every output sample: stored as 0
    r = launch_norm(x, **kw)
    y = R.norm_act_drop_f32(np.repeat(x, rep, 0), None, None, R.ACT_LRELU, keep)
    assert np.array_equal(r.out, y) and np.abs(y).max() < 32768
    if inst == "fanout":
        assert r.flag == int(np.float32(8.0e4).view(np.uint32))
    else:
        assert r.flag == 0                                    # nothing stored reaches the limit
    keep[:, 1, 0, 2, 5] = 1
    r = launch_norm(x, **kw)
    assert r.flag == int(np.float32(8.0e4).view(np.uint32))   # kept: 2 * 4.0e4 is what is stored
    assert np.uint32(r.flag).view(np.float32) >= 32768


# ---------------------------------------------------------------------------------------------------------------------
def _cheap_keep(shape):
    i = np.arange(int(np.prod(shape)), dtype=np.uint32)
    return (((i * np.uint32(2654435761)) >> np.uint32(13)) & np.uint32(1)).astype(np.uint8).reshape(shape)


@pytest.mark.parametrize("which", ["plain", "fanout", "plain_stats", "pool_stats", "wide_stats", "pool_idle_wave"])
def test_grid_stride_trips(which):
    """launches whose grid-stride loops run more than one trip (ops3d_ref.TRIP_SHAPES): the 16384 / N and 32768 / ns caps, the
    (bx + 3) / 4 grid of the _stats forms, and a pooling launch whose last wave is partly idle beside the shuffle"""
    i = ["plain", "fanout", "plain_stats", "pool_stats", "wide_stats", "pool_idle_wave"].index(which)
    pool, wide, c, d, h, w = R.TRIP_SHAPES[i]
    ns = {"plain": 20000, "fanout": 33000}.get(which, 3)
    rep = 2 if which == "fanout" else 1
    inst = {"pool_idle_wave": "pool"}.get(which, which)
    entry, pool_, kname = R.INSTANCES[inst]
    assert pool_ == pool
    (pw, c4, rh), per = R.decode_divisors(pool, wide, c, d, h, w)
    if which in ("plain", "fanout"):
        assert per > 256 and (16384 if which == "plain" else 32768) // ns == 0          # one block of 256 per sample
        assert which == "plain" or ns * rep > 65535                                     # the fan-out grid's y is ns, not N
    elif which != "pool_idle_wave":
        assert per > 1024
    else:
        assert per % 64
    x = _x((ns, d, h, w, c), 51, 2.0, 0.25)
    keep = _cheap_keep((ns * rep, d, h, w, c))
    if entry == "stats":
        part, cnt = R.ideal_partials(x, 3)
        r = launch_norm(x, entry=entry, part=part, count=cnt, drop=_lib.VX_DROP_MASK, keep=keep, pool=pool)
    else:
        # per-sample statistics of 20000 samples: plain float64 numpy (exact enough: the comparison is on the f32 restatement)
        mu, _, rstd = R.instnorm_two_pass(x)
        r = launch_norm(x, entry=entry, repeat=rep, mean=mu.astype(np.float32), rstd=rstd.astype(np.float32), drop=_lib.VX_DROP_MASK,
                        keep=keep, pool=pool)
    assert r.kernel == kname
    y = R.norm_act_drop_f32(np.repeat(x, rep, 0) if rep > 1 else x, np.repeat(r.mean, rep, 0), np.repeat(r.rstd, rep, 0), R.ACT_LRELU, keep)
    assert np.array_equal(r.out, y)
    if pool:
        assert np.array_equal(r.pool, R.maxpool2_f32(y))


def test_index_decode_at_its_limit():
    """per * max(PW, RH) just under 2^32 with the odd divisor PW = 1023 (W = 341, C = 12, D x H = 72 x 57: 67 MB each way); the
    next larger D is refused"""
    L = R.DECODE_LIMIT
    (pw, c4, rh), per = R.decode_divisors(False, False, L["C"], L["D"], L["H"], L["W"])
    assert pw == 1023 and per * max(pw, rh) < 1 << 32 <= (per + rh * pw) * max(pw, rh)
    x = _x((1, L["D"], L["H"], L["W"], L["C"]), 61)
    mu, _, rstd = R.instnorm_two_pass(x)
    mu32, rs32 = mu.astype(np.float32), rstd.astype(np.float32)
    r = launch_norm(x, mean=mu32, rstd=rs32, act=R.ACT_RELU)
    assert r.kernel == "norm_act_drop_pool_kernel<false,false>"
    assert np.array_equal(r.out, R.norm_act_drop_f32(x, mu32, rs32, R.ACT_RELU))
    # the refusal needs no data: the launcher checks the shape before it touches a pointer's target
    lib = _lib.load()
    a = _lib.NormArgs()
    buf = torch.empty(16, dtype=torch.float32, device=dev())
    a.x = a.out = buf.data_ptr(); a.mean = a.rstd = buf.data_ptr()
    a.x_pitch = a.out_pitch = L["C"]
    a.N, a.D, a.H, a.W, a.C = 1, L["D"] + 1, L["H"], L["W"], L["C"]
    assert lib.vx_norm_act_drop_pool(C.byref(a), _lib.stream_ptr()) == E_SHAPE
    # N past the grid's y range: 65536 samples, and 65536 SOURCE samples of a fan-out (its grid's y is N / x_repeat)
    a.N, a.D, a.H, a.W = 65536, 1, 1, 1
    assert lib.vx_norm_act_drop_pool(C.byref(a), _lib.stream_ptr()) == E_SHAPE
    a.N = 2 * 65536
    assert lib.vx_norm_act_drop_pool_bcast(C.byref(a), 2, _lib.stream_ptr()) == E_SHAPE


# ---------------------------------------------------------------------------------------------------------------------
# statistics: vx_instnorm_finalize, and vx_block_instnorm through the three _stats entry points
STAT_CASES = [(4, 1, False, (1, 1, 5)), (8, 37, True, (2, 4, 6)), (8, 300, True, (4, 8, 10)), (16, 9, True, (2, 2, 4)),
              (128, 65, True, (2, 6, 6)), (256, 3, True, (2, 2, 2)), (260, 5, False, (1, 1, 6)), (384, 2, True, (2, 2, 2)),
              (512, 7, True, (2, 2, 2))]
STAT_CONSTANTS = (0.37, 1.0, -3.3e-3)            # one constant channel per sample (the last one)


def _stat_inputs(c, tiles, dhw, builder):
    n = 3
    nvox = int(np.prod(dhw))
    if builder == "ideal":
        x = R.conditioned((n, nvox, c), 700 + c + tiles, (0.0, 3.0, 30.0, 300.0))
        for s in range(n):
            x[s, :, -1] = np.float32(STAT_CONSTANTS[s])
        part, _ = R.ideal_partials(x, tiles)
    else:                                         # the made-up tiling of the sibling tests: arbitrary partials whose sums are the tensor's
        x = _x((n, nvox, c), 800 + c + tiles, 2.0, 0.0)
        part = formula_tensor((n, tiles, c, 2), 801 + c, scale=3.0).astype(np.float32)
        tot = np.stack([x.astype(np.float64).sum(1), (x.astype(np.float64) ** 2).sum(1)], -1)
        part[:, 0] += (tot - part.astype(np.float64).sum(1)).astype(np.float32)
    return x.reshape((n,) + tuple(dhw) + (c,)), part, nvox


def _finalize(part, count):
    n, tiles, c, _ = part.shape
    pd = _d(part)
    mean = torch.full((n, c), SENT, dtype=torch.float32, device=dev()); rstd = torch.full_like(mean, SENT)
    _lib.check(_lib.load().vx_instnorm_finalize(_lib.ptr(pd), n, tiles, c, count, EPS, _lib.ptr(mean), _lib.ptr(rstd), _lib.stream_ptr()), "finalize")
    name = _kernel()
    torch.cuda.synchronize()
    return mean.cpu().numpy(), rstd.cpu().numpy(), name


def launch_split(x, scale, mean=None, rstd=None, part=None, count=None):
    """x [N][nvox][8] -> (fp16 halves [N][nvox][2][2][4], mean_out, rstd_out, kernel)"""
    lib = _lib.load()
    n, nvox, _ = x.shape
    xd = _d(x)
    mo = ro = None
    if part is None:
        md, rd = _d(mean), _d(rstd)
        _lib.check(lib.vx_prenorm_split(_lib.ptr(xd), _lib.ptr(md), _lib.ptr(rd), n, nvox, scale, _lib.stream_ptr()), "split")
    else:
        pd = _d(part)
        mo = torch.full((n, 8), SENT, dtype=torch.float32, device=dev()); ro = torch.full_like(mo, SENT)
        st = _stat_src(pd, part.shape[1], count, mo, ro)
        _lib.check(lib.vx_prenorm_split_stats(_lib.ptr(xd), C.byref(st), n, nvox, scale, _lib.stream_ptr()), "split_stats")
    name = _kernel()
    torch.cuda.synchronize()
    halves = xd.cpu().numpy().view(np.float16).reshape(n, nvox, 2, 2, 4)
    return halves, (mo.cpu().numpy() if mo is not None else mean), (ro.cpu().numpy() if ro is not None else rstd), name


def launch_finish_z(raw, flags, scale2, pitch=16, mean=None, rstd=None, part=None, count=None, expect_rc=0):
    """raw [N][2 Dp][pv][16], flags [N][2 Dp][pv][4] -> (out [N][Dp][pv][16], mean, rstd, kernel)"""
    lib = _lib.load()
    n, d2, pv, _ = raw.shape
    rd, fd = _d(raw), _d(flags.astype(np.uint32).view(np.int32))
    buf = torch.full((n * (d2 // 2) * pv * pitch + 4,), SENT, dtype=torch.float32, device=dev())
    out = buf
    mo = ro = None
    if part is None:
        md, sd = _d(mean), _d(rstd)
        rc = lib.vx_pool_finish_z(_lib.ptr(rd), _lib.ptr(fd), _lib.ptr(md), _lib.ptr(sd), _lib.ptr(out), pitch, n, d2 // 2, pv, int(scale2), _lib.stream_ptr())
    else:
        pd = _d(part)
        mo = torch.full((n, 16), SENT, dtype=torch.float32, device=dev()); ro = torch.full_like(mo, SENT)
        st = _stat_src(pd, part.shape[1], count, mo, ro)
        rc = lib.vx_pool_finish_z_stats(_lib.ptr(rd), _lib.ptr(fd), C.byref(st), _lib.ptr(out), pitch, n, d2 // 2, pv, int(scale2), _lib.stream_ptr())
    assert rc == expect_rc, (rc, lib.vx_last_error_string())
    if rc:
        return None
    name = _kernel()
    torch.cuda.synchronize()
    o = buf.cpu().numpy()
    assert (o[-4:] == SENT).all()
    o = o[:-4].reshape(n, d2 // 2, pv, pitch)
    assert (o[..., 16:] == SENT).all(), "pitch gap written"
    return o[..., :16], (mo.cpu().numpy() if mo is not None else mean), (ro.cpu().numpy() if ro is not None else rstd), name


@pytest.mark.parametrize("builder", ["ideal", "madeup"])
@pytest.mark.parametrize("c,tiles,pool,dhw", STAT_CASES, ids=[f"C{c}-t{t}" for c, t, _, _ in STAT_CASES])
def test_statistics(c, tiles, pool, dhw, builder):
    """mean / rstd of vx_instnorm_finalize and of every _stats entry point that takes this C, against instnorm_from_partials
    (exact sums, the header's formula in float64): within one float32 ulp of the correctly rounded value, written for every
    sample (N = 3: the blockIdx.x == 0 workgroups of each); and the normalised output within y_bound.  The ideal builder's
    channels have |mu| / sigma in {0, 3, 30, 300} and one constant channel per sample.

    |mu| / sigma = 300 is asserted against y_bound ONLY: it lies outside the project's 1e-4 map contract, because
    var = q / n - mu^2 cancels ~1e5 of the float32 partials' 2^-24 (ops3d_ref's docstring; ideal partials measure 8e-4)."""
    x, part, count = _stat_inputs(c, tiles, dhw, builder)
    mu64, rs64, mu32, rs32 = R.instnorm_from_partials(part, count)
    got = {"finalize": _finalize(part, count)}
    assert got["finalize"][2] == "instnorm_finalize_kernel"
    r = launch_norm(x, entry="stats", part=part, count=count, act=R.ACT_NONE, pool=pool)
    assert r.kernel == R.INSTANCES[("wide" if c > 128 else "pool") + "_stats" if pool else "plain_stats"][2]
    got["norm_stats"] = (r.mean, r.rstd)
    if c == 8:
        hv, m, s, name = launch_split(x.reshape(3, -1, 8), 1.0, part=part, count=count)
        assert name == "prenorm_split_kernel<true>" and np.array_equal(hv, R.prenorm_split_f32(x.reshape(3, -1, 8), m, s, 1.0))
        got["split_stats"] = (m, s)
    if c == 16:
        raw, flags = R.pool_windows(x, np.ones(x.shape, np.uint8), 2)
        rz = raw.reshape(3, raw.shape[1], -1, 16); fz = flags.reshape(3, raw.shape[1], -1, 4)
        o, m, s, name = launch_finish_z(rz, fz, False, part=part, count=count)
        assert name == "pool_finish_z_kernel<true>" and np.array_equal(o, R.pool_finish_z_f32(rz, fz, m, s, False))
        got["finish_z_stats"] = (m, s)
    for who, g in got.items():
        assert _ulp_ok(g[0], mu64).all(), who
        assert _ulp_ok(g[1], rs64).all(), who
    if builder == "ideal":
        mu2, _, rstd2 = R.instnorm_two_pass(x)
        y64 = R.norm_act_drop_f64(x, mu2, rstd2, R.ACT_NONE)
        assert np.array_equal(r.out, R.norm_act_drop_f32(x, r.mean, r.rstd, R.ACT_NONE))
        dev_, yb = np.abs(r.out - y64), R.y_bound(x, part, count)
        print(f"C={c} tiles={tiles}: max |dy| {dev_.max():.3e}, largest share of its bound {np.max(dev_ / yb):.3f}")
        assert (dev_ <= yb).all()
        assert np.abs(r.out[..., -1]).max() < 1e-4                 # the constant channel: InstanceNorm gives 0


def test_statistics_of_a_large_constant():
    """A constant channel at 1000: var = q / n - mu^2 is the difference of two float64 values near 1e6, whose own rounding
    (2^-53 each, ~2e-10 absolute) is 2e-5 of eps -- rstd near 1 / sqrt(eps) is defined by the formula to that and no better,
    for the float64 reference as for the device.  So: rstd within one float32 ulp plus that float64 share, the mean to one ulp,
    and the normalised output (0 in exact arithmetic) within the 1e-4 contract."""
    c, tiles, n, nvox = 8, 37, 3, 4096
    x = np.full((n, nvox, c), np.float32(1000.0), dtype=np.float32)
    x[..., :4] = _x((n, nvox, 4), 91)
    part, count = R.ideal_partials(x, tiles)
    mu64, rs64, _, _ = R.instnorm_from_partials(part, count)
    sums = R.exact_sums(part)
    dvar64 = 4.0 * 2.0 ** -53 * (sums[..., 1] / count + mu64 * mu64)
    var_eps = 1.0 / (rs64 * rs64)
    tol = R.ulp32(rs64) + rs64 * dvar64 / (2.0 * np.maximum(var_eps - dvar64, 0.5 * float(np.float32(EPS))))
    m, s, _ = _finalize(part, count)
    r = launch_norm(x.reshape(n, 16, 16, 16, c), entry="stats", part=part, count=count, act=R.ACT_NONE, pool=True)
    for mm, ss in ((m, s), (r.mean, r.rstd)):
        assert _ulp_ok(mm, mu64).all()
        assert (np.abs(ss.astype(np.float64) - rs64) <= tol).all()
    assert np.abs(r.out[..., 4:]).max() < 1e-4


def test_negative_computed_variance_clamps():
    """ops2d_ref.clamp_partials: q / n < mu^2 by the partial's own rounding -- rstd == 1 / sqrt(eps) to one ulp, everywhere"""
    from tests.ops2d_ref import clamp_partials
    cp, count = clamp_partials()                        # [4 tiles][2 channels][2]
    part = np.tile(cp[None, :, [0, 1, 1, 0]], (3, 1, 1, 1)).astype(np.float32)       # C = 4
    want = 1.0 / np.sqrt(float(np.float32(EPS)))
    m, s, _ = _finalize(part, count)
    x = np.zeros((3, 1, 1, count, 4), dtype=np.float32)
    r = launch_norm(x, entry="stats", part=part, count=count, act=R.ACT_NONE)
    for ss in (s, r.rstd):
        assert _ulp_ok(ss, np.full(ss.shape, want)).all()
    _, rs64, _, _ = R.instnorm_from_partials(part, count)
    assert (rs64 == want).all()


# ---------------------------------------------------------------------------------------------------------------------
def _forced_case(n, d, h, w, c, tag):
    """raw tensor and hash keep-mask with, per sample, an all-dropped window, a none-dropped window, and a window whose values are
    all far below the mean with one element dropped (a negative kept maximum beside a dropped element)"""
    x = _x((n, d, h, w, c), tag, 3.0, 0.5)
    keep = R.hash_keep_mask(tag, 3, n, d * h * w * c).reshape(x.shape).copy()
    keep[:, 0:2, 0:2, 0:2] = 0
    keep[:, 0:2, 0:2, 2:4] = 1
    x[:, 0:2, 2:4, 0:2] = -9.0 + 0.01 * x[:, 0:2, 2:4, 0:2]
    keep[:, 0:2, 2:4, 0:2] = 1
    keep[:, 0, 2, 0] = 0
    return x, keep


@pytest.mark.parametrize("pitch_pad", [0, 4])
@pytest.mark.parametrize("scale2", [1, 0])
@pytest.mark.parametrize("layout,dhw", [(1, (2, 4, 6)), (1, (20, 36, 94)), (2, (2, 4, 6)), (2, (20, 36, 94))])
def test_pool_finish_is_pooling_the_normalised_tensor(layout, dhw, scale2, pitch_pad):
    """The header's claim as stated: the finish pass over the window maxima / flags (pool_windows) is BIT-identical to
    vx_norm_act_drop_pool's pool_out on the same raw tensor with that mask, and both to pool_finish_f32.  The large shape
    loops the 64-block cap (> 16384 pieces per sample) and the 16-block cap of the _stats form, with plane_voxels = 18 * 47.
    drop_scale2 == 0 (s = 1) has no pooling pass to stand beside -- vx_norm_act_drop_pool's dropout always scales by 2 -- so the
    finish pass on the masked flags is compared with pool_finish_f32 alone, and three ways without dropout (flags 0)."""
    lib = _lib.load()
    c = 8 * layout
    n = 3
    d, h, w = dhw
    x, keep = _forced_case(n, d, h, w, c, 100 + layout)
    part, count = R.ideal_partials(x, 5)
    _, _, mu32, rs32 = R.instnorm_from_partials(part, count)
    raw, flags = R.pool_windows(x, keep, layout)
    pieces = (d // 2) * (h // 2) * (w // 2) * c // 4
    if d > 2:
        assert pieces > 16384 and ((h // 2) * (w // 2)) & ((h // 2) * (w // 2) - 1)
    pitch = c + pitch_pad
    if layout == 1:
        vox = (d // 2) * (h // 2) * (w // 2)
        rd, fd, md, sd = _d(raw), _d(flags.view(np.int32)), _d(mu32), _d(rs32)
        out = torch.full((n, vox, pitch), SENT, dtype=torch.float32, device=dev())
        _lib.check(lib.vx_pool_finish(_lib.ptr(rd), _lib.ptr(fd), _lib.ptr(md), _lib.ptr(sd), _lib.ptr(out), pitch, n, vox, scale2, _lib.stream_ptr()), "finish")
        assert _kernel() == "pool_finish_kernel"
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[..., c:] == SENT).all()
        fin = o[..., :c].reshape(raw.shape)
        want = R.pool_finish_f32(raw, flags, mu32, rs32, bool(scale2))
        mean_used, rstd_used = mu32, rs32
    else:
        rz, fz = raw.reshape(n, d, -1, 16), flags.reshape(n, d, -1, 4)
        o, _, _, name = launch_finish_z(rz, fz, scale2, pitch, mean=mu32, rstd=rs32)
        assert name == "pool_finish_z_kernel<false>"
        o2, m2, s2, name = launch_finish_z(rz, fz, scale2, pitch, part=part, count=count)
        assert name == "pool_finish_z_kernel<true>"
        assert np.array_equal(o2, R.pool_finish_z_f32(rz, fz, m2, s2, bool(scale2)))
        assert _ulp_ok(m2, R.instnorm_from_partials(part, count)[0]).all()
        fin = o.reshape(n, d // 2, h // 2, w // 2, c)
        want = R.pool_finish_z_f32(raw, flags, mu32, rs32, bool(scale2))
        mean_used, rstd_used = mu32, rs32
    assert np.array_equal(fin, want)
    assert (fin[:, 0, 0, 0] == 0).all() and (fin[:, 0, 1, 0] == 0).all()                # all dropped; negative maximum beside a drop
    if scale2:
        r = launch_norm(x, mean=mean_used, rstd=rstd_used, drop=_lib.VX_DROP_MASK, keep=keep, pool=True)
        assert np.array_equal(fin, r.pool)
    elif d == 2:
        r = launch_norm(x, mean=mean_used, rstd=rstd_used, drop=_lib.VX_DROP_NONE, pool=True)
        raw0, flags0 = R.pool_windows(x, np.ones_like(keep), layout)
        assert not flags0.any()
        if layout == 1:
            assert np.array_equal(r.pool, R.pool_finish_f32(raw0, flags0, mu32, rs32, False))
        else:
            o0, _, _, _ = launch_finish_z(raw0.reshape(n, d, -1, 16), flags0.reshape(n, d, -1, 4), 0, 16, mean=mu32, rstd=rs32)
            assert np.array_equal(o0.reshape(r.pool.shape), r.pool)


def test_pool_finish_refusals():
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev())
    p, s = _lib.ptr(buf), _lib.stream_ptr()
    off = C.c_void_p(buf.data_ptr() + 4)
    assert lib.vx_pool_finish(p, p, p, p, p, 4, 1, 8, 1, s) == E_ALIGN               # out_pitch < 8
    assert lib.vx_pool_finish(p, p, p, p, off, 8, 1, 8, 1, s) == E_ALIGN             # misaligned out
    assert lib.vx_pool_finish_z(p, p, p, p, p, 12, 1, 1, 8, 1, s) == E_ALIGN         # out_pitch < 16
    assert lib.vx_pool_finish_z(p, p, p, p, off, 16, 1, 1, 8, 1, s) == E_ALIGN
    st = _stat_src(buf, 1, 8, None, None)
    assert lib.vx_pool_finish_z_stats(p, p, C.byref(st), p, 12, 1, 1, 8, 1, s) == E_ALIGN
    assert lib.vx_pool_finish_z_stats(p, p, C.byref(st), off, 16, 1, 1, 8, 1, s) == E_ALIGN
    # mean given together with a statistics source (the pass that has both: vx_norm_act_drop_pool_stats)
    a = _lib.NormArgs()
    a.x = a.out = a.mean = a.rstd = buf.data_ptr()
    a.x_pitch = a.out_pitch = 8
    a.N, a.D, a.H, a.W, a.C = 1, 1, 1, 1, 8
    assert lib.vx_norm_act_drop_pool_stats(C.byref(a), C.byref(st), s) == E_SHAPE


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("stats,nvox", [(False, 70001), (True, 17001)])
def test_prenorm_split(stats, nvox, scale):
    """the fp16 bits of vx_prenorm_split(_stats) equal prenorm_split_f32: elements whose lo underflows, elements either side of
    hi's tie, +-0 planted; N = 3; nvox past 512 * 256 / 2 (plain: the 512-block cap loops) and 128 * 256 / 2 (_stats); a second
    call on a fresh copy gives the same bytes (in place: no thread reads what another wrote)"""
    n = 3
    assert 2 * nvox > (128 if stats else 512) * 256
    x = _x((n, nvox, 8), 111, 2.0, 0.3)
    part, count = R.ideal_partials(x, 37)
    _, _, mu32, rs32 = R.instnorm_from_partials(part, count)
    if not stats:
        wanted = R.plant_split_values(x, mu32, rs32, scale)
        hv, m, s, name = launch_split(x, scale, mean=mu32, rstd=rs32)
        assert name == "prenorm_split_kernel<false>"
        t = R.prenorm_split_t_f32(x, mu32, rs32, scale)
        assert abs(float(t[0, 1, 1]) - wanted[1]) < 1e-7 and abs(float(t[0, 3, 3]) - wanted[3]) < 2e-6   # the plants landed
        hv2, _, _, _ = launch_split(x.copy(), scale, mean=mu32, rstd=rs32)
    else:
        hv, m, s, name = launch_split(x, scale, part=part, count=count)
        assert name == "prenorm_split_kernel<true>"
        assert _ulp_ok(m, R.instnorm_from_partials(part, count)[0]).all() and _ulp_ok(s, R.instnorm_from_partials(part, count)[1]).all()
        hv2, _, _, _ = launch_split(x.copy(), scale, part=part, count=count)
    want = R.prenorm_split_f32(x, m, s, scale)
    assert np.array_equal(hv.view(np.uint16), want.view(np.uint16))            # bits: -0 and +0 differ here
    assert np.array_equal(hv.view(np.uint16), hv2.view(np.uint16))


def test_prenorm_split_refusals():
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float32, device=dev())
    p, s = _lib.ptr(buf), _lib.stream_ptr()
    off = C.c_void_p(buf.data_ptr() + 4)
    assert lib.vx_prenorm_split(off, p, p, 1, 4, 1.0, s) == E_ALIGN
    assert lib.vx_prenorm_split(p, p, p, 65536, 4, 1.0, s) == E_SHAPE
    st = _stat_src(buf, 1, 4, None, None)
    assert lib.vx_prenorm_split_stats(off, C.byref(st), 1, 4, 1.0, s) == E_ALIGN
    assert lib.vx_prenorm_split_stats(p, C.byref(st), 65536, 4, 1.0, s) == E_SHAPE


# ---------------------------------------------------------------------------------------------------------------------
C1_SHAPE = (4, 3, 5, 7)
C1_FLIPS = (0, 1, 2, 3, 4, 5, 6, 7)


@pytest.mark.parametrize("mode", ["dst_flip", "no_dst", "no_flip"])
@pytest.mark.parametrize("c", [1, 2, 3, 19])
@pytest.mark.parametrize("f", [8, 16, 32])
def test_conv1x1(f, c, mode):
    """vx_conv1x1_ncdhw against conv1x1_f64 within 2 F 2^-24 (sum |w x| + |b|) per element -- the fma chain's worst case (F
    roundings of partial sums bounded by the sum of magnitudes) with a factor two to spare; in_pitch cycles through F, F + 4,
    2 F; all eight flip codes over two launches; dst a permutation into more slots than samples"""
    lib = _lib.load()
    n, d, h, w = C1_SHAPE
    pitch = (f, f + 4, 2 * f)[(c + f // 8 + ["dst_flip", "no_dst", "no_flip"].index(mode)) % 3]
    x = _x((n, d, h, w, f), 121 + f + c, 2.0, 0.1)
    wt, b = _x((c, f), 122 + f, 1.0, 0.0), _x((c,), 123 + c, 1.0, 0.0)
    xb = np.full((n, d, h, w, pitch), 7.0, dtype=np.float32)
    xb[..., :f] = x
    xd, wd, bd = _d(xb), _d(wt), _d(b)
    for flips in ((C1_FLIPS[:4], C1_FLIPS[4:]) if mode != "no_flip" else (None,)):
        dst = [5, 0, 3, 2] if mode != "no_dst" else None
        slots = 6 if dst else n
        out = torch.full((slots, c, d, h, w), SENT, dtype=torch.float32, device=dev())
        dd = torch.tensor(dst, dtype=torch.int32, device=dev()) if dst else None
        fd = torch.tensor(list(flips), dtype=torch.int32, device=dev()) if flips else None
        _lib.check(lib.vx_conv1x1_ncdhw(_lib.ptr(xd), pitch, _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(out), n, d, h, w, f, c,
                                        _lib.ptr(dd), _lib.ptr(fd), _lib.stream_ptr()), "1x1")
        assert _kernel() == f"conv1x1_ncdhw_kernel<{f}>"
        torch.cuda.synchronize()
        ref, mag = R.conv1x1_f64(x, wt, b, dst=dst, flip=flips, slots=slots)
        got = out.cpu().numpy().astype(np.float64)
        written = ~np.isnan(ref)
        assert (got[~written] == SENT).all() and written.reshape(slots, -1).all(1).sum() == n
        assert (np.abs(got - ref)[written] <= (2.0 * f * R.U24 * mag)[written]).all()


def test_conv1x1_refusals():
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev())
    p, s = _lib.ptr(buf), _lib.stream_ptr()
    off = C.c_void_p(buf.data_ptr() + 4)
    assert lib.vx_conv1x1_ncdhw(p, 12, p, p, p, 1, 1, 1, 2, 12, 2, None, None, s) == E_SHAPE        # F = 12
    assert lib.vx_conv1x1_ncdhw(p, 4, p, p, p, 1, 1, 1, 2, 8, 2, None, None, s) == E_ALIGN          # in_pitch < F
    assert lib.vx_conv1x1_ncdhw(off, 8, p, p, p, 1, 1, 1, 2, 8, 2, None, None, s) == E_ALIGN        # misaligned in


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,shape", [(8, (1, 3, 3, 7)), (16, (1, 3, 5, 9))])
@pytest.mark.parametrize("what", ["constant", "offset"])
def test_chain_with_the_real_producer(cin, shape, what):
    """vx_conv3d_k3 (stats_partial) -> vx_instnorm_finalize -> vx_norm_act_drop_pool on the producer's own partials.

    constant: an all-zero input, biases in +-1 -- every output channel is the constant bias, the case an all-zero sliding-window
    patch produces.  The normalised output stays inside the 1e-4 contract against the float64 InstanceNorm of the conv's own
    float32 output (0), and rstd == 1 / sqrt(eps) to an ulp wherever the computed variance clamps.
    offset: a bias of 30 sigma in every second channel (|mu| / sigma ~ 30): within y_bound with u -> m u, m = voxels per tile
    (the worst case of a float32 running sum over a tile).  The measured deviation is recorded in DESIGN.md."""
    from tests.test_gpu_kernels import run_conv
    lib = _lib.load()
    n, d, h, w = shape
    cout = cin
    wt = torch.from_numpy(formula_tensor((cout, cin, 3, 3, 3), 132, scale=(1.0 / (27 * cin)) ** 0.5))
    if what == "constant":
        x = torch.zeros((n, cin, d, h, w), dtype=torch.float64)
        b = torch.from_numpy(formula_tensor((cout,), 133, scale=1.0))
    else:
        x = torch.from_numpy(formula_tensor((n, cin, d, h, w), 131))
        b = torch.from_numpy(formula_tensor((cout,), 133, scale=0.2))
        b[::2] += 30.0 * 0.24                                   # the conv's output has sigma ~ 0.24 on these inputs
    raw, st, _ = run_conv(x, wt, b, stats=True)
    raw = raw.permute(0, 2, 3, 4, 1).contiguous().numpy()       # the conv's own float32 output, channels-last
    part = st.numpy()
    count = d * h * w
    tiles = part.shape[1]
    assert tiles == lib.vx_conv3d_k3_tiles_for(d, h, w, cout)
    m = -(-count // tiles)
    mean, rstd, _ = _finalize(part, count)
    r = launch_norm(raw, mean=mean, rstd=rstd, act=R.ACT_NONE)
    assert np.array_equal(r.out, R.norm_act_drop_f32(raw, mean, rstd, R.ACT_NONE))
    mu2, var2, rstd2 = R.instnorm_two_pass(raw)
    y64 = R.norm_act_drop_f64(raw, mu2, rstd2, R.ACT_NONE)
    dev_ = np.abs(r.out - y64)
    if what == "constant":
        assert (raw == raw[:, :1, :1, :1]).all() and (y64 == 0).all()
        sums = R.exact_sums(part)
        var_p = sums[..., 1] / count - (sums[..., 0] / count) ** 2
        print(f"chain constant {cin}: tiles {tiles}, max |y| {dev_.max():.3e}, computed var in [{var_p.min():.3e}, {var_p.max():.3e}]")
        clamps = var_p <= 0
        want = 1.0 / np.sqrt(float(np.float32(EPS)))
        assert _ulp_ok(rstd[clamps], np.full(int(clamps.sum()), want)).all()
        assert dev_.max() < 1e-4
    else:
        ratio = np.abs(mu2) / np.sqrt(var2)
        assert (ratio[:, ::2] > 20).all() and (ratio[:, ::2] < 45).all()
        yb = R.y_bound(raw, part, count, u=m * R.U24)
        print(f"chain offset {cin}: tiles {tiles}, m {m}, max |dy| {dev_.max():.3e}, bound there {yb.flat[dev_.argmax()]:.3e}, "
              f"largest share of the bound {np.max(dev_ / yb):.4f}")
        assert (dev_ <= yb).all()
