"""CPU: the routing of the 3D streaming passes (values_amd/csrc/stream3d_route.h) without a GPU -- the dry run
vx_norm_act_drop_pool_route against the kernel names tests/ops3d_ref.py pins (the GPU matrix ties those to real launches) and against
a restatement of the launch arithmetic the route replaced, the refusals of the ten entry points of norm_apply.hip with dummy pointers
(a refused call returns before any launch), and the header alone under ASan / UBSan."""
import ctypes as C
import os
import subprocess

import pytest

from tests import ops3d_ref as R
from tests.helpers import build_host_program
from values_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -5
BIG = 0x7fffffff
P = 0x10000          # a dummy pointer, 16-byte aligned: never dereferenced on the host


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def stat_src(tiles=5, count=100):
    st = _lib.StatSrc()
    st.stats_partial = 0x70000; st.tiles = tiles; st.eps = 1e-5; st.count = count
    return st


def norm_args(shape, c, *, pool=False, stats=False, lay=None, drop=0, **fields):
    """the vx_norm_args tests/test_gpu_stream3d.py launch_norm builds for (N, D, H, W) x C, with dummy pointers"""
    lay = dict(R.parse_layout("dense"), **(lay or {}))
    n, d, h, w = shape
    a = _lib.NormArgs()
    a.x = P
    if lay["x_xblk"]:
        a.x_xblk, a.x_half = lay["x_xblk"], lay["x_half"]
    else:
        a.x_pitch = c + lay["x_pad"]
    a.N, a.D, a.H, a.W, a.C = n, d, h, w, c
    a.act, a.drop_mode = 1, drop
    if not stats:
        a.mean, a.rstd = 0x20000, 0x30000
    if drop == _lib.VX_DROP_MASK:
        a.drop_mask = 0x80000
    if not lay["pool_only"]:
        a.out = 0x40000
        if lay["out_xblk"]:
            a.out_xblk, a.out_half = lay["out_xblk"], lay["out_half"]
        else:
            a.out_pitch, a.out_coff = (2 * c, c) if lay["out_pitch2"] else (c, 0)
    if pool:
        a.pool_out, a.pool_pitch = 0x50000, c + lay["pool_pad"]
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def dry_run(lib, a, repeat=1, st=None):
    """(code, kernel name, (grid_x, grid_y, per_sample, magic_pw, magic_c4, magic_rh)) of vx_norm_act_drop_pool_route"""
    buf, info = C.create_string_buffer(96), _lib.NormRouteInfo()
    rc = lib.vx_norm_act_drop_pool_route(C.byref(a), repeat, C.byref(st) if st is not None else None, buf, len(buf), C.byref(info))
    return rc, buf.value.decode(), tuple(getattr(info, f) for f, _ in _lib.NormRouteInfo._fields_)


def parent_geometry(n, d, h, w, c, pool, repeat, stats):
    """the launch arithmetic at the end of norm_act_drop_pool_impl before stream3d_route.h, literally, for arguments that passed its
    checks: (grid_x, grid_y, per_sample, mPW, mC4, mH), or None where it refused (decode bound, grid y)"""
    wide = pool and c // 4 > 32
    (pw, c4, rh), per = R.decode_divisors(pool, wide, c, d, h, w)
    dmax = pw if pw > rh else rh
    grid_y = n // repeat if (not pool and repeat > 1) else n
    if per * dmax >= (1 << 32) or grid_y > 65535:
        return None
    dc = (per, R.magic(pw), R.magic(c4), R.magic(rh))
    bx = (per + 255) // 256
    cap = (16384 + n - 1) // n
    if not pool and bx > cap:
        bx = cap if cap > 0 else 1
    if not pool and repeat > 1:
        ns = n // repeat
        fx = (per + 255) // 256
        fcap = (32768 + ns - 1) // ns
        if fx > fcap:
            fx = fcap
        return (fx, ns) + dc
    if stats:
        bx = (bx + 3) // 4
    return (bx, n) + dc


def _cases():
    """(id, instance, shape, C, repeat, layout, drop): the matrix, the grid-stride launches and the decode limit of the GPU module"""
    out = []
    for k in R.norm_cases():
        shape = (k.shape[0] * k.repeat,) + tuple(k.shape[1:])
        out.append((R.norm_case_id(k), k.inst, shape, k.C, k.repeat, R.parse_layout(k.layout), k.drop))
    for which, (pool, wide, c, d, h, w) in zip(["plain", "fanout", "plain_stats", "pool_stats", "wide_stats", "pool"], R.TRIP_SHAPES):
        ns, rep = {"plain": 20000, "fanout": 33000}.get(which, 3), 2 if which == "fanout" else 1
        out.append(("trip-" + which, which, (ns * rep, d, h, w), c, rep, None, 2))
    L = R.DECODE_LIMIT
    out.append(("decode-limit", "plain", (1, L["D"], L["H"], L["W"]), L["C"], 1, None, 0))
    return out


def test_dry_run_names_and_geometry(lib):
    """every case the GPU module launches: the dry run names the instance ops3d_ref.INSTANCES pins and reports the grid and the decode
    of the replaced launch arithmetic"""
    seen = set()
    for cid, inst, shape, c, rep, lay, drop in _cases():
        entry, pool, kname = R.INSTANCES[inst]
        stats = entry == "stats"
        a = norm_args(shape, c, pool=pool, stats=stats, lay=lay, drop=drop)
        rc, name, info = dry_run(lib, a, rep, stat_src() if stats else None)
        assert (rc, name) == (0, kname), (cid, rc, name, lib.vx_last_error_string())
        assert info == parent_geometry(*shape, c, pool, rep, stats), cid
        seen.add(name)
    assert seen == {v[2] for v in R.INSTANCES.values()}


def test_caps_and_limits_on_both_sides(lib):
    L = R.DECODE_LIMIT
    dims = (1, L["D"], L["H"], L["W"])
    assert dry_run(lib, norm_args(dims, L["C"]))[0] == 0
    refused = norm_args((1, L["D"] + 1, L["H"], L["W"]), L["C"])
    assert dry_run(lib, refused)[0] == E_SHAPE and parent_geometry(1, L["D"] + 1, L["H"], L["W"], L["C"], False, 1, False) is None
    assert lib.vx_norm_act_drop_pool(C.byref(refused), None) == E_SHAPE and b"32-bit index decode" in lib.vx_last_error_string()
    # the grid's y: 65535 samples, 65536; the fan-out's y is its N / x_repeat source samples
    for n, rep, ok in ((65535, 1, True), (65536, 1, False), (2 * 65535, 2, True), (2 * 65536, 2, False), (3 * 65535, 3, True)):
        a = norm_args((n, 1, 1, 1), 4)
        rc, name, info = dry_run(lib, a, rep)
        assert (rc == 0) == ok and (rc == 0 or rc == E_SHAPE), (n, rep, rc)
        assert (info if ok else None) == parent_geometry(n, 1, 1, 1, 4, False, rep, False)
        if ok:
            assert name == ("norm_act_drop_fanout_kernel" if rep > 1 else "norm_act_drop_pool_kernel<false,false>") and info[:3] == (1, 65535, 1)
    # the 16384 / N and 32768 / ns caps and the _stats quarter grid, restated: 40 x 40 x 40 x 8 channels = 128 000 pieces = 500 blocks
    for n, rep, stats, pool, want in ((1, 1, False, False, 500), (40, 1, False, False, 410), (16384, 1, False, False, 1), (16385, 1, False, False, 1),
                                      (2, 2, False, False, 500), (160, 2, False, False, 410), (40, 1, True, False, 103), (1, 1, True, False, 125),
                                      (40, 1, False, True, 125), (40, 1, True, True, 32), (40, 2, False, True, 125)):
        a = norm_args((n, 40, 40, 40), 8, pool=pool, stats=stats)
        rc, _, info = dry_run(lib, a, rep, stat_src() if stats else None)
        assert rc == 0 and info[0] == want and info == parent_geometry(n, 40, 40, 40, 8, pool, rep, stats), (n, rep, stats, pool, info)
    a = norm_args((2, 2, 2, 2), 8)
    assert lib.vx_norm_act_drop_pool_route(C.byref(a), 1, None, None, 0, None) == 0             # the name and the geometry are optional
    buf = C.create_string_buffer(8)
    assert lib.vx_norm_act_drop_pool_route(C.byref(a), 1, None, buf, 8, None) == 0 and buf.value == b"norm_ac"
    assert lib.vx_norm_act_drop_pool_route(None, 1, None, None, 0, None) == E_NULL


def _both(lib, a, code, rep=1, st=None, needle=b""):
    """refused with `code` by the dry run and, with the same message, by the entry point"""
    assert dry_run(lib, a, rep, st)[0] == code, lib.vx_last_error_string()
    msg = lib.vx_last_error_string()
    assert needle in msg, msg
    if st is not None:
        got = lib.vx_norm_act_drop_pool_stats(C.byref(a), C.byref(st), None)
    elif rep > 1:
        got = lib.vx_norm_act_drop_pool_bcast(C.byref(a), rep, None)
    else:
        got = lib.vx_norm_act_drop_pool(C.byref(a), None)
    assert got == code and lib.vx_last_error_string() == msg
    return msg


def test_refusals_the_gpu_module_asserts(lib):
    # pooling refuses the channel counts the shuffle cannot pair; the same C without pooling runs
    for c in R.POOL_REFUSED_C:
        _both(lib, norm_args((2, 2, 2, 4), c, pool=True), E_SHAPE, needle=b"C/4 to divide 32")
        assert dry_run(lib, norm_args((2, 2, 2, 4), c))[:2] == (0, "norm_act_drop_pool_kernel<false,false>")
    # a concat input goes with pooling and no broadcast
    lay = dict(x_xblk=2, x_half=1)
    _both(lib, norm_args((2, 2, 2, 4), 8, lay=lay), E_SHAPE, needle=b"concat input goes with pooling")
    _both(lib, norm_args((4, 2, 2, 4), 8, pool=True, lay=lay), E_SHAPE, rep=2, needle=b"concat input goes with pooling")
    _both(lib, norm_args((2, 2, 2, 6), 8, pool=True, lay=dict(x_xblk=3, x_half=0)), E_SHAPE, needle=b"bad concat input")     # xb in {1, 2, 4}
    _both(lib, norm_args((1, 2, 2, 2), 516, pool=True, stats=True), E_SHAPE, st=stat_src(2, 8), needle=b"(<= 512)")           # C <= 512
    # the decode limit and the grid's y (test_index_decode_at_its_limit)
    L = R.DECODE_LIMIT
    _both(lib, norm_args((1, L["D"] + 1, L["H"], L["W"]), L["C"]), E_SHAPE)
    _both(lib, norm_args((65536, 1, 1, 1), L["C"]), E_SHAPE)
    _both(lib, norm_args((2 * 65536, 1, 1, 1), L["C"]), E_SHAPE, rep=2)
    # vx_pool_finish and its z forms (test_pool_finish_refusals)
    off, st = P + 4, stat_src(1, 8)
    assert lib.vx_pool_finish(P, P, P, P, P, 4, 1, 8, 1, None) == E_ALIGN               # out_pitch < 8
    assert lib.vx_pool_finish(P, P, P, P, off, 8, 1, 8, 1, None) == E_ALIGN             # misaligned out
    assert lib.vx_pool_finish_z(P, P, P, P, P, 12, 1, 1, 8, 1, None) == E_ALIGN         # out_pitch < 16
    assert lib.vx_pool_finish_z(P, P, P, P, off, 16, 1, 1, 8, 1, None) == E_ALIGN
    assert lib.vx_pool_finish_z_stats(P, P, C.byref(st), P, 12, 1, 1, 8, 1, None) == E_ALIGN
    assert lib.vx_pool_finish_z_stats(P, P, C.byref(st), off, 16, 1, 1, 8, 1, None) == E_ALIGN
    # mean given together with a statistics source
    a = norm_args((1, 1, 1, 1), 8)
    assert lib.vx_norm_act_drop_pool_stats(C.byref(a), C.byref(st), None) == E_SHAPE
    assert lib.vx_norm_act_drop_pool_stats(C.byref(a), None, None) == E_NULL
    # vx_prenorm_split and its _stats form (test_prenorm_split_refusals)
    st = stat_src(1, 4)
    assert lib.vx_prenorm_split(off, P, P, 1, 4, 1.0, None) == E_ALIGN
    assert lib.vx_prenorm_split(P, P, P, 65536, 4, 1.0, None) == E_SHAPE
    assert lib.vx_prenorm_split_stats(off, C.byref(st), 1, 4, 1.0, None) == E_ALIGN
    assert lib.vx_prenorm_split_stats(P, C.byref(st), 65536, 4, 1.0, None) == E_SHAPE
    # the order of the checks: the statistics source before the shape, the shape and the alignment before it in the small passes
    assert lib.vx_norm_act_drop_pool_stats(C.byref(norm_args((0, 1, 1, 1), 8, stats=True)), C.byref(stat_src(0, 4)), None) == E_SHAPE
    assert lib.vx_last_error_string().startswith(b"vx_norm_act_drop_pool_stats: 0 tiles")
    assert lib.vx_prenorm_split_stats(off, None, 1, 4, 1.0, None) == E_ALIGN and lib.vx_prenorm_split_stats(P, None, 1, 4, 1.0, None) == E_NULL
    assert lib.vx_last_error_string() == b"vx_prenorm_split_stats: null statistics source"
    assert lib.vx_pool_finish_z_stats(P, P, None, P, 16, 65536, 1, 8, 1, None) == E_SHAPE and lib.vx_last_error_string() == b"vx_pool_finish_z_stats: N"
    # N % x_repeat comes after the decode / grid-y check
    a = norm_args((2 * 65536 + 1, 1, 1, 1), 4)
    assert b"more than 65535 samples" in _both(lib, a, E_SHAPE, rep=2)
    assert b"not a multiple of x_repeat=2" in _both(lib, norm_args((7, 1, 1, 1), 4), E_SHAPE, rep=2)


def test_refusals_where_the_replaced_arithmetic_wrapped(lib):
    """each at the smallest arguments that reach it; one step below, the call is accepted (dry run only: dummy pointers)"""
    # vx_instnorm_finalize: the grid (unsigned)(N * C) of an int product
    assert lib.vx_instnorm_finalize(P, 1 << 16, 1, 1 << 15, 8, 1e-5, P, P, None) == E_SHAPE
    assert lib.vx_last_error_string().startswith(b"vx_instnorm_finalize: N * C must stay below 2^31")
    # out_coff + C as an int wrapped below the pitch
    _both(lib, norm_args((2, 2, 2, 2), 4, out_coff=BIG - 3, out_pitch=BIG - 3), E_ALIGN, needle=b"pitches/offsets")
    assert dry_run(lib, norm_args((2, 2, 2, 2), 4, out_coff=BIG - 7, out_pitch=BIG - 3))[0] == 0
    # D H W C = 2^65 is 0 in an int64, which passed the < 2^32 guard
    _both(lib, norm_args((1, 1 << 21, 1 << 21, 1 << 21), 4), E_SHAPE, needle=b"vx_norm_act_drop_pool: sample too large")
    _both(lib, norm_args((1, BIG, BIG, BIG), BIG - 3, x_pitch=BIG - 3, out_pitch=BIG - 3), E_SHAPE, needle=b"vx_norm_act_drop_pool: sample too large")
    # the plane index n D + z as an int: N D = 2^31
    _both(lib, norm_args((1 << 15, 1 << 16, 1, 1), 4), E_SHAPE, needle=b"the plane index n D + z")
    assert dry_run(lib, norm_args(((1 << 15) - 1, 1 << 16, 1, 1), 4))[0] == 0
    # ... of the fan-out kernel's N / x_repeat source samples: 2^31 - 2^16 there, accepted as before
    assert dry_run(lib, norm_args((2 * ((1 << 15) - 1), 1 << 16, 1, 1), 4), 2)[:2] == (0, "norm_act_drop_fanout_kernel")
    # Dp * plane_voxels = 2^64 is 0 in an int64
    st = stat_src(1, 8)
    assert lib.vx_pool_finish_z(P, P, P, P, P, 16, 1, 4, 1 << 62, 1, None) == E_SHAPE
    assert lib.vx_last_error_string() == b"vx_pool_finish_z: empty / too large"
    assert lib.vx_pool_finish_z_stats(P, P, C.byref(st), P, 16, 1, 4, 1 << 62, 1, None) == E_SHAPE
    assert lib.vx_last_error_string() == b"vx_pool_finish_z_stats: empty / too large"
    # the guards that were sound stay where they were
    assert lib.vx_pool_finish_z(P, P, P, P, P, 16, 1, 1 << 14, 1 << 14, 1, None) == E_SHAPE
    assert lib.vx_pool_finish(P, P, P, P, P, 8, 1, 1 << 30, 1, None) == E_SHAPE and lib.vx_prenorm_split(P, P, P, 1, 1 << 30, 1.0, None) == E_SHAPE
    assert lib.vx_drop_hash_mask(1, 2, 1, 1 << 32, P, None) == E_SHAPE and lib.vx_drop_hash_mask(1, 2, 1, 8, P + 2, None) == E_ALIGN
    assert lib.vx_drop_hash_mask(1, 2, 1, 8, None, None) == E_ALIGN and lib.vx_instnorm_finalize(None, 1, 1, 8, 8, 1e-5, P, P, None) == E_NULL


# ---------------------------------------------------------------------------------------------
# the routing header under sanitizers: a stand-alone program, no sanitizer runtime in this process

def test_routing_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "stream3d_route_host")
    build_host_program(os.path.join(ROOT, "tests", "stream3d_route_host.cpp"), exe)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr + res.stdout
    out = res.stdout.splitlines()
    walked, inst = (dict(zip(f[::2], f[1::2])) for f in (out[0].split(), out[1].split()[1:]))
    # zero unsound routes: an accepted route names a listed instance, keeps grid_x within its cap, grid_y in 1..65535, the decode exact
    # and the pieces equal to the 128-bit product; a refusal is a VX_E_* code with a message
    assert int(walked["routes"]) > 10 ** 6 and int(walked["norm"]) > 10 ** 6 and int(walked["taken"]) > 10 ** 4 and int(walked["unsound"]) == 0
    # the six instances of the list, the fan-out kernel and the six kernels of the small passes that report a name
    assert out[1].startswith("instances ") and (int(inst["listed"]), int(inst["named"]), int(inst["missing"])) == (13, 13, 0)
