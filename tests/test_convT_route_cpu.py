"""CPU: the routing of vx_convT_k2s2 (values_amd/csrc/convT_route.h) without a GPU -- the dry run vx_convT_k2s2_route against the
routes recorded from real launches (tests/golden/convT_routes.json), its refusals against vx_convT_k2s2's, the 2^27 decode bound
against a restatement of the if-chain the route replaced, and the header alone under ASan / UBSan."""
import ctypes as C
import json
import os
import subprocess

import pytest

from tests import convT_route_cases as rc
from tests.helpers import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -5
NAMES = 2 * (7 + 2) + 2      # tile instances with and without the mask, the rows kernel (one name), the generic kernel


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", rc.GOLDEN)))


@pytest.fixture(scope="module")
def lib():
    from values_amd import _lib
    return _lib.load()


def test_golden_holds_every_case(golden):
    assert sorted(golden["layers"]) == sorted(c["id"] for c in rc.LAYER_CASES)
    names = {r[0] for r in golden["layers"].values()}
    # the cases were chosen to reach all four kernels, every (Cin, RT) of the tile kernels and a mask instance of each: the recorded
    # launches did
    assert {n.split("<")[0] for n in names} == {"convT_k2s2_mfma_kernel", "convT_k2s2_s16_kernel", "convT_k2s2_rows_kernel", "convT_k2s2_kernel"}
    assert {n[:-len(",false>")] for n in names if n.endswith(",false>")} == \
        {f"convT_k2s2_mfma_kernel<{c},{r}" for c, r in ((16, 4), (16, 8), (32, 4), (32, 8), (64, 4), (64, 8), (128, 4))} | \
        {"convT_k2s2_s16_kernel<64,4", "convT_k2s2_s16_kernel<128,2"}
    assert {"convT_k2s2_mfma_kernel<16,4,true>", "convT_k2s2_s16_kernel<64,4,true>"} <= names
    # both sides of the decode bound
    lay = golden["layers"]
    for ch in ("16->8", "32->16"):
        assert lay[f"decode:{ch}:1x1x1x65535"][0].startswith("convT_k2s2_mfma_kernel<") and lay[f"decode:{ch}:1x1x1x65536"][0] == "convT_k2s2_rows_kernel"
    assert lay["generic:16->24:2x2x2x2"][0] == "convT_k2s2_mfma_kernel<16,4,false>" and lay["generic:16->24:1x1x1x65536"][0] == "convT_k2s2_kernel"


def test_dry_run_reproduces_the_recorded_routes(lib, golden, vxcfg):
    """every case: the dry run, with dummy pointers and no GPU, names the kernel the real launch ran and the grid recorded for it"""
    for case in rc.LAYER_CASES:
        vxcfg.set(conv_fp32=0)
        vxcfg.set(**case["cfg"])
        got = rc.dry_run(lib, rc.layer_args(case, rc.dummy_ptr))
        assert list(got) == [0] + golden["layers"][case["id"]], (case["id"], got, lib.vx_last_error_string())


def parent_chain(N, D, H, W, Cin, Cout, conv_fp32, mask=False):
    """the if-chain at the end of vx_convT_k2s2 before convT_route.h, literally (dead conditions included), for arguments that
    passed its checks and whose products fit an int64: the kernel name it noted"""
    m = "true" if mask else "false"
    dmax = (W if W > D else D) if W > H else (H if H > D else D)
    if N * D * H * W < (1 << 27) and N * D * H * W * dmax < (1 << 32):
        tiles = Cout // 2
        if Cin == 16 and tiles % 4 == 0:
            return f"convT_k2s2_mfma_kernel<16,{4 if tiles % 8 else 8},{m}>"
        if Cin == 32 and tiles % 4 == 0:
            return f"convT_k2s2_mfma_kernel<32,{4 if tiles % 8 else 8},{m}>"
        if conv_fp32 == 0:
            if Cin == 64 and tiles % 4 == 0:
                return f"convT_k2s2_s16_kernel<64,4,{m}>"
            if Cin == 128 and tiles % 2 == 0:
                return f"convT_k2s2_s16_kernel<128,2,{m}>"
        if Cin == 64 and tiles % 4 == 0:
            return f"convT_k2s2_mfma_kernel<64,{4 if tiles % 8 else 8},{m}>"
        if Cin == 128 and tiles % 4 == 0:
            return f"convT_k2s2_mfma_kernel<128,4,{m}>"
    if (Cin == 16 or Cin == 32) and Cout <= 128 and 256 % (2 * (Cout // 4)) == 0:
        return "convT_k2s2_rows_kernel"
    return "convT_k2s2_kernel"


# nvox = N x W with D = H = 1 and W <= 16, so that the other decode bound (nvox x dmax < 2^32) holds on both sides of this one:
# 2^27 - 16, 2^27 - 1 = 7 x 19173961, 2^27, 2^27 + 1 = 9 x 14913081
NVOX_2_27 = [((1 << 23) - 1, 16), (19173961, 7), (1 << 23, 16), (14913081, 9)]


def test_decode_bound_2_27_is_the_parents(lib, vxcfg):
    """the bound no launch can reach cheaply: at nvox = 2^27 - 16, 2^27 - 1, 2^27, 2^27 + 1 the dry run takes the kernel the
    replaced if-chain took, for every Cin family and both configurations"""
    assert [n * w - (1 << 27) for n, w in NVOX_2_27] == [-16, -1, 0, 1]
    seen = set()
    for fp32 in (0, 1):
        vxcfg.set(conv_fp32=fp32)
        for n, w in NVOX_2_27:
            for cin in (16, 32, 64, 128, 8):
                for cout in (8, 16, 24, 64):
                    for drop in (rc.DROP_NONE, rc.DROP_MASK):
                        case = rc._case("b27", cin, cout, (n, 1, 1, w), drop=drop)
                        code, name, gx, gy = rc.dry_run(lib, rc.layer_args(case, rc.dummy_ptr))
                        want = parent_chain(n, 1, 1, w, cin, cout, fp32, drop == rc.DROP_MASK)
                        assert (code, name) == (0, want), (case["id"], fp32, code, name, want)
                        seen.add((n * w < (1 << 27), name.split("<")[0]))
    assert seen == {(True, "convT_k2s2_mfma_kernel"), (True, "convT_k2s2_s16_kernel"), (True, "convT_k2s2_kernel"),
                    (False, "convT_k2s2_rows_kernel"), (False, "convT_k2s2_kernel")}
    # ... and the restatement agrees with the recorded launches
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", rc.GOLDEN)))["layers"]
    for case in rc.LAYER_CASES:
        assert parent_chain(*case["vol"], case["cin"], case["cout"], case["cfg"].get("conv_fp32", 0), case["drop"] == rc.DROP_MASK) == golden[case["id"]][0]


BASE = rc._case("base", 16, 8, (2, 4, 4, 4))
BIG = 0x7fffffff
# (fields, code): one call per check of vx_convT_k2s2, in its order
REFUSALS = [
    (dict(in_=None), E_NULL), (dict(w_packed=None), E_NULL), (dict(bias=None), E_NULL), (dict(out=None), E_NULL),
    (dict(Cin=0), E_SHAPE), (dict(Cin=6, in_pitch=8), E_SHAPE), (dict(Cout=4), E_SHAPE), (dict(Cout=-8), E_SHAPE),
    (dict(N=0), E_SHAPE), (dict(D=-1), E_SHAPE), (dict(W=0), E_SHAPE),
    (dict(in_pitch=12), E_ALIGN), (dict(in_pitch=18), E_ALIGN),
    (dict(out_xblk=3), E_SHAPE), (dict(out_xblk=4, W=3), E_SHAPE), (dict(out_xblk=2, out_half=2), E_SHAPE),
    (dict(out_pitch=10), E_ALIGN), (dict(out_coff=2, out_pitch=12), E_ALIGN), (dict(out_coff=4), E_ALIGN),
    (dict(out_coff=BIG - 3, out_pitch=BIG - 3), E_ALIGN),                 # out_coff + Cout as an int wrapped below the pitch
    (dict(drop_mode=rc.DROP_MASK), E_NULL),
    (dict(D=1 << 10, H=1 << 10, W=1 << 6), E_SHAPE),                      # D H W 8 Cout = 2^32
    (dict(D=BIG, H=BIG, W=BIG), E_SHAPE),                                 # ... and beyond int64
    (dict(N=1 << 20, D=1 << 10, H=1, W=1), E_SHAPE),                      # N 2 D = 2^31 on the rows kernel
    (dict(N=1 << 20, D=1 << 10, H=1, W=1, Cin=8), E_SHAPE),               # ... and on the generic kernel
]
CHECKS = ["null tensor", "(mult of 4) Cout=", "empty tensor", "input pitch", "bad concat layout", "pitches/offsets must be",
          "mask mode without mask", "sample too large", "N * 2 D must stay below 2^31"]
ACCEPTED = [
    ({}, "convT_k2s2_mfma_kernel<16,4,false>"), (dict(range_flag=None), "convT_k2s2_mfma_kernel<16,4,false>"),
    (dict(drop_mode=rc.DROP_MASK, drop_mask=0x50000), "convT_k2s2_mfma_kernel<16,4,true>"),
    (dict(in_pitch=20, out_pitch=16, out_coff=8), "convT_k2s2_mfma_kernel<16,4,false>"),
    (dict(out_xblk=4, out_half=1), "convT_k2s2_mfma_kernel<16,4,false>"),
    (dict(D=1 << 10, H=1 << 10, W=(1 << 6) - 1, N=1), "convT_k2s2_rows_kernel"),                     # D H W 8 Cout = 2^32 - 2^26
    (dict(N=(1 << 20) - 1, D=1 << 10, H=1, W=1), "convT_k2s2_rows_kernel"),                          # N 2 D = 2^31 - 2^11
    (dict(N=(1 << 20) - 1, D=1 << 10, H=1, W=1, Cin=8, in_pitch=8), "convT_k2s2_kernel"),
]


def _args(fields):
    a = rc.layer_args(BASE, rc.dummy_ptr)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def test_dry_run_returns_the_refusals_of_the_launch(lib, vxcfg):
    """vx_convT_k2s2_route and vx_convT_k2s2 are one route: the same code and the same message for a refused call"""
    vxcfg.set(conv_fp32=0)
    msgs = set()
    for fields, code in REFUSALS:
        a = _args(fields)
        got = rc.dry_run(lib, a)[0]
        msg = lib.vx_last_error_string()
        assert got == code and msg.startswith(b"vx_convT_k2s2: "), (fields, got, msg)
        assert lib.vx_convT_k2s2(C.byref(a), None) == code and lib.vx_last_error_string() == msg, fields
        msgs.add(msg.decode())
    for check in CHECKS:                                   # every check of the route refused at least one call
        assert any(check in m for m in msgs), check
    for fields, want in ACCEPTED:
        got = rc.dry_run(lib, _args(fields))
        assert got[:2] == (0, want) and got[2] >= 1 and got[3] >= 1, (fields, got, lib.vx_last_error_string())
    assert lib.vx_convT_k2s2_route(None, None, 0, None) == E_NULL and lib.vx_convT_k2s2(None, None) == E_NULL
    a = _args({})
    assert lib.vx_convT_k2s2_route(C.byref(a), None, 0, None) == 0          # the name and the grid are optional
    buf = C.create_string_buffer(8)
    assert lib.vx_convT_k2s2_route(C.byref(a), buf, 8, None) == 0 and buf.value == b"convT_k"    # ... and the name truncated to the caller's buffer
    # the packed size: one rule with the route's channel check, -1 beyond int64
    assert lib.vx_convT_k2s2_packed_floats(16, 8) == 1024 and lib.vx_convT_k2s2_packed_floats(6, 8) == -1
    assert lib.vx_convT_k2s2_packed_floats(16, 4) == -1 and lib.vx_convT_k2s2_packed_floats(BIG - 3, BIG - 7) == -1
    assert lib.vx_convT_k2s2_packed_floats(1 << 28, 1 << 28) == 1 << 59


# ---------------------------------------------------------------------------------------------
# the routing header under sanitizers: a stand-alone program, no sanitizer runtime in this process

def test_routing_header_under_asan_ubsan(golden, tmp_path):
    exe = str(tmp_path / "convT_route_host")
    build_host_program(os.path.join(ROOT, "tests", "convT_route_host.cpp"), exe)
    lines = "".join("%s %d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (
        (c["id"],) + tuple(c["vol"]) + (c["cin"], c["cout"], c["cin"] + c["in_extra"], c["cout"] + c["out_extra"], c["out_coff"], c["xblk"],
                                       c["half"], c["drop"], c["cfg"].get("conv_fp32", 0))) for c in rc.LAYER_CASES)
    res = subprocess.run([exe], input=lines, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr + res.stdout
    out = res.stdout.splitlines()
    walked, inst = (dict(zip(f[::2], f[1::2])) for f in (out[1].split(), out[2].split()[1:]))
    assert out[0].startswith("queries ") and int(out[0].split()[1]) >= 144
    # zero unsound routes: an accepted route names a listed instance with grid_x, grid_y >= 1 and meets every bound the header
    # states for its kernel; a refusal is a VX_E_* code with a message
    assert int(walked["routes"]) > 2 * 10 ** 6 and int(walked["taken"]) > 10 ** 4 and int(walked["unsound"]) == 0
    # every instance of the lists is named by an accepted route of the walk
    assert out[2].startswith("instances ") and (int(inst["listed"]), int(inst["named"]), int(inst["missing"])) == (NAMES, NAMES, 0)
    # the header alone gives the recorded routes (the library is the same header compiled without sanitizers)
    got = {ln.split()[1]: [int(ln.split()[2]), ln.split()[3]] + [int(v) for v in ln.split()[4:6]] for ln in out if ln.startswith("case ")}
    assert got == {cid: [0] + row for cid, row in golden["layers"].items()}
