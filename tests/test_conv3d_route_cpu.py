"""CPU: the routing of vx_conv3d_k3 (values_amd/csrc/conv3d_route.h) without a GPU -- the dry run vx_conv3d_k3_route against the
routes recorded from real launches (tests/golden/conv3d_routes.json, part (b)), and the header alone under ASan / UBSan."""
import ctypes as C
import json
import os
import subprocess

import pytest

from tests import conv3d_route_cases as rc
from tests.helpers import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -5


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", rc.GOLDEN)))


@pytest.fixture(scope="module")
def lib():
    from values_amd import _lib
    return _lib.load()


def test_golden_holds_every_case(golden):
    assert sorted(golden["layers"]) == sorted(c["id"] for c in rc.LAYER_CASES)
    assert sorted(golden["forward"]) == sorted(c[0] for c in rc.FORWARD_CASES)
    # the shapes were chosen to reach each family: the recorded launches did
    fams = {cid.split(":")[0]: set() for cid in golden["layers"]}
    for cid, name in golden["layers"].items():
        fams[cid.split(":")[0]].add(name.split("<")[0])
    assert fams["xp8w"] >= {"conv3d_xp8w_kernel"} and fams["zc16"] >= {"conv3d_zc16_kernel"} and fams["deep"] >= {"conv3d_deep_kernel"}
    assert fams["s16"] == {"conv3d_k3_s16_kernel"} and fams["fp32"] == {"conv3d_k3_mfma_kernel", "conv3d_k3_c8_kernel"}
    # (6, 8, 8): six planes hold no whole deep tile (and the tile kernel's four statistics entries no three) -- every launch falls
    # through to the tile kernel, next to (8, 8, 8) where the deep kernel runs
    assert all(n.startswith("conv3d_k3_s16_kernel") for cid, n in golden["layers"].items() if cid.startswith("deep:6x8x8:"))
    assert golden["layers"]["deep:8x8x8:32->32:stats"] == "conv3d_deep_kernel<4,0,0>"


def test_dry_run_reproduces_the_recorded_routes(lib, golden, vxcfg):
    """every single-layer entry: the dry run, with dummy pointers and no GPU, names the instance the real launch ran"""
    for case in rc.LAYER_CASES:
        vxcfg.set(conv_fp32=case["cfg"].get("conv_fp32", 0))
        code, name = rc.dry_run(lib, rc.layer_args(lib, case, rc.dummy_ptr))
        assert (code, name) == (0, golden["layers"][case["id"]]), (case["id"], code, lib.vx_last_error_string())


def test_dry_run_returns_the_refusals_of_the_launch(lib, vxcfg):
    """vx_conv3d_k3_route and vx_conv3d_k3 are one route: the same code and the same message for a refused call"""
    from values_amd import _lib
    case = dict(shape=(32, 32, 32), cin=16, cout=16, epilogue="lrelu", cfg={})
    for field, value, code in (("in_planar", 1, 0), ("Cin", 12, E_SHAPE), ("in_", None, E_NULL), ("in_pitch", 18, E_ALIGN),
                               ("act", 3, E_DTYPE), ("w_family", 1, E_DTYPE), ("products", 1, E_SHAPE), ("acc_in", 0x90000, 0),
                               ("out_pitch", 1 << 22, E_SHAPE), ("head_out", 0x90000, E_NULL)):
        a = rc.layer_args(lib, case, rc.dummy_ptr)
        setattr(a, field, value)
        if field == "acc_in":
            a.acc_pitch = 16
        got, name = rc.dry_run(lib, a)
        assert got == code, (field, got, lib.vx_last_error_string())
        if code:
            msg = lib.vx_last_error_string()
            assert lib.vx_conv3d_k3(C.byref(a), None) == code and lib.vx_last_error_string() == msg, field
        else:
            assert name.startswith("conv3d_zc16_kernel<16,3,"), (field, name)
    assert lib.vx_conv3d_k3_route(None, None, 0) == E_NULL
    a = rc.layer_args(lib, case, rc.dummy_ptr)
    assert lib.vx_conv3d_k3_route(C.byref(a), None, 0) == 0            # the name is optional
    buf = C.create_string_buffer(8)
    assert lib.vx_conv3d_k3_route(C.byref(a), buf, 8) == 0 and buf.value == b"conv3d_"   # ... and truncated to the caller's buffer


# ---------------------------------------------------------------------------------------------
# the routing header under sanitizers: a stand-alone program, no sanitizer runtime in this process

def test_routing_header_under_asan_ubsan(golden, tmp_path):
    exe = str(tmp_path / "conv3d_route_host")
    build_host_program(os.path.join(ROOT, "tests", "conv3d_route_host.cpp"), exe)
    lines = "".join("%s %d %d %d %d %d %d %s %d\n" % ((c["id"],) + tuple(c["shape"]) + (c["cin"], c["cout"], rc.LAYER_N, c["epilogue"],
                                                                                   c["cfg"].get("conv_fp32", 0))) for c in rc.LAYER_CASES)
    res = subprocess.run([exe], input=lines, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr + res.stdout
    out = res.stdout.splitlines()
    walked = dict(zip(out[1].split()[::2], out[1].split()[1::2]))
    assert out[0].startswith("queries ") and int(out[0].split()[1]) > 10 ** 6
    assert int(walked["routes"]) > 10 ** 6 and int(walked["taken"]) > 10 ** 5 and int(walked["unsound"]) == 0
    # the header alone gives the recorded routes (the library is the same header compiled without sanitizers)
    got = {ln.split()[1]: (int(ln.split()[2]), ln.split()[3]) for ln in out if ln.startswith("case ")}
    assert got == {cid: (0, name) for cid, name in golden["layers"].items()}
