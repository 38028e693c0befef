"""CPU: the routing of vx_conv2d (values_amd/csrc/conv2d_route.h) without a GPU -- the dry run vx_conv2d_route against the routes
recorded from real launches (tests/golden/conv2d_routes.json, part (b)), its refusals against vx_conv2d's, and the header alone
under ASan / UBSan."""
import ctypes as C
import json
import os
import subprocess

import pytest

from tests import conv2d_route_cases as rc
from tests.helpers import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -5
INSTANCES = 56 + 9      # conv2d_s16_kernel + conv2d_mfma_kernel instances (C2S_INSTANCES, C2_INSTANCES)


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
    # the cases were chosen to reach every instance, weights resident and re-staged, one chunk and several: the recorded launches did
    rows = list(golden["layers"].values())
    assert len({r[0] for r in rows}) == INSTANCES
    assert {(r[1] > 1, r[2]) for r in rows} == {(False, 0), (True, 0), (True, 1)}
    assert {r[1] for r in rows} >= {1, 2, 3, 4, 5, 12}
    # eval mode runs every conv but the class head on an epilogue instance (a seventh template argument), training mode none
    epi = {cid: sum(n.count(",") == 6 for n in names) for cid, names in golden["forward"].items()}
    assert epi["eval:default"] == len(golden["forward"]["eval:default"]) - 1 and epi["train:default"] == 0
    assert all(n.startswith("conv2d_mfma_kernel<") for n in golden["forward"]["train:fp32"] + golden["forward"]["eval:fp32"])


def test_dry_run_reproduces_the_recorded_routes(lib, golden, vxcfg):
    """every single-layer entry: the dry run, with dummy pointers and no GPU, names the instance the real launch ran and the
    geometry recorded for it"""
    for case in rc.LAYER_CASES:
        vxcfg.set(conv_fp32=0, c2s_no_wide=0, c2s_no_oct=0)
        vxcfg.set(**case["cfg"])
        code, name, geo, lds = rc.dry_run(lib, rc.layer_args(lib, case, rc.dummy_ptr))
        assert [code, name] + list(geo) == [0] + golden["layers"][case["id"]], (case["id"], code, lib.vx_last_error_string())
        assert 0 < lds <= 160 * 1024


BASE = dict(ks=3, s=1, h=16, w=16, cin=32, cout=16, epi=0, cfg={})
EPI = dict(BASE, epi=1)
# (case, configuration, {field: value}, code): one call per check of vx_conv2d, in its order
REFUSALS = [
    (BASE, {}, dict(in_=None), E_NULL), (BASE, {}, dict(w_packed=None), E_NULL), (BASE, {}, dict(out=None), E_NULL),
    (BASE, {}, dict(N=0), E_SHAPE), (BASE, {}, dict(H=-1), E_SHAPE),
    (BASE, {}, dict(Cin=12), E_SHAPE), (BASE, {}, dict(Cin=0), E_SHAPE), (BASE, {}, dict(Cout=0), E_SHAPE),
    (BASE, {}, dict(KS=5), E_SHAPE), (BASE, {}, dict(S=3), E_SHAPE), (BASE, {}, dict(KS=1, S=2), E_SHAPE),
    (BASE, {}, dict(w_family=3), E_DTYPE), (BASE, {}, dict(w_family=12), E_DTYPE), (BASE, {}, dict(w_family=211), E_DTYPE),
    (BASE, {}, dict(w_family=111), E_DTYPE),                          # one octet pads to Cin = 16, not 32
    (BASE, dict(c2s_no_oct=1), dict(w_family=311), E_DTYPE),          # the configuration packs no octets
    (BASE, dict(conv_fp32=1), dict(w_family=311), E_DTYPE),
    (BASE, {}, dict(in_pitch=16), E_ALIGN),                           # in_pitch <= Cin - 16
    (BASE, {}, dict(in_pitch=22), E_ALIGN), (BASE, {}, dict(out_pitch=12), E_ALIGN), (BASE, {}, dict(out_pitch=18), E_ALIGN),
    (BASE, {}, dict(out_coff=4), E_ALIGN), (BASE, {}, dict(out_coff=2, out_pitch=24), E_ALIGN),
    (BASE, {}, dict(in_=0x10004), E_ALIGN), (BASE, {}, dict(out=0x40008), E_ALIGN), (BASE, {}, dict(bias=0x30004), E_ALIGN),
    (BASE, {}, dict(H=1 << 14, W=1 << 14), E_SHAPE), (BASE, {}, dict(out_pitch=1 << 22), E_SHAPE),
    (BASE, {}, dict(in_scale=0x90000), E_NULL), (BASE, {}, dict(in_shift=0x90000), E_NULL),
    (BASE, {}, dict(in_scale=0x90000, in_shift=0xa0000, in_cpitch=16), E_SHAPE),            # in_cpitch == Cin - 16
    (BASE, {}, dict(in_scale=0x90000, in_shift=0xa0000, in_cpitch=32, in_group_images=-1), E_SHAPE),
    (BASE, dict(conv_fp32=1), dict(in_scale=0x90000, in_shift=0xa0000, in_cpitch=32), E_SHAPE),
    (BASE, {}, dict(out_scale=0x60000, stats_partial=None), E_NULL), (BASE, {}, dict(out_shift=0x60000, stats_partial=None), E_NULL),
    (BASE, {}, dict(out_add=0x80000, out_add_pitch=16), E_NULL), (BASE, {}, dict(out_act=1), E_DTYPE),
    (EPI, {}, dict(stats_partial=0x50000), E_DTYPE), (EPI, dict(conv_fp32=1), {}, E_DTYPE), (EPI, {}, dict(out_act=1), E_DTYPE),
    (EPI, {}, dict(out_add_pitch=12), E_ALIGN), (EPI, {}, dict(out_add_pitch=18), E_ALIGN), (EPI, {}, dict(out_add_pitch=1 << 22), E_SHAPE),
    (EPI, {}, dict(out_add=0x80004), E_ALIGN),
]
CHECKS = ["null tensor pointer", "empty tensor", "positive multiple of 16", "unsupported (3x3 s1/s2, 1x1 s1)", "re-pack them",
          "pitches/offsets must be", "pointers must be 16-byte aligned", "one image must stay below 2 GiB", "in_scale / in_shift must come together",
          "the input prologue needs", "out_scale / out_shift must come together", "out_add needs out_scale", "out_act needs out_scale",
          "out_scale together with stats_partial", "the output epilogue (out_scale) needs the split-fp16", "out_act must be none or relu",
          "out_add_pitch must be", "one image of out_add must stay below 2 GiB", "out_add must be 16-byte aligned"]
# ... and what the same checks let through: the octet families on the padded channel count, both sides of the pitch boundaries
ACCEPTED = [
    (BASE, {}, {}, "conv2d_s16_kernel<3,1,1,2,16,0>"), (EPI, {}, {}, "conv2d_s16_kernel<3,1,1,2,16,0,1>"),
    (BASE, {}, dict(w_family=311), "conv2d_s16_kernel<3,1,1,1,16,3>"),                        # 17..24 real channels pad to 32
    (BASE, {}, dict(w_family=111, Cin=16, in_pitch=4), "conv2d_s16_kernel<3,1,1,1,16,1>"),    # <= 8 real channels pad to 16
    (BASE, {}, dict(in_pitch=20), "conv2d_s16_kernel<3,1,1,2,16,0>"),                         # in_pitch == Cin - 12
    (BASE, {}, dict(in_scale=0x90000, in_shift=0xa0000, in_cpitch=17), "conv2d_s16_kernel<3,1,1,2,16,0>"),   # in_cpitch == Cin - 15
    (BASE, {}, dict(bias=None), "conv2d_s16_kernel<3,1,1,2,16,0>"),
    (EPI, {}, dict(out_add=None, out_add_pitch=0, out_act=0), "conv2d_s16_kernel<3,1,1,2,16,0,1>"),
    (BASE, dict(conv_fp32=1), {}, "conv2d_mfma_kernel<3,1,1,1,16>"),
]


def _args(lib, vxcfg, case, cfg, fields):
    vxcfg.set(conv_fp32=0, c2s_no_wide=0, c2s_no_oct=0)
    vxcfg.set(**cfg)
    a = rc.layer_args(lib, case, rc.dummy_ptr)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def test_dry_run_returns_the_refusals_of_the_launch(lib, vxcfg):
    """vx_conv2d_route and vx_conv2d are one route: the same code and the same message for a refused call"""
    msgs = set()
    for case, cfg, fields, code in REFUSALS:
        a = _args(lib, vxcfg, case, cfg, fields)
        got, name, _, _ = rc.dry_run(lib, a)
        msg = lib.vx_last_error_string()
        assert got == code and msg.startswith(b"vx_conv2d: "), (fields, cfg, got, msg)
        assert lib.vx_conv2d(C.byref(a), None) == code and lib.vx_last_error_string() == msg, (fields, cfg)
        msgs.add(msg.decode())
    for check in CHECKS:                                   # every check of the route refused at least one call
        assert any(check in m for m in msgs), check
    for case, cfg, fields, want in ACCEPTED:
        got, name, _, _ = rc.dry_run(lib, _args(lib, vxcfg, case, cfg, fields))
        assert (got, name) == (0, want), (fields, cfg, got, name, lib.vx_last_error_string())
    assert lib.vx_conv2d_route(None, None, 0, None) == E_NULL and lib.vx_conv2d(None, None) == E_NULL
    a = _args(lib, vxcfg, BASE, {}, {})
    assert lib.vx_conv2d_route(C.byref(a), None, 0, None) == 0          # the name and the geometry are optional
    buf = C.create_string_buffer(8)
    assert lib.vx_conv2d_route(C.byref(a), buf, 8, None) == 0 and buf.value == b"conv2d_"    # ... and the name truncated to the caller's buffer


# ---------------------------------------------------------------------------------------------
# the routing header under sanitizers: a stand-alone program, no sanitizer runtime in this process

def test_routing_header_under_asan_ubsan(golden, tmp_path):
    exe = str(tmp_path / "conv2d_route_host")
    build_host_program(os.path.join(ROOT, "tests", "conv2d_route_host.cpp"), exe)
    lines = "".join("%s %d %d %d %d %d %d %d %d %d %d %d\n" % (c["id"], c["ks"], c["s"], c["h"], c["w"], c["cin"], c["cout"], rc.LAYER_N, c["epi"],
                                                              c["cfg"].get("c2s_no_wide", 0), c["cfg"].get("c2s_no_oct", 0),
                                                              c["cfg"].get("conv_fp32", 0)) for c in rc.LAYER_CASES)
    res = subprocess.run([exe], input=lines, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr + res.stdout
    out = res.stdout.splitlines()
    walked, inst = (dict(zip(f[::2], f[1::2])) for f in (out[1].split(), out[2].split()[1:]))
    assert out[0].startswith("queries ") and int(out[0].split()[1]) > 10 ** 4
    # zero unsound routes: an accepted route names a listed instance with tiles >= 1, 0 < grid_x <= N x tiles and at most 160 KiB of
    # LDS; a refusal is a VX_E_* code with a message
    assert int(walked["routes"]) > 10 ** 6 and int(walked["taken"]) > 10 ** 5 and int(walked["unsound"]) == 0
    # every instance of both lists is named by an accepted route of the walk
    assert out[2].startswith("instances ") and (int(inst["listed"]), int(inst["named"]), int(inst["missing"])) == (INSTANCES, INSTANCES, 0)
    # the header alone gives the recorded routes (the library is the same header compiled without sanitizers)
    got = {ln.split()[1]: [int(ln.split()[2]), ln.split()[3]] + [int(v) for v in ln.split()[4:8]] for ln in out if ln.startswith("case ")}
    assert got == {cid: [0] + row for cid, row in golden["layers"].items()}
