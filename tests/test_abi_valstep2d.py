"""CPU: vx_val_ssn2d_sums_batched and its workspace companion are declared, exported and bound, the workspace size is the
stated layout, and every refusal the header lists is made by a host-side check -- so a wrong call is refused on a box
without a GPU too.  (That the workspace is sufficient is shown by every GPU test: values_amd.validation allocates exactly
what the companion returns.)"""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vx_val_ssn2d_sums_workspace_bytes", "vx_val_ssn2d_sums_batched")
E_NULL, E_SHAPE, E_WORKSPACE = "VX_E_NULL", "VX_E_SHAPE", "VX_E_WORKSPACE"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from values_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


@pytest.fixture(scope="module")
def codes():
    names = [E_NULL, E_SHAPE, E_WORKSPACE]
    code = "#include <stdio.h>\n#include \"values_amd.h\"\nint main(void){printf(\"%d %d %d\\n\", " + ", ".join(names) + "); return 0;}\n"
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write(code)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])  # header is plain C
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    return dict(zip(names, got))


def test_new_symbols_are_declared_exported_and_bound(lib):
    from values_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "values_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vx_[a-zA-Z0-9_]+)\s*\(", hdr))
    for n in NEW:
        assert n in declared and hasattr(lib, n) and n in _lib.SIGNATURES, n


def expected_bytes(B, S, C, h0, w0, H, W):
    lowres = ((S + 1) * B * h0 * w0 * C * 4 + 15) // 16 * 16          # comb [S] | expm, float32, rounded up to 16 bytes
    spans = (H * W + 255) // 256
    return lowres + B * spans * (S * (1 + 2 * C) + C + 2) * 8          # one float64 row per span of 256 pixels


def test_workspace_companion(lib):
    ws = lib.vx_val_ssn2d_sums_workspace_bytes
    for shape in ((1, 1, 2, 1, 1, 1, 1), (3, 10, 19, 5, 7, 19, 27), (4, 10, 19, 64, 120, 256, 478), (1, 32, 32, 16, 24, 64, 96),
                  (1, 1, 3, 1, 1, 16, 16), (2, 3, 5, 1, 3, 16, 17)):
        assert ws(*shape) == expected_bytes(*shape), shape
    assert ws(1, 1, 3, 1, 1, 16, 16) == 32 + (1 * 7 + 5) * 8            # 6 floats of head (24 bytes) round up to 32; one span
    # 0 for what the call refuses
    ok = dict(B=2, S=4, C=4, h0=4, w0=6, H=16, W=24)
    assert ws(*ok.values()) > 0
    for kw in (dict(B=0), dict(B=65536), dict(S=0), dict(S=33), dict(C=1), dict(C=33), dict(h0=0), dict(w0=0), dict(H=0), dict(W=0),
               dict(H=65537), dict(w0=65537), dict(C=32, H=16384, W=8192), dict(B=65535, h0=65536, w0=2)):
        assert ws(*dict(ok, **kw).values()) == 0, kw


def test_every_listed_refusal_is_made_without_a_gpu(lib, codes):
    E = codes
    d, d2, d3, d4, d5, ws, big = 0x10000, 0x90000, 0x110000, 0x190000, 0x210000, 0x290000, 1 << 40   # never dereferenced

    def call(mean=d, pm=4, fac=d2, pf=12, labels=d3, B=2, S=4, C=4, R=3, h0=4, w0=6, H=16, W=24, ig=-1, ss=d4, ts=d5, w=ws, wn=big):
        return lib.vx_val_ssn2d_sums_batched(mean, pm, fac, pf, None, None, 1, 0, labels, B, S, C, R, h0, w0, H, W, 1e-5, ig, ss, ts, w, wn,
                                             None)

    def refused(rc, name, kw):
        assert rc == E[name], (rc, name, kw, lib.vx_last_error_string())

    for kw in (dict(mean=None), dict(fac=None), dict(labels=None), dict(ss=None), dict(ts=None), dict(w=None)):
        refused(call(**kw), E_NULL, kw)
    for kw in (dict(B=0), dict(B=65536), dict(S=0), dict(S=33), dict(C=1), dict(C=33), dict(R=-1), dict(R=33), dict(h0=0), dict(w0=0),
               dict(H=0), dict(W=0), dict(H=65537), dict(W=65537), dict(h0=65537), dict(w0=65537), dict(pm=3), dict(pf=11),
               dict(ig=-2), dict(ig=256), dict(C=32, pm=32, pf=96, H=16384, W=8192), dict(B=65535, h0=65536, w0=2)):
        refused(call(**kw), E_SHAPE, kw)
    need = lib.vx_val_ssn2d_sums_workspace_bytes(2, 4, 4, 4, 6, 16, 24)
    refused(call(wn=need - 1), E_WORKSPACE, dict(wn=need - 1))
    # R = 0 is mean_only: a null factor and any factor pitch are accepted up to the workspace check
    refused(call(fac=None, pf=0, R=0, wn=need - 1), E_WORKSPACE, "R = 0")
