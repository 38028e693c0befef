"""CPU: the three batched entry points of the validation step (vx_val_sums_batched, vx_val_aleatoric_sums_batched,
vx_val_ssn_sums_batched) and their workspace companions are declared, exported and bound, and every refusal the header
lists is made by a host-side check -- so a wrong call is refused on a box without a GPU too."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vx_val_sums_workspace_bytes", "vx_val_sums_batched", "vx_val_aleatoric_sums_workspace_bytes",
       "vx_val_aleatoric_sums_batched", "vx_val_ssn_sums_workspace_bytes", "vx_val_ssn_sums_batched")
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
    """the VX_E_* codes as the header defines them"""
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


def test_workspace_companions(lib):
    span = 256                                                                            # voxels of a workgroup's span
    assert lib.vx_val_sums_workspace_bytes(3, 19, 4097) == 3 * 17 * (5 * 19 + 3) * 8     # 17 spans
    assert lib.vx_val_aleatoric_sums_workspace_bytes(1, 2, span) == 13 * 8
    assert lib.vx_val_aleatoric_sums_workspace_bytes(1, 2, span + 1) == 2 * 13 * 8
    assert lib.vx_val_ssn_sums_workspace_bytes(2, 10, 2, 64 ** 3) == 2 * (64 ** 3 // span) * (10 * 5 + 4) * 8
    # 0 for what the calls refuse
    assert lib.vx_val_sums_workspace_bytes(0, 2, 10) == 0 and lib.vx_val_sums_workspace_bytes(1, 33, 10) == 0
    assert lib.vx_val_sums_workspace_bytes(1, 2, 0) == 0 and lib.vx_val_sums_workspace_bytes(65536, 2, 10) == 0
    assert lib.vx_val_aleatoric_sums_workspace_bytes(1, 1, 10) == 0 and lib.vx_val_aleatoric_sums_workspace_bytes(1, 9, 10) == 0
    assert lib.vx_val_aleatoric_sums_workspace_bytes(1, 2, 1 << 31) == 0
    assert lib.vx_val_ssn_sums_workspace_bytes(1, 0, 2, 10) == 0 and lib.vx_val_ssn_sums_workspace_bytes(1, 33, 2, 10) == 0


def test_every_listed_refusal_is_made_without_a_gpu(lib, codes):
    E = codes
    d, d2, d3, d4, ws, big = 0x10000, 0x90000, 0x110000, 0x190000, 0x210000, 1 << 30   # never dereferenced

    def refused(rc, name):
        assert rc == E[name], (rc, name, lib.vx_last_error_string())

    # ---- vx_val_sums_batched
    def plain(logits=d, labels=d2, B=2, C=3, nvox=100, ig=-1, sums=d3, w=ws, wn=big):
        return lib.vx_val_sums_batched(logits, labels, B, C, nvox, ig, sums, w, wn, None)

    for kw in (dict(logits=None), dict(labels=None), dict(sums=None), dict(w=None)):
        refused(plain(**kw), E_NULL)
    for kw in (dict(B=0), dict(B=65536), dict(C=0), dict(C=33), dict(nvox=0), dict(nvox=(1 << 39) + 1), dict(ig=-2), dict(ig=256)):
        refused(plain(**kw), E_SHAPE)
    refused(plain(wn=lib.vx_val_sums_workspace_bytes(2, 3, 100) - 1), E_WORKSPACE)

    # ---- vx_val_aleatoric_sums_batched
    def al(mu_s=d, eps=None, labels=d2, B=2, T=4, C=2, nvox=100, ig=-1, sums=d3, w=ws, wn=big):
        return lib.vx_val_aleatoric_sums_batched(mu_s, eps, 1, 0, labels, B, T, C, nvox, ig, sums, w, wn, None)

    for kw in (dict(mu_s=None), dict(labels=None), dict(sums=None), dict(w=None)):
        refused(al(**kw), E_NULL)
    for kw in (dict(B=0), dict(B=65536), dict(T=0), dict(T=33), dict(C=1), dict(C=9), dict(nvox=0), dict(nvox=1 << 31),
               dict(ig=-2), dict(ig=256)):
        refused(al(**kw), E_SHAPE)
    refused(al(wn=lib.vx_val_aleatoric_sums_workspace_bytes(2, 2, 100) - 1), E_WORKSPACE)

    # ---- vx_val_ssn_sums_batched
    def ssn(head=d, labels=d2, B=2, S=4, C=2, R=3, nvox=100, ig=-1, ss=d3, ts=d4, w=ws, wn=big):
        return lib.vx_val_ssn_sums_batched(head, None, None, 1, 0, labels, B, S, C, R, nvox, 1e-5, ig, ss, ts, w, wn, None)

    for kw in (dict(head=None), dict(labels=None), dict(ss=None), dict(ts=None), dict(w=None)):
        refused(ssn(**kw), E_NULL)
    for kw in (dict(B=0), dict(B=65536), dict(S=0), dict(S=33), dict(C=1), dict(C=9), dict(R=-1), dict(R=33), dict(nvox=0),
               dict(nvox=1 << 31), dict(ig=-2), dict(ig=256)):
        refused(ssn(**kw), E_SHAPE)
    refused(ssn(wn=lib.vx_val_ssn_sums_workspace_bytes(2, 4, 2, 100) - 1), E_WORKSPACE)
