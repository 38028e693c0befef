"""CPU: vx_train_patches_3d is declared, exported and bound, its item struct has the C size and field offsets, the flag
constants agree with the header, and the refusals its declaration lists are made by host-side checks -- so a wrong call is
refused on a box without a GPU too (the full list runs in tests/test_train3d_plan_cpu.py and, with real buffers, in
tests/test_gpu_trainpatches3d.py)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vx_train_patches_3d_workspace_bytes", "vx_train_patches_3d")
FIELDS = ("image", "label", "image_kind", "label_kind", "label_flags", "dims", "origin", "flags", "index")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from values_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


@pytest.fixture(scope="module")
def c_view():
    """(VX_E_* codes, flag constants, sizeof, field offsets) as the header defines them"""
    names = ["VX_E_NULL", "VX_E_SHAPE", "VX_E_ALIGN", "VX_E_DTYPE", "VX_E_WORKSPACE", "VX_TRAIN3D_MIRROR0", "VX_TRAIN3D_MIRROR1",
             "VX_TRAIN3D_MIRROR2", "VX_TRAIN3D_NOISE", "VX_LABEL_SIGNED", "VX_SELECT_MAX_ITEMS"]
    exprs = names + ["(int)sizeof(vx_train3d_item)"] + [f"(int)offsetof(vx_train3d_item, {f})" for f in FIELDS]
    code = "#include <stdio.h>\n#include <stddef.h>\n#include \"values_amd.h\"\nint main(void){" + \
        "".join(f"printf(\"%d\\n\", {e});" for e in exprs) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])  # the header is plain C
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    return dict(zip(names, got)), got[len(names)], got[len(names) + 1:]


def test_symbols_are_declared_exported_and_bound(lib):
    from values_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "values_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vx_[a-zA-Z0-9_]+)\s*\(", hdr))
    for n in NEW:
        assert n in declared and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert len(_lib.SIGNATURES["vx_train_patches_3d"][1]) == 18
    mk = open(os.path.join(ROOT, "values_amd", "csrc", "Makefile")).read()
    assert "train_patches3d.hip" in mk and "train3d_plan.h" in mk


def test_item_struct_and_constants_match_c(c_view):
    from values_amd import _lib
    consts, size, offsets = c_view
    assert C.sizeof(_lib.Train3dItem) == size == 64
    assert [getattr(_lib.Train3dItem, f).offset for f in FIELDS] == offsets
    assert (_lib.VX_TRAIN3D_MIRROR0, _lib.VX_TRAIN3D_MIRROR1, _lib.VX_TRAIN3D_MIRROR2, _lib.VX_TRAIN3D_NOISE, _lib.VX_LABEL_SIGNED) == \
        tuple(consts[k] for k in ("VX_TRAIN3D_MIRROR0", "VX_TRAIN3D_MIRROR1", "VX_TRAIN3D_MIRROR2", "VX_TRAIN3D_NOISE", "VX_LABEL_SIGNED"))


def test_refusals_are_made_without_a_gpu(lib, c_view):
    from values_amd import _lib
    E, _, _ = c_view
    img, lab, data, seg, sig, st, ws, big = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 1 << 20
    assert lib.vx_train_patches_3d_workspace_bytes(0) == 0 and lib.vx_train_patches_3d_workspace_bytes(E["VX_SELECT_MAX_ITEMS"] + 1) == 0
    assert lib.vx_train_patches_3d_workspace_bytes(3) >= 3 * 64

    def call(n=1, P=(4, 4, 4), table=True, data=data, seg=seg, seg_u8=0, var=(0.0, 0.1), law=0, sig=sig, st=st, ws=ws, ws_n=big, **fields):
        arr = (_lib.Train3dItem * 1)()
        it = arr[0]
        it.image, it.label, it.image_kind, it.label_kind, it.flags = img, lab, _lib.VX_PREP_F32, _lib.VX_COUNT_B2, 5
        for a in range(3):
            it.dims[a], it.origin[a] = 8, 4
        for k, v in fields.items():
            if k in ("dims", "origin"):
                for a in range(3):
                    getattr(it, k)[a] = v[a]
            else:
                setattr(it, k, v)
        return lib.vx_train_patches_3d(arr if table else None, n, P[0], P[1], P[2], data, seg, seg_u8, 1, None, var[0], var[1], law, sig,
                                       st, ws, ws_n, None)

    cases = [("VX_E_NULL", dict(table=False)), ("VX_E_NULL", dict(data=None)), ("VX_E_NULL", dict(st=None)), ("VX_E_NULL", dict(ws=None)),
             ("VX_E_NULL", dict(image=None)),
             ("VX_E_SHAPE", dict(n=0)), ("VX_E_SHAPE", dict(n=65537)), ("VX_E_SHAPE", dict(P=(4, 0, 4))), ("VX_E_SHAPE", dict(dims=(8, 0, 8))),
             ("VX_E_SHAPE", dict(origin=(4, 4, 5))), ("VX_E_SHAPE", dict(origin=(-1, 4, 4))), ("VX_E_SHAPE", dict(P=(9, 4, 4), origin=(0, 0, 0))),
             ("VX_E_SHAPE", dict(P=(1 << 11, 1 << 11, 1 << 10))), ("VX_E_SHAPE", dict(var=(-1.0, 0.1))), ("VX_E_SHAPE", dict(var=(0.2, 0.1))),
             ("VX_E_DTYPE", dict(image_kind=8)), ("VX_E_DTYPE", dict(label_kind=4)), ("VX_E_DTYPE", dict(flags=16)),
             ("VX_E_DTYPE", dict(label_flags=2)), ("VX_E_DTYPE", dict(law=2)),
             ("VX_E_ALIGN", dict(data=data + 2)), ("VX_E_ALIGN", dict(seg=seg + 2)), ("VX_E_ALIGN", dict(sig=sig + 2)),
             ("VX_E_ALIGN", dict(st=st + 2)), ("VX_E_ALIGN", dict(image=img + 2)), ("VX_E_ALIGN", dict(label=lab + 1)),
             ("VX_E_ALIGN", dict(ws=ws + 8)), ("VX_E_WORKSPACE", dict(ws_n=lib.vx_train_patches_3d_workspace_bytes(1) - 1))]
    for name, kw in cases:
        rc = call(**kw)
        assert rc == E[name], (rc, name, kw, lib.vx_last_error_string())
        assert lib.vx_last_error_string().startswith(b"vx_train_patches_3d"), lib.vx_last_error_string()
