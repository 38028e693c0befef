"""CPU: the three batched entry points of the 3D test split (vx_gather_patches_3d, vx_softmax_accumulate_cases,
vx_case_composite) are declared, exported and bound, their item structs have the C sizes, and every refusal their
declarations list is made by a host-side check -- so a wrong call is refused on a box without a GPU too."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vx_gather_patches_3d_workspace_bytes", "vx_gather_patches_3d", "vx_softmax_accumulate_cases_workspace_bytes",
       "vx_softmax_accumulate_cases", "vx_case_composite_workspace_bytes", "vx_case_composite")
E_NULL, E_SHAPE, E_ALIGN, E_DTYPE, E_WORKSPACE = "VX_E_NULL", "VX_E_SHAPE", "VX_E_ALIGN", "VX_E_DTYPE", "VX_E_WORKSPACE"


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
    names = [E_NULL, E_SHAPE, E_ALIGN, E_DTYPE, E_WORKSPACE]
    code = "#include <stdio.h>\n#include \"values_amd.h\"\nint main(void){printf(\"%d %d %d %d %d %zu %zu %zu %zu\\n\", " + \
        ", ".join(names) + ", sizeof(vx_gather3d_item), sizeof(vx_acc3d_item), sizeof(vx_composite_label), sizeof(vx_composite_item)); return 0;}\n"
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write(code)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])  # header is plain C
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    return dict(zip(names, got[:5])), got[5:]


def test_new_symbols_are_declared_exported_and_bound(lib):
    from values_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "values_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vx_[a-zA-Z0-9_]+)\s*\(", hdr))
    for n in NEW:
        assert n in declared and hasattr(lib, n) and n in _lib.SIGNATURES, n


def test_item_struct_sizes_match_c(codes):
    from values_amd import _lib
    _, sizes = codes
    mine = [C.sizeof(c) for c in (_lib.Gather3dItem, _lib.Acc3dItem, _lib.CompositeLabel, _lib.CompositeItem)]
    assert mine == sizes == [40, 40, 16, 64]


def test_every_listed_refusal_is_made_without_a_gpu(lib, codes):
    from values_amd import _lib
    E, _ = codes
    d, d2, big = 0x10000, 0x90000, 1 << 20       # never dereferenced: every call below is refused by a host-side check

    def refused(rc, name):
        assert rc == E[name], (rc, name, lib.vx_last_error_string())

    # ---- vx_gather_patches_3d
    assert lib.vx_gather_patches_3d_workspace_bytes(0) == 0 and lib.vx_gather_patches_3d_workspace_bytes(65537) == 0
    assert lib.vx_gather_patches_3d_workspace_bytes(3) >= 3 * 32

    def gather(items, n=None, out=d2, P=(4, 4, 4), ws=d, ws_n=big, table=True):
        arr = (_lib.Gather3dItem * max(len(items), 1))()
        for it, (src, kind, dims, origin) in zip(arr, items):
            it.src, it.kind = src, kind
            for a in range(3):
                it.dims[a], it.origin[a] = dims[a], origin[a]
        return lib.vx_gather_patches_3d(arr if table else None, len(items) if n is None else n, out, P[0], P[1], P[2], ws, ws_n, None)

    ok = (d, _lib.VX_PREP_F32, (8, 8, 8), (4, 4, 4))
    refused(gather([ok], table=False), E_NULL)
    refused(gather([ok], out=None), E_NULL)
    refused(gather([(None,) + ok[1:]]), E_NULL)
    refused(gather([ok], ws=None), E_NULL)
    refused(gather([ok], n=0), E_SHAPE)
    refused(gather([ok], n=65537), E_SHAPE)
    refused(gather([ok], P=(4, 0, 4)), E_SHAPE)
    refused(gather([(d, _lib.VX_PREP_F32, (8, 0, 8), (4, 0, 4))]), E_SHAPE)          # a dimension below 1
    refused(gather([(d, _lib.VX_PREP_F32, (8, 8, 8), (4, 4, 5))]), E_SHAPE)          # the crop ends past the volume
    refused(gather([(d, _lib.VX_PREP_F32, (8, 8, 8), (-1, 4, 4))]), E_SHAPE)         # ... or starts before it
    refused(gather([ok, (d, _lib.VX_PREP_F32, (3, 8, 8), (0, 0, 0))]), E_SHAPE)      # a volume smaller than the patch
    refused(gather([(d, 8, (8, 8, 8), (4, 4, 4))]), E_DTYPE)
    refused(gather([(d, -1, (8, 8, 8), (4, 4, 4))]), E_DTYPE)
    refused(gather([(d + 2, _lib.VX_PREP_F32, (8, 8, 8), (4, 4, 4))]), E_ALIGN)      # src off its 4-byte elements
    refused(gather([(d + 4, _lib.VX_PREP_F64, (8, 8, 8), (4, 4, 4))]), E_ALIGN)
    refused(gather([ok], out=d2 + 2), E_ALIGN)
    refused(gather([ok], ws=d + 8), E_ALIGN)
    refused(gather([ok], ws_n=lib.vx_gather_patches_3d_workspace_bytes(1) - 1), E_WORKSPACE)

    # ---- vx_softmax_accumulate_cases
    assert lib.vx_softmax_accumulate_cases_workspace_bytes(0) == 0 and lib.vx_softmax_accumulate_cases_workspace_bytes(2) >= 2 * 40

    def acc(items, B=None, T=3, Cn=2, P=(4, 4, 4), logits=d, overlap=0, ws=d2, ws_n=big, table=True):
        arr = (_lib.Acc3dItem * max(len(items), 1))()
        for it, (s, c, dims, origin) in zip(arr, items):
            it.sum, it.count = s, c
            for a in range(3):
                it.dims[a], it.origin[a] = dims[a], origin[a]
        return lib.vx_softmax_accumulate_cases(logits, len(items) if B is None else B, T, Cn, P[0], P[1], P[2], arr if table else None,
                                               overlap, ws, ws_n, None)

    s1, c1, s2, c2 = 0x100000, 0x200000, 0x300000, 0x400000
    a0 = (s1, c1, (8, 8, 8), (0, 0, 0))
    refused(acc([a0], logits=None), E_NULL)
    refused(acc([a0], table=False), E_NULL)
    refused(acc([(None, c1, (8, 8, 8), (0, 0, 0))]), E_NULL)
    refused(acc([(s1, None, (8, 8, 8), (0, 0, 0))]), E_NULL)
    refused(acc([a0], ws=None), E_NULL)
    refused(acc([a0], B=0), E_SHAPE)
    refused(acc([a0], B=65537), E_SHAPE)
    refused(acc([a0], T=0), E_SHAPE)
    refused(acc([a0], P=(4, 4, 0)), E_SHAPE)
    refused(acc([a0], Cn=1), E_SHAPE)
    refused(acc([a0], Cn=9), E_SHAPE)
    refused(acc([(s1, c1, (8, 0, 8), (0, 0, 0))]), E_SHAPE)
    refused(acc([(s1, c1, (8, 8, 8), (0, -4, 0))]), E_SHAPE)
    # two patches of one sum that share a voxel, without sum_overlap -- whatever lies between them in the table
    refused(acc([a0, (s2, c2, (8, 8, 8), (0, 0, 0)), (s1, c1, (8, 8, 8), (2, 2, 3))]), E_SHAPE)
    assert b"overlapping" in lib.vx_last_error_string()
    refused(acc([(s1, c1, (6, 6, 6), (0, 0, 0)), (s1, c1, (6, 6, 6), (3, 3, 3))]), E_SHAPE)   # boxes cut to the image still meet
    refused(acc([(s1 + 2, c1, (8, 8, 8), (0, 0, 0))]), E_ALIGN)
    refused(acc([(s1, c1 + 1, (8, 8, 8), (0, 0, 0))]), E_ALIGN)
    refused(acc([a0], logits=d + 2), E_ALIGN)
    refused(acc([a0], ws=d2 + 4), E_ALIGN)
    refused(acc([a0], ws_n=lib.vx_softmax_accumulate_cases_workspace_bytes(1) - 1), E_WORKSPACE)

    # ---- vx_case_composite
    assert lib.vx_case_composite_workspace_bytes(0, 0) == 0 and lib.vx_case_composite_workspace_bytes(1, -1) == 0
    assert lib.vx_case_composite_workspace_bytes(2, 3) >= 2 * 64 + 3 * 16

    def comp(items, labels=(), n=None, n_labels=None, status=d, ws=d2, ws_n=big, table=True, ltable=True):
        arr = (_lib.CompositeItem * max(len(items), 1))()
        for it, (image, kind, count, data, gt_seg, gt, first, R, dims) in zip(arr, items):
            it.image, it.image_kind, it.count, it.data, it.gt_seg, it.gt, it.first_label, it.R = image, kind, count, data, gt_seg, gt, first, R
            for a in range(3):
                it.dims[a] = dims[a]
        lab = (_lib.CompositeLabel * max(len(labels), 1))()
        for l, (p, kind) in zip(lab, labels):
            l.ptr, l.kind = p, kind
        return lib.vx_case_composite(arr if table else None, len(items) if n is None else n, lab if ltable else None,
                                     len(labels) if n_labels is None else n_labels, status, ws, ws_n, None)

    img, cnt, dat, gs, gt = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    lab1 = [(0x600000, _lib.VX_COUNT_B1)]
    it0 = (img, _lib.VX_PREP_F32, cnt, dat, gs, gt, 0, 1, (4, 4, 4))

    def item(**kw):
        f = dict(zip(("image", "kind", "count", "data", "gt_seg", "gt", "first", "R", "dims"), it0))
        f.update(kw)
        return tuple(f[k] for k in ("image", "kind", "count", "data", "gt_seg", "gt", "first", "R", "dims"))

    refused(comp([it0], lab1, table=False), E_NULL)
    refused(comp([it0], lab1, ltable=False), E_NULL)
    refused(comp([item(count=None)], lab1), E_NULL)
    refused(comp([item(image=None)], lab1), E_NULL)                      # data without an image
    refused(comp([it0], [(None, _lib.VX_COUNT_B1)]), E_NULL)
    refused(comp([it0], lab1, status=None), E_NULL)
    refused(comp([it0], lab1, ws=None), E_NULL)
    refused(comp([it0], lab1, n=0), E_SHAPE)
    refused(comp([it0], lab1, n=65537), E_SHAPE)
    refused(comp([it0], lab1, n_labels=-1), E_SHAPE)
    refused(comp([item(dims=(4, 0, 4))], lab1), E_SHAPE)
    refused(comp([item(dims=(1 << 14, 1 << 14, 1 << 14))], lab1), E_SHAPE)   # more than 2^40 voxels
    refused(comp([item(R=2)], lab1), E_SHAPE)                            # raters beyond the label table
    refused(comp([item(first=-1)], lab1), E_SHAPE)
    refused(comp([item(R=-1)], lab1), E_SHAPE)
    refused(comp([item(kind=9)], lab1), E_DTYPE)
    refused(comp([it0], [(0x600000, 4)]), E_DTYPE)                       # a float "label"
    refused(comp([item(image=img + 2)], lab1), E_ALIGN)
    refused(comp([item(count=cnt + 2)], lab1), E_ALIGN)
    refused(comp([item(data=dat + 4)], lab1), E_ALIGN)
    refused(comp([item(gt_seg=gs + 4)], lab1), E_ALIGN)
    refused(comp([it0], [(0x600002, _lib.VX_COUNT_B4)]), E_ALIGN)
    refused(comp([it0], lab1, ws=d2 + 8), E_ALIGN)
    refused(comp([it0], lab1, ws_n=lib.vx_case_composite_workspace_bytes(1, 1) - 1), E_WORKSPACE)
