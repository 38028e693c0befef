"""CPU: the host half of the 3D preprocessing (values_amd/preprocess.py) -- the mirror against a literal restatement of the
reference's loop body, the pad_sizes quirk, preprocess_dataset(device_io=False) on a tree written here -- and the C ABI of
the two batched kernels: symbols, struct sizes, every refusal with its code and the workspace queries, all before any
device call.  The host plan (values_amd/csrc/prep_plan.h) also runs in a stand-alone program under ASan / UBSan."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest
from tests.helpers import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_DTYPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from values_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def volume(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.standard_normal(shape) * 300 + 40).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(max(info.min, -1000), min(info.max, 3000), size=shape, endpoint=True).astype(dt)


def restated(image, labels, patch_size=64, patch_overlap=1):
    """preprocess_datasets_3d.py:135-168 with pad_nd_image written out as np.pad (below = diff // 2, above = the rest)"""
    def pad_nd(a, new_shape, value):
        new_shape = [max(n, s) for n, s in zip(new_shape, a.shape)]
        diff = [n - s for n, s in zip(new_shape, a.shape)]
        return np.pad(a, [[d // 2, d // 2 + d % 2] for d in diff], "constant", constant_values=value)
    image = (image - image.mean()) / (image.std() + 1e-8)
    pad_size_x = image.shape[0] + (image.shape[0] % int(patch_size * patch_overlap))
    pad_size_y = image.shape[1] + (image.shape[1] % int(patch_size * patch_overlap))
    pad_size_z = image.shape[2] + (image.shape[2] % int(patch_size * patch_overlap))
    image = pad_nd(image, (pad_size_x, pad_size_y, pad_size_z), image.min())
    out = []
    for rater in range(len(labels)):
        out.append(pad_nd(labels[rater], (pad_size_x, pad_size_y, pad_size_z), labels[rater].min()))
    return image, out


@pytest.mark.parametrize("shape,dtype", [((20, 17, 13), "int16"), ((33, 64, 5), "float32"), ((64, 64, 64), "float64"),
                                         ((70, 3, 129), "uint8")])
def test_host_mirror_equals_the_restatement(shape, dtype):
    from values_amd.preprocess import pad_sizes, preprocess_volume
    image = volume(shape, dtype, 3)
    labels = [(volume(shape, "uint8", 5) > 200).astype(np.uint8) + 1, (volume(shape, "int32", 6) % 3).astype(np.int32)]
    got, got_l = preprocess_volume(image, labels)
    want, want_l = restated(image, labels)
    assert got.dtype == want.dtype == (np.float32 if dtype == "float32" else np.float64)
    assert got.shape == want.shape == pad_sizes(shape)[0]
    assert np.array_equal(got, want)
    assert len(got_l) == 2
    for g, w, l in zip(got_l, want_l, labels):
        assert g.dtype == w.dtype == l.dtype and g.shape == w.shape == got.shape
        assert np.array_equal(g, w)
    # the padding carries the normalised minimum, the labels' padding their own (1 and 0)
    if got.shape != tuple(shape):
        mask = np.ones(got.shape, bool)
        mask[tuple(slice(b, b + s) for (b, _), s in zip(pad_sizes(shape)[1], shape))] = False
        assert (got[mask] == got[~mask].min()).all() and (got_l[0][mask] == 1).all()
    got2, _ = preprocess_volume(image, [], patch_size=32, patch_overlap=0.5)
    assert np.array_equal(got2, restated(image, [], 32, 0.5)[0])


def test_pad_sizes_is_the_reference_expression_not_a_round_up():
    from values_amd.preprocess import pad_sizes
    new, split = pad_sizes((64, 70, 100))
    assert new == (64, 76, 136) and split == [(0, 0), (3, 3), (18, 18)]
    assert pad_sizes((130,)) == ((132,), [(1, 1)])
    # int(32 * 0.5) = 16: 64 -> 64, 70 -> 76, 100 -> 104, 130 -> 132, and an odd difference puts the extra voxel above
    new, split = pad_sizes((64, 70, 100, 130), patch_size=32, patch_overlap=0.5)
    assert new == (64, 76, 104, 132) and split == [(0, 0), (3, 3), (2, 2), (1, 1)]
    assert pad_sizes((17, 5), patch_size=32, patch_overlap=0.5) == ((18, 10), [(0, 1), (2, 3)])
    with pytest.raises(ValueError):
        pad_sizes((4,), patch_size=1, patch_overlap=0.5)


def write_tree(root, lidc):
    """3 cases, 2 raters, one rater file missing -> {case id: (image, [labels that exist])}"""
    from values_amd import nifti
    os.makedirs(os.path.join(root, "imagesTr"))
    os.makedirs(os.path.join(root, "labelsTr"))
    cases = {}
    specs = [("case_b", (20, 17, 13), "int16"), ("case_a", (9, 12, 70), "float32"), ("case_c", (5, 4, 30), "uint8")]
    for k, (cid, shape, dt) in enumerate(specs):
        image = volume(shape, dt, 20 + k)
        nifti.save(image, os.path.join(root, "imagesTr", cid + ".nii.gz"))
        labels = []
        for r in range(2):
            if cid == "case_a" and r == 0:
                continue   # the missing rater: the one that remains is stored as rater 00
            lab = ((volume(shape, "int16", 40 + 2 * k + r) > 1500).astype(np.uint8 if r == 0 else np.int32) + (cid == "case_c"))
            name = f"{cid}_{r:02d}_mask.nii.gz" if lidc else f"{cid}_{r:02d}.nii.gz"
            nifti.save(lab, os.path.join(root, "labelsTr", name))
            labels.append(lab)
        cases[cid] = (image, labels)
    open(os.path.join(root, "imagesTr", "notes.txt"), "w").write("not a volume")
    return cases


@pytest.mark.parametrize("dataset", [None, "lidc", "lidc-idri", "toy"])
def test_preprocess_dataset_on_the_host(tmp_path, dataset):
    from values_amd import preprocess_dataset
    from values_amd.preprocess import npy_header, preprocess_volume
    lidc = dataset in ("lidc", "lidc-idri")
    root, save = str(tmp_path / "raw"), str(tmp_path / "out")
    cases = write_tree(root, lidc)
    preprocess_dataset(root, save, 2, image_dirs=["imagesTr"], label_dirs=["labelsTr"], dataset=dataset, patch_size=16,
                       patch_overlap=0.5)
    want_images = sorted(cid + ".npy" for cid in cases)
    want_labels = sorted(f"{cid}_{r:02d}{'_mask' if lidc else ''}.npy" for cid, (_, ls) in cases.items() for r in range(len(ls)))
    assert sorted(os.listdir(os.path.join(save, "preprocessed", "imagesTr"))) == want_images
    assert sorted(os.listdir(os.path.join(save, "preprocessed", "labelsTr"))) == want_labels
    assert len(want_labels) == 5
    for cid, (image, labels) in cases.items():
        mirror, mirror_l = preprocess_volume(image, labels, 16, 0.5)
        path = os.path.join(save, "preprocessed", "imagesTr", cid + ".npy")
        got = np.load(path)
        assert got.dtype == mirror.dtype and got.shape == mirror.shape and got.flags.c_contiguous
        assert got.shape == tuple(s + s % 8 for s in image.shape)
        assert np.array_equal(got, mirror)
        head = npy_header(got.shape, got.dtype)
        assert open(path, "rb").read(len(head)) == head
        for r, ml in enumerate(mirror_l):
            gl = np.load(os.path.join(save, "preprocessed", "labelsTr", f"{cid}_{r:02d}{'_mask' if lidc else ''}.npy"))
            assert gl.dtype == ml.dtype == labels[r].dtype and np.array_equal(gl, ml)


def test_npy_header_is_what_np_save_writes():
    from values_amd.preprocess import npy_header
    for shape, dt in (((3, 4, 5), "int16"), ((64, 76, 136), "float64"), ((1, 1, 1), "float32"), ((200, 300, 400), "uint8"),
                      ((7, 7, 7), "int32"), ((2, 2, 2), "bool")):
        f = io.BytesIO()
        np.save(f, np.zeros(shape, dt))
        head = npy_header(shape, dt)
        assert f.getvalue()[:len(head)] == head and len(f.getvalue()) == len(head) + np.zeros(shape, dt).nbytes


# ---------------------------------------------------------------------------------------------
# the C ABI

def test_new_symbols_are_bound_and_struct_sizes_match_c(lib, tmp_path):
    from values_amd import _lib
    for name in ("vx_volume_stats_batched", "vx_volume_stats_batched_workspace_bytes", "vx_zscore_pad_batched",
                 "vx_zscore_pad_batched_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert name in open(os.path.join(ROOT, "include", "values_amd.h")).read()
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "values_amd.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(vx_prep_item), sizeof(vx_prep_pad_item),'
                   ' offsetof(vx_prep_pad_item, pad_below), offsetof(vx_prep_pad_item, stats_row), VX_PREP_F64, VX_PREP_COPY, VX_PREP_OWN);'
                   ' return 0;}\n')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])   # the header is plain C
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(_lib.PrepItem), C.sizeof(_lib.PrepPadItem), _lib.PrepPadItem.pad_below.offset,
                   _lib.PrepPadItem.stats_row.offset, _lib.VX_PREP_F64, _lib.VX_PREP_COPY, _lib.VX_PREP_OWN]
    assert _lib.VX_SELECT_MAX_ITEMS == 65536
    assert lib.vx_version() >= 870


A, B = 0x10000, 0x4000000   # made-up device addresses: every call below is refused before anything looks at them


def stat_items(rows):
    from values_amd import _lib
    arr = (_lib.PrepItem * max(len(rows), 1))()
    for i, (p, n, kind) in enumerate(rows):
        arr[i].ptr, arr[i].n, arr[i].kind = p, n, kind
    return arr


def pad_items(rows):
    from values_amd import _lib
    arr = (_lib.PrepPadItem * max(len(rows), 1))()
    for i, r in enumerate(rows):
        it = arr[i]
        it.src, it.dst, it.kind = r.get("src", A), r.get("dst", B), r.get("kind", _lib.VX_PREP_I16)
        for a in range(3):
            it.dims[a], it.out_dims[a], it.pad_below[a] = r.get("dims", (2, 2, 2))[a], r.get("out", (2, 3, 2))[a], r.get("below", (0, 1, 0))[a]
        it.out_dtype, it.mode, it.stats_row = r.get("out_dtype", _lib.VX_F64), r.get("mode", _lib.VX_PREP_ZSCORE), r.get("row", 0)
    return arr


def test_volume_stats_refusals_without_a_gpu(lib):
    from values_amd import _lib
    ws, big = C.c_void_p(B), 1 << 30
    call = lambda arr, n, stats=C.c_void_p(A), w=ws, nb=big: lib.vx_volume_stats_batched(arr, n, stats, w, nb, None)
    ok = [(A, 4420, _lib.VX_PREP_I16)]
    cases = [
        (E_NULL, lambda: call(None, 1)),
        (E_SHAPE, lambda: call(stat_items(ok), -1)),
        (E_SHAPE, lambda: call(stat_items(ok), _lib.VX_SELECT_MAX_ITEMS + 1)),
        (E_SHAPE, lambda: call(stat_items([(A, 0, _lib.VX_PREP_I16)]), 1)),
        (E_SHAPE, lambda: call(stat_items([(A, -5, _lib.VX_PREP_I16)]), 1)),
        (E_SHAPE, lambda: call(stat_items([(A, (1 << 40) + 1, _lib.VX_PREP_U8)]), 1)),
        (E_DTYPE, lambda: call(stat_items([(A, 8, 8)]), 1)),
        (E_DTYPE, lambda: call(stat_items([(A, 8, -1)]), 1)),
        (E_NULL, lambda: call(stat_items([(None, 8, _lib.VX_PREP_U8)]), 1)),
        (E_NULL, lambda: call(stat_items(ok + [(None, 8, _lib.VX_PREP_U8)]), 2)),
        (E_ALIGN, lambda: call(stat_items([(A + 1, 8, _lib.VX_PREP_I16)]), 1)),
        (E_ALIGN, lambda: call(stat_items([(A + 4, 8, _lib.VX_PREP_F64)]), 1)),
        (E_NULL, lambda: call(stat_items(ok), 1, stats=None)),
        (E_NULL, lambda: call(stat_items(ok), 1, w=None)),
        (E_ALIGN, lambda: call(stat_items(ok), 1, w=C.c_void_p(B + 8))),
        (E_WORKSPACE, lambda: call(stat_items(ok), 1, nb=int(lib.vx_volume_stats_batched_workspace_bytes(stat_items(ok), 1)) - 1)),
    ]
    for k, (code, fn) in enumerate(cases):
        assert fn() == code, (k, lib.vx_last_error_string())
        assert lib.vx_last_error_string().startswith(b"vx_volume_stats_batched")
    assert call(None, 0) == 0   # an empty batch is a no-op
    q = lib.vx_volume_stats_batched_workspace_bytes
    assert q(stat_items(ok), 1) >= 256 + 32 and q(stat_items(ok), 1) % 256 == 0
    # one partial (32 bytes) per 32 KB work block: 64^3 float32 is 32 blocks, and the size depends on the items alone
    assert q(stat_items([(A, 64 ** 3, _lib.VX_PREP_F32)]), 1) - q(stat_items([(A, 8192, _lib.VX_PREP_F32)]), 1) == 31 * 32 // 256 * 256
    assert q(None, 1) == 0 and q(stat_items(ok), -1) == 0 and q(stat_items(ok), _lib.VX_SELECT_MAX_ITEMS + 1) == 0
    assert q(stat_items([(A, 0, _lib.VX_PREP_I16)]), 1) == 0 and q(stat_items([(A, 8, 8)]), 1) == 0
    assert q(stat_items([(None, 8, 0)]), 1) == 0 and q(stat_items([(A + 1, 8, _lib.VX_PREP_I16)]), 1) == 0
    assert q(None, 0) == 0


def test_zscore_pad_refusals_without_a_gpu(lib):
    from values_amd import _lib
    ws, big = C.c_void_p(B), 1 << 30
    call = lambda rows, n=None, stats=C.c_void_p(A), w=ws, nb=big, table=True: lib.vx_zscore_pad_batched(
        pad_items(rows) if table else None, len(rows) if n is None else n, stats, w, nb, None)
    q = lambda rows: int(lib.vx_zscore_pad_batched_workspace_bytes(pad_items(rows), len(rows)))
    refused = [
        (E_SHAPE, dict(out=(2, 2, 2), below=(0, 1, 0))),                 # out_dims < dims + pad_below
        (E_SHAPE, dict(out=(2, 3, 2), below=(0, -1, 0))),                # negative pad_below
        (E_SHAPE, dict(dims=(2, 0, 2))),
        (E_SHAPE, dict(out=(1 << 20, 1 << 20, 2), below=(0, 0, 0))),     # more than 2^40 output voxels
        (E_SHAPE, dict(row=-1)),
        (E_SHAPE, dict(row=_lib.VX_SELECT_MAX_ITEMS)),
        (E_SHAPE, dict(src=A, dst=A + 8)),                               # overlapping src / dst
        (E_SHAPE, dict(src=A + 64, dst=A)),
        (E_DTYPE, dict(kind=8)),
        (E_DTYPE, dict(mode=2)),
        (E_DTYPE, dict(out_dtype=2)),
        (E_DTYPE, dict(mode=_lib.VX_PREP_COPY, out_dtype=_lib.VX_F32)),  # COPY keeps the source's kind
        (E_NULL, dict(src=None)),
        (E_NULL, dict(dst=None)),
        (E_ALIGN, dict(src=A + 1)),
        (E_ALIGN, dict(dst=B + 4)),
        (E_ALIGN, dict(dst=B + 2, out_dtype=_lib.VX_F32)),
    ]
    for k, (code, row) in enumerate(refused):
        assert call([row]) == code, (k, row, lib.vx_last_error_string())
        assert call([{}, row]) == code, (k, row)
        assert q([row]) == 0 and q([{}, row]) == 0, (k, row)
    assert call([{}], table=False) == E_NULL
    assert call([{}], n=-1) == E_SHAPE and call([{}], n=_lib.VX_SELECT_MAX_ITEMS + 1) == E_SHAPE
    assert call([{}], stats=None) == E_NULL and call([{}], w=None) == E_NULL
    assert call([{}], w=C.c_void_p(B + 4)) == E_ALIGN
    assert call([{}], nb=q([{}]) - 1) == E_WORKSPACE
    assert call([], n=0, table=False) == 0
    assert q([{}]) > 0 and q([{}]) % 256 == 0
    assert q([dict(mode=_lib.VX_PREP_COPY, out_dtype=_lib.VX_PREP_OWN), dict(out_dtype=_lib.VX_PREP_OWN, src=A, dst=A + 16)]) > 0   # src and dst may touch
    assert lib.vx_zscore_pad_batched_workspace_bytes(None, 1) == 0 and lib.vx_zscore_pad_batched_workspace_bytes(None, 0) == 0


def test_device_entry_points_fail_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from values_amd import _lib, load_cases_device
    from values_amd.preprocess import preprocess_batch_device
    with pytest.raises(_lib.VxError):
        preprocess_batch_device([torch.zeros(2, 2, 2)])
    with pytest.raises(_lib.VxError):
        load_cases_device(["a.nii.gz"])


# ---------------------------------------------------------------------------------------------
# the host plan under sanitizers: a stand-alone program, no sanitizer runtime in this process

def test_host_plan_under_asan_ubsan(lib, tmp_path):
    from values_amd import _lib
    exe = str(tmp_path / "prep_plan_host")
    build_host_program(os.path.join(ROOT, "tests", "prep_plan_host.cpp"), exe)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "BAD-BLOCKS" not in res.stdout
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in res.stdout.splitlines()}
    codes = {k: v[0] for k, v in rows.items()}
    assert codes == {
        "s_empty": 0, "s_null": E_NULL, "s_count": E_SHAPE, "s_negative": E_SHAPE, "s_one": 0, "s_mixed": 0, "s_kind": E_DTYPE,
        "s_kind_neg": E_DTYPE, "s_n0": E_SHAPE, "s_nbig": E_SHAPE, "s_nullptr": E_NULL, "s_align": E_ALIGN, "s_max": 0,
        "p_empty": 0, "p_null": E_NULL, "p_count": E_SHAPE, "p_ok": 0, "p_kind": E_DTYPE, "p_mode": E_DTYPE, "p_out": E_DTYPE,
        "p_copy_out": E_DTYPE, "p_dim0": E_SHAPE, "p_fit": E_SHAPE, "p_below": E_SHAPE, "p_huge": E_SHAPE, "p_row": E_SHAPE,
        "p_nullptr": E_NULL, "p_src_align": E_ALIGN, "p_dst_align": E_ALIGN, "p_overlap": E_SHAPE, "p_touch": 0}
    blk = lambda nbytes: -(-nbytes // 32768)   # 32 KB work blocks, counted per item
    assert rows["s_one"][1] == 1 and rows["s_max"][1] == 65536
    assert rows["s_mixed"][1] == blk(4420 * 2) + blk(40 * 33 * 29 * 2) + blk(64 ** 3 * 4) + blk(2600) + blk(8 << 40)
    assert rows["p_ok"][1] == blk(40 * 34 * 26 * 8) + blk(40 * 34 * 26) + blk(64 ** 3 * 4)
    # the library (the same header, compiled without sanitizers) sizes the same workspace
    mixed = stat_items([(A, 4420, _lib.VX_PREP_I16), (B, 40 * 33 * 29, _lib.VX_PREP_I16), (B + 4, 64 ** 3, _lib.VX_PREP_F32),
                        (A + 1, 2600, _lib.VX_PREP_U8), (A, 1 << 40, _lib.VX_PREP_F64)])
    assert rows["s_mixed"][2] == lib.vx_volume_stats_batched_workspace_bytes(mixed, 5)
