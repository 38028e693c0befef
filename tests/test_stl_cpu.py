"""The STL reader, the voxeliser's host mirror and its toy-generator surface, without a GPU (values_amd/stl.py, DESIGN
4.53): the two shipped meshes parse and are closed; the mirror is `==` to the exact-arithmetic restatement of the rule
(tests/voxel_ref.py); known voxel counts from an independent prototype of the rule; geometric bounds on the sphere;
two meshes and an open one; the toy generator fed from a reference config; the C ABI's refusals, all before any
device call; the host plan (values_amd/csrc/voxel_plan.h) in a stand-alone program under ASan / UBSan."""
import ctypes as C
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import voxel_ref as vr
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


# ---------------------------------------------------------------------------------------------
# the reader

def test_shipped_meshes_parse_and_are_closed():
    cube, sphere = vr.cube(), vr.sphere()
    assert cube.shape == (12, 3, 3) and sphere.shape == (960, 3, 3)
    assert cube.dtype == sphere.dtype == np.float32
    assert os.path.getsize(vr.CUBE) == 2211 and os.path.getsize(vr.SPHERE) == 169140
    assert b"\r\n" in open(vr.CUBE, "rb").read()          # the shipped files are CRLF
    assert vr.is_closed(cube) and vr.is_closed(sphere)
    assert set(np.unique(cube)) == {-1.0, 1.0}
    assert vr.is_closed(vr.bipyramid()) and vr.is_closed(vr.slab()) and not vr.is_closed(vr.open_cube())
    sub = vr.subdivided_sphere()
    assert sub.shape == (3840, 3, 3) and vr.is_closed(sub)


def test_ascii_to_binary_round_trip_and_solid_header(tmp_path):
    from values_amd.stl import read_stl, write_stl_binary
    for name, tris in (("cube", vr.cube()), ("sphere", vr.sphere())):
        path = str(tmp_path / (name + ".stl"))
        write_stl_binary(path, tris)
        assert os.path.getsize(path) == 84 + 50 * len(tris)
        assert np.array_equal(read_stl(path), tris)
    path = str(tmp_path / "solid.stl")
    write_stl_binary(path, vr.cube(), header=b"solid vertex 1 2 3\nvertex")   # a binary file that begins with `solid`
    assert open(path, "rb").read(5) == b"solid"
    assert np.array_equal(read_stl(path), vr.cube())
    # any line ending
    text = open(vr.CUBE, "rb").read()
    for k, eol in enumerate((b"\n", b"\r")):
        path = str(tmp_path / f"eol{k}.stl")
        open(path, "wb").write(text.replace(b"\r\n", eol))
        assert np.array_equal(read_stl(path), vr.cube())


def test_truncated_or_garbled_input_raises(tmp_path):
    from values_amd.stl import read_stl, write_stl_binary
    text = open(vr.CUBE, "rb").read()
    lines = text.split(b"\r\n")
    last_vertex = max(i for i, ln in enumerate(lines) if ln.strip().startswith(b"vertex"))
    binary = str(tmp_path / "b.stl")
    write_stl_binary(binary, vr.cube())
    blob = open(binary, "rb").read()
    nan = np.array(vr.cube())
    nan[3, 1, 2] = np.nan
    write_stl_binary(str(tmp_path / "nan.stl"), nan)
    cases = {
        "ascii_cut": b"\r\n".join(lines[:last_vertex]),                       # one vertex short of a triangle
        "ascii_bad_number": text.replace(b"vertex 1.000000 1.000000 1.000000", b"vertex 1.0 x 1.0", 1),
        "ascii_short_line": text.replace(b"vertex 1.000000 1.000000 1.000000", b"vertex 1.0 1.0", 1),
        "ascii_inf": text.replace(b"vertex 1.000000 1.000000 1.000000", b"vertex 1e999 1.0 1.0", 1),
        "binary_cut": blob[:-7],
        "binary_long": blob + b"\0",
        "binary_zero": blob[:80] + b"\0\0\0\0",
        "empty": b"",
        "garbage": bytes(range(256)) * 3,
        "no_vertices": b"solid x\r\nendsolid x\r\n",
    }
    for name, data in cases.items():
        path = str(tmp_path / (name + ".stl"))
        open(path, "wb").write(data)
        with pytest.raises(ValueError):
            read_stl(path)
    with pytest.raises(ValueError):
        read_stl(str(tmp_path / "nan.stl"))


# ---------------------------------------------------------------------------------------------
# the grid and the rule

def test_grid_is_the_stated_one():
    from values_amd.stl import voxel_grid
    origin, h, dims = voxel_grid([vr.sphere()], 13)
    assert origin[0] == -0.9999994933605194 and h == 0.15384615384615385 and list(dims) == [13, 13, 13]
    assert origin.dtype == np.float64
    for meshes, r in (([vr.sphere()], 13), ([vr.slab()], 10), ([vr.slab()], 16), ([vr.cube(), vr.half_sphere()], 24), ([vr.bipyramid()], 1)):
        origin, h, dims = voxel_grid(meshes, r)
        o2, h2, d2 = vr.grid(meshes, r)
        assert list(origin) == o2 and h == h2 and list(dims) == d2 and max(dims) == r
    assert list(voxel_grid([vr.slab()], 10)[2]) == [10, 5, 3]
    with pytest.raises(ValueError):
        voxel_grid([vr.cube()], 0)
    with pytest.raises(ValueError):
        voxel_grid([np.ones((2, 3, 3), np.float32)], 4)      # L == 0
    with pytest.raises(ValueError):
        voxel_grid([], 4)


EXACT_CASES = [("cube", 1), ("cube", 2), ("cube", 3), ("cube", 8), ("bipyramid", 4), ("bipyramid", 8), ("slab", 10), ("sphere", 7)]


@pytest.mark.parametrize("name,resolution", EXACT_CASES)
def test_mirror_equals_the_exact_restatement(name, resolution):
    mesh = getattr(vr, name)()
    want, want_odd = vr.exact_voxelize([mesh], resolution)
    got, odd = vr.mirror(name, [mesh], resolution)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want) and odd == want_odd == 0
    assert got.any()


def test_known_values_cube_and_slab():
    from values_amd.stl import voxelize
    for r in (1, 2, 3, 5, 8, 13, 16):
        vol = voxelize([vr.cube()], r)
        assert vol.shape == (r, r, r) and (vol == 1).all()
    for r, shape, n in ((10, (3, 5, 10), 150), (16, (5, 8, 16), 640)):
        vol, odd = vr.mirror("slab", [vr.slab()], r)
        assert vol.shape == shape and int(vol.sum()) == n == vol.size and odd == 0


@pytest.mark.parametrize("resolution,inside", [(3, 19), (7, 179), (13, 1141), (25, 8089), (32, 16912), (51, 68359)])
def test_known_values_sphere(resolution, inside):
    vol, odd = vr.mirror("sphere", [vr.sphere()], resolution)
    assert vol.shape == (resolution,) * 3 and odd == 0
    assert set(np.unique(vol)) <= {0.0, 1.0} and int(vol.sum()) == inside


@pytest.mark.parametrize("resolution,inside", [(4, 20), (8, 168), (16, 1360)])
def test_known_values_bipyramid_every_column_hit_twice(resolution, inside):
    from values_amd import stl
    mesh = vr.bipyramid()
    vol, odd = vr.mirror("bipyramid", [mesh], resolution)
    assert vol.shape == (resolution,) * 3 and int(vol.sum()) == inside and odd == 0
    # hits per column, straight from the setups: a vertex and a diagonal edge lie exactly on sample points
    origin, h, dims = stl.voxel_grid([mesh], resolution)
    cx, cy = stl.sample_points(origin[0], h, dims[0]), stl.sample_points(origin[1], h, dims[1])
    assert (0.25 in cx and 0.25 in cy) == (resolution == 4)       # the apexes' column is a sample point at 4
    hits = np.zeros((resolution, resolution), dtype=int)
    on_edge = 0
    for tri in mesh.astype(np.float64):
        edges, _ = stl.triangle_setup(tri)
        ok = np.ones_like(hits, dtype=bool)
        for px, py, dx, dy, m in edges:
            w = (dx * (cy[:, None] - py) - dy * (cx[None, :] - px)) * m
            ok &= (w > 0) | ((w == 0) & (m > 0))
            on_edge += int((w == 0).sum())
        hits += ok
    assert (hits == 2).all()
    assert on_edge >= 4 * resolution // 2       # the diagonal edges pass through sample points: the tie rule decides them


@pytest.mark.parametrize("resolution", [13, 32])
def test_sphere_geometry(resolution):
    from values_amd import stl
    sphere = vr.sphere()
    vol, _ = vr.mirror("sphere", [sphere], resolution)
    t = sphere.astype(np.float64)
    normal = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    plane = np.abs((normal * t[:, 0]).sum(axis=1)) / np.linalg.norm(normal, axis=1)
    r_in = plane.min()
    assert 0.9904 < r_in < 0.9905 and np.linalg.norm(t.reshape(-1, 3), axis=1).max() <= 1 + 1e-6   # float32 vertices of a unit sphere
    origin, h, dims = stl.voxel_grid([sphere], resolution)
    cx, cy, cz = (stl.sample_points(origin[a], h, dims[a]) for a in range(3))
    dist = np.sqrt(cz[:, None, None] ** 2 + cy[None, :, None] ** 2 + cx[None, None, :] ** 2)
    assert (vol[dist < r_in] == 1).all()
    assert (vol[dist > 1 + 1e-9] == 0).all()
    undecided = ((dist >= r_in) & (dist <= 1 + 1e-9)).mean()
    assert undecided <= 0.03, undecided
    # rays along x instead of z: coordinates permuted (x, y, z) -> (z, y, x), the result transposed back
    turned = stl.voxelize([np.ascontiguousarray(sphere[:, :, ::-1])], resolution)
    assert np.array_equal(turned.transpose(2, 1, 0), vol)
    for axis in range(3):
        assert np.array_equal(np.flip(vol, axis), vol)


def test_two_meshes_labels_and_overwrite_order():
    from values_amd.stl import voxelize
    cube, small = vr.cube(), vr.half_sphere()
    vol, odd = vr.mirror("cube+half", [cube, small], 12)
    alone = voxelize([small, np.asarray([[[-1, -1, -1], [1, 1, 1], [-1, -1, -1]]], np.float32)], 12)   # same box, zero-area second mesh
    assert odd == 0 and vol.shape == (12, 12, 12) and set(np.unique(vol)) == {1.0, 2.0}
    assert np.array_equal(vol == 2, alone == 1) and 0 < (vol == 2).sum() < vol.size
    swapped = voxelize([small, cube], 12)                      # the cube last: it overwrites the sphere everywhere
    assert (swapped == 2).all()


def test_open_cube_strict_and_count():
    from values_amd.stl import voxelize, voxelize_info
    mesh = vr.open_cube()
    with pytest.raises(ValueError, match="45"):
        voxelize([mesh], 9)
    vol, odd = voxelize_info([mesh], 9)
    want, want_odd = vr.exact_voxelize([mesh], 9)
    assert odd == want_odd == 45 and np.array_equal(vol, want)
    assert np.array_equal(voxelize([mesh], 9, strict=False), vol)


# ---------------------------------------------------------------------------------------------
# the toy generator

def test_plan_samples_replays_the_same_random_calls_with_a_mesh_object():
    from values_amd.stl import MeshObject, mesh_object, voxelize
    from values_amd.toydata import plan_samples
    fn = mesh_object([vr.SPHERE])
    assert isinstance(fn, MeshObject) and not fn.device_io and len(fn.meshes) == 1
    stand_in = lambda r: np.ones((r, r, r), dtype=np.float32)      # an equal-shaped numpy object
    for over_border in (False, True):
        got = plan_samples(fn, 4, (40, 40, 40), 5, 2, over_border, True, 16)
        state = random.getstate()
        want = plan_samples(stand_in, 4, (40, 40, 40), 5, 2, over_border, True, 16)
        assert random.getstate() == state
        for g, w in zip(got, want):
            assert isinstance(g["object"], np.ndarray) and g["object"].dtype == np.float32 and g["object"].shape == w["object"].shape
            assert {k: v for k, v in g.items() if k != "object"} == {k: v for k, v in w.items() if k != "object"}
            assert np.array_equal(g["object"], voxelize([vr.sphere()], g["object"].shape[0]))


def test_plan_samples_keeps_a_tensor_object_as_it_is():
    import torch
    from values_amd.toydata import plan_samples
    made = []

    def fn(r):
        made.append(torch.ones((r, r + 1, r + 2), dtype=torch.float32))
        return made[-1]
    plan = plan_samples(fn, 3, (30, 31, 32), 5, 2, False, False, 3)
    want = plan_samples(lambda r: np.ones((r, r + 1, r + 2), np.float32), 3, (30, 31, 32), 5, 2, False, False, 3)
    for item, t, w in zip(plan, made, want):
        assert item["object"] is t and item["offset"] == w["offset"]


REFERENCE_KEYS = ["json_config", "input_files", "save_path", "n_samples", "image_size", "min_object_ratio", "max_object_ratio",
                  "gauss_sigma", "object_gray", "blur", "noise", "segmentation", "all_raters_same", "n_raters",
                  "object_over_border", "sample_offset", "seed"]


def test_generate_from_the_case_1_config(tmp_path):
    from values_amd import generate_toy_dataset_from_config, nifti
    from values_amd.stl import voxelize
    from values_amd.toydata import embed, gaussian_blur, plan_samples
    cfg = json.load(open(vr.CASE_1_TRAIN))
    assert cfg["input_files"] == ["ballSphere.stl"] and cfg["n_samples"] == 2 and cfg["image_size"] == [64, 64, 64]
    save = str(tmp_path / "imagesTr")
    generate_toy_dataset_from_config(vr.CASE_1_TRAIN, save_path=save)          # the mesh lies in the config's parent directory
    names = sorted(os.listdir(save)) + sorted(os.listdir(os.path.join(save, "segmentation")))
    assert names == ["0000.nii.gz", "0001.nii.gz", "dataset_info_1.json", "segmentation"] + [f"000{i}_0{r}.nii.gz" for i in (0, 1) for r in (0, 1, 2)]
    info = json.load(open(os.path.join(save, "dataset_info_1.json")))
    assert list(info) == REFERENCE_KEYS
    assert info["input_files"] == ["ballSphere.stl"] and info["save_path"] == save and info["seed"] == 16 and info["n_raters"] == 3
    assert info["min_object_ratio"] == 5 and info["gauss_sigma"] == 2 and info["blur"] is True and info["noise"] is False
    assert info["object_gray"] is False and info["sample_offset"] == 0        # absent keys: the argparse defaults
    plan = plan_samples(lambda r: voxelize([vr.sphere()], r), 2, (64, 64, 64), 5, 2, False, False, 16)
    for i, item in enumerate(plan):
        assert 12 <= item["object"].shape[0] <= 32
        image, _ = nifti.load(os.path.join(save, f"000{i}.nii.gz"))
        assert np.array_equal(image.transpose(2, 1, 0), gaussian_blur(embed(item), 2))
    # a config in a directory of its own with mesh_dir given; overrides; a missing mesh
    other = tmp_path / "cfg"
    other.mkdir()
    shutil.copy(vr.CASE_1_TRAIN, str(other / "c.json"))
    with pytest.raises(FileNotFoundError):
        generate_toy_dataset_from_config(str(other / "c.json"), save_path=str(tmp_path / "x"))
    generate_toy_dataset_from_config(str(other / "c.json"), save_path=str(tmp_path / "y"), mesh_dir=vr.STL_DIR, n_samples=1, blur=False,
                                     segmentation=False, image_size=[32])
    info = json.load(open(str(tmp_path / "y" / "dataset_info_1.json")))
    assert info["n_samples"] == 1 and info["image_size"] == [32, 32, 32] and sorted(os.listdir(str(tmp_path / "y"))) == ["0000.nii.gz", "dataset_info_1.json"]
    with pytest.raises(TypeError):
        generate_toy_dataset_from_config(str(other / "c.json"), save_path=str(tmp_path / "z"), mesh_dir=vr.STL_DIR, object_fn=None)


def test_device_route_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from values_amd import _lib
    from values_amd.stl import mesh_object, voxelize_device
    with pytest.raises(_lib.VxError):
        voxelize_device([vr.cube()], 4)
    with pytest.raises(_lib.VxError):
        mesh_object([vr.CUBE], device_io=True)(4)


# ---------------------------------------------------------------------------------------------
# the C ABI

A, B, W = 0x10000, 0x4000000, 0x8000000   # made-up device addresses: every call below is refused before anything looks at them


def test_symbol_is_bound(lib):
    from values_amd import _lib
    header = open(os.path.join(ROOT, "include", "values_amd.h")).read()
    assert hasattr(lib, "vx_voxelize_meshes") and "vx_voxelize_meshes" in _lib.SIGNATURES and "vx_voxelize_meshes" in header
    assert "K44" in header


def test_refusals_without_a_gpu(lib):
    def call(tris=A, off=(0, 12), n_meshes=None, origin=(-1.0, -1.0, -1.0), h=0.1, dims=(9, 9, 9), out=B, odd=W):
        off_arr = None if off is None else (C.c_int64 * len(off))(*off)
        org = None if origin is None else (C.c_double * 3)(*origin)
        d = None if dims is None else (C.c_int32 * 3)(*dims)
        return lib.vx_voxelize_meshes(tris, off_arr, len(off) - 1 if n_meshes is None else n_meshes, org, h, d, out, odd, None)
    many = tuple(range(0, 18 * 5, 5))
    cases = [(E_NULL, dict(tris=None)), (E_NULL, dict(off=None, n_meshes=1)), (E_NULL, dict(origin=None)), (E_NULL, dict(dims=None)),
             (E_NULL, dict(out=None)), (E_NULL, dict(odd=None)),
             (E_SHAPE, dict(n_meshes=0)), (E_SHAPE, dict(off=many, n_meshes=17)), (E_SHAPE, dict(n_meshes=-1)),
             (E_SHAPE, dict(dims=(0, 9, 9))), (E_SHAPE, dict(dims=(9, 1025, 9))), (E_SHAPE, dict(dims=(9, 9, -1))),
             (E_SHAPE, dict(off=(0, 0))), (E_SHAPE, dict(off=(0, (1 << 20) + 1))), (E_SHAPE, dict(off=(1, 12))),
             (E_SHAPE, dict(off=(0, 12, 12))), (E_SHAPE, dict(off=(0, 12, 5))),
             (E_SHAPE, dict(h=0.0)), (E_SHAPE, dict(h=-0.5)), (E_SHAPE, dict(h=float("nan"))), (E_SHAPE, dict(h=float("inf"))),
             (E_SHAPE, dict(origin=(0.0, float("inf"), 0.0))),
             (E_ALIGN, dict(tris=A + 2)), (E_ALIGN, dict(out=B + 1)), (E_ALIGN, dict(odd=W + 4))]
    for k, (code, kw) in enumerate(cases):
        assert call(**kw) == code, (k, lib.vx_last_error_string())
        assert lib.vx_last_error_string().startswith(b"vx_voxelize_meshes")


# ---------------------------------------------------------------------------------------------
# the host plan under sanitizers: a stand-alone program, no sanitizer runtime in this process

def test_host_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "voxel_plan_host")
    build_host_program(os.path.join(ROOT, "tests", "voxel_plan_host.cpp"), exe)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "BAD-" not in res.stdout
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in res.stdout.splitlines()}
    codes = {k: v[0] for k, v in rows.items() if not k.startswith("v_dim")}
    want = {"v_ok": 0, "v_two": 0, "v_max": 0, "v_m16": 0, "v_tri_max": 0, "v_hmin": 0, "v_align4_ok": 0,
            "v_m17": E_SHAPE, "v_m0": E_SHAPE, "v_mneg": E_SHAPE, "v_tri_over": E_SHAPE, "v_tri_zero": E_SHAPE, "v_off_from1": E_SHAPE,
            "v_off_flat": E_SHAPE, "v_off_back": E_SHAPE, "v_off_neg": E_SHAPE, "v_h0": E_SHAPE, "v_hneg": E_SHAPE, "v_hnan": E_SHAPE,
            "v_hinf": E_SHAPE, "v_org_nan": E_SHAPE, "v_null_tris": E_NULL, "v_null_off": E_NULL, "v_null_org": E_NULL,
            "v_null_dims": E_NULL, "v_null_out": E_NULL, "v_null_odd": E_NULL, "v_align_tris": E_ALIGN, "v_align_out": E_ALIGN,
            "v_align_odd": E_ALIGN}
    assert codes == want
    # [tiles_x, tiles_y, mask words, triangles, steps]: a tile is a row of 64 columns, a word 64 k, a step 256 triangles of ONE mesh
    assert rows["v_ok"][1:] == [2, 70, 2, 12, 1] and rows["v_two"][1:] == [2, 70, 2, 972, 1 + 4]
    assert rows["v_max"][1:] == [16, 1024, 16, 12, 1] and rows["v_tri_max"][4:] == [1 << 20, 1 << 12]
    for a in range(3):
        for v in (0, 1025):
            assert rows[f"v_dim{a}_{v}"] == [E_SHAPE]
    for v, words in ((1, 1), (64, 1), (65, 2), (128, 2), (129, 3), (1024, 16)):
        assert rows[f"v_dim0_{v}"][3] == words
    for v, tiles in ((1, 1), (4, 4), (5, 5), (63, 63), (1024, 1024)):
        assert rows[f"v_dim1_{v}"][2] == tiles
    for v, tiles in ((1, 1), (64, 1), (65, 2), (1023, 16), (1024, 16)):
        assert rows[f"v_dim2_{v}"][1] == tiles
