"""STL meshes to occupancy volumes: the first step of the toy data generator (the reference's meshes_to_numpy,
datasets/toy_data_generation/stl_to_nifty.py:82-90, which calls numpy-stl and stl-to-voxel's convert_meshes).

Neither package is part of this project, so the rule is this project's own and is stated exactly: a voxel
is inside a mesh when the column below its sample point crosses the mesh an odd number of times; a point on an edge
belongs to the triangle on the positive side of the lexicographically ordered edge, so a closed mesh is crossed an even
number of times by every column, shared edges and vertices included.  All arithmetic is float64, one rounding per
operation.  Two routes to the same volume: the host mirror (`voxelize`, numpy) and the device (`voxelize_device`,
voxelize.hip), `==` to each other; tests pin the mirror to an exact-arithmetic restatement.

Not pinned: parity with stl-to-voxel 0.9.1 (absent).  That package paints the perimeter of each slice, so its surface
voxels are fatter and its shape may differ by one.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import re

import numpy as np

from . import _lib

MAX_MESHES = 16
MAX_DIM = 1024
MAX_TRIANGLES = 1 << 20


# ---------------------------------------------------------------------------------------------
# files

_REC = np.dtype([("normal", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")])


def read_stl(path):
    """-> float32 [n, 3, 3] (triangle, vertex, xyz).  Binary when len(file) == 84 + 50 n with n the uint32 at byte 80
    (checked first: a binary file may begin with `solid`); else ASCII: every `vertex x y z` line in order, any line
    ending.  Normals are ignored.  ValueError for anything else."""
    with open(path, "rb") as f:
        data = f.read()
    tris = None
    if len(data) >= 84:
        n = int(np.frombuffer(data, dtype="<u4", count=1, offset=80)[0])
        if len(data) == 84 + 50 * n:
            if n == 0:
                raise ValueError(f"{path}: binary STL with zero triangles")
            tris = np.frombuffer(data, dtype=_REC, count=n, offset=84)["v"].astype(np.float32)
    if tris is None:
        coords = []
        for line in re.split(rb"\r\n|\r|\n", data):
            parts = line.split()
            if parts and parts[0] == b"vertex":
                if len(parts) != 4:
                    raise ValueError(f"{path}: malformed vertex line {line[:60]!r}")
                try:
                    coords.append([float(p) for p in parts[1:]])
                except ValueError:
                    raise ValueError(f"{path}: malformed vertex line {line[:60]!r}") from None
        if not coords:
            raise ValueError(f"{path}: neither a binary STL (84 + 50 n bytes) nor an ASCII one with vertex lines")
        if len(coords) % 3:
            raise ValueError(f"{path}: {len(coords)} vertices are not a whole number of triangles")
        with np.errstate(over="ignore"):
            tris = np.asarray(coords, dtype=np.float64).astype(np.float32).reshape(-1, 3, 3)
    if not np.isfinite(tris).all():
        raise ValueError(f"{path}: non-finite coordinate")
    return np.ascontiguousarray(tris)


def write_stl_binary(path, tris, header=b""):
    """The binary form of float32 [n, 3, 3] triangles: 80 header bytes, the count, 50-byte records with zero normals."""
    tris = np.ascontiguousarray(tris, dtype=np.float32)
    if tris.ndim != 3 or tris.shape[1:] != (3, 3):
        raise ValueError("write_stl_binary: triangles are [n, 3, 3]")
    rec = np.zeros(len(tris), dtype=_REC)
    rec["v"] = tris
    with open(path, "wb") as f:
        f.write(bytes(header)[:80].ljust(80, b"\0"))
        f.write(np.uint32(len(tris)).astype("<u4").tobytes())
        f.write(rec.tobytes())


# ---------------------------------------------------------------------------------------------
# the grid

def _check_meshes(meshes):
    meshes = [np.ascontiguousarray(m, dtype=np.float32) for m in meshes]
    if not 1 <= len(meshes) <= MAX_MESHES:
        raise ValueError(f"1..{MAX_MESHES} meshes, not {len(meshes)}")
    for m in meshes:
        if m.ndim != 3 or m.shape[1:] != (3, 3) or len(m) == 0:
            raise ValueError("a mesh is a non-empty float32 [n, 3, 3] array")
        if not np.isfinite(m).all():
            raise ValueError("non-finite coordinate")
    if sum(len(m) for m in meshes) > MAX_TRIANGLES:
        raise ValueError(f"more than {MAX_TRIANGLES} triangles")
    return meshes


def _box(meshes):
    mn = np.min([m.reshape(-1, 3).astype(np.float64).min(axis=0) for m in meshes], axis=0)
    mx = np.max([m.reshape(-1, 3).astype(np.float64).max(axis=0) for m in meshes], axis=0)
    return mn, mx


def _grid_of_box(mn, mx, resolution):
    resolution = int(resolution)
    if resolution < 1:
        raise ValueError("resolution >= 1")
    bb = mx - mn
    L = float(bb.max())
    if L == 0:
        raise ValueError("the meshes have no extent")
    h = L / resolution
    dims = np.zeros(3, dtype=np.int64)
    origin = np.zeros(3, dtype=np.float64)
    for a in range(3):
        n = min(resolution, max(1, int(np.ceil(bb[a] / L * resolution))))
        dims[a] = n
        origin[a] = mn[a] - (n * h - bb[a]) / 2
    if dims.max() > MAX_DIM:
        raise ValueError(f"more than {MAX_DIM} voxels on an axis")
    return origin, np.float64(h), dims


def voxel_grid(meshes, resolution):
    """-> (origin_xyz float64[3], h float64, dims_xyz int[3]).  The longest axis of the meshes' common box gets
    `resolution` voxels of edge h = L / resolution; a shorter axis gets ceil(bb / L * resolution) of them, centred."""
    return _grid_of_box(*_box(_check_meshes(meshes)), resolution)


def sample_points(origin, h, n):
    """c(t) = origin + (t + 0.5) * h in float64, in that order"""
    return np.float64(origin) + (np.arange(int(n), dtype=np.float64) + 0.5) * np.float64(h)


# ---------------------------------------------------------------------------------------------
# the host mirror

def _lex_less(a, b):
    return bool(a[0] < b[0] or (a[0] == b[0] and a[1] < b[1]))


def _canon(a, b):
    """the edge (a, b) on its lexicographically ordered endpoints -> (p, q, swapped)"""
    return (a, b, False) if _lex_less(a, b) else (b, a, True)


def triangle_setup(tri):
    """tri float64 [3, 3] -> None when its projected area is 0, else (edges, z): edges = three (px, py, dx, dy, m) for
    (v1, v2), (v2, v0), (v0, v1) with dx = q.x - p.x, dy = q.y - p.y and m = orient * (swapped ? -1 : +1)."""
    v0, v1, v2 = tri
    p, q, swapped = _canon(v0, v1)
    area = (q[0] - p[0]) * (v2[1] - p[1]) - (q[1] - p[1]) * (v2[0] - p[0])
    if swapped:
        area = -area
    if area == 0:
        return None
    orient = 1.0 if area > 0 else -1.0
    edges = []
    for a, b in ((v1, v2), (v2, v0), (v0, v1)):
        p, q, swapped = _canon(a, b)
        edges.append((p[0], p[1], q[0] - p[0], q[1] - p[1], -orient if swapped else orient))
    return edges, (v0[2], v1[2], v2[2])


def _mesh_inside(tris, cx, cy, cz):
    """one mesh -> (inside bool [nz, ny, nx], number of columns hit an odd number of times)"""
    nz, ny, nx = len(cz), len(cy), len(cx)
    toggles = np.zeros((nz + 1, ny, nx), dtype=np.uint8)   # bit at the first k with c_z(k) > z_hit; row nz: above all
    count = np.zeros((ny, nx), dtype=np.int64)
    for tri in tris.astype(np.float64):
        setup = triangle_setup(tri)
        if setup is None:
            continue
        edges, z = setup
        # a column outside the triangle's closed xy box is never hit (in exact arithmetic the coverage test implies it;
        # stating it keeps the culling of the device route exact under rounding too)
        i0, i1 = np.searchsorted(cx, tri[:, 0].min(), "left"), np.searchsorted(cx, tri[:, 0].max(), "right")
        j0, j1 = np.searchsorted(cy, tri[:, 1].min(), "left"), np.searchsorted(cy, tri[:, 1].max(), "right")
        if i0 >= i1 or j0 >= j1:
            continue
        sx, sy = cx[None, i0:i1], cy[j0:j1, None]
        w = []
        ok = np.ones((j1 - j0, i1 - i0), dtype=bool)
        for px, py, dx, dy, m in edges:
            ec = dx * (sy - py) - dy * (sx - px)
            we = ec * m
            ok &= (we > 0) | ((we == 0) & (m > 0))
            w.append(we)
        if not ok.any():
            continue
        jj, ii = np.nonzero(ok)
        w0, w1, w2 = (we[jj, ii] for we in w)
        with np.errstate(invalid="ignore", divide="ignore"):
            z_hit = ((w0 * z[0] + w1 * z[1]) + w2 * z[2]) / ((w0 + w1) + w2)
        k0 = np.searchsorted(cz, z_hit, "right")            # the first k with z_hit < c_z(k); NaN: none
        toggles[k0, jj + j0, ii + i0] ^= 1
        count[jj + j0, ii + i0] += 1
    inside = np.bitwise_xor.accumulate(toggles[:nz], axis=0).astype(bool)
    return inside, int((count & 1).sum())


def voxelize_info(meshes, resolution):
    """-> (float32 volume [n_z, n_y, n_x], odd_columns): voxels inside mesh i take the value i + 1, later meshes
    overwrite earlier ones; odd_columns is the number of (mesh, column) pairs hit an odd number of times (0 for closed
    meshes)."""
    meshes = _check_meshes(meshes)
    origin, h, dims = _grid_of_box(*_box(meshes), resolution)
    cx, cy, cz = (sample_points(origin[a], h, dims[a]) for a in range(3))
    vol = np.zeros((int(dims[2]), int(dims[1]), int(dims[0])), dtype=np.float32)
    odd = 0
    for index, tris in enumerate(meshes):
        inside, n_odd = _mesh_inside(tris, cx, cy, cz)
        vol[inside] = index + 1
        odd += n_odd
    return vol, odd


def _strict(odd, strict):
    if strict and odd:
        raise ValueError(f"{odd} (mesh, column) pairs are crossed an odd number of times: an open or self-inconsistent mesh")


def voxelize(meshes, resolution, strict=True):
    """The host mirror -> float32 [n_z, n_y, n_x], the axis order convert_meshes returns."""
    vol, odd = voxelize_info(meshes, resolution)
    _strict(odd, strict)
    return vol


# ---------------------------------------------------------------------------------------------
# the device route

class MeshObject:
    """object_fn(resolution) of generate_toy_dataset / plan_samples for a set of meshes, read once.  The host route
    returns the mirror's numpy volume, the device route voxelize_device's tensor; the device copy of the triangles is
    made once per device and kept here."""

    def __init__(self, meshes, device_io=False, strict=True):
        self.meshes = _check_meshes(meshes)
        self.device_io = bool(device_io)
        self.strict = bool(strict)
        self.offsets = np.concatenate([[0], np.cumsum([len(m) for m in self.meshes])]).astype(np.int64)
        self.box = _box(self.meshes)
        self._device_tris = {}

    def device_triangles(self, dev):
        key = str(dev)
        if key not in self._device_tris:
            import torch
            self._device_tris[key] = torch.from_numpy(np.concatenate(self.meshes, axis=0)).to(dev)
        return self._device_tris[key]

    def __call__(self, resolution):
        if self.device_io:
            return voxelize_device(self, resolution, self.strict)
        return voxelize(self.meshes, resolution, self.strict)


def voxelize_device_info(meshes, resolution, device=None, out=None, odd=None):
    """-> (float32 device tensor [n_z, n_y, n_x], int64 device tensor (1,) odd_columns); no sync.  `meshes`: a
    MeshObject (its device triangles are reused) or a list of [n, 3, 3] arrays."""
    import torch
    _lib.require_gpu()
    obj = meshes if isinstance(meshes, MeshObject) else MeshObject(meshes)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    origin, h, dims = _grid_of_box(*obj.box, resolution)
    zyx = [int(dims[2]), int(dims[1]), int(dims[0])]
    tris = obj.device_triangles(dev)
    out = torch.empty(zyx, dtype=torch.float32, device=dev) if out is None else out
    odd = torch.empty(1, dtype=torch.int64, device=dev) if odd is None else odd
    _lib.check(_lib.load().vx_voxelize_meshes(_lib.ptr(tris), (C.c_int64 * len(obj.offsets))(*obj.offsets.tolist()), len(obj.meshes),
                                              (C.c_double * 3)(*origin.tolist()), float(h), (C.c_int32 * 3)(*zyx), _lib.ptr(out),
                                              _lib.ptr(odd), _lib.stream_ptr()), "vx_voxelize_meshes")
    return out, odd


def voxelize_device(meshes, resolution, strict=True, device=None):
    """voxelize on the device -> float32 device tensor, `==` to the mirror.  The odd_columns download is its one sync."""
    out, odd = voxelize_device_info(meshes, resolution, device)
    _strict(int(odd.cpu()[0]), strict)
    return out


def mesh_object(input_files, device_io=False, strict=True):
    """-> object_fn(resolution) over the STL files, the reference's meshes_to_numpy(input_files, resolution)"""
    return MeshObject([read_stl(f) for f in input_files], device_io, strict)


# ---------------------------------------------------------------------------------------------
# the reference's JSON configs (dataset_generation.py:126-141; absent keys take the argparse defaults there)

_CONFIG_DEFAULTS = {"n_samples": 10, "image_size": [256], "min_object_ratio": 10, "max_object_ratio": 2, "gauss_sigma": 8,
                    "object_gray": False, "blur": False, "noise": False, "segmentation": False, "all_raters_same": False,
                    "n_raters": 1, "object_over_border": False, "sample_offset": 0, "seed": 22}


def _resolve(name, dirs):
    if os.path.isabs(name) and os.path.isfile(name):
        return name
    for d in dirs:
        if os.path.isfile(os.path.join(d, name)):
            return os.path.join(d, name)
    raise FileNotFoundError(f"{name}: not found in {', '.join(dirs)}")


def generate_toy_dataset_from_config(json_config, save_path=None, mesh_dir=None, device_io=False, **overrides):
    """generate_toy_dataset from one of the reference's JSON configs.  save_path (and any keyword) overrides the config's
    value; input_files are looked up in mesh_dir, by default the config's directory, then its parent, and are written
    to dataset_info_<k>.json as the config has them."""
    from .toydata import generate_toy_dataset
    with open(json_config, "rt") as f:
        cfg = json.load(f)
    unknown = set(cfg) - set(_CONFIG_DEFAULTS) - {"input_files", "save_path", "json_config"}
    if unknown:
        raise ValueError(f"{json_config}: unknown keys {sorted(unknown)}")
    args = dict(_CONFIG_DEFAULTS, **{k: v for k, v in cfg.items() if k in _CONFIG_DEFAULTS})
    unknown = set(overrides) - set(_CONFIG_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown arguments {sorted(unknown)}")
    args.update(overrides)
    save_path = cfg.get("save_path") if save_path is None else save_path
    if save_path is None:
        raise ValueError(f"{json_config}: no save_path")
    input_files = cfg.get("input_files")
    if not input_files:
        raise ValueError(f"{json_config}: no input_files")
    size = args["image_size"]
    size = [size] if np.isscalar(size) else list(size)
    if len(size) == 1:
        size = size * 3
    elif len(size) != 3:
        raise ValueError("Image size has to be exactly 1 or 3 values")
    args["image_size"] = tuple(int(s) for s in size)
    here = os.path.dirname(os.path.abspath(json_config))
    dirs = [str(mesh_dir)] if mesh_dir is not None else [here, os.path.dirname(here)]
    object_fn = mesh_object([_resolve(name, dirs) for name in input_files], device_io)
    generate_toy_dataset(str(save_path), object_fn=object_fn, input_files=input_files, device_io=device_io, **args)
