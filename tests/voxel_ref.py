"""Test-side restatement of the voxeliser's rule (values_amd/stl.py) in exact rational arithmetic on the
float64 sample points, written from the statement of the rule and sharing no code with the product, and the meshes
the tests are run on."""
import os
from fractions import Fraction

import numpy as np

STL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stl")
CUBE = os.path.join(STL_DIR, "Cube.stl")
SPHERE = os.path.join(STL_DIR, "ballSphere.stl")
CASE_1_TRAIN = os.path.join(STL_DIR, "Case_1", "train.json")   # Case_1/train.json cut to 2 samples

_cache = {}


def cube():
    from values_amd.stl import read_stl
    if "cube" not in _cache:
        _cache["cube"] = read_stl(CUBE)
    return _cache["cube"].copy()


def sphere():
    from values_amd.stl import read_stl
    if "sphere" not in _cache:
        _cache["sphere"] = read_stl(SPHERE)
    return _cache["sphere"].copy()


def bipyramid():
    """apexes (0.25, 0.25, +-1) over the square (+-1, +-1, 0): at resolution 4, 8 and 16 a vertex and a diagonal edge
    lie exactly on sample points"""
    base = [(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)]
    top, bottom = (0.25, 0.25, 1), (0.25, 0.25, -1)
    tris = []
    for i in range(4):
        a, b = base[i], base[(i + 1) % 4]
        tris.append([a, b, top])
        tris.append([b, a, bottom])
    return np.asarray(tris, dtype=np.float32)


def slab():
    return (cube().astype(np.float64) * np.array([1.0, 0.5, 0.26])).astype(np.float32)


def subdivided(tris):
    """one midpoint subdivision in float32: every triangle into four, shared edges get the same midpoint"""
    t = np.asarray(tris, dtype=np.float32)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    mid = lambda u, v: ((u + v) * np.float32(0.5)).astype(np.float32)   # u + v commutes: both sides of an edge agree
    ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
    out = np.stack([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1), np.stack([ab, bc, ca], 1)], 1)
    return np.ascontiguousarray(out.reshape(-1, 3, 3))


def subdivided_sphere():
    if "sub" not in _cache:
        _cache["sub"] = subdivided(sphere())
    return _cache["sub"].copy()


def open_cube():
    return cube()[1:].copy()


def half_sphere():
    return (sphere() * np.float32(0.5)).astype(np.float32)


def is_closed(tris):
    """every directed edge is matched exactly once by its reverse"""
    edges = {}
    for t in np.asarray(tris):
        v = [tuple(float(c) for c in p) for p in t]
        for a, b in ((v[0], v[1]), (v[1], v[2]), (v[2], v[0])):
            edges[(a, b)] = edges.get((a, b), 0) + 1
    return all(n == 1 and edges.get((b, a), 0) == 1 for (a, b), n in edges.items())


# ---------------------------------------------------------------------------------------------
# the rule in exact arithmetic

def grid(meshes, resolution):
    """the grid as the rule states it, in float64"""
    pts = np.concatenate([np.asarray(m, dtype=np.float32).reshape(-1, 3) for m in meshes]).astype(np.float64)
    mn, mx = pts.min(axis=0), pts.max(axis=0)
    bb = mx - mn
    L = bb.max()
    h = L / resolution
    dims, origin = [], []
    for a in range(3):
        n = min(resolution, max(1, int(np.ceil(bb[a] / L * resolution))))
        dims.append(n)
        origin.append(mn[a] - (n * h - bb[a]) / 2)
    return origin, h, dims


def _points(origin, h, n):
    return [float(np.float64(origin) + (np.float64(t) + 0.5) * np.float64(h)) for t in range(n)]


def _edge(a, b, s):
    """(E_c on the ordered endpoints at s, swapped)"""
    swapped = not ((a[0], a[1]) < (b[0], b[1]))
    p, q = (b, a) if swapped else (a, b)
    return (q[0] - p[0]) * (s[1] - p[1]) - (q[1] - p[1]) * (s[0] - p[0]), swapped


def exact_voxelize(meshes, resolution):
    """-> (float32 [n_z, n_y, n_x], odd_columns) with every edge function, weight and hit depth a Fraction"""
    origin, h, dims = grid(meshes, resolution)
    cx, cy, cz = (_points(origin[a], h, dims[a]) for a in range(3))
    fz = [Fraction(c) for c in cz]
    vol = np.zeros((dims[2], dims[1], dims[0]), dtype=np.float32)
    odd = 0
    for index, mesh in enumerate(meshes):
        hits = np.zeros(vol.shape, dtype=np.int64)
        total = np.zeros(vol.shape[1:], dtype=np.int64)
        for tri in np.asarray(mesh, dtype=np.float32):
            v = [[Fraction(float(c)) for c in p] for p in tri]
            area, swapped = _edge(v[0], v[1], v[2])
            area = -area if swapped else area
            if area == 0:
                continue
            orient = 1 if area > 0 else -1
            xs, ys = [float(p[0]) for p in tri], [float(p[1]) for p in tri]
            for j, y in enumerate(cy):
                if y < min(ys) or y > max(ys):
                    continue   # exact comparisons: outside the box is outside the triangle
                for i, x in enumerate(cx):
                    if x < min(xs) or x > max(xs):
                        continue
                    s = (Fraction(x), Fraction(y))
                    w = []
                    for a, b in ((v[1], v[2]), (v[2], v[0]), (v[0], v[1])):
                        ec, sw = _edge(a, b, s)
                        m = orient * (-1 if sw else 1)
                        we = ec * m
                        if not (we > 0 or (we == 0 and m > 0)):
                            break
                        w.append(we)
                    else:
                        z_hit = (w[0] * v[0][2] + w[1] * v[1][2] + w[2] * v[2][2]) / (w[0] + w[1] + w[2])
                        total[j, i] += 1
                        for k in range(dims[2]):
                            if z_hit < fz[k]:
                                hits[k, j, i] += 1
        vol[(hits & 1) == 1] = index + 1
        odd += int((total & 1).sum())
    return vol, odd


_mirror = {}


def mirror(name, meshes, resolution):
    """the host mirror's (volume, odd_columns), computed once per case and shared; never modified"""
    from values_amd.stl import voxelize_info
    key = (name, resolution)
    if key not in _mirror:
        vol, odd = voxelize_info(meshes, resolution)
        vol.setflags(write=False)
        _mirror[key] = (vol, odd)
    return _mirror[key]
