"""GPU: vx_train_patches_3d (train_patches3d.hip), the fused crop / mirror / noise / cast batch of the 3D loaders.

Exact throughout: without noise the outputs are numpy's src[crop][flips].astype(float32) (and the label's astype(intc) as
float32 or its low byte); with noise they are bit-equal to vx_noise_view_3d over the same call's noise-free output with
index0 = item.index (the kernels share one expression, gauss.h).  Every output lives between guard bands.

Shape matrix: the patch shapes PATCHES x the volumes VOLUMES (+ one equal to the patch) x origins {0, 1, 2, 3, dim - P} per
axis x all eight mirror masks x every VX_PREP_* image kind x every label kind, signed and unsigned, x both seg forms --
rows off the access's phase, ragged ends and the reversed vector path.  A call takes one patch shape, so the matrix is one
call per patch shape and seg form, its items cycling through the rest so that every value of every factor and every
(z origin, mask) pair occurs."""
import ctypes as C
import functools
import itertools
import os
import re

import numpy as np
import pytest
import torch

from values_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = b"vx_train_patches_3d"
OK, E_NULL, E_SHAPE, E_DTYPE, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
GUARD = 64
PATCHES = [(1, 1, 1), (2, 3, 1), (3, 5, 6), (4, 4, 4), (5, 5, 5), (7, 2, 9), (8, 8, 8)]
VOLUMES = [(9, 7, 13), (8, 8, 8), (5, 6, 21)]
IMAGE_KINDS = [("uint8", _lib.VX_PREP_U8), ("int8", _lib.VX_PREP_I8), ("uint16", _lib.VX_PREP_U16), ("int16", _lib.VX_PREP_I16),
               ("uint32", _lib.VX_PREP_U32), ("int32", _lib.VX_PREP_I32), ("float32", _lib.VX_PREP_F32), ("float64", _lib.VX_PREP_F64)]
LABEL_KINDS = [("uint8", _lib.VX_COUNT_B1, 0), ("int8", _lib.VX_COUNT_B1, 1), ("uint16", _lib.VX_COUNT_B2, 0), ("int16", _lib.VX_COUNT_B2, 1),
               ("uint32", _lib.VX_COUNT_B4, 0), ("int32", _lib.VX_COUNT_B4, 1), ("uint64", _lib.VX_COUNT_B8, 0), ("int64", _lib.VX_COUNT_B8, 1)]


def _image(shape, dtype, tag=0):
    rs = np.random.RandomState(1000 + tag + sum(shape))
    if dtype == "float64":
        return rs.standard_normal(shape) * 3.0                     # full mantissas: the float32 cast rounds
    if dtype == "float32":
        return (rs.standard_normal(shape) * 3.0).astype(np.float32)
    info = np.iinfo(dtype)
    return rs.randint(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dtype)   # 32-bit kinds pass 2^24: rounding


def _label(shape, dtype, tag=0):
    return np.random.RandomState(2000 + tag + sum(shape)).randint(0, 101, size=shape).astype(dtype)


class _Out:
    """a device array between two guard bands of sentinel bytes"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape)) * self.dtype.itemsize
        self.buf = torch.full((self.n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.p = C.c_void_p(self.buf.data_ptr() + GUARD)

    def get(self):
        raw = self.buf.cpu().numpy()
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + self.n:] == 0xA5).all(), "guard band written"
        return raw[GUARD:GUARD + self.n].copy().view(self.dtype).reshape(self.shape)

    def untouched(self):
        return bool((self.buf == 0xA5).all().item())


class _Sources:
    """the device copies of the arrays items point into (kept alive for the module)"""

    def __init__(self):
        self.t = {}

    def dev(self, a):
        key = id(a)
        if key not in self.t:
            h = np.ascontiguousarray(a)
            signed = {np.dtype("uint16"): np.int16, np.dtype("uint32"): np.int32, np.dtype("uint64"): np.int64}
            h = h.view(signed[h.dtype]) if h.dtype in signed else h          # (torch moves bytes; the kind says how to read them)
            self.t[key] = (a, torch.from_numpy(h).cuda())
        return self.t[key][1]


SRC = _Sources()


def _item(image, kind, origin, flags=0, index=0, label=None, lkind=0, lsigned=0):
    return dict(image=image, kind=kind, origin=tuple(origin), flags=flags, index=index, label=label, lkind=lkind, lsigned=lsigned)


def _table(items):
    arr = (_lib.Train3dItem * max(len(items), 1))()
    for it, d in zip(arr, items):
        it.image, it.image_kind = SRC.dev(d["image"]).data_ptr(), d["kind"]
        if d["label"] is not None:
            it.label, it.label_kind, it.label_flags = SRC.dev(d["label"]).data_ptr(), d["lkind"], _lib.VX_LABEL_SIGNED if d["lsigned"] else 0
        for a in range(3):
            it.dims[a], it.origin[a] = d["image"].shape[a], d["origin"][a]
        it.flags, it.index = d["flags"], d["index"]
    return arr


def _seed_word(k):
    return None if k is None else torch.from_numpy(np.array([k], dtype=np.uint32).view(np.int32)).cuda()


def _run(items, P, seg_u8=0, seed=0, seed_word=None, var=(0.0, 0.1), law=0, want_seg=True):
    """-> data (n, P0, P1, P2) float32, seg (float32 | uint8) or None, sigma (n,), status (n,)"""
    lib = _lib.load()
    n = len(items)
    data, sigma, status = _Out((n,) + tuple(P), np.float32), _Out((n,), np.float32), _Out((n,), np.int32)
    seg = _Out((n,) + tuple(P), np.uint8 if seg_u8 else np.float32) if want_seg else None
    ws = torch.empty(int(lib.vx_train_patches_3d_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    word = _seed_word(seed_word)
    _lib.check(lib.vx_train_patches_3d(_table(items), n, P[0], P[1], P[2], data.p, seg.p if seg else None, seg_u8, seed, _lib.ptr(word),
                                       var[0], var[1], law, sigma.p, status.p, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "vx_train_patches_3d")
    torch.cuda.synchronize()
    return data.get(), (seg.get() if seg else None), sigma.get(), status.get()


def _crop(a, origin, P, flags):
    v = a[tuple(slice(o, o + p) for o, p in zip(origin, P))]
    for ax in range(3):
        if flags >> ax & 1:
            v = np.flip(v, ax)
    return v


def _want(items, P, seg_u8):
    data = np.stack([_crop(d["image"], d["origin"], P, d["flags"]).astype(np.float32) for d in items])
    seg = np.stack([np.zeros(P, np.intc) if d["label"] is None else _crop(d["label"], d["origin"], P, d["flags"]).astype(np.intc)
                    for d in items])
    return data, seg.astype(np.uint8) if seg_u8 else seg.astype(np.float32)


def _origins(dim, p):
    return sorted({o for o in (0, 1, 2, 3, dim - p) if 0 <= o <= dim - p})


@functools.lru_cache(maxsize=None)
def _matrix_items(P):
    """the items of one patch shape: every volume that holds the patch (and one equal to it), all (z origin, mask) pairs,
    the x / y origins, image kinds and label kinds cycling underneath with strides that visit every value (callers copy
    an item before changing it)"""
    items, k = [], 0
    for vi, shape in enumerate(VOLUMES + [tuple(P)]):
        if any(d < p for d, p in zip(shape, P)):
            continue
        images = [_image(shape, name, vi) for name, _ in IMAGE_KINDS]
        labels = [_label(shape, name, vi) for name, _, _ in LABEL_KINDS]
        ox, oy, oz = (_origins(d, p) for d, p in zip(shape, P))
        pairs = list(itertools.product(oz, range(8)))
        for rep in range(-(-64 // len(pairs))):          # >= 64 items a volume: every (mask, image kind) and (mask, label kind) pair
            for z, mask in pairs:                        # (mask == k % 8: the pairs come z-major, eight masks a z)
                ik, lk = (k + k // 8) % 8, (k // 8 + k // 64) % 8
                lab = None if k % 23 == 22 else labels[lk]
                items.append(_item(images[ik], IMAGE_KINDS[ik][1], (ox[k % len(ox)], oy[(k // 3) % len(oy)], z), mask, k,
                                   lab, LABEL_KINDS[lk][1], LABEL_KINDS[lk][2]))
                k += 1
    return items


def test_matrix_covers_every_factor():
    for P in PATCHES:
        items = _matrix_items(P)
        assert {d["kind"] for d in items} == set(range(8)) and {d["flags"] for d in items} == set(range(8))
        assert {(d["lkind"], d["lsigned"]) for d in items if d["label"] is not None} == {(k, s) for _, k, s in LABEL_KINDS}
        assert any(d["label"] is None for d in items) and any(d["image"].shape == tuple(P) for d in items)
        for shape in {d["image"].shape for d in items}:
            got = {(d["origin"][2], d["flags"]) for d in items if d["image"].shape == shape}
            assert got == set(itertools.product(_origins(shape[2], P[2]), range(8)))
            for ax in range(2):
                assert {d["origin"][ax] for d in items if d["image"].shape == shape} == set(_origins(shape[ax], P[ax]))


@pytest.mark.parametrize("seg_u8", [0, 1])
@pytest.mark.parametrize("P", PATCHES, ids=lambda p: "x".join(map(str, p)))
def test_noise_off_equals_numpy(P, seg_u8):
    items = _matrix_items(P)
    data, seg, sigma, status = _run(items, P, seg_u8)
    want_data, want_seg = _want(items, P, seg_u8)
    assert data.tobytes() == want_data.tobytes()
    assert seg.dtype == want_seg.dtype and seg.tobytes() == want_seg.tobytes()
    assert not status.any() and not sigma.any()


@pytest.mark.parametrize("P", PATCHES, ids=lambda p: "x".join(map(str, p)))
def test_without_mirror_bytes_equal_gather_patches_3d(P):
    lib = _lib.load()
    items = [dict(d, flags=0) for d in _matrix_items(P)]
    n = len(items)
    data = _run(items, P, want_seg=False)[0]
    arr = (_lib.Gather3dItem * n)()
    for it, d in zip(arr, items):
        it.src, it.kind = SRC.dev(d["image"]).data_ptr(), d["kind"]
        for a in range(3):
            it.dims[a], it.origin[a] = d["image"].shape[a], d["origin"][a]
    out = _Out((n,) + tuple(P), np.float32)
    ws = torch.empty(int(lib.vx_gather_patches_3d_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.vx_gather_patches_3d(arr, n, out.p, P[0], P[1], P[2], _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "vx_gather_patches_3d")
    assert out.get().tobytes() == data.tobytes()


def _nine(P=(5, 5, 5)):
    """nine mixed items: three volumes, kinds, masks, labels; items 0 and 8 are the same crop under the same index"""
    items = _matrix_items(P)
    pick = [items[i] for i in (0, 9, 18, 27, 85, 100, 150, 170)]
    pick = [dict(d, index=7 * i + 3) for i, d in enumerate(pick)]
    return pick + [dict(pick[0])]


def _noise_view(x, seed, seed_word, index, var, law):
    """vx_noise_view_3d over one patch -> (view, sigma)"""
    lib = _lib.load()
    src = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out, sig = _Out(x.shape, np.float32), _Out((1,), np.float32)
    word = _seed_word(seed_word)
    _lib.check(lib.vx_noise_view_3d(_lib.ptr(src), out.p, 1, x.size, seed, _lib.ptr(word), index, var[0], var[1], law, sig.p,
                                    _lib.stream_ptr()), "vx_noise_view_3d")
    torch.cuda.synchronize()
    return out.get(), sig.get()[0]


@pytest.mark.parametrize("law", [0, 1])
def test_noise_on_is_noise_view_3d_of_the_noise_free_output(law):
    P, seed, word, var = (5, 5, 5), 11, 6, (0.0, 0.1)
    clean = _nine(P)
    noisy = [dict(d, flags=d["flags"] | 8) if i != 4 else d for i, d in enumerate(clean)]       # item 4 stays noise-free
    x, seg0, _, _ = _run(clean, P, 0, seed, word, var, law)
    y, seg1, sigma, status = _run(noisy, P, 0, seed, word, var, law)
    assert seg0.tobytes() == seg1.tobytes() and not status.any()
    for i, d in enumerate(noisy):
        if i == 4:
            assert y[i].tobytes() == x[i].tobytes() and sigma[i] == 0
            continue
        view, sg = _noise_view(x[i], seed, word, d["index"], var, law)
        assert y[i].tobytes() == view.tobytes(), i
        assert sigma[i].tobytes() == sg.tobytes() and sg > 0
    fields = y - x
    assert not np.array_equal(fields[0], fields[1])                       # different indices, different fields
    assert y[0].tobytes() == y[8].tobytes()                               # the same index, the same field, at any position


def test_device_seed_word_is_added_to_the_seed():
    P = (4, 4, 4)
    items = [dict(d, flags=d["flags"] | 8) for d in _matrix_items(P)[:6]]
    a = _run(items, P, seed=5, seed_word=3)
    b = _run(items, P, seed=8)
    c = _run(items, P, seed=5)
    d = _run(items, P, seed=0xFFFFFFFF, seed_word=9)
    assert a[0].tobytes() == b[0].tobytes() == d[0].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert a[0].tobytes() != c[0].tobytes()


@pytest.mark.parametrize("seg_u8", [0, 1])
def test_batch_independence_nine_items_together_and_alone(seg_u8):
    P = (5, 5, 5)
    items = [dict(d, flags=d["flags"] | (8 if i % 2 else 0)) for i, d in enumerate(_nine(P))]
    data, seg, sigma, status = _run(items, P, seg_u8, seed=21)
    for i, d in enumerate(items):
        one = _run([d], P, seg_u8, seed=21)
        assert one[0][0].tobytes() == data[i].tobytes() and one[1][0].tobytes() == seg[i].tobytes(), i
        assert one[2][0] == sigma[i] and one[3][0] == status[i]


def _grid_cap():
    src = open(os.path.join(ROOT, "values_amd", "csrc", "train3d_plan.h")).read()
    return int(re.search(r"#define T3_MAX_GRID (\d+)", src).group(1)), int(re.search(r"#define T3_THREADS (\d+)", src).group(1))


def test_second_trip_of_the_grid_stride_loop():
    grid, threads = _grid_cap()
    P = (32, 32, 32)
    per = P[0] * P[1] * ((P[2] + 3) // 4)                                 # lanes of an item
    n = grid * threads // per + 1                                         # the smallest batch of this patch past the cap
    assert (n - 1) * per <= grid * threads < n * per
    image, label = _image((33, 32, 35), "float32", 77), _label((33, 32, 35), "uint8", 77)
    items = [_item(image, _lib.VX_PREP_F32, (i % 2, 0, i % 4), i % 8, i, label, _lib.VX_COUNT_B1, 0) for i in range(n)]
    data, seg, _, status = _run(items, P, 1)
    want_data, want_seg = _want(items, P, 1)
    assert data.tobytes() == want_data.tobytes() and seg.tobytes() == want_seg.tobytes() and not status.any()


def test_status_counts_labels_outside_0_255():
    P, shape = (4, 5, 6), (6, 7, 9)
    rs = np.random.RandomState(5)
    base = rs.randint(0, 256, size=shape).astype(np.int64)
    where = rs.randint(0, 6, size=shape)
    l64 = base.copy()
    l64[where == 0], l64[where == 1], l64[where == 2] = 256, -1, 1 << 40
    l16 = base.astype(np.int16)
    l16[where == 0], l16[where == 1] = 256, -1
    l8 = (base % 100).astype(np.int8)
    l8[where == 1] = -1
    image = _image(shape, "float32", 5)
    cases = [(l64, _lib.VX_COUNT_B8, 1, l64), (l64, _lib.VX_COUNT_B8, 0, l64.view(np.uint64)), (l16, _lib.VX_COUNT_B2, 1, l16),
             (l16, _lib.VX_COUNT_B2, 0, l16.view(np.uint16)), (l8, _lib.VX_COUNT_B1, 1, l8), (l8, _lib.VX_COUNT_B1, 0, l8.view(np.uint8))]
    items, want_status, want_seg = [], [], []
    for i, (arr, kind, signed, read) in enumerate(cases):
        origin, flags = (i % 3, 2 - i % 3, i % 4), i
        items.append(_item(image, _lib.VX_PREP_F32, origin, flags, i, arr, kind, signed))
        crop = _crop(read, origin, P, flags)
        want_status.append(int(np.count_nonzero((crop < 0) | (crop > 255))))
        want_seg.append(crop.astype(np.intc))
    assert want_status[4] > 0 and want_status[5] == 0 and all(want_status[:4])   # a signed byte -1 read unsigned passes as 255
    for seg_u8 in (0, 1):
        _, seg, _, status = _run(items, P, seg_u8)
        assert status.tolist() == want_status
        want = np.stack(want_seg)
        assert seg.tobytes() == (want.astype(np.uint8) if seg_u8 else want.astype(np.float32)).tobytes()


def test_refusals_return_before_any_launch_and_write_nothing():
    lib = _lib.load()
    P = (4, 4, 4)
    image, label = _image((8, 8, 8), "float32", 9), _label((8, 8, 8), "uint16", 9)
    img64 = _image((8, 8, 8), "float64", 9)
    ok = _item(image, _lib.VX_PREP_F32, (4, 4, 4), 5, 0, label, _lib.VX_COUNT_B2, 0)
    data, seg, sigma, status = _Out((2,) + P, np.float32), _Out((2,) + P, np.float32), _Out((2,), np.float32), _Out((2,), np.int32)
    ws = torch.full((1 << 12,), 0xA5, dtype=torch.uint8, device="cuda")
    need = int(lib.vx_train_patches_3d_workspace_bytes(1))
    assert lib.vx_train_patches_3d_workspace_bytes(0) == 0 and lib.vx_train_patches_3d_workspace_bytes(65537) == 0 and need >= 64

    def off(p, k):
        return C.c_void_p(p.value + k)

    def call(items=(ok,), n=None, P=P, table=True, data_p=data.p, seg_p=seg.p, seg_u8=0, var=(0.0, 0.1), law=0, sigma_p=sigma.p,
             status_p=status.p, ws_p=C.c_void_p(ws.data_ptr()), ws_n=ws.numel(), patch=None):
        arr = _table(list(items))
        if patch:
            patch(arr)
        return lib.vx_train_patches_3d(arr if table else None, len(items) if n is None else n, P[0], P[1], P[2], data_p, seg_p, seg_u8, 3,
                                       None, var[0], var[1], law, sigma_p, status_p, ws_p, ws_n, _lib.stream_ptr())

    def field(name, value):
        return lambda arr: setattr(arr[0], name, value)

    refusals = [
        (E_NULL, dict(table=False)), (E_NULL, dict(data_p=None)), (E_NULL, dict(status_p=None)), (E_NULL, dict(ws_p=None)),
        (E_NULL, dict(patch=field("image", None))),
        (E_SHAPE, dict(n=0)), (E_SHAPE, dict(n=65537)), (E_SHAPE, dict(P=(4, 0, 4))), (E_SHAPE, dict(P=(1 << 11, 1 << 11, 1 << 10))),
        (E_SHAPE, dict(patch=lambda a: a[0].dims.__setitem__(1, 0))),
        (E_SHAPE, dict(items=(dict(ok, origin=(4, 4, 5)),))), (E_SHAPE, dict(items=(dict(ok, origin=(-1, 4, 4)),))),
        (E_SHAPE, dict(P=(9, 4, 4), items=(dict(ok, origin=(0, 0, 0)),))),
        (E_SHAPE, dict(var=(-0.1, 0.1))), (E_SHAPE, dict(var=(0.2, 0.1))),
        (E_DTYPE, dict(patch=field("image_kind", 8))), (E_DTYPE, dict(patch=field("image_kind", -1))),
        (E_DTYPE, dict(patch=field("label_kind", 4))), (E_DTYPE, dict(patch=field("flags", 16))),
        (E_DTYPE, dict(patch=field("label_flags", 2))), (E_DTYPE, dict(law=2)),
        (E_ALIGN, dict(data_p=off(data.p, 2))), (E_ALIGN, dict(seg_p=off(seg.p, 2))), (E_ALIGN, dict(sigma_p=off(sigma.p, 1))),
        (E_ALIGN, dict(status_p=off(status.p, 2))), (E_ALIGN, dict(ws_p=C.c_void_p(ws.data_ptr() + 8))),
        (E_ALIGN, dict(patch=lambda a: setattr(a[0], "image", SRC.dev(image).data_ptr() + 2))),
        (E_ALIGN, dict(patch=lambda a: setattr(a[0], "label", SRC.dev(label).data_ptr() + 1))),
        (E_ALIGN, dict(items=(_item(img64, _lib.VX_PREP_F64, (0, 0, 0)),), patch=lambda a: setattr(a[0], "image", SRC.dev(img64).data_ptr() + 4))),
        (E_WORKSPACE, dict(ws_n=need - 1)),
    ]
    for code, kw in refusals:
        rc = call(**kw)
        assert rc == code, (rc, code, kw, lib.vx_last_error_string())
        assert WHO in lib.vx_last_error_string(), lib.vx_last_error_string()
    torch.cuda.synchronize()
    assert data.untouched() and seg.untouched() and sigma.untouched() and status.untouched() and bool((ws == 0xA5).all().item())
    assert call(seg_p=off(seg.p, 1), seg_u8=1, items=(ok, ok)) == OK          # a byte seg needs no alignment
    torch.cuda.synchronize()
