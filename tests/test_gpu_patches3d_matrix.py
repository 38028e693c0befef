"""GPU: the float64 test matrix of the 3D test-split kernels -- vx_gather_patches_3d (K45), vx_softmax_accumulate_cases
(K46), vx_case_composite (K47) of patches3d.hip and vx_softmax_accumulate (K14, accumulate.hip) -- against the plain
numpy restatements of tests/patches3d_ref.py (held to the reference's fixtures by tests/test_patches3d_ref_cpu.py).
Raw ABI calls; every destination is carved out of a larger flat buffer at an element offset of 1 or 3, between guard
values that must come back untouched."""
import numpy as np
import pytest
import torch

from tests import patches3d_ref as pr

pytestmark = pytest.mark.gpu
GUARD = -7.0
GUARD8 = 0xAB


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _carve(shape, off, fill, dtype=torch.float32, guard=GUARD):
    """-> (flat, view): a contiguous `shape` view `off` elements into a flat buffer of guards, filled with `fill`"""
    n = int(np.prod(shape))
    flat = torch.full((off + n + 5,), guard, dtype=dtype, device="cuda")
    view = flat[off:off + n].view(shape)
    view.fill_(fill)
    return flat, view


def _guards_hold(flat, off, n, guard=GUARD):
    return bool((flat[:off] == guard).all()) and bool((flat[off + n:] == guard).all())


def _dev(a, off=1):
    """the bytes of the numpy array a on the device, `off` ELEMENTS into a fresh allocation (so the base has the alignment
    of its elements and no more) -> (tensor to keep alive, pointer).  Any dtype, the unsigned ones torch lacks too."""
    a = np.ascontiguousarray(a)
    es = a.dtype.itemsize
    host = np.zeros((off + a.size + 3) * es, dtype=np.uint8)
    host[off * es:(off + a.size) * es] = a.reshape(-1).view(np.uint8)
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + off * es


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# accumulate

def _run_accumulate(route, lg, dims, patches, overlap, fill):
    """logits lg (B, T, C, P0, P1, P2) added into fresh images of `dims` pre-filled with `fill` = (sum, count), through
    vx_softmax_accumulate_cases (one call) or vx_softmax_accumulate (one call per image, its patches in order)
    -> [(sum, count)] host float32 arrays; the guards around every destination are asserted"""
    from values_amd import _lib
    lib = _lib.load()
    B, T, C = (int(v) for v in lg.shape[:3])
    P0, P1, P2 = (int(v) for v in lg.shape[3:])
    bufs = []
    for i, d in enumerate(dims):
        off = (1, 3)[i % 2]
        bufs.append((_carve((T, C) + tuple(d), off, fill[0]), off, _carve(tuple(d), 4 - off, fill[1]), 4 - off))
        assert bufs[-1][0][1].data_ptr() % 16 == 4 * off
    ld = _t(lg)
    if route == "K46":
        arr = (_lib.Acc3dItem * B)()
        for it, (i, o) in zip(arr, patches):
            it.sum, it.count = bufs[i][0][1].data_ptr(), bufs[i][2][1].data_ptr()
            for a in range(3):
                it.dims[a], it.origin[a] = int(dims[i][a]), int(o[a])
        ws = _lib.workspace(ld.device, int(lib.vx_softmax_accumulate_cases_workspace_bytes(B)))
        _lib.check(lib.vx_softmax_accumulate_cases(_lib.ptr(ld), B, T, C, P0, P1, P2, arr, int(overlap), _lib.ptr(ws), ws.numel(),
                                                   _lib.stream_ptr()), "vx_softmax_accumulate_cases")
    else:
        for i, d in enumerate(dims):
            idx = [b for b, (j, _) in enumerate(patches) if j == i]
            sub = ld[idx].contiguous()
            crop = torch.tensor([patches[b][1] for b in idx], dtype=torch.int32, device="cuda")
            _lib.check(lib.vx_softmax_accumulate(_lib.ptr(sub), len(idx), T, C, P0, P1, P2, _lib.ptr(crop), _lib.ptr(bufs[i][0][1]),
                                                 _lib.ptr(bufs[i][2][1]), int(d[0]), int(d[1]), int(d[2]), int(overlap), _lib.stream_ptr()),
                       "vx_softmax_accumulate")
    torch.cuda.synchronize()
    out = []
    for (fs, s), so, (fc, c), co in bufs:
        assert _guards_hold(fs, so, s.numel()) and _guards_hold(fc, co, c.numel())
        out.append((s.cpu().numpy(), c.cpu().numpy()))
    return out


@pytest.mark.parametrize("C", range(2, 9))
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("route", ["K14", "K46"])
def test_accumulate_exact_placement(route, overlap, C):
    """One-hot softmax values (pr.hot_logits) placed by non-cubic patches with ragged quads: the sums are small integers,
    equal to the restatement's exactly in both overlap modes.  Destinations start at 5.0 / 2.0, so `=` for `+=` fails;
    the placement cases see a swapped (P0, P1) or (P1, P2) decode (test_placement_cases_can_see_a_transposed_decode)."""
    for P in pr.placement_patches(C):
        dims, patches = pr.placement(P, overlap, route == "K46")
        T = pr.placement_T(P)
        image, origins = [i for i, _ in patches], [o for _, o in patches]
        lg = pr.hot_logits(len(patches), T, C, P)
        sums, counts = pr.accumulate_ref(lg, origins, dims, T, C, image=image)
        got = _run_accumulate(route, lg, dims, patches, overlap, (pr.PREFILL_SUM, pr.PREFILL_COUNT))
        for i, ((s, c), ws, wc) in enumerate(zip(got, sums, counts)):
            assert np.array_equal(c, (pr.PREFILL_COUNT + wc).astype(np.float32)), (P, i)
            assert np.array_equal(s, (pr.PREFILL_SUM + ws).astype(np.float32)), (P, i)
        assert counts[0].max() >= 12 if overlap else counts[0].max() == 1


def test_accumulate_cases_refuses_overlapping_boxes_without_sum_overlap():
    from values_amd import _lib
    P = (3, 5, 7)
    dims, patches = pr.placement(P, 1, True)
    lg = pr.hot_logits(len(patches), 1, 2, P)
    with pytest.raises(_lib.VxError, match="overlapping"):
        _run_accumulate("K46", lg, dims, patches, 0, (0.0, 0.0))


@pytest.fixture(scope="module")
def stride_case():
    """B = 6, T = 4, C = 2, P = (40, 40, 111) into one (40, 40, 666) image: 1 075 200 lanes for K46 (its grid holds
    2048 * 256 = 524 288) and 4 262 400 threads for K14 (its grid holds 16384 * 256 = 4 194 304)"""
    B, T, C, P = 6, 4, 2, (40, 40, 111)
    assert B * T * P[0] * P[1] * ((P[2] + 3) // 4) > 2048 * 256 and B * T * P[0] * P[1] * P[2] > 16384 * 256
    dims = [(40, 40, 666)]
    patches = [(0, (0, 0, 111 * b)) for b in range(B)]
    lg = pr.hot_logits(B, T, C, P)
    sums, counts = pr.accumulate_ref(lg, [o for _, o in patches], dims, T, C, image=[0] * B)
    return lg, dims, patches, (pr.PREFILL_SUM + sums[0]).astype(np.float32), (pr.PREFILL_COUNT + counts[0]).astype(np.float32)


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("route", ["K14", "K46"])
def test_accumulate_takes_a_second_trip_of_the_grid_stride_loop(route, overlap, stride_case):
    lg, dims, patches, want_sum, want_count = stride_case
    (s, c), = _run_accumulate(route, lg, dims, patches, overlap, (pr.PREFILL_SUM, pr.PREFILL_COUNT))
    assert np.array_equal(c, want_count) and np.array_equal(s, want_sum)


@pytest.mark.parametrize("C", [2, 5, 8])
@pytest.mark.parametrize("route", ["K14", "K46"])
def test_accumulate_numeric(route, C):
    """Random logits of scale 3 with rows of equal logits and rows with gaps of +-80 and +-100, patch (3, 5, 7), the
    overlapping lattice (count up to 12 and more), against the float64 restatement.  Counts are equal exactly; per voxel
        |sum - ref| <= n (C + 4) 2^-23 + (n - 1) n 2^-24,   n the voxel's count.
    First term, per addend p_c = e_c * (1 / den) in [0, 1] (no fast-math, -ffp-contract=off): expf is a few ulp off
    (<= 2 * 2^-23 relative on e_c and, through den, the same on 1 / den), the C - 1 float adds of den contribute
    (C - 1) 2^-24 relative, the correctly rounded reciprocal 2^-24 and the correctly rounded product 2^-24: together
    below (4 + (C + 1) / 2) 2^-23 <= (C + 4) 2^-23 relative to a value <= 1.  Second term: n addends in [0, 1] and n - 1
    float32 roundings of partial sums <= n leave the sum within (n - 1) n 2^-24 of the exact one in any order of the
    atomics (the bound test_accumulate_cases_overlapping_crops_within_the_summation_bound uses).  The float32 numpy
    emulation of the same expressions uses under 0.2 of it (tests/test_patches3d_ref_cpu.py)."""
    P, T = (3, 5, 7), 3
    dims, patches = pr.placement(P, 1, route == "K46")
    image, origins = [i for i, _ in patches], [o for _, o in patches]
    lg = pr.numeric_logits(len(patches), T, C, P, seed=100 + C)
    sums, counts = pr.accumulate_ref(lg, origins, dims, T, C, image=image)
    got = _run_accumulate(route, lg, dims, patches, 1, (0.0, 0.0))
    worst = 0.0
    for (s, c), ws, wc in zip(got, sums, counts):
        assert np.array_equal(c, wc.astype(np.float32))
        bound = pr.numeric_bound(wc, C)[None, None]
        diff = np.abs(s.astype(np.float64) - ws)
        worst = max(worst, float((diff / np.maximum(bound, 1e-300)).max()))
    print(f"accumulate numeric {route} C{C}: max |diff| / bound = {worst:.4f}")
    for (s, c), ws, wc in zip(got, sums, counts):
        assert (np.abs(s.astype(np.float64) - ws) <= pr.numeric_bound(wc, C)[None, None]).all()
    assert counts[0].max() >= 12


# ---------------------------------------------------------------------------------------------------------------------
# gather

def _gather(vols, origins, P, out_off):
    """one vx_gather_patches_3d call: item i is the crop at origins[i] of vols[i] (numpy arrays, uploaded one element
    into their allocations) -> (n, P0, P1, P2) host float32"""
    from values_amd import _lib
    from values_amd.dataset3d import _IMAGE_KIND
    lib = _lib.load()
    n = len(vols)
    keep, items = {}, (_lib.Gather3dItem * n)()
    for it, v, o in zip(items, vols, origins):
        if id(v) not in keep:
            keep[id(v)] = _dev(v, 1)
        it.src, it.kind = keep[id(v)][1], _IMAGE_KIND[v.dtype.name]
        assert it.src % min(16, 4 * v.dtype.itemsize) != 0                              # off the pack's alignment
        for a in range(3):
            it.dims[a], it.origin[a] = v.shape[a], int(o[a])
    flat, out = _carve((n,) + tuple(P), out_off, -3.0)
    ws = _lib.workspace(out.device, int(lib.vx_gather_patches_3d_workspace_bytes(n)))
    _lib.check(lib.vx_gather_patches_3d(items, n, _lib.ptr(out), P[0], P[1], P[2], _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "gather")
    torch.cuda.synchronize()
    assert _guards_hold(flat, out_off, out.numel())
    return out.cpu().numpy()


def _gather_volume(rng, dtype):
    """(3, 4, 13) of dtype, D2 odd; the dtype's special values planted twice over inside [1:3, 1:4, :], at every z phase"""
    vol = pr.random_volume(rng, (3, 4, 13), dtype)
    sp = pr.gather_specials(dtype)
    if len(sp):
        pos = np.arange(2 * 3 * 13)[::3][:2 * len(sp)]
        x, y, z = np.unravel_index(pos, (2, 3, 13))
        vol[1 + x, 1 + y, z] = np.tile(sp, 2)[:len(pos)]
    return vol


@pytest.mark.parametrize("dtype", pr.IMAGE_DTYPES)
def test_gather_kind_phase_and_row_length(dtype):
    """every stored kind x z origin phase 0..3 (and the row that ends at the volume's edge) x P2 in 1, 3, 4, 7, 9, the
    volume base one element off: equal to astype(float32) in value, NaN and sign of zero -- float64 in the float32
    denormal range and beyond the float32 maximum, the ties of the 32-bit integers"""
    rng = np.random.default_rng(7)
    vol = _gather_volume(rng, dtype)
    seen = set()
    for n, P2 in enumerate((1, 3, 4, 7, 9)):
        P = (2, 3, P2)
        origins = [(1, 1, ph) for ph in range(4)] + [(1, 1, 13 - P2)]
        want = np.stack([pr.gather_ref(vol, o, P) for o in origins])
        got = _gather([vol] * len(origins), origins, P, (1, 3)[n % 2])
        assert np.array_equal(got, want, equal_nan=True), P2
        assert np.array_equal(np.signbit(got), np.signbit(want)), P2
        seen |= set(want.view(np.uint32).ravel().tolist())
    with np.errstate(over="ignore"):
        planted = pr.gather_specials(dtype).astype(np.float32)
    assert set(planted.view(np.uint32).tolist()) <= seen                      # every planted value was inside some crop


def test_gather_takes_a_second_trip_of_the_grid_stride_loop():
    """5 crops of (48, 48, 197) from (50, 50, 200) volumes of mixed kinds: 576 000 lanes, the grid holds 524 288"""
    P = (48, 48, 197)
    assert 5 * 48 * 48 * ((197 + 3) // 4) > 2048 * 256
    rng = np.random.default_rng(9)
    vols = [pr.random_volume(rng, (50, 50, 200), d) for d in ("float64", "uint8", "int16", "float32", "uint32")]
    origins = [(1, 2, 3), (2, 1, 0), (0, 0, 1), (2, 2, 2), (1, 0, 3)]
    want = np.stack([pr.gather_ref(v, o, P) for v, o in zip(vols, origins)])
    got = _gather(vols, origins, P, 3)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# composite

# n = 1, 2, 3, 5, 1023, 1024, 1025 (and a second 5): below a quad, the ragged tail of one and of two work blocks; the
# eight image kinds; the eight label dtypes; R = 0, 1, 3
COMP_SHAPES = [(1, 1, 1), (1, 2, 1), (1, 1, 3), (1, 1, 5), (3, 11, 31), (4, 16, 16), (5, 5, 41), (5, 1, 1)]
COMP_KINDS = ["uint8", "int8", "uint16", "float32", "float64", "int32", "uint32", "int16"]
COMP_LABELS = [["uint16"], [], ["int64"], ["int8", "uint8", "int16"], ["uint16", "int16", "int64"], ["int32", "uint32", "uint64"],
               ["uint8"], ["int32"]]
COUNTS = np.array([0, 1, 2, 3, 12], dtype=np.float32)


def _composite_inputs():
    rng = np.random.default_rng(13)
    items = []
    for shape, kind, ldt in zip(COMP_SHAPES, COMP_KINDS, COMP_LABELS):
        n = int(np.prod(shape))
        image = pr.random_volume(rng, (n,), kind)
        count = rng.choice(COUNTS, size=n)
        labels = [rng.integers(0, 128 if d == "int8" else 256, size=n).astype(d) for d in ldt]
        items.append({"shape": shape, "image": image, "count": count, "labels": labels})

    def plant(i, r, at, value, cnt):
        items[i]["labels"][r][at] = value
        items[i]["count"][at] = cnt

    def plant_image(i, at, value, cnt):
        items[i]["image"][at] = value
        items[i]["count"][at] = cnt

    plant_image(3, 0, np.nan, 0), plant_image(3, 1, np.inf, 1), plant_image(3, 2, np.nan, 2)
    plant(3, 0, 4, -1, 2)                       # a signed byte -1 (VX_LABEL_SIGNED)
    plant_image(4, 0, np.nan, 0), plant_image(4, 1, np.inf, 0), plant_image(4, 2, np.nan, 3), plant_image(4, 3, -np.inf, 2)
    plant_image(4, 4, 1e308, 12)                # the sum overflows
    plant(4, 0, 10, 256, 2), plant(4, 0, 11, 65535, 1)
    plant(4, 1, 20, -1, 12), plant(4, 1, 21, -1, 0)
    plant(4, 2, 30, -1, 3), plant(4, 2, 31, 2 ** 32 + 7, 2), plant(4, 2, 1022, -2 ** 63, 1)
    plant(5, 0, 5, -1, 12), plant(5, 0, 6, 2 ** 31 - 1, 3), plant(5, 0, 7, -2 ** 31, 2)      # the intc sum wraps
    plant(5, 1, 8, 2 ** 32 - 1, 1), plant(5, 1, 1023, 2 ** 31, 3)
    plant(5, 2, 9, 2 ** 40 + 3, 1), plant(5, 2, 12, 2 ** 64 - 1, 12)
    for it in items:
        it["image"] = it["image"].reshape(it["shape"])
        it["count"] = it["count"].reshape(it["shape"])
        it["labels"] = [l.reshape(it["shape"]) for l in it["labels"]]
        it["want"] = pr.composite_ref(it["image"], it["labels"], it["count"])
    return items


def _run_composite(items, null=None):
    """one vx_case_composite call over `items`; null: the output left out ("data" also leaves out the image)
    -> per item {"data", "gt_seg", "gt" (host arrays, absent when left out or R == 0), "status"}"""
    from values_amd import _lib
    from values_amd.dataset3d import _IMAGE_KIND, _LABEL_KIND
    lib = _lib.load()
    n_items = len(items)
    n_labels = sum(len(it["labels"]) for it in items)
    arr = (_lib.CompositeItem * n_items)()
    lab = (_lib.CompositeLabel * max(n_labels, 1))()
    keep, outs, k = [], [], 0
    for i, (a, it) in enumerate(zip(arr, items)):
        n, R = it["count"].size, len(it["labels"])
        keep.append(_dev(it["count"], (1, 3)[i % 2]))
        a.count = keep[-1][1]
        a.image_kind = _IMAGE_KIND[it["image"].dtype.name]
        a.first_label, a.R = k, R
        a.dims[0], a.dims[1], a.dims[2] = it["shape"]
        o = {}
        if null != "data":
            keep.append(_dev(it["image"], 1))
            a.image = keep[-1][1]
            o["data"] = (_carve((n,), 1, 99.0, torch.float64), 1)
            a.data = o["data"][0][1].data_ptr()
        if null != "gt_seg" and R:
            o["gt_seg"] = (_carve((R, n), (3, 1)[i % 2], 99.0, torch.float64), (3, 1)[i % 2])
            a.gt_seg = o["gt_seg"][0][1].data_ptr()
        if null != "gt" and R:
            o["gt"] = (_carve((R, n), (1, 3)[i % 2], 0x11, torch.uint8, GUARD8), (1, 3)[i % 2])
            a.gt = o["gt"][0][1].data_ptr()
        for l in it["labels"]:
            keep.append(_dev(l, 1))
            lab[k].ptr, lab[k].kind = keep[-1][1], _LABEL_KIND[l.dtype.itemsize]
            lab[k].flags = _lib.VX_LABEL_SIGNED if l.dtype.kind == "i" else 0
            k += 1
        outs.append(o)
    status = torch.full((n_items + 2,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    ws = _lib.workspace(status.device, int(lib.vx_case_composite_workspace_bytes(n_items, n_labels)))
    _lib.check(lib.vx_case_composite(arr, n_items, lab, n_labels, _lib.ptr(status[1:]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "vx_case_composite")
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    assert st[0] == 0x5a5a5a5a and st[-1] == 0x5a5a5a5a
    res = []
    for i, (o, it) in enumerate(zip(outs, items)):
        r = {"status": st[1 + i]}
        for key, ((flat, view), off) in o.items():
            assert _guards_hold(flat, off, view.numel(), GUARD8 if key == "gt" else GUARD), (i, key)
            r[key] = view.cpu().numpy().reshape(((len(it["labels"]),) if key != "data" else ()) + tuple(it["shape"]))
        res.append(r)
    return res


@pytest.fixture(scope="module")
def comp_inputs():
    return _composite_inputs()


@pytest.fixture(scope="module")
def comp_batch(comp_inputs):
    return _run_composite(comp_inputs)


def test_composite_matrix_equals_the_restatement(comp_inputs, comp_batch):
    """all items in one call: the item boundaries fall inside the binary search.  data, gt_seg and gt are the
    restatement's to the bit -- on the planted labels outside 0..255, the wrapping intc sums and NaN / inf images too --
    and status is exactly the number of labels outside 0..255, whatever it held before."""
    assert [it["want"]["n_bad"] for it in comp_inputs] == [0, 0, 0, 1, 7, 7, 0, 0]
    assert sorted({it["image"].dtype.name for it in comp_inputs}) == sorted(pr.IMAGE_DTYPES)
    assert sorted({l.dtype.name for it in comp_inputs for l in it["labels"]}) == sorted(pr.LABEL_DTYPES)
    w5 = comp_inputs[5]["want"]["gt_seg"][0].ravel()
    assert w5[5] == -1.0 and w5[6] == (2 ** 31 - 3) / 3 and w5[7] == 0.0                        # the wraps are in the case
    assert comp_inputs[4]["want"]["gt_seg"][2].ravel()[31] == 7.0 and comp_inputs[4]["want"]["gt_seg"][1].ravel()[20] == -1.0
    for i, (it, got) in enumerate(zip(comp_inputs, comp_batch)):
        want = it["want"]
        assert got["status"] == want["n_bad"], i
        assert np.array_equal(got["data"], want["data"], equal_nan=True), i
        assert np.array_equal(np.signbit(got["data"]) & ~np.isnan(got["data"]), np.signbit(want["data"]) & ~np.isnan(want["data"])), i
        if it["labels"]:
            assert np.array_equal(got["gt_seg"], want["gt_seg"]), i
            assert got["gt"].dtype == np.uint8 and np.array_equal(got["gt"], want["gt"].astype(np.uint8)), i
        else:
            assert "gt_seg" not in got and "gt" not in got
    d4, w4 = comp_batch[4]["data"].ravel(), comp_inputs[4]["want"]["data"].ravel()
    assert d4[0] == 0 and d4[1] == 0 and np.isnan(d4[2]) and d4[3] == -np.inf and d4[4] == np.inf and np.isnan(w4[2])


def test_composite_item_alone_equals_the_item_in_the_batch(comp_inputs, comp_batch):
    for i, it in enumerate(comp_inputs):
        alone, = _run_composite([it])
        assert set(alone) == set(comp_batch[i]) and alone["status"] == comp_batch[i]["status"], i
        for key in alone:
            if key != "status":
                assert _same_bits(alone[key], comp_batch[i][key]), (i, key)


@pytest.mark.parametrize("null", ["data", "gt_seg", "gt"])
def test_composite_outputs_left_null(null, comp_inputs, comp_batch):
    got = _run_composite(comp_inputs, null=null)
    for i, (g, full) in enumerate(zip(got, comp_batch)):
        assert set(g) == set(full) - {null} and g["status"] == full["status"], i
        for key in g:
            if key != "status":
                assert _same_bits(g[key], full[key]), (i, key)


def test_composite_takes_a_second_trip_of_the_grid_stride_loop():
    """(129, 128, 127) is 2048 work blocks of 1024 voxels -- the whole grid -- so the (10, 10, 10) item behind it is
    reached in the second trip of the loop only"""
    assert -(-129 * 128 * 127 // 1024) == 2048
    rng = np.random.default_rng(17)
    items = []
    for shape in ((129, 128, 127), (10, 10, 10)):
        it = {"shape": shape, "image": pr.random_volume(rng, shape, "uint8"), "count": rng.choice(COUNTS, size=shape),
              "labels": [pr.random_volume(rng, shape, "uint8")]}
        it["want"] = pr.composite_ref(it["image"], it["labels"], it["count"])
        items.append(it)
    for it, got in zip(items, _run_composite(items)):
        assert got["status"] == 0
        assert np.array_equal(got["data"], it["want"]["data"]) and np.array_equal(got["gt_seg"], it["want"]["gt_seg"])
        assert np.array_equal(got["gt"], it["want"]["gt"].astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# signed byte labels through the wrappers

def _case(name, labels):
    shape = tuple(labels[0].shape)
    img = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    return {"image_path": name + ".npy", "label_paths": [f"{name}_{r:02d}.npy" for r in range(len(labels))], "image_id": name,
            "image": _t(img), "labels": [_t(l) for l in labels]}


def test_negative_int8_label_raises_on_both_paths():
    from values_amd.dataset2d import label_switch_device
    from values_amd.dataset3d import composite_device
    rng = np.random.default_rng(19)
    lab = rng.integers(0, 128, size=(3, 5, 7)).astype(np.int8)
    lab[1, 2, 3] = -1
    ok = rng.integers(0, 128, size=(3, 5, 7)).astype(np.int8)
    cnt = torch.ones((3, 5, 7), device="cuda")
    with pytest.raises(ValueError, match=r"neg_00\.npy, neg_01\.npy: 1 labels outside 0\.\.255"):
        composite_device([_case("fine", [ok]), _case("neg", [ok, lab])], [cnt, cnt])
    lab2 = rng.integers(0, 128, size=(37, 131)).astype(np.int8)
    lab2[0, 0] = lab2[36, 130] = -1
    lab2[17, 64] = -128
    with pytest.raises(ValueError, match=r"^m\.npy: 3 labels outside 0\.\.255"):
        label_switch_device([_t(ok[0]), _t(lab2)], [0, 1], 2, seed=3, names=["k.npy", "m.npy"])
    with pytest.raises(ValueError, match=r"^item 1: 3 labels outside 0\.\.255"):
        label_switch_device([_t(ok[0]), _t(lab2)], [0, 1], 2, seed=3, variance=True)


def test_2d_device_loader_widens_int8_label_files(tmp_path):
    """the loader builds its label-switch table itself: an int8 file's -1 is counted there too, and a clean int8 file gives
    the raters of its uint8 copy"""
    from tests.dataset2d_trees import augmentations, make_tree
    from values_amd import dataset2d as d2
    segs = {}
    for name, dtype in (("s", np.int8), ("u", np.uint8)):
        base, splits, _ = make_tree(tmp_path / name, label_dtype=dtype)          # the tree's labels hold 255: -1 as a signed byte
        ds = d2.CityscapesTestSet(splits, base, split="id_test", transforms=d2.parse_test_transforms(augmentations(5)), seed=21)
        if dtype == np.int8:
            assert (np.load(ds.masks[0]) == -1).any()
            with d2.DeviceTestLoader2D(ds, 2, seed=21) as loader:
                with pytest.raises(ValueError, match=r"labels/\w+\.npy: \d+ labels outside 0\.\.255"):
                    list(loader)
        for m in ds.masks:
            a = np.load(m)
            a[(a == -1) | (a == 255)] = 0
            np.save(m, a)
        with d2.DeviceTestLoader2D(ds, 2, seed=21) as loader:
            segs[name] = [b["seg"].clone() for b in loader]
    assert len(segs["s"]) == 3 and all(torch.equal(a, b) for a, b in zip(segs["s"], segs["u"]))


def test_non_negative_int8_labels_equal_their_uint8_copy():
    from values_amd.dataset2d import label_switch_device
    from values_amd.dataset3d import composite_device
    rng = np.random.default_rng(23)
    lab = rng.integers(0, 128, size=(3, 5, 7)).astype(np.int8)
    lab[0, 0, 0], lab[2, 4, 6] = 127, 0
    cnt = _t(rng.choice(COUNTS, size=(3, 5, 7)))
    a, = composite_device([_case("s", [lab])], [cnt])
    b, = composite_device([_case("s", [lab.astype(np.uint8)])], [cnt])
    assert set(a) == {"data", "gt_seg", "gt"} and all(torch.equal(a[k], b[k]) for k in a)
    lab2 = rng.integers(0, 128, size=(37, 131)).astype(np.int8)
    ra, va = label_switch_device([_t(lab2)], [5], 3, seed=3, variance=True)
    rb, vb = label_switch_device([_t(lab2.astype(np.uint8))], [5], 3, seed=3, variance=True)
    assert torch.equal(ra[0], rb[0]) and torch.equal(va[0], vb[0])
    assert ra[0].shape == (3, 37, 131) and va[0].shape == (131, 37)
