"""GPU: vx_one_minus_msr_batched / uncertainty.one_minus_msr_batch -- 1 - max softmax for a batch of images whose class
planes are separate device arrays, in one launch.

The operation is exact in the input precision (comparisons, one subtraction from 1), so every check is bit equality: with
numpy on NaN-free inputs, with calculate_one_minus_msr (the per-image kernel on the contiguously stacked planes) on all
inputs.  The sizes: every n below 5 (no whole 16-byte chunk), around 64 / 256 / 1024 (a wave, a workgroup, a work block's
lanes), 4099 and 9001 (a work block is 1024 chunks = 4096 float32 / 2048 float64 elements: whole work blocks, the vector
path, exist only beyond that -- at 9001 also for planes that do not start on a 16-byte boundary).
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests.formula import formula_tensor

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 9001)
CS = (1, 2, 3, 8, 19, 20)
GUARD = 64
SENTINEL = -7.25


def _probs(shape, tag, dtype):
    """formula_tensor mapped into (0, 1)"""
    return ((formula_tensor(shape, tag) + 1.0) * 0.499 + 0.001).astype(dtype)


class _Arena:
    """planes and guarded outputs cut from one 256-byte aligned device buffer at chosen element offsets"""

    def __init__(self, dtype, n_elems):
        self.buf = torch.full((n_elems,), SENTINEL, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.per256 = 256 // self.buf.element_size()
        self.pos = 0

    def cut(self, n, offset):
        """n elements that start `offset` elements after a 256-byte boundary"""
        start = self.pos + offset
        self.pos = (start + n + self.per256 - 1) // self.per256 * self.per256
        assert self.pos <= self.buf.numel()
        return self.buf[start:start + n]

    def cut_guarded(self, n, offset):
        g = self.cut(n + 2 * GUARD, offset)
        return g[GUARD:GUARD + n], g


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _ref_stacked(planes):
    from values_amd.uncertainty import calculate_one_minus_msr
    return calculate_one_minus_msr(torch.stack([p.contiguous() for p in planes]))["pred_entropy"]


def _matrix(dtype, same_offset, special):
    """every (n, C) of the matrix as one item each of ONE call -> [(planes, out, guarded out, host planes)]"""
    from values_amd.uncertainty import one_minus_msr_batch
    npdt = np.float32 if dtype == torch.float32 else np.float64
    total = sum((n + 2 * 256) * (c + 1) + 4 * GUARD for n in NS for c in CS)
    arena = _Arena(dtype, total)
    cases = []
    for i, (n, c) in enumerate((n, c) for n in NS for c in CS):
        host = _probs((c, n), 100 + i, npdt)
        if special:
            v = host.reshape(-1)
            v[0::7] = np.nan if i % 2 == 0 else v[0::7]          # a NaN in plane 0 (and beyond) ...
            if c > 1:
                host[c - 1, 0::5] = np.nan                        # ... in the last plane
                host[c // 2, 1::5] = np.inf
            host[0, 2::11] = -np.inf
            host[:, 3::13] = -0.0                                 # every plane -0.0: the maximum keeps the sign
            host[0, 4::17] = 1.5                                  # values above 1
        planes = [arena.cut(n, i % 4 if same_offset else (i + k) % 4) for k in range(c)]
        out, guarded = arena.cut_guarded(n, (i // 4) % 4)         # independent of the planes' offsets
        for p, h in zip(planes, host):
            p.copy_(torch.from_numpy(h))
        cases.append((planes, out, guarded, host))
    got = one_minus_msr_batch([planes for planes, _, _, _ in cases], out=[o for _, o, _, _ in cases])
    assert all(g.data_ptr() == o.data_ptr() for g, (_, o, _, _) in zip(got, cases))
    torch.cuda.synchronize()
    return cases


@pytest.mark.parametrize("same_offset", [True, False], ids=["same_offset", "mixed_offsets"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_matrix_equals_numpy_and_the_per_image_kernel(dtype, same_offset):
    for planes, out, guarded, host in _matrix(dtype, same_offset, special=False):
        n, c = out.numel(), len(planes)
        want = 1 - np.max(np.stack(host), 0)
        assert want.dtype == host.dtype
        assert (out.cpu().numpy() == want).all(), (n, c)
        assert torch.equal(_bits(out), _bits(_ref_stacked(planes))), (n, c)
        g = guarded.cpu()
        assert (g[:GUARD] == SENTINEL).all() and (g[GUARD + n:] == SENTINEL).all(), (n, c)


@pytest.mark.parametrize("same_offset", [True, False], ids=["same_offset", "mixed_offsets"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_matrix_nan_inf_negative_zero_bits(dtype, same_offset):
    saw_nan = False
    for planes, out, guarded, host in _matrix(dtype, same_offset, special=True):
        n, c = out.numel(), len(planes)
        assert torch.equal(_bits(out), _bits(_ref_stacked(planes))), (n, c)
        saw_nan = saw_nan or bool(torch.isnan(out).any())
        g = guarded.cpu()
        assert (g[:GUARD] == SENTINEL).all() and (g[GUARD + n:] == SENTINEL).all(), (n, c)
    assert saw_nan


def test_an_item_does_not_depend_on_its_batch_mates():
    from values_amd.uncertainty import one_minus_msr_batch
    specs = [(torch.float32, 4099, 3), (torch.float64, 257, 2), (torch.float32, 0, 2), (torch.float64, 9001, 19),
             (torch.float32, 5, 1), (torch.float32, 1025, 20), (torch.float64, 3, 8)]
    items, guards = [], []
    for i, (dt, n, c) in enumerate(specs):
        npdt = np.float32 if dt == torch.float32 else np.float64
        planes = [torch.from_numpy(_probs((n,), 300 + 10 * i + k, npdt)).cuda() for k in range(c)]
        guards.append(torch.full((n + 2 * GUARD,), SENTINEL, dtype=dt, device="cuda"))
        items.append(planes)
    together = one_minus_msr_batch(items, out=[g[GUARD:GUARD + n] for g, (_, n, _) in zip(guards, specs)])
    torch.cuda.synchronize()
    assert (guards[2] == SENTINEL).all()          # the n == 0 item wrote nothing
    for planes, t, (dt, n, c) in zip(items, together, specs):
        alone = one_minus_msr_batch([planes])[0]
        assert alone.dtype == dt and alone.shape == (n,)
        assert torch.equal(_bits(t), _bits(alone)), (dt, n, c)
        if n:
            assert torch.equal(_bits(t), _bits(_ref_stacked(planes)))
    for g, (_, n, _) in zip(guards, specs):
        assert (g[:GUARD] == SENTINEL).all() and (g[GUARD + n:] == SENTINEL).all()


def test_wrapper_forms_and_memory_order():
    from values_amd.uncertainty import one_minus_msr_batch
    assert one_minus_msr_batch([]) == []
    x = torch.from_numpy(_probs((3, 5, 4, 7), 500, np.float64)).cuda()
    whole, listed = one_minus_msr_batch([x, list(x.unbind(0))])
    assert whole.shape == (5, 4, 7) and whole.is_contiguous()
    assert torch.equal(_bits(whole), _bits(listed)) and torch.equal(_bits(whole), _bits(_ref_stacked(list(x.unbind(0)))))
    # a reader's [x, y, z] view: a (Z, Y, X) block indexed the other way round.  The result keeps the planes' strides.
    planes = [torch.from_numpy(_probs((7, 4, 5), 510 + k, np.float32)).cuda().permute(2, 1, 0) for k in range(3)]
    assert not planes[0].is_contiguous()
    got = one_minus_msr_batch([planes])[0]
    assert got.shape == (5, 4, 7) and got.stride() == planes[0].stride()
    want = 1 - torch.stack(planes).max(0).values
    assert torch.equal(got, want)
    # planes that are no dense block (a strided slice) are made contiguous
    wide = torch.from_numpy(_probs((2, 6, 10), 520, np.float32)).cuda()
    got = one_minus_msr_batch([[wide[0, :, ::2], wide[1, :, ::2]]])[0]
    assert got.is_contiguous() and torch.equal(got, 1 - torch.maximum(wide[0, :, ::2], wide[1, :, ::2]))
    with pytest.raises(ValueError):
        one_minus_msr_batch([[wide[0], wide[1].double()]])
    with pytest.raises(ValueError):
        one_minus_msr_batch([wide.cpu()])


def _raw(entries, n_items=None, n_planes=None, null_items=False, null_planes=False, ws="ok"):
    """vx_one_minus_msr_batched with hand-made tables; -> the VxError's rc"""
    from values_amd import _lib
    from values_amd.uncertainty import msr_tables
    lib = _lib.load()
    items, table, count = msr_tables(entries)
    n_items = len(entries) if n_items is None else n_items
    n_planes = count if n_planes is None else n_planes
    need = int(lib.vx_one_minus_msr_batched_workspace_bytes(max(n_items, 1), max(n_planes, 1)))
    buf = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    wsp, wsn = {"ok": (buf.data_ptr(), need), "short": (buf.data_ptr(), need - 1), "odd": (buf.data_ptr() + 8, need),
                "null": (None, need)}[ws]
    with pytest.raises(_lib.VxError) as e:
        _lib.check(lib.vx_one_minus_msr_batched(None if null_items else items, n_items, None if null_planes else table, n_planes,
                                                wsp, wsn, _lib.stream_ptr()), "vx_one_minus_msr_batched")
    return int(re.search(r"rc=(-?\d+)", str(e.value)).group(1))


def test_refusals_come_before_any_device_call():
    NULL, SHAPE, DTYPE, WORKSPACE, ALIGN = -1, -2, -3, -4, -5
    F32, F64 = 0, 1
    out = torch.full((64,), SENTINEL, dtype=torch.float64, device="cuda")
    a = torch.zeros(64, dtype=torch.float64, device="cuda")
    b = torch.zeros(64, dtype=torch.float64, device="cuda")
    o, pa, pb = out.data_ptr(), a.data_ptr(), b.data_ptr()
    good = (o, 16, F64, [pa, pb])
    assert _raw([good], null_items=True) == NULL
    assert _raw([good], null_planes=True) == NULL
    assert _raw([(o, 16, F64, [pa, None])]) == NULL                    # a null plane of an item with n > 0
    assert _raw([(None, 16, F64, [pa, pb])]) == NULL                   # a null out of an item with n > 0
    assert _raw([good], ws="null") == NULL
    assert _raw([good], n_items=0) == SHAPE
    assert _raw([(o, -1, F64, [pa, pb])]) == SHAPE
    assert _raw([(o, 16, F64, [])], n_planes=2) == SHAPE               # C < 1
    assert _raw([good], n_planes=1) == SHAPE                            # first_plane + C > n_planes
    assert _raw([good, (o, 16, F64, [pa, pb])], n_planes=3) == SHAPE
    assert _raw([(o, 16, 2, [pa, pb])]) == DTYPE
    assert _raw([(o, 16, -1, [pa, pb])]) == DTYPE
    assert _raw([(o + 4, 16, F64, [pa, pb])]) == ALIGN                  # off the 8-byte elements
    assert _raw([(o, 16, F64, [pa, pb + 4])]) == ALIGN
    assert _raw([(o, 16, F32, [pa + 2, pb])]) == ALIGN                  # off the 4-byte elements
    assert _raw([good], ws="odd") == ALIGN
    assert _raw([good], ws="short") == WORKSPACE
    # a refused item after a good one: the good one is not computed either
    assert _raw([good, (o, 16, 7, [pa, pb])]) == DTYPE
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
