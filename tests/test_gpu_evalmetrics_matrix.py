"""GPU: the calibration kernels of values_amd/csrc/evalmetrics.hip (vx_platt_sums_batched, vx_calib_bins_batched) against
the long double reference and the bounds of tests/em_ref.py, whose conditions tests/test_em_ref_cpu.py proves without a
device; and the two paths of the NCC half that no other test crosses.

* Platt matrix (R x size x dtype x ignore x (A, B): 432 items in six calls): the two counts `==`, sums[2..7] inside
  their bounds, every sum finite, |z| past 709 included.
* The lattice items (A = B = 0, map on m / 1024): sums[3..7] `==` the reference whatever the libm: an element read at the
  wrong place changes them.
* Bins matrix (the same 432 items): bin_true and bin_total `==` numpy's per bin, bin_sums inside their bounds.
* Special map values: p = 0.5 in bin 9, p = 1 in bin 19, p = 0 in bin 0, +inf by the sign of A, NaN in bin 20 as
  np.digitize puts it (so the ACE of such an image is NaN, as the reference's).
* vx_ncc_batched with a rater stack as ground truth past one trip of the grid, vx_rater_variance past one trip of its
  own, `==` their host restatements.
* _RaterInputs given device tensors, the map stored as (W, H): the same 8 + 63 numbers as from host arrays.

Largest |err| / tol observed over the matrix (MI355X, ROCm 7.2.0, L = 2 in the bounds; the two counts, bin_true and
bin_total are `==`, ratio 0): loss 0.157, dA 0.025, dB 0.016, AA 0.023, AB 0.019, BB 0.020; bin_sums 0.029.  The largest is the loss at A = B = 0, where every
element adds the same rounded ln 2 and the errors do not cancel.  L, measured with float64 torch.exp / torch.log1p on the
device over the z of the 300001-voxel float64 map at the six (A, B), against long double: exp 0.85 ulp, log1p 1.0 ulp
at the most; rounded up plus one that is the 2 the bounds were written with.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import em_ref
from tests.em_inputs import calib_bins_numpy, ncc_sums_restated, rater_variance_restated

pytestmark = pytest.mark.gpu

_EXACT = [0, 1, 3, 4, 5, 6, 7]


@pytest.fixture(scope="module")
def on_device():
    """cases -> their _RaterInputs; an input goes up once per ignore value, whatever the number of cases that share it"""
    from values_amd import evalmetrics as vm
    cache = {}

    def get(cases):
        xs = []
        for c in cases:
            key = (id(c.ref), id(c.unc), c.ignore)
            if key not in cache:
                cache[key] = (vm._RaterInputs(c.ref.copy(), c.pred.copy(), c.unc.copy(), c.ignore), c.ref, c.unc)   # (the shared inputs are read-only)
            xs.append(cache[key][0])
        return xs
    return get


def _platt(cases, on_device):
    """one vx_platt_sums_batched call for cases that share an ignore value"""
    from values_amd import evalmetrics as vm
    assert len({c.ignore for c in cases}) == 1 and len(cases) <= 4096
    return np.array(vm._platt_sums_batch(on_device(cases), [(c.A, c.B, c.t_pos, c.t_neg) for c in cases]))


def _bins(cases, on_device):
    """one vx_calib_bins_batched call, every item with its own (A, B): [n][63]"""
    from values_amd import _lib, evalmetrics as vm
    assert len({c.ignore for c in cases}) == 1 and len(cases) <= 4096
    lib, xs, n = _lib.load(), on_device(cases), len(cases)
    items = vm._em_items(xs)
    ab = (C.c_double * (2 * n))(*[v for c in cases for v in (c.A, c.B)])
    edges = (C.c_double * 21)(*em_ref.EDGES.tolist())
    ws = _lib.workspace(xs[0].dev, int(lib.vx_calib_batched_workspace_bytes(items, n)))
    out = torch.empty((n, 63), dtype=torch.float64, device=xs[0].dev)
    _lib.check(lib.vx_calib_bins_batched(items, n, ab, edges, xs[0].ignore, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                         _lib.stream_ptr()), "vx_calib_bins_batched")
    return out.cpu().numpy()


def _report(what, names, ratios, cases):
    ratios = np.asarray(ratios)
    worst = np.nanargmax(ratios, axis=0)
    for k, name in enumerate(names):
        print(f"{what}: largest |err| / tol of {name}: {ratios[worst[k], k]:.4g} at {cases[worst[k]]}")


@pytest.mark.parametrize("R", em_ref.RATERS)
@pytest.mark.parametrize("ignore", em_ref.IGNORES)
def test_platt_matrix(ignore, R, on_device):
    cases = em_ref.matrix(ignores=(ignore,), raters=(R,))
    got = _platt(cases, on_device)
    ratios = []
    for c, g in zip(cases, got):
        want, tol = em_ref.platt_reference(c)
        ratios.append(em_ref.ratio(g, want, tol)[2:])
    _report(f"platt, R {R}, ignore {ignore}", em_ref.SUM_NAMES[2:], ratios, cases)
    assert np.isfinite(got).all(), [c for c, g in zip(cases, got) if not np.isfinite(g).all()]
    assert np.array_equal(got[:, 0], [c.n_valid for c in cases]) and np.array_equal(got[:, 1], [c.n_correct for c in cases])
    bad = [(c, r) for c, r in zip(cases, ratios) if not (r < 1).all()]
    assert not bad, bad[:5]


def test_platt_lattice_sums_are_exact(on_device):
    for ignore in em_ref.IGNORES:
        cases = [c for c in em_ref.lattice_cases() if c.ignore == ignore]
        assert len(cases) == 6
        for c, g in zip(cases, _platt(cases, on_device)):
            want, tol = em_ref.platt_reference(c)
            assert np.array_equal(g[_EXACT].astype(em_ref.LD), want[_EXACT]), (c, g, want)
            assert want[3] != 0 and em_ref.ratio(g, want, tol)[2] < 1, (c, g[2], want[2], tol[2])


@pytest.mark.parametrize("R", em_ref.RATERS)
@pytest.mark.parametrize("ignore", em_ref.IGNORES)
def test_bins_matrix(ignore, R, on_device):
    cases = em_ref.matrix(ignores=(ignore,), raters=(R,))
    got = _bins(cases, on_device)
    ratios, wrong = [], []
    for c, g in zip(cases, got):
        ws, wt, wn, wtol, _ = em_ref.bins_reference(c)
        ratios.append([em_ref.ratio(g[:21], ws, wtol).max()])
        if not (np.array_equal(g[21:42], wt) and np.array_equal(g[42:], wn)):
            wrong.append((c, g[21:], wt, wn))
    _report(f"bins, R {R}, ignore {ignore}", ["bin_sums"], ratios, cases)
    assert np.isfinite(got).all() and not wrong, wrong[:3]
    bad = [(c, r) for c, r in zip(cases, ratios) if not r[0] < 1]
    assert not bad, bad[:5]
    # numpy's own bins on one large case: the reference's counts are np.digitize's and np.bincount's
    c = cases[-1]
    _, bt, bn, _ = calib_bins_numpy(c.ref, c.pred, c.unc, c.A, c.B, c.ignore)
    assert np.array_equal(got[-1][21:42], bt) and np.array_equal(got[-1][42:], bn)


def test_bins_of_special_map_values(on_device):
    from values_amd import evalmetrics as vm
    cases = em_ref.special_cases()
    got = dict(zip(cases, _bins(list(cases.values()), on_device)))
    for name, (_, _, _, k) in em_ref.SPECIALS.items():
        c, g = cases[name], got[name]
        want = np.zeros(63)
        want[[k, 21 + k, 42 + k]] = {9: 0.5, 19: 1.0, 0: 0.0, 20: np.nan}[k] * c.n_valid, c.n_correct, c.n_valid
        assert np.array_equal(g, want, equal_nan=True), (name, g)
    c, g = cases["mixed"], got["mixed"]
    bs, bt, bn, _ = calib_bins_numpy(c.ref, c.pred, c.unc, c.A, c.B, c.ignore)
    ws, _, _, wtol, _ = em_ref.bins_reference(c)
    assert np.array_equal(g[21:42], bt) and np.array_equal(g[42:], bn) and bn[[0, 9, 19, 20]].min() >= 5, g[21:]
    assert g[0] == 0.0 and g[19] == bn[19] and np.isnan(g[20])           # exp overflowed, exp underflowed, NaN
    assert (em_ref.ratio(g[1:19], ws[1:19], wtol[1:19]) < 1).all() and np.isfinite(wtol[1:19]).all()
    # the host part follows: a NaN voxel makes a bin of its own and the ACE NaN, as calib_stats of ace.py does
    ref, pred = c.ref.copy(), c.pred.copy()
    disc, weights, k = vm.calib_stats(ref, pred, c.unc, c.A, c.B, c.ignore)
    assert k == np.count_nonzero(bn) and np.isnan(disc[-1]) and np.isfinite(disc[:-1]).all() and weights[-1] == bn[20] / bn.sum()
    assert np.isnan(vm.calc_ace(ref, pred, c.unc, c.A, c.B, c.ignore))


def test_ncc_rater_stack_beyond_one_grid_trip():
    from values_amd.evalmetrics import _ncc_sums_batch
    rng = np.random.default_rng(43)
    stacks, preds = [], []
    for R in em_ref.RATERS:
        for k, n in enumerate((131072, 131073, 300001)):
            stacks.append(em_ref.labels(R, n)[0].copy())
            preds.append((0.5 * np.var(stacks[-1], axis=0) + 0.5 * rng.random(n)).astype(em_ref.DTYPES[(R + k) % 2]))
    for labels, p, (n, row) in zip(stacks, preds, _ncc_sums_batch(stacks, preds)):
        want = ncc_sums_restated(rater_variance_restated(labels), p)
        assert n == len(p) and row == want, (labels.shape, row, want)
        assert labels.shape[0] == 1 or want[4] > 0


def test_rater_variance_beyond_one_grid_trip():
    from values_amd.evalmetrics import rater_variance
    n = 4096 * 256 + 257
    labels = np.random.default_rng(47).integers(0, 4, (3, n)).astype(np.int32)
    want = np.var(labels, axis=0)
    got = rater_variance(labels).cpu().numpy()
    assert np.array_equal(got, want) and want[4096 * 256:].max() > 0


def test_device_inputs_with_a_swapped_2d_map_give_the_host_routes_numbers(on_device):
    from values_amd import evalmetrics as vm
    rng = np.random.default_rng(53)
    R, H, W = 3, 20, 33
    ref, pred = (a.reshape(a.shape[:-1] + (H, W)).copy() for a in em_ref.labels(R, H * W))
    unc = (rng.random((H, W)) * 0.7).astype(np.float32)
    swapped = np.ascontiguousarray(unc.T)
    cases = [em_ref.Case(ref.reshape(R, -1), pred.reshape(-1), unc.reshape(-1), ign, -3.5, 1.25) for ign in em_ref.IGNORES]
    for c in cases:
        host = vm._RaterInputs(ref, pred, swapped, c.ignore)
        dev = vm._RaterInputs(torch.from_numpy(ref).cuda(), torch.from_numpy(pred).cuda(), torch.from_numpy(swapped).cuda(), c.ignore)
        assert dev.unc.is_cuda and tuple(dev.unc.shape) == (H, W) and dev.unc.is_contiguous() and (dev.R, dev.nvox) == (R, H * W)
        params = [(c.A, c.B, c.t_pos, c.t_neg)]
        sums = [vm._platt_sums_batch([x], params)[0] for x in (host, dev)]
        bins = [_bins([c], lambda cases, x=x: [x])[0] for x in (host, dev)]
        assert sums[0] == sums[1] and np.array_equal(bins[0], bins[1])
        # ... which are the numbers of the unswapped map
        want, tol = em_ref.platt_reference(c)
        ws, wt, wn, wtol, _ = em_ref.bins_reference(c)
        assert sums[1][0] == c.n_valid and sums[1][1] == c.n_correct and (em_ref.ratio(sums[1], want, tol) < 1).all()
        assert np.array_equal(bins[1][21:42], wt) and np.array_equal(bins[1][42:], wn)
        assert (em_ref.ratio(bins[1][:21], ws, wtol) < 1).all()
