"""Inputs shared by tests/test_evalmetrics_batched_cpu.py, tests/test_gpu_evalmetrics_batched.py and the matrix tests
(tests/test_em_ref_cpu.py, tests/test_gpu_evalmetrics_matrix.py): numpy stand-ins for the Platt sums and the calibration
bins, images whose Platt fits finish in different rounds, rater label stacks, host restatements of the device
arithmetic (the rater variance, the five NCC sums in the documented association), and a datamodule stub for a results tree whose reference segmentations come from a dataloader."""
import os

import numpy as np


def platt_sums_numpy(unc, correct, A, B, t_pos, t_neg):
    """numpy stand-in for one item of vx_platt_sums_batched (R = 1, nothing ignored): the same eight sums, numpy's
    summation order"""
    F = -np.asarray(unc, dtype=np.float64)
    T = np.where(correct, t_pos, t_neg)
    z = A * F + B
    e = np.exp(-np.abs(z))
    P = np.where(z >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    loss = np.where(z >= 0, T * z, (T - 1.0) * z) + np.log1p(e)
    d, w = T - P, P * (1.0 - P)
    return [float(len(F)), float(np.sum(correct)), float(loss.sum()), float((d * F).sum()), float(d.sum()),
            float((w * F * F).sum()), float((w * F).sum()), float(w.sum())]


def platt_sums_raters_numpy(ref, pred, unc, A, B, t_pos, t_neg, ignore=None):
    """platt_sums_numpy for R reference segmentations ref [R][nvox] against pred [nvox] and the map unc [nvox], as
    ace.py:24-31 lays them out (prediction and map repeated per rater, rater-voxels with ref == ignore dropped)"""
    valid = np.ones(ref.shape, dtype=bool) if ignore is None else ref != ignore
    return platt_sums_numpy(np.broadcast_to(unc[None], ref.shape)[valid], (ref == pred[None])[valid], A, B, t_pos, t_neg)


def calib_bins_numpy(ref, pred, unc, A, B, ignore=None):
    """(bin_sums, bin_true, bin_total, bin ids) of one item of vx_calib_bins_batched as ace.py:46 and :67-73 form them:
    numpy's 1 / (1 + np.exp(...)), np.digitize and np.bincount in float64.  bin_sums alone are added per bin with numpy's
    pairwise sum, not with np.bincount(weights=...): bincount adds a bin's members one after the other, a chain of additions
    as long as the bin (1.4e-8 off on 131072 values near 1), where the bound of tests/em_ref.py allows for the 523 to 532
    of the device's association"""
    valid = np.ones(ref.shape, dtype=bool) if ignore is None else ref != ignore
    conf = -np.broadcast_to(np.asarray(unc, dtype=np.float64)[None], ref.shape)[valid]
    with np.errstate(over="ignore", invalid="ignore"):
        prob = 1 / (1 + np.exp(conf * A + B))
    bins = np.linspace(0.0, 1.0 + 1e-8, 21)
    binids = np.digitize(prob, bins) - 1
    correct = (ref == pred[None])[valid].astype(np.float64)
    return (np.array([prob[binids == k].sum() for k in range(21)]), np.bincount(binids, weights=correct, minlength=21),
            np.bincount(binids, minlength=21).astype(np.float64), binids)


def platt_items():
    """(uncertainty, correct) of six one-rater images that finish in different rounds: one whose start point is already the
    optimum (zero map, as many correct as wrong voxels), well and badly separated ones, and two heavy-tailed maps (a few
    huge uncertainties among tiny ones) on which the full Newton step overshoots, so the line search halves it"""
    items = [(np.zeros(40), np.arange(40) % 2 == 0)]
    rng = np.random.default_rng(7)
    for n, sep, flip in ((500, 0.0, 0.3), (257, 0.5, 0.0), (1031, 0.3, 0.02)):
        correct = rng.random(n) < 0.7
        unc = np.where(correct, rng.random(n) * 0.2, 0.2 + sep + rng.random(n) * 0.2)
        items.append((unc, correct ^ (rng.random(n) < flip)))
    for seed, n in ((27, 241), (7, 103)):
        rng = np.random.default_rng(seed)
        correct = rng.random(n) < 0.97
        correct[:2] = (True, False)
        items.append((np.exp(rng.normal(0.0, 3.0, n)) * np.where(correct, 0.1, 1.0), correct))
    return items


def rater_label_cases():
    """label stacks (R, *spatial) for R in {1, 3, 4}, labels 0..3, a 3D and a 2D shape"""
    rng = np.random.default_rng(21)
    return [rng.integers(0, 4, (R,) + shape).astype(np.int32) for R in (1, 3, 4) for shape in ((5, 7, 3), (64, 48))]


def rater_variance_restated(labels):
    """np.var(labels, axis=0) in the order of the device function em_rater_var, one float64 operation at a time"""
    R = labels.shape[0]
    s = np.zeros(labels.shape[1:], dtype=np.float64)
    for r in range(R):
        s = s + labels[r].astype(np.float64)
    mean = s / np.float64(R)
    q = np.zeros_like(s)
    for r in range(R):
        d = labels[r].astype(np.float64) - mean
        q = q + d * d
    return q / np.float64(R)


EM_BLOCKS, EM_THREADS = 512, 256          # the grid of every reduction of evalmetrics.hip


def _sum_in_device_order(x):
    """the sum of the float64 vector x in the association include/values_amd.h documents: element i belongs to thread
    i % 131072, which adds its elements in ascending i starting from 0.0 (elements past the end are never added); in every
    wave of 64 threads the shuffle-down tree with offsets 32, 16, ..., 1, of which lane 0's value is kept; the four waves
    of a block added in order from 0.0; the 512 block rows added in index order from 0.0"""
    grid = EM_BLOCKS * EM_THREADS
    acc = np.zeros(grid, dtype=np.float64)
    for lo in range(0, len(x), grid):
        part = x[lo:lo + grid]
        acc[:len(part)] = acc[:len(part)] + part
    lanes = acc.reshape(EM_BLOCKS, EM_THREADS // 64, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):          # lane l < off takes lane l + off; only those lanes reach lane 0
        lanes[..., :off] = lanes[..., :off] + lanes[..., off:2 * off]
    rows = np.zeros(EM_BLOCKS, dtype=np.float64)
    for w in range(EM_THREADS // 64):
        rows = rows + lanes[:, w, 0]
    total = np.float64(0.0)
    for b in range(EM_BLOCKS):
        total = total + rows[b]
    return float(total)


def ncc_sums_restated(g, p):
    """[sum g, sum p, sum (g-mg)^2, sum (p-mp)^2, sum (g-mg)(p-mp)] of a map pair as vx_ncc_batched forms them, one float64
    operation at a time: pass 0, then mg = sum g / n and mp = sum p / n, then pass 1 with the products formed unfused"""
    g, p = np.asarray(g).reshape(-1).astype(np.float64), np.asarray(p).reshape(-1).astype(np.float64)
    n = len(g)
    sg, sp = _sum_in_device_order(g), _sum_in_device_order(p)
    da, db = g - np.float64(sg) / np.float64(n), p - np.float64(sp) / np.float64(n)
    return [sg, sp, _sum_in_device_order(da * da), _sum_in_device_order(db * db), _sum_in_device_order(da * db)]


class StubDataModule:
    """datamodule_config target of a test tree: <root>/<split>/<id>.npy is an image's (H, W) label (what gta.gt_unc_map
    reads through dataset.masks), <id>_seg.npy its (R, H, W) reference segmentations"""

    def __init__(self, root, test_split):
        self.dir = os.path.join(root, test_split)

    def setup(self, stage):
        pass

    def test_dataloader(self):
        return _StubLoader(self.dir)


class _StubDataset:
    def __init__(self, d):
        self.dir = d
        self.image_ids = sorted(f[:-4] for f in os.listdir(d) if f.endswith(".npy") and not f.endswith("_seg.npy"))
        self.masks = [os.path.join(d, f"{i}.npy") for i in self.image_ids]

    def __getitem__(self, idx):
        import torch
        return {"seg": torch.from_numpy(np.load(os.path.join(self.dir, f"{self.image_ids[idx]}_seg.npy")))[None]}


class _StubLoader:
    def __init__(self, d):
        self.dataset = _StubDataset(d)
