"""Downstream scalars of the evaluation stage: same function names, arguments and result files as
evaluation/metrics/{aurc,ncc,ace,auroc}.py, so the task functions of evaluation/configs/tasks/*.yaml can be re-pointed.

Where the work is per voxel it runs on the GPU in float64 (values_amd/csrc/evalmetrics.hip, deterministic reductions), a
whole batch of images per device call:
  ncc_batch                  ncc.py:9-25    two-pass mean / std(ddof=1) / cross product of two maps
  sigmoid_calibration_batch  ace.py:13-41   Platt scaling of -uncertainty against "reference == prediction": loss,
                                            gradient and Hessian sums on the device, Newton steps on the host (the
                                            iterations of all images in lock step)
  calc_ace_batch             ace.py:44-90   platt_scale_confid + the 20-bin statistics of calib_stats in one pass
compute_ncc, sigmoid_calibration and calc_ace, the reference's per-image functions, are a batch of one: an image's numbers
do not depend on its batch mates, so both forms give the same bits.  The drivers ambiguity_modeling_device /
platt_scale_params_device / calibration_error_device / calibration_device take a DeviceExperimentDataloader and write the
same JSON files as the reference's per-image loops (ambiguity_modeling, platt_scale_params, ...), byte for byte.
Where it is one scalar per IMAGE (AURC / E-AURC over (risk, confidence) pairs, AUROC over (OoD label, score) pairs:
a few hundred numbers) it stays on the host, restated in numpy float64: aurc.py:14-67, and sklearn's roc_curve + auc
as auroc.py:126-127 calls them.  scikit-learn itself is not needed.
"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib


def _on_device(a):
    return isinstance(a, torch.Tensor) and a.is_cuda


def _dev():
    _lib.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def _float_map(a, dev):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.detach()
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    t = t.to(dev).contiguous()
    return t, (_lib.VX_F64 if t.dtype == torch.float64 else _lib.VX_F32)


# ------------------------------------------------------------------------------------------------ failure detection
def rc_curve_stats(risks, confids):
    """aurc.py:14-51: coverages, selective risks and weights of the risk-coverage curve (ties in the confidence
    collapse into one point)."""
    risks, confids = np.asarray(risks, dtype=np.float64), np.asarray(confids, dtype=np.float64)
    assert risks.ndim == 1 and confids.ndim == 1 and len(risks) == len(confids)
    n = len(risks)
    order = np.argsort(confids)
    r, c = risks[order], confids[order]
    coverage, err = n, float(sum(r))
    coverages, selective, weights = [coverage / n], [err / n], []
    pending = 0
    for i in range(n - 1):
        coverage -= 1
        err -= r[i]
        pending += 1
        if i == 0 or c[i] != c[i - 1]:
            coverages.append(coverage / n)
            selective.append(err / (n - 1 - i))
            weights.append(pending / n)
            pending = 0
    if pending > 0:
        coverages.append(0)
        selective.append(selective[-1])
        weights.append(pending / n)
    return coverages, selective, weights


def aurc(risks, confids):
    _, sel, w = rc_curve_stats(risks, confids)
    return sum((sel[i] + sel[i + 1]) * 0.5 * w[i] for i in range(len(w)))


def eaurc(risks, confids):
    """AURC minus the AURC of the optimal confidence ranking (aurc.py:61-67)"""
    risks = np.asarray(risks, dtype=np.float64)
    n = len(risks)
    best = np.sort(risks).cumsum() / np.arange(1, n + 1)
    return aurc(risks, confids) - best.sum() / n


def _metric_entry(metrics, image_id):
    if image_id not in metrics:
        keys = [k for k in metrics if k.split("/")[-1].split(".")[0] == image_id]
        if len(keys) > 1:
            print(f"Found multiple matches for image id {image_id}. Using the first match {keys[0]}")
        image_id = keys[0]
    e = metrics[image_id]
    return e["dice"] if "dice" in e else e["metrics"]["dice"]


def get_dice(image_id, metrics_file):
    with open(metrics_file) as f:
        return _metric_entry(json.load(f), image_id)


def get_risk(image_id, metrics_file):
    return 1 - get_dice(image_id, metrics_file)


def get_confid(image_name, aggregated_unc_file, aggregation_level, unc_file_ending):
    with open(aggregated_unc_file) as f:
        unc = json.load(f)
    return -unc[f"{image_name}{unc_file_ending}"][aggregation_level]["max_score"]


def get_risks_and_confids(dataset_path, image_ids, unc_type, aggregation, unc_file_ending):
    risks, confids, dices = [], [], []
    for image in image_ids:
        dice = get_dice(image, dataset_path / "metrics.json")
        dices.append(dice)
        risks.append(1 - dice)
        confids.append(get_confid(image, dataset_path / f"aggregated_{unc_type}.json", aggregation, unc_file_ending))
    return risks, confids, dices


def failure_detection(exp_dataloader):
    """aurc.py:128-153 (its `main`): failure_detection.json with AURC / E-AURC per uncertainty type and aggregation"""
    ev = exp_dataloader.exp_version
    res = {"mean": {}}
    for unc_type in ev.unc_types:
        res["mean"][unc_type] = {}
        for aggregation in ev.aggregations:
            risks, confids, _ = get_risks_and_confids(exp_dataloader.dataset_path, exp_dataloader.image_ids, unc_type,
                                                      aggregation, ev.unc_ending)
            res["mean"][unc_type][aggregation] = {"metrics": {"aurc": aurc(np.array(risks), np.array(confids)),
                                                              "eaurc": eaurc(np.array(risks), np.array(confids))}}
    with open(exp_dataloader.dataset_path / "failure_detection.json", "w") as f:
        json.dump(res, f, indent=2)
    return res


# ------------------------------------------------------------------------------------------------ ambiguity modelling
def compute_ncc(gt_unc_map, pred_unc_map):
    """ncc.py:9-25 on the device: numpy's two-pass moments, in float64 whatever the maps' dtype (numpy works in the
    dtype of the map: a float32 map read back from NIfTI gives the reference a float32-rounded value, ~1e-7 away)."""
    dev = _dev()
    g, p = _float_map(gt_unc_map, dev)[0], _float_map(pred_unc_map, dev)[0]     # (an integer ground truth is a MAP here)
    if p.numel() != g.numel():
        raise ValueError("compute_ncc: maps of different size")
    (n, row), = _ncc_sums_batch([g], [p])
    return _ncc_value(n, row[2], row[3], row[4])


def _ncc_value(n, vg, vp, prod):
    """ncc.py:21-25 from the three centred sums (Python floats) of a pair of n-element maps"""
    sg, sp = np.sqrt(vg / (n - 1)), np.sqrt(vp / (n - 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(1.0) / (np.float64(n) * sg * sp) * np.float64(prod)


def _integer_dtype(a):
    dt = a.dtype
    return (not dt.is_floating_point and not dt.is_complex) if isinstance(dt, torch.dtype) else dt.kind in "biu"


def _is_rater_stack(g, p):
    """the ground-truth side of ncc_batch is a stack of label volumes (R, *spatial) when it has an integer / bool dtype
    and one axis more than the predicted map; anything else is a map"""
    return _integer_dtype(g) and g.ndim == p.ndim + 1 and tuple(g.shape[1:]) == tuple(p.shape)


def _labels(a, dev):
    """label volume(s) as a contiguous int32 device tensor; a device tensor is converted where it lies"""
    if _on_device(a):
        return a.detach().to(torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.int32)).to(dev)


def rater_variance(reference_segs):
    """np.var(reference_segs, axis=0) of integer label volumes (R, *spatial) as a float64 device map, bit for bit"""
    dev = _dev()
    lab = _labels(reference_segs, dev)
    out = torch.empty(tuple(lab.shape[1:]), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().vx_rater_variance(_lib.ptr(lab), int(lab.shape[0]), out.numel(), _lib.ptr(out), _lib.stream_ptr()),
               "vx_rater_variance")
    return out


def _ncc_sums_batch(gts, preds):
    """[(n, [sum g, sum p, sum (g-mg)^2, sum (p-mp)^2, sum (g-mg)(p-mp)])] per pair: one vx_ncc_batched call and ONE
    device -> host copy per VX_EM_MAX_ITEMS pairs"""
    lib, dev = _lib.load(), _dev()
    rows = [None] * len(gts)
    for lo in range(0, len(gts), _lib.VX_EM_MAX_ITEMS):
        members = range(lo, min(lo + _lib.VX_EM_MAX_ITEMS, len(gts)))
        keep, items = [], []
        for i in members:
            g, p = gts[i], preds[i]
            pt, pdt = _float_map(p, dev)
            if _is_rater_stack(g, p):
                gt, gdt, R = _labels(g, dev), _lib.VX_F32, int(g.shape[0])
                n_gt = gt.numel() // R
            else:
                gt, gdt = _float_map(g, dev)
                R, n_gt = 0, gt.numel()
            if n_gt != pt.numel():
                raise ValueError(f"ncc_batch: pair {i}: maps of different size")
            keep.append((gt, pt))
            items.append(_lib.NccItem(gt.data_ptr(), pt.data_ptr(), n_gt, pt.numel(), gdt, pdt, R, 0))
        arr = (_lib.NccItem * len(items))(*items)
        ws = _lib.workspace(dev, int(lib.vx_ncc_batched_workspace_bytes(arr, len(items))))
        sums = torch.empty((len(items), 5), dtype=torch.float64, device=dev)
        _lib.check(lib.vx_ncc_batched(arr, len(items), _lib.ptr(sums), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "vx_ncc_batched")
        for i, it, row in zip(members, items, sums.cpu().tolist()):
            rows[i] = (int(it.n_gt), row)
    return rows


def ncc_batch(gt_maps_or_rater_stacks, pred_maps):
    """[compute_ncc(g, p)] for a list of pairs (arrays or tensors, host or device; sizes and dtypes may differ), bit for
    bit, from one device call and one device -> host copy per batch (_ncc_sums_batch).  A ground-truth entry with an
    integer dtype and shape (R, *pred.shape) is a stack of rater label volumes: the pair's value is
    compute_ncc(np.var(stack, axis=0), p), the variance evaluated inside the kernel."""
    gts, preds = list(gt_maps_or_rater_stacks), list(pred_maps)
    if len(gts) != len(preds):
        raise ValueError("ncc_batch: lists of different length")
    return [_ncc_value(n, row[2], row[3], row[4]) for n, row in _ncc_sums_batch(gts, preds)]


def ambiguity_modeling(exp_dataloader):
    """ncc.py:28-44 (its `main`): ambiguity_modeling.json"""
    res = {"mean": {}}
    for unc_type in exp_dataloader.exp_version.unc_types:
        vals = []
        for image_id in exp_dataloader.image_ids:
            res.setdefault(image_id, {})
            ncc = float(compute_ncc(exp_dataloader.get_gt_unc_map(image_id), exp_dataloader.get_unc_map(image_id, unc_type)))
            res[image_id][unc_type] = {"metrics": {"ncc": ncc}}
            vals.append(ncc)
        res["mean"][unc_type] = {"metrics": {"ncc": float(np.mean(np.array(vals)))}}
    with open(exp_dataloader.dataset_path / "ambiguity_modeling.json", "w") as f:
        json.dump(res, f, indent=2)
    return res


# ------------------------------------------------------------------------------------------------ calibration
class _RaterInputs:
    """reference segmentations (R, *spatial), mean prediction (*spatial) and uncertainty map on the device, shaped as
    ace.py:19-29 / :104-114 shape them (a 2D map loaded as (W, H) is swapped to the prediction's (H, W))"""

    def __init__(self, reference_segs, pred_seg, unc_map, ignore_value=None):
        dev = _dev()
        self.ignore = -1 if ignore_value is None else int(ignore_value)
        if ignore_value is not None and int(ignore_value) < 0:
            raise ValueError("ignore_value must be a non-negative label")
        self.dev = dev
        if any(_on_device(a) for a in (reference_segs, pred_seg, unc_map)):
            # device inputs stay on the device: labels converted where they lie, the 2D swap as a device transpose
            ref, pred = _labels(reference_segs, dev), _labels(pred_seg, dev)
            unc, self.dtype = _float_map(unc_map if isinstance(unc_map, (np.ndarray, torch.Tensor)) else np.asarray(unc_map), dev)
            if tuple(pred.shape) != tuple(unc.shape):
                unc = unc.transpose(0, 1).contiguous()
            if tuple(ref.shape[1:]) != tuple(pred.shape) or tuple(unc.shape) != tuple(pred.shape):
                raise ValueError(f"reference {tuple(ref.shape)}, prediction {tuple(pred.shape)} and map {tuple(unc.shape)} "
                                 "do not fit together")
            self.R, self.nvox = int(ref.shape[0]), int(pred.numel())
            self.ref, self.pred, self.unc = ref, pred, unc
            return
        ref = np.asarray(reference_segs)
        pred = np.asarray(pred_seg)
        unc = unc_map.detach().cpu().numpy() if isinstance(unc_map, torch.Tensor) else np.asarray(unc_map)
        if pred.shape != unc.shape:
            unc = np.swapaxes(unc, 0, 1)
        if ref.shape[1:] != pred.shape or unc.shape != pred.shape:
            raise ValueError(f"reference {ref.shape}, prediction {pred.shape} and map {unc.shape} do not fit together")
        self.R, self.nvox = int(ref.shape[0]), int(pred.size)
        self.ref = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int32)).to(dev)
        self.pred = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.int32)).to(dev)
        self.unc, self.dtype = _float_map(unc, dev)


def _platt_sums(x: _RaterInputs, A, B, t_pos, t_neg):
    return _platt_sums_batch([x], [(A, B, t_pos, t_neg)])[0]


def _em_items(xs):
    return (_lib.EmItem * len(xs))(*[_lib.EmItem(x.unc.data_ptr(), x.ref.data_ptr(), x.pred.data_ptr(), x.nvox, x.dtype, x.R)
                                     for x in xs])


def _platt_sums_batch(xs, params):
    """the eight sums (valid and correct voxels, loss, gradient, Hessian: em_platt_body of evalmetrics.hip) for every x of
    xs at its own (A, B, t_pos, t_neg): one vx_platt_sums_batched call
    and one device -> host copy per VX_EM_MAX_ITEMS inputs"""
    lib, rows = _lib.load(), []
    for lo in range(0, len(xs), _lib.VX_EM_MAX_ITEMS):
        part, par = xs[lo:lo + _lib.VX_EM_MAX_ITEMS], params[lo:lo + _lib.VX_EM_MAX_ITEMS]
        dev, n = part[0].dev, len(part)
        items = _em_items(part)
        flat = (C.c_double * (4 * n))(*[float(v) for p in par for v in p])
        ws = _lib.workspace(dev, int(lib.vx_platt_batched_workspace_bytes(items, n)))
        sums = torch.empty((n, 8), dtype=torch.float64, device=dev)
        _lib.check(lib.vx_platt_sums_batched(items, n, flat, part[0].ignore, _lib.ptr(sums), _lib.ptr(ws), ws.numel(),
                                             _lib.stream_ptr()), "vx_platt_sums_batched")
        rows += sums.cpu().tolist()
    return rows


class _PlattFit:
    """The damped Newton iteration of sigmoid_calibration for ONE image as a state machine: `request` is the
    (A, B, t_pos, t_neg) whose eight sums it wants next, feed(sums) takes them and moves on, until `done`.  Phases (the
    evaluation that is outstanding): "counts" (valid / correct voxels), "start" (the start point), "newton" (the full
    Newton step, t = 1), "line_search" (a halved step).  sigmoid_calibration feeds it one evaluation at a time,
    sigmoid_calibration_batch feeds a whole batch of them per device call: the same arithmetic on the same sums, so the
    same (A, B) sequence.  `visited` lists the (phase, A, B, t) evaluated."""

    def __init__(self, max_iter=100):
        self.max_iter, self.iters = max_iter, 0
        self.phase, self.done, self.t = "counts", False, 1.0
        self.request = (0.0, 0.0, 0.5, 0.5)
        self.visited = []

    def _ask(self, phase, A, B):
        self.phase, self.request = phase, (float(A), float(B), self.t_pos, self.t_neg)

    def feed(self, s):
        self.visited.append((self.phase, self.request[0], self.request[1], self.t))
        if self.phase == "counts":
            self.n, n1 = s[0], s[1]
            if self.n <= 0:
                raise ValueError("sigmoid_calibration: no valid voxel")
            prior1, prior0 = n1, self.n - n1
            self.t_pos, self.t_neg = (prior1 + 1.0) / (prior1 + 2.0), 1.0 / (prior0 + 2.0)
            self.A, self.B = 0.0, float(np.log((prior0 + 1.0) / (prior1 + 1.0)))
            self._ask("start", self.A, self.B)
        elif self.phase == "start":
            self.s = s
            self._newton()
        else:
            if s[2] <= self.loss + 1e-12 * abs(self.loss) or self.t < 1e-10:
                self.A, self.B, self.s = self.trial[0], self.trial[1], s
                self.iters += 1
                self._newton()
            else:
                self.t *= 0.5
                self._trial("line_search")

    def _trial(self, phase):
        self.trial = (self.A - self.t * self.step[0], self.B - self.t * self.step[1])
        self._ask(phase, *self.trial)

    def _newton(self):
        s = self.s
        self.loss, g, H = s[2], np.array([s[3], s[4]]), np.array([[s[5], s[6]], [s[6], s[7]]])
        if self.iters >= self.max_iter or np.abs(g).max() < 1e-10 * max(1.0, self.n):
            self.done, self.request = True, None
            return
        self.step = np.linalg.solve(H + 1e-12 * np.eye(2), g)
        self.t = 1.0
        self._trial("newton")

    @property
    def result(self):
        return float(self.A), float(self.B)


def _platt_fit_one(evaluate, max_iter=100):
    """evaluate(A, B, t_pos, t_neg) -> the eight sums of one image"""
    fit = _PlattFit(max_iter)
    while not fit.done:
        fit.feed(evaluate(*fit.request))
    return fit


def _platt_fit_lockstep(n_items, evaluate, max_iter=100):
    """evaluate(indices, requests) -> the eight sums of every listed item at its request.  Every round evaluates all
    unfinished items at once; a finished item drops out of the table."""
    fits = [_PlattFit(max_iter) for _ in range(n_items)]
    active = list(range(n_items))
    while active:
        rows = evaluate(active, [fits[i].request for i in active])
        for i, s in zip(active, rows):
            try:
                fits[i].feed(s)
            except ValueError as e:
                raise ValueError(f"item {i}: {e}") from None
        active = [i for i in active if not fits[i].done]
    return fits


def sigmoid_calibration(reference_segs, pred_seg, unc_map, ignore_value=None, max_iter=100):
    """(a, b) of sklearn.calibration._sigmoid_calibration(-unc, reference == prediction) as ace.py:30-36 calls it:
    Platt's regularised targets, P = 1 / (1 + exp(a F + b)).  The objective is convex in (a, b); every evaluation
    (loss, gradient, Hessian: sums over all rater-voxels) is one device pass, the host does damped Newton steps to the
    optimum (|gradient| below 1e-10 per sample).  sklearn reaches the same optimum with BFGS (1.2.2, the reference's
    pin) or L-BFGS-B (>= 1.4) to ITS tolerance -- that difference is the only unpinned part."""
    x = _RaterInputs(reference_segs, pred_seg, unc_map, ignore_value)
    return _platt_fit_one(lambda A, B, t_pos, t_neg: _platt_sums(x, A, B, t_pos, t_neg), max_iter).result


def sigmoid_calibration_batch(ref_list, pred_list, unc_list, ignore_value=None, max_iter=100):
    """[sigmoid_calibration(ref, pred, unc, ignore_value, max_iter)] for lists of inputs (host or device), the same floats:
    the Newton iterations of all images run in lock step, one vx_platt_sums_batched call and one device -> host copy
    per round over the images that have not converged yet."""
    xs = [_RaterInputs(r, p, u, ignore_value) for r, p, u in zip(ref_list, pred_list, unc_list)]
    fits = _platt_fit_lockstep(len(xs), lambda idx, req: _platt_sums_batch([xs[i] for i in idx], req), max_iter)
    return [f.result for f in fits]


def platt_scale_confid(uncalib_confid, platt_scale_file, uncertainty):
    """ace.py:44-48 (host form, for scalars / small arrays; calc_ace fuses it into the binning pass)"""
    with open(platt_scale_file) as f:
        params = json.load(f)[uncertainty]
    return 1 / (1 + np.exp(np.asarray(uncalib_confid, dtype=np.float64) * params["a"] + params["b"]))


def calib_stats(reference_segs, pred_seg, unc_map, a, b, ignore_value=None):
    """calib_stats (ace.py:51-82) of platt_scale_confid(-unc, a, b) against "reference == prediction": bin discrepancies,
    bin weights and the number of non-empty bins; the 20 bins of np.linspace(0, 1 + 1e-8, 21)."""
    return calib_stats_batch([reference_segs], [pred_seg], [unc_map], a, b, ignore_value)[0]


def _calib_from_bins(h):
    """calib_stats' host part from the 63 numbers of one image"""
    bin_sums, bin_true, bin_total = h[:21], h[21:42], h[42:]
    n = bin_total.sum()
    if n <= 0:
        raise ValueError("calib_stats: no valid voxel")
    if bin_true.sum() == n or bin_true.sum() == 0:
        # one label only: sklearn's label_binarize(y, classes=[label])[:, 0] is a column of zeros (ace.py:68), even when
        # every voxel is correct -- reproduced
        bin_true = np.zeros_like(bin_true)
    nz = bin_total != 0
    disc = np.abs(bin_true[nz] / bin_total[nz] - bin_sums[nz] / bin_total[nz])
    return disc, bin_total[nz] / n, int(nz.sum())


def calib_stats_batch(ref_list, pred_list, unc_list, a, b, ignore_value=None):
    """[calib_stats(ref, pred, unc, a, b, ignore_value)] for lists of inputs (host or device), bit for bit: one
    vx_calib_bins_batched call and one device -> host copy per VX_EM_MAX_ITEMS images"""
    xs = [_RaterInputs(r, p, u, ignore_value) for r, p, u in zip(ref_list, pred_list, unc_list)]
    lib = _lib.load()
    e = (C.c_double * 21)(*np.linspace(0.0, 1.0 + 1e-8, 21).tolist())
    res = []
    for lo in range(0, len(xs), _lib.VX_EM_MAX_ITEMS):
        part = xs[lo:lo + _lib.VX_EM_MAX_ITEMS]
        dev, n = part[0].dev, len(part)
        items = _em_items(part)
        ab = (C.c_double * (2 * n))(*([float(a), float(b)] * n))
        ws = _lib.workspace(dev, int(lib.vx_calib_batched_workspace_bytes(items, n)))
        out = torch.empty((n, 63), dtype=torch.float64, device=dev)
        _lib.check(lib.vx_calib_bins_batched(items, n, ab, e, part[0].ignore, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                             _lib.stream_ptr()), "vx_calib_bins_batched")
        res += [_calib_from_bins(h) for h in out.cpu().numpy()]
    return res


def calc_ace(reference_segs, pred_seg, unc_map, a, b, ignore_value=None):
    """ace.py:85-87 on the device inputs: average calibration error over the non-empty bins"""
    disc, _, k = calib_stats(reference_segs, pred_seg, unc_map, a, b, ignore_value)
    return (1 / k) * np.sum(disc)


def calc_ace_batch(ref_list, pred_list, unc_list, a, b, ignore_value=None):
    """[calc_ace(ref, pred, unc, a, b, ignore_value)] from one calib_stats_batch call"""
    return [(1 / k) * np.sum(disc) for disc, _, k in calib_stats_batch(ref_list, pred_list, unc_list, a, b, ignore_value)]


def platt_scale_params(val_exp_dataloader, ignore_value=None):
    """ace.py:13-41: per uncertainty type the mean (a, b) over the validation images -> platt_scale_params.json"""
    res = {}
    for unc_type in val_exp_dataloader.exp_version.unc_types:
        aa, bb = [], []
        for image_id in val_exp_dataloader.image_ids:
            a, b = sigmoid_calibration(val_exp_dataloader.get_reference_segs(image_id),
                                       val_exp_dataloader.get_mean_pred_seg(image_id),
                                       val_exp_dataloader.get_unc_map(image_id, unc_type), ignore_value)
            aa.append(a)
            bb.append(b)
        res[unc_type] = {"a": float(np.mean(np.array(aa))), "b": float(np.mean(np.array(bb)))}
    with open(val_exp_dataloader.exp_version.exp_path / "platt_scale_params.json", "w") as f:
        json.dump(res, f, indent=2)
    return res


def calibration_error(exp_dataloader, ignore_value=None):
    """ace.py:90-131: calibration.json with the ACE per image and uncertainty type"""
    with open(exp_dataloader.exp_version.exp_path / "platt_scale_params.json") as f:
        params = json.load(f)
    res = {"mean": {}}
    for unc_type in exp_dataloader.exp_version.unc_types:
        vals = []
        for image_id in exp_dataloader.image_ids:
            res.setdefault(image_id, {})
            ace = float(calc_ace(exp_dataloader.get_reference_segs(image_id), exp_dataloader.get_mean_pred_seg(image_id),
                                 exp_dataloader.get_unc_map(image_id, unc_type), params[unc_type]["a"], params[unc_type]["b"],
                                 ignore_value))
            res[image_id][unc_type] = {"metrics": {"ace": ace}}
            vals.append(ace)
        res["mean"][unc_type] = {"metrics": {"ace": float(np.mean(np.array(vals)))}}
    with open(exp_dataloader.dataset_path / "calibration.json", "w") as f:
        json.dump(res, f, indent=2)
    return res


def calibration(exp_dataloader, ignore_value=None):
    """ace.py:134-143 (its `main`): fit the Platt parameters on the validation split if they are not there yet"""
    if not os.path.isfile(exp_dataloader.exp_version.exp_path / "platt_scale_params.json"):
        from .experiment import ExperimentDataloader
        platt_scale_params(ExperimentDataloader(exp_dataloader.exp_version, "val"), ignore_value=ignore_value)
    return calibration_error(exp_dataloader, ignore_value=ignore_value)


# ------------------------------------------------------------------------------------------------ batched drivers
def _image_chunks(exp_dataloader, batch):
    """the split's image ids in chunks of `batch`; a DeviceExperimentDataloader reads each chunk's files ahead (prefetch,
    under its byte budget) before the chunk is scored"""
    from .experiment import _chunks
    for chunk in _chunks(exp_dataloader.image_ids, batch):
        if hasattr(exp_dataloader, "prefetch"):
            exp_dataloader.prefetch(chunk)
        yield chunk


def _gt_side(exp_dataloader, image_id):
    """what ncc_batch takes for an image's ground truth: the hook's map, or in the file branch the stack of reference
    segmentations itself (a stack of a floating dtype, which numpy would not evaluate in float64, goes through
    get_gt_unc_map as before)"""
    if exp_dataloader.exp_version.gt_unc_map_loading is not None:
        return exp_dataloader.get_gt_unc_map(image_id)
    device_files = hasattr(exp_dataloader, "prefetch") and exp_dataloader.dataloader is None
    stack = exp_dataloader.get_reference_segs(image_id) if device_files else exp_dataloader._reference_segs(image_id)
    return stack if _integer_dtype(stack) else np.var(np.asarray(stack.cpu() if _on_device(stack) else stack), axis=0)


def _rater_labels(exp_dataloader, chunk):
    """int32 device reference segmentations and mean predictions of a chunk, converted once for all uncertainty types"""
    dev = _dev()
    return ([_labels(exp_dataloader.get_reference_segs(i), dev) for i in chunk],
            [_labels(exp_dataloader.get_mean_pred_seg(i), dev) for i in chunk])


def ambiguity_modeling_device(exp_dataloader, batch=32):
    """ambiguity_modeling with `batch` images per ncc_batch call: the same ambiguity_modeling.json, byte for byte.  Takes
    a DeviceExperimentDataloader (nothing but the five sums per image leaves the device) or a plain ExperimentDataloader
    (its arrays go up once)."""
    unc_types = exp_dataloader.exp_version.unc_types
    res, vals = {"mean": {}}, {u: [] for u in unc_types}
    for chunk in _image_chunks(exp_dataloader, batch):
        gts = [_gt_side(exp_dataloader, i) for i in chunk]
        for image_id in chunk:
            res.setdefault(image_id, {})
        for unc_type in unc_types:
            nccs = ncc_batch(gts, [exp_dataloader.get_unc_map(i, unc_type) for i in chunk])
            for image_id, ncc in zip(chunk, nccs):
                res[image_id][unc_type] = {"metrics": {"ncc": float(ncc)}}
                vals[unc_type].append(float(ncc))
    for unc_type in unc_types:
        res["mean"][unc_type] = {"metrics": {"ncc": float(np.mean(np.array(vals[unc_type])))}}
    with open(exp_dataloader.dataset_path / "ambiguity_modeling.json", "w") as f:
        json.dump(res, f, indent=2)
    return res


def platt_scale_params_device(val_exp_dataloader, ignore_value=None, batch=32):
    """platt_scale_params with `batch` images per lock-step fit: the same platt_scale_params.json, byte for byte"""
    unc_types = val_exp_dataloader.exp_version.unc_types
    aa, bb = {u: [] for u in unc_types}, {u: [] for u in unc_types}
    for chunk in _image_chunks(val_exp_dataloader, batch):
        refs, preds = _rater_labels(val_exp_dataloader, chunk)
        for unc_type in unc_types:
            uncs = [val_exp_dataloader.get_unc_map(i, unc_type) for i in chunk]
            for a, b in sigmoid_calibration_batch(refs, preds, uncs, ignore_value):
                aa[unc_type].append(a)
                bb[unc_type].append(b)
    res = {u: {"a": float(np.mean(np.array(aa[u]))), "b": float(np.mean(np.array(bb[u])))} for u in unc_types}
    with open(val_exp_dataloader.exp_version.exp_path / "platt_scale_params.json", "w") as f:
        json.dump(res, f, indent=2)
    return res


def calibration_error_device(exp_dataloader, ignore_value=None, batch=32):
    """calibration_error with `batch` images per calc_ace_batch call: the same calibration.json, byte for byte"""
    with open(exp_dataloader.exp_version.exp_path / "platt_scale_params.json") as f:
        params = json.load(f)
    unc_types = exp_dataloader.exp_version.unc_types
    res, vals = {"mean": {}}, {u: [] for u in unc_types}
    for chunk in _image_chunks(exp_dataloader, batch):
        refs, preds = _rater_labels(exp_dataloader, chunk)
        for image_id in chunk:
            res.setdefault(image_id, {})
        for unc_type in unc_types:
            uncs = [exp_dataloader.get_unc_map(i, unc_type) for i in chunk]
            aces = calc_ace_batch(refs, preds, uncs, params[unc_type]["a"], params[unc_type]["b"], ignore_value)
            for image_id, ace in zip(chunk, aces):
                res[image_id][unc_type] = {"metrics": {"ace": float(ace)}}
                vals[unc_type].append(float(ace))
    for unc_type in unc_types:
        res["mean"][unc_type] = {"metrics": {"ace": float(np.mean(np.array(vals[unc_type])))}}
    with open(exp_dataloader.dataset_path / "calibration.json", "w") as f:
        json.dump(res, f, indent=2)
    return res


def calibration_device(exp_dataloader, ignore_value=None, batch=32):
    """calibration with the batched drivers; the validation split is read with the class of loader it was given"""
    if not os.path.isfile(exp_dataloader.exp_version.exp_path / "platt_scale_params.json"):
        platt_scale_params_device(type(exp_dataloader)(exp_dataloader.exp_version, "val"), ignore_value=ignore_value, batch=batch)
    return calibration_error_device(exp_dataloader, ignore_value=ignore_value, batch=batch)


# ------------------------------------------------------------------------------------------------ OoD detection
def roc_auc(y_true, y_score):
    """sklearn.metrics.roc_curve + auc as auroc.py:126-127 calls them (positive label 1): one threshold per distinct
    score, cumulative true / false positive rates, trapezoid."""
    y_true = np.asarray(y_true)
    y_score = np.asarray(y_score, dtype=np.float64)
    order = np.argsort(-y_score, kind="mergesort")
    score, pos = y_score[order], y_true[order] == 1
    last = np.r_[np.where(np.diff(score))[0], len(score) - 1]      # last index of every run of equal scores
    tps = np.r_[0.0, np.cumsum(pos)[last]]
    fps = np.r_[0.0, 1 + last - np.cumsum(pos)[last]]
    if tps[-1] <= 0 or fps[-1] <= 0:
        return float("nan")
    tpr, fpr = tps / tps[-1], fps / fps[-1]
    return float(np.sum((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) * 0.5))


def is_ood_toy(sample):
    """auroc.py:18-24: in the toy data sets samples numbered up to 20 are out of distribution"""
    return not int(sample.split(".")[0]) > 20


def get_auroc_input(uncertainties, aggregation, is_ood=is_ood_toy):
    """auroc.py:79-93: (OoD labels, scores) from an aggregated_<unc>.json dict"""
    y, s = [], []
    for sample, unc in uncertainties.items():
        y.append(1 if is_ood(f"{sample.split('.')[0]}.npy") else 0)
        s.append(unc[aggregation]["max_score"])
    return y, s


def ood_auroc(exp_dataloader, is_ood=is_ood_toy):
    """the AUROC half of ood_detection (auroc.py:95-139) for every aggregated_<unc>.json; the active-learning split
    files that decide `is_ood` for the non-toy data sets are outside this build (pass your own predicate)"""
    res = {"mean": {}}
    for unc, path in exp_dataloader.get_aggregated_unc_files_dict().items():
        with open(path) as f:
            uncertainties = json.load(f)
        res["mean"][unc] = {}
        for aggregation in exp_dataloader.exp_version.aggregations:
            y, s = get_auroc_input(uncertainties, aggregation, is_ood)
            res["mean"][unc][aggregation] = {"metrics": {"auroc": roc_auc(y, s)}}
    return res
