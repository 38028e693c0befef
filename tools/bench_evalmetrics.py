"""NCC, Platt fit and ACE of a split (values_amd.evalmetrics): the per-image loop the host drivers run (compute_ncc,
sigmoid_calibration, calc_ace per image: each a batch of ONE through the same entry points) against the batch functions
(ncc_batch, sigmoid_calibration_batch, calc_ace_batch) over all images, on the same device-resident synthetic inputs, in
one process.  One JSON line per (case, score):

  case                   "3d": 32 images of 64^3, R = 4 raters;  "2d": 32 images of 256 x 478, R = 1
  score                  "ncc" (map against map), "ncc_stack" (3d only: the rater stack as ground truth; the loop forms
                         the variance map with rater_variance first), "platt", "ace"
  loop_ms_per_image      host clock around the per-image loop over the images, final synchronise included, / images
  batch_ms_per_image     the same around one batch call
  loop_launches / batch_launches        kernel launches of the library for the whole split, counted from the launchers:
                         NCC 4 per image against 4 per call; Platt 2 per evaluation against 2 per lock-step round; ACE 2
                         per image against 2 per call (ncc_stack's loop: + 1 per image for the variance map)
  loop_copies / batch_copies            blocking device -> host copies for the whole split: NCC 1 per image against 1 per
                         call; Platt 1 per evaluation against 1 per round; ACE 1 per image against 1 per call
  loop_uploads / batch_uploads          descriptor tables uploaded through the pinned staging buffer (no wait on the stream):
                         one per call, so as many as copies
  evaluations, rounds    (platt) the sum over the images of their evaluations, and the lock-step rounds (= the largest)
  loop_workspace_bytes   the call's workspace query for ONE image, what a per-image call needs
  batch_workspace_bytes  the same query for the whole batch (both are served from _lib.workspace, which holds 64 KiB at least)
  speedup                loop_ms_per_image / batch_ms_per_image

The results of the two paths are compared with `==` (nan == nan) before anything is timed.

  python tools/bench_evalmetrics.py [--iters 5] [--images 32]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--images", type=int, default=32)
    a = ap.parse_args()
    import numpy as np
    import torch

    from values_amd import _lib, evalmetrics as vm
    _lib.require_gpu()
    lib = _lib.load()
    B = a.images

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def same(x, y):
        return len(x) == len(y) and all(np.array_equal(np.asarray(p), np.asarray(q), equal_nan=True) for p, q in zip(x, y))

    for case, shape, R in (("3d", (64, 64, 64), 4), ("2d", (256, 478), 1)):
        g = torch.Generator(device="cuda").manual_seed(len(shape))
        rnd = lambda *s: torch.rand(*s, device="cuda", generator=g)
        preds, refs, uncs, gts = [], [], [], []
        for i in range(B):
            pred = (rnd(shape) < 0.3).to(torch.int32)
            flip = rnd((R,) + shape) < (0.05 + 0.01 * (i % 8))
            ref = torch.where(flip, 1 - pred[None], pred[None]).to(torch.int32)
            unc = (0.6 * flip.float().mean(0) + 0.4 * rnd(shape)).to(torch.float32)
            preds.append(pred); refs.append(ref); uncs.append(unc)
            gts.append((0.5 * unc + 0.5 * rnd(shape)).to(torch.float32))
        n = preds[0].numel()
        ncc_items = (_lib.NccItem * B)(*[_lib.NccItem(0x100, 0x100, n, n, 0, 0, 0, 0) for _ in range(B)])
        em_items = (_lib.EmItem * B)(*[_lib.EmItem(0x100, 0x100, 0x100, n, 0, R) for _ in range(B)])   # (the queries read no map)
        fits = [vm._platt_fit_one(lambda A, Bp, tp, tn, x=vm._RaterInputs(r, p, u): vm._platt_sums(x, A, Bp, tp, tn))
                for r, p, u in zip(refs, preds, uncs)]
        evals, rounds = sum(len(f.visited) for f in fits), max(len(f.visited) for f in fits)
        pa = float(np.mean([f.result[0] for f in fits])), float(np.mean([f.result[1] for f in fits]))
        scores = {
            "ncc": (lambda: [vm.compute_ncc(x, y) for x, y in zip(gts, uncs)], lambda: vm.ncc_batch(gts, uncs),
                    4 * B, 4, B, 1, lib.vx_ncc_batched_workspace_bytes, ncc_items),
            "platt": (lambda: [vm.sigmoid_calibration(r, p, u) for r, p, u in zip(refs, preds, uncs)],
                      lambda: vm.sigmoid_calibration_batch(refs, preds, uncs),
                      2 * evals, 2 * rounds, evals, rounds, lib.vx_platt_batched_workspace_bytes, em_items),
            "ace": (lambda: [vm.calc_ace(r, p, u, *pa) for r, p, u in zip(refs, preds, uncs)],
                    lambda: vm.calc_ace_batch(refs, preds, uncs, *pa),
                    2 * B, 2, B, 1, lib.vx_calib_batched_workspace_bytes, em_items)}
        if R > 1:
            scores["ncc_stack"] = (lambda: [vm.compute_ncc(vm.rater_variance(r), u) for r, u in zip(refs, uncs)],
                                   lambda: vm.ncc_batch(refs, uncs), 5 * B, 4, B, 1, *scores["ncc"][6:])
        for score, (loop, batch, ll, bl, lc, bc, query, items) in scores.items():
            assert same(batch(), loop()), f"{case} {score}: batched and per-image results differ"
            loop_ms = timed(loop, max(1, a.iters // 2))
            batch_ms = timed(batch, a.iters)
            line = {"case": case, "score": score, "images": B, "shape": list(shape), "R": R,
                    "loop_ms_per_image": round(loop_ms / B, 4), "batch_ms_per_image": round(batch_ms / B, 4),
                    "loop_launches": ll, "batch_launches": bl, "loop_copies": lc, "batch_copies": bc,
                    "loop_uploads": lc, "batch_uploads": bc, "loop_workspace_bytes": int(query(items, 1)),
                    "batch_workspace_bytes": int(query(items, B)), "speedup": round(loop_ms / batch_ms, 2)}
            if score == "platt":
                line.update(evaluations=evals, rounds=rounds)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
