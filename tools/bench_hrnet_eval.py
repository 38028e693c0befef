#!/usr/bin/env python3
"""What eval mode is worth on the 2D path: one HRNet forward in train mode (batch statistics: today's launches), in eval mode
on the unfused route (raw conv + vx_affine_gather fed from the running-statistics table, VX_HRNET_NO_FOLD=1) and in eval mode
with the BatchNorm affine, residual and ReLU in the conv epilogue -- all three in ONE process, each captured into a hipGraph
(the eager walk is host-bound), timed with HIP events around blocks of replays, the modes interleaved round by round so that
clock drift and neighbours on the machine hit all three alike.

    python tools/bench_hrnet_eval.py [--rounds 6] [--only w18|w18_tta|w48]

Prints one JSON line per configuration: ms per step (median over the rounds, with the min / max as the spread), library
launches per forward (counted on an eager walk) and images/s for each mode, plus whether the two eval routes gave the same
bits.  The baseline is train mode measured here, in the same process."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from values_amd import _lib  # noqa: E402
from values_amd.hrnet import HighResolutionNet  # noqa: E402
from values_amd.hrnet_configs import hrnet_w18_extra, hrnet_w48_extra  # noqa: E402

CONFIGS = {   # name -> (extra, classes, images, views, H, W, replays per timed block)
    "w18": (lambda: hrnet_w18_extra(False), 19, 8, 1, 512, 1024, 16),
    "w18_tta": (lambda: hrnet_w18_extra(False), 19, 8, 8, 512, 1024, 3),
    "w48": (lambda: hrnet_w48_extra(False), 24, 12, 1, 256, 478, 16),
}
MODES = ("train", "eval_unfused", "eval_fused")


def set_mode(model, mode):
    model.train(mode == "train")
    if mode == "eval_unfused":
        os.environ["VX_HRNET_NO_FOLD"] = "1"
    else:
        os.environ.pop("VX_HRNET_NO_FOLD", None)


def count_launches(fn):
    n, orig = [0], _lib.check

    def counting(rc, what=""):
        n[0] += 1
        return orig(rc, what)

    _lib.check = counting
    try:
        fn()
    finally:
        _lib.check = orig
    return n[0]


def calibrate(model, x):
    """running statistics = the batch statistics of one train-mode forward (read back from the scale / shift rows the walk
    computes), so that the eval forwards see activations of the size the train forward sees: the clock the chip holds
    depends on the data, and a random-weight network without renormalisation decays towards zeros"""
    rec, orig = {}, model._conv_bn

    def spy(x_, conv_name, bn_name, pre=None):
        r = orig(x_, conv_name, bn_name, pre=pre)
        rec[bn_name] = (r[1], r[2])
        return r

    model._conv_bn = spy
    try:
        model.train()
        model.forward_samples(x, 1)
        torch.cuda.synchronize()
    finally:
        del model._conv_bn
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                sc, sh = (t.reshape(-1)[:c].double() for t in rec[name])
                m.running_var.copy_(((m.weight.double() / sc) ** 2 - m.eps).clamp_min(1e-6).float())
                m.running_mean.copy_(((m.bias.double() - sh) / sc).float())


def bench(name, rounds):
    extra, ncls, images, views, H, W, reps = CONFIGS[name]
    torch.manual_seed(0)
    model = HighResolutionNet({"MODEL": {"EXTRA": extra(), "ALIGN_CORNERS": False, "INPUT_CHANNELS": 3},
                               "DATASET": {"NUM_CLASSES": ncls}}).cuda()
    n = images * views
    x = torch.randn(n, 3, H, W, device="cuda")
    calibrate(model, x[:images])
    kw = dict(groups=views, group_flips=[v % 4 for v in range(views)]) if views > 1 else {}
    side = torch.cuda.Stream()
    graphs, outs, launches, keep = {}, {}, {}, []
    for mode in MODES:
        set_mode(model, mode)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):     # warm-up on the capture stream: packed weights, tables, zero-tail buffers, side streams
            model.forward_samples(x, 1, **kw)
            launches[mode] = count_launches(lambda: model.forward_samples(x, 1, **kw))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            outs[mode] = model.forward_samples(x, 1, **kw)
        keep.append(model._hold_last)
        model._hold_last = None
        graphs[mode] = g
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    for mode in MODES:                    # every graph warm before the timed rounds
        graphs[mode].replay()
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["eval_unfused"], outs["eval_fused"]))
    ms = {mode: [] for mode in MODES}
    for r in range(rounds):
        order = MODES[r % 3:] + MODES[:r % 3]
        for mode in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                graphs[mode].replay()
            e1.record()
            e1.synchronize()
            ms[mode].append(e0.elapsed_time(e1) / reps)
    res = {"config": name, "images": images, "views": views, "size": [H, W], "rounds": rounds, "replays_per_block": reps,
           "eval_routes_same_bits": same}
    for mode in MODES:
        med = statistics.median(ms[mode])
        res[mode] = {"ms_per_step": round(med, 3), "min_ms": round(min(ms[mode]), 3), "max_ms": round(max(ms[mode]), 3),
                     "launches_per_forward": launches[mode], "images_per_s": round(images / med * 1e3, 1)}
    res["eval_fused_over_train"] = round(res["eval_fused"]["ms_per_step"] / res["train"]["ms_per_step"], 4)
    print(json.dumps(res), flush=True)
    os.environ.pop("VX_HRNET_NO_FOLD", None)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--only", choices=sorted(CONFIGS), default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    for cfg in ([args.only] if args.only else ["w18", "w18_tta", "w48"]):
        bench(cfg, args.rounds)
        torch.cuda.empty_cache()
