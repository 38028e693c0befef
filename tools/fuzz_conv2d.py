#!/usr/bin/env python3
"""Randomised shapes through vx_conv2d (HRNet path).     python tools/fuzz_conv2d.py [cases] [seed] [kind]

kind `plain` (default): split-fp16 (default) and native-fp32 kernels against a float64 F.conv2d on the device's host,
statistics partials included.
kind `pre`: the input prologue (vx_conv2d_args.in_scale / in_shift / in_relu / in_cpitch / in_group_images) of the split-fp16
kernels on conv -> BN -> (ReLU) -> conv chains -- equal bits to vx_affine_gather + vx_conv2d, and the float64 oracle on the
restated activated tensor (tests/test_gpu_ops2d.py: prologue_case)."""
import os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from values_amd import _lib


def run_cases(cases, seed):
    from tests.test_gpu_kernels2d import run_conv2d
    rng = random.Random(seed)
    bad = 0
    for case in range(cases):
        ks, s = rng.choice([(3, 1), (3, 1), (3, 2), (1, 1)])
        cin = rng.choice([3, 5, 8, 16, 17, 18, 24, 25, 32, 36, 48, 64, 72, 96, 144, 192, 270]) if ks == 3 else rng.choice([16, 18, 48, 64, 96, 256, 270, 720])
        cout = rng.choice([16, 18, 32, 36, 48, 64, 72, 96, 144, 19, 4, 24, 128] + ([240, 320, 720] if ks == 1 else []))
        n = rng.randint(1, 3)
        h, w = rng.randint(1, 40), rng.randint(1, 70)
        g = torch.Generator().manual_seed(case)
        x = torch.randn((n, cin, h, w), generator=g)
        wt = torch.randn((cout, cin, ks, ks), generator=g) * (1.0 / (ks * ks * cin)) ** 0.5
        b = torch.randn((cout,), generator=g) * 0.2 if rng.random() < 0.4 else None
        ref = F.conv2d(x.double(), wt.double(), None if b is None else b.double(), stride=s, padding=ks // 2)
        tag = f"case {case}: {cin}->{cout} k{ks} s{s} n={n} {h}x{w} bias={b is not None}"
        if os.environ.get("FUZZ_VERBOSE"):
            print(tag, flush=True)
        for mode in (0, 1):
            try:
                with _lib.config(conv_fp32=mode):
                    got, st, _ = run_conv2d(x, wt, b, ks, s, narrow=bool(case & 1))
            except Exception as e:
                print(f"ERROR {tag} mode={mode}: {e}")
                bad += 1
                continue
            err = (got.double() - ref).abs().max().item()
            ssum = st.double().sum(0)
            e1 = (ssum[:, 0] - ref.sum((0, 2, 3))).abs().max().item()
            e2 = (ssum[:, 1] - (ref * ref).sum((0, 2, 3))).abs().max().item()
            tol = 3e-5 * max(1.0, ref.abs().max().item())
            stol = 2e-3 + 1e-4 * (ref * ref).sum((0, 2, 3)).max().item()
            if got.shape != ref.shape or err > tol or e1 > stol or e2 > stol or torch.isnan(got).any():
                bad += 1
                print(f"FAIL {tag} mode={mode}: err {err:.2e} stats {e1:.2e} {e2:.2e}")
    return cases, bad


def run_pre_cases(cases, seed):
    """-> (cases, failures, the kernel instances that ran)"""
    from tests.test_gpu_ops2d import prologue_case
    rng = random.Random(seed)
    bad, names = 0, set()
    for case in range(cases):
        ks, s = rng.choice([(3, 1), (3, 1), (3, 2), (1, 1)])
        cin = rng.choice([5, 8, 16, 17, 18, 24, 32, 36, 48, 64, 72, 96, 144]) if ks == 3 else rng.choice([16, 18, 48, 64, 96, 144, 270])
        cout = rng.choice([16, 18, 32, 36, 48, 64, 72, 19, 4, 24])
        gi = rng.choice([0, 0, 1, 2, 3])
        n = gi * rng.randint(1, 2) if gi else rng.randint(1, 3)
        h, w = rng.randint(3, 40), rng.randint(3, 50)
        opt = dict(narrow=rng.random() < 0.5, gi=gi, relu=rng.random() < 0.8, tag=5000 + 10 * case)
        cfg = dict(c2s_no_oct=int(rng.random() < 0.25), c2s_no_wide=int(rng.random() < 0.25))
        tag = f"case {case}: {cin}->{cout} k{ks} s{s} n={n} {h}x{w} {opt} {cfg}"
        if os.environ.get("FUZZ_VERBOSE"):
            print(tag, flush=True)
        try:
            with _lib.config(conv_fp32=0, **cfg):
                names.add(prologue_case(cin, cout, ks, s, n, h, w, **opt))
        except AssertionError as e:      # (a VxError or a HIP error ends the run: nothing more is started on the device)
            bad += 1
            print(f"FAIL {tag}: {e}")
    return cases, bad, names


if __name__ == "__main__":
    torch.set_num_threads(16)
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 150
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    kind = sys.argv[3] if len(sys.argv) > 3 else "plain"
    if kind == "pre":
        cases, bad, names = run_pre_cases(cases, seed)
        print("instances:", ", ".join(sorted(names)))
    else:
        cases, bad = run_cases(cases, seed)
    print(f"{cases} cases, {bad} failures")
    sys.exit(1 if bad else 0)
