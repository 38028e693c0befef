#!/usr/bin/env python3
"""Randomised shapes through the streaming kernels (transposed conv, InstanceNorm apply / pool / concat / fan-out) by
calling the parity tests' bodies with random parameters.      python tools/fuzz_misc.py [cases] [seed]"""
import os, random, sys, traceback
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(16)
from tests import test_gpu_kernels as T
from tests import test_gpu_stream3d as S3
from tests import ops3d_ref as R3
from values_amd._lib import VxError

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 150
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
bad = unsupported = 0
for case in range(cases):
    kind = rng.choice(["convT", "norm", "norm", "c1"])
    try:
        if kind == "convT":
            cin = rng.choice([16, 32, 64, 128, 8, 24, 48])
            cout = rng.choice([8, 16, 32, 64, 24, 40])   # multiples of 8 (others: packed_floats() = -1)
            shape = (rng.randint(1, 3), rng.randint(1, 5), rng.randint(1, 9), rng.randint(1, 17))
            tag = f"convT {cin}->{cout} {shape}"
            T.test_convT_matches_oracle(cin, cout, shape)
        elif kind == "norm":
            # instance, activation, dropout mode, concat input / output, pool-only and the _stats form, through the body of
            # tests/test_gpu_stream3d.py::test_norm_matrix (bits against the float32 restatement, float64 against its bound)
            inst = rng.choice(sorted(R3.INSTANCES))
            pool = R3.INSTANCES[inst][1]
            c = rng.choice(R3.C_WIDE if inst.startswith("wide") else R3.C_SHUFFLE if pool else R3.C_NOPOOL + (256, 12))
            layout = rng.choice(R3._POOL_LAYOUTS if pool else R3._COMMON_LAYOUTS)
            lay = R3.parse_layout(layout)
            xb = max(lay["out_xblk"], lay["x_xblk"], 1)
            if pool:
                shape = (rng.randint(1, 3), 2 * rng.randint(1, 4), 2 * rng.randint(1, 6), 2 * xb * rng.randint(1, 5))
            else:
                shape = (rng.randint(1, 3), rng.randint(1, 7), rng.randint(1, 11), xb * rng.randint(1, 21 // xb))
            act, drop = rng.randint(0, 2), rng.randint(0, 2)
            repeat = rng.choice([2, 3, 5]) if inst == "fanout" else 1
            tiles = rng.choice([1, 2, 5, 37, 300])
            tag = f"norm {inst} C={c} {shape} act={act} drop={drop} {layout} tiles={tiles} x{repeat}"
            S3.norm_case_body(inst, c, shape, act, drop, layout, tiles, repeat)
        else:
            cout = rng.choice([8, 16, 32])
            shape = (rng.randint(1, 3), rng.randint(1, 9), rng.randint(1, 20), rng.randint(1, 40))
            flip = rng.randint(0, 7)
            tag = f"c1 ->{cout} {shape} flip={flip}"
            T.test_conv3d_c1_matches_oracle(cout, shape, flip)
    except VxError as e:
        unsupported += 1
        print(f"rejected ({tag}): {e}")
    except Exception:
        bad += 1
        print(f"FAIL case {case}: {tag}")
        traceback.print_exc(limit=2)
print(f"{cases} cases, {bad} failures, {unsupported} rejected loudly")
sys.exit(1 if bad else 0)
