"""Generate tests/golden/label_switch_kat.npz by IMPORTING the reference's StochasticLabelSwitches
(uncertainty_modeling/augmentations.py) and running its apply_to_mask after np.random.seed.

    python tools/gen_golden_labelswitch.py --reference <checkout of the reference>

albumentations is absent: the class needs it only for its base class, so a stub module with an empty BasicTransform
stands in (this project's code; the reference's class body runs unchanged).  The fixture is data only: three small int64
label maps, the numpy seeds, n_reference_samples in {1, 5} and the recorded outputs, each with the binomial draws made.
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = np.array([0, 1, 2, 5, 8, 11, 13, 255], dtype=np.int64)
SIZES = [(6, 7), (17, 33), (1, 1)]
SEEDS = [0, 1, 7, 123]
RS = [1, 5]


def import_reference_class(reference):
    stub = types.ModuleType("albumentations")

    class BasicTransform:
        def __init__(self, always_apply=False, p=0.5):
            self.always_apply, self.p = always_apply, p

    stub.BasicTransform = BasicTransform
    sys.modules["albumentations"] = stub
    sys.path.insert(0, reference)
    from uncertainty_modeling.augmentations import StochasticLabelSwitches
    return StochasticLabelSwitches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "label_switch_kat.npz"))
    args = ap.parse_args()
    cls = import_reference_class(args.reference)
    rng = np.random.default_rng(20)
    out = {"seeds": np.array(SEEDS, dtype=np.int64), "n_reference_samples": np.array(RS, dtype=np.int64)}
    for m, (h, w) in enumerate(SIZES):
        mask = IDS[rng.integers(0, len(IDS), size=(h, w))]
        if m == 1:
            mask[0, :len(IDS)] = IDS   # every id is present in the larger map
        out[f"mask_{m}"] = mask
        for seed in SEEDS:
            for r in RS:
                t = cls(n_reference_samples=r)
                np.random.seed(seed)
                got = t.apply_to_mask(mask)
                np.random.seed(seed)   # the class's draws equal this sequence: per reference, then per class in dict order
                draws = np.array([[np.random.binomial(1, p, 1)[0] for p in t._label_switches.values()] for _ in range(r)], dtype=np.uint8)
                out[f"out_{m}_{seed}_{r}"] = np.asarray(got)
                out[f"draws_{seed}_{r}"] = draws
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
