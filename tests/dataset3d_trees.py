"""The tiny 3D test-split trees shared by tools/gen_golden_dataset3d.py (which runs the reference over them) and the
dataset3d tests (which run this project over them): closed-form cases, both datamodules' folder layouts."""
import os

import numpy as np

from tests.formula import formula_tensor, formula_volume

PATCH = 16
# name -> (shape, stored image dtype, patch_overlap the case is listed with)
CASES = {"c16": ((16, 16, 16), "float32", 1), "c32": ((32, 16, 16), "int16", 1), "c1632": ((16, 32, 24), "float64", 1),
         "c24": ((24, 24, 24), "float32", 0.5), "c2416": ((24, 16, 16), "float64", 0.25)}
LABEL_DTYPES = ("uint8", "int32", "int64")          # the stored dtype of rater 0, 1, 2
# the listing tests' raters: all three, a missing middle one, none at all
LISTING_RATERS = {"c16": [0, 1, 2], "c32": [0, 2], "c1632": [], "c24": [0, 1], "c2416": [0]}
PATTERN = "c*.npy"                                  # filters out other.npy


def image(name):
    shape, dtype, _ = CASES[name]
    tag = 100 + sorted(CASES).index(name)
    if dtype == "float64":   # full 53-bit mantissas: d + d + d rounds, so (d + d + d) / 3 != d in places
        return formula_volume(shape, tag=tag) + formula_tensor(shape, tag + 50) / 3.0
    if dtype == "int16":
        return np.round(formula_volume(shape, tag=tag) * 900).astype(np.int16)
    return formula_volume(shape, tag=tag).astype(dtype)


def label(name, rater):
    shape = CASES[name][0]
    tag = 200 + 10 * sorted(CASES).index(name) + rater
    return (formula_volume(shape, tag=tag) > 0.3 * (rater + 1)).astype(LABEL_DTYPES[rater])


def label_name(name, rater, layout):
    return f"{name}_{str(rater).zfill(2)}.npy" if layout == "toy" else f"{name}_{str(rater).zfill(2)}_mask.npy"


def build_tree(root, layout, raters=None, names=None):
    """-> base_dir of a tree in the layout of the toy ("toy": imagesTs / labelsTs) or the LIDC ("lidc": images / labels)
    datamodule: the images of `names` (default: all), the rater files raters[name], and other.npy"""
    raters = LISTING_RATERS if raters is None else raters
    names = list(CASES) if names is None else list(names)
    base = os.path.join(str(root), layout)
    idir, ldir = (("imagesTs", "labelsTs") if layout == "toy" else ("images", "labels"))
    os.makedirs(os.path.join(base, idir))
    os.makedirs(os.path.join(base, ldir))
    for name in names:
        np.save(os.path.join(base, idir, name + ".npy"), image(name))
        for r in raters[name]:
            np.save(os.path.join(base, ldir, label_name(name, r, layout)), label(name, r))
    np.save(os.path.join(base, idir, "other.npy"), np.zeros((16, 16, 16), dtype=np.float32))
    return base


def listing_key(samples, base):
    """a listing as data: [image path suffix, [label path suffixes] or None, crop]"""
    rel = lambda p: os.path.relpath(p, base).replace(os.sep, "/")
    return [[rel(s["image_path"]), None if s["label_paths"] is None else [rel(p) for p in s["label_paths"]],
             [list(int(v) for v in ax) for ax in s["crop_idx"]]] for s in samples]
