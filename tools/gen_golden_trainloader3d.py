#!/usr/bin/env python3
"""Generate tests/golden/trainloader3d_kat.npz by IMPORTING the reference's two NumpyDataLoader classes
(toy_datamodule_3D.py, lidc_idri_datamodule_3D.py) and running them over the tiny trees of tests/dataset3d_trees.py (build
container only, like tools/gen_golden_dataset3d.py, whose mocks of the absent third-party packages are used here too).
batchgenerators is absent, so two stand-ins of this tool's own take its place: the base class DataLoader (_data,
batch_size, thread_id, number_of_threads_in_multithreaded -- what the reference's loader reads) and crop, which applies
the rule values_amd.datamodule3d BELIEVES batchgenerators applies and returns the origins it drew.  Recorded, as data only:

    listing|<layout>|<ids>        get_train_data_samples as path suffixes
    order|<layout>|<W>|<B>|<t>    the batches worker t of W yields at batch size B (image names), over >= 3 restarts, with
                                  the rater files random.choice picked after random.seed(RATER_SEED) and the origins the
                                  stand-in crop drew after np.random.seed(CROP_SEED)
    val|<layout>                  the validation loader's batches: image name, crop, rater file, sha1 of the float32 data
                                  and of the float32 seg

    python tools/gen_golden_trainloader3d.py [reference root]
"""
from __future__ import annotations

import hashlib
import importlib.abc
import importlib.machinery
import json
import os
import random
import sys
import tempfile
import types
from unittest.mock import MagicMock

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VALUES_REFERENCE", "")
if not os.path.isdir(REF):
    sys.exit("usage: gen_golden_trainloader3d.py <reference root>")

import numpy as np  # noqa: E402

MOCK_ROOTS = ("hydra", "omegaconf", "torchmetrics", "batchgenerators", "medpy", "pytorch_lightning", "torchvision", "cv2",
              "albumentations", "jsbeautifier", "pydantic_settings", "SimpleITK", "tqdm")
RATER_SEED, CROP_SEED = 7, 5
ORIGINS = []          # what the stand-in crop drew, in call order


class DataLoader:
    """stand-in for batchgenerators.dataloading.data_loader.DataLoader: the attributes NumpyDataLoader reads"""

    def __init__(self, data, batch_size, num_threads_in_multithreaded=1, *args, **kwargs):
        self._data = data
        self.batch_size = batch_size
        self.thread_id = 0
        self.number_of_threads_in_multithreaded = num_threads_in_multithreaded


def crop(data, seg=None, crop_size=128, margins=(0, 0, 0), crop_type="center", *args, **kwargs):
    """stand-in for batchgenerators' crop on (1, 1, X, Y, Z) arrays, crop_type "random", zero margins: per axis
    np.random.randint(0, dim - P) when dim - P > 0, else (dim - P) // 2"""
    assert crop_type == "random" and data.shape[:2] == (1, 1)
    origin = []
    for dim in data.shape[2:]:
        origin.append(int(np.random.randint(0, dim - crop_size)) if dim - crop_size > 0 else (dim - crop_size) // 2)
    ORIGINS.append(origin)
    sl = (slice(None), slice(None)) + tuple(slice(o, o + crop_size) for o in origin)
    return data[sl], (seg[sl] if seg is not None else None)


class _MockFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in MOCK_ROOTS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        if spec.name == "batchgenerators.dataloading.data_loader":
            m = types.ModuleType(spec.name)
            m.DataLoader = DataLoader
        elif spec.name == "batchgenerators.augmentations.crop_and_pad_augmentations":
            m = types.ModuleType(spec.name)
            m.crop = crop
        else:
            m = MagicMock(name=spec.name)
        m.__path__ = []
        m.__spec__ = spec
        return m

    def exec_module(self, module):
        pass


sys.meta_path.insert(0, _MockFinder())
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "uncertainty_modeling"))

from uncertainty_modeling import lidc_idri_datamodule_3D as ref_lidc  # noqa: E402
from uncertainty_modeling import toy_datamodule_3D as ref_toy  # noqa: E402

from tests import dataset3d_trees as trees  # noqa: E402

WORKERS, BATCHES = (1, 3), (1, 2, 3)      # five samples: batch sizes 2 and 3 do not divide them
IDS = sorted(n + ".npy" for n in trees.CASES)


def train_tree(td, layout, raters=None):
    base = trees.build_tree(td, layout, raters=raters)
    if layout == "toy":           # the training folders of the toy layout
        for sub in ("images", "labels"):
            os.rename(os.path.join(base, sub + "Ts"), os.path.join(base, sub + "Tr"))
    return base


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    kat = {}
    with tempfile.TemporaryDirectory() as td:
        for layout, mod in (("toy", ref_toy), ("lidc", ref_lidc)):
            base = train_tree(td, layout)
            rel = lambda p: os.path.relpath(p, base).replace(os.sep, "/")
            for tag, ids in (("none", None), ("some", ["c16.npy", "c1632.npy", "c24.npy", "other.npy", "absent.npy"]), ("all", IDS)):
                s = mod.get_train_data_samples(base_dir=base, pattern=trees.PATTERN, subject_ids=ids, num_raters=3)
                kat[f"listing|{layout}|{tag}"] = [[rel(x["image_path"]), None if x["label_paths"] is None else [rel(p) for p in x["label_paths"]]]
                                                  for x in s]
            # the loaders run over trees in which every case has all three raters (a batch that mixes cases with and
            # without labels ends the reference's loader in np.asarray)
            base = train_tree(os.path.join(td, "full"), layout, {n: [0, 1, 2] for n in trees.CASES})
            for W in WORKERS:
                for B in BATCHES:
                    if len(IDS) <= (W - 1) * B:      # the last worker would start past the end: the reference recurses for ever
                        continue
                    for t in range(W):
                        dl = mod.NumpyDataLoader(base_dir=base, batch_size=B, patch_size=trees.PATCH, file_pattern=trees.PATTERN,
                                                 subject_ids=IDS, training=True, num_raters=3)
                        dl.thread_id, dl.number_of_threads_in_multithreaded = t, W
                        random.seed(RATER_SEED)
                        np.random.seed(CROP_SEED)
                        del ORIGINS[:]
                        rows = []
                        while dl.num_restarted < 4 or len(rows) < 8:
                            n0 = len(ORIGINS)
                            b = dl.generate_train_batch()
                            assert b["data"].shape[1:] == (1,) + (trees.PATCH,) * 3
                            rows.append({"images": [rel(p) for p in b["image_paths"]], "raters": [rel(p) for p in b["label_paths"]],
                                         "origins": ORIGINS[n0:], "restarts": dl.num_restarted})
                        kat[f"order|{layout}|{W}|{B}|{t}"] = rows
            dl = mod.NumpyDataLoader(base_dir=base, batch_size=1, patch_size=trees.PATCH, file_pattern=trees.PATTERN, subject_ids=IDS,
                                     training=False, num_raters=3)
            random.seed(RATER_SEED)
            rows = []
            for s in list(dl._data):
                b = dl.generate_train_batch()
                assert b["image_paths"] == [s["image_path"]]
                rows.append({"image": rel(s["image_path"]), "crop": [[int(v) for v in ax] for ax in s["crop_idx"]],
                             "raters": [rel(p) for p in b["label_paths"]], "data": sha(b["data"].astype(np.float32)),
                             "data_shape": list(b["data"].shape),
                             "seg": sha(b["seg"].astype(np.float32)) if b["label_paths"] else None})
            kat[f"val|{layout}"] = rows
            assert len(dl) == len(rows)
    kat["seeds"] = {"rater": RATER_SEED, "crop": CROP_SEED}
    path = os.path.join(ROOT, "tests", "golden", "trainloader3d_kat.npz")
    np.savez_compressed(path, kat=np.frombuffer(json.dumps(kat).encode(), dtype=np.uint8))
    print("trainloader3d_kat.npz", os.path.getsize(path), "bytes;", len(kat), "records")


if __name__ == "__main__":
    main()
