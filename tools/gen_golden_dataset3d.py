#!/usr/bin/env python3
"""Generate tests/golden/dataset3d_kat.npz by IMPORTING the reference and running its own functions over the tiny trees of
tests/dataset3d_trees.py (build container only, like tools/gen_golden.py, whose mocks of the absent third-party packages
are used here too; none of them is on the path captured below):

    listing   get_val_test_data_samples of toy_datamodule_3D and lidc_idri_datamodule_3D, as path suffixes and crop tuples,
              for subject_ids None / given, patch overlaps 1, 0.5 and 0.25
    <case>_data / _seg / _num   what DataCarrier3D.concat_data builds for three cases fed patch by patch through
              DataCarrier3D.load_image (the un-normalised float64 / intc sums and the count)

    python tools/gen_golden_dataset3d.py [reference root]
"""
from __future__ import annotations

import importlib.abc
import importlib.machinery
import json
import os
import sys
import tempfile
from unittest.mock import MagicMock

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"

MOCK_ROOTS = ("hydra", "omegaconf", "torchmetrics", "batchgenerators", "medpy", "pytorch_lightning", "torchvision", "cv2",
              "albumentations", "jsbeautifier", "pydantic_settings", "SimpleITK", "tqdm")


class _MockFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in MOCK_ROOTS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = MagicMock(name=spec.name)
        m.__path__ = []
        m.__spec__ = spec
        return m

    def exec_module(self, module):
        pass


sys.meta_path.insert(0, _MockFinder())
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "uncertainty_modeling"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from uncertainty_modeling.data_carrier_3D import DataCarrier3D  # noqa: E402
from uncertainty_modeling.lidc_idri_datamodule_3D import get_val_test_data_samples as ref_samples_lidc  # noqa: E402
from uncertainty_modeling.toy_datamodule_3D import get_val_test_data_samples as ref_samples_toy  # noqa: E402

from tests import dataset3d_trees as trees  # noqa: E402

COMPOSITE_CASES = ("c1632", "c24", "c2416")


def main():
    out = {}
    listing = {}
    with tempfile.TemporaryDirectory() as td:
        for layout, fn in (("toy", ref_samples_toy), ("lidc", ref_samples_lidc)):
            base = trees.build_tree(td, layout)
            for overlap in (1, 0.5, 0.25):
                for tag, ids in (("none", None), ("some", ["c16.npy", "c1632.npy", "c24.npy", "other.npy", "absent.npy"])):
                    s = fn(base_dir=base, pattern=trees.PATTERN, subject_ids=ids, num_raters=3, test=True, patch_size=trees.PATCH,
                           patch_overlap=overlap)
                    listing[f"{layout}|{overlap}|{tag}"] = trees.listing_key(s, base)
        base = trees.build_tree(os.path.join(td, "comp"), "toy", raters={n: [0, 1, 2] for n in trees.CASES})
        for name in COMPOSITE_CASES:
            samples = [s for s in ref_samples_toy(base_dir=base, pattern=name + ".npy", num_raters=3, test=True, patch_size=trees.PATCH,
                                                  patch_overlap=trees.CASES[name][2])]
            dc = DataCarrier3D()
            for s in samples:
                inp = DataCarrier3D.load_image(s)
                batch = dict(inp, data=torch.from_numpy(np.expand_dims(inp["data"], 0).copy()), seg=torch.from_numpy(inp["seg"].copy()))
                dc.concat_data(batch=batch, softmax_pred=torch.zeros((1, 2) + (trees.PATCH,) * 3, dtype=torch.float64), n_pred=1, pred_idx=0)
            (v,) = dc.data.values()
            out[name + "_data"], out[name + "_seg"], out[name + "_num"] = v["data"], v["seg"], v["num_predictions"][0]
            out[name + "_crops"] = np.array([s["crop_idx"] for s in samples], dtype=np.int32)
            print(name, len(samples), "patches; count max", v["num_predictions"].max(), v["data"].dtype, v["seg"].dtype)
    out["listing"] = np.frombuffer(json.dumps(listing).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "dataset3d_kat.npz")
    np.savez_compressed(path, **out)
    print("dataset3d_kat.npz", os.path.getsize(path), "bytes;", {k: len(v) for k, v in listing.items()})


if __name__ == "__main__":
    main()
