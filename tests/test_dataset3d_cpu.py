"""CPU: the 3D test split's host mirror (values_amd.dataset3d) against tests/golden/dataset3d_kat.npz, which
tools/gen_golden_dataset3d.py filled by running the reference's own get_val_test_data_samples (both datamodules),
DataCarrier3D.load_image and DataCarrier3D.concat_data over the trees of tests/dataset3d_trees.py."""
import json
import os
import pickle

import numpy as np
import pytest

from tests import dataset3d_trees as trees
from tests.helpers import load_npz

SOME = ["c16.npy", "c1632.npy", "c24.npy", "other.npy", "absent.npy"]


@pytest.fixture(scope="module")
def kat():
    g = load_npz("dataset3d_kat.npz")
    return g, json.loads(bytes(g["listing"]).decode())


@pytest.mark.parametrize("layout", ["toy", "lidc"])
def test_listing_equals_the_reference(tmp_path, kat, layout):
    from values_amd.dataset3d import cases, get_val_test_data_samples
    _, listing = kat
    base = trees.build_tree(tmp_path, layout)
    for overlap in (1, 0.5, 0.25):
        for tag, ids in (("none", None), ("some", SOME)):
            s = get_val_test_data_samples(base, pattern=trees.PATTERN, subject_ids=ids, num_raters=3, test=True,
                                          patch_size=trees.PATCH, patch_overlap=overlap, layout=layout)
            assert trees.listing_key(s, base) == listing[f"{layout}|{overlap}|{tag}"], (layout, overlap, tag)
    # what the fixture pins, spelled out: subject_ids=None lists everything in the toy layout and nothing in the LIDC one
    s = get_val_test_data_samples(base, pattern=trees.PATTERN, subject_ids=None, num_raters=3, test=True, patch_size=16, layout=layout)
    names = [os.path.basename(x["image_path"]) for x in s]
    assert names == (["c16.npy", "c1632.npy", "c1632.npy", "c24.npy", "c2416.npy", "c32.npy", "c32.npy"] if layout == "toy" else [])
    s = get_val_test_data_samples(base, pattern=trees.PATTERN, subject_ids=SOME + ["c32.npy"], num_raters=3, test=True, patch_size=16,
                                  layout=layout)
    by = {os.path.basename(x["image_path"]): x for x in s}
    assert "other.npy" not in by                                        # listed in subject_ids, filtered by the pattern
    suffix = ".npy" if layout == "toy" else "_mask.npy"
    assert [os.path.basename(p) for p in by["c32.npy"]["label_paths"]] == ["c32_00" + suffix, "c32_02" + suffix]   # the middle rater is missing
    assert by["c1632.npy"]["label_paths"] is None                       # no rater at all
    assert len(by["c16.npy"]["label_paths"]) == 3
    assert [x["crop_idx"] for x in s if x["image_path"].endswith("c32.npy")] == [((0, 16), (0, 16), (0, 16)), ((16, 32), (0, 16), (0, 16))]
    # the same layout read as the other datamodule's finds no folder
    with pytest.raises(StopIteration):
        get_val_test_data_samples(base, test=True, layout="lidc" if layout == "toy" else "toy")
    with pytest.raises(ValueError):
        get_val_test_data_samples(base, layout="both")
    # case records: from the headers alone
    cs = cases(s)
    assert [c["image_id"] for c in cs] == ["c16", "c1632", "c24", "c32"]
    c = cs[1]
    assert c["shape"] == (16, 32, 24) and c["dtype"] == np.float64 and c["label_paths"] == [] and len(c["crops"]) == 2
    assert [str(d) for d in cs[0]["label_dtypes"]] == ["uint8", "int32", "int64"] and cs[3]["dtype"] == np.int16


def test_io_seams_resolve_to_both_listings(tmp_path):
    from values_amd.io import instantiate
    for layout, mod in (("toy", "toy_datamodule_3D"), ("lidc", "lidc_idri_datamodule_3D")):
        base = trees.build_tree(tmp_path, layout)
        for prefix in ("uncertainty_modeling.", ""):
            s = instantiate({"_target_": f"{prefix}{mod}.get_val_test_data_samples"}, base_dir=base, subject_ids=["c16.npy"],
                            num_raters=3, test=True, patch_size=16)
            assert len(s) == 1 and os.path.basename(s[0]["label_paths"][0]) == trees.label_name("c16", 0, layout)


def test_split_resolvers(tmp_path):
    from values_amd.dataset3d import dir_and_subjects_from_train, dir_and_subjects_from_train_lidc
    root = tmp_path / "data"
    (root / "toy3d").mkdir(parents=True)
    splits = [{"train": ["a.npy"], "val": ["b.npy"], "id_test": ["c.npy"], "ood_test": ["d.npy"],
               "id_unlabeled_pool": np.array(["e.npy"]), "ood_unlabeled_pool": np.array(["f.npy", "g.npy"])},
              {"train": ["z.npy"], "val": [], "id_test": ["y.npy"], "ood_test": [], "id_unlabeled_pool": np.array([]),
               "ood_unlabeled_pool": np.array([])}]
    for p in (root / "toy3d" / "splits.pkl", root / "splits_malignancy.pkl", root / "all", root / "my_splits.pkl"):
        with open(p, "wb") as f:
            pickle.dump(splits, f)
    hp = {"data_input_dir": str(root), "datamodule": {"dataset_name": "toy3d", "data_fold_id": 0}}
    assert dir_and_subjects_from_train(hp, test_split="id_test") == (str(root / "toy3d" / "preprocessed"), ["c.npy"])
    hp1 = {"data_input_dir": "/somewhere/else", "datamodule": {"dataset_name": "toy3d", "data_fold_id": 1}}
    assert dir_and_subjects_from_train(hp1, data_input_dir=str(root), test_split="train") == (str(root / "toy3d" / "preprocessed"), ["z.npy"])
    # LIDC: splits_<shift>.pkl, "all" without a shift feature, the test-split branches
    hl = {"data_input_dir": str(root), "datamodule": {"shift_feature": "malignancy", "data_fold_id": 0}}
    d, ids = dir_and_subjects_from_train_lidc(hl, test_split="id")
    assert d == str(root / "preprocessed") and ids == ["c.npy"]
    assert dir_and_subjects_from_train_lidc(hl, test_split="ood")[1] == ["d.npy"]
    assert dir_and_subjects_from_train_lidc(hl, test_split="val")[1] == ["b.npy"]
    assert dir_and_subjects_from_train_lidc(hl, test_split="train")[1] == ["a.npy"]
    assert list(dir_and_subjects_from_train_lidc(hl, test_split="unlabeled")[1]) == ["e.npy", "f.npy", "g.npy"]
    hn = {"data_input_dir": str(root), "datamodule": {"shift_feature": None, "data_fold_id": 0, "splits_path": None}}
    assert dir_and_subjects_from_train_lidc(hn)[1] == ["c.npy"]
    # splits_path: used as it is, or with the training-time data_input_dir replaced by the given one
    hs = {"data_input_dir": "/train/time/dir", "datamodule": {"shift_feature": "malignancy", "data_fold_id": 0,
                                                                "splits_path": "/train/time/dir/my_splits.pkl"}}
    d, ids = dir_and_subjects_from_train_lidc(hs, data_input_dir=str(root), test_split="id")
    assert d == str(root / "preprocessed") and ids == ["c.npy"]
    with pytest.raises(FileNotFoundError):
        dir_and_subjects_from_train_lidc(hs)
    hs2 = dict(hs, data_input_dir=str(root), datamodule=dict(hs["datamodule"], splits_path=str(root / "my_splits.pkl")))
    assert dir_and_subjects_from_train_lidc(hs2)[1] == ["c.npy"]


@pytest.mark.parametrize("name", ["c1632", "c24", "c2416"])
def test_compose_case_equals_concat_data(kat, name):
    from values_amd.dataset3d import compose_case
    g, _ = kat
    img = trees.image(name)
    labels = [trees.label(name, r) for r in range(3)]
    crops = [tuple(tuple(int(v) for v in ax) for ax in c) for c in g[name + "_crops"]]
    from values_amd import crop_indices
    assert crops == crop_indices(img.shape, trees.PATCH, trees.CASES[name][2])
    c = compose_case(img, labels, crops)
    num, clip = g[name + "_num"], np.clip(g[name + "_num"], 1, None)
    assert c["num_predictions"].dtype == np.float64 and np.array_equal(c["num_predictions"], num)
    # save_data (data_carrier_3D.py:209-214) and calculate_metrics (test_3D.py:555-562) on the reference's own sums
    want_data, want_seg = g[name + "_data"] / clip, g[name + "_seg"] / clip
    assert c["data"].dtype == np.float64 and np.array_equal(c["data"], want_data)
    assert c["gt_seg"].dtype == np.float64 and c["gt_seg"].shape == (3,) + img.shape and np.array_equal(c["gt_seg"], want_seg)
    assert c["gt"].dtype == np.intc and np.array_equal(c["gt"], np.asarray(want_seg, dtype=np.intc))
    assert np.array_equal(c["gt"][:, num > 0], np.stack(labels)[:, num > 0])   # under a patch: the label itself
    if name == "c1632":      # z 16..23 lies under no patch
        assert num[:, :, 16:].max() == 0 and num[:, :, :16].min() == 1
        for k in ("data", "gt_seg", "gt"):
            assert not c[k][..., 16:].any(), k
        assert np.abs(img[:, :, 16:]).min() > 0 and labels[0][:, :, 16:].any()
        assert np.array_equal(c["data"][:, :, :16], img[:, :, :16])
    if name == "c24":
        assert num.max() == 8 and num[8:16, 8:16, 8:16].min() == 8 and num[0, 0, 0] == 1
    if name == "c2416":
        # The additions are made: under three patches the composite is (d + d + d) / 3, which is not d everywhere -- for a
        # float64 image.  (For a float32 image it IS d everywhere: 3 d is exact in float64 and so is its third.)
        assert img.dtype == np.float64 and num.max() == 3
        three = num == 3
        thrice = (img + img + img) / 3
        assert (thrice != img)[three].any()
        assert np.array_equal(c["data"][three], thrice[three]) and not np.array_equal(c["data"][three], img[three])
        f32 = trees.image("c24")
        assert f32.dtype == np.float32 and np.array_equal((f32.astype(np.float64) * 3) / 3, f32)


def test_compose_case_without_raters_and_host_loader(tmp_path):
    from values_amd.dataset3d import HostTestLoader3D, cases, compose_case, get_val_test_data_samples
    c = compose_case(trees.image("c16"), None, [((0, 16),) * 3])
    assert c["gt_seg"].shape == (0, 16, 16, 16) and c["gt"].shape == (0, 16, 16, 16)
    base = trees.build_tree(tmp_path, "toy")
    cs = cases(get_val_test_data_samples(base, pattern=trees.PATTERN, num_raters=3, test=True, patch_size=16))
    groups = list(HostTestLoader3D(cs, 2))
    assert [len(g) for g in groups] == [2, 2, 1] and len(HostTestLoader3D(cs, 2)) == 3
    flat = [c for g in groups for c in g]
    assert [c["image_id"] for c in flat] == [c["image_id"] for c in cs]
    for c in flat:
        assert np.array_equal(c["image"], trees.image(c["image_id"])) and c["image"].dtype == c["dtype"]
        assert len(c["labels"]) == len(trees.LISTING_RATERS[c["image_id"]])
        for lab, r in zip(c["labels"], trees.LISTING_RATERS[c["image_id"]]):
            assert np.array_equal(lab, trees.label(c["image_id"], r)) and str(lab.dtype) == trees.LABEL_DTYPES[r]
    with pytest.raises(ValueError):
        HostTestLoader3D(cs, 0)
