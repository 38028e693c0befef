"""CPU: the host mirror of the 2D test split (values_amd.dataset2d) against the reference class's recorded raters
(tests/golden/label_switch_kat.npz, tools/gen_golden_labelswitch.py), the integer restatement of the device draw, the
listing / datamodule on a temporary tree, and the re-pointed targets.  Every comparison is on integers and exact."""
import math

import numpy as np
import pytest
import torch

from tests.dataset2d_trees import IDS, MEAN, STD, augmentations, datamodule_config, make_tree
from tests.helpers import load_npz
from values_amd import dataset2d as d2
from values_amd import gta


def test_label_switch_references_equal_the_reference_class_after_np_random_seed():
    g = load_npz("label_switch_kat.npz")
    n = 0
    for m in range(3):
        mask = g[f"mask_{m}"]
        assert mask.dtype == np.int64
        for s in g["seeds"]:
            for r in g["n_reference_samples"]:
                want = g[f"out_{m}_{s}_{r}"]
                np.random.seed(int(s))
                got = d2.label_switch_references(mask, int(r))
                assert got.shape == want.shape == ((r,) + mask.shape if r > 1 else mask.shape) and got.dtype == want.dtype
                np.testing.assert_array_equal(got, want)
                np.testing.assert_array_equal(d2.label_switch_references(mask, int(r), g[f"draws_{s}_{r}"]), want)
                n += 1
    assert n == 24


def test_explicit_decisions_all_zero_and_all_one():
    rng = np.random.default_rng(2)
    mask = IDS[rng.integers(0, len(IDS), size=(9, 14))]
    zero = d2.label_switch_references(mask, 3, np.zeros((3, 5), dtype=np.uint8))
    assert zero.shape == (3, 9, 14)
    for r in range(3):
        np.testing.assert_array_equal(zero[r], mask)
    one = d2.label_switch_references(mask, 1, np.ones((1, 5), dtype=np.uint8))
    assert one.shape == (9, 14)
    moved = {f: t for f, t, _ in d2.switch_table()}
    assert moved == {1: 19, 11: 20, 13: 21, 8: 22, 0: 23}
    want = mask.copy()
    for f, t in moved.items():
        want[mask == f] = t
    np.testing.assert_array_equal(one, want)
    keep = ~np.isin(mask, list(moved))
    np.testing.assert_array_equal(one[keep], mask[keep])    # 2, 5 and 255 pass through


def test_switch_decisions_depend_on_seed_index_rater_and_class_alone():
    R = 5
    alone = {i: d2.switch_decisions(77, [i], R)[0] for i in (0, 1, 5, 6, 1000, 2 ** 31 + 3)}
    batch = d2.switch_decisions(77, [5, 0, 1000, 1, 2 ** 31 + 3, 6], R)
    assert batch.shape == (6, R, 5) and batch.dtype == np.uint8 and set(np.unique(batch)) <= {0, 1}
    for pos, i in enumerate([5, 0, 1000, 1, 2 ** 31 + 3, 6]):
        np.testing.assert_array_equal(batch[pos], alone[i])
    np.testing.assert_array_equal(d2.switch_decisions(77, [6, 5], R), batch[[5, 0]])
    np.testing.assert_array_equal(d2.switch_decisions(77, [3], 31)[0][:R], d2.switch_decisions(77, [3], R)[0])
    many = d2.switch_decisions(77, range(64), R)
    assert (many != d2.switch_decisions(78, range(64), R)).any()
    assert len({many[i].tobytes() for i in range(64)}) > 32         # 25 bits per index: the indices differ
    assert d2.switch_thresholds() == [int((1.0 / 3.0) * 2 ** 24)] * 5 == [5592405] * 5


def test_switch_decisions_rate():
    """N = 20 000 decisions of seed 2024: the ones lie within 5 sqrt(N p (1 - p)) of N p, p = thr / 2^24 (the draw is
    deterministic: 6673 ones for this seed, N p = 6666.7, bound 333.3)"""
    dec = d2.switch_decisions(2024, range(4000), 1)
    N, p = dec.size, d2.switch_thresholds()[0] / 2 ** 24
    assert N == 20000
    assert abs(int(dec.sum()) - N * p) <= 5 * math.sqrt(N * p * (1 - p))


def test_variance_table_is_the_hook_s_values():
    tab = d2.switch_variance_table()
    assert tab.dtype == np.float32 and tab.shape == (256,)
    lab = np.arange(256, dtype=np.int64).reshape(16, 16)
    np.testing.assert_array_equal(np.swapaxes(tab[lab], 0, 1).view(np.uint32), gta._switch_variance(lab).view(np.uint32))
    assert sorted(np.flatnonzero(tab).tolist()) == sorted(gta.NAME2TRAINID.values())


def test_listing_order_split_names_and_attributes(tmp_path):
    base, splits, ids = make_tree(tmp_path)
    assert [d2.test_split_name(s) for s in ("id", "ood", "val", "unlabeled")] == ["id_test", "ood_test", "val", "unlabeled"]
    keys = d2.split_keys(splits, 0)
    assert set(keys) == {"train", "val", "id_test", "ood_test", "unlabeled"} and len(keys["id_test"]) == 5
    assert keys["unlabeled"].shape == (2, 2)
    ds = d2.CityscapesTestSet(splits, base, split="id_test", transforms=d2.parse_test_transforms(augmentations(5)))
    assert len(ds) == 5 and ds.image_ids == ids == ["g005", "g006", "g007", "city_08_x", "city_09_x"]
    assert ds.datasets == ["gta"] * 3 + ["cs"] * 2
    assert all("OriginalData/preprocessed/images" in p for p in ds.imgs) and all("CityScapesOriginalData" in p for p in ds.imgs[3:])
    assert [p.replace("/images/", "/labels/") for p in ds.imgs] == ds.masks
    assert [s["image_id"] for s in ds.samples] == ids and set(ds.samples[0]) == {"image_path", "label_path", "image_id", "dataset"}
    assert d2.CityscapesTestSet(splits, base, split="ood_test").image_ids == ["city_08_x", "city_09_x"]
    assert "unlisted" not in ds.image_ids
    with pytest.raises(ValueError):
        d2.CityscapesTestSet(splits, base, split="nowhere")
    smp = d2.get_data_samples(base + "/OriginalData/preprocessed", "*.npy", ["g007.npy"], "gta")
    assert [s["image_id"] for s in smp] == ["g007"] and smp[0]["label_path"].endswith("labels/g007.npy")


@pytest.mark.parametrize("tta", [False, True])
@pytest.mark.parametrize("R", [1, 5])
def test_getitem_keys_dtypes_shapes(tmp_path, tta, R):
    from values_amd.data import TTA_2D_TRANSFORMS, tta_views_2d
    base, splits, ids = make_tree(tmp_path)
    ds = d2.CityscapesTestSet(splits, base, split="id_test", transforms=d2.parse_test_transforms(augmentations(R)), tta=tta, seed=11)
    item = ds[3]
    assert set(item) == {"data", "seg", "image_id", "dataset"} | ({"transforms"} if tta else set())
    assert item["image_id"] == "city_08_x" and item["dataset"] == "cs"
    img, mask = np.load(ds.imgs[3]), np.load(ds.masks[3])
    views, _ = tta_views_2d(img, MEAN, STD)
    if tta:
        assert isinstance(item["data"], list) and len(item["data"]) == 4 and item["transforms"] == TTA_2D_TRANSFORMS
        for got, want in zip(item["data"], views):
            assert got.dtype == torch.float32 and tuple(got.shape) == (3, 17, 33)
            np.testing.assert_array_equal(got.numpy(), want)
    else:
        assert item["data"].dtype == torch.float32 and tuple(item["data"].shape) == (3, 17, 33)
        np.testing.assert_array_equal(item["data"].numpy(), views[0])
    assert item["seg"].dtype == torch.int64 and tuple(item["seg"].shape) == ((R, 17, 33) if R > 1 else (17, 33))
    want = d2.label_switch_references(mask, R, d2.switch_decisions(11, [3], R)[0])
    np.testing.assert_array_equal(item["seg"].numpy(), want)
    np.testing.assert_array_equal(ds[3]["seg"].numpy(), want)        # a seeded set returns the same raters every time
    # without a seed the raters come from np.random, as in the reference
    free = d2.CityscapesTestSet(splits, base, split="id_test", transforms=d2.parse_test_transforms(augmentations(R)), tta=tta)
    np.random.seed(4)
    got = free[3]["seg"].numpy()
    np.random.seed(4)
    np.testing.assert_array_equal(got, d2.label_switch_references(mask, R))


def test_datamodule_batches_short_last_batch_and_transform_names(tmp_path):
    base, splits, ids = make_tree(tmp_path)
    dm = d2.TestDataModule2D(base, {"_target_": "values_amd.dataset2d.CityscapesTestSet", "splits_path": splits}, 6, 2, 0,
                             augmentations(5), tta=True, seed=3, test_split="id")
    with pytest.raises(RuntimeError):
        dm.test_dataloader()
    dm.setup("test")
    loader = dm.test_dataloader()
    assert loader.dataset is dm.DS_test and len(loader) == 3
    batches = list(loader)
    assert [len(b["image_id"]) for b in batches] == [2, 2, 1]
    assert [i for b in batches for i in b["image_id"]] == ids
    assert [i for b in batches for i in b["dataset"]] == ["gta"] * 3 + ["cs"] * 2
    b = batches[0]
    assert set(b) == {"data", "seg", "image_id", "dataset", "transforms"}
    assert len(b["data"]) == 4 and tuple(b["data"][0].shape) == (2, 3, 17, 33) and tuple(b["seg"].shape) == (2, 5, 17, 33)
    assert tuple(batches[2]["seg"].shape) == (1, 5, 17, 33)
    from values_amd.data import hflip_flags
    assert hflip_flags(b["transforms"]) == [False, True, False, True]
    np.testing.assert_array_equal(b["seg"][1].numpy(), loader.dataset[1]["seg"].numpy())
    # one rater, no TTA: the collate stacks (H, W) items
    dm1 = d2.TestDataModule2D(base, {"_target_": "values_amd.dataset2d.CityscapesTestSet", "splits_path": splits}, 6, 4, 0,
                              augmentations(), test_split="ood")
    dm1.setup("test")
    (b1,) = list(dm1.test_dataloader())
    assert set(b1) == {"data", "seg", "image_id", "dataset"} and tuple(b1["data"].shape) == (2, 3, 17, 33)
    assert tuple(b1["seg"].shape) == (2, 17, 33) and dm1.DS_test.transforms.n_reference_samples == 1
    with pytest.raises(ValueError, match="GaussNoise"):
        d2.TestDataModule2D(base, {"_target_": "values_amd.dataset2d.CityscapesTestSet", "splits_path": splits}, 6, 2, 0,
                            augmentations(5, extra="GaussNoise"), test_split="id").setup("test")
    with pytest.raises(ValueError):      # the device loader draws on the device: it needs the seed
        d2.TestDataModule2D(base, {}, 6, 2, 0, augmentations(5), device_io=True)


def test_set_n_reference_samples():
    hp = {"AUGMENTATIONS": augmentations(1)}
    assert d2.set_n_reference_samples(hp, 7) is hp
    assert d2.parse_test_transforms(hp["AUGMENTATIONS"]).n_reference_samples == 7
    t = d2.parse_test_transforms(hp["AUGMENTATIONS"])
    assert t.mean == MEAN and t.std == STD and t.max_pixel_value == 255.0


def test_target_map_entries_resolve_and_instantiate_builds_the_datamodule(tmp_path):
    import importlib
    from values_amd.io import TARGET_MAP, instantiate
    want = {"uncertainty_modeling.data.torch_dataloader.BaseDataModule": d2.TestDataModule2D,
            "data.torch_dataloader.BaseDataModule": d2.TestDataModule2D,
            "uncertainty_modeling.data.cityscapes_dataset.Cityscapes_dataset": d2.CityscapesTestSet,
            "data.cityscapes_dataset.Cityscapes_dataset": d2.CityscapesTestSet}
    for k, cls in want.items():
        mod, _, name = TARGET_MAP[k].rpartition(".")
        assert getattr(importlib.import_module(mod), name) is cls
    base, splits, ids = make_tree(tmp_path)
    for spelling in ("uncertainty_modeling.", ""):
        dm = instantiate(datamodule_config(base, splits, spelling=spelling), test_split="id")   # as ExperimentDataloader does
        assert isinstance(dm, d2.TestDataModule2D)
        dm.setup("test")
        loader = dm.test_dataloader()
        assert isinstance(loader.dataset, d2.CityscapesTestSet) and loader.dataset.image_ids == ids
        assert loader.dataset.data_fold_id == 0 and [len(b["image_id"]) for b in loader] == [2, 2, 1]


def test_label_switch_call_is_refused_on_the_host_before_any_device_call():
    """the argument checks of vx_label_switch_batched run before the first device call, so they answer without a GPU (the
    pointers are never dereferenced: every call below is refused)"""
    import ctypes as C
    import os
    import __graft_entry__ as ge
    from values_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    lib = _lib.load()
    rows, vt = d2.switch_rows(), d2.switch_variance_table()

    def call(n=1, R=5, rows=rows, ns=5, status=0x20000, ws=0x30000, wsn=1 << 20, **item):
        arr = (_lib.LswitchItem * 1)()
        arr[0].labels, arr[0].refs, arr[0].H, arr[0].W, arr[0].kind = 0x10000, 0x40000, 4, 6, _lib.VX_COUNT_B8
        for k, v in item.items():
            setattr(arr[0], k, v)
        return lib.vx_label_switch_batched(arr, n, R, rows, ns, None, 1, vt.ctypes.data_as(C.POINTER(C.c_float)), status, ws, wsn, None)

    two = (_lib.LswitchRow * 2)()
    two[0].from_, two[0].to, two[1].from_, two[1].to = 1, 19, 19, 20
    assert call(labels=None) == -1 and call(status=None) == -1 and call(ws=None) == -1
    assert call(R=0) == call(R=32) == call(n=0) == call(ns=9) == call(H=0) == call(H=1 << 16, W=1 << 15) == call(rows=two, ns=2) == -2
    assert call(kind=4) == -3 and call(wsn=64) == -4
    assert call(labels=0x10004) == call(variance=0x50002) == call(ws=0x30008) == -5
    assert b"vx_label_switch_batched" in lib.vx_last_error_string()
    assert lib.vx_label_switch_batched_workspace_bytes(1, 5) >= 1024 + 88 and lib.vx_label_switch_batched_workspace_bytes(1, 0) == 0
