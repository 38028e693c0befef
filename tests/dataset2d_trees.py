"""A small preprocessed GTA / Cityscapes tree with its splits.pkl, for the 2D test split's tests (CPU and GPU)."""
import os
import pickle

import numpy as np

IDS = np.array([0, 1, 2, 5, 8, 11, 13, 255])
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def augmentations(n_reference_samples=None, extra=None):
    """the AUGMENTATIONS of the reference's 2D configs, TEST part, as a plain resolved dict"""
    sw = {} if n_reference_samples is None else {"n_reference_samples": n_reference_samples}
    tr = [{"Normalize": {"mean": list(MEAN), "std": list(STD)}}, {"StochasticLabelSwitches": sw}, {"ToTensorV2": None}]
    if extra:
        tr.insert(1, {extra: {}})
    return {"TEST": [{"Compose": {"transforms": tr}}]}


def make_tree(root, n_gta=3, n_cs=2, H=17, W=33, label_dtype=np.int64, seed=5):
    """-> (base_dir, splits_path, ids in loader order).  The id_test split holds every case, listed out of order and
    with the two data sets interleaved; an image that is in no split lies beside them."""
    rng = np.random.default_rng(seed)
    root = str(root)
    names = {"gta": [f"g{7 - i:03d}" for i in range(n_gta)], "cs": [f"city_{9 - i:02d}_x" for i in range(n_cs)]}
    for ds, sub in (("gta", "OriginalData"), ("cs", "CityScapesOriginalData")):
        for kind in ("images", "labels"):
            os.makedirs(os.path.join(root, sub, "preprocessed", kind), exist_ok=True)
        for n in names[ds] + ["unlisted"]:
            d = os.path.join(root, sub, "preprocessed")
            np.save(os.path.join(d, "images", n + ".npy"), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
            np.save(os.path.join(d, "labels", n + ".npy"), IDS[rng.integers(0, len(IDS), size=(H, W))].astype(label_dtype))
    keys = [(n + ".npy", "cs") for n in names["cs"]] + [(n + ".npy", "gta") for n in names["gta"]]
    keys = keys[1::2] + keys[0::2]
    empty = np.empty((0, 2), dtype="<U32")
    fold = {"train": [], "val": keys[:1], "id_test": keys, "ood_test": [k for k in keys if k[1] == "cs"],
            "id_unlabeled_pool": empty, "ood_unlabeled_pool": np.array(keys[:2], dtype="<U32")}
    splits_path = os.path.join(root, "splits.pkl")
    with open(splits_path, "wb") as f:
        pickle.dump([fold], f)
    return root, splits_path, sorted(names["gta"]) + sorted(names["cs"])


def datamodule_config(base_dir, splits_path, val_batch_size=2, n_reference_samples=5, spelling="uncertainty_modeling.", **kw):
    """a gta_torch_config-shaped dict (uncertainty_modeling/configs/datamodule/gta_torch_config.yaml), resolved"""
    cfg = {"_target_": spelling + "data.torch_dataloader.BaseDataModule", "num_classes": 24, "ignore_index": 255, "num_workers": 2,
           "batch_size": 6, "val_batch_size": val_batch_size, "data_fold_id": 0, "augmentations": augmentations(n_reference_samples),
           "dataset": {"_target_": spelling + "data.cityscapes_dataset.Cityscapes_dataset", "splits_path": splits_path},
           "data_input_dir": base_dir}
    cfg.update(kw)
    return cfg
