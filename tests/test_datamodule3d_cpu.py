"""CPU: values_amd.datamodule3d, the host mirror of the 3D train / validation loaders -- against what the reference's own
NumpyDataLoader classes recorded over the trees of tests/dataset3d_trees.py (tests/golden/trainloader3d_kat.npz, written by
tools/gen_golden_trainloader3d.py), against the literal restatement in tests/trainloader3d_ref.py, against scikit-learn's
KFold, and against numpy slicing."""
import hashlib
import json
import os
import pickle
import random

import numpy as np
import pytest

from tests import dataset3d_trees as trees
from tests import trainloader3d_ref as ref
from tests.helpers import load_npz
from values_amd import datamodule3d as dm

IDS = sorted(n + ".npy" for n in trees.CASES)
FULL = {n: [0, 1, 2] for n in trees.CASES}


@pytest.fixture(scope="module")
def kat():
    return json.loads(bytes(load_npz("trainloader3d_kat.npz")["kat"]).decode())


def train_tree(root, layout, raters=None):
    base = trees.build_tree(root, layout, raters=raters)
    if layout == "toy":
        for sub in ("images", "labels"):
            os.rename(os.path.join(base, sub + "Ts"), os.path.join(base, sub + "Tr"))
    return base


@pytest.fixture(scope="module")
def bases(tmp_path_factory):
    root = tmp_path_factory.mktemp("trainloader3d")
    return {(layout, full): train_tree(os.path.join(root, "full" if full else "listing"), layout, FULL if full else None)
            for layout in ("toy", "lidc") for full in (False, True)}


def _rel(base):
    return lambda p: os.path.relpath(p, base).replace(os.sep, "/")


def _samples(bases, layout):
    return dm.get_train_data_samples(bases[layout, True], trees.PATTERN, IDS, 3, layout)


def _sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- against the recorded reference ------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["toy", "lidc"])
def test_listing_equals_the_reference(kat, bases, layout):
    base = bases[layout, False]
    rel = _rel(base)
    for tag, ids in (("none", None), ("some", ["c16.npy", "c1632.npy", "c24.npy", "other.npy", "absent.npy"]), ("all", IDS)):
        s = dm.get_train_data_samples(base, trees.PATTERN, ids, 3, layout)
        got = [[rel(x["image_path"]), None if x["label_paths"] is None else [rel(p) for p in x["label_paths"]]] for x in s]
        assert got == kat[f"listing|{layout}|{tag}"], (layout, tag)
    assert len(kat["listing|toy|none"]) == 5 and kat["listing|lidc|none"] == []          # subject_ids=None: everything / nothing
    with pytest.raises(ValueError):
        dm.get_train_data_samples(base, layout="other")


def _order_keys(kat, layout):
    return sorted({tuple(int(v) for v in k.split("|")[2:4]) for k in kat if k.startswith(f"order|{layout}|")})


@pytest.mark.parametrize("layout", ["toy", "lidc"])
def test_sample_order_rater_choice_and_crops_equal_the_reference(kat, bases, layout):
    samples = _samples(bases, layout)
    rel = _rel(bases[layout, True])
    combos = _order_keys(kat, layout)
    assert combos == [(1, 1), (1, 2), (1, 3), (3, 1), (3, 2)]
    for W, B in combos:
        rows = [kat[f"order|{layout}|{W}|{B}|{t}"] for t in range(W)]
        assert all(r[-1]["restarts"] >= 4 for r in rows)                                  # at least three restarts after the first pass
        # the order: worker t's batches are the drain's batches t, t + W, ...
        n = min(len(r) for r in rows)
        order = dm.SampleOrder(samples, B, True, W)
        for k in range(n * W):
            got = [rel(s["image_path"]) for s in order.next_batch()]
            assert got == rows[k % W][k // W]["images"], (W, B, k)
        # the rater after random.seed and the crop after np.random.seed, worker by worker (each recorded from fresh seeds)
        for t in range(W):
            rng, py = np.random.RandomState(kat["seeds"]["crop"]), random.Random(kat["seeds"]["rater"])
            worker = dm.SampleOrder(samples, B, True, W).workers[t]
            for row in rows[t]:
                plan = dm.plan_batch([samples[i] for i in worker.next()], trees.PATCH, False, rng, py, 0)
                assert [rel(r["label_path"]) for r in plan] == row["raters"]
                assert [list(r["origin"]) for r in plan] == row["origins"]


@pytest.mark.parametrize("layout", ["toy", "lidc"])
def test_validation_batches_equal_the_reference(kat, bases, layout):
    base = bases[layout, True]
    rel = _rel(base)
    samples = dm.get_val_test_data_samples(base, trees.PATTERN, IDS, 3, test=False, patch_size=trees.PATCH, layout=layout)
    loader = dm.HostLoader3D(samples, batch_size=1, patch_size=trees.PATCH, training=False, num_workers=1, seed=kat["seeds"]["rater"])
    rows = kat[f"val|{layout}"]
    assert len(loader) == len(rows) == len(samples)
    plans = []
    loader_plan = loader.next_plan
    loader.next_plan = lambda: plans.append(loader_plan()) or plans[-1]
    for row, batch, k in zip(rows, loader, range(len(rows))):
        r = plans[k][0]
        assert rel(r["image_path"]) == row["image"] and [list(o) for o in zip(r["origin"], [o + trees.PATCH for o in r["origin"]])] == row["crop"]
        assert [rel(p) for p in batch["label_paths"]] == row["raters"]
        assert list(batch["data"].shape) == row["data_shape"] and batch["data"].dtype == np.float32
        assert _sha(batch["data"]) == row["data"] and _sha(batch["seg"]) == row["seg"]
        assert not any(r["mirror"]) and not r["noise"]


# ---- against the literal restatement -----------------------------------------------------------------------------------

@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("n,B,W", [(5, 1, 1), (5, 2, 1), (5, 3, 1), (5, 2, 3), (5, 1, 3), (7, 3, 2), (1, 4, 1), (12, 4, 3), (13, 16, 1)])
def test_sample_order_equals_the_restated_loader(n, B, W, training):
    data = [{"image_path": f"s{i}", "label_paths": None} for i in range(n)]
    want = ref.drained(data, B, training, W, 40)
    order = dm.SampleOrder(data, B, training, W)
    got = [order.next_batch() for _ in range(40)]
    assert got == want
    assert len(order) == n and len(dm.SampleOrder(data, B, training, W, batches_per_epoch=3)) == 3
    assert any(len(b) < B for b in got) == (n % B != 0 or n < B)                         # the last batch of a pass is short
    assert sum(1 for _ in dm.SampleOrder(data, B, training, W)) == n                     # an "epoch" is len(samples) BATCHES


def test_sample_order_refuses_what_the_reference_cannot_run():
    data = [{"image_path": f"s{i}", "label_paths": None} for i in range(5)]
    with pytest.raises(ValueError):
        dm.SampleOrder(data, 3, True, 3)         # worker 2 would start at 6 >= 5 and restart for ever
    with pytest.raises(ValueError):
        dm.SampleOrder([], 1)
    with pytest.raises(ValueError):
        dm.SampleOrder(data, 0)


# ---- create_splits -----------------------------------------------------------------------------------------------------

def test_kfold_indices_equal_scikit_learn():
    model_selection = pytest.importorskip("sklearn.model_selection")
    for n in range(1, 24):
        for k in range(2, 6):
            if k > n:
                continue
            for seed in (0, 42, 12345):
                want = list(model_selection.KFold(n_splits=k, shuffle=True, random_state=seed).split(np.zeros(n)))
                got = dm.kfold_indices(n, k, seed)
                assert len(got) == len(want) == k
                for (gt, gv), (wt, wv) in zip(got, want):
                    assert np.array_equal(gt, wt) and np.array_equal(gv, wv), (n, k, seed)


def test_kfold_indices_properties_and_refusals():
    for n, k, seed in ((7, 3, 1), (23, 5, 42), (4, 4, 0)):
        folds = dm.kfold_indices(n, k, seed)
        sizes = [len(v) for _, v in folds]
        assert sizes == [n // k + (1 if i < n % k else 0) for i in range(k)]
        assert sorted(np.concatenate([v for _, v in folds]).tolist()) == list(range(n))
        for t, v in folds:
            assert sorted(t.tolist() + v.tolist()) == list(range(n)) and t.tolist() == sorted(t.tolist()) and v.tolist() == sorted(v.tolist())
    with pytest.raises(ValueError):
        dm.kfold_indices(3, 4, 0)
    with pytest.raises(ValueError):
        dm.kfold_indices(3, 1, 0)


def test_create_splits_pickle_layout(tmp_path):
    images, tests_ = tmp_path / "imagesTr", tmp_path / "imagesTs"
    images.mkdir(), tests_.mkdir()
    for i in range(7):
        np.save(images / f"{i:03d}.npy", np.zeros(1))
    (images / "notes.txt").write_text("x")
    for i in range(3):
        np.save(tests_ / f"t{i}.npy", np.zeros(1))
    dm.create_splits(str(tmp_path), str(images), str(tests_), seed=42, n_splits=3)
    splits = pickle.load(open(tmp_path / "splits.pkl", "rb"))
    assert isinstance(splits, list) and len(splits) == 3
    names = [f"{i:03d}.npy" for i in range(7)]
    for fold, (t, v) in zip(splits, dm.kfold_indices(7, 3, 42)):
        assert sorted(fold) == ["test", "train", "val"]
        for key in fold:
            assert isinstance(fold[key], np.ndarray) and fold[key].dtype.kind == "U"
        assert fold["train"].tolist() == [names[i] for i in t] and fold["val"].tolist() == [names[i] for i in v]
        assert fold["test"].tolist() == ["t0.npy", "t1.npy", "t2.npy"]


# ---- plan_batch --------------------------------------------------------------------------------------------------------

class _CountingRng:
    """a RandomState that counts its draws"""

    def __init__(self, seed):
        self.rs, self.randints, self.uniforms = np.random.RandomState(seed), 0, 0

    def randint(self, lo, hi):
        self.randints += 1
        return self.rs.randint(lo, hi)

    def uniform(self):
        self.uniforms += 1
        return self.rs.uniform()


def test_plan_batch_rules():
    P = 16
    shapes = {"a": (16, 19, 40), "b": (17, 16, 16), "small": (16, 15, 16)}
    samples = [{"image_path": "a", "label_paths": ["a0", "a1", "a2"]}, {"image_path": "b", "label_paths": None}]
    seen = {"a": set(), "b": set()}
    for seed in range(300):
        rng, py = _CountingRng(seed), random.Random(seed)
        plan = dm.plan_batch(samples, P, True, rng, py, 10, shapes=shapes)
        # a fixed number of draws per sample, whatever their values: one randint per axis with dim > P, three mirror
        # uniforms and one noise uniform
        assert rng.randints == 2 + 1 and rng.uniforms == 2 * (3 + 1)
        assert [r["index"] for r in plan] == [10, 11] and plan[0]["label_path"] in samples[0]["label_paths"] and plan[1]["label_path"] is None
        for r in plan:
            shape = shapes[r["image_path"]]
            assert all(0 <= o and o + P <= d for o, d in zip(r["origin"], shape))                      # inside the volume
            assert all(o == 0 for o, d in zip(r["origin"], shape) if d == P)                           # the centre rule at dim == P
            assert len(r["mirror"]) == 3 and all(isinstance(m, bool) for m in r["mirror"]) and isinstance(r["noise"], bool)
            seen[r["image_path"]].add(r["origin"])
    assert {o[1] for o in seen["a"]} == {0, 1, 2} and {o[2] for o in seen["a"]} == set(range(24))      # never 3, never 24: the last origin
    assert {o[0] for o in seen["b"]} == {0}                                                              # dim - P == 1: randint(0, 1)
    with pytest.raises(ValueError, match="smaller than the patch"):
        dm.plan_batch([{"image_path": "small", "label_paths": None}], P, False, np.random.RandomState(0), random.Random(0), 0, shapes=shapes)
    # without augment: no mirror, no noise, no uniform drawn; noise_p 0 / 1 decide the flag, the draw count stays
    rng = _CountingRng(1)
    plan = dm.plan_batch(samples, P, False, rng, random.Random(1), 0, shapes=shapes)
    assert rng.uniforms == 0 and not any(any(r["mirror"]) or r["noise"] for r in plan)
    on = dm.plan_batch(samples, P, True, np.random.RandomState(3), random.Random(3), 0, noise_p=1.0, shapes=shapes)
    off = dm.plan_batch(samples, P, True, np.random.RandomState(3), random.Random(3), 0, noise_p=0.0, shapes=shapes)
    assert all(r["noise"] for r in on) and not any(r["noise"] for r in off)
    assert [(r["origin"], r["mirror"], r["label_path"]) for r in on] == [(r["origin"], r["mirror"], r["label_path"]) for r in off]
    # validation: the sample's crop_idx
    val = [{"image_path": "a", "label_paths": ["a0"], "crop_idx": ((0, 16), (3, 19), (16, 32))}]
    plan = dm.plan_batch(val, P, True, _CountingRng(0), random.Random(0), 5, training=False)
    assert plan[0]["origin"] == (0, 3, 16) and plan[0]["index"] == 5 and not any(plan[0]["mirror"]) and not plan[0]["noise"]
    with pytest.raises(ValueError):
        dm.plan_batch([dict(val[0], crop_idx=((0, 16), (3, 18), (16, 32)))], P, False, _CountingRng(0), random.Random(0), 0, training=False)


# ---- host loader -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["toy", "lidc"])
@pytest.mark.parametrize("seg_dtype", ["float32", "uint8"])
def test_host_loader_is_numpy_slicing(bases, layout, seg_dtype):
    samples = _samples(bases, layout)
    P = trees.PATCH
    loader = dm.HostLoader3D(samples, batch_size=2, patch_size=P, augment=True, num_workers=3, seed=9, seg_dtype=seg_dtype, noise_p=0.0)
    twin = dm.HostLoader3D(samples, batch_size=2, patch_size=P, augment=True, num_workers=3, seed=9, noise_p=0.0)
    mirrored = 0
    for batch in loader:
        plan = twin.next_plan()
        B = len(plan)
        assert batch["data"].shape == (B, 1, P, P, P) and batch["data"].dtype == np.float32
        assert batch["seg"].shape == (B, 1, P, P, P) and batch["seg"].dtype == np.dtype(seg_dtype)
        assert batch["image_paths"] == [r["image_path"] for r in plan] and batch["label_paths"] == [r["label_path"] for r in plan]
        for i, r in enumerate(plan):
            sl = tuple(slice(o, o + P) for o in r["origin"])
            flip = tuple(slice(None, None, -1) if m else slice(None) for m in r["mirror"])
            assert np.array_equal(batch["data"][i, 0], np.load(r["image_path"])[sl][flip].astype(np.float32))
            assert np.array_equal(batch["seg"][i, 0], np.load(r["label_path"])[sl][flip].astype(np.intc).astype(seg_dtype))
            mirrored += any(r["mirror"])
    assert mirrored and loader.emitted == twin.emitted


def test_host_loader_noise_and_seed(bases):
    samples = _samples(bases, "toy")
    kw = dict(batch_size=2, patch_size=trees.PATCH, augment=True, num_workers=1, seed=4, batches_per_epoch=3)
    clean = list(dm.HostLoader3D(samples, noise_p=0.0, **kw))
    noisy = list(dm.HostLoader3D(samples, noise_p=1.0, **kw))
    again = list(dm.HostLoader3D(samples, noise_p=1.0, **kw))
    other = list(dm.HostLoader3D(samples, noise_p=1.0, **dict(kw, seed=5)))
    for c, n, a in zip(clean, noisy, again):
        assert c["image_paths"] == n["image_paths"] and np.array_equal(c["seg"], n["seg"])      # the fields do not move the decisions
        d = n["data"].astype(np.float64) - c["data"]
        assert n["data"].dtype == np.float32 and 0 < d.std() < 0.1 ** 0.5 * 1.2 and abs(d.mean()) < 0.05
        assert np.array_equal(n["data"], a["data"])                                             # reproducible from the seed
    assert [b["image_paths"] for b in other] != [b["image_paths"] for b in noisy] or not np.array_equal(other[0]["data"], noisy[0]["data"])
    with pytest.raises(ValueError):
        dm.HostLoader3D(samples, seg_dtype="int64")


def test_host_loader_uint8_seg_raises_on_a_label_outside_0_255(tmp_path):
    base = train_tree(tmp_path, "toy", FULL)
    bad = np.load(os.path.join(base, "labelsTr", "c16_01.npy")).astype(np.int32)
    bad[3, 3, 3] = 256
    for r in range(3):
        np.save(os.path.join(base, "labelsTr", f"c16_{r:02d}.npy"), bad)
    samples = dm.get_train_data_samples(base, "c16.npy", None, 3)
    with pytest.raises(ValueError, match="outside 0..255"):
        list(dm.HostLoader3D(samples, batch_size=1, patch_size=trees.PATCH, seg_dtype="uint8"))
    assert len(list(dm.HostLoader3D(samples, batch_size=1, patch_size=trees.PATCH))) == 1       # float32 seg: as the reference, no check


# ---- cache policy ------------------------------------------------------------------------------------------------------

def test_payload_cache_against_a_small_model():
    rs = np.random.RandomState(2)
    sizes = {f"f{i}": int(rs.randint(1, 50)) for i in range(12)}
    for budget in (None, 0, 60, 200):
        cache, model = dm.PayloadCache(budget), []                      # model: keys, least recently used first
        for step in range(200):
            cur = [f"f{i}" for i in rs.choice(12, size=3, replace=False)]
            nxt = [f"f{i}" for i in rs.choice(12, size=3, replace=False)]
            for k in cur:
                if k in cache:
                    assert cache.get(k) == k.upper()
                    model.remove(k)
                else:
                    assert k not in model
                    cache.put(k, k.upper(), sizes[k])
                model.append(k)
            cache.pin(cur + nxt)
            if budget is not None:                                     # the model's eviction: oldest first, never a pinned one
                for k in list(model):
                    if sum(sizes[m] for m in model) <= budget:
                        break
                    if k not in cur + nxt:
                        model.remove(k)
            assert list(cache.entries) == model and cache.bytes == sum(sizes[m] for m in model)
            assert all(k in cache for k in cur)                        # the current batch is never evicted
            pinned = sum(sizes[m] for m in model if m in cur + nxt)
            if budget is None:
                assert len(model) == len({m for m in model})
            else:
                assert cache.bytes <= max(budget, pinned)              # the budget holds unless the pinned entries alone exceed it
                if budget == 0:
                    assert set(model) <= set(cur + nxt)
    with pytest.raises(ValueError):
        dm.PayloadCache(-1)


# ---- datamodules, io ---------------------------------------------------------------------------------------------------

def test_io_resolves_both_targets(tmp_path, monkeypatch):
    from values_amd import io
    monkeypatch.delenv("DATASET_LOCATION", raising=False)
    for prefix in ("uncertainty_modeling.", ""):
        toy = io.instantiate({"_target_": prefix + "toy_datamodule_3D.ToyDataModule3D", "dataset_name": "Case_1", "num_raters": 3,
                              "data_input_dir": str(tmp_path), "batch_size": 2, "patch_size": 16, "augment": True})
        lidc = io.instantiate({"_target_": prefix + "lidc_idri_datamodule_3D.LidcIdriDataModule3D", "shift_feature": None,
                               "data_input_dir": str(tmp_path), "splits_path": None})
        assert isinstance(toy, dm.ToyDataModule3D) and isinstance(lidc, dm.LIDCDataModule3D)
        assert toy.batch_size == 2 and toy.augment and not toy.device_io and toy.num_classes == 2
        assert lidc.splits_path == os.path.join(str(tmp_path), "splits_all.pkl")
    with pytest.raises(FileNotFoundError):
        lidc.prepare_data()


@pytest.mark.parametrize("layout", ["toy", "lidc"])
def test_datamodule_from_a_preprocessed_tree(tmp_path, monkeypatch, layout):
    monkeypatch.delenv("DATASET_LOCATION", raising=False)
    if layout == "toy":
        root = tmp_path / "Case_1"
        base = train_tree(root, "toy", FULL)
        os.rename(base, root / "preprocessed")
        os.makedirs(root / "preprocessed" / "imagesTs")
        module = dm.ToyDataModule3D("Case_1", 3, str(tmp_path), data_num_folds=2, batch_size=2, patch_size=16, num_workers=1, seed=1)
        module.prepare_data()                                          # preprocessed exists; splits.pkl is created
    else:
        base = train_tree(tmp_path, "lidc", FULL)
        os.rename(base, tmp_path / "preprocessed")
        names = sorted(f for f in os.listdir(tmp_path / "preprocessed" / "images"))
        pickle.dump([{"train": np.array(names[:4]), "val": np.array(names[4:]), "id_test": np.array([]), "ood_test": np.array([])}],
                    open(tmp_path / "splits_all.pkl", "wb"))
        module = dm.LIDCDataModule3D(None, 3, str(tmp_path), batch_size=2, patch_size=16, num_workers=1, seed=1)
        module.prepare_data()
    module.setup()
    train, val = module.train_dataloader(), module.val_dataloader()
    assert isinstance(train, dm.HostLoader3D) and train.training and not val.training
    assert len(train) == len(module.tr_keys) and val.order.batch_size == 1 and val.order.num_workers == 1
    batch = next(iter(train))
    assert batch["data"].shape[1:] == (1, 16, 16, 16) and batch["seg"].dtype == np.float32
    assert {os.path.basename(p) for b in val for p in b["image_paths"]} == set(module.val_keys.tolist())
