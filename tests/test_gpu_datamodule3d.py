"""GPU: DeviceLoader3D (values_amd.datamodule3d) against HostLoader3D over the trees of tests/dataset3d_trees.py, and the
validation epoch from a directory (validation.validate_split).  Without noise the two loaders are held to equality, batch
by batch; the device noise is held to the float64 restatement of vx_noise_view_3d in tests/noise_ref.py at the bounds
tests/test_gpu_noise.py holds that kernel to (CONTRACT and REG["view"], imported from there: no tolerance of this file's
own)."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import dataset3d_trees as trees
from tests import noise_ref as nr
from tests.formula import formula_unet3d_state_dict
from tests.test_gpu_noise import CONTRACT, REG
from tests.test_gpu_sample import deviation
from values_amd import datamodule3d as dm
from values_amd import validation as va

pytestmark = pytest.mark.gpu

IDS = sorted(n + ".npy" for n in trees.CASES)
FULL = {n: [0, 1, 2] for n in trees.CASES}
P = trees.PATCH


def train_tree(root, layout):
    base = trees.build_tree(root, layout, raters=FULL)
    if layout == "toy":
        for sub in ("images", "labels"):
            os.rename(os.path.join(base, sub + "Ts"), os.path.join(base, sub + "Tr"))
    return base


@pytest.fixture(scope="module")
def bases(tmp_path_factory):
    root = tmp_path_factory.mktemp("datamodule3d")
    return {layout: train_tree(root, layout) for layout in ("toy", "lidc")}


def _same(dev, host):
    assert dev["image_paths"] == host["image_paths"] and dev["label_paths"] == host["label_paths"]
    for k in ("data", "seg"):
        d = dev[k].cpu().numpy()
        assert dev[k].is_cuda and d.dtype == host[k].dtype and d.shape == host[k].shape
        assert d.tobytes() == host[k].tobytes(), k


@pytest.mark.parametrize("seg_dtype", ["float32", "uint8"])
@pytest.mark.parametrize("workers", [1, 3])
@pytest.mark.parametrize("layout", ["toy", "lidc"])
def test_train_batches_equal_the_host_loader(bases, layout, workers, seg_dtype):
    samples = dm.get_train_data_samples(bases[layout], trees.PATTERN, IDS, 3, layout)
    assert len(samples) == 5
    # batch 2 over five cases: three batches a pass, so six batches are two passes (one restart of every worker)
    kw = dict(batch_size=2, patch_size=P, training=True, augment=True, num_workers=workers, seed=13, seg_dtype=seg_dtype, noise_p=0.0,
              batches_per_epoch=6)
    host = list(dm.HostLoader3D(samples, **kw))
    with dm.DeviceLoader3D(samples, **kw) as loader:
        dev = list(loader)
        assert loader.emitted == 10 and all(w.num_restarted == 2 for w in loader.order.workers)
    assert len(dev) == len(host) == 6
    for d, h in zip(dev, host):
        _same(d, h)


@pytest.mark.parametrize("layout", ["toy", "lidc"])
def test_validation_batches_equal_the_host_loader(bases, layout):
    samples = dm.get_val_test_data_samples(bases[layout], trees.PATTERN, IDS, 3, test=False, patch_size=P, layout=layout)
    kw = dict(batch_size=1, patch_size=P, training=False, num_workers=1, seed=3)
    host = list(dm.HostLoader3D(samples, **kw))
    with dm.DeviceLoader3D(samples, **kw) as loader:
        dev = list(loader)
    assert len(dev) == len(host) == len(samples) > 5
    for d, h in zip(dev, host):
        _same(d, h)


@pytest.mark.parametrize("law", [0, 1])
def test_device_noise_is_the_restated_noise_view(bases, law):
    # the bound is an absolute one, derived on z-scored intensities (tests/noise_ref.py: magnitude of a few units), which
    # is what a preprocessed tree holds.  c32 stores raw int16 counts up to 3733, where half a float32 ulp (1.2e-4) alone
    # is a hundred times the bound: it stays in the exact tests above and out of this one.
    samples = [s for s in dm.get_train_data_samples(bases["toy"], trees.PATTERN, IDS, 3, "toy") if not s["image_path"].endswith("c32.npy")]
    assert len(samples) == 4 and max(float(np.abs(np.load(s["image_path"])).max()) for s in samples) < 5.0
    seed = 21
    kw = dict(batch_size=2, patch_size=P, training=True, augment=True, num_workers=1, seed=seed, sigma_law=law, batches_per_epoch=4)
    with dm.DeviceLoader3D(samples, noise_p=0.0, **kw) as a, dm.DeviceLoader3D(samples, noise_p=1.0, **kw) as b:
        clean, noisy = list(a), list(b)
    index, worst = 0, 0.0
    for c, n in zip(clean, noisy):
        assert c["image_paths"] == n["image_paths"] and torch.equal(c["seg"], n["seg"])
        x = c["data"].cpu().numpy()
        want, _ = nr.view3d(x.reshape(len(x), -1), seed, index, dm.NOISE_VARIANCE[0], dm.NOISE_VARIANCE[1], law)   # index0: the running count
        err = deviation(n["data"].cpu().numpy().reshape(len(x), -1), want)
        worst = max(worst, err)
        index += len(x)
    print(f"deviation datamodule3d noise law={law} {worst:.3e}")
    assert index == 8 and worst <= CONTRACT and worst <= REG["view"]
    # keyed by the global sample index: the same records in other chunks are the same batch
    with dm.DeviceLoader3D(samples, noise_p=1.0, **dict(kw, batch_size=4)) as loader:
        dev = torch.device("cuda", torch.cuda.current_device())
        plan = loader.next_plan()
        files = dm._plan_files(plan)
        loader._upload(files, [open(f, "rb").read() for f in files], dev)
        whole = loader.make(plan, dev)
        parts = [loader.make(chunk, dev) for chunk in (plan[:1], plan[1:3], plan[3:])]
    assert [r["index"] for r in plan] == [0, 1, 2, 3] and all(r["noise"] for r in plan)
    assert torch.equal(whole["data"], torch.cat([p["data"] for p in parts])) and torch.equal(whole["seg"], torch.cat([p["seg"] for p in parts]))


def test_device_batches_do_not_depend_on_the_cache_budget(bases):
    samples = dm.get_train_data_samples(bases["lidc"], trees.PATTERN, IDS, 3, "lidc")
    kw = dict(batch_size=2, patch_size=P, training=True, augment=True, num_workers=3, seed=5, noise_p=0.5, batches_per_epoch=9)
    with dm.DeviceLoader3D(samples, cache_bytes=None, **kw) as keep, dm.DeviceLoader3D(samples, cache_bytes=0, **kw) as drop:
        for i, (a, b) in enumerate(zip(keep, drop)):
            assert a["image_paths"] == b["image_paths"] and a["label_paths"] == b["label_paths"]
            assert torch.equal(a["data"], b["data"]) and torch.equal(a["seg"], b["seg"])
            files = set(a["image_paths"]) | set(a["label_paths"])
            assert files <= set(drop.cache.entries) and set(drop.cache.entries) <= drop.cache.pinned     # nothing beyond current + prefetched
            assert len(drop.cache.entries) <= 8 and set(keep.cache.entries) >= files
        assert i == 8 and len(keep.cache.entries) > len(drop.cache.entries)


def test_device_loader_raises_on_a_label_outside_0_255(tmp_path):
    base = train_tree(tmp_path, "toy")
    bad = np.load(os.path.join(base, "labelsTr", "c16_00.npy")).astype(np.int16)
    bad[2, 2, 2] = -1
    for r in range(3):
        np.save(os.path.join(base, "labelsTr", f"c16_{r:02d}.npy"), bad)
    samples = dm.get_train_data_samples(base, "c16.npy", None, 3)
    with dm.DeviceLoader3D(samples, batch_size=1, patch_size=P) as loader:
        with pytest.raises(ValueError, match=r"c16_0\d\.npy: 1 labels outside 0..255"):
            list(loader)


def test_validate_split_from_a_directory(tmp_path, monkeypatch):
    from values_amd import UNet3D
    monkeypatch.delenv("DATASET_LOCATION", raising=False)
    root = tmp_path / "Case_1"
    os.rename(train_tree(root, "toy"), root / "preprocessed")
    pickle.dump([{"train": np.array(IDS[:3]), "val": np.array(IDS[3:]), "test": np.array([])}], open(root / "splits.pkl", "wb"))
    model = UNet3D(num_classes=2)
    model.load_state_dict({k: torch.from_numpy(v).float() for k, v in formula_unet3d_state_dict().items()})
    model = model.cuda()
    results = {}
    for device_io in (False, True):
        module = dm.ToyDataModule3D("Case_1", 3, str(tmp_path), patch_size=P, seed=8, device_io=device_io, seg_dtype="uint8")
        module.setup()
        assert type(module.val_dataloader()) is (dm.DeviceLoader3D if device_io else dm.HostLoader3D)
        results[device_io] = va.validate_split(model, module)
    host = [(torch.from_numpy(b["data"]).cuda(), b["seg"]) for b in
            dm.HostLoader3D(dm.get_val_test_data_samples(str(root / "preprocessed"), "*.npy", np.array(IDS[3:]), 3, test=False, patch_size=P),
                            batch_size=1, patch_size=P, training=False, seed=8, seg_dtype="uint8")]
    want = va.validate(model, host)
    assert len(want["batches"]) == len(host) > 2
    assert results[True] == want and results[False] == want
    assert np.isfinite(want["validation/val_loss"]) and 0.0 <= want["validation/val_dice"] <= 1.0
