"""GPU: the Softmax tree's pred_entropy/ set up by DeviceExperimentDataloader -- class files read with the device readers,
one one_minus_msr_batch call per chunk of images, maps encoded and written from the device -- against the tree the host
ExperimentDataloader builds from the same pred_prob files: same names, .nii.gz files that gunzip to the same bytes
(float64), byte-identical .tif files."""
import gzip
import math
import os
import shutil

import numpy as np
import pytest
import torch

from tests.formula import formula_tensor

pytestmark = pytest.mark.gpu

SHAPES_3D = ((5, 4, 3), (8, 8, 8), (16, 9, 7))
SHAPES_2D = ((6, 5), (9, 4))      # (H, W)


def _softmax(shape, tag):
    z = formula_tensor(shape, tag, scale=3.0)
    e = np.exp(z - z.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def _version(base, n_classes, ending=".nii.gz"):
    from values_amd.experiment import ExperimentVersion
    return ExperimentVersion(base_path=base, naming_scheme_version="fold{fold}", pred_model="Softmax",
                             image_ending=".png" if ending == ".tif" else ending, unc_ending=ending,
                             unc_types=["predictive_uncertainty"], aggregations=None, n_reference_segs=0, n_classes=n_classes,
                             fold=0)


def _write_3d(base, n_classes):
    from values_amd.results import results_dir, save_case
    d = results_dir(str(base), "Softmax", "fold0", "id")
    for i, shape in enumerate(SHAPES_3D):
        save_case(d, f"case{i}", _softmax((n_classes,) + shape, 40 + 7 * i + n_classes)[None])
    assert not os.path.exists(os.path.join(d, "pred_entropy"))


def _write_2d(base, n_classes=3):
    from values_amd.image_io import write_png, write_tiff_f32
    from values_amd.results import results_dir
    d = results_dir(str(base), "Softmax", "fold0", "id")
    os.makedirs(os.path.join(d, "pred_seg"))
    os.makedirs(os.path.join(d, "pred_prob"))
    for i, (h, w) in enumerate(SHAPES_2D):
        p = _softmax((n_classes, h, w), 90 + i).astype(np.float32)
        write_png(os.path.join(d, "pred_seg", f"img{i}_01.png"), p.argmax(0).astype(np.uint8))
        for c in range(n_classes):
            write_tiff_f32(os.path.join(d, "pred_prob", f"img{i}_01_{c + 1:02d}.tif"), p[c])


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """per tree kind: (directory of the untouched tree, the host dataloader built on a copy of it)"""
    from values_amd.experiment import ExperimentDataloader
    out = {}
    for key, write, n_classes, ending in (("c2", _write_3d, 2, ".nii.gz"), ("c3", _write_3d, 3, ".nii.gz"), ("2d", _write_2d, 3, ".tif")):
        root = tmp_path_factory.mktemp(f"softmax_{key}")
        write(root / "src", n_classes)
        shutil.copytree(root / "src", root / "host")
        out[key] = (root / "src", ExperimentDataloader(_version(root / "host", n_classes, ending), "id"), n_classes, ending)
    return out


def _device_loader(src, dst, n_classes, ending, monkeypatch, chunk=None):
    """the device dataloader on a fresh copy of the tree -> (dataloader, number of one_minus_msr_batch calls)"""
    from values_amd import uncertainty
    from values_amd.experiment import DeviceExperimentDataloader
    shutil.copytree(src, dst)
    calls = []
    real = uncertainty.one_minus_msr_batch
    monkeypatch.setattr(uncertainty, "one_minus_msr_batch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    if chunk is not None:
        monkeypatch.setattr(DeviceExperimentDataloader, "softmax_chunk", chunk)
    dl = DeviceExperimentDataloader(_version(dst, n_classes, ending), "id")
    return dl, len(calls)


def _same_tree(host_dl, dev_dl, ending):
    from values_amd import nifti
    a, b = host_dl.dataset_path / "pred_entropy", dev_dl.dataset_path / "pred_entropy"
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names == [f"{i}{ending}" for i in host_dl.image_ids]
    for n in names:
        ha, hb = open(a / n, "rb").read(), open(b / n, "rb").read()
        if ending == ".nii.gz":
            ha, hb = gzip.decompress(ha), gzip.decompress(hb)
            assert nifti.parse_header(hb).dtype == np.float64
            assert ha[:352] == hb[:352], n
        assert ha == hb, n


@pytest.mark.parametrize("chunk", [1, 2, 32])
@pytest.mark.parametrize("key", ["c2", "c3"])
def test_3d_tree_equals_the_host_tree(trees, tmp_path, monkeypatch, key, chunk):
    src, host_dl, n_classes, ending = trees[key]
    dev_dl, calls = _device_loader(src, tmp_path / "dev", n_classes, ending, monkeypatch, chunk)
    assert dev_dl.image_ids == host_dl.image_ids == ["case0", "case1", "case2"]
    assert calls == math.ceil(3 / chunk)
    _same_tree(host_dl, dev_dl, ending)


def test_2d_tree_is_byte_identical(trees, tmp_path, monkeypatch):
    src, host_dl, n_classes, ending = trees["2d"]
    dev_dl, calls = _device_loader(src, tmp_path / "dev", n_classes, ending, monkeypatch)
    assert calls == 1 and dev_dl.image_ids == ["img0", "img1"]
    _same_tree(host_dl, dev_dl, ending)


@pytest.mark.parametrize("key,chunk", [("c3", 2), ("2d", 1)])
def test_the_device_path_is_taken(trees, tmp_path, monkeypatch, key, chunk):
    """no host codec is touched: they all raise, and the tree is still built, by ceil(images / chunk) batched calls"""
    from values_amd import image_io, nifti
    src, host_dl, n_classes, ending = trees[key]

    def refuse(*a, **k):
        raise AssertionError("host codec called")
    for mod, name in ((nifti, "load"), (nifti, "save"), (image_io, "read_tiff_f32"), (image_io, "write_tiff_f32")):
        monkeypatch.setattr(mod, name, refuse)
    dev_dl, calls = _device_loader(src, tmp_path / "dev", n_classes, ending, monkeypatch, chunk)
    assert calls == math.ceil(len(host_dl.image_ids) / chunk)
    monkeypatch.undo()
    _same_tree(host_dl, dev_dl, ending)


def test_an_existing_directory_is_left_alone(trees, tmp_path, monkeypatch):
    src, host_dl, n_classes, ending = trees["c2"]
    shutil.copytree(host_dl.exp_version.base_path, tmp_path / "pre")     # a tree that already has its pred_entropy/
    pe = tmp_path / "pre" / "Softmax" / "test_results" / "fold0" / "id" / "pred_entropy"
    with open(pe / "case0.nii.gz", "wb") as f:
        f.write(b"not a volume")
    before = {n: (open(pe / n, "rb").read(), os.stat(pe / n).st_mtime_ns) for n in sorted(os.listdir(pe))}
    dev_dl, calls = _device_loader(tmp_path / "pre", tmp_path / "dev", n_classes, ending, monkeypatch)
    assert calls == 0
    pe = dev_dl.dataset_path / "pred_entropy"
    assert {n: open(pe / n, "rb").read() for n in sorted(os.listdir(pe))} == {n: v[0] for n, v in before.items()}


def test_get_max_softmax_pred_is_a_device_tensor_equal_to_the_host_array(trees, tmp_path, monkeypatch):
    for key in ("c3", "2d"):
        src, host_dl, n_classes, ending = trees[key]
        dev_dl, _ = _device_loader(src, tmp_path / f"dev_{key}", n_classes, ending, monkeypatch)
        for image_id in host_dl.image_ids:
            want = host_dl.get_max_softmax_pred(image_id)
            got = dev_dl.get_max_softmax_pred(image_id)
            assert isinstance(got, torch.Tensor) and got.is_cuda
            assert got.shape == want.shape and str(got.dtype).replace("torch.", "") == want.dtype.name
            assert (got.cpu().numpy() == want).all()


def test_a_write_error_surfaces_from_the_constructor(trees, tmp_path, monkeypatch):
    from values_amd import _devio
    src, host_dl, n_classes, ending = trees["c2"]
    # pred_entropy is a file: the directory cannot be made
    shutil.copytree(src, tmp_path / "blocked")
    blocked = tmp_path / "blocked" / "Softmax" / "test_results" / "fold0" / "id" / "pred_entropy"
    with open(blocked, "wb") as f:
        f.write(b"in the way")
    with pytest.raises(OSError):
        _device_loader(tmp_path / "blocked", tmp_path / "dev_blocked", n_classes, ending, monkeypatch)
    # a writer thread fails on one file: the constructor waits for the writer and re-raises its error
    real = _devio.write_span

    def failing(path, *a, **k):
        if os.path.basename(path).startswith("case1"):
            raise OSError(28, "no space left on device", str(path))
        return real(path, *a, **k)
    monkeypatch.setattr(_devio, "write_span", failing)
    with pytest.raises(OSError, match="no space left"):
        _device_loader(src, tmp_path / "dev_full", n_classes, ending, monkeypatch, chunk=1)
