"""GPU: the device results writer -- vx_crc32 against zlib, gzip members that gzip.decompress reads back, and
save_case_device / ResultsWriter writing the tree save_case writes (same names, the same decoded bytes per file)."""
import gzip
import os
import zlib

import numpy as np
import pytest
import torch

from tests.formula import formula_volume

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("n", [0, 1, 7, 32767, 32768, 32769, 5 * MIB])
def test_crc32_matches_zlib(n):
    from values_amd import gz
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, n + 3, dtype=np.uint8)
    t = _dev(a)
    assert gz.crc32(t[:n]) == zlib.crc32(a[:n].tobytes())
    assert gz.crc32(t[3:]) == zlib.crc32(a[3:].tobytes())   # unaligned start


def _inputs():
    rng = np.random.default_rng(5)
    soft = torch.softmax(torch.from_numpy(formula_volume((2, 64, 64, 64), tag=3)).float(), 0)[0]
    mask = np.zeros((64, 64, 64), np.uint8)
    mask[20:30, 10:40, 30:34] = 1
    mask[40:44, 40:44, 40:44] = 2
    return {
        "empty": np.zeros(0, np.uint8),
        "one": np.array([42], np.uint8),
        "zeros": np.zeros(MIB, np.uint8),
        "random": rng.integers(0, 256, MIB, dtype=np.uint8),
        "softmax_f64": np.asfortranarray(soft.double().numpy()).tobytes(order="F"),
        "mask": np.asfortranarray(mask).tobytes(order="F"),
        "edge_a": rng.integers(0, 4, 32768 * 3 - 1, dtype=np.uint8),
        "edge_b": rng.integers(0, 4, 32768 * 2 + 1, dtype=np.uint8),
        "edge_c": np.tile(np.arange(100, dtype=np.uint8), 655)[:65536],
    }


def _u8(b):
    return _dev(np.frombuffer(b, np.uint8).copy() if isinstance(b, bytes) else b)


HINTS = {"softmax_f64": (8, 512, 32768), "mask": (1, 64, 4096)}


def test_gzip_encode_round_trip_batched_and_deterministic():
    from values_amd import gz
    ins = _inputs()
    names = list(ins)
    tens = [_u8(ins[k]) for k in names]
    hints = [HINTS.get(k) for k in names]
    batched = gz.gzip_encode(tens, hints)
    again = gz.gzip_encode(tens, hints)
    sizes = {}
    for k, t, h, out, out2 in zip(names, tens, hints, batched, again):
        src = bytes(np.frombuffer(ins[k], np.uint8)) if isinstance(ins[k], bytes) else ins[k].tobytes()
        assert gzip.decompress(bytes(out)) == src, k
        assert bytes(out) == bytes(out2), ("not deterministic", k)
        single = gz.gzip_encode([t], [h])[0]
        assert gzip.decompress(bytes(single)) == src, k
        assert bytes(single) == bytes(out), ("a member depends on its batch", k)
        assert len(out) <= gz.bound(len(src)), k
        sizes[k] = (len(src), len(out))
    n, c = sizes["zeros"]
    assert n / c >= 100, sizes["zeros"]           # a stored-only encoder gives < 1
    n, c = sizes["mask"]
    assert n / c >= 50, sizes["mask"]
    n, c = sizes["random"]
    assert c <= gz.bound(n)
    print("gzip sizes", sizes)


def _files(d):
    out = {}
    for root, _, fs in os.walk(d):
        for f in fs:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = p
    return out


def _same_trees(host_dir, dev_dir):
    h, d = _files(host_dir), _files(dev_dir)
    assert set(h) == set(d)
    hb = db = 0
    for k in h:
        a, b = open(h[k], "rb").read(), open(d[k], "rb").read()
        assert gzip.decompress(b) == gzip.decompress(a), k
        hb += len(a)
        db += len(b)
    return hb, db


def _sliding_case(i):
    from tests.test_gpu_unet3d import make_model
    from values_amd import predict_image_sliding
    model = make_model(do_dropout=True)
    img = torch.from_numpy(formula_volume((32, 32, 32), tag=60 + i))
    out = predict_image_sliding([model], img, patch_size=32, n_pred=4, seeds=[i])
    return img, out


def test_save_case_device_sliding_window_matches_host_and_reads_back(tmp_path):
    from values_amd.experiment import ExperimentDataloader, ExperimentVersion
    from values_amd.results import results_dir, save_case, save_case_device
    hd = results_dir(str(tmp_path / "host"), "Dropout", "fold0_seed123", "id")
    dd = results_dir(str(tmp_path / "dev"), "Dropout", "fold0_seed123", "id")
    keep = {}
    for i in range(2):
        img, out = _sliding_case(i)
        save_case(hd, f"case{i}", out["softmax_sum"], out, data=img, num_predictions=out["num_predictions"])
        save_case_device(dd, f"case{i}", out["softmax_sum"], out, data=img, num_predictions=out["num_predictions"])
        keep[f"case{i}"] = out
    hb, db = _same_trees(hd, dd)
    print(f"sliding-window tree: host {hb} B, device {db} B, ratio {db / hb:.3f}")
    assert db <= 1.25 * hb, (db, hb)
    ev = ExperimentVersion(base_path=tmp_path / "dev", naming_scheme_version="fold{fold}_seed{seed}", pred_model="Dropout",
                           image_ending=".nii.gz", unc_ending=".nii.gz",
                           unc_types=["predictive_uncertainty", "epistemic_uncertainty"], aggregations=None,
                           n_reference_segs=0, fold=0, seed=123)
    dl = ExperimentDataloader(ev, "id")
    assert dl.image_ids == ["case0", "case1"]
    np.testing.assert_array_equal(dl.get_unc_map("case1", "epistemic_uncertainty"),
                                  keep["case1"]["epistemic_uncertainty"].cpu().numpy())
    np.testing.assert_array_equal(dl.get_mean_pred_seg("case0"), keep["case0"]["pred_seg_mean"].cpu().numpy())


def _ties_case():
    """C = 3, non-cubic, exact ties between classes and a NaN"""
    rng = np.random.default_rng(11)
    T, C, X, Y, Z = 3, 3, 37, 70, 19
    sm = rng.random((T, C, X, Y, Z)).astype(np.float32)
    sm[:, 1, :5] = sm[:, 0, :5]                      # tie 0 / 1: first index wins
    sm[:, 2, 5:9] = sm[:, 1, 5:9]                    # tie 1 / 2
    sm[0, 1, 10, 10, 10] = np.nan
    sm[2, 2, 11, 3, 4] = np.nan
    sm[1, 0, 12, :, :] = 1.0
    return sm


CASES = {
    "t1": lambda: dict(softmax_pred=np.random.default_rng(1).random((1, 2, 16, 20, 24)).astype(np.float32)),
    "ties_nan": lambda: dict(softmax_pred=torch.from_numpy(_ties_case()).cuda(),
                             maps={"pred_entropy": torch.rand(37, 70, 19, device="cuda")}),
    "header": lambda: dict(softmax_pred=torch.rand(2, 2, 24, 16, 8, device="cuda", dtype=torch.float64),
                           data=np.random.default_rng(2).random((24, 16, 8)).astype(np.float32),
                           header={"pixdim": [0.7, 0.8, 2.5], "affine": np.diag([0.7, -0.8, 2.5, 1.0])}),
    "gt_int64": lambda: dict(softmax_pred=torch.rand(4, 2, 20, 20, 20, device="cuda"),
                             gt_seg=torch.randint(0, 3, (3, 20, 20, 20), dtype=torch.int64),
                             num_predictions=torch.randint(0, 4, (20, 20, 20), device="cuda").float()),
}


@pytest.mark.parametrize("case", list(CASES))
def test_save_case_device_matches_host(tmp_path, case):
    from values_amd.results import save_case, save_case_device
    kw = CASES[case]()
    save_case(str(tmp_path / "host"), "c0", **kw)
    save_case_device(str(tmp_path / "dev"), "c0", **kw)
    _same_trees(str(tmp_path / "host"), str(tmp_path / "dev"))
    if case == "t1":
        assert not any("mean" in p for p in _files(str(tmp_path / "dev")))


def test_results_writer_matches_save_case_device_and_reraises(tmp_path):
    from values_amd.results import ResultsWriter, save_case_device
    cases = []
    for i in range(3):
        g = torch.Generator(device="cuda").manual_seed(i)
        sm = torch.rand(3, 2, 24, 24, 24, device="cuda", generator=g)
        cases.append(dict(softmax_pred=sm, maps={"pred_entropy": sm[0, 0].clone()}, data=sm[1, 1].cpu().numpy()))
    for i, kw in enumerate(cases):
        save_case_device(str(tmp_path / "one"), f"c{i}", **kw)
    with ResultsWriter(workers=2) as w:
        for i, kw in enumerate(cases):
            w.submit(str(tmp_path / "pipe"), f"c{i}", **kw)
    a, b = _files(str(tmp_path / "one")), _files(str(tmp_path / "pipe"))
    assert set(a) == set(b) and len(a) == 3 * (1 + 1 + 2 + 3 * 3 + 1)
    for k in a:
        assert open(a[k], "rb").read() == open(b[k], "rb").read(), k
    # a write error surfaces at close(): a directory stands where a file is to be written
    bad = tmp_path / "bad"
    os.makedirs(bad / "pred_prob" / "c0_01_01.nii.gz")
    w = ResultsWriter(workers=2)
    w.submit(str(bad), "c0", **cases[0])
    with pytest.raises(IsADirectoryError):
        w.close()
