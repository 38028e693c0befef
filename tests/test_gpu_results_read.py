"""GPU: reading the results tree on the device -- gz.gunzip (vx_inflate) against zlib on a generated corpus and a
corrupt set (the same statuses as the host reference decoder of inflate_core.h), nifti.load_device (vx_nifti_decode)
against nifti.load, and the device consumers (DeviceExperimentDataloader, aggregate_uncertainties_device,
find_threshold(device_io=True)) against the host paths."""
import gzip
import json
import os
import struct
import tempfile

import numpy as np
import pytest
import torch

from tests import inflate_corpus as ic

pytestmark = pytest.mark.gpu

FMT = {ic.GZIP: "gzip", ic.ZLIB: "zlib", ic.RAW: "raw"}


def _raw_inflate(items):
    """items: [(format, bytes, capacity)] -> [(status, bytes)] from one vx_inflate call"""
    from values_amd import gz
    srcs = [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if b else torch.empty(0, dtype=torch.uint8, device="cuda")
            for _, b, _ in items]
    dst, offs, sizes, st = gz.inflate_into([(s.data_ptr() if s.numel() else None, s.numel(), f, c)
                                            for s, (f, _, c) in zip(srcs, items)], torch.device("cuda"))
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    return [(s, host[o:o + n].tobytes()) for s, o, n in zip(st, offs, sizes)]


def test_gunzip_corpus_mixed_batch_matches_zlib():
    from values_amd import gz
    corpus = ic.good_corpus()
    rng = np.random.default_rng(3)
    members = [rng.integers(0, 4, n, dtype=np.uint8) for n in (0, 1, 40000, 200001)]
    enc = gz.gzip_encode([torch.from_numpy(m).cuda() for m in members])
    names = list(corpus)
    items = [(corpus[k][0], corpus[k][1], ic.capacity_for(len(corpus[k][2]))) for k in names]
    items += [(ic.GZIP, bytes(e), len(m)) for e, m in zip(enc, members)]
    want = [corpus[k][2] for k in names] + [m.tobytes() for m in members]
    a = _raw_inflate(items)
    b = _raw_inflate(items)
    for i, ((st, out), (st2, out2)) in enumerate(zip(a, b)):
        label = names[i] if i < len(names) else f"gzip_encode_{i - len(names)}"
        assert st == ic.OK, (label, st)
        assert out == want[i], label
        assert (st2, out2) == (st, out), ("not deterministic", label)
    # the wrapper, per format
    for fmt in (ic.GZIP, ic.ZLIB, ic.RAW):
        ks = [k for k in names if corpus[k][0] == fmt]
        outs = gz.gunzip([corpus[k][1] for k in ks], fmt=FMT[fmt])
        for k, t in zip(ks, outs):
            assert t.cpu().numpy().tobytes() == corpus[k][2], k


def test_gunzip_multi_member_understated_isize_and_errors():
    from values_amd import _lib, gz
    data = [b"a" * 100000, b"b" * 10]
    blob = b"".join(gzip.compress(d) for d in data)
    out = gz.gunzip([blob, torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()])
    for t in out:
        assert t.cpu().numpy().tobytes() == b"".join(data)
    with pytest.raises(_lib.VxError, match="item 1: checksum mismatch"):
        bad = bytearray(blob)
        bad[-8] ^= 1    # the last member's CRC-32
        gz.gunzip([blob, bytes(bad)])


def test_corrupt_set_statuses_match_host_decoder():
    bad = ic.corrupt_corpus()
    names = list(bad)
    items = [(bad[k][0], bad[k][1], bad[k][2] or 1 << 16) for k in names]
    good = ic.good_corpus()
    keep = ["text_l6", "walk_zlib_l1", "walk_raw_l9", "multi_member"]
    items_all = items + [(good[k][0], good[k][1], ic.capacity_for(len(good[k][2]))) for k in keep]
    with tempfile.TemporaryDirectory() as td:
        exe = ic.build_host_decoder(td, sanitize=False)
        host = ic.run_host_decoder(exe, items, td)
    dev = _raw_inflate(items_all)
    for k, (hs, hout), (ds, dout) in zip(names, host, dev):
        assert ds == hs, (k, ds, hs)
        if bad[k][3] is not None:
            assert ds == bad[k][3], (k, ds)
        assert dout == hout, ("bytes written", k)
    for k, (ds, dout) in zip(keep, dev[len(items):]):
        assert ds == ic.OK and dout == good[k][2], k


def _same(dev, host):
    (t, h), (a, ha) = dev, host
    assert t.is_cuda
    got = t.cpu().numpy()
    assert got.dtype == a.dtype and got.shape == a.shape
    np.testing.assert_array_equal(got, a)
    assert h["pixdim"] == ha["pixdim"] and h["datatype"] == ha["datatype"]
    np.testing.assert_array_equal(h["affine"], ha["affine"])


def test_load_device_matches_load(tmp_path):
    from values_amd import nifti
    rng = np.random.default_rng(11)
    paths = []
    hdr = {"pixdim": [0.7, 0.8, 2.5], "affine": np.diag([0.7, -0.8, 2.5, 1.0])}
    shapes = [(1, 1, 1), (65, 3, 17), (64, 64, 64), (7,), (5, 9), (3, 4, 5, 6), (2, 3, 1, 2, 3, 2, 2)]
    for dt in nifti._DT:
        for si, shp in enumerate(shapes):
            if dt.itemsize == 8 and shp == (64, 64, 64) and dt != np.float64:
                continue
            a = (rng.random(shp) * 200 - 50).astype(dt) if dt.kind == "f" else rng.integers(0, 100, shp).astype(dt)
            p = str(tmp_path / f"{dt.name}_{si}.nii") + (".gz" if si % 2 == 0 else "")
            nifti.save(a, p, hdr if si == 1 else None)
            paths.append(p)
    # big endian
    a = rng.random((6, 7, 8)).astype(np.float32)
    h = bytearray(nifti.header_bytes(a.shape, a.dtype))
    be = bytearray(352)
    for off, fmt in ((0, "i"), (40, "8h"), (70, "h"), (72, "h"), (76, "8f"), (108, "f"), (112, "2f"), (280, "12f")):
        struct.pack_into(">" + fmt, be, off, *struct.unpack_from("<" + fmt, h, off))
    be[344:348] = h[344:348]
    raw = bytes(be) + np.asfortranarray(a).astype(">f4").tobytes(order="F")
    open(tmp_path / "be.nii", "wb").write(raw)
    open(tmp_path / "be.nii.gz", "wb").write(gzip.compress(raw))
    paths += [str(tmp_path / "be.nii"), str(tmp_path / "be.nii.gz")]
    # slope / intercept
    for dt in (np.uint8, np.int16, np.float32, np.float64, np.uint64):
        h = bytearray(nifti.header_bytes((9, 10, 11), np.dtype(dt)))
        struct.pack_into("<2f", h, 112, 0.37, -1.25)
        p = tmp_path / f"scaled_{np.dtype(dt).name}.nii.gz"
        open(p, "wb").write(gzip.compress(bytes(h) + rng.integers(0, 100, 990).astype(dt).tobytes()))
        paths.append(str(p))
    # several members (ISIZE is the last member's size)
    a = rng.random((30, 20, 10))
    nifti.save(a, str(tmp_path / "one.nii"))
    raw = open(tmp_path / "one.nii", "rb").read()
    open(tmp_path / "multi.nii.gz", "wb").write(gzip.compress(raw[:1000]) + gzip.compress(raw[1000:]))
    paths.append(str(tmp_path / "multi.nii.gz"))
    dev = nifti.load_device(paths)
    for p, d in zip(paths, dev):
        _same(d, nifti.load(p))
    again = nifti.load_device(paths[::-1])
    for p, d in zip(paths[::-1], again):
        _same(d, nifti.load(p))
    with nifti.NiftiReader() as r:
        batches = [paths[i:i + 7] for i in range(0, len(paths), 7)]
        for b, res in zip(batches, r.read(batches)):
            for p, d in zip(b, res):
                _same(d, nifti.load(p))


def _lidc_tree(root, n=3):
    from values_amd.results import ResultsWriter, results_dir
    d = results_dir(str(root), "Dropout", "fold0_seed123", "id")
    with ResultsWriter(workers=2) as w:
        for i in range(n):
            g = torch.Generator(device="cuda").manual_seed(i)
            sm = torch.softmax(torch.randn(3, 2, 20, 24, 16, device="cuda", generator=g) * 3, 1)
            maps = {k: torch.rand(20, 24, 16, device="cuda", generator=g) * 0.5 for k in
                    ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")}
            gt = torch.rand(2, 20, 24, 16, generator=torch.Generator().manual_seed(i)) > 0.8
            w.submit(d, f"case{i}", softmax_pred=sm, maps=maps, data=sm[0, 0].cpu().numpy(), gt_seg=gt)
    return d


def test_save_case_files_read_back(tmp_path):
    from values_amd import nifti
    from values_amd.results import save_case, save_case_device
    sm = torch.softmax(torch.randn(2, 2, 17, 9, 5, device="cuda"), 1)
    save_case(str(tmp_path / "h"), "c", sm, {"pred_entropy": sm[0, 0].clone()})
    save_case_device(str(tmp_path / "d"), "c", sm, {"pred_entropy": sm[0, 0].clone()})
    files = [os.path.join(r, f) for base in ("h", "d") for r, _, fs in os.walk(tmp_path / base) for f in fs]
    assert len(files) > 10
    for p, d in zip(files, nifti.load_device(files)):
        _same(d, nifti.load(p))


def test_device_consumers_match_host(tmp_path):
    from values_amd import thresholds
    from values_amd.experiment import (DeviceExperimentDataloader, ExperimentDataloader, ExperimentVersion,
                                       aggregate_uncertainties, aggregate_uncertainties_device)
    _lidc_tree(tmp_path)
    ev = ExperimentVersion(base_path=tmp_path, naming_scheme_version="fold{fold}_seed{seed}", pred_model="Dropout",
                           image_ending=".nii.gz", unc_ending=".nii.gz",
                           unc_types=["predictive_uncertainty", "aleatoric_uncertainty", "epistemic_uncertainty"],
                           aggregations=None, n_reference_segs=2, fold=0, seed=123)
    host, dev = ExperimentDataloader(ev, "id"), DeviceExperimentDataloader(ev, "id")
    assert host.image_ids == dev.image_ids == ["case0", "case1", "case2"]
    assert dev.prefetch(["case1"]) > 0
    for i in host.image_ids:
        for u in ev.unc_types:
            t = dev.get_unc_map(i, u)
            assert t.is_cuda
            np.testing.assert_array_equal(t.cpu().numpy(), host.get_unc_map(i, u))
        np.testing.assert_array_equal(dev.get_mean_pred_seg(i).cpu().numpy(), host.get_mean_pred_seg(i))
        hs = sorted(host.get_pred_segs(i), key=lambda a: a.tobytes())
        ds = sorted((t.cpu().numpy() for t in dev.get_pred_segs(i)), key=lambda a: a.tobytes())
        for a, b in zip(hs, ds):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(dev.get_reference_segs(i).cpu().numpy(), host.get_reference_segs(i))
        np.testing.assert_array_equal(dev.get_gt_unc_map(i), host.get_gt_unc_map(i))
    aggs = {"patch_level": {"_target_": "values_amd.aggregation.patch_level_aggregation", "patch_size": 5},
            "image_level": {"_target_": "values_amd.aggregation.image_level_aggregation", "mean": True},
            "threshold": {"_target_": "values_amd.aggregation.threshold_aggregation", "threshold": 0.2}}
    aggregate_uncertainties(host, aggs)
    want = {u: open(host.dataset_path / f"aggregated_{u}.json", "rb").read() for u in ev.unc_types}
    for u in ev.unc_types:
        os.remove(host.dataset_path / f"aggregated_{u}.json")
    aggregate_uncertainties_device(dev, aggs, batch=2)
    for u in ev.unc_types:
        assert open(host.dataset_path / f"aggregated_{u}.json", "rb").read() == want[u], u
    # thresholds: quantiles from the device pred segs, thresholds from device-read maps
    qh = thresholds.get_foreground_quantile(host)
    qd = thresholds.get_foreground_quantile(dev)
    assert qh == qd
    qdir = tmp_path / "q"
    os.makedirs(qdir)
    thresholds.save_foreground_quantiles(qh, qdir)
    paths = thresholds.threshold_images_paths(host)
    out = {}
    for dio in (False, True):
        d = tmp_path / f"t{int(dio)}"
        os.makedirs(d)
        thresholds.find_threshold(paths, qdir, d, device_io=dio)
        out[dio] = open(d / "threshold_analysis.json", "rb").read()
    assert out[True] == out[False]
    assert json.loads(out[True])["Dropout"]
