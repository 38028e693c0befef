"""GPU: vx_label_switch_batched against the host mirror (values_amd.dataset2d), the device test loader against the host
loader, the experiment getters and the run_test_2d driver.  Every comparison is on integers or bits and exact."""
import ctypes as C
import filecmp
import json
import os

import numpy as np
import pytest
import torch

from tests.dataset2d_trees import IDS, MEAN, STD, augmentations, datamodule_config, make_tree
from values_amd import _lib, dataset2d as d2, gta

pytestmark = pytest.mark.gpu
DTYPES = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
SIZES = [(1, 1), (3, 5), (17, 33), (64, 67), (256, 478)]
SENT, FSENT, MARGIN = 0xA7, -7.5, 64


def _maps(es, sizes=SIZES, seed=0):
    rng = np.random.default_rng(100 + seed)
    out = []
    for h, w in sizes:
        m = IDS[rng.integers(0, len(IDS), size=(h, w))].astype(DTYPES[es])
        m.reshape(-1)[:len(IDS)] = IDS[:m.size]
        out.append(m)
    return out


class Call:
    """one vx_label_switch_batched call with sentinel-filled outputs and 64 bytes of margin on each side"""

    def __init__(self, maps, R, refs=True, variance=True, shift=False, indices=None):
        self.maps, self.R, self.n = maps, R, len(maps)
        self.arr = (_lib.LswitchItem * self.n)()
        self.lab, self.rbuf, self.vbuf = [], [], []
        self.status = torch.full((self.n,), -3, dtype=torch.int32, device="cuda")
        for i, m in enumerate(maps):
            es, (h, w) = m.dtype.itemsize, m.shape
            off = 1 if (shift and i % 2 == 0) else 0          # pointers one element past an aligned address
            lab = torch.zeros(m.size + 1, dtype=getattr(torch, m.dtype.name), device="cuda")
            lab[off:off + m.size] = torch.from_numpy(m.reshape(-1)).cuda()
            self.lab.append(lab)
            it = self.arr[i]
            it.labels, it.H, it.W, it.kind = lab.data_ptr() + off * es, h, w, {1: 0, 2: 1, 4: 2, 8: 3}[es]
            it.index = i if indices is None else indices[i]
            rb = torch.full((2 * MARGIN + R * h * w + 1,), SENT, dtype=torch.uint8, device="cuda")
            vb = torch.full((2 * MARGIN // 4 + h * w + 1,), FSENT, dtype=torch.float32, device="cuda")
            self.rbuf.append((rb, MARGIN + off))
            self.vbuf.append((vb, MARGIN // 4 + off))
            if refs:
                it.refs = rb.data_ptr() + MARGIN + off
            if variance:
                it.variance = vb.data_ptr() + MARGIN + 4 * off
        self.has_refs, self.has_var = refs, variance

    def run(self, seed=0, decisions=None, **kw):
        d2.label_switch_call(self.arr, self.n, self.R, self.status, seed, decisions, **kw)
        torch.cuda.synchronize()
        return self

    def refs(self, i):
        h, w = self.maps[i].shape
        rb, o = self.rbuf[i]
        return rb[o:o + self.R * h * w].cpu().numpy().reshape(self.R, h, w)

    def var(self, i):
        h, w = self.maps[i].shape
        vb, o = self.vbuf[i]
        return vb[o:o + h * w].cpu().numpy().reshape(w, h)

    def margins_untouched(self, everything=False):
        for i, m in enumerate(self.maps):
            n = m.size
            rb, o = self.rbuf[i]
            rb = rb.cpu().numpy()
            used = self.R * n if (self.has_refs and not everything) else 0
            assert (rb[:o] == SENT).all() and (rb[o + used:] == SENT).all(), f"item {i}: refs margin"
            vb, o = self.vbuf[i]
            vb = vb.cpu().numpy()
            used = n if (self.has_var and not everything) else 0
            assert (vb[:o] == FSENT).all() and (vb[o + used:] == FSENT).all(), f"item {i}: variance margin"


def _want_refs(m, R, dec):
    return np.asarray(d2.label_switch_references(m.astype(np.int64), R, dec)).reshape((R,) + m.shape).astype(np.uint8)


def _check(call, decisions, who=""):
    for i, m in enumerate(call.maps):
        if call.has_refs:
            np.testing.assert_array_equal(call.refs(i), _want_refs(m, call.R, decisions[i]), err_msg=f"{who} item {i} refs")
        if call.has_var:
            np.testing.assert_array_equal(call.var(i).view(np.uint32), gta._switch_variance(m).view(np.uint32),
                                          err_msg=f"{who} item {i} variance")
    call.margins_untouched()
    assert call.status.cpu().tolist() == [0] * call.n


@pytest.mark.parametrize("R", [1, 5, 31])
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_kernel_equals_the_mirror_with_given_decisions(es, R):
    maps = _maps(es, seed=es)
    rng = np.random.default_rng(es * 100 + R)
    dec = rng.integers(0, 2, size=(len(maps), R, 5), dtype=np.uint8)
    dec[0] = 1
    dec[1] = 0
    for refs, variance in ((True, True), (True, False), (False, True)):
        for shift in (False, True):
            _check(Call(maps, R, refs, variance, shift).run(decisions=dec), dec, f"es={es} R={R} batch shift={shift}")
    for i in range(len(maps) - 1):      # every size alone (the large one is covered by the batch-independence test)
        _check(Call([maps[i]], R, shift=True).run(decisions=dec[i:i + 1]), dec[i:i + 1], f"es={es} R={R} alone {i}")


def test_drawn_decisions_equal_switch_decisions_and_do_not_depend_on_the_batch():
    seed, R = 4242, 5
    maps = _maps(8, SIZES[:4] + [(40, 130), (33, 129), (256, 478)], seed=9)
    indices = [3, 0, 17, 2 ** 31 + 5, 1000, 6, 7]
    dec = d2.switch_decisions(seed, indices, R)
    assert 0 < dec.sum() < dec.size
    batch = Call(maps, R, indices=indices).run(seed=seed)
    _check(batch, dec, "batch of 7")
    rev = Call(maps[::-1], R, indices=indices[::-1], shift=True).run(seed=seed)
    for i in range(len(maps)):
        alone = Call([maps[i]], R, indices=[indices[i]]).run(seed=seed)
        j = len(maps) - 1 - i
        assert alone.refs(0).tobytes() == batch.refs(i).tobytes() == rev.refs(j).tobytes()
        assert alone.var(0).tobytes() == batch.var(i).tobytes() == rev.var(j).tobytes()
    other = Call(maps[-1:], R, indices=indices[-1:]).run(seed=seed + 1)
    assert other.refs(0).tobytes() != batch.refs(len(maps) - 1).tobytes()


def test_variance_is_the_host_hook_bit_for_bit_with_swapped_axes():
    lab = np.arange(256, dtype=np.int64).repeat(3).reshape(24, 32)       # every label value
    c = Call([lab, lab.T.copy()], 1, refs=False).run()
    for i, m in enumerate(c.maps):
        want = gta._switch_variance(m)
        assert c.var(i).shape == want.shape == m.shape[::-1]
        np.testing.assert_array_equal(c.var(i).view(np.uint32), want.view(np.uint32))
    assert np.count_nonzero(c.var(0)) == 15


def test_labels_outside_uint8_are_counted_and_the_loader_names_the_file(tmp_path):
    maps = _maps(8, [(17, 33), (3, 5)])
    maps[0][4, 7], maps[0][16, 32], maps[0][0, 0] = 300, -1, 2 ** 40 + 1
    c = Call(maps, 5).run(seed=1)
    assert c.status.cpu().tolist() == [3, 0]
    r = c.refs(0)
    assert (r[:, 4, 7] == 255).all() and (r[:, 16, 32] == 255).all() and (r[:, 0, 0] == 255).all()
    clean = maps[0].copy()
    clean[4, 7] = clean[16, 32] = clean[0, 0] = 255
    np.testing.assert_array_equal(r, _want_refs(clean, 5, d2.switch_decisions(1, [0], 5)[0]))
    c.margins_untouched()
    c2 = Call(_maps(2, [(3, 5)]), 1)
    c2.lab[0][2] = -2
    assert c2.run().status.cpu().tolist() == [1]
    base, splits, ids = make_tree(tmp_path)
    ds = d2.CityscapesTestSet(splits, base, split="id_test", transforms=d2.parse_test_transforms(augmentations(5)))
    bad = np.load(ds.masks[2])
    bad[1, 1] = 300
    np.save(ds.masks[2], bad)
    with d2.DeviceTestLoader2D(ds, 2, seed=3) as loader:
        with pytest.raises(ValueError, match="labels/g007.npy"):
            list(loader)
        with pytest.raises(ValueError, match="labels/g007.npy"):
            loader.reference_segs("g007")


def test_every_refusal_returns_its_code_and_writes_nothing():
    lib = _lib.load()
    E_NULL, E_SHAPE, E_DTYPE, E_WS, E_ALIGN = -1, -2, -3, -4, -5
    maps = _maps(8, [(3, 5), (17, 33)])
    c = Call(maps, 5)
    rows = d2.switch_rows()
    vt = d2.switch_variance_table()
    ws = torch.empty(int(lib.vx_label_switch_batched_workspace_bytes(2, 5)) + 16, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0 and ws.numel() > 16
    dec = np.zeros((2, 5, 5), dtype=np.uint8)

    def call(items=c.arr, n=2, R=5, rows=rows, ns=5, dec=None, vt=vt, status=c.status, wsp=ws.data_ptr(), wsn=ws.numel() - 16):
        return lib.vx_label_switch_batched(items, n, R, rows, ns, None if dec is None else dec.ctypes.data_as(C.c_void_p), 7,
                                           None if vt is None else vt.ctypes.data_as(C.POINTER(C.c_float)),
                                           None if status is None else C.c_void_p(status.data_ptr()), C.c_void_p(wsp) if wsp else None,
                                           wsn, _lib.stream_ptr())

    def item(**kw):
        arr = (_lib.LswitchItem * 2)()
        for i in range(2):
            for f, _ in _lib.LswitchItem._fields_:
                setattr(arr[i], f, getattr(c.arr[i], f))
        for k, v in kw.items():
            setattr(arr[1], k, v)
        return arr

    def table(*triples):
        r = (_lib.LswitchRow * len(triples))()
        for k, (f, t, thr) in enumerate(triples):
            r[k].from_, r[k].to, r[k].thr = f, t, thr
        return r

    bad_dec = dec.copy()
    bad_dec[1, 4, 4] = 2
    cases = [(dict(items=None), E_NULL), (dict(rows=None), E_NULL), (dict(items=item(labels=None)), E_NULL),
             (dict(status=None), E_NULL), (dict(wsp=0), E_NULL), (dict(vt=None), E_NULL),
             (dict(R=0), E_SHAPE), (dict(R=32), E_SHAPE), (dict(n=0), E_SHAPE), (dict(n=_lib.VX_SELECT_MAX_ITEMS + 1), E_SHAPE),
             (dict(ns=0), E_SHAPE), (dict(ns=9), E_SHAPE), (dict(items=item(H=0)), E_SHAPE), (dict(items=item(W=-1)), E_SHAPE),
             (dict(items=item(H=65536, W=32768)), E_SHAPE), (dict(dec=bad_dec), E_SHAPE),
             (dict(rows=table((1, 19, 5), (1, 20, 5)), ns=2), E_SHAPE),      # two rows from one label
             (dict(rows=table((1, 19, 5), (19, 20, 5)), ns=2), E_SHAPE),     # a `to` that is a `from`
             (dict(rows=table((1, 256, 5)), ns=1), E_SHAPE), (dict(rows=table((-1, 2, 5)), ns=1), E_SHAPE),
             (dict(rows=table((1, 2, 2 ** 24 + 1)), ns=1), E_SHAPE),
             (dict(items=item(kind=4)), E_DTYPE), (dict(items=item(kind=-1)), E_DTYPE),
             (dict(items=item(labels=c.arr[1].labels + 4)), E_ALIGN), (dict(items=item(variance=c.arr[1].variance + 2)), E_ALIGN),
             (dict(wsp=ws.data_ptr() + 8), E_ALIGN), (dict(wsn=int(lib.vx_label_switch_batched_workspace_bytes(2, 5)) - 1), E_WS)]
    for kw, code in cases:
        assert call(**kw) == code, (kw.keys(), lib.vx_last_error_string())
    assert lib.vx_label_switch_batched_workspace_bytes(0, 5) == 0 and lib.vx_label_switch_batched_workspace_bytes(2, 32) == 0
    torch.cuda.synchronize()
    c.margins_untouched(everything=True)
    assert c.status.cpu().tolist() == [-3, -3]
    assert call(dec=dec) == 0      # and the same arguments, unharmed, run
    torch.cuda.synchronize()
    _check(c, dec, "after the refusals")


# ---------------------------------------------------------------------------------------------------------------------
# loader

def _loaders(tmp_path, tta, R=5, seed=21, batch=2, **tree):
    base, splits, ids = make_tree(tmp_path, **tree)
    tr = d2.parse_test_transforms(augmentations(R))
    ds = d2.CityscapesTestSet(splits, base, split="id_test", transforms=tr, tta=tta, seed=seed)
    return ds, d2.HostTestLoader2D(ds, batch), ids


@pytest.mark.parametrize("tta", [False, True])
@pytest.mark.parametrize("prefetch", [True, False])
def test_device_loader_equals_the_host_mirror(tmp_path, tta, prefetch):
    from values_amd.data import TTA_2D_VIEW_CODES, tta_views_2d_device
    ds, host, ids = _loaders(tmp_path, tta, label_dtype=np.uint8 if prefetch else np.int64)
    with d2.DeviceTestLoader2D(ds, 2, seed=21, prefetch=prefetch) as dev:
        assert dev.dataset is ds and len(dev) == len(host) == 3
        got = list(dev)
    want = list(host)
    assert [len(b["image_id"]) for b in got] == [2, 2, 1]
    first = 0
    for g, w in zip(got, want):
        B = len(w["image_id"])
        assert g["image_id"] == list(w["image_id"]) and g["dataset"] == list(w["dataset"])
        assert g["seg"].is_cuda and g["seg"].dtype == torch.uint8 and tuple(g["seg"].shape) == (B, 5, 17, 33)
        np.testing.assert_array_equal(g["seg"].cpu().numpy(), w["seg"].numpy().astype(np.uint8))
        G = 4 if tta else 1
        assert g["data"].is_cuda and tuple(g["data"].shape) == (G, B, 17, 33, 4) and ("transforms" in g) == tta
        data = g["data"].cpu().numpy()
        assert (data[..., 3] == 0).all()
        views = w["data"] if tta else [w["data"]]
        for v in ((0, 1) if tta else (0,)):      # the clean views, bit for bit against tta_views_2d
            np.testing.assert_array_equal(data[v, ..., :3].view(np.uint32), views[v].numpy().transpose(0, 2, 3, 1).view(np.uint32))
        if tta:
            assert g["transforms"] == [[], ["HorizontalFlip"], ["GaussNoise"], ["HorizontalFlip", "GaussNoise"]]
            img = torch.from_numpy(np.stack([np.load(ds.imgs[first + b]) for b in range(B)]))
            by_hand, _ = tta_views_2d_device(img, MEAN, STD, view_codes=TTA_2D_VIEW_CODES, noise_seed=21, image_index0=first)
            assert torch.equal(by_hand, g["data"])
            assert not torch.equal(g["data"][2], g["data"][0])      # the noisy views carry noise
        first += B


def test_device_loader_refuses_a_mixed_batch_and_needs_a_seed(tmp_path):
    ds, host, ids = _loaders(tmp_path, False)
    with pytest.raises(ValueError, match="seed"):
        d2.DeviceTestLoader2D(ds, 2, seed=None)
    np.save(ds.imgs[1], np.zeros((9, 33, 3), dtype=np.uint8))
    np.save(ds.masks[1], np.zeros((9, 33), dtype=np.int64))
    with d2.DeviceTestLoader2D(ds, 2, seed=1) as dev:
        with pytest.raises(ValueError, match="one size"):
            list(dev)


# ---------------------------------------------------------------------------------------------------------------------
# experiment

def _experiment(tmp_path, device_io):
    from values_amd.experiment import DeviceExperimentDataloader, ExperimentVersion
    base, splits, ids = make_tree(tmp_path / "data")
    cfg = datamodule_config(base, splits, seed=13, device_io=device_io)
    ev = ExperimentVersion(tmp_path / "exp", "v1", "Dropout", ".png", ".tif", ["predictive_uncertainty"], [], 5,
                           datamodule_config=cfg, gt_unc_map_loading={"_target_": "evaluation.utils.gta.gt_unc_map"})
    os.makedirs(ev.exp_path / "id" / "pred_seg", exist_ok=True)
    return DeviceExperimentDataloader(ev, "id"), ids


def test_experiment_getters_with_the_device_loader_and_with_the_host_loader(tmp_path):
    dev, ids = _experiment(tmp_path / "a", True)
    host, _ = _experiment(tmp_path / "b", False)
    assert isinstance(dev.dataloader, d2.DeviceTestLoader2D) and isinstance(host.dataloader, d2.HostTestLoader2D)
    for k, image_id in enumerate(ids):
        r1, r2 = dev.get_reference_segs(image_id), dev.get_reference_segs(image_id)
        assert r1.is_cuda and r1.dtype == torch.uint8 and tuple(r1.shape) == (5, 17, 33) and torch.equal(r1, r2)
        h = host.get_reference_segs(image_id)                     # what it returns today: the dataset item, squeezed, as numpy
        assert isinstance(h, np.ndarray) and h.dtype == np.int64
        np.testing.assert_array_equal(h, host.dataloader.dataset[k]["seg"].squeeze().numpy())
        np.testing.assert_array_equal(r1.cpu().numpy(), h.astype(np.uint8))      # same seed: same raters
        want = gta.gt_unc_map(image_id, host.dataloader)
        m = dev.get_gt_unc_map(image_id)
        assert m.is_cuda and m.dtype == torch.float32 and tuple(m.shape) == (33, 17)
        np.testing.assert_array_equal(m.cpu().numpy().view(np.uint32), want.view(np.uint32))
        mh = host.get_gt_unc_map(image_id)                        # the host read, uploaded
        assert mh.is_cuda and torch.equal(mh, m)
    dev.dataloader.close()


# ---------------------------------------------------------------------------------------------------------------------
# driver

def _model(ncls=24):
    from tests.formula import formula_state_dict_from_shapes
    from tests.test_gpu_hrnet import small_cfg
    from values_amd.hrnet import HighResolutionNet
    m = HighResolutionNet(small_cfg(dropout_final=False, ncls=ncls))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = {k: torch.from_numpy(v).float() for k, v in formula_state_dict_from_shapes(shapes).items()}
    m.load_state_dict(sd, strict=False)
    return m.cuda()


def _tree_files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_run_test_2d_device_and_host_loaders_write_the_same_tree(tmp_path):
    from values_amd.metrics import process_metrics_2d
    from values_amd.predict2d import predict_logits_2d, process_output_2d, run_test_2d
    ds, host, ids = _loaders(tmp_path / "data", False, seed=5, H=64, W=96)
    model = _model()
    with d2.DeviceTestLoader2D(ds, 2, seed=5) as dev:
        res_d = run_test_2d([model], dev, str(tmp_path / "dev"))
        by_hand = {}
        for batch in dev:
            out = process_output_2d(predict_logits_2d([model], batch["data"], nhwc=True))
            by_hand.update(process_metrics_2d(out, batch["seg"], image_ids=batch["image_id"]))
    res_h = run_test_2d([model], host, str(tmp_path / "host"))
    files = _tree_files(tmp_path / "dev")
    assert files == _tree_files(tmp_path / "host")
    assert sorted(f for f in files if f.startswith("pred_seg")) == sorted(f"pred_seg/{i}_01.png" for i in ids)
    assert "metrics.json" in files and sum(f.startswith("pred_entropy/") for f in files) == 5
    for f in files:
        assert filecmp.cmp(tmp_path / "dev" / f, tmp_path / "host" / f, shallow=False), f
    assert res_d == res_h and json.load(open(tmp_path / "dev" / "metrics.json")) == res_d
    assert list(res_d) == ids + ["mean"]
    for i, ds_name in zip(ids, ["gta"] * 3 + ["cs"] * 2):
        assert res_d[i]["dataset"] == ds_name and res_d[i]["metrics"] == by_hand[i]
        assert set(res_d[i]["metrics"]) >= {"dice", "ged"}
