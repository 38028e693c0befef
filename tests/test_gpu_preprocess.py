"""GPU: the 3D preprocessing on the device (values_amd/preprocess.py over vx_volume_stats_batched and
vx_zscore_pad_batched): statistics against numpy on the widened data, the normalise-and-pad pass voxel for voxel, batch
independence bit for bit, the data set end to end against the host mirror, and the drivers.

Shapes: the smallest that reach every path -- (20, 17, 13) int16: ragged z, one work block; (40, 33, 29) int16: three
32 KB blocks, z no multiple of the vector width; 64^3 float32: no padding, whole chunks only; (5, 4, 130) uint8: padding
on z alone, a head and a tail per row; (1, 1, 1) float64; a constant volume (std = 0, the quotient by 1e-8); a volume with
a NaN; labels int32 and uint8.

Measured on an MI355X (the regression bounds below are about 5x these):
  relative deviation of the float means from numpy's   <= 2.4e-16 (float64 (9, 11, 10); contract there n * 2^-52 = 2.2e-13)
  relative deviation of std from numpy's, all kinds    <= 1.4e-16 (uint16 (3, 50, 9); contract there 3.0e-13)
  device data set vs host mirror: int16 0, uint8 max |d| / (n 2^-52 (1 + |v|)) = 1.5e-3 (contract: 4)
  float32 (9, 12, 70): the mirror's own gap to the float64 computation 4.77e-7, the device's distance from the mirror 4.77e-7
"""
import os

import numpy as np
import pytest
import torch

from tests.test_preprocess_cpu import volume, write_tree

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
# regression bounds at about 5x the measured deviation, asserted beside the contract n * 2^-52
REG_MEAN, REG_STD = 1.2e-15, 7e-16


def make_volumes():
    vols = {
        "ragged": volume((20, 17, 13), "int16", 1),
        "blocks": volume((40, 33, 29), "int16", 2),
        "vec": np.abs(volume((64, 64, 64), "float32", 3)) + np.float32(1),
        "zpad": volume((5, 4, 130), "uint8", 4),
        "one": np.full((1, 1, 1), 3.25, np.float64),
        "const": np.full((6, 5, 7), 7, np.int16),
        "f64": np.abs(volume((9, 11, 10), "float64", 5)) + 1.0,
        "i8": volume((7, 3, 33), "int8", 6),
        "u16": volume((3, 50, 9), "uint16", 7),
        "i32": volume((12, 5, 18), "int32", 8) * 70001,
    }
    nan = np.abs(volume((8, 9, 10), "float32", 9))
    nan[3, 4, 5] = np.nan
    vols["nan"] = nan
    return vols


VOLS = make_volumes()
LABELS = {"ragged": [(volume((20, 17, 13), "int16", 11) > 1500).astype(np.int32) + 2, (volume((20, 17, 13), "int16", 12) > 0).astype(np.uint8)],
          "zpad": [(volume((5, 4, 130), "uint8", 13) > 128).astype(np.uint8) + 1]}
FINITE = [k for k in VOLS if k != "nan"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


@pytest.fixture(scope="module")
def device_stats():
    """the statistics of all test volumes from ONE call, downloaded: {name: (mean, std, min, n)}"""
    from values_amd.preprocess import volume_stats_device
    names = list(VOLS)
    st = volume_stats_device([dev(VOLS[k]) for k in names]).cpu().numpy()
    return {k: st[i] for i, k in enumerate(names)}


def test_statistics_against_numpy_on_the_widened_data(device_stats):
    worst_mean, worst_std = 0.0, 0.0
    for k in FINITE:
        x = VOLS[k].astype(np.float64)
        mean, std, mn, n = device_stats[k]
        assert n == x.size and mn == x.min(), k
        bound = x.size * EPS
        if VOLS[k].dtype.kind in "iu":
            assert mean == x.mean(), (k, mean, x.mean())          # the 64-bit integer sum is exact and converted once
        else:
            rel = abs(mean - x.mean()) / abs(x.mean())
            worst_mean = max(worst_mean, rel)
            print(f"{k}: mean rel {rel:.3e} (contract {bound:.3e})")
            assert rel <= bound and rel <= REG_MEAN, (k, rel)
        if x.std() == 0:
            assert std == 0.0, k
            continue
        rel = abs(std - x.std()) / x.std()
        worst_std = max(worst_std, rel)
        print(f"{k}: std rel {rel:.3e} (contract {bound:.3e})")
        assert rel <= bound and rel <= REG_STD, (k, rel)
    print(f"worst: mean {worst_mean:.3e} std {worst_std:.3e}")
    assert device_stats["const"][0] == 7.0 and device_stats["one"][0] == 3.25 and device_stats["one"][1] == 0.0
    assert np.isnan(device_stats["nan"][:3]).all() and device_stats["nan"][3] == VOLS["nan"].size


@pytest.mark.parametrize("out_dtype", [None, torch.float32, torch.float64])
def test_normalise_and_pad_exactly(out_dtype):
    """every output voxel == the numpy float64 expression on the device's own statistics row, rounded once"""
    from values_amd.preprocess import pad_sizes, preprocess_batch_device
    names = list(VOLS)
    labels = [[dev(l) for l in LABELS.get(k, [])] for k in names]
    images, labs, stats = preprocess_batch_device([dev(VOLS[k]) for k in names], labels, out_dtype=out_dtype)
    assert stats.shape == (len(names), 4) and stats.dtype == torch.float64 and stats.is_cuda
    st = stats.cpu().numpy()
    for i, k in enumerate(names):
        x = VOLS[k]
        new, split = pad_sizes(x.shape)
        mean, std, mn, n = st[i]
        want_dt = {None: np.float32 if x.dtype == np.float32 else np.float64, torch.float32: np.float32, torch.float64: np.float64}[out_dtype]
        with np.errstate(invalid="ignore"):
            inside = (x.astype(np.float64) - mean) / (std + 1e-8)
            fill = (mn - mean) / (std + 1e-8)
        want = np.pad(inside, split, "constant", constant_values=fill).astype(want_dt)
        got = images[i].cpu().numpy()
        assert got.dtype == want_dt and got.shape == new == want.shape, k
        assert images[i].is_contiguous()
        if k == "nan":
            assert np.isnan(got).all()
            continue
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (k, out_dtype, len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
        if k == "const":
            assert (got == 0).all()
        for l, g in zip(LABELS.get(k, []), labs[i]):
            wl = np.pad(l, split, "constant", constant_values=l.min())
            gl = g.cpu().numpy()
            assert gl.dtype == l.dtype and gl.shape == new and np.array_equal(gl, wl), k
    assert [len(l) for l in labs] == [len(LABELS.get(k, [])) for k in names]


def test_batch_independence_bit_for_bit():
    """an item's statistics and output alone, first in a batch of 7 and last in it: the same bits"""
    from values_amd.preprocess import preprocess_batch_device, volume_stats_device
    batch = ["ragged", "blocks", "vec", "zpad", "one", "f64", "nan"]
    for k in batch:
        others = [b for b in batch if b != k]
        target = dev(VOLS[k])
        labs = [dev(l) for l in LABELS.get(k, [])]
        alone_i, alone_l, alone_s = preprocess_batch_device([target], [labs])
        for at in (0, 6):
            names = [k] + others if at == 0 else others + [k]
            assert len(names) == 7 and names[at] == k
            vols = [target if j == at else dev(VOLS[n]) for j, n in enumerate(names)]
            ll = [labs if j == at else [dev(l) for l in LABELS.get(n, [])] for j, n in enumerate(names)]
            imgs, lbs, st = preprocess_batch_device(vols, ll)
            assert torch.equal(bits(st[at]), bits(alone_s[0])), (k, at)
            assert torch.equal(bits(imgs[at]), bits(alone_i[0])), (k, at)
            assert len(lbs[at]) == len(alone_l[0])
            for a, b in zip(lbs[at], alone_l[0]):
                assert torch.equal(bits(a), bits(b)), (k, at)
            assert torch.equal(bits(volume_stats_device(vols)[at]), bits(alone_s[0])), (k, at)


def test_unaligned_views_take_the_element_path_with_the_same_bits():
    """a volume that starts off a 16-byte boundary (a view into a larger buffer) and a dst behind it: same bits"""
    from values_amd.preprocess import preprocess_batch_device, volume_stats_device
    x = VOLS["blocks"]
    base = torch.zeros(x.size + 8, dtype=torch.int16, device="cuda")
    base[3:3 + x.size] = dev(x).reshape(-1)
    view = base[3:3 + x.size].view(x.shape)
    assert view.data_ptr() % 16 != 0
    assert torch.equal(bits(volume_stats_device([view])), bits(volume_stats_device([dev(x)])))
    a, b = preprocess_batch_device([view], out_dtype=torch.float32)[0][0], preprocess_batch_device([dev(x)], out_dtype=torch.float32)[0][0]
    assert torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """a raw tree and both preprocessed trees: (cases, host directory, device directory, lidc)"""
    from values_amd import preprocess_dataset
    out = []
    for lidc in (False, True):
        d = tmp_path_factory.mktemp("prep_lidc" if lidc else "prep_toy")
        root = str(d / "raw")
        cases = write_tree(root, lidc)
        kw = dict(image_dirs=["imagesTr"], label_dirs=["labelsTr"], dataset="lidc" if lidc else None, patch_size=16, patch_overlap=0.5)
        preprocess_dataset(root, str(d / "host"), 2, device_io=False, **kw)
        preprocess_dataset(root, str(d / "dev"), 2, device_io=True, batch=2, **kw)
        out.append((cases, root, str(d / "host" / "preprocessed"), str(d / "dev" / "preprocessed"), lidc))
    return out


def test_data_set_end_to_end_against_the_host_mirror(trees):
    from values_amd.preprocess import npy_header
    for cases, root, host, devd, lidc in trees:
        for sub in ("imagesTr", "labelsTr"):
            assert sorted(os.listdir(os.path.join(host, sub))) == sorted(os.listdir(os.path.join(devd, sub)))
        assert len(os.listdir(os.path.join(devd, "labelsTr"))) == 5 and len(os.listdir(os.path.join(devd, "imagesTr"))) == 3
        for name in os.listdir(os.path.join(host, "labelsTr")):      # labels: byte-identical files
            assert name.endswith("_mask.npy") == lidc
            assert open(os.path.join(host, "labelsTr", name), "rb").read() == open(os.path.join(devd, "labelsTr", name), "rb").read(), name
        for cid, (image, _) in cases.items():
            v = np.load(os.path.join(host, "imagesTr", cid + ".npy"))
            path = os.path.join(devd, "imagesTr", cid + ".npy")
            g = np.load(path)
            assert g.dtype == v.dtype and g.shape == v.shape and g.flags.c_contiguous, cid
            head = npy_header(g.shape, g.dtype)
            assert open(path, "rb").read(len(head)) == head
            n = image.size
            if image.dtype == np.float32:
                # numpy accumulates float32 statistics in float32: the yardstick is the mirror's own distance from the
                # float64 computation rounded to float32
                x = image.astype(np.float64)
                z = (x - x.mean()) / (x.std() + 1e-8)
                diff = [a - b for a, b in zip(v.shape, x.shape)]
                z = np.pad(z, [(d // 2, d // 2 + d % 2) for d in diff], "constant", constant_values=z.min()).astype(np.float32)
                gap = float(np.abs(v.astype(np.float64) - z).max())
                bound = np.maximum(np.spacing(np.abs(v)).astype(np.float64), 2 * gap)
                d = np.abs(g.astype(np.float64) - v)
                print(f"{cid} float32: mirror's gap to the float64 computation {gap:.3e}, device vs mirror {d.max():.3e}")
                assert (d <= bound).all(), (cid, d.max(), gap)
            else:
                d = np.abs(g - v)
                bound = 4 * n * EPS * (1 + np.abs(v))
                print(f"{cid} {image.dtype}: device vs mirror max |d| / (n eps (1 + |v|)) = {(d / (bound / 4)).max():.3e} (contract 4)")
                assert (d <= bound).all(), (cid, d.max())


def test_load_cases_device_equals_the_npy_route(trees):
    from values_amd import load_cases_device
    cases, root, host, devd, lidc = trees[0]
    ids = sorted(cases)
    got = load_cases_device([os.path.join(root, "imagesTr", c + ".nii.gz") for c in ids], patch_size=16, patch_overlap=0.5, batch=2)
    assert len(got) == 3
    for c, t in zip(ids, got):
        want = torch.from_numpy(np.load(os.path.join(devd, "imagesTr", c + ".npy")).astype(np.float32))
        assert t.is_cuda and t.dtype == torch.float32 and torch.equal(t.cpu(), want), c


def test_predict_image_sliding_takes_the_device_volume(tmp_path):
    """one 64^3 case: raw NIfTI -> load_cases_device -> predict_image_sliding gives the maps of the .npy route"""
    from tests.formula import formula_volume
    from tests.test_gpu_unet3d import make_model
    from values_amd import load_cases_device, nifti, predict_image_sliding, preprocess_dataset
    root = tmp_path / "raw"
    os.makedirs(root / "images")
    os.makedirs(root / "labels")
    raw = (formula_volume((64, 64, 64), tag=23) * 400 + 100).astype(np.int16)
    nifti.save(raw, str(root / "images" / "c0.nii.gz"))
    preprocess_dataset(root, tmp_path, 1, device_io=True)
    stored = np.load(tmp_path / "preprocessed" / "images" / "c0.npy")
    assert stored.shape == (64, 64, 64) and stored.dtype == np.float64
    vol = load_cases_device([root / "images" / "c0.nii.gz"])[0]
    assert torch.equal(vol.cpu(), torch.from_numpy(stored.astype(np.float32)))
    model = make_model(seed_tag=0, do_dropout=False)
    a = predict_image_sliding([model], vol, n_pred=1)
    b = predict_image_sliding([model], torch.from_numpy(stored), n_pred=1)
    for k in ("softmax_sum", "pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty", "mean_softmax", "pred_seg_mean"):
        assert torch.equal(a[k], b[k]), k


def test_reader_yields_what_one_call_per_batch_yields(trees):
    from values_amd import nifti
    from values_amd.preprocess import PreprocessReader, preprocess_batch_device
    d = os.path.dirname(trees[0][1])
    root = os.path.join(d, "six")
    os.makedirs(root)
    batches, k = [], 0
    for b in range(3):
        batch = []
        for c in range(2):
            shape, dt = [((10, 9, 21), "int16"), ((4, 30, 5), "float32"), ((16, 16, 16), "uint8")][(k + c) % 3]
            ip = os.path.join(root, f"v{k}.nii.gz")
            nifti.save(volume(shape, dt, 60 + k), ip)
            lps = []
            for r in range(k % 3):
                lps.append(os.path.join(root, f"v{k}_{r:02d}.nii.gz"))
                nifti.save((volume(shape, "int16", 80 + 3 * k + r) > 0).astype(np.uint8), lps[-1])
            batch.append((ip, lps))
            k += 1
        batches.append(batch)
    with PreprocessReader(patch_size=16, patch_overlap=0.5) as reader:
        got = [[(img.clone(), [l.clone() for l in labs], row.clone(), head) for img, labs, row, head in res] for res in reader.read(batches)]
    assert [len(g) for g in got] == [2, 2, 2]
    for batch, res in zip(batches, got):
        loaded = nifti.load_device([ip for ip, _ in batch])
        labs = [[t for t, _ in nifti.load_device(lps)] for _, lps in batch]
        imgs, lbs, st = preprocess_batch_device([t for t, _ in loaded], labs, patch_size=16, patch_overlap=0.5)
        for i, (img, ll, row, head) in enumerate(res):
            assert torch.equal(bits(img), bits(imgs[i])) and torch.equal(bits(row), bits(st[i]))
            assert len(ll) == len(lbs[i]) and all(torch.equal(a, b) for a, b in zip(ll, lbs[i]))
            assert head["datatype"] == loaded[i][1]["datatype"]
