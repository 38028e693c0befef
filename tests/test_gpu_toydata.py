"""GPU: the toy data set generator on the device (values_amd/toydata.py over toydata.hip).  Everything is held to `==`:
the blur to the numpy restatement of scipy's order of operations (tests/toy_ref.py, itself bit-equal to
scipy.ndimage.gaussian_filter: tests/test_toydata_cpu.py), the embed to the host mirror, the order statistics to
np.partition, the thresholds to np.quantile of the downloaded image, the segmentations to np.where, the noise to the
restated generator, the device tree to the host mirror's.

Blur shapes: the four the restatement is pinned to scipy on; (70, 65, 130) sigma 8 -- every tile edge crossed, a partial
last wave, five ring steps of the 64-column slab on axes 0 and 1 and a last step of 6 (axis 0) and 1 (axis 1) rows, so a
thread that stores one of its two rows; (3, 3, 3) sigma 8 -- many reflections per tap; (1, 1, 257) -- one row, three
segments, odd extent; (70, 18, 40) sigma 16 -- radius 64, the 32-column slab, three ring steps; (130, 6, 20) sigma 32 --
radius 128, the 16-column slab, three ring steps; even extents behind a pointer 8 bytes off 16 -- the 8-byte path where the 16-byte one would otherwise
run."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import toy_ref

pytestmark = pytest.mark.gpu

BLUR_CASES = [((5, 7, 3), 2), ((40, 33, 17), 8), ((9, 70, 12), 8), ((1, 2, 66), 3), ((70, 65, 130), 8), ((3, 3, 3), 8),
              ((1, 1, 257), 3), ((70, 18, 40), 16), ((130, 6, 20), 32)]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # a copy: the shared references are read-only


@functools.lru_cache(maxsize=None)
def blur_reference(shape, sigma):
    """-> (input, [axis 0 alone, axis 1 alone, axis 2 alone], the three in turn), computed once"""
    a = toy_ref.sparse_volume(shape, 11)
    w, r = toy_ref.gaussian_weights(sigma)
    alone = [toy_ref.blur_axis(a, w, r, ax) for ax in range(3)]
    chain = toy_ref.blur_axis(toy_ref.blur_axis(alone[0], w, r, 1), w, r, 2)
    for v in alone + [chain]:
        v.setflags(write=False)
    return a, alone, chain


@pytest.mark.parametrize("shape,sigma", BLUR_CASES)
def test_blur_equals_the_restatement(shape, sigma):
    from values_amd import toydata
    a, alone, chain = blur_reference(shape, sigma)
    w, r = toydata.gaussian_weights(sigma)
    x, wd = dev(a), dev(w)
    for ax in range(3):
        got = toydata.blur_axis_device(x, ax, wd, r).cpu().numpy()
        assert np.array_equal(got, alone[ax]), (shape, sigma, ax, float(np.abs(got - alone[ax]).max()))
    got = toydata.gaussian_blur_device(x, sigma).cpu().numpy()
    assert np.array_equal(got, chain), float(np.abs(got - chain).max())
    assert np.array_equal(x.cpu().numpy(), a)          # the source is left alone


def test_blur_8_byte_path_on_even_extents():
    from values_amd import toydata
    a, alone, _ = blur_reference((6, 10, 12), 2)
    w, r = toydata.gaussian_weights(2)
    wd = dev(w)
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    x = buf[1:].view(a.shape)                           # 8 bytes off a 16-byte boundary
    x.copy_(dev(a))
    assert x.data_ptr() % 16 == 8 and x.is_contiguous()
    for ax in range(3):
        assert np.array_equal(toydata.blur_axis_device(x, ax, wd, r).cpu().numpy(), alone[ax]), ax
    obuf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    out = obuf[1:].view(a.shape)
    for ax in range(3):
        toydata.blur_axis_device(dev(a), ax, wd, r, out=out)
        assert np.array_equal(out.cpu().numpy(), alone[ax]), ax


def test_blur_refuses_in_place():
    from values_amd import _lib, toydata
    x = torch.zeros((4, 4, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.VxError):
        toydata.blur_axis_device(x, 0, dev(np.ones(3) / 3), 1, out=x)


def test_embed_equals_the_mirror():
    from values_amd import toydata
    rng = np.random.default_rng(5)
    obj = (rng.random((9, 7, 11)) > 0.3).astype(np.float32) * rng.random((9, 7, 11)).astype(np.float32)
    size = (20, 16, 24)
    base = {"object": obj, "image_size": size, "negative": False, "fliplr": False, "flipud": False, "gray": None}
    items = [dict(base, offset=[3, 9, 13]), dict(base, offset=[11, 0, 0], gray=0.61)]
    for off in ([-6, -4, -7], [-6, 2, 0], [4, -1, 13]):     # the first clips on all three axes
        for lr in (False, True):
            for ud in (False, True):
                items.append(dict(base, offset=off, negative=True, fliplr=lr, flipud=ud, gray=0.7 if lr else None))
    for it in items:
        want = toydata.embed(it)
        got = toydata.embed_device(it).cpu().numpy()
        assert got.dtype == np.float64 and np.array_equal(got, want), (it["offset"], it["fliplr"], it["flipud"])
        assert not np.signbit(got).any()
    # the kernel clips on the high side too and takes an object that lies wholly outside
    got = toydata.embed_device(dict(base, offset=[15, 12, 20])).cpu().numpy()
    want = np.zeros(size)
    want[15:, 12:, 20:] = obj[:5, :4, :4]
    assert np.array_equal(got, want)
    assert not toydata.embed_device(dict(base, offset=[-9, 0, 0])).any()


def tied_values():
    rng = np.random.default_rng(9)
    x = np.round(rng.standard_normal(100003), 3)       # heavy ties, negatives
    x[:2000] = 0.0
    x[2000:2500] = -0.0
    x[2500:2510] = np.inf
    x[2510:2517] = -np.inf
    return rng.permutation(x)


def test_order_stats_equal_np_partition():
    from values_amd import _lib, toydata
    x = tied_values()
    n = x.size
    rng = np.random.default_rng(10)
    ks = [0, n - 1, n - 2] + [int(k) for k in rng.integers(0, n, 13)]
    both = sorted(set(ks) | {min(k + 1, n - 1) for k in ks})
    part = np.partition(x, both)
    out, status, reads = toydata.order_stats_device(dev(x), ks)
    out = out.cpu().numpy()
    assert int(status.cpu()[0]) == _lib.VX_SELECT_OK
    for i, k in enumerate(ks):
        assert out[i, 0] == part[k] and out[i, 1] == part[min(k + 1, n - 1)], (i, k, out[i], part[k])
    assert out[1, 0] == out[1, 1] == np.inf and out[0, 0] == -np.inf
    assert reads == 8 * -(-len(both) // 16)
    print(f"order statistics: {len(ks)} ranks, {len(both)} distinct among (k, k + 1), {reads} reads of the data")
    # n = 1, and a NaN
    out, status, _ = toydata.order_stats_device(dev(np.array([-2.5])), [0])
    assert out.cpu().numpy().tolist() == [[-2.5, -2.5]] and int(status.cpu()[0]) == _lib.VX_SELECT_OK
    y = x.copy()
    y[777] = np.nan
    _, status, _ = toydata.order_stats_device(dev(y), [5, 100])
    assert int(status.cpu()[0]) == _lib.VX_SELECT_NAN


@functools.lru_cache(maxsize=None)
def blurred_object():
    """a blurred sphere on the device and its download"""
    from values_amd import toydata
    item = toydata.plan_samples(toydata.sphere_object, 1, (40, 36, 44), object_gray=True, seed=3)[0]
    image = toydata.gaussian_blur_device(toydata.embed_device(item), 3)
    host = image.cpu().numpy()
    host.setflags(write=False)
    return image, host


@pytest.mark.parametrize("n_raters", [3, 5])
def test_thresholds_equal_np_quantile_and_segmentations_np_where(n_raters):
    from values_amd import toydata
    image, host = blurred_object()
    assert int(toydata.count_ge_device(image, 0.1).cpu()[0]) == np.count_nonzero(host >= 0.1) > 0
    want = toydata.rater_thresholds(host, n_raters)
    got = toydata.rater_thresholds_device(image, n_raters)
    assert len(got) == len(want) and np.array_equal(got, want), (got, want)
    segs = toydata.segment_device(image, got).cpu().numpy()
    assert segs.dtype == np.int32 and segs.shape == (len(want),) + host.shape
    for r, t in enumerate(want):
        assert np.array_equal(segs[r], np.where(host >= t, 1, 0))
    assert toydata.rater_thresholds_device(image, 1) == [0.1] and toydata.rater_thresholds_device(image, 4, True) == [0.1] * 4
    # the 4-byte store path: an element count that is no multiple of 4
    flat = image.reshape(-1)[:1001]
    s = toydata.segment_device(flat, [0.1, 0.3]).cpu().numpy()
    assert np.array_equal(s, np.stack([np.where(host.reshape(-1)[:1001] >= t, 1, 0) for t in (0.1, 0.3)]))


def test_noise_equals_the_restated_generator():
    from values_amd import toydata
    _, host = blurred_object()
    for seed, stream in ((22, 0), (22, 3), (0xFFFFFFFF, 70000)):
        got = toydata.add_noise_device(dev(host), seed, stream).cpu().numpy()
        assert np.array_equal(got, toy_ref.add_noise(host, seed, stream)), (seed, stream)
        keep = host >= 0.1
        assert keep.any() and np.array_equal(got[keep], host[keep])
    a = toydata.add_noise_device(dev(host), 22, 0).cpu().numpy()
    b = toydata.add_noise_device(dev(host), 22, 1).cpu().numpy()
    assert not np.array_equal(a, b)
    nan = host.copy()
    nan[0, 0, 0] = np.nan
    assert np.isnan(toydata.add_noise_device(dev(nan), 22, 0).cpu().numpy()[0, 0, 0])


def test_noise_statistics_on_a_background_volume():
    from values_amd import toydata
    out = toydata.add_noise_device(torch.zeros((64, 64, 64), dtype=torch.float64, device="cuda"), 22, 0, 0.5).cpu().numpy()
    n = out.size
    zero = float((out == 0).mean())
    assert abs(zero - 0.5) <= 5 * np.sqrt(0.25 / n), zero
    nz = out[out != 0]
    assert nz.min() > 0 and nz.max() < 1
    assert abs(nz.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / nz.size), float(nz.mean())
    out3 = toydata.add_noise_device(torch.zeros((64, 64, 64), dtype=torch.float64, device="cuda"), 22, 0, 0.25).cpu().numpy()
    assert abs(float((out3 == 0).mean()) - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / n)


def test_a_sample_is_the_same_alone_or_as_sample_3_of_5(tmp_path):
    from values_amd import generate_toy_dataset, nifti, toydata
    save = str(tmp_path / "five")
    kw = dict(n_samples=5, image_size=(24, 20, 28), gauss_sigma=2, object_gray=True, blur=True, noise=True, seed=9)
    generate_toy_dataset(save, toydata.box_object, device_io=True, **kw)
    item = toydata.plan_samples(toydata.box_object, 5, (24, 20, 28), object_gray=True, seed=9)[3]
    alone = toydata.add_noise_device(toydata.gaussian_blur_device(toydata.embed_device(item), 2), 9, 3).cpu().numpy()
    got, _ = nifti.load(os.path.join(save, "0003.nii.gz"))
    assert np.array_equal(got, alone.transpose(2, 1, 0))
    assert np.array_equal(alone, toy_ref.add_noise(toydata.gaussian_blur(toydata.embed(item), 2), 9, 3))


# ---------------------------------------------------------------------------------------------
# end to end

def tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(dirpath, f), root)] = os.path.join(dirpath, f)
    return out


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """{noise: (host tree, device tree)}; both trees of a pair are generated into the SAME save_path (the host one is moved
    away first), so the dataset_info files can be compared byte for byte"""
    from values_amd import generate_toy_dataset
    from values_amd.toydata import sphere_object
    root = tmp_path_factory.mktemp("toy")
    out = {}
    for noise in (False, True):
        kw = dict(n_samples=3, image_size=(48, 48, 48), gauss_sigma=3, object_gray=True, blur=True, noise=noise, segmentation=True,
                  n_raters=3, object_over_border=noise, seed=22)
        save = str(root / f"set{int(noise)}")
        generate_toy_dataset(save, sphere_object, device_io=False, **kw)
        host = str(root / f"host{int(noise)}")
        os.rename(save, host)
        generate_toy_dataset(save, sphere_object, device_io=True, **kw)
        out[noise] = (host, save)
    return out


def test_device_tree_equals_the_host_mirror(trees):
    from values_amd import nifti
    host, device = trees[False]
    th, td = tree(host), tree(device)
    assert sorted(th) == sorted(td) and len(th) >= 3 + 3 * 3 + 1
    for rel in sorted(th):
        if rel.endswith(".json"):
            assert open(th[rel], "rb").read() == open(td[rel], "rb").read()
            assert json.load(open(td[rel]))["n_raters"] == 3
            continue
        a, _ = nifti.load(th[rel])
        b, _ = nifti.load(td[rel])
        assert a.dtype == b.dtype == (np.int32 if "segmentation" in rel else np.float64) and a.shape == b.shape == (48, 48, 48)
        assert np.array_equal(a, b), rel
        assert a.any()


def test_device_tree_with_noise_keeps_the_object_and_the_segmentations(trees):
    from values_amd import nifti
    from values_amd.toydata import embed, gaussian_blur, plan_samples, sphere_object
    host, device = trees[True]
    th, td = tree(host), tree(device)
    assert sorted(th) == sorted(td)
    plan = plan_samples(sphere_object, 3, (48, 48, 48), object_over_border=True, object_gray=True, seed=22)
    for rel in sorted(th):
        if rel.endswith(".json"):
            assert open(th[rel], "rb").read() == open(td[rel], "rb").read()
            continue
        a, _ = nifti.load(th[rel])
        b, _ = nifti.load(td[rel])
        if "segmentation" in rel:
            assert np.array_equal(a, b), rel
            continue
        clean = gaussian_blur(embed(plan[int(rel[:4])]), 3).transpose(2, 1, 0)
        keep = clean >= 0.1
        assert keep.any() and np.array_equal(a[keep], clean[keep]) and np.array_equal(b[keep], clean[keep])
        assert np.array_equal(b, toy_ref.add_noise(clean.transpose(2, 1, 0), 22, int(rel[:4])).transpose(2, 1, 0))
        assert not np.array_equal(a[~keep], b[~keep])      # numpy's stream on the host, the library's generator here
