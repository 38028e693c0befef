"""The generator of the toy 3D data sets (the reference's datasets/toy_data_generation/dataset_generation.py:144-254 with
the helpers of stl_to_nifty.py:93-155): an object is placed in an empty volume, optionally grayed, blurred with a
Gaussian, thresholded into one segmentation per rater at quantiles of the blurred image, and its background is filled
with noise.  Every C1 / C2 configuration, the benchmark shapes and is_ood_toy are defined on these data sets.

Two routes to the same tree.  The host mirror (device_io=False) is the reference's numpy expressions line for line; its
blur restates scipy.ndimage.gaussian_filter operation by operation (no scipy in the product) and is slow by
construction.  The device route (device_io=True) makes the same plan on the host and runs embed -> blur -> count ->
order statistics -> segmentations -> noise in float64 on the device (toydata.hip, DESIGN 4.49 ff.); the files go through
results.MapsWriter, so sample i is written while sample i + 1 is computed.

Pinned: the blur to scipy.ndimage.gaussian_filter bit for bit; the placements, flips and gray values to the reference's
calls on Python's `random` for the same seed and object shapes; the thresholds to np.quantile in float64.
The object of a sample comes from `object_fn(resolution)`: stl.mesh_object(input_files) voxelises the reference's STL
meshes (meshes_to_numpy) under this project's own rule, on the host or, with device_io, on the device, where the
volume stays as a tensor from the voxeliser to the embed (stl.py, voxelize.hip);
stl.generate_toy_dataset_from_config runs one of the reference's JSON configs.  sphere_object / box_object are
mesh-free stand-ins.
Not pinned: parity of the voxeliser with stl-to-voxel 0.9.1 (numpy-stl and stltovoxel are absent; that package paints
the perimeter of each slice, so its surface voxels are fatter and its shape may differ by one), SimpleITK's header bytes (the files are nifti.save's), and, on the device route, numpy's noise stream: the noise is
drawn by this library's generator from (seed, sample index, voxel), so a data set generated here has other noise values
than the reference's for the same seed -- the same distribution, not the same numbers.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import random

import numpy as np

from . import _lib, nifti
from .thresholds import _lerp


# ---------------------------------------------------------------------------------------------
# objects (mesh-free stand-ins for meshes_to_numpy: float32 occupancy volumes of about `resolution` voxels per axis)

def _is_tensor(obj):
    return type(obj).__module__.split(".")[0] == "torch"


def sphere_object(resolution: int):
    r = int(resolution)
    c = (r - 1) / 2.0
    g = np.arange(r, dtype=np.float64) - c
    d2 = g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2
    return (d2 <= (r / 2.0) ** 2).astype(np.float32)


def box_object(resolution: int):
    r = int(resolution)
    return np.ones((r, max(1, (2 * r) // 3), max(1, r // 2)), dtype=np.float32)


# ---------------------------------------------------------------------------------------------
# the plan: every call on Python's `random`, in the reference's order (create_dataset_samples, :181-235)

def plan_samples(object_fn, n_samples, image_size, min_object_ratio=10, max_object_ratio=2, object_over_border=False,
                 object_gray=False, seed=22):
    """-> one dict per sample: object (float32 array, or the device tensor object_fn returned), offset, image_size, negative (which embed function), fliplr, flipud,
    gray (None: the object keeps its values).  Seeds Python's `random` as the reference's __main__ does."""
    image_size = (int(image_size),) * 3 if np.isscalar(image_size) else tuple(int(s) for s in image_size)
    if len(image_size) != 3:
        raise ValueError("Image size has to be exactly 1 or 3 values")
    random.seed(seed)
    plan = []
    for _ in range(n_samples):
        resolution = random.randint(int(max(image_size) / min_object_ratio), int(max(image_size) / max_object_ratio))
        obj = object_fn(resolution)
        obj = obj if _is_tensor(obj) else np.asarray(obj)   # a device tensor stays where it is: only its shape is used here
        max_offset = [image_size[a] - obj.shape[a] for a in range(3)]
        item = {"object": obj, "image_size": image_size, "negative": bool(object_over_border), "fliplr": False, "flipud": False,
                "gray": None}
        if not object_over_border:
            item["offset"] = [random.randint(0, max_offset[0]), random.randint(0, max_offset[1]), random.randint(0, max_offset[2])]
        else:
            min_offset = [int(-2 * obj.shape[a] / 3) for a in range(3)]
            binary_number = format(random.randint(1, 7), "b").zfill(3)
            item["offset"] = [random.randint(min_offset[a], 0) if int(binary_number[a]) else random.randint(0, max_offset[a])
                              for a in range(3)]
            item["fliplr"] = random.random() > 0.5
            item["flipud"] = random.random() > 0.5
        if object_gray:
            item["gray"] = random.uniform(0.5, 0.9)
        plan.append(item)
    return plan


def _embed_positive(start, obj, image_size):
    """embed_object_in_image (stl_to_nifty.py:93-102); where the reference prints and returns the object, this raises"""
    image = np.zeros(image_size)
    image[start[0]:start[0] + obj.shape[0], start[1]:start[1] + obj.shape[1], start[2]:start[2] + obj.shape[2]] = obj
    return image


def _embed_negative(start, obj, image_size):
    """embed_object_in_image_negative_offset (stl_to_nifty.py:127-142)"""
    image = np.zeros(image_size)
    s = [start[a] if start[a] > 0 else 0 for a in range(3)]
    o = [0 if start[a] > 0 else abs(start[a]) for a in range(3)]
    image[s[0]:start[0] + obj.shape[0], s[1]:start[1] + obj.shape[1], s[2]:start[2] + obj.shape[2]] = obj[o[0]:, o[1]:, o[2]:]
    return image


def embed(item):
    """The float64 image of one plan item before the blur: embed, flips, gray value (:196-235)."""
    fn = _embed_negative if item["negative"] else _embed_positive
    image = fn(item["offset"], item["object"], item["image_size"])
    if item["fliplr"]:
        image = np.fliplr(image)
    if item["flipud"]:
        image = np.flipud(image)
    if item["gray"] is not None:
        image = image * item["gray"]
    return image


# ---------------------------------------------------------------------------------------------
# the blur, in scipy's order of operations

def gaussian_weights(sigma, truncate: float = 4.0):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, radius) with radius = int(truncate * sigma + 0.5) -> (weights, radius)"""
    sd = float(sigma)
    radius = int(truncate * sd + 0.5)
    sigma2 = sd * sd
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    return phi_x[::-1].copy(), radius


def reflect_index(i, n):
    """scipy's `reflect` (d c b a | a b c d | d c b a) for any integer array i and n >= 1"""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _blur_axis(a, w, radius, axis):
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    ext = a[reflect_index(np.arange(-radius, n + radius), n)]
    out = ext[radius:radius + n] * w[radius]
    for i in range(radius, 0, -1):
        out = out + (ext[radius - i:radius - i + n] + ext[radius + i:radius + i + n]) * w[radius - i]
    return np.moveaxis(out, 0, axis)


def gaussian_blur(image, sigma, truncate: float = 4.0):
    """scipy.ndimage.gaussian_filter(image, sigma) (mode 'reflect') of a float64 array, bit for bit: axes in turn; per
    output the centre tap first, then the pairs from the farthest to the nearest as (x[-i] + x[+i]) * w[i], one float64
    rounding per operation."""
    out = np.ascontiguousarray(image, dtype=np.float64)
    if float(sigma) <= 1e-15:
        return out.copy()
    w, radius = gaussian_weights(sigma, truncate)
    for axis in range(out.ndim):
        out = _blur_axis(out, w, radius, axis)
    return np.ascontiguousarray(out)


# ---------------------------------------------------------------------------------------------
# raters, segmentations, noise (create_segmentations :144-166, add_noise stl_to_nifty.py:145-150)

def _perc_thresholds(n_raters):
    perc_range = 1 - 0.1
    perc_step = perc_range / (n_raters - 1)
    return np.arange(0.1, 1 + perc_step, perc_step)   # may hold n_raters + 1 elements: one more file, as in the reference


def rater_thresholds(image, n_raters, all_raters_same=False):
    if n_raters == 1:
        return [0.1]
    if all_raters_same:
        return [0.1] * n_raters
    perc_thresholds = _perc_thresholds(n_raters)
    all_object_pixels = np.count_nonzero(image >= 0.1)
    object_ratio = all_object_pixels / image.size
    perc_thresholds *= object_ratio
    return np.quantile(image, (1 - perc_thresholds))


def segment(image, thresholds):
    return [np.where(image >= threshold, 1, 0).astype(np.intc) for threshold in thresholds]


def add_noise(image, noise_prob=0.5):
    """numpy's global stream, as the reference draws it; changes `image` in place and returns it"""
    prob_array = np.random.rand(image.shape[0], image.shape[1], image.shape[2])
    noise_array = np.random.rand(image.shape[0], image.shape[1], image.shape[2])
    noise_array[prob_array <= noise_prob] = 0
    image[image < 0.1] = noise_array[image < 0.1]
    return image


# ---------------------------------------------------------------------------------------------
# the device route

def _dims(shape):
    return (C.c_int32 * 3)(*[int(s) for s in shape])


def embed_device(item, device=None):
    """embed(item) on the device -> float64 tensor [D0][D1][D2]"""
    import torch
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if _is_tensor(item["object"]):
        obj = item["object"].to(device=dev, dtype=torch.float32).contiguous()   # the voxeliser's tensor: no host round trip
    else:
        obj = torch.from_numpy(np.ascontiguousarray(item["object"], dtype=np.float32)).to(dev)
    image = torch.empty(tuple(item["image_size"]), dtype=torch.float64, device=dev)
    gray = 1.0 if item["gray"] is None else float(item["gray"])
    _lib.check(_lib.load().vx_toy_embed(_lib.ptr(obj), _dims(obj.shape), _dims(item["offset"]), gray, int(item["flipud"]),
                                        int(item["fliplr"]), _lib.ptr(image), _dims(image.shape), _lib.stream_ptr()), "vx_toy_embed")
    return image


def blur_axis_device(src, axis, weights, radius, out=None):
    """one pass of the filter along `axis` of a contiguous float64 device tensor [D0][D1][D2]; weights: device float64"""
    import torch
    if src.dim() != 3 or src.dtype != torch.float64 or not src.is_contiguous():
        raise ValueError("blur_axis_device: a contiguous float64 (D0, D1, D2) tensor")
    out = torch.empty_like(src) if out is None else out
    _lib.check(_lib.load().vx_gauss_blur_axis_f64(_lib.ptr(src), _lib.ptr(out), _dims(src.shape), axis, _lib.ptr(weights), radius,
                                                  _lib.stream_ptr()), "vx_gauss_blur_axis_f64")
    return out


def gaussian_blur_device(image, sigma, truncate: float = 4.0):
    """gaussian_blur on the device: three passes, two buffers"""
    import torch
    if float(sigma) <= 1e-15:
        return image.clone()
    w, radius = gaussian_weights(sigma, truncate)
    wd = torch.from_numpy(w).to(image.device)
    a = blur_axis_device(image, 0, wd, radius)
    b = blur_axis_device(a, 1, wd, radius)
    return blur_axis_device(b, 2, wd, radius, out=a)


def count_ge_device(x, thr):
    """-> int64 device tensor (1,): #{x >= thr}"""
    import torch
    count = torch.empty(1, dtype=torch.int64, device=x.device)
    _lib.check(_lib.load().vx_count_ge_f64(_lib.ptr(x), x.numel(), float(thr), _lib.ptr(count), _lib.stream_ptr()), "vx_count_ge_f64")
    return count


def order_stats_device(x, ks):
    """-> (float64 device tensor (len(ks), 2): the k-th and (k + 1)-th smallest of the dense float64 tensor x, int32
    device status (1,), reads of the data the call made)"""
    import torch
    lib = _lib.load()
    ks = [int(k) for k in ks]
    arr = (C.c_int64 * max(len(ks), 1))(*ks)
    out = torch.empty((len(ks), 2), dtype=torch.float64, device=x.device)
    status = torch.empty(1, dtype=torch.int32, device=x.device)
    ws = torch.empty(max(int(lib.vx_order_stats_f64_workspace_bytes(len(ks))), 256), dtype=torch.uint8, device=x.device)
    _lib.check(lib.vx_order_stats_f64(_lib.ptr(x), x.numel(), arr, len(ks), _lib.ptr(out), _lib.ptr(status), _lib.ptr(ws), ws.numel(),
                                      _lib.stream_ptr()), "vx_order_stats_f64")
    return out, status, int(lib.vx_order_stats_f64_reads(x.numel(), arr, len(ks)))


def rater_thresholds_device(image, n_raters, all_raters_same=False):
    """rater_thresholds of a device image: vx_count_ge_f64, one vx_order_stats_f64 call for all quantiles, two small
    downloads (the count, from which the ranks follow; then the order statistics with the status), numpy's linear
    interpolation on the host in float64."""
    import torch
    if n_raters == 1:
        return [0.1]
    if all_raters_same:
        return [0.1] * n_raters
    n = image.numel()
    perc_thresholds = _perc_thresholds(n_raters)
    object_ratio = int(count_ge_device(image, 0.1).cpu()[0]) / n
    perc_thresholds *= object_ratio
    qs = 1 - perc_thresholds
    virt = [float(q) * (n - 1) for q in qs]            # numpy: the virtual index of method "linear"
    lo = [min(max(int(np.floor(v)), 0), n - 1) for v in virt]
    out = []
    for c in range(0, len(lo), 32):
        stats, status, _ = order_stats_device(image, lo[c:c + 32])
        host = torch.cat([stats.reshape(-1), status.to(torch.float64)]).cpu().numpy()
        if int(host[-1]) == _lib.VX_SELECT_NAN:
            return np.full(len(qs), np.nan)
        out.extend(_lerp(host[2 * i], host[2 * i + 1], virt[c + i] - lo[c + i]) for i in range(len(lo[c:c + 32])))
    return np.asarray(out, dtype=np.float64)


def segment_device(image, thresholds):
    """-> int32 device tensor (R, D0, D1, D2)"""
    import torch
    thr = [float(t) for t in thresholds]
    out = torch.empty((len(thr),) + tuple(image.shape), dtype=torch.int32, device=image.device)
    _lib.check(_lib.load().vx_toy_segment(_lib.ptr(image), image.numel(), (C.c_double * len(thr))(*thr), len(thr), _lib.ptr(out),
                                          _lib.stream_ptr()), "vx_toy_segment")
    return out


def add_noise_device(image, seed, sample_index, noise_prob=0.5):
    """in place on a contiguous float64 device tensor: stream `sample_index` of `seed`"""
    _lib.check(_lib.load().vx_toy_noise(_lib.ptr(image), image.numel(), int(seed) & 0xFFFFFFFF, int(sample_index) & 0xFFFFFFFF,
                                        float(noise_prob), _lib.stream_ptr()), "vx_toy_noise")
    return image


# ---------------------------------------------------------------------------------------------
# the data set

def _info_path(save_path):
    """args_to_json's suffix search (:169-178): the first dataset_info_<k>.json that does not exist yet"""
    suffix = 1
    filename = os.path.join(save_path, f"dataset_info_{suffix}.json")
    while os.path.isfile(filename):
        suffix += 1
        filename = os.path.join(save_path, "dataset_info_{}.json".format(str(suffix)))
    return filename


def generate_toy_dataset(save_path, object_fn=sphere_object, n_samples=10, image_size=(256, 256, 256), min_object_ratio=10,
                         max_object_ratio=2, gauss_sigma=8, object_gray=False, blur=False, noise=False, segmentation=False,
                         all_raters_same=False, n_raters=1, object_over_border=False, sample_offset=0, seed=22, input_files=None,
                         device_io=False) -> None:
    """create_dataset_samples + args_to_json: save_path/NNNN.nii.gz (float64), save_path/segmentation/NNNN_RR.nii.gz (int32)
    and save_path/dataset_info_<k>.json with the reference's keys.  A numpy [a0, a1, a2] array is stored with a2 fastest,
    as SimpleITK stores it: nifti.load returns the transposed array.  device_io=False: the host mirror (noise from numpy's
    stream seeded with `seed`).  device_io=True: the device route (noise from this library's generator)."""
    save_path = str(save_path)
    image_size = (int(image_size),) * 3 if np.isscalar(image_size) else tuple(int(s) for s in image_size)
    info = {"json_config": None, "input_files": input_files, "save_path": save_path, "n_samples": n_samples,
            "image_size": list(image_size), "min_object_ratio": min_object_ratio, "max_object_ratio": max_object_ratio,
            "gauss_sigma": gauss_sigma, "object_gray": bool(object_gray), "blur": bool(blur), "noise": bool(noise),
            "segmentation": bool(segmentation), "all_raters_same": bool(all_raters_same), "n_raters": n_raters,
            "object_over_border": bool(object_over_border), "sample_offset": sample_offset, "seed": seed}
    plan = plan_samples(object_fn, n_samples, image_size, min_object_ratio, max_object_ratio, object_over_border, object_gray, seed)
    os.makedirs(save_path, exist_ok=True)
    if segmentation:
        os.makedirs(os.path.join(save_path, "segmentation"), exist_ok=True)
    name = lambda i: os.path.join(save_path, "{}.nii.gz".format(str(sample_offset + i).zfill(4)))
    seg_name = lambda i, r: os.path.join(save_path, "segmentation", "{}_{}.nii.gz".format(str(sample_offset + i).zfill(4), str(r).zfill(2)))
    if not device_io:
        np.random.seed(seed)
        for i, item in enumerate(plan):
            image = embed(item)
            if blur:
                image = gaussian_blur(image, gauss_sigma)
            if segmentation:
                for r, seg in enumerate(segment(image, rater_thresholds(image, n_raters, all_raters_same))):
                    nifti.save(seg.transpose(2, 1, 0), seg_name(i, r))
            if noise:
                image = add_noise(np.array(image), 0.5)
            nifti.save(image.transpose(2, 1, 0), name(i))
    else:
        from .results import MapsWriter
        _lib.require_gpu()
        with MapsWriter() as writer:
            for i, item in enumerate(plan):
                image = embed_device(item)
                if blur:
                    image = gaussian_blur_device(image, gauss_sigma)
                paths, tensors = [], []
                if segmentation:
                    segs = segment_device(image, rater_thresholds_device(image, n_raters, all_raters_same))
                    for r in range(segs.shape[0]):
                        paths.append(seg_name(i, r))
                        tensors.append(segs[r].permute(2, 1, 0))
                if noise:
                    add_noise_device(image, seed, sample_offset + i, 0.5)
                paths.append(name(i))
                tensors.append(image.permute(2, 1, 0))   # the [x, y, z] view whose reverse is contiguous: copied in order
                writer.submit(paths, tensors)
    with open(_info_path(save_path), "w") as f:
        json.dump(info, f, indent=2)
