"""Numpy restatements the toy data tests hold the product to (values_amd/toydata.py, toydata.hip): scipy's symmetric
correlate1d as gaussian_filter drives it, the `reflect` index, the two hash words of the library's generator
(values_amd/csrc/gauss.h) and the two embed functions.  Written independently of the product: loops over
output positions and taps where the product uses slices."""
import numpy as np


def reflect_index(i, n):
    """d c b a | a b c d | d c b a: period 2n, the second half mirrored"""
    i = int(i) % (2 * n)
    return i if i < n else 2 * n - 1 - i


def gaussian_weights(sigma, truncate=4.0):
    sd = float(sigma)
    radius = int(truncate * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    phi = phi / phi.sum()
    return phi[::-1].copy(), radius


def blur_axis(a, w, radius, axis):
    """one pass: for every line along `axis`, tmp = x[l] * w[c]; for j = -radius .. -1: tmp += (x[l + j] + x[l - j]) * w[c + j]"""
    a = np.moveaxis(np.asarray(a, dtype=np.float64), axis, -1)
    n = a.shape[-1]
    idx = np.array([reflect_index(e, n) for e in range(-radius, n + radius)])
    ext = a[..., idx]
    out = np.empty_like(a)
    for l in range(n):
        tmp = ext[..., l + radius] * w[radius]
        for j in range(-radius, 0):
            tmp = tmp + (ext[..., l + radius + j] + ext[..., l + radius - j]) * w[radius + j]
        out[..., l] = tmp
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))


def gaussian_blur(a, sigma):
    w, radius = gaussian_weights(sigma)
    out = np.asarray(a, dtype=np.float64)
    for axis in range(out.ndim):
        out = blur_axis(out, w, radius, axis)
    return out


def sparse_volume(shape, seed):
    """mostly zero, some values in (0, 1): what a placed object looks like to the filter"""
    rng = np.random.default_rng(seed)
    a = rng.random(shape)
    a[rng.random(shape) < 0.7] = 0.0
    return a


def _mix32(h):
    h = h.astype(np.uint64)
    M = np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7feb352d)) & M
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846ca68b)) & M
    h ^= h >> np.uint64(16)
    return h


def hash_words(seed, stream, n):
    """(h1, h2) of elements 0 .. n - 1 of stream `stream` of `seed` (gauss.h)"""
    M = np.uint64(0xFFFFFFFF)
    a = np.arange(n, dtype=np.uint64)
    key = _mix32(np.array([(int(seed) ^ ((int(stream) * 0x85EBCA6B + 0x165667B1) & 0xFFFFFFFF)) & 0xFFFFFFFF], dtype=np.uint64))[0]
    h1 = _mix32(((a * np.uint64(0x9E3779B1)) & M) ^ key)
    h2 = _mix32(h1 ^ np.uint64(0x27D4EB2F) ^ ((a * np.uint64(0xC2B2AE35)) & M))
    return h1, h2


def add_noise(image, seed, stream, noise_prob=0.5):
    """where image < 0.1: (u_p <= noise_prob) ? 0 : u_n, u = (h >> 8) * 2^-24"""
    flat = np.array(image, dtype=np.float64).reshape(-1)
    h1, h2 = hash_words(seed, stream, flat.size)
    up = (h1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    un = (h2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    noise = np.where(up <= noise_prob, 0.0, un)
    return np.where(flat < 0.1, noise, flat).reshape(np.shape(image))


def embed_positive(start, obj, image_size):
    """the object's box written at `start` of a zero float64 image (a box that does not fit raises, as numpy does)"""
    image = np.zeros(image_size)
    box = tuple(slice(start[a], start[a] + obj.shape[a]) for a in range(3))
    image[box] = obj
    return image


def embed_negative(start, obj, image_size):
    """an offset <= 0 on an axis cuts |offset| leading object voxels and starts at image voxel 0; a positive one places
    the whole extent at the offset"""
    image = np.zeros(image_size)
    dst = tuple(slice(max(start[a], 0), start[a] + obj.shape[a]) for a in range(3))
    src = tuple(slice(0 if start[a] > 0 else abs(start[a]), None) for a in range(3))
    image[dst] = obj[src]
    return image
