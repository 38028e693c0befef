"""Builders shared by tests/test_preprocess2d_cpu.py and tests/test_gpu_preprocess2d.py: palette PNG files with a chosen
filter per row and a chosen palette length, and two tiny raw data-set trees -- one in the Cityscapes layout, one in the
GTA5 layout -- with every case the skip rules name.  The sources are 13 x 22 and 9 x 17 pixels: with crop (8, 16) the crop
box starts at odd offsets (2, 3) and at (0, 0)."""
import os
import struct
import zlib

import numpy as np

from tests import png_build
from values_amd import gta
from values_amd.image_io import write_png

CROP, FACTOR = (8, 16), 4
SIZES = ((13, 22), (9, 17))
COLOURS = np.array(list(gta.COLOR2TRAINID), dtype=np.uint8)          # every colour color2trainId knows


def indexed_png_bytes(idx, palette, ft, n_idat=1):
    """a colour-type-3 PNG of the (H, W) uint8 index image idx with the (n <= 256, 3) palette; row y has filter ft[y]"""
    h, w = idx.shape
    z = zlib.compress(png_build.scanlines(idx[..., None], np.asarray(ft, np.uint8)), 6)
    cuts = [len(z) * k // n_idat for k in range(n_idat + 1)]
    out = b"\x89PNG\r\n\x1a\n" + png_build._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 3, 0, 0, 0))
    out += png_build._chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    for k in range(n_idat):
        out += png_build._chunk(b"IDAT", z[cuts[k]:cuts[k + 1]])
    return out + png_build._chunk(b"IEND", b"")


def rgb_image(h, w, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[0, :] = 255      # both ends of the range in the rounding
    a[-1, :] = 0
    return a


def label_ids(h, w, seed):
    """grey label ids: every id of the table, ids beyond it (they keep their value), 255"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array(list(range(0, 39)) + [40, 100, 200, 255], dtype=np.uint8), (h, w))


def label_colours(h, w, seed):
    """-> (index image, the colour image) over COLOURS"""
    idx = np.random.default_rng(seed).integers(0, len(COLOURS), (h, w)).astype(np.uint8)
    return idx, COLOURS[idx]


def _write(path, data):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def _png(path, a):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    write_png(path, a)


def cityscapes_tree(root):
    """-> {image_id: (image, label ids)} of the cases that are to be preprocessed.  Also in the tree: a case whose label
    has another resolution ("aachen_000009_000019"), a mac "._" file, a file that is no PNG, a city that is a plain file."""
    root = str(root)
    im = lambda split, city, i: os.path.join(root, "images", "leftImg8bit", split, city, f"{i}_leftImg8bit.png")
    lb = lambda split, city, i: os.path.join(root, "labels", "gtFine", split, city, f"{i}_gtFine_labelIds.png")
    cases = {}
    for k, (split, city, i, (h, w)) in enumerate((("train", "aachen", "aachen_000000_000019", SIZES[0]),
                                                  ("train", "zurich", "zurich_000001_000019", SIZES[1]),
                                                  ("val", "bonn", "bonn_000002_000019", SIZES[0]))):
        image, ids = rgb_image(h, w, 10 + k), label_ids(h, w, 20 + k)
        if k == 1:      # an RGBA image: the alpha channel is dropped
            rgba = np.concatenate([image, np.full((h, w, 1), 77, np.uint8)], -1)
            _write(im(split, city, i), png_build.png_bytes(rgba, png_build.filters("cyclic", h)))
        else:
            _png(im(split, city, i), image)
        _png(lb(split, city, i), ids)
        cases[i] = (image, ids)
    _png(im("train", "aachen", "aachen_000009_000019"), rgb_image(*SIZES[0], 31))
    _png(lb("train", "aachen", "aachen_000009_000019"), label_ids(*SIZES[1], 32))
    _write(im("train", "aachen", "._aachen_000000_000019"), b"mac")
    _write(os.path.join(root, "images", "leftImg8bit", "train", "aachen", "notes.txt"), b"no png")
    _write(os.path.join(root, "images", "leftImg8bit", "train", "README"), b"a file among the cities")
    return cases


def gta_tree(root, unknown=False):
    """-> {image_id: (image, label colour image)}.  00001: an RGB label file; 00002: a palette label file with a short
    palette, every filter; 00004: an RGBA label file.  Also: 15188.png and 17705.png (never read: their label files do
    not exist), 00003 with a label of another resolution.  unknown: one pixel of 00001's label, inside the crop and on the
    nearest grid, gets a colour color2trainId does not know."""
    root = str(root)
    im = lambda i: os.path.join(root, "images", f"{i}.png")
    lb = lambda i: os.path.join(root, "labels", f"{i}.png")
    cases = {}
    for k, (i, (h, w)) in enumerate((("00001", SIZES[0]), ("00002", SIZES[1]), ("00004", SIZES[0]))):
        image = rgb_image(h, w, 40 + k)
        idx, colour = label_colours(h, w, 50 + k)
        _png(im(i), image)
        if k == 0:
            if unknown:
                colour = colour.copy()
                colour[2 + 4, 3 + 8] = (1, 2, 3)
            _png(lb(i), colour)
        elif k == 1:
            _write(lb(i), indexed_png_bytes(idx, COLOURS, png_build.filters("cyclic", h), n_idat=2))
        else:
            rgba = np.concatenate([colour, np.full((h, w, 1), 255, np.uint8)], -1)
            _write(lb(i), png_build.png_bytes(rgba, png_build.filters("paeth", h)))
        cases[i] = (image, colour)
    for i in ("15188", "17705"):
        _png(im(i), rgb_image(*SIZES[0], 60))
    _png(im("00003"), rgb_image(*SIZES[0], 61))
    _png(lb("00003"), label_colours(*SIZES[1], 62)[1])
    return cases
