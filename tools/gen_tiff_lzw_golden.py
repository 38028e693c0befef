"""Writes tests/golden/tiff_lzw: a handful of small float32 maps as LZW TIFF files written by libtiff (through PIL:
Image.save(compression="tiff_lzw", tiffinfo={317: predictor, 278: rows per strip})), each with its source array as
.npy -- predictors 1, 2 and 3, one, seven and all rows per strip, and a 40 x 300 map (upper half random, lower half
constant) that as one strip reaches all four code widths and several table resets.  The tests read these files and need
neither PIL nor libtiff on the machine they run on.

  python tools/gen_tiff_lzw_golden.py        (needs PIL built with libtiff)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from PIL import Image, features

    from tests import lzw_build as lb
    if not features.check("libtiff"):
        raise SystemExit("PIL without libtiff")
    os.makedirs(lb.GOLDEN_LZW, exist_ok=True)
    small, big = lb.smooth_map(21, 13), lb.half_random_map()
    cases = [("p1_rps1_21x13", small, 1, 1), ("p2_rps1_21x13", small, 2, 1), ("p3_rps1_21x13", small, 3, 1),
             ("p1_rps7_21x13", small, 1, 7), ("p2_rps7_21x13", small, 2, 7), ("p3_rps7_21x13", small, 3, 7),
             ("p2_whole_21x13", small, 2, 21), ("p1_whole_40x300", big, 1, 40), ("p3_whole_40x300", big, 3, 40)]
    total = 0
    for name, m, pred, rps in cases:
        tif, npy = os.path.join(lb.GOLDEN_LZW, name + ".tif"), os.path.join(lb.GOLDEN_LZW, name + ".npy")
        Image.fromarray(m).save(tif, compression="tiff_lzw", tiffinfo={317: pred, 278: rps})
        np.save(npy, m)
        back = np.array(Image.open(tif))
        assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), m.view(np.uint32)), name
        total += os.path.getsize(tif) + os.path.getsize(npy)
        print(name, os.path.getsize(tif), "bytes")
    print("total", total, "bytes")
    assert total < 200_000


if __name__ == "__main__":
    main()
