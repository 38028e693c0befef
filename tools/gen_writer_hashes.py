"""Writes tests/golden/writer_bytes.json: {relative path: sha256} of every file the device writers produce for the small
seeded inputs of tests/writer_trees.py -- save_case_device / ResultsWriter, save_maps_device / MapsWriter,
save_images_device / ResultsWriter2D (uncompressed and LZW TIFFs, predictors 1 to 3, default strips and 7 rows per
strip), gz.gzip_encode, results2d.png_encode and one vx_gzip_encode call whose members start at every residue mod 4.  The
encoders are deterministic, so the recorded bytes gate any change that is meant to leave the files as they are
(tests/test_gpu_writer_bytes.py).  Run it on the GPU at the commit whose bytes are to be kept:

  python tools/gen_writer_hashes.py
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import writer_trees as wt
    with tempfile.TemporaryDirectory(prefix="writer_hashes_") as root:
        hashes = wt.build(root)
        # the copy loops' head and tail: PNG streams start at every residue mod 4
        assert wt.png_stream_residues(root) == {0, 1, 2, 3}, wt.png_stream_residues(root)
    out = sys.argv[1] if len(sys.argv) > 1 else wt.GOLDEN
    with open(out, "w") as f:
        json.dump(hashes, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(hashes), "hashes ->", out)


if __name__ == "__main__":
    main()
