"""GPU: every file of every device writer, byte for byte against tests/golden/writer_bytes.json -- the hashes
tools/gen_writer_hashes.py recorded before the writers' shared steps were moved into one core (tests/writer_trees.py
describes the inputs).  The encoders are deterministic, so a changed hash is a changed file."""
import json

import pytest

from tests import writer_trees as wt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("writer_bytes"))
    return root, wt.build(root)


@pytest.fixture(scope="module")
def golden():
    with open(wt.GOLDEN) as f:
        return json.load(f)


def test_the_same_files_are_written(built, golden):
    assert sorted(built[1]) == sorted(golden)
    kinds = {k.split("/")[0] for k in golden}
    assert kinds == {"case3d", "maps", "2d", "gzip_encode", "png_encode", "abi_gzip"}


@pytest.mark.parametrize("kind", ("case3d", "maps", "2d", "gzip_encode", "png_encode", "abi_gzip"))
def test_every_byte_is_the_recorded_one(built, golden, kind):
    names = [k for k in golden if k.split("/")[0] == kind]
    assert names
    bad = [k for k in names if built[1].get(k) != golden[k]]
    assert not bad, (len(bad), "of", len(names), "differ; first:", bad[:5])


def test_png_streams_start_at_every_residue_mod_4(built):
    assert wt.png_stream_residues(built[0]) == {0, 1, 2, 3}
