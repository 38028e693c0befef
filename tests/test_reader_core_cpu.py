"""CPU: the reader core the device readers share (values_amd/_devio.py) -- the staging layout as a pure function, and
the pipelined reader's order, look-ahead and error behaviour with the device half replaced by a subclass that returns
what it was given."""
import threading

import pytest

from values_amd import _devio


def test_plan_lays_items_out_at_256_byte_boundaries():
    pieces = [(b"", []), (b"x" * 600, [(10, 100), (300, 200)]), (b"y" * 257, [(0, 257)])]
    offs, sizes, total = _devio.plan(pieces)
    assert sizes == [0, 300, 257]
    assert all(o % 256 == 0 for o in offs) and total % 256 == 0
    regions = sorted(zip(offs, sizes))
    for (o, n), (o2, _) in zip(regions, regions[1:] + [(total, 0)]):
        assert o + max(n, 1) <= o2, (offs, sizes, total)      # no overlap; an empty item keeps a region of its own
    assert len(set(offs)) == 3
    assert _devio.plan([]) == ([], [], 0)


class EchoReader(_devio.PipelinedReader):
    def __init__(self, on_decode=None, **kw):
        super().__init__(**kw)
        self.decoded = []
        self.on_decode = on_decode

    def _decode(self, names, raws, device):
        if self.on_decode:
            self.on_decode(names)
        self.decoded.append(list(names))
        return names, raws


@pytest.fixture
def no_gpu(monkeypatch):
    monkeypatch.setattr(_devio._lib, "require_gpu", lambda: None)
    monkeypatch.setattr(_devio, "current_device", lambda device=None: "dev")


@pytest.fixture
def files(tmp_path):
    out = []
    for nm in "abc":
        p = tmp_path / f"{nm}.bin"
        p.write_bytes(nm.encode() * 3)
        out.append(p)
    return out


def test_batches_come_back_in_order_and_an_empty_batch_is_not_decoded(files, no_gpu):
    a, b, c = (str(p) for p in files)
    with EchoReader(workers=2) as r:
        out = list(r.read([files[:2], [], files[2:]]))
    assert out == [([a, b], [b"aaa", b"bbb"]), [], ([c], [b"ccc"])]
    assert r.decoded == [[a, b], [c]]          # the empty batch never reached _decode


def test_the_next_batch_is_with_the_pool_before_this_one_is_decoded(files, monkeypatch, no_gpu):
    a, b, c = (str(p) for p in files)
    handed_over = threading.Event()
    plain_read = _devio._read

    def read(path):
        if path == c:
            handed_over.set()
        return plain_read(path)

    monkeypatch.setattr(_devio, "_read", read)
    ahead = []

    def on_decode(names):
        if names == [a, b]:
            ahead.append(handed_over.wait(timeout=10))   # set by a pool thread: returns at once where the reader looks ahead

    with EchoReader(on_decode=on_decode, workers=2) as r:
        out = list(r.read([files[:2], files[2:]]))
    assert ahead == [True]
    assert [names for names, _ in out] == [[a, b], [c]]


def test_a_missing_file_raises_at_its_batch_and_close_returns(tmp_path, no_gpu):
    a = tmp_path / "a.bin"
    a.write_bytes(b"a")
    r = EchoReader(workers=2)
    it = r.read([[a], [tmp_path / "missing.bin"]])
    assert next(it) == ([str(a)], [b"a"])
    with pytest.raises(FileNotFoundError):
        next(it)
    r.close()
    assert r.decoded == [[str(a)]]


def test_messages_carry_the_subclass_name():
    with pytest.raises(ValueError, match="EchoReader: workers >= 1"):
        EchoReader(workers=0)
    from values_amd import images, nifti
    with pytest.raises(ValueError, match="NiftiReader: workers >= 1"):
        nifti.NiftiReader(workers=0)
    with pytest.raises(ValueError, match="ImageReader: workers >= 1"):
        images.ImageReader(workers=0)
