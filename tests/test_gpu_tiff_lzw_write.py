"""GPU: LZW-compressed float32 TIFF maps written on the device -- vx_tiff_predict against the forward predictors of
tests/lzw_build.py, vx_tiff_lzw_encode against the test encoder (tests/lzw_build.lzw_encode, validated against libtiff
in test_tiff_lzw_cpu.py) byte for byte, vx_tiff_lzw_pack, the argument checks, and the 2D writers with tiff="lzw"
against the host writer's files, both readers and the aggregation of a written tree.  Expected bytes are never the code
under test's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import lzw_build as lb

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
OK, NO_ROOM = 0, 3


@pytest.fixture(scope="module")
def corpus():
    """[(name, payload, the strip the test encoder makes of it)]: empty, 1, 3 and 4 bytes, 48 000 random bytes, a random
    walk, text, 200 000 constant bytes"""
    out = [(name, data, strip) for name, (strip, data, _) in lb.stream_corpus().items() if "_" not in name]
    assert [c[0] for c in out] == ["empty", "b1", "b3", "b4", "random", "walk", "text", "const"]
    return out


def _table(entries):
    from values_amd import _lib
    arr = (_lib.TiffLzwItem * max(len(entries), 1))()
    for it, (src, n, off, cap) in zip(arr, entries):
        it.src, it.src_n, it.dst_off, it.dst_cap = src, n, off, cap
    return arr


def _encode(items):
    """items: [(payload, window size, gap before the window, gap before the source)] -> (sizes, statuses, [the window's
    bytes]): one vx_tiff_lzw_encode call; sources and windows lie in one buffer each, the gaps put them at odd addresses,
    and every byte outside the windows must keep the sentinel."""
    from values_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    blob, srcs = bytearray(), []
    for d, _, _, sgap in items:
        blob += bytes([0x5A]) * sgap
        srcs.append(len(blob))
        blob += d
    src = torch.from_numpy(np.frombuffer(bytes(blob) + b"\x5A", dtype=np.uint8).copy()).to(dev)
    offs, off = [], 0
    for _, cap, gap, _ in items:
        off += gap
        offs.append(off)
        off += cap
    total = off + 5
    dst = torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
    n = len(items)
    arr = _table([(C.c_void_p(src.data_ptr() + a) if d else None, len(d), o, cap) for (d, cap, _, _), a, o in zip(items, srcs, offs)])
    sizes = torch.full((n,), -7, dtype=torch.int64, device=dev)
    st = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.vx_tiff_lzw_encode_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    _lib.check(lib.vx_tiff_lzw_encode(arr, n, dst.data_ptr(), total, sizes.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _lib.stream_ptr()), "vx_tiff_lzw_encode")
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    inside = np.zeros(total, dtype=bool)
    for o, (_, cap, _, _) in zip(offs, items):
        inside[o:o + cap] = True
    assert (host[~inside] == SENTINEL).all(), "a write outside every window"
    return sizes.cpu().tolist(), st.cpu().tolist(), [host[o:o + cap] for o, (_, cap, _, _) in zip(offs, items)]


def _check(names, want, sizes, st, outs):
    for name, w, n, s, out in zip(names, want, sizes, st, outs):
        assert s == OK and n == len(w), (name, s, n, len(w))
        assert out[:n].tobytes() == w, (name, "first mismatch at", int(np.argmax(out[:n] != np.frombuffer(w, np.uint8))))
        assert (out[n:] == SENTINEL).all(), (name, "bytes at or behind out_sizes were written")   # the header: none are


def test_predict_against_the_forward_predictors():
    """W 1, 2, 3 (less than a quad), 63, 64, 65 (around a wave), 300, 1025 (several blocks, a last quad of one), rows 1
    and 7, both predictors; random bit patterns, so the differences wrap mod 256 and mod 2^32; sources and outputs at
    every alignment; then vx_tiff_unpredict gives the source back"""
    from values_amd import _lib, images
    from values_amd._devio import item_statuses
    dev = torch.device("cuda")
    rng = np.random.default_rng(43)
    cases = []
    for w in (1, 2, 3, 63, 64, 65, 300, 1025):
        for rows in (1, 7):
            for pred in (2, 3):
                m = rng.integers(0, 1 << 32, (rows, w), dtype=np.uint64).astype(np.uint32).view(np.float32)
                cases.append((m, pred, lb.row_bytes(m, "<", pred).tobytes()))
    blob, soffs = bytearray(), []
    for k, (m, _, _) in enumerate(cases):
        blob += bytes((k % 4 - len(blob)) % 4 + 4)             # source alignment k % 4
        soffs.append(len(blob))
        blob += m.tobytes()
    src = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).to(dev)
    doffs, off = [], 0
    for k, (m, _, _) in enumerate(cases):
        off += ((k // 4) % 4 - off) % 4 + 4                    # output alignment (k // 4) % 4: all 16 pairs occur
        doffs.append(off)
        off += m.nbytes
    assert {(s % 4, d % 4) for s, d in zip(soffs, doffs)} == {(a, b) for a in range(4) for b in range(4)}
    dst = torch.full((off + 8,), SENTINEL, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 4 == 0 and dst.data_ptr() % 4 == 0
    arr = (_lib.TiffUnpredictItem * len(cases))()
    for it, (m, pred, _), so, do in zip(arr, cases, soffs, doffs):
        it.src, it.dst, it.rows, it.W, it.predictor = src.data_ptr() + so, dst.data_ptr() + do, m.shape[0], m.shape[1], pred
    assert item_statuses("vx_tiff_predict", arr, dev) == [0] * len(cases)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    inside = np.zeros(host.size, dtype=bool)
    for (m, pred, fwd), so, do in zip(cases, soffs, doffs):
        got = host[do:do + m.nbytes]
        bad = np.flatnonzero(got != np.frombuffer(fwd, np.uint8))
        assert bad.size == 0, (m.shape, pred, so % 4, do % 4, "first mismatch at byte", int(bad[0]))
        inside[do:do + m.nbytes] = True
    assert (host[~inside] == SENTINEL).all(), "a write outside every output"
    # and back: vx_tiff_unpredict of the result is the source, bit for bit
    back = torch.full((len(blob) + 8,), SENTINEL, dtype=torch.uint8, device=dev)
    st = images.tiff_unpredict([(C.c_void_p(dst.data_ptr() + do), C.c_void_p(back.data_ptr() + so), m.shape[0], m.shape[1], pred)
                                for (m, pred, _), so, do in zip(cases, soffs, doffs)], dev)
    assert st == [0] * len(cases)
    hb = back.cpu().numpy()
    for (m, pred, _), so in zip(cases, soffs):
        assert hb[so:so + m.nbytes].tobytes() == m.tobytes(), (m.shape, pred)


def test_encode_the_corpus_in_one_call_and_one_by_one(corpus):
    from values_amd import _lib, images
    lib = _lib.load()
    names = [c[0] for c in corpus]
    want = [c[2] for c in corpus]
    for (_, d, s) in corpus:
        assert len(s) <= lib.vx_tiff_lzw_bound(len(d))
    assert [lib.vx_tiff_lzw_bound(n) for n in (-1, 0, 1, 3835, 3836, 8192)] == [-1, 3, 5, 5756, 5759, 12294]
    # windows of the bound and of exactly the strip, at every alignment; sources at odd addresses
    items = [(d, int(lib.vx_tiff_lzw_bound(len(d))) if k % 2 else len(s), 1 + k % 4, (3 * k) % 4) for k, (_, d, s) in enumerate(corpus)]
    sizes, st, outs = _encode(items)
    _check(names, want, sizes, st, outs)
    # batch independence: the same items one per call
    for name, item, w in zip(names, items, want):
        s1, t1, o1 = _encode([item])
        _check([name], [w], s1, t1, o1)
    # vx_tiff_lzw decodes every produced strip back to its payload
    dev = torch.device("cuda")
    blob = b"".join(o[:n].tobytes() for o, n in zip(outs, sizes))
    src = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).to(dev)
    total = sum(len(d) for _, d, _ in corpus)
    dec = torch.full((total + 1,), SENTINEL, dtype=torch.uint8, device=dev)
    entries, so, do = [], 0, 0
    for (_, d, _), n in zip(corpus, sizes):
        entries.append((C.c_void_p(src.data_ptr() + so), n, do, len(d)))
        so += n
        do += len(d)
    dsz, dst_ = images.lzw_into(entries, dev, dec)
    assert dst_ == [0] * len(corpus) and dsz == [len(d) for _, d, _ in corpus]
    assert dec.cpu().numpy()[:total].tobytes() == b"".join(d for _, d, _ in corpus)


def test_a_window_one_byte_too_small_is_no_room_for_that_item_only(corpus):
    by = {c[0]: c for c in corpus}
    # (name, bytes the window lacks): one byte too small overflows at the strip's last bytes; the last item's window of
    # 5000 bytes overflows while the strip is still being flushed
    order = [("text", 0), ("random", 1), ("b1", 1), ("empty", 1), ("walk", 0), ("const", 1), ("b4", 0),
             ("random", len(by["random"][2]) - 5000)]
    items = [(by[n][1], len(by[n][2]) - cut, 1 + k % 3, k % 4) for k, (n, cut) in enumerate(order)]
    sizes, st, outs = _encode(items)
    for (name, cut), (_, cap, _, _), n, s, out in zip(order, items, sizes, st, outs):
        w = by[name][2]
        if cut:
            assert s == NO_ROOM and n == cap, (name, s, n, cap)     # the header: the strip's first dst_cap bytes
            assert out[:n].tobytes() == w[:n] and (out[n:] == SENTINEL).all(), name
        else:
            _check([name], [w], [n], [s], [out])


def test_pack_makes_the_strips_contiguous(corpus):
    """the corpus' strips from windows at odd places into a blob at an odd address: the exclusive scan of the sizes, the
    bytes, nothing outside the blob; a size outside [0, dst_cap] is read as clamped; a blob larger than out_n is not
    written beyond it"""
    from values_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    strips = [c[2] for c in corpus]
    n = len(strips)
    blob, wins = bytearray(), []
    for k, s in enumerate(strips):
        blob += bytes([0x11]) * (1 + k % 4)
        wins.append((len(blob), len(s) + k))              # a window larger than the strip
        blob += s + bytes([0x22]) * k
    src = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).to(dev)
    arr = _table([(None, 0, o, cap) for o, cap in wins])
    ws = torch.empty(int(lib.vx_tiff_lzw_pack_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    total = sum(len(s) for s in strips)

    def pack(size_list, out_n, shift):
        sizes = torch.tensor(size_list, dtype=torch.int64, device=dev)
        out = torch.full((shift + out_n + 9,), SENTINEL, dtype=torch.uint8, device=dev)
        offs = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
        _lib.check(lib.vx_tiff_lzw_pack(arr, n, src.data_ptr(), src.numel(), sizes.data_ptr(), out.data_ptr() + shift, out_n,
                                        offs.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "vx_tiff_lzw_pack")
        torch.cuda.synchronize()
        return out.cpu().numpy(), offs.cpu().tolist()

    for shift in (0, 1, 3):
        host, offs = pack([len(s) for s in strips], total, shift)
        assert offs == [sum(len(s) for s in strips[:k]) for k in range(n + 1)]
        assert host[shift:shift + total].tobytes() == b"".join(strips)
        assert (host[:shift] == SENTINEL).all() and (host[shift + total:] == SENTINEL).all()
    # sizes outside the windows are read as clamped
    host, offs = pack([-5] + [len(s) for s in strips[1:-1]] + [1 << 40], total + n, 0)
    assert offs[1] == 0 and offs[n] - offs[n - 1] == wins[-1][1]
    # a blob larger than out_n: the strips that fit are copied, nothing lies beyond out_n, the total says so
    host, offs = pack([len(s) for s in strips], total - 100, 2)
    assert offs[n] == total and (host[2 + total - 100:] == SENTINEL).all() and (host[:2] == SENTINEL).all()
    k = max(k for k in range(n) if offs[k + 1] <= total - 100)
    assert host[2:2 + offs[k + 1]].tobytes() == b"".join(strips[:k + 1])


def test_argument_errors_are_refused_before_any_launch():
    from values_amd import _lib
    lib = _lib.load()
    dummy, big = 0x10000, 1 << 20

    def enc(items, n=None, dst=dummy, dst_n=4096, sizes=dummy, st=dummy, ws=dummy, ws_n=big, table=True):
        return lib.vx_tiff_lzw_encode(_table(items) if table else None, len(items) if n is None else n, dst, dst_n, sizes, st, ws,
                                      ws_n, None)

    ok = (dummy, 10, 0, 100)
    assert enc([], n=0, table=False) == 0
    assert lib.vx_tiff_lzw_encode_workspace_bytes(-1) == -1 and lib.vx_tiff_lzw_pack_workspace_bytes(-1) == -1
    assert lib.vx_tiff_predict_workspace_bytes(-1) == -1
    refused = [enc([ok], table=False), enc([ok], n=-1), enc([ok], dst=None), enc([ok], sizes=None), enc([ok], st=None), enc([ok], ws=None),
               enc([ok], ws_n=lib.vx_tiff_lzw_encode_workspace_bytes(1) - 1), enc([ok], dst_n=-1),
               enc([(None, 10, 0, 100)]), enc([(dummy, -1, 0, 100)]), enc([(dummy, 10, -1, 100)]), enc([(dummy, 10, 0, -1)]),
               enc([(dummy, 10, 4000, 100)]),                                # a window beyond dst_n
               enc([ok, (dummy, 10, 50, 100)])]                              # windows that overlap
    for rc in refused:
        assert rc < 0, (rc, lib.vx_last_error_string())

    def prd(items, n=None, status=dummy, ws=dummy, ws_n=big, table=True):
        arr = (_lib.TiffUnpredictItem * max(len(items), 1))()
        for it, (src, dst, rows, w, pred) in zip(arr, items):
            it.src, it.dst, it.rows, it.W, it.predictor = src, dst, rows, w, pred
        return lib.vx_tiff_predict(arr if table else None, len(items) if n is None else n, status, ws, ws_n, None)

    a, b = 0x10000, 0x90000
    good = (a, b, 4, 16, 3)
    assert prd([], n=0, table=False) == 0
    refused = [prd([good], table=False), prd([good], n=-1), prd([good], status=None), prd([good], ws=None),
               prd([good], ws_n=lib.vx_tiff_predict_workspace_bytes(1) - 1),
               prd([(a, b, 4, 0, 3)]), prd([(a, b, 0, 16, 2)]), prd([(a, b, 4, 16, 1)]), prd([(a, b, 4, 16, 4)]),
               prd([(None, b, 4, 16, 2)]), prd([(a, None, 4, 16, 2)]),
               prd([(a, a, 4, 16, 2)]), prd([(a, a + 64, 4, 16, 3)])]          # in place, a partial overlap
    for rc in refused:
        assert rc < 0, (rc, lib.vx_last_error_string())

    def pck(items, n=None, src=a, src_n=4096, sizes=dummy, out=b, out_n=4096, offs=dummy, ws=dummy, ws_n=big, table=True):
        return lib.vx_tiff_lzw_pack(_table(items) if table else None, len(items) if n is None else n, src, src_n, sizes, out, out_n,
                                    offs, ws, ws_n, None)

    w = (None, 0, 0, 100)
    assert pck([], n=0, table=False) == 0
    refused = [pck([w], table=False), pck([w], n=-1), pck([w], src=None), pck([w], sizes=None), pck([w], out=None), pck([w], offs=None),
               pck([w], ws=None), pck([w], ws_n=lib.vx_tiff_lzw_pack_workspace_bytes(1) - 1), pck([w], src_n=-1), pck([w], out_n=-1),
               pck([(None, 0, 4000, 100)]), pck([(None, 0, -1, 100)]), pck([(None, 0, 0, -1)]), pck([w], out=a + 64)]
    for rc in refused:
        assert rc < 0, (rc, lib.vx_last_error_string())


# ---------------------------------------------------------------------------------------------------------------------
NAMES = ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")


@pytest.fixture(scope="module")
def batches():
    """two batches of B = 2 images, N = 2 predictions, 7 x 700, three maps each: smooth fields with -0.0, infinities, a
    NaN and denormals among them"""
    rng = np.random.default_rng(9)
    B, N, H, W = 2, 2, 7, 700
    out = []
    for k in range(2):
        pm = rng.integers(0, 24, (B, N, H, W)).astype(np.uint8)
        mm = rng.integers(0, 24, (B, H, W)).astype(np.uint8)
        unc = {}
        for j, name in enumerate(NAMES):
            m = np.stack([lb.smooth_map(H, W, seed=10 * k + 3 * j + b) for b in range(B)])
            flat = m.reshape(-1).view(np.uint32)
            for i, v in enumerate((0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0x00000001, 0x807FFFFF)):
                flat[(1000 * j + 577 * i) % flat.size] = v
            unc[name] = m
        ign = (rng.random((B, H, W)) < 0.1).astype(np.uint8)
        out.append(([f"img{k}_{b}" for b in range(B)], pm, mm, unc, ign))
    return out


def _tree(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def default_tree(batches, tmp_path_factory):
    """the trees of the default call over the first batch, with and without an ignore map"""
    from values_amd import results2d
    ids, pm, mm, unc, ign = batches[0]
    out = {}
    for with_ign in (False, True):
        d = str(tmp_path_factory.mktemp("default"))
        results2d.save_images_device(d, ids, pm, mm, unc, ign if with_ign else None)
        out[with_ign] = _tree(d)
    return out


def test_default_call_writes_the_uncompressed_files(batches, default_tree, tmp_path):
    from values_amd.image_io import write_tiff_f32
    ids, _, _, unc, _ = batches[0]
    for name in NAMES:
        for b, iid in enumerate(ids):
            p = str(tmp_path / "w.tif")
            write_tiff_f32(p, unc[name][b])
            assert default_tree[False][os.path.join(name, iid + ".tif")] == open(p, "rb").read()
    assert sum(k.endswith(".tif") for k in default_tree[False]) == 6 and sum(k.endswith(".png") for k in default_tree[False]) == 6


@pytest.mark.parametrize("with_ign", (False, True))
@pytest.mark.parametrize("predictor", (1, 2, 3))
def test_device_writer_equals_the_host_writer(batches, default_tree, tmp_path, predictor, with_ign):
    from values_amd import images, results2d
    from values_amd.image_io import read_tiff_f32, tiff_parse
    ids, pm, mm, unc, ign = batches[0]
    d = str(tmp_path / "dev")
    results2d.save_images_device(d, ids, pm, mm, unc, ign if with_ign else None, tiff="lzw", tiff_predictor=predictor)
    got = _tree(d)
    base = default_tree[with_ign]
    assert sorted(got) == sorted(base)
    h = str(tmp_path / "host")
    for b, iid in enumerate(ids):
        results2d.save_uncertainty(h, iid, {k: torch.from_numpy(v[b]) for k, v in unc.items()}, compression="lzw", predictor=predictor)
    want = _tree(h)
    tifs = sorted(k for k in got if k.endswith(".tif"))
    assert tifs == sorted(want) and len(tifs) == 6
    for k in tifs:
        assert got[k] == want[k], k
        t = tiff_parse(got[k])
        assert t.lzw and t.predictor == predictor and [s[:2] for s in t.strips] == [(0, 2), (2, 2), (4, 2), (6, 1)]
    for k in got:
        if k.endswith(".png"):
            assert got[k] == base[k], k                     # the PNG files do not depend on the TIFF option
    paths = [os.path.join(d, k) for k in tifs]
    for k, p, t in zip(tifs, paths, images.load_tiff_device(paths)):
        m = unc[os.path.dirname(k)][ids.index(os.path.basename(k)[:-4])]
        assert torch.equal(t.view(torch.int32).cpu(), torch.from_numpy(m.view(np.int32).copy())), k
        assert np.array_equal(read_tiff_f32(p).view(np.uint32), m.view(np.uint32)), k


def test_rows_per_strip_and_refused_options(batches, tmp_path):
    from values_amd import results2d
    ids, pm, mm, unc, _ = batches[0]
    for rps in (1, 7, 100):
        d = str(tmp_path / f"dev{rps}")
        results2d.save_images_device(d, ids, pm, mm, unc, tiff="lzw", tiff_predictor=2, tiff_rows_per_strip=rps)
        h = str(tmp_path / f"host{rps}")
        for b, iid in enumerate(ids):
            results2d.save_uncertainty(h, iid, {k: v[b] for k, v in unc.items()}, compression="lzw", predictor=2, rows_per_strip=rps)
        got, want = _tree(d), _tree(h)
        for k in want:
            assert got[k] == want[k], (rps, k)
    for kw in ({"tiff": "deflate"}, {"tiff": "lzw", "tiff_predictor": 4}, {"tiff": "lzw", "tiff_rows_per_strip": 0}):
        with pytest.raises(ValueError):
            results2d.save_images_device(str(tmp_path / "bad"), ids, pm, mm, unc, **kw)
    with pytest.raises(ValueError):
        results2d.ResultsWriter2D(tiff="zip")


def test_pipelined_writer_equals_two_calls(batches, tmp_path):
    from values_amd import results2d
    a, b = str(tmp_path / "writer"), str(tmp_path / "calls")
    with results2d.ResultsWriter2D(tiff="lzw", tiff_predictor=3) as w:
        for ids, pm, mm, unc, ign in batches:
            w.submit(a, ids, pm, mm, unc, ign)
    for ids, pm, mm, unc, ign in batches:
        results2d.save_images_device(b, ids, pm, mm, unc, ign, tiff="lzw", tiff_predictor=3)
    got, want = _tree(a), _tree(b)
    assert sorted(got) == sorted(want) and len(want) == 24
    for k in want:
        assert got[k] == want[k], k


def test_aggregation_over_an_lzw_tree_equals_the_uncompressed_tree(tmp_path):
    """experiment.aggregate_uncertainties_device over the tree save_images_device(tiff="lzw") wrote and over the
    uncompressed tree of the same maps: byte-equal aggregated_<unc>.json"""
    from values_amd import results2d
    from values_amd.experiment import DeviceExperimentDataloader, ExperimentVersion, aggregate_uncertainties_device
    from values_amd.image_io import tiff_parse
    rng = np.random.default_rng(5)
    ids, T, H, W = ["img_a", "img_b", "img_c"], 2, 20, 33
    pm = torch.from_numpy(rng.integers(0, 24, (3, T, H, W)).astype(np.uint8)).cuda()
    mm = torch.from_numpy(rng.integers(0, 24, (3, H, W)).astype(np.uint8)).cuda()
    unc = {k: torch.from_numpy(rng.random((3, H, W), dtype=np.float32)).cuda() for k in NAMES}
    types = ["predictive_uncertainty", "aleatoric_uncertainty", "epistemic_uncertainty"]
    aggs = {"patch_level": {"_target_": "values_amd.aggregation.patch_level_aggregation", "patch_size": 5},
            "image_level": {"_target_": "values_amd.aggregation.image_level_aggregation", "mean": True},
            "threshold": {"_target_": "values_amd.aggregation.threshold_aggregation", "threshold": 0.6}}
    out = {}
    for tag, kw in (("plain", {}), ("lzw", {"tiff": "lzw", "tiff_predictor": 3})):
        ev = ExperimentVersion(base_path=tmp_path / tag, naming_scheme_version="seed{seed}", pred_model="Dropout",
                               image_ending=".png", unc_ending=".tif", unc_types=types, aggregations=None, n_reference_segs=1,
                               pred_seg_loading={"_target_": "evaluation.utils.gta.pred_seg_loading"}, seed=7)
        results2d.save_images_device(str(ev.exp_path / "val"), ids, pm, mm, unc, **kw)
        n = 0
        for root, _, fs in os.walk(ev.exp_path / "val"):
            for f in fs:
                if f.endswith(".tif"):
                    assert tiff_parse(open(os.path.join(root, f), "rb").read()).lzw == (tag == "lzw")
                    n += 1
        assert n == 9
        dev = DeviceExperimentDataloader(ev, "val")
        assert dev.image_ids == ids
        aggregate_uncertainties_device(dev, aggs, batch=2)
        out[tag] = {u: open(dev.dataset_path / f"aggregated_{u}.json", "rb").read() for u in types}
    for u in types:
        assert out["lzw"][u] == out["plain"][u] and len(out["plain"][u]) > 50, u
