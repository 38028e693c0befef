"""GPU: the 2D device results writer -- vx_png_encode files checked chunk by chunk (signature, CRCs, the inflated IDAT
against write_png's raw scanlines, decoded pixels against colorize), save_images_device / ResultsWriter2D writing the
tree save_prediction / save_uncertainty write, and vx_gzip_encode's members unchanged by the shared encoder."""
import hashlib
import io
import os
import struct
import tempfile
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

UNC = ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")


def blocky_masks(B, N, H, W, seed=0):
    """(B, N, H, W) uint8 street-scene-like arg-max masks: sky / building / road bands, a few dozen rectangular objects,
    and per-view disagreement in small patches (what the TTA views of one image differ by)"""
    rng = np.random.default_rng(seed)
    out = np.empty((B, N, H, W), np.uint8)
    for b in range(B):
        base = np.empty((H, W), np.uint8)
        h1, h2 = int(H * rng.uniform(0.25, 0.4)), int(H * rng.uniform(0.55, 0.7))
        base[:h1], base[h1:h2], base[h2:] = 10, 2, 0
        for _ in range(40):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            hh, ww = int(rng.integers(H // 40 + 1, H // 6 + 2)), int(rng.integers(W // 60 + 1, W // 5 + 2))
            base[y0:y0 + hh, x0:x0 + ww] = rng.choice([1, 5, 8, 11, 13, 17, 18])
        for t in range(N):
            m = base.copy()
            for _ in range(12):
                y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                m[y0:y0 + H // 50 + 1, x0:x0 + W // 50 + 1] = rng.integers(0, 19)
            out[b, t] = m
    return out


def _gzip_inputs():
    """fixed, seeded members for the gzip digests: (bytes as a uint8 array, stride hints); integer-only generation, so
    the bytes are the same on every host"""
    rng = np.random.default_rng(2024)
    W = 640
    blocks = np.repeat(np.repeat(rng.integers(0, 24, (12, 20), dtype=np.uint8), 40, 0), 32, 1)     # 480 x 640 labels
    rgb = np.stack([blocks * 7, blocks * 13, 255 - blocks * 5], -1).astype(np.uint8)
    raw = np.concatenate([np.zeros((480, 1), np.uint8), rgb.reshape(480, 3 * W)], 1).reshape(-1)   # PNG scanlines
    mask = np.zeros((64, 64, 64), np.uint8)
    mask[20:30, 10:40, 30:34] = 1
    mask[40:44, 40:44, 40:44] = 2
    f64 = rng.random((32, 32, 16))
    f64[:, :, 8:] = np.round(f64[:, :, 8:] * 4) / 4
    return {
        "empty": (np.zeros(0, np.uint8), None),
        "one": (np.array([42], np.uint8), None),
        "zeros": (np.zeros(200_000, np.uint8), None),
        "random": (rng.integers(0, 256, 300_000, dtype=np.uint8), None),
        "low_entropy": (rng.integers(0, 4, 3 * 32768 - 1, dtype=np.uint8), None),
        "edge_exact": (rng.integers(0, 16, 2 * 32768, dtype=np.uint8), (1, 0, 0)),
        "edge_plus": (rng.integers(0, 8, 2 * 32768 + 1, dtype=np.uint8), None),
        "ramp": (np.tile(np.arange(100, dtype=np.uint8), 1000), None),
        "png_scanlines": (raw, (3, 3 * W + 1, 0)),
        "mask": (np.asfortranarray(mask).ravel(order="F"), (1, 64, 4096)),
        "f64": (np.frombuffer(np.asfortranarray(f64).tobytes(order="F"), np.uint8), (8, 256, 8192)),
    }


GZIP_SHA256 = {  # vx_gzip_encode of _gzip_inputs() at the commit before the encoder was shared with png.hip
    "empty": "ac73670af3abed54ac6fb4695131f4099be9fbe39d6076c5d0264a6bbdae9d83",
    "one": "9815d26fccc3ba164cdc9b6683aeb7b73223cd561b93455b6f0621eac2e942f7",
    "zeros": "6b699e66d685a1fc533da28029d79b43bcd39c16ba311b3136e2007a1cf76877",
    "random": "7416ecad74f9e1c4b4f83e17a31cd9a41818f2ca911e1c388e686f783933bc69",
    "low_entropy": "7c16ab18e2243238fed2b4ba90226df9b7bef4293858340c86ada16ca29121cb",
    "edge_exact": "69444d60b9cf0e7e271df69f6b6f52f3a0dfb3f725671dc89092f85a591bba8d",
    "edge_plus": "ef2a145aceb5fe4565ae6060f6f882bc545022b39ca218207f886c6fc6c91aa7",
    "ramp": "21c30471cd6ac5a2027772114a12651284fb159bee2482310c4cb5b861aff024",
    "png_scanlines": "d6c9b97d4a50623731bdab8adb2215235af03fbdce14c7c574eca9ecead8f2f1",
    "mask": "7043499dbe54d03d985af78eec874cae01bdb1d838d4633971c5cda519410424",
    "f64": "ae32d723b71f0f136ff74176aa43cf00da6d0e10f6b8be72039894d6467d6284",
}


def _chunks(buf):
    assert buf[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(buf):
        n, tag = struct.unpack(">I4s", buf[pos:pos + 8])
        data = buf[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", buf[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xFFFFFFFF, ("chunk CRC", tag)
        out.append((tag, data))
        pos += 12 + n
    assert pos == len(buf)
    return out


def _check_png(buf, lab, ign=None):
    """signature, every chunk's CRC, IHDR, the inflated IDAT against write_png's raw scanlines, the decoded pixels
    against colorize (and PIL where it is installed)"""
    from values_amd.image_io import read_png
    from values_amd.results2d import colorize
    H, W = lab.shape
    ch = _chunks(buf)
    assert [t for t, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    assert ch[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    assert ch[2][1] == b""
    assert ch[1][1][:2] == b"\x78\x01"
    rgb = colorize(lab, ign).cpu().numpy()
    raw = np.concatenate([np.zeros((H, 1), np.uint8), rgb.reshape(H, -1)], axis=1).tobytes()
    assert zlib.decompress(ch[1][1]) == raw   # zlib checks the Adler-32
    with tempfile.NamedTemporaryFile(suffix=".png") as f:
        f.write(buf)
        f.flush()
        np.testing.assert_array_equal(read_png(f.name), rgb)
    try:
        from PIL import Image
    except ImportError:
        return
    np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(buf)).convert("RGB")), rgb)


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _encode(masks, ignores=None):
    from values_amd.results2d import png_encode
    return png_encode(masks, ignores)


@pytest.mark.parametrize("shape", [(1, 1), (300, 1), (1, 7), (2, 5461), (3, 5461), (1024, 2048)])
def test_png_shapes_random_labels(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    lab = _dev(rng.integers(0, 24, shape, dtype=np.uint8))
    (buf,) = _encode([lab])
    _check_png(buf, lab)


def test_png_contents():
    rng = np.random.default_rng(3)
    H, W = 97, 131
    cases = {
        "one_label": (_dev(np.full((H, W), 13, np.uint8)), None),
        "outside_table_and_255": (_dev(rng.integers(0, 256, (H, W), dtype=np.uint8)), None),
        "all_255": (_dev(np.full((H, W), 255, np.uint8)), None),
        "all_ignored": (_dev(rng.integers(0, 24, (H, W), dtype=np.uint8)), _dev(np.ones((H, W), np.uint8))),
        "some_ignored": (_dev(rng.integers(0, 24, (H, W), dtype=np.uint8)), _dev(rng.integers(0, 3, (H, W), dtype=np.uint8))),
    }
    bufs = _encode([c[0] for c in cases.values()], [c[1] for c in cases.values()])
    for (k, (lab, ign)), buf in zip(cases.items(), bufs):
        _check_png(buf, lab, ign)
    assert len(bufs[0]) < 1000, len(bufs[0])   # one colour everywhere: a few hundred bytes, not a stored image


def test_png_mixed_shapes_one_call_deterministic():
    rng = np.random.default_rng(4)
    shapes = [(1, 1), (5, 3), (2, 5461), (64, 64), (3, 5461), (256, 478), (1, 1), (700, 9)]
    labs = [_dev(rng.integers(0, 24, s, dtype=np.uint8)) for s in shapes]
    ign = [None if i % 2 else _dev(rng.integers(0, 2, s, dtype=np.uint8)) for i, s in enumerate(shapes)]
    a = _encode(labs, ign)
    b = _encode(labs, ign)
    assert a == b
    for buf, lab, g in zip(a, labs, ign):
        _check_png(buf, lab, g)
    singles = [_encode([lab], [g])[0] for lab, g in zip(labs, ign)]
    assert singles == a   # a file does not depend on its batch


def _files(d):
    out = {}
    for root, _, fs in os.walk(d):
        for f in fs:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = p
    return out


def _same_trees(host_dir, dev_dir):
    from values_amd.image_io import read_png
    h, d = _files(host_dir), _files(dev_dir)
    assert set(h) == set(d)
    for k in h:
        a, b = open(h[k], "rb").read(), open(d[k], "rb").read()
        if k.endswith(".png"):
            _chunks(b)
            np.testing.assert_array_equal(read_png(d[k]), read_png(h[k]), err_msg=k)
        else:
            assert a == b, k
    return h


def _batch(B, N, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    pm = _dev(blocky_masks(B, N, H, W, seed))
    mean = pm[:, 0].clone() if N > 1 else None
    unc = {k: torch.rand(B, H, W, device="cuda", generator=g) for k in UNC}
    ign = (torch.rand(B, H, W, device="cuda", generator=g) > 0.9).to(torch.uint8)
    return pm, mean, unc, ign


def _host_tree(root, ids, pm, mean, unc, ign):
    from values_amd.results2d import save_prediction, save_uncertainty
    os.makedirs(os.path.join(root, "pred_seg"), exist_ok=True)
    for b, iid in enumerate(ids):
        save_prediction(os.path.join(root, "pred_seg"), iid, pm[b], None if mean is None else mean[b], ign[b])
        save_uncertainty(root, iid, {k: v[b] for k, v in unc.items()})


@pytest.mark.parametrize("N", [1, 4])
def test_save_images_device_and_writer_match_host(tmp_path, N):
    from values_amd.results2d import ResultsWriter2D, plan_images, save_images_device
    B, H, W = 3, 96, 160
    ids = ["frankfurt_000000_000294", "lindau_000001_000019", "munster_000002_000019"]
    pm, mean, unc, ign = _batch(B, N, H, W, seed=N)
    _host_tree(str(tmp_path / "host"), ids, pm, mean, unc, ign)
    save_images_device(str(tmp_path / "dev"), ids, pm, mean, unc, ign)
    files = _same_trees(str(tmp_path / "host"), str(tmp_path / "dev"))
    assert sorted(files) == sorted(f.path for f in plan_images(ids, N, UNC))
    # the pipelined writer, two batches through both buffer sets and a third that reuses the first
    with ResultsWriter2D(workers=3) as w:
        for r in range(3):
            w.submit(str(tmp_path / f"pipe{r}"), ids, pm, mean, unc, ign)
    for r in range(3):
        _same_trees(str(tmp_path / "host"), str(tmp_path / f"pipe{r}"))
    # a shared (H, W) ignore map
    _host_tree(str(tmp_path / "host2"), ids, pm, mean, unc, [ign[0]] * B)
    save_images_device(str(tmp_path / "dev2"), ids, pm, mean, unc, ign[0])
    _same_trees(str(tmp_path / "host2"), str(tmp_path / "dev2"))


def test_writer_reraises_write_error(tmp_path):
    from values_amd.results2d import ResultsWriter2D
    pm, mean, unc, ign = _batch(1, 2, 16, 24, seed=9)
    bad = tmp_path / "bad"
    os.makedirs(bad / "pred_seg" / "x_mean.png")   # a directory stands where a file is to be written
    w = ResultsWriter2D(workers=2)
    w.submit(str(bad), ["x"], pm, mean, unc)
    with pytest.raises(IsADirectoryError):
        w.close()


PNG_BYTES_RATIO_MAX = 1.12   # about 1.2 x the 0.94 measured on one MI355X


def test_compression_against_write_png(tmp_path):
    from values_amd.image_io import write_png
    from values_amd.results2d import colorize
    masks = blocky_masks(2, 3, 512, 1024, seed=0).reshape(6, 512, 1024)
    labs = [_dev(m) for m in masks]
    bufs = _encode(labs)
    host = 0
    for lab in labs:
        p = str(tmp_path / "h.png")
        write_png(p, colorize(lab).cpu().numpy())
        host += os.path.getsize(p)
    dev = sum(len(b) for b in bufs)
    print(f"PNG bytes: device {dev}, write_png {host}, ratio {dev / host:.3f}")
    assert dev <= PNG_BYTES_RATIO_MAX * host, (dev, host)


def test_gzip_members_unchanged():
    from values_amd import gz
    ins = _gzip_inputs()
    names = list(ins)
    outs = gz.gzip_encode([_dev(ins[k][0]) for k in names], [ins[k][1] for k in names])
    got = {k: hashlib.sha256(bytes(o)).hexdigest() for k, o in zip(names, outs)}
    assert got == GZIP_SHA256
