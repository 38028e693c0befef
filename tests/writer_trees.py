"""The trees behind tests/golden/writer_bytes.json: every device writer (3D cases, maps, 2D batches, the gzip and PNG
encoders and one vx_gzip_encode call at every destination alignment) run through the public API on small seeded inputs.
tools/gen_writer_hashes.py records {relative path: sha256} once; tests/test_gpu_writer_bytes.py builds the same trees
again and compares.  The inputs are ramps of exact binary fractions plus a block of generator noise, so stored, fixed and
dynamic DEFLATE blocks all occur and no libm function decides a byte."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "writer_bytes.json")
UNC = ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty")


def _mixed(shape, seed, dtype=np.float32):
    """a ramp over the axes (multiples of 1/64) with the generator's noise in its second half along the last axis"""
    rng = np.random.default_rng(seed)
    grid = np.indices(shape)
    a = sum((3 + 2 * k) * g for k, g in enumerate(grid)).astype(np.float64) / 64.0
    half = shape[-1] // 2
    a[..., half:] += rng.random(a[..., half:].shape)
    return a.astype(dtype)


def _labels(shape, seed, classes):
    """blocks of one label with a noisy corner"""
    rng = np.random.default_rng(seed)
    grid = np.indices(shape)
    a = (sum(g // 5 for g in grid) % classes).astype(np.uint8)
    a[..., :3] = rng.integers(0, classes, a[..., :3].shape, dtype=np.uint8)
    return a


def case3d(name, vol, seed):
    """save_case_device's arguments for one case: T = 2, C = 2 float64 probability sums with their counts"""
    rng = np.random.default_rng(seed)
    T, C = 2, 2
    cnt = rng.integers(0, 4, vol).astype(np.float64)            # zeros among them: clipped to 1
    p = _mixed((T, 1) + vol, seed + 1, np.float64)
    p = p / (p.max() + 1.0)
    sm = np.concatenate([p, 1.0 - p], 1) * np.clip(cnt, 1, None)
    return dict(image_id=name, softmax_pred=sm, maps={k: _mixed(vol, seed + 2 + j) for j, k in enumerate(UNC)},
                data=_mixed(vol, seed + 5), gt_seg=_labels((2,) + vol, seed + 6, C), num_predictions=cnt)


def cases3d():
    return [case3d("small", (5, 6, 7), 100), case3d("big", (17, 16, 16), 200)]


def maps(root):
    """(paths, tensors) of one save_maps_device call: .nii.gz (float32, float64), .nii, two .tif of different shapes; the
    first map is a reader's [x, y, z] view (x fastest in memory), the others are arrays in C order"""
    import torch
    arrays = [("a_f32.nii.gz", torch.from_numpy(_mixed((11, 10, 9), 300)).permute(2, 1, 0)), ("b_f64.nii.gz", _mixed((17, 16, 16), 301, np.float64)),
              ("c.nii", _mixed((6, 5, 4), 302)), ("d_9x13.tif", _mixed((9, 13), 303)), ("e.nii", _mixed((7, 3), 304, np.float64)),
              ("f_40x33.tif", _mixed((40, 33), 305))]
    return [os.path.join(root, n) for n, _ in arrays], [a for _, a in arrays]


def batch2d(tag, B, N, H, W, seed, ignore):
    rng = np.random.default_rng(seed)
    pm = _labels((B, N, H, W), seed, 19)
    pm[:, :, H // 2:, W // 2:] = rng.integers(0, 24, pm[:, :, H // 2:, W // 2:].shape, dtype=np.uint8)
    ign = (rng.random((B, H, W)) < 0.1).astype(np.uint8) if ignore else None
    return dict(image_ids=[f"{tag}_{b}" for b in range(B)], pred_masks=pm, mean_masks=_labels((B, H, W), seed + 1, 19),
                uncertainty={k: _mixed((B, H, W), seed + 2 + j) for j, k in enumerate(UNC)}, ignore_index_map=ign)


SMALL, LARGE = (37, 53), (96, 128)   # one chunk per PNG file; 36960 scanline bytes: two
LZW = [dict(tiff="lzw", tiff_predictor=p) for p in (1, 2, 3)]
# (directory, (H, W), N, ignore map, keyword arguments)
CALLS2D = [("s_n2_plain_ign", SMALL, 2, True, {}), ("s_n2_plain", SMALL, 2, False, {}), ("s_n1_plain", SMALL, 1, False, {}),
           ("s_n2_p1_ign", SMALL, 2, True, LZW[0]), ("s_n2_p2", SMALL, 2, False, LZW[1]), ("s_n2_p3_ign", SMALL, 2, True, LZW[2]),
           ("s_n1_p3_ign", SMALL, 1, True, LZW[2])] + \
          [(f"s_n2_p{kw['tiff_predictor']}_rps7", SMALL, 2, p == 1, dict(kw, tiff_rows_per_strip=7)) for p, kw in enumerate(LZW)] + \
          [("l_n2_plain_ign", LARGE, 2, True, {}), ("l_n1_plain", LARGE, 1, False, {}), ("l_n2_p1", LARGE, 2, False, LZW[0]),
           ("l_n2_p2_ign", LARGE, 2, True, LZW[1]), ("l_n2_p3", LARGE, 2, False, LZW[2]), ("l_n1_p3", LARGE, 1, False, LZW[2])]


def _gzip_tensors():
    """(arrays, stride hints) for gz.gzip_encode: empty, one chunk, two chunks with a short last one, noise"""
    rng = np.random.default_rng(400)
    return ([np.zeros(0, np.uint8), _mixed((5, 6, 7), 401), _mixed((17, 16, 16), 402, np.float64),
             rng.integers(0, 256, 40000, dtype=np.uint8)], [None, (4, 20, 120), (8, 136, 2176), None])


def build(root):
    """Writes every tree under root; -> {relative path: sha256} of the files and of the encoders' returned bytes."""
    import torch

    from values_amd import _lib, gz, results, results2d
    extra = {}
    cases = cases3d()
    for c in cases:
        results.save_case_device(os.path.join(root, "case3d", "direct"), **c)
    with results.ResultsWriter() as w:                           # two submissions: both buffer sets
        for c in cases:
            w.submit(os.path.join(root, "case3d", "writer"), **c)
    results.save_maps_device(*maps(os.path.join(root, "maps", "direct")))
    with results.MapsWriter() as w:
        w.submit(*maps(os.path.join(root, "maps", "writer")))
        w.submit(*maps(os.path.join(root, "maps", "writer2")))
    for k, (d, (H, W), N, ign, kw) in enumerate(CALLS2D):
        results2d.save_images_device(os.path.join(root, "2d", d), **batch2d("img", 2, N, H, W, 500 + 10 * k, ign), **kw)
    for tag, kw in (("writer_plain", {}), ("writer_p3", LZW[2]), ("writer_p2_rps7", dict(LZW[1], tiff_rows_per_strip=7))):
        with results2d.ResultsWriter2D(**kw) as w:
            for j, (H, W) in enumerate((SMALL, LARGE, SMALL)):
                w.submit(os.path.join(root, "2d", tag), **batch2d(f"sub{j}", 2, 2, H, W, 700 + j, j != 1))
    dev = torch.device("cuda")
    arrays, hints = _gzip_tensors()
    for i, b in enumerate(gz.gzip_encode([torch.from_numpy(a).to(dev) for a in arrays], hints)):
        extra[f"gzip_encode/{i}"] = b
    masks = [batch2d("m", 1, 1, H, W, 800 + i, True) for i, (H, W) in enumerate((SMALL, LARGE, (5, 3)))]
    for i, b in enumerate(results2d.png_encode([torch.from_numpy(m["pred_masks"][0, 0]).to(dev) for m in masks],
                                               [None if i == 1 else m["ignore_index_map"][0] for i, m in enumerate(masks)])):
        extra[f"png_encode/{i}"] = b
    # the C ABI: one vx_gzip_encode call whose members start at 0, 1, 2, 3 mod 4
    srcs = [torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(dev) for a in arrays[1:]] + \
           [torch.from_numpy(np.frombuffer(_mixed((9, 13), 403).tobytes(), np.uint8).copy()).to(dev)]
    offs, off = [], 0
    for r, s in enumerate(srcs):
        off += (r - off) % 4
        offs.append(off)
        off += gz.bound(s.numel())
    assert [o % 4 for o in offs] == [0, 1, 2, 3]
    dst = torch.zeros(off, dtype=torch.uint8, device=dev)
    sizes = torch.empty(len(srcs), dtype=torch.int64, device=dev)
    ws = torch.empty(gz.workspace_bytes([s.numel() for s in srcs]), dtype=torch.uint8, device=dev)
    gz.encode_into([(_lib.ptr(s), s.numel(), o, None) for s, o in zip(srcs, offs)], dst, sizes, ws)
    host = dst.cpu().numpy()
    for i, (o, n) in enumerate(zip(offs, sizes.cpu().tolist())):
        extra[f"abi_gzip/{i}"] = host[o:o + n].tobytes()
    out = {k: hashlib.sha256(v).hexdigest() for k, v in extra.items()}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root).replace(os.sep, "/")] = hashlib.sha256(fh.read()).hexdigest()
    return dict(sorted(out.items()))


def png_stream_residues(root):
    """{stream offset mod 4} over the PNG files of every 2D call: file i of a call starts 63 i + the streams before it
    behind the call's first byte, its DEFLATE stream 43 bytes further"""
    from values_amd.results2d import plan_images
    seen = set()
    for d, (H, W), N, _, _ in CALLS2D:
        off = 0
        for f in plan_images(["img_0", "img_1"], N, ()):
            seen.add((off + 43) % 4)
            off += os.path.getsize(os.path.join(root, "2d", d, f.path))
    return seen
