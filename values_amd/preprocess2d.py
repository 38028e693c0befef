"""Preprocessing of the GTA / Cityscapes 2D data sets (the reference's
datasets/gta_cityscapes/preprocess_gta_cityscapes.py:47-182): every raw image is centre-cropped to 1024 x 1912 and shrunk
to a quarter (256 x 478) with cv2.resize(INTER_LINEAR), its label file cropped the same way and shrunk with INTER_NEAREST,
the labels turned into train ids (Cityscapes: label ids through id2trainId; GTA: colours through color2trainId, int64)
and into a colour image, and all of it stored as

    <save_dir>/preprocessed/images/<id>.npy       uint8 (256, 478, 3) RGB
    <save_dir>/preprocessed/images/vis/<id>.png   the same pixels
    <save_dir>/preprocessed/labels/<id>.npy       train ids: uint8 (cityscapes) / int64 (gta), (256, 478)
    <save_dir>/preprocessed/labels/vis/<id>.png   the colour image of the labels

-- the files HRNet's data set, the 2D TTA views, results2d, the gta.py hooks and the 2D metrics stand on.

Two routes to the same files.  The host mirror (center_crop_box, resize_linear_u8, resize_nearest, preprocess_image,
preprocess_dataset_2d(device_io=False)) is numpy and needs no device.  The device route (Preprocess2DReader,
preprocess_images_device, preprocess_dataset_2d(device_io=True)) decodes a batch of PNG files on the device
(vx_inflate, vx_png_unfilter; a palette file is one bpp = 1 image of indices), runs ONE vx_crop_resize_batched call over
all images and labels of the batch (preprocess2d.hip), ONE vx_png_encode_rgb call for both vis/ sets, and
brings the batch down in one pinned buffer that the writer pool turns into files while the next batch decodes.

What is restated and not observed here -- **parity unpinned**:
  * OpenCV is absent.  cv2.resize on uint8 is derived from its published source: at fx = fy = 1 / k with k
    even, INTER_LINEAR's source coordinate of output d is k d + k/2 - 1/2, two taps of weight exactly 1/2 per axis, and
    the 11-bit fixed-point arithmetic reduces to (p00 + p01 + p10 + p11 + 2) >> 2; INTER_NEAREST reads (k y, k x); the
    output size is size / k rounded half to even.
  * albumentations is absent.  A.CenterCrop(1024, 1912) is restated: y0 = (H - 1024) // 2, x0 = (W - 1912) // 2, and an
    image smaller than the crop raises ValueError.
  * The byte stream OpenCV gives the PNGs (decoded content is the contract, as for row f1 of DESIGN section 7), and the
    GTA5 label files' format (handled as 8-bit palette PNGs as well as RGB / RGBA ones).
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib, gta
from ._devio import PipelinedWriter, Stages, align, gather
from .image_io import png_color_type, png_parse, png_parse_indexed, read_png_any, write_png
from .images import ImageReader, _decode_png
from .preprocess import _File, npy_header
from .results2d import _lut as _palette

CROP = (1024, 1912)     # A.CenterCrop(height=1024, width=1912)
FACTOR = 4              # fx = fy = 0.25
SKIPPED = ("15188.png", "17705.png")
# cityscapes_labels.id2trainId for the ids 0..38 (tests/golden/cityscapes_id_tables.json holds it against the reference);
# its keys -1 and -2 never match a uint8
ID2TRAINID = (255, 255, 255, 255, 255, 255, 255, 0, 1, 255, 255, 2, 3, 4, 255, 255, 255, 5, 255, 6, 7, 8, 9, 10, 11, 12, 13,
              14, 15, 255, 255, 16, 17, 18, 19, 20, 21, 22, 23)


# ---------------------------------------------------------------------------------------------
# The host mirror

def center_crop_box(h: int, w: int, crop=CROP):
    """-> (y0, x0, crop_h, crop_w) of A.CenterCrop(*crop) on an (h, w) image (restated, parity unpinned): the box starts at
    ((h - crop_h) // 2, (w - crop_w) // 2); an image smaller than the crop raises ValueError."""
    ch, cw = int(crop[0]), int(crop[1])
    if ch < 1 or cw < 1:
        raise ValueError(f"center_crop_box: crop {crop}")
    if h < ch or w < cw:
        raise ValueError(f"Requested crop size ({ch}, {cw}) is larger than the image size ({h}, {w})")
    return (h - ch) // 2, (w - cw) // 2, ch, cw


def out_size(size: int, factor: int = FACTOR) -> int:
    """size / factor rounded half to even on the exact quotient: cv2.resize's saturate_cast<int>(size * fx)"""
    if factor < 1 or factor % 2:
        raise ValueError(f"factor {factor}: a positive even integer")
    q, r = divmod(int(size), factor)
    if 2 * r != factor:
        return q + (2 * r > factor)
    return q + (q & 1)


def resize_linear_u8(img: np.ndarray, factor: int = FACTOR) -> np.ndarray:
    """cv2.resize(img, (0, 0), fx=1/factor, fy=1/factor, interpolation=INTER_LINEAR) on a uint8 (H, W) or (H, W, C)
    array, for an even factor (derived from OpenCV's source, parity unpinned): the taps factor * d + factor/2 - 1 and
    factor * d + factor/2 on each axis, the second clamped to the last row / column, (sum of the four + 2) >> 2."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError("resize_linear_u8: a uint8 (H, W) or (H, W, C) array expected")
    oh, ow = out_size(a.shape[0], factor), out_size(a.shape[1], factor)
    ya = factor * np.arange(oh) + factor // 2 - 1
    xa = factor * np.arange(ow) + factor // 2 - 1
    yb, xb = np.minimum(ya + 1, a.shape[0] - 1), np.minimum(xa + 1, a.shape[1] - 1)
    s = a.astype(np.int32)
    total = s[ya][:, xa] + s[ya][:, xb] + s[yb][:, xa] + s[yb][:, xb]
    return np.ascontiguousarray(((total + 2) >> 2).astype(np.uint8))   # (C order, as cv2 returns it and np.save stores it)


def resize_nearest(img: np.ndarray, factor: int = FACTOR) -> np.ndarray:
    """cv2.resize(..., interpolation=INTER_NEAREST) at fx = fy = 1 / factor: source pixel min(floor(d * factor), size - 1)"""
    a = np.asarray(img)
    if a.ndim not in (2, 3):
        raise ValueError("resize_nearest: an (H, W) or (H, W, C) array expected")
    oh, ow = out_size(a.shape[0], factor), out_size(a.shape[1], factor)
    ys = np.minimum(factor * np.arange(oh), a.shape[0] - 1)
    xs = np.minimum(factor * np.arange(ow), a.shape[1] - 1)
    return np.ascontiguousarray(a[ys][:, xs])


def id_to_trainid_lut() -> np.ndarray:
    """(256,) uint8: the reference's loop `mask_train_indices[mask_labels == id] = trainId` over id2trainId as one table
    (the loop reads the untouched copy); an id without an entry keeps its value"""
    lut = np.arange(256, dtype=np.uint8)
    lut[:len(ID2TRAINID)] = ID2TRAINID
    return lut


def trainid_to_color_lut() -> np.ndarray:
    """(256, 3) uint8: the reference's loop `mask_color[mask_train_indices == trainId] = color` over trainId2color as one
    table -- results2d's palette; a value that is no train id stays black"""
    return _palette()


def preprocess_image(image, mask, dataset: str, crop=CROP, factor: int = FACTOR, name: str = ""):
    """The reference's loop body (:128-174) on the arrays read_png_any returns -> (image_u8 (oh, ow, 3) RGB, train_ids
    (oh, ow): uint8 for "cityscapes", int64 else, mask_color (oh, ow, 3) RGB).  image: (H, W, 3 | 4), alpha dropped as
    cv2.cvtColor(BGR2RGB) drops it; mask: grey label ids (cityscapes) or the colour label image (H, W, 3 | 4).  An unknown
    colour raises the reference's AssertionError, naming `name`."""
    image, mask = np.asarray(image), np.asarray(mask)
    if image.ndim != 3 or image.shape[2] not in (3, 4) or image.dtype != np.uint8:
        raise ValueError(f"{name}: a uint8 RGB / RGBA image expected, got {image.dtype} {image.shape}")
    if image.shape[:2] != mask.shape[:2]:
        raise ValueError(f"{name}: image {image.shape[:2]} and mask {mask.shape[:2]} differ in resolution")
    y0, x0, ch, cw = center_crop_box(image.shape[0], image.shape[1], crop)
    image = resize_linear_u8(image[y0:y0 + ch, x0:x0 + cw, :3], factor)
    mask = mask[y0:y0 + ch, x0:x0 + cw]
    if dataset == "cityscapes":
        if mask.ndim != 2:
            raise ValueError(f"{name}: grey label ids expected, got an array of shape {mask.shape}")
        train_ids = id_to_trainid_lut()[resize_nearest(mask.astype(np.uint8), factor)]
        return image, train_ids, trainid_to_color_lut()[train_ids]
    if mask.ndim != 3 or mask.shape[2] not in (3, 4):
        raise ValueError(f"{name}: a colour label image expected, got an array of shape {mask.shape}")
    mask_color = resize_nearest(mask[..., :3].astype(np.uint8), factor)
    train_ids = gta.rgb_to_trainid_host(mask_color)
    assert gta.UNKNOWN not in train_ids, f"Unknown color value in mask for image {name}!"
    return image, train_ids, mask_color


# ---------------------------------------------------------------------------------------------
# The listing

def _png_files(d):
    """batchgenerators' subfiles(d, suffix=".png", join=False): sorted; then without the mac "._" files"""
    return [f for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f)) and f.endswith(".png") and not f.startswith(".")]


def _out_paths(root, image_id):
    return (os.path.join(root, "images", f"{image_id}.npy"), os.path.join(root, "images", "vis", f"{image_id}.png"),
            os.path.join(root, "labels", f"{image_id}.npy"), os.path.join(root, "labels", "vis", f"{image_id}.png"))


def list_cases(dataset_dir, save_dir, dataset: str):
    """The cases the reference's loops would read, in its order: [(image_id, image_name, image_path, label_path)].  Left
    out before anything is read: a case whose four outputs all exist, and 15188.png / 17705.png."""
    dataset_dir, root = str(dataset_dir), os.path.join(str(save_dir), "preprocessed")
    if dataset == "cityscapes":
        image_dirs, label_dirs = [], []
        for split in ("train", "val"):
            split_images = os.path.join(dataset_dir, "images", "leftImg8bit", split)
            for city in os.listdir(split_images):
                if os.path.isdir(os.path.join(split_images, city)):
                    image_dirs.append(os.path.join(split_images, city))
                    label_dirs.append(os.path.join(dataset_dir, "labels", "gtFine", split, city))
        image_dirs, label_dirs = sorted(image_dirs), sorted(label_dirs)
    else:
        image_dirs, label_dirs = [os.path.join(dataset_dir, "images")], [os.path.join(dataset_dir, "labels")]
    cases = []
    for image_dir, label_dir in zip(image_dirs, label_dirs):
        for name in _png_files(image_dir):
            image_id = name.split("_leftImg8bit")[0] if dataset == "cityscapes" else name.split(".")[0]
            if all(os.path.isfile(p) for p in _out_paths(root, image_id)) or name in SKIPPED:
                continue
            label = f"{image_id}_gtFine_labelIds.png" if dataset == "cityscapes" else name
            cases.append((image_id, name, os.path.join(image_dir, name), os.path.join(label_dir, label)))
    return cases


def _different(name):
    print(f"Different resolutions between image and mask for {name}!")


# ---------------------------------------------------------------------------------------------
# The device route

_tables = {}


def _device_tables(dev):
    """-> (vx_p2d_tables, the tensors it points into) for the device, made once"""
    import torch
    k = dev.index if dev.index is not None else torch.cuda.current_device()
    if k not in _tables:
        keep = (torch.from_numpy(id_to_trainid_lut()).to(dev), torch.from_numpy(trainid_to_color_lut()).to(dev),
                torch.from_numpy(gta._table().view(np.int32)).to(dev))
        t = _lib.P2dTables()
        t.id2trainid, t.trainid2color, t.color2trainid = (x.data_ptr() for x in keep)
        t.n_color, t.default_id = int(keep[2].shape[0]), gta.UNKNOWN
        _tables[k] = (t, keep)
    return _tables[k][0]


def _parse_any(name, raw):
    """-> ((w, h, ctype, bpp, IDAT spans), palette or None): a palette file is a bpp = 1 image of indices"""
    try:
        if png_color_type(raw) == 3:
            w, h, palette, spans = png_parse_indexed(raw)
            return (w, h, 3, 1, spans), palette
        return png_parse(raw), None
    except ValueError as e:
        raise ValueError(f"{name}: {e}") from None


class Preprocess2DReader(ImageReader):
    """Pipelined decode of (image, label) PNG pairs: a batch is a list of (image_path, label_path); read(batches) yields
    per batch one entry per pair -- (image tensor, label tensor, image palette, label palette), the tensors on the device
    as images.load_png_device returns them except that a palette file comes as its (H, W) index image with its (256, 3)
    uint8 palette (a host array; None for the other files) -- or None for a pair whose image and label differ in
    resolution: that is read from the files' headers, and such a pair is not decoded.  The files of batch i + 1 are read
    from disk while batch i is decoded."""

    def _submit(self, batch):
        return super()._submit([p for pair in batch for p in pair])

    def _decode(self, names, raws, device):
        parsed = [_parse_any(nm, r) for nm, r in zip(names, raws)]
        same = [parsed[k][0][:2] == parsed[k + 1][0][:2] for k in range(0, len(names), 2)]
        sel = [k for k in range(len(names)) if same[k // 2]]
        outs = iter(_decode_png([names[k] for k in sel], [raws[k] for k in sel], device, self._staging, self._timing,
                                heads=[parsed[k][0] for k in sel]) if sel else [])
        return [(next(outs), next(outs), parsed[2 * c][1], parsed[2 * c + 1][1]) if ok else None for c, ok in enumerate(same)]


def _plan_batch(decoded, dataset, crop, factor, dev, bufs=None):
    """decoded: Preprocess2DReader's entries of one batch (no None) -> (the vx_p2d_item table: image and label of case c
    are items 2 c and 2 c + 1; the arena; [(image, train_ids, mask_color)] views of it; [(offset, bytes)] three per
    case; the palettes on the device).  Nothing is launched."""
    import torch
    cityscapes = dataset == "cityscapes"
    pals = [p for d in decoded for p in d[2:] if p is not None]
    pal_dev = torch.from_numpy(np.stack(pals)).to(dev) if pals else None
    arr = (_lib.P2dItem * max(2 * len(decoded), 1))()
    spans, off, npal, shapes = [], 0, 0, []
    for c, (img, lab, ipal, lpal) in enumerate(decoded):
        if cityscapes and (lab.dim() != 2 or lpal is not None):
            raise ValueError("preprocess2d: the label file of a cityscapes case is a grey image of label ids")
        h, w = int(img.shape[0]), int(img.shape[1])
        y0, x0, ch, cw = center_crop_box(h, w, crop)
        oh, ow = out_size(ch, factor), out_size(cw, factor)
        shapes.append((oh, ow))
        for j, (t, pal) in enumerate(((img, ipal), (lab, lpal))):
            it = arr[2 * c + j]
            it.src, it.H, it.W, it.bpp = t.data_ptr(), h, w, (1 if t.dim() == 2 else int(t.shape[2]))
            if pal is not None:
                it.palette = pal_dev[npal].data_ptr()
                npal += 1
            it.y0, it.x0, it.crop_h, it.crop_w, it.factor = y0, x0, ch, cw, factor
            it.mode = _lib.VX_P2D_IMAGE if j == 0 else (_lib.VX_P2D_LABEL_IDS if cityscapes else _lib.VX_P2D_LABEL_COLOR)
        for nbytes in (3 * oh * ow, (1 if cityscapes else 8) * oh * ow, 3 * oh * ow):
            spans.append((off, nbytes))
            off += align(nbytes)
    arena = torch.empty(off, dtype=torch.uint8, device=dev) if bufs is None else bufs.get("p2d", off, dev)
    outs = []
    for c, (oh, ow) in enumerate(shapes):
        (o0, n0), (o1, n1), (o2, n2) = spans[3 * c:3 * c + 3]
        image = arena[o0:o0 + n0].view(oh, ow, 3)
        ids = arena[o1:o1 + n1].view(oh, ow) if cityscapes else arena[o1:o1 + n1].view(torch.int64).view(oh, ow)
        color = arena[o2:o2 + n2].view(oh, ow, 3)
        outs.append((image, ids, color))
        arr[2 * c].out_rgb = image.data_ptr()
        arr[2 * c + 1].out_rgb, arr[2 * c + 1].out_ids = color.data_ptr(), ids.data_ptr()
    return arr, arena, outs, spans, pal_dev


def _crop_resize_call(arr, n, status, dev):
    """one vx_crop_resize_batched call over the first n items of the table; status: int32 device tensor, one per item"""
    lib, tables = _lib.load(), _device_tables(dev)
    need = int(lib.vx_crop_resize_batched_workspace_bytes(arr, n, tables))
    ws = _lib.workspace(dev, need)   # (need = 0: refused, the call names the reason)
    _lib.check(lib.vx_crop_resize_batched(arr, n, tables, _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "vx_crop_resize_batched")


def _batch(decoded, dataset, crop, factor, dev, bufs=None, status=None):
    """_plan_batch and the call -> (arena, outs, spans, status, palettes); nothing is waited for"""
    import torch
    arr, arena, outs, spans, pal_dev = _plan_batch(decoded, dataset, crop, factor, dev, bufs)
    n = 2 * len(decoded)
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    if n:
        _crop_resize_call(arr, n, status, dev)
    return arena, outs, spans, status, pal_dev


def _check_unknown(status, names):
    """status: the host list of a batch; names: the image names of its cases.  The reference's assert (:172-174)."""
    for c, name in enumerate(names):
        assert status[2 * c + 1] == 0, f"Unknown color value in mask for image {name}!"


def preprocess_images_device(image_paths, label_paths, dataset: str, crop=CROP, factor: int = FACTOR, device=None,
                             batch: int = 8):
    """-> [(image, train_ids, mask_color)] device tensors for the (image, label) PNG pairs, what preprocess_image gives
    for the decoded files; nothing is written.  The 2D counterpart of preprocess.preprocess_batch_device: `image` (oh, ow,
    3) uint8 goes to data.tta_views_2d_device as it is.  The tensors of a batch are views of one device buffer.  A pair
    whose resolutions differ raises ValueError, an unknown label colour the reference's AssertionError."""
    _lib.require_gpu()
    pairs = list(zip([str(p) for p in image_paths], [str(p) for p in label_paths]))
    if batch < 1:
        raise ValueError("preprocess_images_device: batch >= 1")
    groups = [pairs[b:b + batch] for b in range(0, len(pairs), batch)]
    out = []
    with Preprocess2DReader(device=device) as reader:
        for g, res in zip(groups, reader.read(groups)):
            for (ip, _), r in zip(g, res):
                if r is None:
                    raise ValueError(f"{ip}: image and mask differ in resolution")
            _, outs, _, status, _ = _batch(res, dataset, crop, factor, res[0][0].device)
            if dataset != "cityscapes":
                _check_unknown(status.cpu().tolist(), [os.path.basename(ip) for ip, _ in g])
            out.extend(outs)
    return out


def _encode_batch(bufs, cases, decoded, dataset, crop, factor, timing=None):
    """One batch on the device: vx_crop_resize_batched over its images and labels, vx_png_encode_rgb over both vis/ sets,
    one small read (the PNG files' places and the labels' counts of unknown colours), then the arrays and the PNG bytes
    into the buffer set's pinned host buffer -> (plan, host, spans) for _devio.emit."""
    import torch
    from .results2d import _png_rgb_launch, _png_rgb_table
    dev = decoded[0][0].device
    n_png, n_items = 2 * len(decoded), 2 * len(decoded)
    place = bufs.get("place", 16 * n_png + 4 * n_items, dev)[:16 * n_png + 4 * n_items]
    stages = Stages(timing)
    stages.mark()
    arena, outs, spans, _, keep = _batch(decoded, dataset, crop, factor, dev, bufs, place[16 * n_png:].view(torch.int32))
    stages.mark()
    entries = [(t.data_ptr(), int(t.shape[0]), int(t.shape[1])) for image, _, color in outs for t in (image, color)]
    items, bound, ws_bytes = _png_rgb_table(entries)
    dst = bufs.get("png", bound, dev)
    _png_rgb_launch(items, dst, place[:16 * n_png].view(torch.int64), bufs.get("png_ws", ws_bytes, dev))
    stages.mark()
    host_place = place.cpu()                 # the one small read: synchronises the stream
    if dataset != "cityscapes":
        _check_unknown(host_place[16 * n_png:].view(torch.int32).tolist(), [name for _, name in cases])
    pl = host_place[:16 * n_png].view(torch.int64).tolist()
    offs, sizes = pl[:n_png], pl[n_png:]
    n_arena = spans[-1][0] + spans[-1][1]
    host, (a0, p0) = gather(bufs, [(arena, n_arena), (dst, offs[-1] + sizes[-1])], dev)
    stages.add(("crop_resize_ms", "png_encode_ms"), {"png_bytes": offs[-1] + sizes[-1], "array_bytes": sum(n for _, n in spans)})
    plan, out = [], []
    for c, ((image_id, _), (image, ids, _)) in enumerate(zip(cases, outs)):
        (o0, n0), (o1, n1), _ = spans[3 * c:3 * c + 3]
        plan += [_File(os.path.join("images", f"{image_id}.npy")), _File(os.path.join("images", "vis", f"{image_id}.png")),
                 _File(os.path.join("labels", f"{image_id}.npy")), _File(os.path.join("labels", "vis", f"{image_id}.png"))]
        out += [(a0 + o0, n0, npy_header(image.shape, "uint8"), b""), (p0 + offs[2 * c], sizes[2 * c]),
                (a0 + o1, n1, npy_header(ids.shape, str(ids.dtype).replace("torch.", "")), b""),
                (p0 + offs[2 * c + 1], sizes[2 * c + 1])]
    return plan, host, out


class _Writer2D(PipelinedWriter):
    _encode = staticmethod(_encode_batch)
    _dirs = ("images", os.path.join("images", "vis"), "labels", os.path.join("labels", "vis"))

    def submit(self, root, cases, decoded, dataset, crop, factor, _timing=None):
        self._submit(root, cases, decoded, dataset, crop, factor, _timing)


# ---------------------------------------------------------------------------------------------
# The data set

def preprocess_dataset_2d(dataset_dir, save_dir, dataset: str, device_io: bool = False, batch: int = 8, crop=CROP,
                          factor: int = FACTOR, _timing=None) -> int:
    """The reference's preprocess_dataset (preprocess_gta_cityscapes.py:47-182; this package's preprocess_dataset is the
    3D step).  dataset "cityscapes": every images/leftImg8bit/{train,val}/<city>/<id>_leftImg8bit.png with
    labels/gtFine/{train,val}/<city>/<id>_gtFine_labelIds.png; any other value: images/<id>.png with labels/<id>.png
    (the GTA5 layout).  Writes the four files of the module docstring per case under <save_dir>/preprocessed and returns
    the number of cases left out because image and mask differ in resolution (the reference only counts them).
    device_io=False: the host mirror.  device_io=True: Preprocess2DReader batches of `batch` cases, per batch one
    vx_crop_resize_batched call, one vx_png_encode_rgb call and one pinned buffer of results, written on the writer pool
    while the next batch decodes; it raises without the library or a GPU.  A batch costs the inflate of its largest file
    (vx_inflate decodes one stream per wavefront), whatever its size: measured, batch=8 is slower than the host mirror and
    batch=128 about twice as fast -- give the device route large batches.  Either way the .npy files are byte-identical
    and start with the bytes np.save writes, and the PNG files decode to the same pixels."""
    if batch < 1:
        raise ValueError("preprocess_dataset_2d: batch >= 1")
    out_size(crop[0], factor), out_size(crop[1], factor)   # refuses a bad factor before anything is created
    if device_io:
        _lib.require_gpu()
    root = os.path.join(str(save_dir), "preprocessed")
    for d in _Writer2D._dirs:
        os.makedirs(os.path.join(root, d), exist_ok=True)
    cases = list_cases(dataset_dir, save_dir, dataset)
    num_diff_res = 0
    if not device_io:
        for image_id, name, image_path, label_path in cases:
            image, mask = read_png_any(image_path), read_png_any(label_path)
            if image.shape[:2] != mask.shape[:2]:
                num_diff_res += 1
                _different(name)
                continue
            image, train_ids, mask_color = preprocess_image(image, mask, dataset, crop, factor, name)
            image_npy, image_png, mask_npy, mask_png = _out_paths(root, image_id)
            np.save(image_npy, image)
            write_png(image_png, image)
            np.save(mask_npy, train_ids)
            write_png(mask_png, mask_color)
        return num_diff_res
    groups = [cases[b:b + batch] for b in range(0, len(cases), batch)]
    with Preprocess2DReader(_timing=_timing) as reader, _Writer2D() as writer:
        for g, res in zip(groups, reader.read([[(ip, lp) for _, _, ip, lp in g] for g in groups])):
            kept = [(case, r) for case, r in zip(g, res) if r is not None]
            for case, r in zip(g, res):
                if r is None:
                    num_diff_res += 1
                    _different(case[1])
            if kept:
                writer.submit(root, [(case[0], case[1]) for case, _ in kept], [r for _, r in kept], dataset, crop, factor, _timing)
    return num_diff_res
