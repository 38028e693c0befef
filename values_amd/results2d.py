"""2D results directory (Tester.create_save_dirs / save_prediction / save_uncertainty, test_2D.py:75-89, 116-159):

    <save_dir>/pred_seg/<image_id>_mean.png, <image_id>_NN.png     colour arg-max masks (NN = 01.. per prediction)
    <save_dir>/<unc_type>/<image_id>.tif                           float32 uncertainty maps

The label -> colour table is the Cityscapes train-id palette extended by the five "_2" shift classes of the
GTA/Cityscapes setup (uncertainty_modeling/data/cityscapes_labels.py:59-102, trainId2color; 255 = unlabeled = black).
Arg-max and colour lookup run on the device (vx_unc_reduce's sample_argmax, vx_colorize_u8); the files are written
with values_amd.image_io.

save_images_device / ResultsWriter2D write the same tree from the device: one vx_png_encode call builds every PNG file of a
batch (colour lookup, scanlines, DEFLATE, zlib and PNG framing) and the host only copies the finished bytes back.

The uncertainty maps are uncompressed single-strip TIFFs by default.  With compression="lzw" (save_uncertainty) /
tiff="lzw" (save_images_device, ResultsWriter2D) they are LZW strip TIFFs with Predictor 1, 2 or 3 -- the file libtiff
writes for cv2.imwrite, read by image_io.read_tiff_f32, images.load_tiff_device, PIL and OpenCV alike -- and the device
writers compress them on the GPU (vx_tiff_predict, vx_tiff_lzw_encode, vx_tiff_lzw_pack): only the compressed bytes
come back.  Host and device writers produce the same bytes.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _devio, _lib
from .image_io import write_png, write_tiff_f32

UNLABELED = 255  # cs_labels.name2trainId["unlabeled"]
TRAINID2COLOR = {
    0: (128, 64, 128), 1: (244, 35, 232), 2: (70, 70, 70), 3: (102, 102, 156), 4: (190, 153, 153), 5: (153, 153, 153),
    6: (250, 170, 30), 7: (220, 220, 0), 8: (107, 142, 35), 9: (152, 251, 152), 10: (70, 130, 180), 11: (220, 20, 60),
    12: (255, 0, 0), 13: (0, 0, 142), 14: (0, 0, 70), 15: (0, 60, 100), 16: (0, 80, 100), 17: (0, 0, 230),
    18: (119, 11, 32), 19: (46, 247, 180), 20: (167, 242, 242), 21: (30, 193, 252), 22: (242, 160, 19), 23: (84, 86, 22),
    255: (0, 0, 0),
}


def _lut() -> np.ndarray:
    lut = np.zeros((256, 3), dtype=np.uint8)
    for k, v in TRAINID2COLOR.items():
        lut[k] = v
    return lut


def colorize(labels: torch.Tensor, ignore_index_map=None) -> torch.Tensor:
    """labels (..., H, W) uint8 on the device -> (..., H, W, 3) uint8 RGB; pixels of the ignore map become unlabeled."""
    _lib.require_gpu()
    lib = _lib.load()
    lab = labels.to(torch.uint8).contiguous()
    dev = lab.device
    lut = torch.from_numpy(_lut()).to(dev)
    ign = None
    if ignore_index_map is not None:
        ign = torch.as_tensor(np.asarray(ignore_index_map) if not isinstance(ignore_index_map, torch.Tensor) else ignore_index_map)
        ign = (ign != 0).to(device=dev, dtype=torch.uint8).expand_as(lab).contiguous()
    out = torch.empty(tuple(lab.shape) + (3,), dtype=torch.uint8, device=dev)
    _lib.check(lib.vx_colorize_u8(lab.data_ptr(), None if ign is None else ign.data_ptr(), lab.numel(), lut.data_ptr(), UNLABELED,
                                  out.data_ptr(), _lib.stream_ptr()), "vx_colorize_u8")
    return out


def create_save_dirs(save_root_dir: str, exp_name: str, version, test_split: str) -> Dict[str, str]:
    save_dir = os.path.join(save_root_dir, exp_name, "test_results", str(version), test_split)
    pred = os.path.join(save_dir, "pred_seg")
    os.makedirs(pred, exist_ok=True)
    return {"save_dir": save_dir, "save_pred_dir": pred, "save_pred_prob_dir": os.path.join(save_dir, "pred_prob")}


def save_prediction(save_pred_dir: str, image_id: str, pred_masks: torch.Tensor, mean_mask: Optional[torch.Tensor],
                    ignore_index_map=None) -> None:
    """pred_masks (Npred, H, W) uint8 = arg-max of each prediction, mean_mask (H, W) = arg-max of the mean prediction.
    File names as test_2D.py:136-141: with several predictions `<id>_mean.png` then `<id>_01.png`...; with one, `<id>_01.png`."""
    n = pred_masks.shape[0]
    if n > 1:
        stack = torch.cat([mean_mask.unsqueeze(0).to(pred_masks.device), pred_masks], 0)
        names = [f"{image_id}_mean"] + [f"{image_id}_{str(i).zfill(2)}" for i in range(1, n + 1)]
    else:
        stack, names = pred_masks, [f"{image_id}_01"]
    rgb = colorize(stack, ignore_index_map).cpu().numpy()
    for img, name in zip(rgb, names):
        write_png(os.path.join(save_pred_dir, f"{name}.png"), img)


def save_uncertainty(save_dir: str, image_id: str, uncertainty_dict: Dict[str, torch.Tensor], compression=None, predictor: int = 3,
                     rows_per_strip=None) -> None:
    """test_2D.py:151-158: one float32 TIFF per uncertainty type.  compression, predictor, rows_per_strip: as
    image_io.write_tiff_f32 takes them (None: uncompressed; "lzw": what the reference's cv2.imwrite writes)."""
    for unc_type, unc_map in uncertainty_dict.items():
        d = os.path.join(save_dir, unc_type)
        os.makedirs(d, exist_ok=True)
        m = unc_map.detach().cpu().numpy() if isinstance(unc_map, torch.Tensor) else np.asarray(unc_map)
        write_tiff_f32(os.path.join(d, f"{image_id}.tif"), m.astype(np.float32), compression, predictor, rows_per_strip)


def save_results_dict(save_dir: str, results_dict: Dict[str, Dict]) -> Dict[str, Dict]:
    """Tester.save_results_dict (test_2D.py:258-271): <save_dir>/metrics.json with one {"dataset": ..., "metrics": {...}}
    entry per image id (values_amd.metrics.process_metrics_2d gives the metrics) plus "mean": {"metrics": {...}}, the plain
    mean of every metric over the images that carry it; indent=2.  Returns the written dict (the argument is left as it
    was).  This is the file evalmetrics.get_dice / failure_detection read."""
    scores: Dict[str, List[float]] = {}
    for image_id, value in results_dict.items():
        for metric, score in value["metrics"].items():
            scores.setdefault(metric, []).append(score)
    full = dict(results_dict)
    full["mean"] = {"metrics": {metric: float(np.asarray(v).mean()) for metric, v in scores.items()}}
    os.makedirs(save_dir, exist_ok=True)
    with open(os.path.join(save_dir, "metrics.json"), "w") as f:
        json.dump(full, f, indent=2)
    return full


# ---------------------------------------------------------------------------------------------------------------------
# device results writer (2D)

class PlannedImage(NamedTuple):
    """One file of the 2D results tree: path relative to save_dir, kind ("png" / "tif") and source: ("mean", b),
    ("pred", b, t) with t 0-based, or ("unc", name, b)."""
    path: str
    kind: str
    source: tuple


def plan_images(image_ids: Sequence[str], n_pred: int, unc_types: Sequence[str]) -> List[PlannedImage]:
    """The files save_prediction(<save_dir>/pred_seg, ...) and save_uncertainty(<save_dir>, ...) write for each image, in
    that order: `<id>_mean.png` then `<id>_01.png`... with several predictions, `<id>_01.png` alone with one; then
    `<unc_type>/<id>.tif` per uncertainty type."""
    out = []
    for b, iid in enumerate(image_ids):
        if n_pred > 1:
            out.append(PlannedImage(os.path.join("pred_seg", f"{iid}_mean.png"), "png", ("mean", b)))
        for t in range(n_pred):
            out.append(PlannedImage(os.path.join("pred_seg", f"{iid}_{str(t + 1).zfill(2)}.png"), "png", ("pred", b, t)))
        for name in unc_types:
            out.append(PlannedImage(os.path.join(name, f"{iid}.tif"), "tif", ("unc", name, b)))
    return out


_luts: Dict[int, torch.Tensor] = {}


def _device_lut(dev) -> torch.Tensor:
    k = dev.index if dev.index is not None else torch.cuda.current_device()
    if k not in _luts:
        _luts[k] = torch.from_numpy(_lut()).to(dev)
    return _luts[k]


def _as_device(a, dev, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.detach().to(dev)
    return t if dtype is None else t.to(dtype)


def _png_table(entries):
    """the vx_png_item table of (labels_ptr, ignore_ptr or None, H, W) entries -> (table, sum of vx_png_bound, workspace bytes)"""
    lib = _lib.load()
    items = (_lib.PngItem * len(entries))()
    bound = 0
    for it, (lab, ig, H, W) in zip(items, entries):
        it.labels, it.ignore, it.H, it.W = lab, ig, H, W
        bound += int(lib.vx_png_bound(H, W))
    return items, bound, int(lib.vx_png_workspace_bytes(items, len(entries)))


def _png_launch(items, dst, place, ws):
    """vx_png_encode of a _png_table into dst (uint8); place (int64, two per item) receives the files' offsets, then their
    sizes; ws: the workspace.  All three are device tensors, freshly made or cut from a buffer set."""
    n = len(items)
    _lib.check(_lib.load().vx_png_encode(items, n, _device_lut(dst.device).data_ptr(), UNLABELED, dst.data_ptr(), dst.numel(),
                                         place.data_ptr(), place[n:].data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "vx_png_encode")


def png_encode(masks: Sequence[torch.Tensor], ignores: Optional[Sequence] = None) -> List[bytes]:
    """One RGB PNG file per device (H, W) label mask, coloured like colorize (ignored pixels unlabeled), all in one
    vx_png_encode call; the shapes may differ.  ignores: per mask an (H, W) map or None."""
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    labs = [_as_device(m, dev, torch.uint8).contiguous() for m in masks]
    if not labs:
        return []
    igs = [None if g is None else (_as_device(g, dev) != 0).to(torch.uint8).contiguous() for g in (ignores or [None] * len(labs))]
    entries = []
    for lab, ig in zip(labs, igs):
        if lab.dim() != 2 or (ig is not None and ig.shape != lab.shape):
            raise ValueError("png_encode: (H, W) masks and ignore maps of the same shape expected")
        entries.append((lab.data_ptr(), None if ig is None else ig.data_ptr(), int(lab.shape[0]), int(lab.shape[1])))
    items, bound, ws_bytes = _png_table(entries)
    n = len(labs)
    dst = torch.empty(bound, dtype=torch.uint8, device=dev)
    place = torch.empty(2 * n, dtype=torch.int64, device=dev)
    _png_launch(items, dst, place, torch.empty(ws_bytes, dtype=torch.uint8, device=dev))
    pl = place.cpu().tolist()
    host = dst[:pl[n - 1] + pl[2 * n - 1]].cpu().numpy()
    return [host[o:o + k].tobytes() for o, k in zip(pl[:n], pl[n:])]


def _png_rgb_table(entries):
    """the vx_png_rgb_item table of (rgb_ptr, H, W) entries -> (table, sum of vx_png_bound, workspace bytes)"""
    lib = _lib.load()
    items = (_lib.PngRgbItem * len(entries))()
    bound = 0
    for it, (rgb, H, W) in zip(items, entries):
        it.rgb, it.H, it.W = rgb, H, W
        bound += int(lib.vx_png_bound(H, W))
    return items, bound, int(lib.vx_png_encode_rgb_workspace_bytes(items, len(entries)))


def _png_rgb_launch(items, dst, place, ws):
    """vx_png_encode_rgb of a _png_rgb_table: dst, place and ws as _png_launch takes them"""
    n = len(items)
    _lib.check(_lib.load().vx_png_encode_rgb(items, n, dst.data_ptr(), dst.numel(), place.data_ptr(), place[n:].data_ptr(),
                                             ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "vx_png_encode_rgb")


def png_encode_rgb(images: Sequence[torch.Tensor]) -> List[bytes]:
    """One RGB PNG file per (H, W, 3) uint8 image, all in one vx_png_encode_rgb call; the shapes may differ.  The files
    have png_encode's layout (filter-0 scanlines, one IDAT) and decode to the images' pixels."""
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    imgs = [_as_device(m, dev).contiguous() for m in images]
    if not imgs:
        return []
    for im in imgs:
        if im.dim() != 3 or im.shape[2] != 3 or im.dtype != torch.uint8:
            raise ValueError("png_encode_rgb: (H, W, 3) uint8 images expected")
    items, bound, ws_bytes = _png_rgb_table([(im.data_ptr(), int(im.shape[0]), int(im.shape[1])) for im in imgs])
    n = len(imgs)
    dst = torch.empty(bound, dtype=torch.uint8, device=dev)
    place = torch.empty(2 * n, dtype=torch.int64, device=dev)
    _png_rgb_launch(items, dst, place, torch.empty(ws_bytes, dtype=torch.uint8, device=dev))
    pl = place.cpu().tolist()
    host = dst[:pl[n - 1] + pl[2 * n - 1]].cpu().numpy()
    return [host[o:o + k].tobytes() for o, k in zip(pl[:n], pl[n:])]


def _encode_images(bufs, image_ids, pred_masks, mean_masks, uncertainty, ignore_index_map, timing=None, tiff=None,
                   tiff_predictor=3, tiff_rows_per_strip=None):
    """vx_png_encode over every mask of the batch, the TIFF stage over every map (_devio.TiffStage: raw, or LZW strips
    compressed on the device), one small read of the PNG files' places and sizes (and the strips' sizes) + one copy of the
    PNG bytes and one of the maps' bytes into pinned memory: -> (plan, host uint8 array, [(offset, size)] per planned PNG
    file, [(offset, size, head, tail)] per TIFF)."""
    ids = list(image_ids)
    shapes = [tuple(int(v) for v in np.shape(m)[1:]) for m in (uncertainty or {}).values()] * len(ids)   # the maps in plan order
    tif = _devio.TiffStage("save_images_device", shapes, tiff, tiff_predictor, tiff_rows_per_strip)   # refuses a bad option first
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    pm = _as_device(pred_masks, dev, torch.uint8)
    if pm.dim() != 4:
        raise ValueError(f"save_images_device: pred_masks (B, N, H, W) expected, got {tuple(pm.shape)}")
    B, N, H, W = (int(v) for v in pm.shape)
    if len(ids) != B:
        raise ValueError(f"save_images_device: {len(ids)} image ids for {B} images")
    pm = pm.contiguous()
    mm = None
    if N > 1:
        if mean_masks is None:
            raise ValueError("save_images_device: several predictions need mean_masks")
        mm = _as_device(mean_masks, dev, torch.uint8).reshape(B, H, W).contiguous()
    ign = None
    if ignore_index_map is not None:
        ign = (_as_device(ignore_index_map, dev) != 0).to(torch.uint8)
        ign = (ign.expand(B, H, W) if ign.dim() == 2 else ign.reshape(B, H, W)).contiguous()
    unc = {k: _as_device(v, dev, torch.float32) for k, v in (uncertainty or {}).items()}
    plan = plan_images(ids, N, list(unc))

    pngs = [f for f in plan if f.kind == "png"]
    entries = []
    for f in pngs:
        b = f.source[1]
        lab = mm[b] if f.source[0] == "mean" else pm[b, f.source[2]]
        entries.append((lab.data_ptr(), ign[b].data_ptr() if ign is not None else None, H, W))
    items, bound, ws_bytes = _png_table(entries)
    n = len(pngs)
    dst = bufs.get("png", bound, dev)
    # [PNG offsets | PNG sizes] int64, then the TIFF stage's
    place = bufs.get("place", 16 * n + tif.place_bytes, dev)[:16 * n + tif.place_bytes]
    ws = bufs.get("png_ws", ws_bytes, dev)
    stages = _devio.Stages(timing)
    stages.mark()
    _png_launch(items, dst, place[:16 * n].view(torch.int64), ws)
    stages.mark()
    region = tif.launch(bufs, [unc[k][b] for b in range(B) for k in unc], place[16 * n:], dev, stages)
    host_place = place.cpu()              # the one small read: synchronises the stream
    pl = host_place[:16 * n].view(torch.int64).tolist()
    offs, sizes = pl[:n], pl[n:]
    png_bytes = offs[-1] + sizes[-1]
    tif_bytes, parts = tif.finish(host_place[16 * n:])
    host, (png0, tif0) = _devio.gather(bufs, [(dst, png_bytes), (region, tif_bytes)], dev)
    stages.add(("encode_ms", None, "tiff_predict_ms", "tiff_encode_ms", "tiff_pack_ms"),
               {"raw_bytes": n * H * (3 * W + 1), "png_bytes": png_bytes, "tiff_raw_bytes": tif.raw_bytes, "tiff_bytes": tif_bytes})
    png_spans = iter([(png0 + o, k) for o, k in zip(offs, sizes)])
    tif_spans = iter([(tif0 + p[0],) + p[1:] for p in parts])
    return plan, host, [next(png_spans if f.kind == "png" else tif_spans) for f in plan]


def save_images_device(save_dir: str, image_ids: Sequence[str], pred_masks, mean_masks, uncertainty: Optional[Dict] = None,
                       ignore_index_map=None, _timing=None, tiff=None, tiff_predictor: int = 3, tiff_rows_per_strip=None) -> None:
    """Writes the tree save_prediction(<save_dir>/pred_seg, id, pred_masks[b], mean_masks[b], ignore) and
    save_uncertainty(<save_dir>, id, {name: map[b]}) write for every image b of a batch, with the same names, the same
    decoded PNG pixels and byte-identical TIFFs.

    pred_masks (B, N, H, W) uint8 arg-max per prediction, mean_masks (B, H, W) arg-max of the mean prediction (needed when
    N > 1), uncertainty {name: (B, H, W) float32}, ignore_index_map (B, H, W) or (H, W) (non-zero: unlabeled).  From
    predict2d, per batch:

        out = process_output_2d(logits)                   # pred_seg (B, H, W): arg-max of the mean; the three maps
        pm = uncertainty_maps(out["softmax_pred"], want_sample_argmax=True)["sample_argmax"]   # (B, N, H, W)
        save_images_device(save_dir, ids, pm, out["pred_seg"],
                           {k: out[k] for k in ("pred_entropy", "aleatoric_uncertainty", "epistemic_uncertainty") if k in out})

    One vx_png_encode call encodes all B (N + 1) masks (B N with one prediction); one small read brings back the file
    sizes, then the PNG bytes and the uncertainty maps come back in one copy each into reused pinned memory.

    tiff=None: uncompressed TIFFs, the bytes of write_tiff_f32(path, map).  tiff="lzw": the bytes of write_tiff_f32(path, map,
    "lzw", tiff_predictor, tiff_rows_per_strip) -- LZW strips with Predictor 1, 2 or 3 -- compressed on the device: one
    vx_tiff_predict call over all maps (not for predictor 1), one vx_tiff_lzw_encode call over all strips of all maps, one
    vx_tiff_lzw_pack; the strips' sizes join the small read and only the compressed bytes are copied back.  The PNG files
    are the same bytes either way."""
    _devio.save_once(save_dir, ("pred_seg",), _encode_images, image_ids, pred_masks, mean_masks, uncertainty, ignore_index_map,
                     _timing, tiff, tiff_predictor, tiff_rows_per_strip)


class ResultsWriter2D(_devio.PipelinedWriter):
    """Pipelined save_images_device: submit() encodes a batch on the GPU and hands its files to a small thread pool, so
    the files of batch i are written while batch i + 1 is encoded.  Two buffer sets alternate; a set is reused only once
    its files are written.  close() (or leaving the `with` block) waits and re-raises the first write error.
    tiff, tiff_predictor, tiff_rows_per_strip: as save_images_device takes them, for every batch of this writer."""

    _encode = staticmethod(_encode_images)
    _dirs = ("pred_seg",)

    def __init__(self, workers: int = 4, tiff=None, tiff_predictor: int = 3, tiff_rows_per_strip=None):
        if tiff not in (None, "lzw"):
            raise ValueError(f"ResultsWriter2D: tiff={tiff!r}: None or \"lzw\"")
        super().__init__(workers)
        self._tiff = (tiff, tiff_predictor, tiff_rows_per_strip)

    def submit(self, save_dir: str, image_ids: Sequence[str], pred_masks, mean_masks, uncertainty: Optional[Dict] = None,
               ignore_index_map=None, _timing=None) -> None:
        self._submit(save_dir, image_ids, pred_masks, mean_masks, uncertainty, ignore_index_map, _timing, *self._tiff)
