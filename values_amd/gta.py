"""The GTA / Cityscapes hooks of the evaluation stage (evaluation/utils/gta.py), OpenCV-free: what an ExperimentVersion
names as `pred_seg_loading` and `gt_unc_map_loading` for the 2D experiments.

    pred_seg_loading(pred_seg_path)       colour PNG mask -> train ids (int64 (H, W); a colour that is no class's: 128)
    gt_unc_map(image_id, dataloader)      the label-switch variance map of an image's label (float32, axes swapped)

The `_device` forms return device tensors: the PNG is read with images.load_png_device and the colours are looked up by
vx_rgb_to_trainid.  COLOR2TRAINID is the reference's cityscapes_labels.color2trainId (tools/gen_golden.py writes it to
tests/golden/cityscapes_color2trainid.json, which tests/test_images_read_cpu.py holds this table against).
"""
from __future__ import annotations

import numpy as np

UNKNOWN = 128   # gta.py:10: color2trainId.get(tuple(x), 128)
COLOR2TRAINID = {
    (84, 86, 22): 23, (242, 160, 19): 22, (30, 193, 252): 21, (167, 242, 242): 20, (46, 247, 180): 19,
    (20, 20, 20): 255, (0, 0, 142): 13, (119, 11, 32): 18, (0, 0, 230): 17, (0, 80, 100): 16, (0, 0, 110): 255,
    (0, 0, 90): 255, (0, 60, 100): 15, (0, 0, 70): 14, (255, 0, 0): 12, (220, 20, 60): 11, (70, 130, 180): 10,
    (152, 251, 152): 9, (107, 142, 35): 8, (220, 220, 0): 7, (250, 170, 30): 6, (153, 153, 153): 5,
    (150, 120, 90): 255, (150, 100, 100): 255, (180, 165, 180): 255, (190, 153, 153): 4, (102, 102, 156): 3,
    (70, 70, 70): 2, (230, 150, 140): 255, (250, 170, 160): 255, (244, 35, 232): 1, (128, 64, 128): 0,
    (81, 0, 81): 255, (111, 74, 0): 255, (0, 0, 0): 255,
}
# gta.py:20-33: every class a label switch starts from, and the switch's probability
LABEL_SWITCHES = {"sidewalk": 1.0 / 3.0, "person": 1.0 / 3.0, "car": 1.0 / 3.0, "vegetation": 1.0 / 3.0, "road": 1.0 / 3.0}
NAME2TRAINID = {"sidewalk": 1, "person": 11, "car": 13, "vegetation": 8, "road": 0}


def rgb_keys(rgb: np.ndarray) -> np.ndarray:
    """(..., 3) uint8 RGB -> 0x00RRGGBB keys"""
    a = np.asarray(rgb).astype(np.uint32)
    return (a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2]


def _table() -> np.ndarray:
    """(n, 2) uint32: (0x00RRGGBB key, train id) per colour -- vx_rgb_to_trainid's table"""
    return np.array([[(r << 16) | (g << 8) | b, i] for (r, g, b), i in COLOR2TRAINID.items()], dtype=np.uint32)


def rgb_to_trainid_host(rgb: np.ndarray) -> np.ndarray:
    """(H, W, 3) uint8 RGB -> (H, W) int64 train ids, UNKNOWN for any other colour"""
    keys = rgb_keys(rgb)
    out = np.full(keys.shape, UNKNOWN, dtype=np.int64)
    for k, i in _table():
        out[keys == k] = i
    return out


def pred_seg_loading(pred_seg_path):
    """gta.py:6-12: cv2.imread + BGR2RGB is the file's RGB image; alpha, if any, is dropped as cvtColor drops it."""
    from .image_io import read_png
    img = read_png(pred_seg_path)
    if img.ndim != 3:
        raise ValueError(f"{pred_seg_path}: a colour mask (RGB / RGBA) expected, got a grey image")
    return rgb_to_trainid_host(img[..., :3])


def _switch_variance(label):
    unc_map = np.zeros_like(label, dtype=np.single)
    for c, p in LABEL_SWITCHES.items():
        mean = p   # (1 - p) * 0 + p * 1
        unc_map[label == NAME2TRAINID[c]] = (1 - p) * np.square(0 - mean) + p * np.square(1 - mean)
    return np.swapaxes(unc_map, 0, 1)


def gt_unc_map(image_id, dataloader):
    """gta.py:15-35: the variance of the Bernoulli label switch on every pixel of a class that switches, 0 elsewhere;
    float32, first two axes swapped as the reference returns it."""
    idx = dataloader.dataset.image_ids.index(image_id)
    return _switch_variance(np.load(str(dataloader.dataset.masks[idx])))


# ---------------------------------------------------------------------------------------------------------------------
_tables = {}


def _device_table(dev):
    import torch
    k = dev.index if dev.index is not None else torch.cuda.current_device()
    if k not in _tables:
        _tables[k] = torch.from_numpy(_table().view(np.int32)).to(dev)
    return _tables[k]


def rgb_to_trainid(rgb, table=None, default_id: int = UNKNOWN):
    """(..., 3) uint8 device tensor -> (...) uint8 train ids on the device (vx_rgb_to_trainid); table: an (n <= 256, 2)
    int32 / uint32 device tensor of (0x00RRGGBB, id) pairs, default COLOR2TRAINID."""
    import torch
    from . import _lib
    _lib.require_gpu()
    if not isinstance(rgb, torch.Tensor) or not rgb.is_cuda or rgb.dtype != torch.uint8 or rgb.shape[-1] != 3:
        raise _lib.VxError("rgb_to_trainid: a (..., 3) uint8 device tensor expected")
    rgb = rgb.contiguous()
    tab = _device_table(rgb.device) if table is None else table.contiguous()
    out = torch.empty(rgb.shape[:-1], dtype=torch.uint8, device=rgb.device)
    _lib.check(_lib.load().vx_rgb_to_trainid(_lib.ptr(rgb), out.numel(), _lib.ptr(tab), int(tab.shape[0]), int(default_id),
                                             _lib.ptr(out), _lib.stream_ptr()), "vx_rgb_to_trainid")
    return out


def pred_seg_loading_device(pred_seg_path, device=None):
    """pred_seg_loading as an int64 (H, W) device tensor"""
    import torch
    from .images import load_png_device
    img = load_png_device([pred_seg_path], device)[0]
    if img.dim() != 3:
        raise ValueError(f"{pred_seg_path}: a colour mask (RGB / RGBA) expected, got a grey image")
    return rgb_to_trainid(img[..., :3]).to(torch.int64)


def gt_unc_map_device(image_id, dataloader, device=None):
    """gt_unc_map as a float32 device tensor (the label is a .npy file: read on the host)"""
    import torch
    m = torch.from_numpy(np.ascontiguousarray(gt_unc_map(image_id, dataloader)))
    return m.to(torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device()))
