"""The results-directory contract of the evaluation stage, MedPy/hydra-free.

`ExperimentVersion` and `ExperimentDataloader` mirror evaluation/experiment_version.py:4-51 and
evaluation/experiment_dataloader.py:11-169: same constructor arguments, attributes, method names and path scheme
    <base_path>/<naming_scheme_pred_model>/test_results/<version_name>/<split>/{pred_seg,pred_prob,pred_entropy,
    aleatoric_uncertainty,epistemic_uncertainty,gt_seg}/<id>...<ending>
so evaluation code written against the reference classes runs unchanged.  Files are read by their ending (`_load_file`):
volumes with `values_amd.nifti`, the 2D tree's PNG masks and TIFF maps with `values_amd.image_io`; the two arithmetic
methods (1 - max softmax, aggregation) run on the GPU.

Axis order of 2D files: UNPINNED.  The reference reads every file with medpy.io.load, MedPy is absent here, and for an
image file its axis order is not documented; evaluation/utils/gta.py:34 swaps the axes of the ground-truth map it builds
from a numpy label (`np.swapaxes(unc_map, 0, 1)`) to match what the loader hands back, so the loader returns [x, y].
A PNG / TIFF file is therefore returned with its first two axes swapped ((W, H) or (W, H, 3)).  The hooks are the
exception: `pred_seg_loading` / `gt_unc_map_loading` return what the hook returns.
`aggregate_uncertainties` mirrors evaluation/uncertainty_aggregation/aggregate_uncertainties.py:70-95.
"""
from __future__ import annotations

import json
import os
from pathlib import Path

import numpy as np

from . import nifti
from .io import instantiate


NIFTI_ENDINGS, PNG_ENDINGS, TIFF_ENDINGS = (".nii", ".nii.gz"), (".png",), (".tif", ".tiff")


def _kind(path) -> str:
    p = str(path).lower()
    for kind, ends in (("nifti", NIFTI_ENDINGS), ("png", PNG_ENDINGS), ("tiff", TIFF_ENDINGS)):
        if p.endswith(ends):
            return kind
    raise ValueError(f"{path}: not a results file (.nii, .nii.gz, .png, .tif, .tiff)")


def _load_file(path):
    """One file of a results tree as a numpy array: a volume indexed [x, y, z] (nifti.load), a 2D image with its first
    two axes swapped (module docstring: unpinned)."""
    kind = _kind(path)
    if kind == "nifti":
        return nifti.load(path)[0]
    from .image_io import read_png, read_tiff_f32
    return np.swapaxes(read_png(path) if kind == "png" else read_tiff_f32(path), 0, 1)


def _save_file(arr, path):
    """The inverse of _load_file for the files the dataloader itself writes (pred_entropy of a Softmax model)."""
    if _kind(path) == "tiff":
        from .image_io import write_tiff_f32
        write_tiff_f32(path, np.ascontiguousarray(np.swapaxes(np.asarray(arr, dtype=np.float32), 0, 1)))
    else:
        nifti.save(arr, path)


def _load_files_device(paths):
    """_load_file for a batch of paths, as device tensors: one load_device / load_png_device / load_tiff_device call per
    kind of file in the batch"""
    from . import images
    paths = [str(p) for p in paths]
    kinds = [_kind(p) for p in paths]
    out = [None] * len(paths)
    for kind in ("nifti", "png", "tiff"):
        sel = [i for i, k in enumerate(kinds) if k == kind]
        if not sel:
            continue
        if kind == "nifti":
            got = [t for t, _ in nifti.load_device([paths[i] for i in sel])]
        else:
            fn = images.load_png_device if kind == "png" else images.load_tiff_device
            got = [t.transpose(0, 1) for t in fn([paths[i] for i in sel])]
        for i, t in zip(sel, got):
            out[i] = t
    return out


PREFETCH_BATCH_2D = 256   # files per device call for PNG / TIFF files


def _read_batches_device(paths, batch, batch_2d=None):
    """(path, device tensor) for every path, read with the pipelined readers: the volumes `batch` files per
    nifti.NiftiReader call, then the 2D files `batch_2d` (default: batch) per images.ImageReader call"""
    from . import images
    paths = [str(p) for p in paths]
    vols = [p for p in paths if _kind(p) == "nifti"]
    imgs = [p for p in paths if _kind(p) != "nifti"]
    if vols:
        with nifti.NiftiReader() as r:
            for chunk, res in zip(_chunks(vols, batch), r.read(_chunks(vols, batch))):
                for p, (t, _) in zip(chunk, res):
                    yield p, t
    if imgs:
        n2 = batch if batch_2d is None else batch_2d
        with images.ImageReader() as r:
            for chunk, res in zip(_chunks(imgs, n2), r.read(_chunks(imgs, n2))):
                for p, t in zip(chunk, res):
                    yield p, t.transpose(0, 1)


def _decoded_shape_dtype(path):
    """(shape, numpy dtype) of what the readers return for one results file, from the file's header alone"""
    path = str(path)
    if _kind(path) == "nifti":
        import gzip
        with (gzip.open if path.lower().endswith(".gz") else open)(path, "rb") as f:
            h = nifti.parse_header(f.read(352), path)
        return h.shape, np.dtype(h.out_dtype)
    from .image_io import tiff_parse
    with open(path, "rb") as f:
        buf = f.read()
    lay = tiff_parse(buf, path)
    return (lay.w, lay.h), np.dtype("float32")


def softmax_chunk_size(shapes, dtypes, n_classes: int, chunk: int, budget_bytes: int) -> int:
    """Images per chunk of the Softmax tree setup: `chunk`, shrunk until the decoded class planes of a chunk of the
    largest images -- n_classes planes of `shape` and `dtype` each -- stay under budget_bytes; never below one image.
    Host logic on shapes and dtypes only."""
    largest = max((int(np.prod(s, dtype=np.int64)) * np.dtype(d).itemsize * int(n_classes) for s, d in zip(shapes, dtypes)),
                  default=0)
    fit = int(budget_bytes) // largest if largest > 0 else int(chunk)
    return max(1, min(int(chunk), fit))


class ExperimentVersion:
    def __init__(self, base_path, naming_scheme_version, pred_model, image_ending, unc_ending, unc_types, aggregations,
                 n_reference_segs, second_cycle_path=None, n_classes=2, naming_scheme_pred_model="{pred_model}",
                 datamodule_config=None, pred_seg_loading=None, gt_unc_map_loading=None, **kwargs):
        self.pred_model = pred_model
        self.naming_scheme_pred_model = naming_scheme_pred_model
        self.naming_scheme_version = naming_scheme_version
        self.version_params = kwargs
        self.version_name = self._build_version_name(naming_scheme_version=naming_scheme_version, **kwargs)
        self.base_path = Path(base_path)
        self.exp_path = (self.base_path / naming_scheme_pred_model.format(pred_model=pred_model, **kwargs)
                         / "test_results" / self.version_name)
        self.second_cycle_path = Path(second_cycle_path) if second_cycle_path is not None else None
        self.image_ending, self.unc_ending = image_ending, unc_ending
        self.n_reference_segs, self.n_classes = n_reference_segs, n_classes
        self.unc_types, self.aggregations = unc_types, aggregations
        self.datamodule_config = datamodule_config
        self.pred_seg_loading, self.gt_unc_map_loading = pred_seg_loading, gt_unc_map_loading

    def _build_version_name(self, naming_scheme_version: str, **kwargs):
        return naming_scheme_version.format(**kwargs)


def set_seed(seed: int) -> None:
    """evaluation/utils/set_seed.py:9-18 without the Lightning call: python / numpy / torch generators (the downstream
    tasks that sample -- Platt-scaling splits, threshold searches -- start from the experiment's seed)"""
    import random
    import numpy as np
    import torch
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)


class ExperimentDataloader:
    def __init__(self, exp_version: ExperimentVersion, dataset_split):
        self.exp_version = exp_version
        if "seed" in getattr(exp_version, "version_params", {}):      # experiment_dataloader.py:14
            set_seed(int(exp_version.version_params["seed"]))
        self.dataset_split = dataset_split
        self.dataset_path = exp_version.exp_path / dataset_split if dataset_split else exp_version.exp_path
        self.pred_seg_dir = self.dataset_path / "pred_seg"
        prob = self.dataset_path / "pred_prob"
        self.pred_prob_dir = prob if os.path.exists(prob) else None
        self.image_ids = sorted(self._get_image_ids())
        if exp_version.pred_model == "Softmax":
            self._setup_pred_entropy_softmax()
        self.unc_path_dict = self._setup_unc_path_dict()
        if exp_version.datamodule_config is not None:
            self.dataloader = self.setup_dataloader()
            self.ref_seg_dir = None
        else:
            self.dataloader = None
            self.ref_seg_dir = self.dataset_path / "gt_seg"

    # -- 1 - max softmax for plain Softmax models (experiment_dataloader.py:38-61), on the GPU
    def get_max_softmax_pred(self, image_id: str):
        import torch
        from .uncertainty import calculate_one_minus_msr
        probs = []
        for c in range(self.exp_version.n_classes):
            f = os.path.join(self.pred_prob_dir, f"{image_id}_01_{str(c + 1).zfill(2)}{self.exp_version.unc_ending}")
            probs.append(_load_file(f))
        return calculate_one_minus_msr(torch.from_numpy(np.array(probs)))["pred_entropy"].numpy()

    def _setup_pred_entropy_softmax(self):
        target = self.dataset_path / "pred_entropy"
        if not os.path.exists(target):
            os.makedirs(target)
            for image_id in self.image_ids:
                _save_file(self.get_max_softmax_pred(image_id), target / f"{image_id}{self.exp_version.unc_ending}")

    def _setup_unc_path_dict(self):
        return {u: self.dataset_path / ("pred_entropy" if u == "predictive_uncertainty" else u)
                for u in self.exp_version.unc_types}

    def _get_image_ids(self):
        end = self.exp_version.image_ending
        return set("_".join(n.split("_")[:-1]) for n in os.listdir(self.pred_seg_dir) if n.endswith(end))

    def get_pred_seg_paths(self, image_id):
        end = self.exp_version.image_ending
        return [self.pred_seg_dir / n for n in os.listdir(self.pred_seg_dir) if n.startswith(image_id) and n.endswith(end)]

    def get_pred_segs(self, image_id):
        return [_load_file(p) for p in self.get_pred_seg_paths(image_id)]

    def get_aggregated_unc_files_dict(self):
        return {u: self.dataset_path / f"aggregated_{u}.json" for u in self.unc_path_dict
                if os.path.isfile(self.dataset_path / f"aggregated_{u}.json")}

    def setup_dataloader(self):
        dm = instantiate(dict(self.exp_version.datamodule_config), test_split=self.dataset_split)
        dm.setup("test")
        return dm.test_dataloader()

    def _reference_segs(self, image_id):
        end = self.exp_version.image_ending
        return np.array([_load_file(self.ref_seg_dir / f"{image_id}_{i:02d}{end}")
                         for i in range(self.exp_version.n_reference_segs)])

    def get_reference_segs(self, image_id):
        if self.dataloader is not None:
            idx = self.dataloader.dataset.image_ids.index(image_id)
            return self.dataloader.dataset.__getitem__(idx)["seg"].squeeze().numpy()
        return self._reference_segs(image_id)

    def get_gt_unc_map(self, image_id):
        if self.exp_version.gt_unc_map_loading is None:
            return np.var(self._reference_segs(image_id), axis=0)  # experiment_dataloader.py:142
        return instantiate(dict(self.exp_version.gt_unc_map_loading), image_id=image_id, dataloader=self.dataloader)

    def get_mean_pred_seg(self, image_id):
        tag = "mean" if self.exp_version.pred_model != "Softmax" else "01"
        p = self.pred_seg_dir / f"{image_id}_{tag}{self.exp_version.image_ending}"
        if self.exp_version.pred_seg_loading is None:
            return _load_file(p)
        return instantiate(dict(self.exp_version.pred_seg_loading), pred_seg_path=p)

    def get_unc_map(self, image_id, unc_type):
        return _load_file(self.unc_path_dict[unc_type] / f"{image_id}{self.exp_version.unc_ending}")


def _aggregate(exp_dataloader, aggregations, images_of, batch):
    """aggregated_<unc>.json for every uncertainty type; images_of(unc_path, keys) yields the (key, image) pairs of a type's
    files, each image loaded once (the reference reloads per aggregation).  `_target_`s naming the reference's functions
    are re-pointed to values_amd.aggregation (GPU).  `batch` consecutive images go to one aggregation.aggregate_batch
    call (one device call each; any other `_target_` is instantiated per image there)."""
    from . import aggregation
    ending = exp_dataloader.exp_version.unc_ending
    pred_model = exp_dataloader.exp_version.pred_model
    for unc, unc_path in exp_dataloader.unc_path_dict.items():
        all_uncs, pending = {}, []

        def flush():
            got = aggregation.aggregate_batch([im for _, im in pending], aggregations, pred_model=pred_model, unc_type=unc)
            all_uncs.update(zip((k for k, _ in pending), got))
            pending.clear()
        for pair in images_of(unc_path, [f"{image_id}{ending}" for image_id in exp_dataloader.image_ids]):
            pending.append(pair)
            if len(pending) >= max(int(batch), 1):
                flush()
        if pending:
            flush()
        with open(exp_dataloader.dataset_path / f"aggregated_{unc}.json", "w") as f:
            json.dump(all_uncs, f, indent=4)


def aggregate_uncertainties(exp_dataloader: ExperimentDataloader, aggregations):
    """aggregate_uncertainties.py:70-95: for every uncertainty type, image and aggregation config
    ({"_target_": ..., **params}) -> aggregated_<unc>.json.  The files are read on the host, one image per device call."""
    _aggregate(exp_dataloader, aggregations, lambda unc_path, keys: ((k, _load_file(unc_path / k)) for k in keys), batch=1)


class DeviceExperimentDataloader(ExperimentDataloader):
    """ExperimentDataloader whose file getters return device tensors read with nifti.load_device, or for a 2D tree with
    images.load_png_device / load_tiff_device (same constructor, same paths, same axis order as the host getters).  get_reference_segs returns the stacked reference segmentations as one device tensor in the
    file branch; the GTA hooks (values_amd.gta) run in their device forms, any other hook, get_gt_unc_map without a hook
    and the datamodule branch are inherited unchanged.  prefetch() reads a split's files in
    batches ahead of the getters, under a byte budget.  For a Softmax model the constructor builds pred_entropy/ on the
    device as well (_setup_pred_entropy_softmax), and get_max_softmax_pred returns a device tensor."""

    def __init__(self, exp_version: ExperimentVersion, dataset_split):
        self._cache = {}
        super().__init__(exp_version, dataset_split)

    softmax_chunk = 32              # images per one_minus_msr_batch call of the Softmax tree setup ...
    softmax_budget_bytes = 1 << 30  # ... shrunk so that a chunk's decoded class planes stay under this (softmax_chunk_size)

    def _prob_paths(self, image_id):
        return [os.path.join(self.pred_prob_dir, f"{image_id}_01_{str(c + 1).zfill(2)}{self.exp_version.unc_ending}")
                for c in range(self.exp_version.n_classes)]

    def get_max_softmax_pred(self, image_id: str):
        """1 - max softmax of one image as a device tensor: the class files read on the device, a batch of one"""
        from . import uncertainty
        return uncertainty.one_minus_msr_batch([self._load_many(self._prob_paths(image_id))])[0]

    def _setup_pred_entropy_softmax(self):
        """pred_entropy/ of a Softmax tree without the host codecs: per chunk of images the C class files of each go
        through the pipelined readers, one one_minus_msr_batch call reduces the chunk, and results.MapsWriter encodes the
        maps on the device and writes chunk i while chunk i + 1 is read and reduced.  Same file names and decoded bytes as
        the host dataloader's; an existing directory is left alone."""
        from . import results, uncertainty
        target = self.dataset_path / "pred_entropy"
        if os.path.isdir(target):
            return
        os.makedirs(target)
        if not self.image_ids:
            return
        C, end = self.exp_version.n_classes, self.exp_version.unc_ending
        first = [_decoded_shape_dtype(self._prob_paths(i)[0]) for i in self.image_ids]
        B = softmax_chunk_size([s for s, _ in first], [d for _, d in first], C, self.softmax_chunk, self.softmax_budget_bytes)
        stream = _read_batches_device([p for i in self.image_ids for p in self._prob_paths(i)], C * B)
        try:
            with results.MapsWriter() as writer:
                for part in _chunks(self.image_ids, B):
                    planes = [[next(stream)[1] for _ in range(C)] for _ in part]
                    writer.submit([target / f"{i}{end}" for i in part], uncertainty.one_minus_msr_batch(planes))
        finally:
            stream.close()

    def _load(self, path):
        p = str(path)
        if p in self._cache:
            return self._cache.pop(p)
        return _load_files_device([p])[0]

    def _load_many(self, paths):
        paths = [str(p) for p in paths]
        missing = [p for p in paths if p not in self._cache]
        got = dict(zip(missing, _load_files_device(missing))) if missing else {}
        return [self._cache.pop(p) if p in self._cache else got[p] for p in paths]

    def _files_of(self, image_id):
        end = self.exp_version.image_ending
        out = [str(p) for p in self.get_pred_seg_paths(image_id)]
        out += [str(self.unc_path_dict[u] / f"{image_id}{self.exp_version.unc_ending}") for u in self.unc_path_dict]
        if self.dataloader is None and self.ref_seg_dir is not None:
            out += [str(self.ref_seg_dir / f"{image_id}_{i:02d}{end}") for i in range(self.exp_version.n_reference_segs)]
        return [p for p in dict.fromkeys(out) if os.path.isfile(p)]

    def prefetch(self, image_ids=None, budget_bytes: int = 1 << 30, batch: int = 64, batch_2d: int = PREFETCH_BATCH_2D) -> int:
        """Read the files of `image_ids` (default: the split) the getters read, `batch` volumes per load_device call
        (`batch_2d` PNG / TIFF files per call for a 2D tree: a device call costs about its slowest stream, so the small
        2D files want many in flight), until the decoded tensors reach `budget_bytes`; the getters then take them from
        the cache (once each).  Returns the number of files cached."""
        paths = [p for i in (self.image_ids if image_ids is None else image_ids) for p in self._files_of(i)]
        paths = [p for p in paths if p not in self._cache]
        used = sum(t.numel() * t.element_size() for t in self._cache.values())
        n = 0
        for p, t in _read_batches_device(paths, batch, batch_2d):
            if used + t.numel() * t.element_size() > budget_bytes:
                return n
            self._cache[p] = t
            used += t.numel() * t.element_size()
            n += 1
        return n

    def get_pred_segs(self, image_id):
        return self._load_many(self.get_pred_seg_paths(image_id))

    def _device_loader_2d(self):
        """the datamodule's loader when it is a dataset2d.DeviceTestLoader2D (datamodule config with device_io=True), else None"""
        from .dataset2d import DeviceTestLoader2D
        return self.dataloader if isinstance(self.dataloader, DeviceTestLoader2D) else None

    def get_reference_segs(self, image_id):
        import torch
        if self.dataloader is not None:
            if self._device_loader_2d() is not None:   # the raters drawn on the device, keyed by the image's split index
                return self.dataloader.reference_segs(image_id)
            return super().get_reference_segs(image_id)
        end = self.exp_version.image_ending
        return torch.stack(self._load_many([self.ref_seg_dir / f"{image_id}_{i:02d}{end}"
                                            for i in range(self.exp_version.n_reference_segs)]))

    @staticmethod
    def _device_hook(cfg):
        """a hook config with the GTA hooks (values_amd.gta, under any of their spellings) re-pointed to their device
        forms; any other hook runs as it is"""
        from .io import TARGET_MAP
        cfg = dict(cfg)
        target = TARGET_MAP.get(cfg["_target_"], cfg["_target_"])
        if target in ("values_amd.gta.pred_seg_loading", "values_amd.gta.gt_unc_map"):
            cfg["_target_"] = target + "_device"
        return cfg

    def get_gt_unc_map(self, image_id):
        if self.exp_version.gt_unc_map_loading is None:
            return super().get_gt_unc_map(image_id)
        cfg = self._device_hook(self.exp_version.gt_unc_map_loading)
        if cfg["_target_"] == "values_amd.gta.gt_unc_map_device" and self._device_loader_2d() is not None:
            return self.dataloader.gt_unc_map(image_id)   # the label goes up as it is: no map is made on the host
        return instantiate(cfg, image_id=image_id, dataloader=self.dataloader)

    def get_gt_unc_map_device(self, image_id):
        """get_gt_unc_map without the host: in the file branch the variance over the device-read reference segmentations
        (evalmetrics.rater_variance: np.var(..., axis=0) bit for bit, a float64 device map); with a hook, the hook's map.
        get_gt_unc_map itself keeps returning the host array in the file branch."""
        if self.exp_version.gt_unc_map_loading is None and self.dataloader is None:
            from .evalmetrics import rater_variance
            refs = self.get_reference_segs(image_id)
            if not refs.dtype.is_floating_point:
                return rater_variance(refs)
        return self.get_gt_unc_map(image_id)

    def get_mean_pred_seg(self, image_id):
        tag = "mean" if self.exp_version.pred_model != "Softmax" else "01"
        p = self.pred_seg_dir / f"{image_id}_{tag}{self.exp_version.image_ending}"
        if self.exp_version.pred_seg_loading is not None:
            return instantiate(self._device_hook(self.exp_version.pred_seg_loading), pred_seg_path=p)
        return self._load(p)

    def get_unc_map(self, image_id, unc_type):
        return self._load(self.unc_path_dict[unc_type] / f"{image_id}{self.exp_version.unc_ending}")


def _chunks(seq, n):
    return [seq[i:i + n] for i in range(0, len(seq), max(int(n), 1))]


def aggregate_uncertainties_device(exp_dataloader: ExperimentDataloader, aggregations, batch: int = 32):
    """aggregate_uncertainties with the maps read on the device: every map of a type is read with nifti.NiftiReader (or,
    for a 2D tree's TIFF maps, images.ImageReader), `batch` files per call, and the maps of one reader batch are
    aggregated by one aggregation.aggregate_batch call.  Writes the same aggregated_<unc>.json, byte for byte."""
    def images_of(unc_path, keys):
        for key, (_, unc_image) in zip(keys, _read_batches_device([unc_path / k for k in keys], batch)):
            yield key, unc_image

    _aggregate(exp_dataloader, aggregations, images_of, batch=batch)
