"""The 3D train and validation loaders of the toy and LIDC datamodules (uncertainty_modeling/toy_datamodule_3D.py:198-297,
369-578; lidc_idri_datamodule_3D.py:320-383, 455-664), Lightning- and batchgenerators-free.

Host mirror (numpy; the reference restated, device_io=False behaviour throughout):
    get_train_data_samples   the training listing of both datamodules (layout "toy" | "lidc")
    SampleOrder              NumpyDataLoader.reset / generate_train_batch as num_workers worker state machines, drained
                             round-robin
    plan_batch               the per-sample decisions: rater, crop origin, mirror flags, noise flag, global sample index
    HostLoader3D             np.load(mmap_mode="r"), slicing, [::-1] flips, float64 noise before the float32 cast
    create_splits            ToyDataModule3D.create_splits with KFold(shuffle=True) restated in numpy
    ToyDataModule3D, LIDCDataModule3D   the reference's constructor arguments plus device_io / cache_bytes
Device loader:
    DeviceLoader3D   the same SampleOrder and plan_batch; payloads go up once, in their stored dtype, and stay in a cache
                     keyed by path; a batch is ONE vx_train_patches_3d call (crop, mirror, noise and cast fused, image and
                     label in the same pass); the next batch's missing files are read while this one is in use.  No CPU
                     worker process.

Host and device loader share SampleOrder and plan_batch, so with the same seed they form identical batches; with noise
they differ: the host draws numpy normals, the device its own stream (vx_gauss), keyed by seed and the global sample index
(the running count of samples emitted since construction), so a device batch does not depend on how batch_size chunks a
given order and is reproducible from the seed.

NOT PINNED.  batchgenerators is not available to this project, so these are restated from belief, not observed:
  * the crop rule (batchgenerators' crop(..., crop_type="random") with zero margins: per axis np.random.randint(0, dim - P)
    when dim - P > 0, else (dim - P) // 2 -- the exclusive upper bound means the last origin is never drawn);
  * MirrorTransform's draw order (per sample three uniforms in axis order, mirror when < 0.5);
  * the drain order of MultiThreadedAugmenter (round-robin over the workers);
  * GaussianNoiseTransform's scale law (sigma_law, as values_amd.predict: 0 sqrt(var), 1 var) and p_per_sample = 0.1.
Also not pinned: the seeding of the worker processes (here ONE numpy RandomState(seed) and ONE random.Random(seed) serve
all workers in drain order), and the device noise, which is this project's stream, not numpy's.  Pinned: the listing, the
order within a worker over restarts, the rater choice after random.seed and the validation crops
(tests/golden/trainloader3d_kat.npz, recorded from the reference's NumpyDataLoader classes).
"""
from __future__ import annotations

import fnmatch
import os
import pickle
import random
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _devio, _lib
from .dataset2d import _npy_header, check_label_status
from .dataset3d import (_IMAGE_KIND, _LABEL_KIND, _check_case_files, _npy_file_header, _typed, get_val_test_data_samples)

NOISE_P = 0.1                 # GaussianNoiseTransform's p_per_sample
NOISE_VARIANCE = (0.0, 0.1)   # ... and its noise_variance


# ---------------------------------------------------------------------------------------------------------------------
# listing

def get_train_data_samples(base_dir, pattern: str = "*.npy", subject_ids=None, num_raters: int = 1, layout: str = "toy") -> List[Dict]:
    """toy_datamodule_3D.py:526-578 (layout "toy": imagesTr / labelsTr, <id>_<rr>.npy, subject_ids=None lists everything)
    and lidc_idri_datamodule_3D.py:612-664 (layout "lidc": images / labels, <id>_<rr>_mask.npy, subject_ids=None lists
    nothing).  One dict per image, in sorted order: image_path, label_paths (the rater files that exist, None when none
    does)."""
    if layout not in ("toy", "lidc"):
        raise ValueError(f"get_train_data_samples: layout {layout!r} is not 'toy' or 'lidc'")
    toy = layout == "toy"
    (image_dir, _, image_filenames) = next(os.walk(os.path.join(base_dir, "imagesTr" if toy else "images")))
    (label_dir, _, label_filenames) = next(os.walk(os.path.join(base_dir, "labelsTr" if toy else "labels")))
    name = "{}_{}.npy" if toy else "{}_{}_mask.npy"
    samples = []
    for image_filename in sorted(fnmatch.filter(image_filenames, pattern)):
        listed = (subject_ids is None or image_filename in subject_ids) if toy else \
            (subject_ids is not None and image_filename in subject_ids)
        if not listed:
            continue
        label_paths = []
        for rater in range(num_raters):
            label_name = name.format(image_filename.split(".")[0], str(rater).zfill(2))
            if label_name in label_filenames:
                label_paths.append(os.path.join(label_dir, label_name))
        samples.append({"image_path": os.path.join(image_dir, image_filename),
                        "label_paths": label_paths if len(label_paths) > 0 else None})
    return samples


# ---------------------------------------------------------------------------------------------------------------------
# sample order

class _Worker:
    """One copy of NumpyDataLoader as a MultiThreadedAugmenter worker holds it (toy_datamodule_3D.py:410-453): its own
    list, num_restarted, current_position; the list holds sample indices."""

    def __init__(self, n, batch_size, training, thread_id, n_threads):
        self.data = list(range(n))
        self.batch_size, self.training, self.thread_id, self.n_threads = batch_size, training, thread_id, n_threads
        self.num_restarted, self.current_position, self.was_initialized = 0, 0, False

    def reset(self):
        rs = np.random.RandomState(self.num_restarted)
        if self.training:
            rs.shuffle(self.data)                       # cumulative: the list is shuffled in place, restart after restart
        self.was_initialized = True
        self.num_restarted += 1
        self.current_position = self.thread_id * self.batch_size

    def next(self):
        while True:
            if not self.was_initialized:
                self.reset()
            idx = self.current_position
            if idx < len(self.data):
                self.current_position = idx + self.batch_size * self.n_threads
                return self.data[idx:min(len(self.data), idx + self.batch_size)]
            self.was_initialized = False


class SampleOrder:
    """The batches a FixedLengthAugmenter over NumpyDataLoader yields, as lists of samples: num_workers worker state
    machines (each its own copy of the list, start thread_id * batch_size, stride batch_size * num_workers, a restart when
    its position passes the end, the last batch of a pass short), drained round-robin -- the drain order is BELIEVED to be
    MultiThreadedAugmenter's, not observed.  len() is len(samples), as FixedLengthAugmenter reports it: BATCHES per
    "epoch", not samples (the reference's quirk); batches_per_epoch overrides it.  Iterating yields len() batches and keeps
    its state: the next iteration goes on where this one stopped."""

    def __init__(self, samples: Sequence[Dict], batch_size: int, training: bool = True, num_workers: int = 1,
                 batches_per_epoch: Optional[int] = None):
        self.samples = list(samples)
        if batch_size < 1 or num_workers < 1:
            raise ValueError("SampleOrder: batch_size >= 1 and num_workers >= 1")
        if not self.samples:
            raise ValueError("SampleOrder: no samples (the reference's loader would never return)")
        self.batch_size, self.training, self.num_workers = int(batch_size), bool(training), int(num_workers)
        if len(self.samples) <= (self.num_workers - 1) * self.batch_size:
            raise ValueError(f"SampleOrder: {len(self.samples)} samples leave worker {self.num_workers - 1} nothing at batch size "
                             f"{self.batch_size}: its generate_train_batch would restart for ever")
        self.workers = [_Worker(len(self.samples), self.batch_size, self.training, t, self.num_workers) for t in range(self.num_workers)]
        self.turn = 0
        self.batches_per_epoch = batches_per_epoch

    def __len__(self):
        return len(self.samples) if self.batches_per_epoch is None else int(self.batches_per_epoch)

    def next_indices(self) -> List[int]:
        w = self.workers[self.turn % self.num_workers]
        self.turn += 1
        return list(w.next())

    def next_batch(self) -> List[Dict]:
        return [self.samples[i] for i in self.next_indices()]

    def __iter__(self):
        for _ in range(len(self)):
            yield self.next_batch()


# ---------------------------------------------------------------------------------------------------------------------
# per-sample decisions

def plan_batch(samples: Sequence[Dict], patch_size: int, augment: bool, rng, pyrandom, index0: int, training: bool = True,
               noise_p: float = NOISE_P, shapes=None) -> List[Dict]:
    """One record per sample: {"image_path", "label_path" (random.choice of the rater files; None without any), "origin",
    "mirror" (three flags), "noise", "index" (index0 + i)}.  rng: a numpy RandomState, pyrandom: a random.Random.
    Draw order, as the reference's loop and transforms follow each other: per sample the rater and then the crop; with
    augment, per sample the three mirror uniforms in axis order; then per sample the noise uniform.  The number of draws
    per sample is fixed by (its label list, its shape, augment), whatever the draws' values.
    training: random crop -- per axis rng.randint(0, dim - P) when dim - P > 0, else (dim - P) // 2 (BELIEVED to be
    batchgenerators' rule; the exclusive bound means the last origin is never drawn); a volume smaller than the patch
    raises ValueError (batchgenerators would zero-pad; no preprocessed tree holds such a volume).  Validation: the
    sample's crop_idx, no mirror, no noise.  shapes: {image_path: shape}, read from the .npy headers where absent."""
    P = int(patch_size)
    out = []
    for i, s in enumerate(samples):
        label_path = pyrandom.choice(s["label_paths"]) if s.get("label_paths") is not None else None
        if training:
            shape = shapes[s["image_path"]] if shapes is not None and s["image_path"] in shapes else _npy_file_header(s["image_path"])[0]
            if len(shape) != 3:
                raise ValueError(f"{s['image_path']}: a 3-D image expected, got shape {shape}")
            origin = []
            for dim in shape:
                if dim < P:
                    raise ValueError(f"{s['image_path']}: shape {tuple(shape)} is smaller than the patch size {P}")
                origin.append(int(rng.randint(0, dim - P)) if dim - P > 0 else (dim - P) // 2)
        else:
            crop = s["crop_idx"]
            if any(int(b) - int(a) != P for a, b in crop):
                raise ValueError(f"{s['image_path']}: crop {crop} is not a patch of size {P}")
            origin = [int(a) for a, _ in crop]
        out.append({"image_path": s["image_path"], "label_path": label_path, "origin": tuple(origin), "mirror": (False, False, False),
                    "noise": False, "index": (int(index0) + i) & 0xFFFFFFFF})
    if training and augment:
        for r in out:
            r["mirror"] = tuple(bool(rng.uniform() < 0.5) for _ in range(3))
        for r in out:
            r["noise"] = bool(rng.uniform() < noise_p)
    return out


def _check_seg_dtype(seg_dtype):
    if seg_dtype not in ("float32", "uint8"):
        raise ValueError(f"seg_dtype {seg_dtype!r}: 'float32' (NumpyToTensor(cast_to='float')) or 'uint8'")
    return seg_dtype


class _Loader3D:
    """what the host and the device loader share: the order, the two generators of the decisions, the running index"""

    def __init__(self, samples, batch_size, patch_size, training, augment, num_workers, seed, seg_dtype, noise_p, noise_variance,
                 sigma_law, batches_per_epoch):
        self.order = SampleOrder(samples, batch_size, training, num_workers, batches_per_epoch)
        self.patch_size, self.training, self.augment = int(patch_size), bool(training), bool(augment)
        self.seed = int(seed)
        self.seg_dtype = _check_seg_dtype(seg_dtype)
        self.noise_p, self.noise_variance, self.sigma_law = float(noise_p), (float(noise_variance[0]), float(noise_variance[1])), int(sigma_law)
        if self.sigma_law not in (0, 1):
            raise ValueError("sigma_law: 0 (sqrt(var)) or 1 (var)")
        self.rng = np.random.RandomState(self.seed & 0xFFFFFFFF)
        self.pyrandom = random.Random(self.seed)
        self.emitted = 0                                # samples emitted since construction: the next global sample index
        self._shapes = {}

    def __len__(self):
        return len(self.order)

    def _shape(self, path):
        if path not in self._shapes:
            self._shapes[path] = _npy_file_header(path)[0]
        return self._shapes[path]

    def next_plan(self) -> List[Dict]:
        samples = self.order.next_batch()
        for s in samples:
            self._shape(s["image_path"])
        plan = plan_batch(samples, self.patch_size, self.augment, self.rng, self.pyrandom, self.emitted, self.training, self.noise_p,
                          self._shapes)
        self.emitted += len(plan)
        return plan


# ---------------------------------------------------------------------------------------------------------------------
# host loader

def host_patch(array, origin, mirror, P):
    """array[crop][flips]: the crop [origin, origin + P) with the mirrored axes reversed"""
    sl = tuple(slice(o, o + P) for o in origin)
    v = array[sl]
    for a in range(3):
        if mirror[a]:
            v = v[(slice(None),) * a + (slice(None, None, -1),)]
    return v


class HostLoader3D(_Loader3D):
    """The reference's loader on the host.  Iterating yields len() dicts: data (B, 1, P, P, P) float32, seg (B, 1, P, P, P)
    float32 -- NumpyToTensor(cast_to="float") casts every key -- or uint8 (seg_dtype="uint8": what
    validation.validation_step takes without a cast copy; a label outside 0..255 then raises ValueError), image_paths,
    label_paths.  seg is left out when no sample of the batch has a label; a sample without one in a batch that has some
    gets zeros.  Noise: data float64 + normal(0, sigma) from a generator of its own (RandomState(seed + 1): the decisions'
    generator is not advanced by the fields, so host and device loader stay in step), then the float32 cast."""

    def __init__(self, samples, batch_size: int = 16, patch_size: int = 64, training: bool = True, augment: bool = False,
                 num_workers: int = 1, seed: int = 42, seg_dtype: str = "float32", noise_p: float = NOISE_P,
                 noise_variance=NOISE_VARIANCE, sigma_law: int = 0, batches_per_epoch: Optional[int] = None):
        super().__init__(samples, batch_size, patch_size, training, augment, num_workers, seed, seg_dtype, noise_p, noise_variance,
                         sigma_law, batches_per_epoch)
        self.noise_rng = np.random.RandomState((self.seed + 1) & 0xFFFFFFFF)

    def make(self, plan):
        P = self.patch_size
        data, seg = [], []
        for r in plan:
            image = np.load(r["image_path"], mmap_mode="r")
            patch = np.asarray(host_patch(image, r["origin"], r["mirror"], P))
            if r["noise"]:
                var = self.noise_rng.uniform(*self.noise_variance)
                sigma = var if self.sigma_law else np.sqrt(var)
                patch = patch.astype(np.float64) + self.noise_rng.normal(0.0, sigma, size=patch.shape)
            data.append(patch.astype(np.float32)[None])
            if r["label_path"] is None:
                seg.append(None)
                continue
            lab = np.asarray(host_patch(np.load(r["label_path"], mmap_mode="r"), r["origin"], r["mirror"], P))
            if self.seg_dtype == "uint8":
                bad = int(np.count_nonzero((lab < 0) | (lab > 255)))
                check_label_status([bad], [r["label_path"]])
            seg.append(lab.astype(np.intc).astype(self.seg_dtype)[None])
        batch = {"data": np.stack(data), "image_paths": [r["image_path"] for r in plan],
                 "label_paths": [r["label_path"] for r in plan if r["label_path"] is not None]}
        if any(s is not None for s in seg):
            zero = np.zeros((1, P, P, P), dtype=self.seg_dtype)
            batch["seg"] = np.stack([zero if s is None else s for s in seg])
        return batch

    def __iter__(self):
        for _ in range(len(self)):
            yield self.make(self.next_plan())


# ---------------------------------------------------------------------------------------------------------------------
# device loader

class PayloadCache:
    """Payloads by path under a byte budget, least recently used out first.  budget None keeps everything, 0 nothing
    beyond what is pinned (the current and the prefetched batch); a pinned entry is never evicted, so the total may
    stand above the budget while the pinned entries alone exceed it."""

    def __init__(self, budget: Optional[int] = None):
        if budget is not None and budget < 0:
            raise ValueError("cache_bytes: None or >= 0")
        self.budget = budget
        self.entries = OrderedDict()     # path -> (value, nbytes), least recently used first
        self.pinned = set()
        self.bytes = 0

    def __contains__(self, key):
        return key in self.entries

    def get(self, key):
        self.entries.move_to_end(key)
        return self.entries[key][0]

    def put(self, key, value, nbytes):
        if key in self.entries:
            self.bytes -= self.entries.pop(key)[1]
        self.entries[key] = (value, int(nbytes))
        self.bytes += int(nbytes)

    def pin(self, keys):
        """the entries no eviction may take from now on (replaces the previous set), then evicts down to the budget"""
        self.pinned = set(keys)
        self.evict()

    def evict(self):
        if self.budget is None:
            return
        for key in list(self.entries):
            if self.bytes <= self.budget:
                break
            if key not in self.pinned:
                self.bytes -= self.entries.pop(key)[1]


def _plan_files(plan):
    out = []
    for r in plan:
        for p in (r["image_path"], r["label_path"]):
            if p is not None and p not in out:
                out.append(p)
    return out


class DeviceLoader3D(_Loader3D, _devio.PipelinedReader):
    """HostLoader3D's batches on the device: data / seg are torch tensors that stay there.  The .npy payloads of a batch's
    images and drawn rater files that are not resident go up in ONE pinned upload, in their stored dtype (the checks and
    errors of dataset3d's device loader), and stay in a PayloadCache keyed by path (cache_bytes: None keeps everything, 0
    nothing beyond the current and the prefetched batch; the budget counts payload bytes -- files that went up together
    share one device buffer, which lives as long as any of them is resident); the files the NEXT batch misses are read on
    the reader's pool while this batch is in use.  A batch is one vx_train_patches_3d call; a label outside 0..255 raises
    ValueError naming the rater file.  Noise: the project's stream under `seed`, keyed by the global sample index."""

    def __init__(self, samples, batch_size: int = 16, patch_size: int = 64, training: bool = True, augment: bool = False,
                 num_workers: int = 1, seed: int = 42, seg_dtype: str = "float32", noise_p: float = NOISE_P,
                 noise_variance=NOISE_VARIANCE, sigma_law: int = 0, batches_per_epoch: Optional[int] = None,
                 cache_bytes: Optional[int] = None, device=None, workers: int = 8):
        _Loader3D.__init__(self, samples, batch_size, patch_size, training, augment, num_workers, seed, seg_dtype, noise_p,
                           noise_variance, sigma_law, batches_per_epoch)
        _devio.PipelinedReader.__init__(self, device, workers)
        self.cache = PayloadCache(cache_bytes)

    def _missing(self, plan, also=()):
        return [p for p in _plan_files(plan) if p not in self.cache and p not in also]

    def _upload(self, names, raws, device):
        """the files' payloads -> the cache; shapes and dtypes are checked where the plan pairs image and label"""
        if not names:
            return
        heads = [_npy_header(nm, raw) for nm, raw in zip(names, raws)]
        pieces = [(raw, [(off, int(np.prod(shape, dtype=np.int64)) * dtype.itemsize)]) for raw, (shape, dtype, off) in zip(raws, heads)]
        buf, offs, sizes = self._staging.upload(pieces, device)
        for nm, (shape, dtype, _), o, n in zip(names, heads, offs, sizes):
            self.cache.put(nm, (_typed(buf, o, n, shape, dtype), shape, dtype), n)

    def make(self, plan, device):
        import torch
        lib = _lib.load()
        n, P = len(plan), self.patch_size
        items = (_lib.Train3dItem * n)()
        any_label = any(r["label_path"] is not None for r in plan)
        for it, r in zip(items, plan):
            img, shape, dtype = self.cache.get(r["image_path"])
            heads = [(r["image_path"], shape, dtype)]
            if r["label_path"] is not None:
                lab, lshape, ldtype = self.cache.get(r["label_path"])
                heads.append((r["label_path"], lshape, ldtype))
            _check_case_files(r, heads)
            it.image, it.image_kind = img.data_ptr(), _IMAGE_KIND[dtype.name]
            if r["label_path"] is not None:
                it.label, it.label_kind = lab.data_ptr(), _LABEL_KIND[ldtype.itemsize]
                it.label_flags = _lib.VX_LABEL_SIGNED if ldtype.kind == "i" else 0
            for a in range(3):
                it.dims[a], it.origin[a] = shape[a], r["origin"][a]
            it.flags = sum(1 << a for a in range(3) if r["mirror"][a]) | (_lib.VX_TRAIN3D_NOISE if r["noise"] else 0)
            it.index = r["index"]
        data = torch.empty((n, 1, P, P, P), dtype=torch.float32, device=device)
        seg = torch.empty((n, 1, P, P, P), dtype=getattr(torch, self.seg_dtype), device=device) if any_label else None
        status = torch.empty(n, dtype=torch.int32, device=device)
        ws = _lib.workspace(device, int(lib.vx_train_patches_3d_workspace_bytes(n)))
        _lib.check(lib.vx_train_patches_3d(items, n, P, P, P, _lib.ptr(data), _lib.ptr(seg), int(self.seg_dtype == "uint8"),
                                           self.seed & 0xFFFFFFFF, None, self.noise_variance[0], self.noise_variance[1], self.sigma_law,
                                           None, _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "vx_train_patches_3d")
        check_label_status(status.cpu().tolist(), [r["label_path"] or r["image_path"] for r in plan])
        batch = {"data": data, "image_paths": [r["image_path"] for r in plan],
                 "label_paths": [r["label_path"] for r in plan if r["label_path"] is not None]}
        if seg is not None:
            batch["seg"] = seg
        return batch

    def __iter__(self):
        _lib.require_gpu()
        dev = _devio.current_device(self.device)
        left = len(self)
        if left < 1:
            return
        plan = self.next_plan()
        pending = self._submit(self._missing(plan))
        while plan is not None:
            left -= 1
            names, futs = pending
            self._upload(names, [f.result() for f in futs], dev)
            nxt = self.next_plan() if left > 0 else None
            self.cache.pin(_plan_files(plan) + (_plan_files(nxt) if nxt is not None else []))
            pending = self._submit(self._missing(nxt)) if nxt is not None else None
            yield self.make(plan, dev)
            plan = nxt


# ---------------------------------------------------------------------------------------------------------------------
# splits

def kfold_indices(n: int, n_splits: int, seed):
    """sklearn's KFold(n_splits, shuffle=True, random_state=seed).split over n samples, restated: arange(n) permuted by
    RandomState(seed).shuffle; fold sizes n // k, one more for the first n % k folds; the fold's members in ascending
    order are the validation indices, the sorted complement the training indices.  -> [(train_idx, val_idx)]"""
    n, k = int(n), int(n_splits)
    if k < 2:
        raise ValueError("k-fold cross-validation requires at least one train/test split (n_splits >= 2)")
    if k > n:
        raise ValueError(f"Cannot have number of splits n_splits={k} greater than the number of samples: n_samples={n}.")
    perm = np.arange(n)
    np.random.RandomState(seed).shuffle(perm)
    sizes = np.full(k, n // k, dtype=int)
    sizes[:n % k] += 1
    out, start = [], 0
    for size in sizes:
        mask = np.zeros(n, dtype=bool)
        mask[perm[start:start + size]] = True
        out.append((np.arange(n)[~mask], np.arange(n)[mask]))
        start += size
    return out


def create_splits(output_dir, image_dir, test_dir, seed, n_splits: int = 5) -> None:
    """ToyDataModule3D.create_splits (toy_datamodule_3D.py:198-228): splits.pkl = one dict per fold, {"train", "val", "test"}
    numpy string arrays of the .npy file names (sorted listings of image_dir / test_dir)."""
    train_npy_files = sorted(f for f in os.listdir(image_dir) if f.endswith(".npy") and os.path.isfile(os.path.join(image_dir, f)))
    test_npy_files = sorted(f for f in os.listdir(test_dir) if f.endswith(".npy") and os.path.isfile(os.path.join(test_dir, f)))
    splits = []
    for train_idx, val_idx in kfold_indices(len(train_npy_files), n_splits, seed):
        splits.append({"train": np.array(train_npy_files)[train_idx], "val": np.array(train_npy_files)[val_idx],
                       "test": np.array(test_npy_files)})
    with open(os.path.join(output_dir, "splits.pkl"), "wb") as f:
        pickle.dump(splits, f)


# ---------------------------------------------------------------------------------------------------------------------
# datamodules

class _DataModule3D:
    layout = "toy"

    def _init(self, num_raters, data_input_dir, data_num_folds, data_fold_id, batch_size, patch_size, patch_overlap, num_workers, seed,
              augment, device_io, cache_bytes, seg_dtype):
        self.num_raters = num_raters
        self.data_input_dir = os.environ.get("DATASET_LOCATION", data_input_dir if data_input_dir is not None else os.getcwd())
        self.data_num_folds, self.data_fold_id = data_num_folds, data_fold_id
        self.batch_size, self.patch_size, self.patch_overlap = batch_size, patch_size, patch_overlap
        self.num_workers, self.seed, self.augment = num_workers, seed, augment
        self.device_io, self.cache_bytes, self.seg_dtype = bool(device_io), cache_bytes, seg_dtype
        self.tr_keys = self.val_keys = None

    @property
    def num_classes(self) -> int:
        return 2

    def _loader(self, samples, **kw):
        if self.device_io:
            return DeviceLoader3D(samples, patch_size=self.patch_size, seed=self.seed, seg_dtype=self.seg_dtype,
                                  cache_bytes=self.cache_bytes, **kw)
        return HostLoader3D(samples, patch_size=self.patch_size, seed=self.seed, seg_dtype=self.seg_dtype, **kw)

    def train_dataloader(self):
        samples = get_train_data_samples(self.base_dir, "*.npy", self.tr_keys, self.num_raters, self.layout)
        return self._loader(samples, batch_size=self.batch_size, training=True, augment=self.augment, num_workers=self.num_workers)

    def val_dataloader(self):
        samples = get_val_test_data_samples(self.base_dir, "*.npy", self.val_keys, self.num_raters, test=False,
                                            patch_size=self.patch_size, layout=self.layout)   # (patch_overlap: the loader's default 1)
        return self._loader(samples, batch_size=1, training=False, augment=False, num_workers=1)


class ToyDataModule3D(_DataModule3D):
    """toy_datamodule_3D.ToyDataModule3D without Lightning: the reference's constructor arguments, plus device_io (the
    preprocessing and both loaders on the device), cache_bytes (DeviceLoader3D) and seg_dtype."""
    layout = "toy"

    def __init__(self, dataset_name: str = "Case_1", num_raters: int = 3, data_input_dir: Optional[str] = None,
                 data_num_folds: int = 5, data_fold_id: int = 0, batch_size: int = 16, patch_size: int = 64,
                 patch_overlap: float = 1, num_workers: int = 8, seed: int = 42, augment: bool = False, *args,
                 device_io: bool = False, cache_bytes: Optional[int] = None, seg_dtype: str = "float32", **kwargs):
        self.dataset_name = dataset_name
        self._init(num_raters, data_input_dir, data_num_folds, data_fold_id, batch_size, patch_size, patch_overlap, num_workers, seed,
                   augment, device_io, cache_bytes, seg_dtype)
        self.test_keys = None

    @property
    def root_dir(self):
        return os.path.join(self.data_input_dir, self.dataset_name)

    @property
    def base_dir(self):
        return os.path.join(self.root_dir, "preprocessed")

    def prepare_data(self) -> None:
        from . import preprocess
        if not os.path.exists(self.base_dir):
            preprocess.preprocess_dataset(self.root_dir, self.root_dir, self.num_raters, image_dirs=["imagesTr", "imagesTs"],
                                          label_dirs=["labelsTr", "labelsTs"], patch_size=self.patch_size,
                                          patch_overlap=self.patch_overlap, device_io=self.device_io)
        if not os.path.exists(os.path.join(self.root_dir, "splits.pkl")):
            create_splits(self.root_dir, os.path.join(self.base_dir, "imagesTr"), os.path.join(self.base_dir, "imagesTs"), self.seed,
                          self.data_num_folds)

    def setup(self, stage: Optional[str] = None) -> None:
        with open(os.path.join(self.root_dir, "splits.pkl"), "rb") as f:
            splits = pickle.load(f)
        self.tr_keys, self.val_keys = splits[self.data_fold_id]["train"], splits[self.data_fold_id]["val"]
        self.test_keys = splits[self.data_fold_id]["test"]

    create_splits = staticmethod(create_splits)


class LIDCDataModule3D(_DataModule3D):
    """lidc_idri_datamodule_3D.LidcIdriDataModule3D without Lightning.  prepare_data leaves preprocessing (nodule cropping)
    and the patient-level, shift-feature splits to the caller: both must exist."""
    layout = "lidc"

    def __init__(self, shift_feature: Optional[str] = "internal Structure", num_raters: int = 3, data_input_dir: Optional[str] = None,
                 data_num_folds: int = 5, data_fold_id: int = 0, batch_size: int = 16, patch_size: int = 64,
                 patch_overlap: float = 1, num_workers: int = 8, seed: int = 42, splits_path: Optional[str] = None,
                 augment: bool = False, *args, device_io: bool = False, cache_bytes: Optional[int] = None,
                 seg_dtype: str = "float32", **kwargs):
        self.shift_feature = shift_feature
        self._init(num_raters, data_input_dir, data_num_folds, data_fold_id, batch_size, patch_size, patch_overlap, num_workers, seed,
                   augment, device_io, cache_bytes, seg_dtype)
        self.splits_path = splits_path if splits_path is not None else os.path.join(
            self.data_input_dir, "splits_{}.pkl".format(shift_feature if shift_feature is not None else "all"))
        self.id_test_keys = self.ood_test_keys = None

    @property
    def base_dir(self):
        return os.path.join(self.data_input_dir, "preprocessed")

    def prepare_data(self) -> None:
        for path in (self.base_dir, self.splits_path):
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path}: LIDC preprocessing and split creation are the caller's (not built here)")

    def setup(self, stage: Optional[str] = None) -> None:
        with open(self.splits_path, "rb") as f:
            splits = pickle.load(f)
        fold = splits[self.data_fold_id]
        self.tr_keys, self.val_keys = fold["train"], fold["val"]
        self.id_test_keys, self.ood_test_keys = fold.get("id_test"), fold.get("ood_test")
