"""Sliding-window inference over whole images: get_val_test_data_samples + predict_cases + concat_data +
caculcate_uncertainty_multiple_pred (toy_datamodule_3D.py:637-655, test_3D.py:417-534, data_carrier_3D.py:99-179,
208-217) with the patches batched on the device.

run_test_3d is run_test of test_3D.py:625-696 over a whole split: the forward batches are formed from the crop lists of
several cases (vx_gather_patches_3d, vx_softmax_accumulate_cases, vx_case_composite: csrc/patches3d.hip); predict_split_3d
is the same without the results writer.

compat=True reproduces the reference exactly, including quirk D10: `calculate_uncertainty` is applied to the
UN-normalised sums of overlapping patches and only the resulting maps are divided by clip(count, 1) at save time
(data_carrier_3D.py:323-337).  With the shipped `patch_overlap: 1` the count is 1 and both modes agree.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .predict import crop_indices, derive_seed, guarded, pin_seeds, predict_logits
from .uncertainty import uncertainty_maps


@torch.no_grad()
def predict_image_sliding(models: Sequence, image: torch.Tensor, patch_size: int = 64, patch_overlap: float = 1,
                          n_pred: int = 1, tta: bool = False, patch_batch: int = 8, compat: bool = True,
                          seeds=None, noise_fn=None, n_aleatoric_samples: int = 10, ssn: bool = False,
                          range_check: str = "fallback", noise_seed: Optional[int] = None,
                          **predict_kw) -> Dict[str, torch.Tensor]:
    """image: (X, Y, Z) float tensor (the preprocessed .npy of load_image).  Returns device tensors:
    softmax_sum (T, C, X,Y,Z), num_predictions (X,Y,Z), pred_entropy / aleatoric_uncertainty / epistemic_uncertainty
    (X,Y,Z) -- already divided by clip(count,1) like save_data --, mean_softmax (C, X,Y,Z), pred_seg_mean (X,Y,Z) u8.
    The number of passes T is whatever predict_logits produced for the model kind (n_pred, 16 TTA views, or
    n_aleatoric_samples for an aleatoric head: test_3D.py:458-469 sets n_pred := n_aleatoric_samples there), times the
    number of members.  ssn=True swaps the aleatoric / epistemic maps like calculate_uncertainty(ssn=True)
    (test_3D.py:510-516).
    noise_seed (tta=True): the noisy view of every patch is drawn on the device (values_amd.predict.noise_view_device), the
    patch's index in the crop list being its stream: the result does not depend on patch_batch.  noise_fn(x) -> x_noise, the
    caller's own draw per patch batch, keeps working; passing both raises ValueError.
    range_check: the fp16 range guard of values_amd.predict.guarded over the WHOLE image -- the range word is zeroed before
    the first patch batch (no read), read once after the last accumulate, and on overflow the image is computed again on
    the native-fp32 kernels with the same seeds ("raise": VxError; "off": the caller checks model.check_range())."""
    _lib.require_gpu()
    if noise_seed is not None and noise_fn is not None:
        raise ValueError("predict_image_sliding: pass noise_seed or noise_fn, not both")
    if range_check != "off":
        if seeds is None:
            seeds = pin_seeds(models, {}, tta=tta).get("seeds")
        return guarded(models, lambda: predict_image_sliding(models, image, patch_size=patch_size, patch_overlap=patch_overlap,
                                                             n_pred=n_pred, tta=tta, patch_batch=patch_batch, compat=compat,
                                                             seeds=seeds, noise_fn=noise_fn,
                                                             n_aleatoric_samples=n_aleatoric_samples, ssn=ssn,
                                                             range_check="off", noise_seed=noise_seed, **predict_kw),
                       range_check, "predict_image_sliding")
    lib = _lib.load()
    dev = image.device if image.is_cuda else torch.device("cuda", torch.cuda.current_device())
    img = image.to(dev, torch.float32).contiguous()
    X, Y, Z = img.shape
    crops = crop_indices((X, Y, Z), patch_size, patch_overlap)
    P = patch_size
    C = models[0].num_classes
    T, ssum = None, None          # allocated once the first batch has shown how many passes a patch gets
    count = torch.zeros((X, Y, Z), dtype=torch.float32, device=dev)
    overlap = int(int(P * patch_overlap) < P)
    for b0 in range(0, len(crops), patch_batch):
        batch = crops[b0:b0 + patch_batch]
        x = torch.stack([img[c[0][0]:c[0][1], c[1][0]:c[1][1], c[2][0]:c[2][1]] for c in batch]).unsqueeze(1)
        kw = {}
        if seeds is not None:
            kw["seeds"] = [derive_seed(int(s), 1, b0) for s in seeds]   # (one stream per patch batch: predict.derive_seed)
        x_noise = noise_fn(x) if (tta and noise_fn is not None) else None
        if tta and noise_seed is not None:
            kw.update(noise_seed=noise_seed, noise_index0=b0)           # (slot = the patch's index in the crop list)
        logits = predict_logits(models, x, n_pred=n_pred, tta=tta, x_noise=x_noise,
                                n_aleatoric_samples=n_aleatoric_samples, **kw, **predict_kw)  # (B, T, C, P,P,P)
        if ssum is None:
            T = int(logits.shape[1])
            ssum = torch.zeros((T, C, X, Y, Z), dtype=torch.float32, device=dev)
        if tuple(logits.shape) != (len(batch), T, C, P, P, P):
            raise _lib.VxError(f"predict_image_sliding: logits {tuple(logits.shape)} != {(len(batch), T, C, P, P, P)}")
        logits = logits.contiguous()
        crop_t = torch.tensor([[c[0][0], c[1][0], c[2][0]] for c in batch], dtype=torch.int32, device=dev)
        rc = lib.vx_softmax_accumulate(_lib.ptr(logits), len(batch), T, C, P, P, P, _lib.ptr(crop_t), _lib.ptr(ssum),
                                       _lib.ptr(count), X, Y, Z, overlap, _lib.stream_ptr())
        _lib.check(rc, "vx_softmax_accumulate")
    # maps of the un-normalised sums divided by clip(count, 1) afterwards (compat: quirk D10), or of the normalised
    # sums -- either division happens inside the reduction pass (vx_unc_reduce_ex), no separate tensor arithmetic
    cnt = count.unsqueeze(0)
    m = uncertainty_maps(ssum.unsqueeze(0), from_logits=False, want_variance=True,
                         **({"out_count": cnt} if compat else {"in_count": cnt}))
    pe, ee, mi = (m[k][0] for k in ("pred_entropy", "expected_entropy", "mutual_information"))
    # mean over T of softmax / clip(count,1) and its argmax (data_carrier_3D.py:215-217, 254-255); the per-voxel
    # count does not change the argmax
    mean = m["mean_softmax"][0]
    if ssn:
        ee, mi = mi, ee
    return {"softmax_sum": ssum, "num_predictions": count, "pred_entropy": pe, "aleatoric_uncertainty": ee,
            "epistemic_uncertainty": mi, "mean_softmax": mean, "pred_seg_mean": m["argmax"][0],
            "softmax_variance": m["softmax_variance"][0]}


def _patch_tables(patches, P):
    """patches: [(device case record, crop)] -> the vx_gather3d_item array of one forward batch"""
    from .dataset3d import _IMAGE_KIND
    arr = (_lib.Gather3dItem * len(patches))()
    for it, (c, crop) in zip(arr, patches):
        img = c["image"]
        if any(b - a != P for a, b in crop):
            raise ValueError(f"run_test_3d: {c['image_path']}: crop {crop} is not a {P}^3 patch")
        it.src, it.kind = img.data_ptr(), _IMAGE_KIND[str(img.dtype).replace("torch.", "")]
        for a in range(3):
            it.dims[a], it.origin[a] = int(img.shape[a]), int(crop[a][0])
    return arr


def gather_patches_3d(patches, P: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One vx_gather_patches_3d call: patches [(case record with a contiguous device "image", crop)] -> (B, 1, P, P, P)
    float32, numpy's astype(float32) of each crop, whatever the volumes' shapes and stored dtypes."""
    lib = _lib.load()
    B = len(patches)
    dev = patches[0][0]["image"].device
    if out is None:
        out = torch.empty((B, 1, P, P, P), dtype=torch.float32, device=dev)
    ws = _lib.workspace(dev, int(lib.vx_gather_patches_3d_workspace_bytes(B)))
    _lib.check(lib.vx_gather_patches_3d(_patch_tables(patches, P), B, _lib.ptr(out), P, P, P, _lib.ptr(ws), ws.numel(),
                                        _lib.stream_ptr()), "vx_gather_patches_3d")
    return out


def accumulate_cases(logits: torch.Tensor, dests, sum_overlap: bool) -> None:
    """One vx_softmax_accumulate_cases call: logits (B, T, C, P, P, P) float32, dests [(sum (T, C, X, Y, Z), count (X, Y, Z),
    origin)] per patch."""
    lib = _lib.load()
    B, T, C, P0, P1, P2 = (int(v) for v in logits.shape)
    arr = (_lib.Acc3dItem * B)()
    for it, (ssum, count, origin) in zip(arr, dests):
        it.sum, it.count = ssum.data_ptr(), count.data_ptr()
        for a in range(3):
            it.dims[a], it.origin[a] = int(count.shape[a]), int(origin[a])
    ws = _lib.workspace(logits.device, int(lib.vx_softmax_accumulate_cases_workspace_bytes(B)))
    _lib.check(lib.vx_softmax_accumulate_cases(_lib.ptr(logits), B, T, C, P0, P1, P2, arr, int(bool(sum_overlap)), _lib.ptr(ws),
                                               ws.numel(), _lib.stream_ptr()), "vx_softmax_accumulate_cases")


@torch.no_grad()
def predict_split_3d(models: Sequence, loader, n_pred: int = 1, tta: bool = False, ssn: bool = False, patch_size: int = 64,
                     patch_overlap: float = 1, patch_batch: int = 32, n_aleatoric_samples: int = 10, compat: bool = True,
                     seeds=None, noise_seed: Optional[int] = None, range_check: str = "fallback"):
    """The device half of run_test_3d as a generator: per case of the split, in order, {"image_id", "metrics",
    "softmax_sum" (T, C, X, Y, Z), "num_predictions" (X, Y, Z), "maps", "data", "gt_seg", "gt"} -- device tensors that are
    views of their group's buffers (a group's cases are yielded once the whole group is computed).  Arguments as
    run_test_3d."""
    from .dataset3d import composite_device, upload_group
    from .metrics import process_metrics_3d
    from .uncertainty import one_minus_msr_batch
    _lib.require_gpu()
    P = int(patch_size)
    sum_overlap = int(P * patch_overlap) < P
    if patch_batch < 1:
        raise ValueError("run_test_3d: patch_batch >= 1")
    if range_check != "off" and seeds is None:
        seeds = pin_seeds(models, {}, tta=tta).get("seeds")
    C = models[0].num_classes
    state = {"k": 0, "patch": 0, "T": None}
    for group in loader:
        if not group:
            continue
        if not isinstance(group[0]["image"], torch.Tensor):
            group = upload_group(group)
        for c in group:
            if not c["labels"]:
                raise ValueError(f"run_test_3d: {c['image_path']}: no rater file")
            c["image"] = c["image"].contiguous()
        dev = group[0]["image"].device
        patches = [(c, crop) for c in group for crop in c["crops"]]
        # cases of one shape and rater count lie side by side: their maps, masks and metrics are one call each
        keys = []
        for c in group:
            key = (tuple(int(v) for v in c["image"].shape), len(c["labels"]))
            if key not in keys:
                keys.append(key)
        blocks = [[c for c in group if (tuple(int(v) for v in c["image"].shape), len(c["labels"])) == key] for key in keys]
        k0, patch0 = state["k"], state["patch"]
        bufs = {}

        def compute():
            k, g = k0, patch0
            for b0 in range(0, len(patches), patch_batch):
                batch = patches[b0:b0 + patch_batch]
                x = gather_patches_3d(batch, P)
                kw = {}
                if seeds is not None:
                    kw["seeds"] = [derive_seed(int(s), 1, k) for s in seeds]
                if tta and noise_seed is not None:
                    kw.update(noise_seed=noise_seed, noise_index0=g)
                logits = predict_logits(models, x, n_pred=n_pred, tta=tta, n_aleatoric_samples=n_aleatoric_samples, **kw)
                T = int(logits.shape[1])
                if tuple(logits.shape) != (len(batch), T, C, P, P, P) or state["T"] not in (None, T):
                    raise _lib.VxError(f"run_test_3d: logits {tuple(logits.shape)} != {(len(batch), state['T'] or T, C, P, P, P)}")
                state["T"] = T
                if b0 == 0:      # (the first batch has shown how many passes a patch gets)
                    per = [(T * C + 1) * len(blk) * int(np.prod(key[0])) for blk, key in zip(blocks, keys)]
                    offs = np.cumsum([0] + [(n + 3) // 4 * 4 for n in per])
                    flat = _lib.zeros((int(offs[-1]),), torch.float32, dev)
                    bufs.clear()
                    for blk, key, o in zip(blocks, keys, offs):
                        n, nb = int(np.prod(key[0])), len(blk)
                        ssum = flat[o:o + nb * T * C * n].view((nb, T, C) + key[0])
                        cnt = flat[o + nb * T * C * n:o + nb * (T * C + 1) * n].view((nb,) + key[0])
                        bufs[key] = (ssum, cnt)
                        for i, c in enumerate(blk):
                            bufs[id(c)] = (ssum[i], cnt[i])
                accumulate_cases(logits.contiguous(), [bufs[id(c)] + ([a for a, _ in crop],) for c, crop in batch], sum_overlap)
                k += 1
                g += len(batch)
            return k, g

        state["k"], state["patch"] = guarded(models, compute, range_check, "run_test_3d")
        T = state["T"]
        per_block, gt_of, cnt_of = [], {}, {}
        for blk, key in zip(blocks, keys):
            ssum, cnt = bufs[key]
            m = uncertainty_maps(ssum, from_logits=False, want_sample_argmax=True, **({"out_count": cnt} if compat else {"in_count": cnt}))
            if T > 1:
                a, e = ("aleatoric_uncertainty", "epistemic_uncertainty") if not ssn else ("epistemic_uncertainty", "aleatoric_uncertainty")
                maps = {"pred_entropy": m["pred_entropy"], a: m["expected_entropy"], e: m["mutual_information"]}
            else:   # calculate_one_minus_msr under the key "pred_entropy" (test_3D.py:521-525), as process_output_2d's T = 1 branch
                msr = torch.empty((len(blk),) + key[0], dtype=torch.float32, device=dev)
                one_minus_msr_batch([m["mean_softmax"][i] for i in range(len(blk))], out=list(msr.unbind(0)))
                maps = {"pred_entropy": msr}
            # gt of the block as ONE (B, R, X, Y, Z) tensor: process_metrics_3d takes it where the composite call wrote it
            gt = torch.empty((len(blk), key[1]) + key[0], dtype=torch.uint8, device=dev)
            for i, c in enumerate(blk):
                gt_of[id(c)], cnt_of[id(c)] = gt[i], cnt[i]
            per_block.append((m, maps, gt))
        comp = composite_device(group, [cnt_of[id(c)] for c in group], gt_out=[gt_of[id(c)] for c in group])
        comp_of = {id(c): o for c, o in zip(group, comp)}
        per_case = {}
        for blk, key, (m, maps, gt) in zip(blocks, keys, per_block):
            ssum, cnt = bufs[key]
            res = process_metrics_3d({"mean_softmax": m["mean_softmax"], "argmax": m["argmax"]}, gt,
                                     sample_argmax=m["sample_argmax"])
            for i, c in enumerate(blk):
                per_case[id(c)] = (res[i], ssum[i], cnt[i], {k_: v[i] for k_, v in maps.items()}, comp_of[id(c)])
        for c in group:
            res, ssum, cnt, maps, comp = per_case[id(c)]
            yield {"image_id": c["image_id"], "metrics": res, "softmax_sum": ssum, "num_predictions": cnt, "maps": maps,
                   "data": comp["data"], "gt_seg": comp["gt_seg"], "gt": comp["gt"]}


@torch.no_grad()
def run_test_3d(models: Sequence, loader, save_dir: str, n_pred: int = 1, tta: bool = False, ssn: bool = False,
                patch_size: int = 64, patch_overlap: float = 1, patch_batch: int = 32, n_aleatoric_samples: int = 10,
                compat: bool = True, seeds=None, noise_seed: Optional[int] = None, range_check: str = "fallback",
                header=False, workers: int = 4) -> Dict[str, Dict]:
    """run_test of test_3D.py:625-696 over a whole split: per group of `loader` (a dataset3d.DeviceTestLoader3D, or the
    host loader, whose groups are uploaded here and take the same device path) the crops of the group's cases are joined
    into forward batches of patch_batch patches -- a batch may straddle cases --, each gathered straight from the resident
    file payloads (vx_gather_patches_3d), forwarded by predict_logits with the arguments predict_image_sliding passes, and
    accumulated into its patches' own images (vx_softmax_accumulate_cases; float atomics exactly when
    int(P * patch_overlap) < P).  Then, per group: the uncertainty maps and per-sample arg-max masks (compat as in
    predict_image_sliding; with one pass the score is 1 - max of the normalised softmax under "pred_entropy" and there are
    no aleatoric / epistemic maps), one vx_case_composite call (input, gt_seg, gt), process_metrics_3d per case shape, and
    ResultsWriter.submit per case; at the end metrics.json.  Returns {image_id: metrics}.
    Every case needs at least one rater file.  The sums and counts of a group's cases are one allocation zeroed by vx_zero.
    seeds: forward batch k OF THE SPLIT draws derive_seed(seed_m, 1, k); the batch slots of the hash dropout depend on the
    batching, so an MC-dropout result is a function of (seeds, patch_batch, the loader's group_cases).  noise_seed
    (tta): a patch's stream is its index in the split's crop list: a TTA result does not depend on the batching.
    range_check: predict.guarded's rule per group -- the range word is zeroed before the group's first batch, read once
    after its last, and on overflow the group is computed again under conv_fp32=1 with the same seeds."""
    from . import results
    metrics: Dict[str, Dict] = {}
    with results.ResultsWriter(workers=workers) as writer:
        for case in predict_split_3d(models, loader, n_pred=n_pred, tta=tta, ssn=ssn, patch_size=patch_size,
                                     patch_overlap=patch_overlap, patch_batch=patch_batch, n_aleatoric_samples=n_aleatoric_samples,
                                     compat=compat, seeds=seeds, noise_seed=noise_seed, range_check=range_check):
            metrics[case["image_id"]] = case["metrics"]
            writer.submit(save_dir, case["image_id"], case["softmax_sum"], case["maps"], data=case["data"], gt_seg=case["gt_seg"],
                          num_predictions=case["num_predictions"], header=header)
    results.log_metrics(save_dir, metrics)
    return metrics
