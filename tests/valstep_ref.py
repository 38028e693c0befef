"""Restatement of the validation step's reductions (numpy float64, no GPU, nothing from values_amd): what
vx_val_sums_batched, vx_val_aleatoric_sums_batched and vx_val_ssn_sums_batched (valstep.hip) are held to in
tests/test_gpu_valstep.py, and the host arithmetic that turns their sums into validation/val_loss and
validation/val_dice (LightningExperiment.validation_step / forward_ssn(val=True), lightning_experiment.py:175-219,
278-377).  Pinned to torch and to tests/golden/valstep_kat.npz by tests/test_valstep_ref_cpu.py.

The reductions take float32 logits -- for the sampled kernels the float32 SAMPLES, formed in numpy (sample_ref with
dtype=float32) or written by the sample kernels -- and follow the kernels' float64 order (valstep.hip's header):
    a = lowest index of max_c y_c;  m = y_a;  se = sum_c exp(y_c - m) in class order;  lsm_c = (y_c - m) - log(se)
    plain: p_c = exp(y_c - m) / se
    aleatoric: running logsumexp over t of lsm_c[t]: (M, A) <- (l, 1) at t = 0; d = l - M, e = exp(-|d|),
               d > 0: (l, A e + 1) else (M, A + e);  lavg_c = (M + log A) - log T;  p_c = exp(lavg_c); arg-max of lavg
Each returns (sums, mag, allow): sums and mag like metrics3d_ref.np_soft_sums (mag: the same sums over |term|), allow: the
per-term allowances of the bound below, added up per slot.

THE BOUND of a float slot (float_bound): what separates the device's number from this file's is
  1. the order of the float64 additions: n * 2^-52 * mag for n terms;
  2. the device's double exp / log against numpy's.  ULP_DEV = 3: the OpenCL C specification's table of relative errors
     (section "Relative Error as ULPs", double precision: exp <= 3 ulp, log <= 3 ulp), the accuracy the ROCm device
     library (OCML) implements its double-precision functions to; numpy's are within 1 ulp.  So two evaluations differ by
     at most U = (ULP_DEV + 1) * 2^-53 relative.  Through one log-softmax: se carries U (each term does), log(se) then
     U + U |log se| <= U (1 + log C); with the subtraction's rounding a log term moves by at most
         e_lsm = U (2 + log C) + 2^-52 |lsm|
     and a softmax probability by 3 U p.  Through the aleatoric average: every step of the running sum adds one exp
     (U), feeds the moved lsm in twice (d, and M) and rounds twice, the closing log adds U (1 + |log A|) <= U (1 + log T),
     log T itself is one more evaluation:
         e_lavg = U (T + 3 + 2 log T) + 3 e_lsm(max_t |lsm|) + 2^-52 |lavg|,     p = exp(lavg): p (e_lavg + U)
     The np_val_* functions add these per-term figures up over a slot's terms (`allow`).
  3. only where the samples were formed in numpy: a differently contracted or rounded sample expression moves a sample
     logit by an ulp32 or two, and a log-softmax follows its inputs with slope <= 2:  sum_v 2 ulp32(max_c |y_c|)
     (for p slots weighted with p <= 1).
Integer slots (counts) are exact: ==.
"""
from __future__ import annotations

import math

import numpy as np

ULP_DEV = 3                          # double exp / log of the device library, OpenCL C specification (see above)
U = (ULP_DEV + 1) * 2.0 ** -53       # device against numpy, one evaluation, relative
SMOOTH = 1e-5                        # SoftDiceLoss()


# ---- the per-voxel arithmetic ------------------------------------------------------------------------------------------------
def log_softmax64(y):
    """y (..., C, nvox) float32 -> a (..., nvox) int64 the arg-max (lowest index on ties), lsm (..., C, nvox) float64,
    d = y - m and se (the plain kernel's softmax is exp(d) / se)"""
    y = np.asarray(y)
    assert y.dtype == np.float32
    a = np.argmax(y, axis=-2)                       # first occurrence of the maximum
    y64 = y.astype(np.float64)
    m = np.take_along_axis(y64, a[..., None, :], -2)
    d = y64 - m
    se = np.zeros(m.shape, np.float64)
    for c in range(y.shape[-2]):                    # class order
        se = se + np.exp(d[..., c:c + 1, :])
    return a, d - np.log(se), d, se


def _label_masks(t, C, ignore_label):
    t = np.asarray(t).astype(np.int64)
    ign = (t == ignore_label) if ignore_label is not None and ignore_label >= 0 else np.zeros(t.shape, bool)
    take = (t < C) & ~ign
    inv = (t >= C) & ~ign
    return t, take, inv


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def _class_sums(p, lt, a, t, take, inv, C, e_p, e_l, u32):
    """the [5C + 3] row of one item: p (C, nvox) float64, lt (nvox) the log term where taken, a (nvox) arg-max;
    e_p (C, nvox) / e_l (nvox): per-term allowances; u32 (nvox): 2 ulp32 of the sample logits or None.
    -> sums, mag, allow (all (5C + 3,))"""
    K = 5 * C + 3
    sums, mag, allow = np.zeros(K), np.zeros(K), np.zeros(K)
    for c in range(C):
        tc = t == c
        sums[5 * c + 0] = mag[5 * c + 0] = p[c][tc].sum()
        sums[5 * c + 1] = tc.sum()
        sums[5 * c + 2] = mag[5 * c + 2] = p[c].sum()
        sums[5 * c + 3] = (tc & (a == c)).sum()
        sums[5 * c + 4] = (a == c).sum()
        allow[5 * c + 0] = e_p[c][tc].sum() + (0.0 if u32 is None else (p[c] * u32)[tc].sum())
        allow[5 * c + 2] = e_p[c].sum() + (0.0 if u32 is None else (p[c] * u32).sum())
    sums[5 * C] = lt[take].sum()
    mag[5 * C] = np.abs(lt[take]).sum()
    allow[5 * C] = e_l[take].sum() + (0.0 if u32 is None else u32[take].sum())
    sums[5 * C + 1] = take.sum()
    sums[5 * C + 2] = inv.sum()
    return sums, mag, allow


def int_slots(C):
    """the integer slots of a [5C + 3] row"""
    return [5 * c + k for c in range(C) for k in (1, 3, 4)] + [5 * C + 1, 5 * C + 2]


def float_bound(n, mag, allow):
    """reordering of n float64 terms + the per-term allowances (module docstring)"""
    return n * 2.0 ** -52 * mag + allow


def np_val_sums(logits, labels, ignore_label=-1):
    """logits (B, C, nvox) float32, labels (B, nvox) -> sums, mag, allow (B, 5C + 3)"""
    logits = np.asarray(logits)
    B, C, nvox = logits.shape
    out = []
    for b in range(B):
        t, take, inv = _label_masks(labels[b], C, ignore_label)
        a, lsm, d, se = log_softmax64(logits[b])
        p = np.exp(d) / se
        tt = np.where(t < C, t, 0)
        lt = np.take_along_axis(lsm, tt[None], 0)[0]
        e_l = U * (2 + math.log(C)) + 2.0 ** -52 * np.abs(lt)
        out.append(_class_sums(p, lt, a, t, take, inv, C, 3 * U * p, e_l, None))
    return tuple(np.stack(x) for x in zip(*out))


def np_val_aleatoric_sums(samples, labels, ignore_label=-1, numpy_samples=False):
    """samples (B, T, C, nvox) float32 = fmaf(exp(s / 2), eps, mu), labels (B, nvox) -> sums, mag, allow (B, 5C + 3).
    numpy_samples: the samples were formed in numpy, not by the device's sample kernel (allowance 3)."""
    samples = np.asarray(samples)
    B, T, C, nvox = samples.shape
    out = []
    for b in range(B):
        t, take, inv = _label_masks(labels[b], C, ignore_label)
        _, lsm, _, _ = log_softmax64(samples[b])               # (T, C, nvox)
        M, A = lsm[0].copy(), np.ones((C, nvox))
        for k in range(1, T):
            d = lsm[k] - M
            e = np.exp(-np.abs(d))
            A = np.where(d > 0, A * e + 1.0, A + e)
            M = np.where(d > 0, lsm[k], M)
        lavg = (M + np.log(A)) - math.log(T)
        p = np.exp(lavg)
        a = np.argmax(lavg, axis=0)
        tt = np.where(t < C, t, 0)
        lt = np.take_along_axis(lavg, tt[None], 0)[0]
        e_lsm = U * (2 + math.log(C)) + 2.0 ** -52 * np.abs(lsm).max(0)          # (C, nvox)
        e_lavg = U * (T + 3 + 2 * math.log(T)) + 3 * e_lsm + 2.0 ** -52 * np.abs(lavg)
        u32 = 2 * ulp32(np.abs(samples[b]).max(1)).max(0) if numpy_samples else None
        out.append(_class_sums(p, lt, a, t, take, inv, C, p * (e_lavg + U), np.take_along_axis(e_lavg, tt[None], 0)[0], u32))
    return tuple(np.stack(x) for x in zip(*out))


def np_val_ssn_sums(samples, labels, ignore_label=-1, numpy_samples=False):
    """samples (B, S, C, nvox) float32 (vx_ssn_sample's layout), labels (B, nvox)
    -> sample_sums, smag, sallow (B, S, 1 + 2C): sum_v lsm_t | tp_c | pred_c;  target_sums (B, C + 2)"""
    samples = np.asarray(samples)
    B, S, C, nvox = samples.shape
    ss, sm, sa = (np.zeros((B, S, 1 + 2 * C)) for _ in range(3))
    ts = np.zeros((B, C + 2))
    for b in range(B):
        t, take, inv = _label_masks(labels[b], C, ignore_label)
        a, lsm, _, _ = log_softmax64(samples[b])               # (S, nvox), (S, C, nvox)
        tt = np.where(t < C, t, 0)
        for s in range(S):
            lt = np.take_along_axis(lsm[s], tt[None], 0)[0]
            ss[b, s, 0] = lt[take].sum()
            sm[b, s, 0] = np.abs(lt[take]).sum()
            sa[b, s, 0] = (U * (2 + math.log(C)) + 2.0 ** -52 * np.abs(lt[take])).sum()
            if numpy_samples:
                sa[b, s, 0] += (2 * ulp32(np.abs(samples[b, s]).max(0)))[take].sum()
            for c in range(C):
                ss[b, s, 1 + c] = ((a[s] == c) & (t == c)).sum()
                ss[b, s, 1 + C + c] = (a[s] == c).sum()
        for c in range(C):
            ts[b, c] = (t == c).sum()
        ts[b, C], ts[b, C + 1] = take.sum(), inv.sum()
    return ss, sm, sa, ts


# ---- the host arithmetic (validation_step's ratios from the sums) -----------------------------------------------------------------
def micro_dice(tp, pred, tgt, C, ignore_index):
    """torchmetrics dice(average='micro', mdmc_average='global', zero_division=0) from per-class counts pooled over the
    batch: the ignore_index column is deleted, tp / fp / fn are summed over the classes that are left"""
    cls = [c for c in range(C) if c != ignore_index]
    tp_, fp, fn = sum(tp[c] for c in cls), sum(pred[c] - tp[c] for c in cls), sum(tgt[c] - tp[c] for c in cls)
    den = 2 * tp_ + fp + fn
    return 0.0 if den == 0 else 2.0 * tp_ / den


def ce_ignore_label(ignore_index):
    """the reference's quirk: with ignore_index == 0 the cross-entropy is called WITHOUT ignore_index"""
    return -1 if ignore_index == 0 else int(ignore_index)


def loss_dice_from_sums(sums, C, nvox, ignore_index, aleatoric=False):
    """sums (B, 5C + 3) of a batch -> (val_loss, val_dice).  ignore_index == 0 (or the aleatoric branch, which never
    looks at it for the loss): SoftDice + CE / NLL over every voxel; else CE(ignore_index) alone."""
    sums = np.asarray(sums, np.float64)
    B = sums.shape[0]
    cls = sums[:, :5 * C].reshape(B, C, 5)
    inter, cnt, psum, tp, pred = (cls[:, :, k] for k in range(5))
    lsum, nval = sums[:, 5 * C].sum(), sums[:, 5 * C + 1].sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        ce = -lsum / nval if nval else float("nan")                # mean over the voxels that take a log term; none: nan
        if ignore_index == 0 or aleatoric:
            soft = np.mean(-((2.0 * inter + SMOOTH) / ((psum + cnt) + SMOOTH)))
            loss = soft + ce
        else:
            loss = ce
    dice = micro_dice(tp.sum(0), pred.sum(0), cnt.sum(0), C, ignore_index)
    return float(loss), float(dice)


def ssn_loss_dice_from_sums(sample_sums, target_sums, C, ignore_index):
    """sample_sums (B, S, 1 + 2C), target_sums (B, C + 2) -> (val_loss, val_dice):
    loss = -mean_b(logsumexp_s ll[b][s] - log S); val_dice = mean over s of the per-sample Dice over the whole batch
    (float64 here; the reference stores the S values in a float32 tensor and averages there: one float32 ulp apart)"""
    ss, ts = np.asarray(sample_sums, np.float64), np.asarray(target_sums, np.float64)
    B, S = ss.shape[:2]
    ll = ss[:, :, 0]             # (every voxel ignored: cross_entropy(reduction='none') is 0 there, ll = 0, loss = 0)
    mx = ll.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(ll - mx).sum(1))
    loss = -np.mean(lse - math.log(S))
    tgt = ts[:, :C].sum(0)
    d = np.array([micro_dice(ss[:, s, 1:1 + C].sum(0), ss[:, s, 1 + C:].sum(0), tgt, C, ignore_index) for s in range(S)])
    return float(loss), float(d.mean())


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def top_two_gap_ok(y, n_ulp=4):
    """every voxel of every sample: the two largest logits are further apart than n_ulp float32 ulps of the larger
    magnitude -- or bit-equal (an intended tie, which goes to the lowest index on any route).  y (..., C, nvox) float32"""
    y = np.asarray(y, np.float32)
    srt = np.sort(y.astype(np.float64), axis=-2)
    top, second = srt[..., -1, :], srt[..., -2, :]
    gap = top - second
    lim = n_ulp * ulp32(np.maximum(np.abs(top), np.abs(second)))
    return bool(np.all((gap > lim) | (gap == 0.0)))


def place_labels(rng, B, nvox, C, ignore_label, invalid=False):
    """labels (B, nvox) uint8: classes 0..C-1 at random, every class present where nvox allows; ignore_label at voxel
    nvox // 2 of every item (and on ~10 % of the others) when it is one; one invalid label (C + 1) at voxel 0 of the last
    item on request.  Asserts that they are where this says."""
    lab = rng.integers(0, C, size=(B, nvox)).astype(np.uint8)
    if nvox >= C:
        lab[:, :C] = np.arange(C, dtype=np.uint8)
    if ignore_label is not None and ignore_label >= 0:
        lab[rng.random((B, nvox)) < 0.1] = ignore_label
        lab[:, nvox // 2] = ignore_label
        assert (lab[:, nvox // 2] == ignore_label).all() and (lab == ignore_label).any(1).all()
    if invalid:
        bad = C + 1 if C + 1 != ignore_label else C + 2
        lab[B - 1, 0] = bad
        assert lab[B - 1, 0] >= C and lab[B - 1, 0] != ignore_label
    else:
        assert ((lab < C) | (lab == (ignore_label if ignore_label is not None else -1))).all()
    return lab


def separated_logits(rng, shape, scale=3.0, tie_at=None):
    """float32 logits (..., C, nvox) whose classes are well apart: class means spread by `scale`, top-two gap asserted;
    tie_at = (index tuple into the leading axes, voxel): every class of that voxel gets the same value"""
    y = (rng.standard_normal(shape) * scale).astype(np.float32)
    if tie_at is not None:
        lead, v = tie_at
        y[lead + (slice(None), v)] = np.float32(0.75)
    assert top_two_gap_ok(y), "input builder: a top-two gap within 4 float32 ulps"
    return y


def _separate(form, bump, what):
    """re-form the float32 samples until every top-two gap is wide (or an intended tie): bump(b, v) moves the offending
    voxels' class-0 mean by one; asserted at the end"""
    for _ in range(8):
        y = form()
        srt = np.sort(y.astype(np.float64), axis=-2)
        gap = srt[..., -1, :] - srt[..., -2, :]
        badv = ((gap <= 4 * ulp32(np.maximum(np.abs(srt[..., -1, :]), np.abs(srt[..., -2, :])))) & (gap != 0.0)).any(1)   # (B, nvox)
        if not badv.any():
            break
        bump(badv)
    assert top_two_gap_ok(y), f"input builder ({what}): a top-two gap within 4 float32 ulps"
    return y


def aleatoric_case(rng, B, T, C, nvox, tie=True):
    """mu_s (B, 2C, nvox), eps (B, T, C, nvox) float32 and the float32 samples (B, T, C, nvox) formed in numpy
    (sample_ref, dtype float32); tie: voxel nvox // 3 of item 0 has one value in every class of every sample"""
    from tests import sample_ref as sr
    mu = (rng.standard_normal((B, C, nvox)) * 3.0).astype(np.float32)
    s = (rng.standard_normal((B, C, nvox)) * 0.5 - 2.0).astype(np.float32)
    eps = rng.standard_normal((B, T, C, nvox)).astype(np.float32)
    if tie:
        mu[0, :, nvox // 3] = np.float32(0.75)
        eps[0, :, :, nvox // 3] = 0.0

    def form():
        return sr.aleatoric(np.concatenate([mu, s], 1), eps, 0, B, T, C, nvox, dtype=np.float32)[0].astype(np.float32)

    def bump(badv):
        mu[:, 0][badv] += np.float32(1.0)

    y = _separate(form, bump, "aleatoric")
    if tie:
        assert (y[0, :, :, nvox // 3] == np.float32(0.75)).all()
    return np.concatenate([mu, s], 1), eps, y


def ssn_case(rng, B, S, C, R, nvox, epsilon=1e-5, tie=True):
    """head (B, (2 + R)C, nvox), eps_w (S, B, R), eps_d (S, B, C * nvox) float32 and the float32 samples (B, S, C, nvox)
    formed in numpy; tie: voxel nvox // 3 of item 0 (factors and eps_d zero there, one mean for every class)"""
    from tests import sample_ref as sr
    mean = (rng.standard_normal((B, C, nvox)) * 3.0).astype(np.float32)
    logd = (rng.standard_normal((B, C, nvox)) * 0.5 - 2.0).astype(np.float32)
    fac = (rng.standard_normal((B, R * C, nvox)) * 0.2).astype(np.float32)
    eps_w = rng.standard_normal((S, B, R)).astype(np.float32)
    eps_d = rng.standard_normal((S, B, C, nvox)).astype(np.float32)
    if tie:
        mean[0, :, nvox // 3] = np.float32(0.75)
        fac[0, :, nvox // 3] = 0.0
        eps_d[:, 0, :, nvox // 3] = 0.0

    def form():
        return sr.ssn(np.concatenate([mean, logd, fac], 1), eps_w, eps_d, 0, B, S, C, R, nvox, epsilon, dtype=np.float32).astype(np.float32)

    def bump(badv):
        mean[:, 0][badv] += np.float32(1.0)

    y = _separate(form, bump, "ssn")
    if tie:
        assert (y[0, :, :, nvox // 3] == np.float32(0.75)).all()
    return np.concatenate([mean, logd, fac], 1), eps_w, eps_d.reshape(S, B, C * nvox), y
