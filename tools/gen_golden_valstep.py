"""Generate tests/golden/valstep_kat.npz: tiny inputs and the reference-dtype (float32) validation/val_loss and
validation/val_dice of the three branches of LightningExperiment.validation_step, with ignore_index 0 (the 3D default:
nothing is ignored by the cross-entropy) and 1.

    python tools/gen_golden_valstep.py --reference <checkout of the reference>

SoftDiceLoss is IMPORTED from the reference's loss_modules.py; the cross-entropy, NLL, log-softmax, logsumexp and arg-max
are torch's CPU ops on float32 tensors, in the order validation_step / forward_ssn apply them.  The low-rank normal's
rsample is written out with the injected normals (loc + W eps_W + sqrt(D) eps_D, torch's formula) so that the recorded
numbers belong to recorded inputs.  torchmetrics is absent here: val_dice is its micro / global definition (the
ignore_index column of the one-hot tensors deleted, 2 tp / (2 tp + fp + fn)) written with torch ops -- parity with the
package itself stays unpinned, as for every Dice of this project.  The fixture is data only.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, R, S, T = 2, 2, 3, 4, 4
SP = (4, 5, 6)
EPSILON = 1e-5
IGNORE = (0, 1)


def micro_dice(pred_labels, target, ignore_index):
    oh_p = F.one_hot(pred_labels.reshape(-1), C)
    oh_t = F.one_hot(target.reshape(-1), C)
    keep = [c for c in range(C) if c != ignore_index]
    oh_p, oh_t = oh_p[:, keep], oh_t[:, keep]
    tp = (oh_p * oh_t).sum()
    fp = (oh_p * (1 - oh_t)).sum()
    fn = ((1 - oh_p) * oh_t).sum()
    den = 2 * tp + fp + fn
    return torch.tensor(0.0) if den == 0 else (2 * tp).float() / den.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "valstep_kat.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "uncertainty_modeling"))
    from loss_modules import SoftDiceLoss
    dice_loss, ce_loss, nll_loss = SoftDiceLoss(), torch.nn.CrossEntropyLoss(), torch.nn.NLLLoss()

    g = torch.Generator().manual_seed(20)
    nvox = int(np.prod(SP))
    seg = torch.randint(0, C, (B, 1) + SP, generator=g)
    logits = torch.randn((B, C) + SP, generator=g) * 2.0
    mu_s = torch.cat([torch.randn((B, C) + SP, generator=g) * 2.0, torch.randn((B, C) + SP, generator=g) * 0.8 - 1.0], 1)
    eps_al = torch.randn((B, T, C) + SP, generator=g)
    head = torch.cat([torch.randn((B, C) + SP, generator=g) * 2.0, torch.randn((B, C) + SP, generator=g) * 0.8 - 2.0,
                      torch.randn((B, R * C) + SP, generator=g) * 0.3], 1)
    eps_w = torch.randn((S, B, R), generator=g)
    eps_d = torch.randn((S, B, C * nvox), generator=g)
    out = {"seg": seg.numpy(), "logits": logits.numpy(), "mu_s": mu_s.numpy(), "eps_aleatoric": eps_al.numpy(),
           "head": head.numpy(), "eps_w": eps_w.numpy(), "eps_d": eps_d.numpy(), "epsilon": np.float32(EPSILON),
           "ignore_index": np.array(IGNORE, dtype=np.int64)}
    target = seg.long().squeeze(1)

    def ssn_samples(rank):
        loc = head[:, :C].reshape(B, -1)
        diag = head[:, C:2 * C].exp().reshape(B, -1) + EPSILON
        smp = loc[None] + diag.sqrt()[None] * eps_d
        if rank:
            fac = head[:, 2 * C:].reshape(B, R, C * nvox).transpose(1, 2)     # (B, C * nvox, R)
            smp = loc[None] + torch.einsum("bnr,sbr->sbn", fac, eps_w) + diag.sqrt()[None] * eps_d
        return smp.view(S, B, C, *SP)

    for ig in IGNORE:
        # the deterministic branch
        sm = F.softmax(logits, dim=1)
        loss = F.cross_entropy(logits, target, ignore_index=ig) if ig != 0 else dice_loss(sm, target) + ce_loss(logits, target)
        out[f"plain_loss_{ig}"] = loss.numpy()
        out[f"plain_dice_{ig}"] = micro_dice(torch.argmax(sm, dim=1), target, ig).numpy()
        # the aleatoric branch
        mu, s = mu_s[:, :C], mu_s[:, C:]
        sigma = torch.exp(s / 2)
        allp = torch.stack([F.log_softmax(mu + sigma * eps_al[:, t], dim=1) for t in range(T)])
        lavg = torch.logsumexp(allp, 0) - torch.log(torch.tensor(T))
        out[f"aleatoric_loss_{ig}"] = (dice_loss(torch.exp(lavg), target) + nll_loss(lavg, target)).numpy()
        out[f"aleatoric_dice_{ig}"] = micro_dice(torch.argmax(torch.exp(lavg), dim=1), target, ig).numpy()
        # the SSN branch, full rank and the pretraining epochs' mean_only distribution
        for name, rank in (("ssn", R), ("ssn_mean_only", 0)):
            smp = ssn_samples(rank)
            vd = torch.zeros([S])
            for i, lab in enumerate(torch.argmax(smp, dim=2)):
                vd[i] = micro_dice(lab, target, ig)
            tt = target.unsqueeze(1).expand((S,) + target.unsqueeze(1).shape).reshape(S * B, -1)
            flat = smp.reshape(S * B, C, -1)
            ce = F.cross_entropy(flat, tt, ignore_index=ig, reduction="none") if ig != 0 else F.cross_entropy(flat, tt, reduction="none")
            ll = torch.mean(torch.logsumexp(torch.sum(-ce.view(S, B, -1), dim=-1), dim=0) - math.log(S))
            out[f"{name}_loss_{ig}"] = (-ll).numpy()
            out[f"{name}_dice_{ig}"] = torch.mean(vd).numpy()
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
