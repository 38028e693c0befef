"""float64 torch restatement of the composed level-1 up-convolution (values_amd/csrc/upcompose16.h), shared by the CPU and the GPU
tests: the composed weights and the border table from the torch-layout tensors, and conv3d(conv_transpose3d(coarse)) rebuilt
from them."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.formula import formula_tensor


def formula_weights(seed=910):
    """(w1 [16][32][3][3][3], uw [32][16][2][2][2], ub [16]) float32, the scales of the evaluated-path kernel test; a LARGE up bias
    (a wrong border class moves the output by about one)"""
    w1 = torch.from_numpy(formula_tensor((16, 32, 3, 3, 3), seed, scale=(1.0 / (27 * 16)) ** 0.5)).float().contiguous()
    uw = torch.from_numpy(formula_tensor((32, 16, 2, 2, 2), seed + 1, scale=(1.0 / 32) ** 0.5)).float().contiguous()
    ub = torch.from_numpy(formula_tensor((16,), seed + 2, scale=3.0)).float().contiguous()
    return w1, uw, ub


def _sel():
    """S[p][a][k][d] = 1 where tap k of parity p maps to coarse tap a and sub-position d (t = p + k - 1, o = floor(t / 2))"""
    S = np.zeros((2, 2, 3, 2))
    for p in range(2):
        for k in range(3):
            t = p + k - 1
            o = t // 2
            S[p, o - (p - 1), k, t % 2] = 1.0
    return torch.from_numpy(S)


def weff_btab(w1, uw, ub):
    """Weff [8 classes (pz, py, px)][8 taps (a, b, c)][32 ci][16 co] and btab [3][3][3][16], float64"""
    W = w1.double()[:, :16]                      # the up half
    S = _sel()
    weff = torch.einsum("zakd,ybme,xcnf,oukmn,iudef->zyxabcio", S, S, S, W, uw.double()).reshape(8, 8, 32, 16)
    field = ub.double().view(1, 16, 1, 1, 1).expand(1, 16, 3, 3, 3)          # size 3 per axis: first, interior, last
    btab = F.conv3d(field, W, None, padding=1)[0].permute(1, 2, 3, 0).contiguous()
    return weff, btab


def apply_composed(coarse, weff, btab):
    """coarse (N, 32, Dc, Hc, Wc) float64 -> (N, 16, 2 Dc, 2 Hc, 2 Wc): the composed evaluation"""
    n, _, dc, hc, wc = coarse.shape
    cp = F.pad(coarse, (1, 1, 1, 1, 1, 1))
    out = torch.zeros((n, 16, 2 * dc, 2 * hc, 2 * wc), dtype=torch.float64)

    def cls_of(size):
        c = torch.ones(size, dtype=torch.long)
        c[0], c[-1] = 0, 2
        return c
    cz, cy, cx = cls_of(2 * dc), cls_of(2 * hc), cls_of(2 * wc)
    out += btab[cz][:, cy][:, :, cx].permute(3, 0, 1, 2).unsqueeze(0)
    for cls in range(8):
        pz, py, px = cls >> 2, (cls >> 1) & 1, cls & 1
        acc = 0
        for tap in range(8):
            a, b, c = tap >> 2, (tap >> 1) & 1, tap & 1
            win = cp[:, :, pz + a:pz + a + dc, py + b:py + b + hc, px + c:px + c + wc]
            acc = acc + torch.einsum("nizyx,io->nozyx", win, weff[cls, tap])
        out[:, :, pz::2, py::2, px::2] += acc
    return out
