"""HRNetV2 segmentation network on MI355X: the reference's class surface, HIP kernels underneath.

Mirrors `uncertainty_modeling.models.hrnet_module.HighResolutionNet` / `get_seg_model` (hrnet_module.py:340-745): the
same config object (MODEL.EXTRA stages, DROPOUT_FINAL, FINAL_CONV_KERNEL, DATASET.NUM_CLASSES), the same module tree
and therefore the same state-dict key names (`conv1.weight`, `layer1.0.downsample.1.bias`,
`stage3.2.fuse_layers.1.0.0.0.weight`, `last_layer.3.bias`, ...), so the reference's checkpoints load unchanged.
The torch.nn layers are PARAMETER CONTAINERS; `forward` walks the tree and launches libvalues_amd.so kernels:
vx_conv2d (+ batch statistics) -> vx_bn_finalize -> vx_affine_gather (BN affine, ReLU, residual add, bilinear
fusion, dropout, concat) -> vx_bilinear_nchw (eval mode: vx_conv2d with its output epilogue -> vx_fuse_sum / the
concat -> vx_bilinear_nchw).  ATen is never used for arithmetic.

BatchNorm.  Default (train mode, the state of a fresh nn.Module): batch statistics as the reference runs --
every BatchNorm normalises with the statistics of the CURRENT batch (the reference never calls .eval()); the running-
statistics side effect is not reproduced, so a forward never changes the buffers.  `.eval()`: running statistics -- every
BatchNorm is the per-channel affine of its stored running_mean / running_var (one table for the model, one
vx_bn_running_affine launch per checkpoint), applied with the residual and the ReLU in the producing conv's epilogue
(vx_conv2d_args.out_scale): no statistics partials, no vx_bn_finalize launches, no block-end affine pass, and an image's
logits no longer depend on its batch mates; statistics groups (the batched TTA views) mean nothing there.  `.train()`
afterwards gives the bits of a model that never left train mode.
DROPOUT_FINAL is F.dropout(0.5, training=True) on the four stage-4 outputs -- live in BOTH modes, as in the reference --
so only the head differs between MC samples: `forward_samples` runs the backbone once and the head T times (exact).

fp16 range.  The split-fp16 convs stage every activation as hi + lo * 2^-11 in fp16: they assume |activation| < 65504.  In
train mode the batch statistics renormalise every layer, whatever the weights; in eval mode the range is whatever the
checkpoint's running statistics leave, and nothing guards it: a checkpoint whose activations pass 65504 needs the
native-fp32 kernels (vx_config.conv_fp32 = 1, where eval mode takes the raw conv + vx_affine_gather route).

HIP path limits: every branch width and the stem/bottleneck widths must be multiples of 16 (true for the shipped W48
config: 48/96/192/384, 64/256, 720).  The SSN head (hrnet_config_ssn.yaml) returns a LowRankNormal2D: `sample` /
`sample_images` for the test split, and `lowres()` for values_amd.validation, which reduces the validation sums from the
1/4-resolution head without writing a sample (val_sums_ssn2d).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib


def _cfg_get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default) if hasattr(cfg, key) else (cfg[key] if key in cfg else default)


class _Block(nn.Module):
    """BasicBlock (expansion 1) / Bottleneck (expansion 4) parameter container (hrnet_module.py:44-119)."""

    def __init__(self, kind, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.kind, self.stride = kind, stride
        if kind == "BASIC":
            self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
            self.bn1 = nn.BatchNorm2d(planes)
            self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
            self.bn2 = nn.BatchNorm2d(planes)
        else:
            self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
            self.bn1 = nn.BatchNorm2d(planes)
            self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
            self.bn2 = nn.BatchNorm2d(planes)
            self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
            self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample


def _expansion(kind):
    return 1 if kind == "BASIC" else 4


def _make_layer(kind, inplanes, planes, blocks, stride=1):
    ds = None
    if stride != 1 or inplanes != planes * _expansion(kind):
        ds = nn.Sequential(nn.Conv2d(inplanes, planes * _expansion(kind), 1, stride, bias=False),
                           nn.BatchNorm2d(planes * _expansion(kind)))
    layers = [_Block(kind, inplanes, planes, stride, ds)]
    for _ in range(1, blocks):
        layers.append(_Block(kind, planes * _expansion(kind), planes))
    return nn.Sequential(*layers)


class _HRModule(nn.Module):
    """HighResolutionModule container: branches + fuse_layers (hrnet_module.py:122-306)."""

    def __init__(self, num_branches, kind, num_blocks, num_inchannels, num_channels, multi_scale_output=True):
        super().__init__()
        self.num_branches = num_branches
        self.kind = kind
        branches = []
        num_inchannels = list(num_inchannels)
        for i in range(num_branches):
            branches.append(_make_layer(kind, num_inchannels[i], num_channels[i], num_blocks[i]))
            num_inchannels[i] = num_channels[i] * _expansion(kind)
        self.branches = nn.ModuleList(branches)
        self.num_inchannels = num_inchannels
        self.fuse_layers = None
        if num_branches > 1:
            fuse = []
            for i in range(num_branches if multi_scale_output else 1):
                row = []
                for j in range(num_branches):
                    if j > i:
                        row.append(nn.Sequential(nn.Conv2d(num_inchannels[j], num_inchannels[i], 1, 1, 0, bias=False),
                                                 nn.BatchNorm2d(num_inchannels[i])))
                    elif j == i:
                        row.append(None)
                    else:
                        chain = []
                        for k in range(i - j):
                            last = k == i - j - 1
                            cout = num_inchannels[i] if last else num_inchannels[j]
                            mods = [nn.Conv2d(num_inchannels[j], cout, 3, 2, 1, bias=False), nn.BatchNorm2d(cout)]
                            if not last:
                                mods.append(nn.ReLU(inplace=True))
                            chain.append(nn.Sequential(*mods))
                        row.append(nn.Sequential(*chain))
                fuse.append(nn.ModuleList(row))
            self.fuse_layers = nn.ModuleList(fuse)


class _Act:
    """A channels-last activation: tensor [N, H, W, pitch] whose channels [0, C) are valid."""
    __slots__ = ("t", "C", "real_c")

    def __init__(self, t, c):
        self.t, self.C, self.real_c = t, c, c

    @property
    def N(self):
        return self.t.shape[0]

    @property
    def H(self):
        return self.t.shape[1]

    @property
    def W(self):
        return self.t.shape[2]

    @property
    def pitch(self):
        return self.t.shape[3]


def _r16(c: int) -> int:
    return (c + 15) // 16 * 16


def _rp(c: int) -> int:
    """pitch (floats per pixel) of an activation of c channels: the next multiple of 4, the channels beyond c zero.  The
    convolutions take Cin = round16(c) and read channels at and beyond the pitch as zeros (vx_conv2d_args.in_pitch), so
    HRNet-W18's 18-channel full-resolution branch moves 20 floats per pixel, not 32 (round 2's layout)."""
    return (c + 3) // 4 * 4


def _softmax_pitch(c: int) -> int:
    """pitch of the class logits: vx_bilinear_softmax_nchw keeps the C interpolated logits in registers only where a pixel
    holds ALL the channel quads of the instance that covers them (1, 2, 5 or 8).  9 .. 16 classes therefore travel at 20
    floats per pixel and 21 .. 28 at 32 (round4(C) would send them to the three-sweep scalar kernel); every other count at
    round4(C) as before (19 classes: 20).  The lanes beyond round4(C) are never written and never used."""
    q = (c + 3) // 4
    for inst in (1, 2, 5, 8):
        if q <= inst:
            return 4 * inst
    return 4 * q


def _pad_mask(m: torch.Tensor, dev) -> torch.Tensor:
    """(B, C, H, W) bool keep-mask -> channels-last uint8 with the channel padding of the activations"""
    t = m.to(dev).permute(0, 2, 3, 1).to(torch.uint8)
    c = t.shape[-1]
    if c % 4:
        t = torch.nn.functional.pad(t, (0, _rp(c) - c))
    return t.contiguous()


class LowRankNormal2D:
    """The distribution object of hrnet_ssn as test_2D.py:285-299 uses it: sample([n_pred]) -> (n, B, C*H*W).
    The rank-R combination is formed at the head's resolution and upsampled once per sample (bilinear interpolation
    is linear); the diagonal term uses interp(exp(mean)) + epsilon at full resolution (the reference takes
    `last_layer(x).exp()` for cov_diag, i.e. the SAME tensor as the mean, hrnet_module.py:560-568)."""

    def __init__(self, mean_lo: "_Act", fac_lo: "_Act", num_classes, rank, epsilon, size, seed):
        self._m, self._f = mean_lo, fac_lo
        self.num_classes, self.rank, self.epsilon, self.size = num_classes, rank, epsilon, size
        self._seed, self._draws = seed, 0

    def _up(self, t: torch.Tensor, pitch, n, out, dst):
        lib = _lib.load()
        h0, w0 = self._m.H, self._m.W
        _lib.check(lib.vx_bilinear_nchw(t.data_ptr(), pitch, n, h0, w0, self.num_classes, self.size[0], self.size[1],
                                        out.data_ptr(), _lib.ptr(dst), None, _lib.stream_ptr()), "vx_bilinear_nchw")

    @property
    def mean(self) -> torch.Tensor:
        B = self._m.N
        out = torch.empty((B, self.num_classes) + tuple(self.size), dtype=torch.float32, device=self._m.t.device)
        self._up(self._m.t, self._m.pitch, B, out, None)
        return out.reshape(B, -1)

    @classmethod
    def from_lowres(cls, mean: torch.Tensor, factor: Optional[torch.Tensor], num_classes: int, rank: int, epsilon: float, size,
                    seed: int = 0) -> "LowRankNormal2D":
        """the distribution of a head given as channels-last float32 device tensors: mean (B, h0, w0, pitch >= C), factor
        (B, h0, w0, pitch >= rank * C; channel r * C + c; None at rank 0), for the full-resolution size (H, W)"""
        if mean.dim() != 4 or mean.shape[3] < num_classes or mean.dtype != torch.float32 or not mean.is_contiguous():
            raise ValueError(f"LowRankNormal2D.from_lowres: mean (B, h0, w0, >= {num_classes}) contiguous float32 expected")
        if rank:
            if (factor is None or factor.dim() != 4 or tuple(factor.shape[:3]) != tuple(mean.shape[:3]) or factor.shape[3] < rank * num_classes
                    or factor.dtype != torch.float32 or not factor.is_contiguous()):
                raise ValueError(f"LowRankNormal2D.from_lowres: factor {tuple(mean.shape[:3])} + (>= {rank * num_classes},) contiguous float32 expected")
        return cls(_Act(mean, num_classes), _Act(factor, rank * num_classes) if rank else None, num_classes, rank, epsilon,
                   (int(size[0]), int(size[1])), seed)

    def next_seed(self) -> int:
        """the seed of this distribution's next draw (sample_images and validation.val_sums_ssn2d take it when none is
        given, so the materialised and the fused route see the same normals)"""
        seed = (self._seed * 7919 + self._draws) & 0xFFFFFFFF
        self._draws += 1
        return seed

    def lowres(self) -> dict:
        """the head at its own resolution, as vx_ssn2d_lowres / vx_val_ssn2d_sums_batched take it: channels-last tensors
        "mean" (B, h0, w0, mean_pitch) and "factor" (B, h0, w0, factor_pitch; channel r * C + c; None at rank 0), their
        pitches, and the sizes B, h0, w0, H, W"""
        R = self.rank
        return {"mean": self._m.t, "mean_pitch": self._m.pitch, "factor": self._f.t if R else None,
                "factor_pitch": self._f.pitch if R else 0, "B": self._m.N, "h0": self._m.H, "w0": self._m.W,
                "H": int(self.size[0]), "W": int(self.size[1])}

    def sample_images(self, n: int, eps_w=None, eps_d=None, seed: Optional[int] = None) -> torch.Tensor:
        """(B, n, C, H, W) logit samples (per-image stacks, the layout process_output_2d reads)."""
        lib = _lib.load()
        dev = self._m.t.device
        B, C, R = self._m.N, self.num_classes, self.rank
        h0, w0 = self._m.H, self._m.W
        H, W = self.size
        pix = h0 * w0
        if seed is None:
            seed = self.next_seed()
        hold = []
        pw = pd = None
        if eps_w is not None:
            ew = eps_w.to(device=dev, dtype=torch.float32).contiguous(); hold.append(ew); pw = ew.data_ptr()
        if eps_d is not None:
            ed = eps_d.to(device=dev, dtype=torch.float32).contiguous(); hold.append(ed); pd = ed.data_ptr()
        comb = torch.empty((n, B * pix, C), dtype=torch.float32, device=dev)
        expm = torch.empty((B * pix, C), dtype=torch.float32, device=dev)
        _lib.check(lib.vx_ssn2d_lowres(self._m.t.data_ptr(), self._m.pitch, self._f.t.data_ptr() if R else None,
                                       self._f.pitch if R else 0, pw, int(seed) & 0xFFFFFFFF, B, pix, n, C, R,
                                       comb.data_ptr(), expm.data_ptr(), _lib.stream_ptr()), "vx_ssn2d_lowres")
        out = torch.empty((B, n, C, H, W), dtype=torch.float32, device=dev)
        for s in range(n):   # image b of sample s -> slot b * n + s
            dst = torch.arange(B, dtype=torch.int32, device=dev) * n + s
            hold.append(dst)
            self._up(comb[s], C, B, out, dst)
        diag = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
        self._up(expm, C, B, diag, None)
        _lib.check(lib.vx_ssn2d_add_diag(out.data_ptr(), diag.data_ptr(), pd, int(seed) & 0xFFFFFFFF, n, B, C * H * W,
                                         float(self.epsilon), _lib.stream_ptr()), "vx_ssn2d_add_diag")
        self._hold = hold + [comb, expm, diag]
        return out

    def sample(self, sample_shape=(1,), **kw) -> torch.Tensor:
        n = int(sample_shape[0]) if len(sample_shape) else 1
        v = self.sample_images(n, **kw)
        return v.transpose(0, 1).reshape(n, v.shape[0], -1)

    rsample = sample


class HighResolutionNet(nn.Module):
    def __init__(self, config, **kwargs):
        super().__init__()
        model_cfg = _cfg_get(config, "MODEL")
        extra = _cfg_get(model_cfg, "EXTRA")
        if _cfg_get(model_cfg, "ALIGN_CORNERS", False):
            raise NotImplementedError("values_amd.HighResolutionNet: ALIGN_CORNERS must be False (every shipped config)")
        self.ssn = bool(_cfg_get(model_cfg, "SSN", False))          # hrnet_module.py:430-435
        if self.ssn:
            self.rank = int(_cfg_get(model_cfg, "SSN_RANK"))
            self.epsilon = float(_cfg_get(model_cfg, "SSN_EPS"))
        self.num_classes = int(_cfg_get(_cfg_get(config, "DATASET"), "NUM_CLASSES"))
        self.in_channels = int(_cfg_get(model_cfg, "INPUT_CHANNELS", 3))
        self.extra = {k: (dict(v) if hasattr(v, "keys") else v) for k, v in dict(extra).items()}
        self.conv1 = nn.Conv2d(self.in_channels, 64, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.conv2 = nn.Conv2d(64, 64, 3, 2, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(64)
        s1 = self.extra["STAGE1"]
        self.layer1 = _make_layer(s1["BLOCK"], 64, s1["NUM_CHANNELS"][0], s1["NUM_BLOCKS"][0])
        pre = [_expansion(s1["BLOCK"]) * s1["NUM_CHANNELS"][0]]
        for si in (2, 3, 4):
            cfg = self.extra[f"STAGE{si}"]
            chans = [c * _expansion(cfg["BLOCK"]) for c in cfg["NUM_CHANNELS"]]
            setattr(self, f"transition{si - 1}", self._make_transition(pre, chans))
            mods, inch = [], chans
            for _ in range(cfg["NUM_MODULES"]):
                m = _HRModule(cfg["NUM_BRANCHES"], cfg["BLOCK"], cfg["NUM_BLOCKS"], inch, cfg["NUM_CHANNELS"], True)
                mods.append(m)
                inch = m.num_inchannels
            setattr(self, f"stage{si}", nn.Sequential(*mods))
            pre = inch
        self.dropout_final = bool(self.extra.get("DROPOUT_FINAL", False))
        last = int(sum(pre))
        k = int(self.extra.get("FINAL_CONV_KERNEL", 1))
        if k != 1:
            raise NotImplementedError("values_amd.HighResolutionNet: FINAL_CONV_KERNEL must be 1 (every shipped config)")
        self.last_layer = nn.Sequential(nn.Conv2d(last, last, 1), nn.BatchNorm2d(last), nn.ReLU(inplace=True),
                                        nn.Conv2d(last, self.num_classes, 1))
        if self.ssn:   # hrnet_module.py:436-453
            self.cov_factor_conv = nn.Sequential(nn.Conv2d(last, last, 1), nn.BatchNorm2d(last), nn.ReLU(inplace=True),
                                                 nn.Conv2d(last, self.num_classes * self.rank, 1))
        # widths that are not multiples of 16 (HRNet-W18: 18/36/72/144, 270 concatenated) run zero-padded: every
        # activation tensor has round16(C) channels whose tail is exactly 0 (zero weight rows, zero BN scale/shift)
        self._last_parts = list(pre)
        self._packed, self._packed_key = None, None
        self._affine, self._affine_key, self._affine_hold = None, None, None   # eval mode: _ensure_affine
        self._ev = False       # the forward in flight runs in eval mode (running statistics)
        self._zcache = {}      # persistent zero-padded buffers (see _conv): (layer, device, stream) -> (geometry, tensor)
        self._zreal = {}       # layer -> real channel count of its padded output (zero_tails_intact)
        self._groups = 1       # statistics groups of the forward in flight (forward_samples)
        self.seed, self._calls = 123, 0

    def zero_tails_intact(self) -> bool:
        """Debug check of the invariant the persistent zero-padded buffers rely on: no kernel ever wrote channels at or
        beyond the real channel count of a padded tensor (reads them back: synchronises)."""
        for key, (geo, t) in self._zcache.items():
            if key[0] == "bn":
                continue
            real = self._zreal.get(key[0])
            if real is not None and real < t.shape[-1] and bool((t[..., real:] != 0).any().item()):
                return False
        return True

    @staticmethod
    def _make_transition(pre, cur):
        layers = []
        for i in range(len(cur)):
            if i < len(pre):
                if cur[i] != pre[i]:
                    layers.append(nn.Sequential(nn.Conv2d(pre[i], cur[i], 3, 1, 1, bias=False), nn.BatchNorm2d(cur[i]),
                                                nn.ReLU(inplace=True)))
                else:
                    layers.append(None)
            else:
                chain = []
                for j in range(i + 1 - len(pre)):
                    cout = cur[i] if j == i - len(pre) else pre[-1]
                    chain.append(nn.Sequential(nn.Conv2d(pre[-1], cout, 3, 2, 1, bias=False), nn.BatchNorm2d(cout),
                                               nn.ReLU(inplace=True)))
                layers.append(nn.Sequential(*chain))
        return nn.ModuleList(layers)

    # ------------------------------------------------------------------ weights
    def _ensure_packed(self, dev):
        key = tuple((p.data_ptr(), p._version, str(p.device)) for p in self.parameters()) + (_lib.pack_mode(),)
        if self._packed is not None and self._packed_key == key:
            return self._packed
        lib = _lib.load()
        st = _lib.stream_ptr()
        packed = {}
        for name, mod in self.named_modules():
            if isinstance(mod, nn.Conv2d):
                w = mod.weight.detach().to(dev, torch.float32).contiguous()
                if name in ("last_layer.0", "cov_factor_conv.0") and any(c % 4 for c in self._last_parts):
                    # the head reads the concat of the four PADDED stage-4 tensors: spread the input channels
                    wpad = torch.zeros((w.shape[0], sum(_rp(c) for c in self._last_parts)) + tuple(w.shape[2:]),
                                       dtype=torch.float32, device=dev)
                    src = dst = 0
                    for c in self._last_parts:
                        wpad[:, dst:dst + c] = w[:, src:src + c]
                        src += c
                        dst += _rp(c)
                    w = wpad.contiguous()
                cout, cin, ks, _ = w.shape
                wp = torch.empty(lib.vx_conv2d_packed_floats(cin, cout, ks), dtype=torch.float32, device=dev)
                _lib.check(lib.vx_pack_conv2d(_lib.ptr(w), _lib.ptr(wp), cin, cout, ks, st), "vx_pack_conv2d")
                b = None
                if mod.bias is not None:
                    b = torch.zeros((cout + 15) // 16 * 16, dtype=torch.float32, device=dev)  # readable per 16-row tile
                    b[:cout] = mod.bias.detach().to(dev, torch.float32)
                packed[name] = (wp, b, cin, cout, ks, mod.stride[0], w, lib.vx_conv2d_family(cin, cout, ks))
            elif isinstance(mod, nn.BatchNorm2d):
                packed[name] = (mod.weight.detach().to(dev, torch.float32).contiguous(),
                                mod.bias.detach().to(dev, torch.float32).contiguous())
        self._packed, self._packed_key = packed, key
        return packed

    # ------------------------------------------------------------------ kernel wrappers
    def _conv(self, x: _Act, name, stats=True, pre=None, out_pitch=None, epi=None, tail=None):
        """pre = (scale, shift): `x` is the RAW output of the previous conv and relu(x * scale + shift) -- its training-mode
        BatchNorm + ReLU -- is applied while this conv stages its tiles (vx_conv2d_args.in_scale): the affine pass that
        would write the activated tensor (and the read of it) disappear.
        epi = (scale, shift, add, relu): eval mode, the running-statistics BatchNorm, the residual `add` (an _Act or None)
        and the ReLU applied as the conv stores (vx_conv2d_args.out_scale).  tail: the output feeds another conv, so a
        width that is no multiple of 4 goes to the layer's zero-tailed buffer (default: as `stats`)."""
        if tail is None:
            tail = stats
        lib = _lib.load()
        wp, b, cin, cout, ks, stride, _w, fam = self._pk[name]
        cin_pad = (cin + 15) // 16 * 16
        assert x.C == _rp(cin) or x.C == cin, (name, x.C, cin)
        n, h, w = x.N, x.H, x.W
        oh = (h + 2 * (ks // 2) - ks) // stride + 1
        ow = (w + 2 * (ks // 2) - ks) // stride + 1
        pitch = (cout + 3) // 4 * 4
        if cout % 4 and tail:       # feeds another conv: the channels [cout, round4(cout)) stay zero (see __init__)
            pitch = _rp(cout)
            # the conv writes channels [0, round4(cout)) only, so the zero tail survives from forward to forward: one
            # buffer per layer and geometry, zero-filled once (a fill kernel per conv launch was the top entry of the
            # W18 profile)
            # ONE geometry per (layer, stream): another batch size / image size replaces the entry instead of piling a
            # second set of activation-sized buffers on top (a captured graph keeps its own references, _hold_last)
            key = (name, str(x.t.device), torch.cuda.current_stream().cuda_stream)
            geo = (n, oh, ow, pitch)
            hit = self._zcache.get(key)
            if hit is None or hit[0] != geo:
                hit = self._zcache[key] = (geo, _lib.zeros(geo, dtype=torch.float32, device=x.t.device))
            self._zreal[name] = cout
            out = hit[1]
        else:
            if out_pitch is not None:       # (the class logits: _softmax_pitch)
                assert out_pitch % 4 == 0 and out_pitch >= pitch
                pitch = out_pitch
            out = torch.empty((n, oh, ow, pitch), dtype=torch.float32, device=x.t.device)
        part = None
        a = _lib.Conv2dArgs()
        a.w_family = fam
        a.in_ = x.t.data_ptr(); a.in_pitch = x.pitch; a.w_packed = wp.data_ptr()
        a.bias = b.data_ptr() if b is not None else None
        a.out = out.data_ptr(); a.out_pitch = pitch; a.out_coff = 0
        a.N, a.H, a.W, a.Cin, a.Cout, a.KS, a.S = n, h, w, cin_pad, cout, ks, stride
        ntiles = n * lib.vx_conv2d_tiles(h, w, ks, stride)
        if stats:
            part = torch.empty((ntiles, cout, 2), dtype=torch.float32, device=x.t.device)
            a.stats_partial = part.data_ptr()
        if pre is not None:
            scale, shift = pre
            a.in_scale, a.in_shift, a.in_relu = scale.data_ptr(), shift.data_ptr(), 1
            a.in_cpitch = x.C                                   # rows of scale / shift [G][C] (C = the padded channel count)
            a.in_group_images = (n // self._groups) if self._groups > 1 else 0
        if epi is not None:
            e_scale, e_shift, e_add, e_relu = epi
            a.out_scale, a.out_shift = e_scale.data_ptr(), e_shift.data_ptr()
            a.out_act = _lib.VX_ACT_RELU if e_relu else _lib.VX_ACT_NONE
            if e_add is not None:
                assert (e_add.N, e_add.H, e_add.W) == (n, oh, ow) and e_add.pitch >= _rp(cout), name
                a.out_add, a.out_add_pitch = e_add.t.data_ptr(), e_add.pitch
        prof = getattr(self, "_prof", None)
        if prof is not None:       # diagnostic (profile_forward): a HIP event pair around the launch, on its stream
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream())
        _lib.check(lib.vx_conv2d(C.byref(a), self._st), "vx_conv2d " + name)
        if prof is not None:
            e1.record(torch.cuda.current_stream())
            prof.append((lib.vx_last_kernel_name().decode(), 2.0 * ks * ks * cin * cout * n * oh * ow,
                         4.0 * (n * h * w * cin + n * oh * ow * cout + ks * ks * cin * cout), e0, e1))
        self._hold += [out, part]
        act = _Act(out, pitch if (cout % 4 and tail) else cout)
        act.real_c = cout
        return act, part, ntiles

    def _conv_bn(self, x: _Act, conv_name, bn_name, pre=None):
        lib = _lib.load()
        raw, part, ntiles = self._conv(x, conv_name, pre=pre)
        gamma, beta = self._pk[bn_name]
        creal = raw.real_c
        G = self._groups
        if creal != raw.C:      # padded channels: scale = shift = 0 there, written once (the finalize kernel fills [0, creal))
            key = ("bn", bn_name, str(raw.t.device), torch.cuda.current_stream().cuda_stream)
            geo = (2, G, raw.C)
            hit = self._zcache.get(key)
            if hit is None or hit[0] != geo:
                hit = self._zcache[key] = (geo, _lib.zeros(geo, dtype=torch.float32, device=raw.t.device))
            ss = hit[1]
        else:
            ss = torch.empty((2, G, raw.C), dtype=torch.float32, device=raw.t.device)
        scale, shift = ss[0], ss[1]
        # G statistics groups of N / G consecutive images each (the TTA views of one batched forward; G = 1: plain BatchNorm)
        _lib.check(lib.vx_bn_finalize_groups(_lib.ptr(part), ntiles // G, G, creal, raw.C, (raw.N // G) * raw.H * raw.W, 1e-5,
                                             _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(scale), _lib.ptr(shift), self._st),
                   "vx_bn_finalize " + bn_name)
        self._hold += [ss]
        return raw, scale, shift

    def _fold(self) -> bool:
        import os
        return _lib.get_config().conv_fp32 == 0 and not os.environ.get("VX_HRNET_NO_FOLD")

    def _conv_bn_after(self, r, conv_name, bn_name):
        """conv + BatchNorm statistics of relu(bn(r)): r = (raw, scale, shift) of the previous conv"""
        if self._fold():
            return self._conv_bn(r[0], conv_name, bn_name, pre=(r[1], r[2]))
        return self._conv_bn(self._aff(r[0], r[1], r[2], relu=True), conv_name, bn_name)

    # ------------------------------------------------------------------ eval mode: running statistics
    def _ensure_affine(self, dev):
        """model.eval(): every BatchNorm is the per-channel affine of its RUNNING statistics, known before the forward
        starts.  One table for the whole model -- per layer a scale row and a shift row of round4(C) floats, the tail
        zero -- written by ONE vx_bn_running_affine launch, rebuilt when a parameter or a running buffer changes
        (load_state_dict bumps their versions).  Built by the first eval forward, i.e. before any graph capture (graphed()
        and GraphedPredictor2D warm up eagerly)."""
        bns = [(n, m) for n, m in self.named_modules() if isinstance(m, nn.BatchNorm2d)]
        for n, m in bns:
            if m.running_mean is None or m.running_var is None:
                raise ValueError(f"eval mode needs running statistics: {n} tracks none (track_running_stats=False)")
        key = self._packed_key + tuple((b.data_ptr(), b._version, str(b.device)) for _, m in bns
                                       for b in (m.running_mean, m.running_var)) + (str(dev),)
        if self._affine is not None and self._affine_key == key:
            return self._affine
        eps = {float(m.eps) for _, m in bns}
        if len(eps) != 1:
            raise NotImplementedError("values_amd.HighResolutionNet: the BatchNorm layers must share one eps")
        rows = torch.empty(sum(2 * _rp(m.num_features) for _, m in bns), dtype=torch.float32, device=dev)
        items = (_lib.BnAffineItem * len(bns))()
        tab, hold, off = {}, [], 0
        for k, (n, m) in enumerate(bns):
            c, cp = m.num_features, _rp(m.num_features)
            gamma, beta = self._pk[n]
            mean = m.running_mean.detach().to(dev, torch.float32).contiguous()
            var = m.running_var.detach().to(dev, torch.float32).contiguous()
            hold += [mean, var]
            sc, sh = rows[off:off + cp], rows[off + cp:off + 2 * cp]
            off += 2 * cp
            it = items[k]
            it.gamma, it.beta, it.running_mean, it.running_var = gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr()
            it.scale, it.shift, it.C, it.cpitch = sc.data_ptr(), sh.data_ptr(), c, cp
            tab[n] = (sc, sh)
        dtab = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev)
        _lib.check(_lib.load().vx_bn_running_affine(_lib.ptr(dtab), len(bns), eps.pop(), _lib.stream_ptr()),
                   "vx_bn_running_affine")
        # the launch reads the statistics and the item table in stream order: keep them until the next rebuild
        self._affine, self._affine_key, self._affine_hold = tab, key, (rows, dtab, hold)
        return tab

    def _cba(self, x: _Act, conv_name, bn_name, relu, add: Optional[_Act] = None) -> _Act:
        """eval mode: act(add + bn(conv(x))) with the running statistics.  Split-fp16 path: in the conv's epilogue, nothing
        else is launched.  VX_HRNET_NO_FOLD=1 / conv_fp32 = 1: the raw conv, then vx_affine_gather fed from the table
        (the same bits: vx_conv2d_args.out_scale)."""
        sc, sh = self._affine[bn_name]
        if self._fold():
            return self._conv(x, conv_name, stats=False, tail=True, epi=(sc, sh, add, relu))[0]
        raw = self._conv(x, conv_name, stats=False, tail=True)[0]
        return self._aff(raw, sc, sh, relu=relu, add=add)

    def _aff(self, x: _Act, scale=None, shift=None, relu=False, add: Optional[_Act] = None, out: Optional[_Act] = None,
               out_coff=0, size=None, drop=None):
        lib = _lib.load()
        oh, ow = size if size is not None else (x.H, x.W)
        if out is None:
            out = _Act(torch.empty((x.N, oh, ow, x.C), dtype=torch.float32, device=x.t.device), x.C)
        a = _lib.AffineArgs()
        a.x = x.t.data_ptr(); a.x_pitch = x.pitch
        if scale is not None:
            a.scale = scale.data_ptr(); a.shift = shift.data_ptr()
            if self._groups > 1:
                a.group_images = x.N // self._groups
        if add is not None:
            a.add = add.t.data_ptr(); a.add_pitch = add.pitch
        a.out = out.t.data_ptr(); a.out_pitch = out.pitch; a.out_coff = out_coff
        a.N, a.H, a.W, a.C, a.OH, a.OW = x.N, x.H, x.W, x.C, oh, ow
        a.act = _lib.VX_ACT_RELU if relu else _lib.VX_ACT_NONE
        if drop is not None:
            mode, seed, layer, mask = drop
            a.drop_mode, a.drop_seed, a.drop_layer = mode, seed & 0xFFFFFFFF, layer
            if mask is not None:
                a.drop_mask = mask.data_ptr()
        _lib.check(lib.vx_affine_gather(C.byref(a), self._st), "vx_affine_gather")
        self._hold.append(out.t)
        return out

    def _itensor(self, values, dev):
        """small int32 index tensor (slot / flip tables), uploaded once per content: a hipGraph capture cannot contain the
        synchronous host-to-device copy torch.tensor(list, device=...) makes"""
        cache = self.__dict__.setdefault("_icache", {})
        key = (tuple(int(v) for v in values), str(dev))
        t = cache.get(key)
        if t is None:
            t = cache[key] = torch.tensor(list(key[0]), dtype=torch.int32, device=dev)
        return t

    def _streams(self, n):
        # the pool only ever GROWS: stage 2's two streams are the first two of stage 4's four, so a layer sees the same
        # stream in every forward (its persistent zero-padded buffer is keyed on it)
        if not hasattr(self, "_side"):
            self._side = []
        while len(self._side) < n:
            self._side.append(torch.cuda.Stream())
        return self._side

    # ------------------------------------------------------------------ network walk
    def _block(self, x: _Act, p: str, blk: _Block) -> _Act:
        # relu(bn(conv)) feeding the next conv of the block is never written: that conv applies it on load (FOLD; the
        # separate affine pass remains behind VX_HRNET_NO_FOLD=1 for A/B and for the native-fp32 kernels)
        if self._ev:     # running statistics: every conv finishes its BatchNorm (+ residual, ReLU) itself (_cba)
            res = x if blk.downsample is None else self._cba(x, p + ".downsample.0", p + ".downsample.1", relu=False)
            a = self._cba(x, p + ".conv1", p + ".bn1", relu=True)
            if blk.kind == "BASIC":
                return self._cba(a, p + ".conv2", p + ".bn2", relu=True, add=res)
            a = self._cba(a, p + ".conv2", p + ".bn2", relu=True)
            return self._cba(a, p + ".conv3", p + ".bn3", relu=True, add=res)
        if blk.kind == "BASIC":
            r1 = self._conv_bn(x, p + ".conv1", p + ".bn1")
            r2 = self._conv_bn_after(r1, p + ".conv2", p + ".bn2")
        else:
            r1 = self._conv_bn(x, p + ".conv1", p + ".bn1")
            rm = self._conv_bn_after(r1, p + ".conv2", p + ".bn2")
            r2 = self._conv_bn_after(rm, p + ".conv3", p + ".bn3")
        res = x
        if blk.downsample is not None:
            rd = self._conv_bn(x, p + ".downsample.0", p + ".downsample.1")
            res = self._aff(rd[0], rd[1], rd[2], relu=False)
        return self._aff(r2[0], r2[1], r2[2], relu=True, add=res)  # out = relu(bn(conv) + residual), :72-75 / :114-117

    def _module(self, xs: List[_Act], p: str, mod: _HRModule) -> List[_Act]:
        xs = list(xs)
        # the branches of a module are independent until the fusion: run them on separate HIP streams so the
        # low-resolution branches (a few dozen workgroups per launch) fill the chip together with the wide ones
        import os
        main = torch.cuda.current_stream()
        multi = mod.num_branches > 1 and not os.environ.get("VX_HRNET_SINGLE_STREAM")
        side = self._streams(mod.num_branches) if multi else [main] * mod.num_branches
        for i in range(mod.num_branches):
            st = side[i]
            if st is not main:
                st.wait_stream(main)
            with torch.cuda.stream(st):
                self._st = C.c_void_p(st.cuda_stream)
                for b, blk in enumerate(mod.branches[i]):
                    xs[i] = self._block(xs[i], f"{p}.branches.{i}.{b}", blk)
        self._st = C.c_void_p(main.cuda_stream)
        for i in range(mod.num_branches):
            if side[i] is not main:
                main.wait_stream(side[i])
        if mod.num_branches == 1:
            return xs
        outs = []
        nb = mod.num_branches
        multifuse = nb <= 4 and not os.environ.get("VX_HRNET_NO_MULTIFUSE")
        for i in range(len(mod.fuse_layers)):
            if self._ev:
                # the reference's order: upsample(bn(conv(x))) -- the affine at the term's own resolution (in its conv), then
                # the terms enter the sum with null scale / shift
                terms = []
                for j in range(nb):
                    t = xs[j]
                    if j > i:
                        q = f"{p}.fuse_layers.{i}.{j}"
                        t = self._cba(t, q + ".0", q + ".1", relu=False)
                    elif j < i:
                        for k in range(i - j):
                            q = f"{p}.fuse_layers.{i}.{j}.{k}"
                            t = self._cba(t, q + ".0", q + ".1", relu=k < i - j - 1)
                    terms.append((t, None, None))
                if multifuse:
                    outs.append(self._fuse(terms, xs[i]))
                    continue
                size = (xs[i].H, xs[i].W)    # term by term (vx_fuse_sum states itself as this chain)
                y = terms[0][0] if (terms[0][0].H, terms[0][0].W) == size else self._aff(terms[0][0], size=size)
                for k in range(1, nb):
                    y = self._aff(terms[k][0], relu=k == nb - 1, add=y, size=size)
                outs.append(y)
                continue
            if multifuse:
                # Round 4: all terms of output i in ONE pass (vx_fuse_sum) -- the term-by-term chain below re-read and
                # re-wrote the accumulator once per term (three passes over the full-resolution branch per stage-4 module)
                terms = []
                for j in range(nb):
                    if j == i:
                        terms.append((xs[j], None, None))
                    elif j > i:
                        q = f"{p}.fuse_layers.{i}.{j}"
                        r = self._conv_bn(xs[j], q + ".0", q + ".1")
                        terms.append(r)
                    else:
                        t = xs[j]
                        r = None
                        for k in range(i - j):
                            q = f"{p}.fuse_layers.{i}.{j}.{k}"
                            r = self._conv_bn(t, q + ".0", q + ".1") if r is None else self._conv_bn_after(r, q + ".0", q + ".1")
                        terms.append(r)
                outs.append(self._fuse(terms, xs[i]))
                continue
            y: Optional[_Act] = None
            for j in range(nb):
                last = j == nb - 1
                if j == i:
                    if y is None:
                        y = xs[j]  # i == 0: the sum starts from x[0] itself (never written: later terms go to a new buffer)
                        if last:
                            y = self._aff(xs[j], relu=True)
                        continue
                    term = (xs[j], None, None, None)
                elif j > i:
                    q = f"{p}.fuse_layers.{i}.{j}"
                    r = self._conv_bn(xs[j], q + ".0", q + ".1")
                    term = (r[0], r[1], r[2], (xs[i].H, xs[i].W))
                else:
                    t = xs[j]
                    r = None
                    for k in range(i - j):
                        q = f"{p}.fuse_layers.{i}.{j}.{k}"
                        r = self._conv_bn(t, q + ".0", q + ".1") if r is None else self._conv_bn_after(r, q + ".0", q + ".1")
                    term = (r[0], r[1], r[2], None)
                if y is None:
                    y = self._aff(term[0], term[1], term[2], relu=last, size=term[3])
                else:
                    fresh = y is xs[0] and i == 0
                    y = self._aff(term[0], term[1], term[2], relu=last, add=y, out=None if fresh else y, size=term[3])
            outs.append(y)
        return outs

    def _fuse(self, terms, like: _Act) -> _Act:
        """relu(T_0 + T_1 + ...) in term order, T = (raw, scale, shift) of a conv + BatchNorm (upsampled to `like`'s size where
        it is smaller) or (x, None, None) for the identity term: vx_fuse_sum, one pass"""
        lib = _lib.load()
        out = _Act(torch.empty((like.N, like.H, like.W, like.C), dtype=torch.float32, device=like.t.device), like.C)
        a = _lib.FuseArgs()
        a.nterms = len(terms)
        for k, (x, sc, sh) in enumerate(terms):
            a.term[k].x = x.t.data_ptr(); a.term[k].x_pitch = x.pitch; a.term[k].H = x.H; a.term[k].W = x.W
            if sc is not None:
                a.term[k].scale = sc.data_ptr(); a.term[k].shift = sh.data_ptr()
        a.out = out.t.data_ptr(); a.out_pitch = out.pitch
        a.N, a.OH, a.OW, a.C = like.N, like.H, like.W, like.C
        a.act = _lib.VX_ACT_RELU
        if self._groups > 1:
            a.group_images = like.N // self._groups
        _lib.check(lib.vx_fuse_sum(C.byref(a), self._st), "vx_fuse_sum")
        self._hold.append(out.t)
        return out

    def _transition(self, ys: List[_Act], tname: str, layers) -> List[_Act]:
        n_prev = len(ys)
        out = []
        for i, tl in enumerate(layers):
            if i < n_prev:
                if tl is None:
                    out.append(ys[i])
                elif self._ev:
                    out.append(self._cba(ys[i], f"{tname}.{i}.0", f"{tname}.{i}.1", relu=True))
                else:
                    r = self._conv_bn(ys[i], f"{tname}.{i}.0", f"{tname}.{i}.1")
                    out.append(self._aff(r[0], r[1], r[2], relu=True))
            elif self._ev:
                t = ys[-1]
                for j in range(len(tl)):
                    t = self._cba(t, f"{tname}.{i}.{j}.0", f"{tname}.{i}.{j}.1", relu=True)
                out.append(t)
            else:
                r = None
                for j in range(len(tl)):
                    nm = f"{tname}.{i}.{j}"
                    r = self._conv_bn(ys[-1], nm + ".0", nm + ".1") if r is None else self._conv_bn_after(r, nm + ".0", nm + ".1")
                out.append(self._aff(r[0], r[1], r[2], relu=True))
        return out

    def _backbone(self, x: torch.Tensor, nhwc: bool = False) -> List[_Act]:
        if nhwc:
            cin = self.in_channels
            xin = x
        else:
            n, cin, h, w = x.shape
            if cin != self.in_channels:
                raise ValueError(f"expected {self.in_channels} input channels, got {cin}")
            xin = _lib.zeros((n, h, w, _rp(cin)), dtype=torch.float32, device=x.device)   # channels-last, pitch round4(cin)
            xin[..., :cin] = x.permute(0, 2, 3, 1)
        self._hold.append(xin)
        a = _Act(xin, _rp(cin))
        if self._ev:
            a = self._cba(self._cba(a, "conv1", "bn1", relu=True), "conv2", "bn2", relu=True)
        else:
            r = self._conv_bn(a, "conv1", "bn1")
            r = self._conv_bn_after(r, "conv2", "bn2")
            a = self._aff(r[0], r[1], r[2], relu=True)
        for b, blk in enumerate(self.layer1):
            a = self._block(a, f"layer1.{b}", blk)
        ys = [a]
        for si in (2, 3, 4):
            xs = self._transition(ys, f"transition{si - 1}", getattr(self, f"transition{si - 1}"))
            for m, mod in enumerate(getattr(self, f"stage{si}")):
                xs = self._module(xs, f"stage{si}.{m}", mod)
            ys = xs
        return ys

    def _head_lowres(self, feats: List[_Act], drop_mode, seed, masks, device):
        """concat of the four (dropped, upsampled) stage-4 outputs -> last_layer [and cov_factor_conv] at 1/4 resolution"""
        n, h0, w0 = feats[0].N, feats[0].H, feats[0].W
        ctot = sum(f.C for f in feats)
        cat = _Act(torch.empty((n, h0, w0, ctot), dtype=torch.float32, device=device), ctot)
        off = 0
        for k, f in enumerate(feats):
            drop = None
            if drop_mode != _lib.VX_DROP_NONE:
                drop = (drop_mode, seed, k, None if masks is None else masks[k])
            self._aff(f, out=cat, out_coff=off, size=(h0, w0), drop=drop)
            off += f.C
        outs = []
        for head in (("last_layer",) + (("cov_factor_conv",) if self.ssn else ())):
            if self._ev:
                outs.append(self._conv(self._cba(cat, head + ".0", head + ".1", relu=True), head + ".3", stats=False)[0])
                continue
            r = self._conv_bn(cat, head + ".0", head + ".1")
            if self._fold():
                raw, _, _ = self._conv(r[0], head + ".3", stats=False, pre=(r[1], r[2]))
            else:
                raw, _, _ = self._conv(self._aff(r[0], r[1], r[2], relu=True), head + ".3", stats=False)
            outs.append(raw)
        return outs

    def _head(self, feats: List[_Act], out: torch.Tensor, size, dst, flip, drop_mode, seed, masks, softmax=False):
        lib = _lib.load()
        n, h0, w0 = feats[0].N, feats[0].H, feats[0].W
        ctot = sum(f.C for f in feats)
        cat = _Act(torch.empty((n, h0, w0, ctot), dtype=torch.float32, device=out.device), ctot)
        off = 0
        for k, f in enumerate(feats):
            drop = None
            if drop_mode != _lib.VX_DROP_NONE:
                drop = (drop_mode, seed, k, None if masks is None else masks[k])
            self._aff(f, out=cat, out_coff=off, size=(h0, w0), drop=drop)   # dropout -> bilinear -> concat slot
            off += f.C
        if self._ev:
            raw, _, _ = self._conv(self._cba(cat, "last_layer.0", "last_layer.1", relu=True), "last_layer.3", stats=False,
                                   out_pitch=_softmax_pitch(self.num_classes))
        elif self._fold():
            r = self._conv_bn(cat, "last_layer.0", "last_layer.1")
            raw, _, _ = self._conv(r[0], "last_layer.3", stats=False, pre=(r[1], r[2]), out_pitch=_softmax_pitch(self.num_classes))
        else:
            r = self._conv_bn(cat, "last_layer.0", "last_layer.1")
            raw, _, _ = self._conv(self._aff(r[0], r[1], r[2], relu=True), "last_layer.3", stats=False,
                                   out_pitch=_softmax_pitch(self.num_classes))
        # softmax: `out` receives F.softmax(dim=1) of the upsampled logits (what test_2D.py:300-303 takes of every forward)
        # in the same pass; the full-resolution logits are not written
        fn = lib.vx_bilinear_softmax_nchw if softmax else lib.vx_bilinear_nchw
        _lib.check(fn(_lib.ptr(raw.t), raw.pitch, n, h0, w0, self.num_classes, size[0], size[1],
                      _lib.ptr(out), _lib.ptr(dst), _lib.ptr(flip), self._st), "vx_bilinear_nchw")

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def forward_samples(self, x: torch.Tensor, n_samples: int = 1, dropout_masks: Optional[Sequence] = None,
                        seeds: Optional[Sequence[int]] = None, hflip_back: bool = False,
                        out: Optional[torch.Tensor] = None, slot_stride: int = 0, slot_offset: int = 0,
                        vflip_back: bool = False, groups: int = 1, group_flips: Optional[Sequence[int]] = None,
                        softmax_out: bool = False, nhwc: bool = False) -> torch.Tensor:
        """(n_samples, B, C, H, W) logits (softmax_out: their class softmax instead, computed in the
        upsampling pass): backbone once, DROPOUT_FINAL head per sample.  dropout_masks:
        [sample][4] keep-masks (B, C_k, H_k, W_k) bool (parity tests).  hflip_back: un-flip the output along W
        (a HorizontalFlip TTA view, test_2D.py:304-309); vflip_back: along H (VerticalFlip, the 8-view extension).
        nhwc: x is (N, H, W, 4) channels-last at the stem's pitch with channel 3 zero -- what vx_tta_views_2d writes
        (values_amd.data.tta_views_2d_device): staged as it is, no permute / zero-fill copies."""
        _lib.require_gpu()
        dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
        x = x.detach().to(dev, torch.float32)
        self._pk = self._ensure_packed(dev)
        self._ev = not self.training
        if self._ev:
            self._ensure_affine(dev)
        self._st = _lib.stream_ptr()
        # the previous forward's intermediates were kept until now (its kernels are enqueued ahead of everything this call
        # launches, on streams this call joins before reusing memory): release them BEFORE allocating this forward's, or two
        # forwards' worth of activations are alive at once (W48 at 32 views: ~2 x 150 GB)
        self._hold_last = None
        self._hold = []
        if nhwc:
            if x.dim() != 4 or x.shape[-1] != _rp(self.in_channels) or not x.is_contiguous():
                raise ValueError(f"forward_samples(nhwc=True): expected a contiguous (N, H, W, {_rp(self.in_channels)}) tensor")
            n, h, w, _ = x.shape
        else:
            n, _, h, w = x.shape
        # groups > 1: x holds `groups` independent BatchNorm batches of n / groups consecutive images (the TTA views of
        # one image batch, test_2D.py:299-311: every view is its own forward with its own batch statistics); group g is
        # un-flipped by group_flips[g] (bit 0 horizontal, bit 1 vertical) and lands in slot offset slot_offset + g
        if groups < 1 or n % groups:
            raise ValueError("forward_samples: the batch must hold `groups` equal groups of images")
        if groups > 1 and n_samples != 1:
            raise ValueError("forward_samples: batched view groups go with n_samples = 1")
        # eval mode: the statistics are the checkpoint's, the same for every view -- one table row, no groups
        self._groups = 1 if self._ev else groups
        try:
            feats = self._backbone(x, nhwc=nhwc)
        except Exception:
            self._groups = 1
            raise
        user_out = out is not None
        if out is None:
            out = torch.empty((n_samples * n, self.num_classes, h, w), dtype=torch.float32, device=dev)
        code = (1 if hflip_back else 0) | (2 if vflip_back else 0)
        flip = torch.full((n,), code, dtype=torch.int32, device=dev) if code else None
        per = n // groups
        if groups > 1 and group_flips is not None:
            flip = self._itensor([int(group_flips[i // per]) for i in range(n)], dev)
        for t in range(n_samples):
            mode = _lib.VX_DROP_NONE
            masks = None
            seed = 0
            if self.dropout_final and dropout_masks is not None:
                mode = _lib.VX_DROP_MASK
                masks = [_pad_mask(m, dev) for m in dropout_masks[t]]
                self._hold += masks
            elif self.dropout_final:  # F.dropout(..., training=True): live even in eval mode (hrnet_module.py:642-646)
                mode = _lib.VX_DROP_HASH
                if seeds is not None:
                    seed = int(seeds[t])
                else:
                    seed = self.seed * 1000003 + self._calls
                    self._calls += 1
            if user_out and groups > 1:   # image b of view g -> slot b * slot_stride + slot_offset + g
                dst = self._itensor([(i % per) * slot_stride + slot_offset + i // per for i in range(n)], dev)
            elif user_out:  # image b, sample t -> slot b * slot_stride + slot_offset + t  (per-image (Npred, C, H, W) stacks)
                dst = self._itensor([i * slot_stride + slot_offset + t for i in range(n)], dev)
            else:      # (cached per content like every slot table: no per-forward ATen kernel, nothing a capture cannot hold)
                dst = self._itensor(range(t * n, (t + 1) * n), dev)
            self._hold.append(dst)
            self._head(feats, out, (h, w), dst, flip, mode, seed, masks, softmax=softmax_out)
        self._hold_last = self._hold  # keep everything alive until the stream has consumed it
        self._groups = 1
        if user_out:
            return out
        return out.view(n_samples, n, self.num_classes, h, w)

    def profile_forward(self, x: torch.Tensor, peak_tflops: float, hbm_gbs: float, reps: int = 3, groups: int = 1, nhwc: bool = False):
        """bench.py's roofline leg for the 2D path: one forward per rep on ONE stream with a HIP event pair around every
        convolution launch; the dominant convolution kernel instance with its algorithmic TFLOP/s and GB/s and the roof
        that binds it (the larger of flops / matrix roof and bytes / HBM roof)."""
        import os
        old = os.environ.get("VX_HRNET_SINGLE_STREAM")
        os.environ["VX_HRNET_SINGLE_STREAM"] = "1"
        acc, shapes = {}, {}
        try:
            for rep in range(reps + 1):
                self._prof = []
                self.forward_samples(x, 1, groups=groups, nhwc=nhwc)
                torch.cuda.synchronize()
                rows, self._prof = self._prof, None
                if rep == 0:
                    continue
                for name, fl, by, e0, e1 in rows:
                    ms = e0.elapsed_time(e1)
                    a = acc.setdefault(name, {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0})
                    a["ms"] += ms; a["flops"] += fl; a["bytes"] += by; a["launches"] += 1
                    # ... and per LAYER SHAPE of the instance (its algorithmic flops / bytes identify the shape): one template
                    # instance serves layers whose launches differ 100 x in duration, an instance average says little
                    b = shapes.setdefault((name, fl, by), {"ms": 0.0, "launches": 0})
                    b["ms"] += ms; b["launches"] += 1
        finally:
            self._prof = None
            if old is None:
                os.environ.pop("VX_HRNET_SINGLE_STREAM", None)
            else:
                os.environ["VX_HRNET_SINGLE_STREAM"] = old
        name, a = max(acc.items(), key=lambda kv: kv[1]["ms"])
        conv_ms = sum(v["ms"] for v in acc.values()) / reps
        # the object names ONE layer shape: the one the dominant instance spends most of its time on (round-4 verdict, item 4c)
        (_, lfl, lby), sh = max(((k, v) for k, v in shapes.items() if k[0] == name), key=lambda kv: kv[1]["ms"])
        sec = sh["ms"] * 1e-3
        tf, gb = lfl * sh["launches"] / sec / 1e12, lby * sh["launches"] / sec / 1e9
        bound = "mfma" if lfl / (peak_tflops * 1e12) >= lby / (hbm_gbs * 1e9) else "hbm"
        return {"bound": bound, "kernel": name, "achieved": round(tf if bound == "mfma" else gb, 3),
                "peak": peak_tflops if bound == "mfma" else hbm_gbs, "unit": "TFLOP/s" if bound == "mfma" else "GB/s",
                "frac": round(tf / peak_tflops if bound == "mfma" else gb / hbm_gbs, 4),
                "frac_mfma": round(tf / peak_tflops, 4), "frac_hbm": round(gb / hbm_gbs, 4),
                "layer": {"flops_per_launch": lfl, "bytes_per_launch": lby, "launches_per_forward": sh["launches"] // reps,
                          "avg_launch_ms": round(sh["ms"] / sh["launches"], 4),
                          "share_of_the_instance": round(sh["ms"] / a["ms"], 3),
                          "note": "achieved / frac are THIS layer shape's (algorithmic flops and bytes of one launch over its own "
                                  "average duration); the instance serves other shapes too"},
                "avg_launch_ms": round(sh["ms"] / sh["launches"], 4),
                "instance_avg_launch_ms": round(a["ms"] / a["launches"], 4), "launches_per_forward": a["launches"] // reps,
                "conv_launches_per_forward": sum(v["launches"] for v in acc.values()) // reps,
                "conv_ms_per_forward": round(conv_ms, 3), "share_of_conv_time": round(a["ms"] / reps / conv_ms, 3),
                "traffic": None}

    def forward(self, x: torch.Tensor, mean_only: bool = False):
        if self.ssn:
            return self.forward_ssn(x, mean_only=mean_only)
        return self.forward_samples(x, 1)[0]

    @torch.no_grad()
    def forward_ssn(self, x: torch.Tensor, mean_only: bool = False, dropout_masks=None, seed: Optional[int] = None):
        """hrnet_ssn (hrnet_module.py:559-595): backbone + mean / factor heads -> a LowRankNormal2D whose
        sample([n]) has the reference's shape (n, B, C*H*W)."""
        _lib.require_gpu()
        dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
        x = x.detach().to(dev, torch.float32)
        self._pk = self._ensure_packed(dev)
        self._ev = not self.training
        if self._ev:
            self._ensure_affine(dev)
        self._st = _lib.stream_ptr()
        # the previous forward's intermediates were kept until now (its kernels are enqueued ahead of everything this call
        # launches, on streams this call joins before reusing memory): release them BEFORE allocating this forward's, or two
        # forwards' worth of activations are alive at once (W48 at 32 views: ~2 x 150 GB)
        self._hold_last = None
        self._hold = []
        n, _, h, w = x.shape
        feats = self._backbone(x)
        mode, masks, sd = _lib.VX_DROP_NONE, None, 0
        if self.dropout_final and dropout_masks is not None:
            mode = _lib.VX_DROP_MASK
            masks = [_pad_mask(m, dev) for m in dropout_masks]
            self._hold += masks
        elif self.dropout_final:
            mode = _lib.VX_DROP_HASH
            sd = int(seed) if seed is not None else self.seed * 1000003 + self._calls
            self._calls += 1
        mean_lo, fac_lo = self._head_lowres(feats, mode, sd, masks, dev)
        self._hold_last = self._hold
        return LowRankNormal2D(mean_lo, fac_lo, self.num_classes, 0 if mean_only else self.rank, self.epsilon, (h, w),
                               self.seed + self._calls)

    def graphed(self, example: torch.Tensor, n_samples: int = 1, seeds: Optional[Sequence[int]] = None):
        """Capture forward_samples for a fixed input shape into one hipGraph (the eager walk is ~1200 launches and
        host-bound below ~20 ms).  Returns f(x) -> logits view of a static output buffer; dropout seeds are baked in."""
        dev = torch.device("cuda", torch.cuda.current_device())
        static_x = example.detach().to(dev, torch.float32).clone()
        seeds = list(seeds) if seeds is not None else list(range(n_samples))
        self.forward_samples(static_x, n_samples, seeds=seeds)  # warm-up: packs weights, creates side streams
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static_y = self.forward_samples(static_x, n_samples, seeds=seeds)
        keep = self._hold_last

        def run(x):
            static_x.copy_(x)
            g.replay()
            return static_y

        run._keep = (g, keep, static_x, static_y)
        return run


def get_seg_model(cfg, **kwargs):
    """hrnet_module.py:740-745 (PRETRAINED weights are loaded by the caller through load_state_dict)."""
    return HighResolutionNet(cfg)
