"""GPU: upscale3 composed into expand_2_1's up half (vx_conv3d_args.up_fused on the 16-channel z-column kernel: the composed bodies
of conv3d_zc16_kernel<16,EPI,0,1,1>, weights from vx_pack_conv3d_upfused_zc16) -- kernel level through vx_conv3d_k3 against the
float64 oracle conv_transpose3d + conv3d + partial sums + LeakyReLU + mask, at the smallest shapes where the geometry can go
wrong, and network level against the evaluated path and the float64 oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_lattice as L
from tests import test_gpu_kernels as K
from tests.formula import formula_tensor
from tests.upcompose16_ref import formula_weights
from values_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 8e-5          # the evaluated path's bound for the same launch (test_conv3d_zc16_fused_upconvolution_matches_oracle)


def _presplit(cd):
    """a channels-last float tensor as the fp16 pairs [hi0..3 | lo0..3] per 16-byte piece (vx_conv3d_args.out_split / up_split)"""
    v = cd.reshape(-1, 4)
    hi = v.half()
    lo = ((v - hi.float()) * 2048.0).half()
    return torch.cat([hi, lo], 1).view(torch.float32).reshape(cd.shape).contiguous()


def _unplanar(y, n, d, h, w):
    """[n][d][h][octet][hi | lo][w][8 halves] -> channels-last float"""
    pl = y.contiguous().view(torch.float16).view(n, d, h, 2, 2, w, 8).float()
    return (pl[:, :, :, :, 0] + pl[:, :, :, :, 1] / 2048.0).permute(0, 1, 2, 4, 3, 5).reshape(n, d, h, w, 16)


class Case:
    """device tensors of one up-half launch: coarse tensor (pitch, split), partial sums, both packs of the up-convolution"""

    def __init__(self, shape, pitch, split, seed=920, weights=None, coarse=None, part=None):
        lib = _lib.load()
        n, d, h, w = shape
        assert lib.vx_conv3d_k3_upfuse_ok(d, h, w, 16, 16) == 2
        self.shape, self.pitch, self.split = shape, pitch, split
        self.w1, self.uw, self.ub = weights if weights is not None else formula_weights()
        self.coarse = coarse if coarse is not None else torch.from_numpy(formula_tensor((n, 32, d // 2, h // 2, w // 2), seed, scale=1.3)).float()
        self.part = part if part is not None else torch.from_numpy(formula_tensor((n, 16, d, h, w), seed + 1, scale=0.7)).float()
        dv = K.dev()
        cd = torch.full((n, d // 2, h // 2, w // 2, pitch), 1e30, dtype=torch.float32, device=dv)      # (the pad channels are never read)
        cd[..., :32] = K.cl(self.coarse).to(dv)
        if split:
            cd[..., :32] = _presplit(cd[..., :32].contiguous())
        self.cd = cd.contiguous()
        st = _lib.stream_ptr()
        self.w1d, self.uwd, self.ubd = self.w1.to(dv), self.uw.to(dv), self.ub.to(dv)
        up_half = self.w1d[:, :16].contiguous()
        self.wp = torch.empty(lib.vx_conv3d_k3_packed_floats(16, 16), dtype=torch.float32, device=dv)
        _lib.check(lib.vx_pack_conv3d_k3(_lib.ptr(up_half), _lib.ptr(self.wp), 16, 16, st), "vx_pack_conv3d_k3")
        self.uwp = torch.empty(lib.vx_convT_zc16_packed_floats(), dtype=torch.float32, device=dv)
        _lib.check(lib.vx_pack_convT_zc16(_lib.ptr(self.uwd), _lib.ptr(self.uwp), st), "vx_pack_convT_zc16")
        self.fused = torch.empty(lib.vx_conv3d_upfused_zc16_packed_floats(), dtype=torch.float32, device=dv)
        _lib.check(lib.vx_pack_conv3d_upfused_zc16(_lib.ptr(self.w1d), _lib.ptr(self.uwd), _lib.ptr(self.ubd), _lib.ptr(self.fused), st),
                   "vx_pack_conv3d_upfused_zc16")
        self.bias = torch.zeros(16, dtype=torch.float32, device=dv)             # (not added: it rides in the partial sums)
        up = F.conv_transpose3d(self.coarse.double(), self.uw.double(), self.ub.double(), stride=2)
        self.pre = F.conv3d(up, self.w1.double()[:, :16].contiguous(), None, padding=1) + self.part.double()

    def args(self, out, *, composed, hashed, planar, act=None):
        lib = _lib.load()
        n, d, h, w = self.shape
        a = _lib.ConvArgs()
        a.w_family = lib.vx_conv3d_k3_family(16, 16)
        a.in_ = self.cd.data_ptr(); a.w_packed = self.wp.data_ptr(); a.bias = self.bias.data_ptr(); a.out = out.data_ptr()
        a.in_pitch, a.out_pitch, a.out_coff = 16, 16, 0
        a.N, a.D, a.H, a.W, a.Cin, a.Cout = n, d, h, w, 16, 16
        a.act = _lib.VX_ACT_LRELU if act is None else act
        if hashed:
            a.drop_mode, a.drop_seed, a.drop_layer = _lib.VX_DROP_HASH, 9, 14
        a.up_in, a.up_w, a.up_b, a.up_pitch, a.up_split = self.cd.data_ptr(), self.uwp.data_ptr(), self.ubd.data_ptr(), self.pitch, self.split
        a.up_fused = self.fused.data_ptr() if composed else None
        a.out_planar = 1 if planar else 0
        return a

    def run(self, *, composed, hashed, planar, act=None, lib=None):
        """-> channels-last float output on the device (the planar tensor un-planarised)"""
        n, d, h, w = self.shape
        accd = K.cl(self.part).to(K.dev()).contiguous()
        out = torch.full((n, d, h, w, 16), -77.0, dtype=torch.float32, device=K.dev()) if planar else accd
        a = self.args(out, composed=composed, hashed=hashed, planar=planar, act=act)
        a.acc_in, a.acc_pitch = accd.data_ptr(), 16
        own = _lib.load()
        _lib.check((lib or own).vx_conv3d_k3(C.byref(a), _lib.stream_ptr()), "vx_conv3d_k3 (up half)")
        torch.cuda.synchronize()
        if lib is None:
            epi = (5 if hashed else 6) if planar else (1 if hashed else 3)
            assert own.vx_last_kernel_name().decode() == "conv3d_zc16_kernel<16,%d,0,1,1>" % epi
        return _unplanar(out, n, d, h, w) if planar else out

    def ref(self, hashed):
        n, d, h, w = self.shape
        r = F.leaky_relu(self.pre, 0.01)
        return r * K._hash_mask(9, 14, n, 16, d, h, w) * 2.0 if hashed else r


def _check(c, got, hashed):
    dlt = (K.ncdhw(got).cpu().double() - c.ref(hashed)).abs()
    err = dlt.max().item()
    print("max |composed - oracle| = %.3g at |out| up to %.3g" % (err, c.ref(hashed).abs().max().item()))
    bad = [(dlt.amax(ax) > TOL).nonzero().flatten().tolist() for ax in ((0, 1, 3, 4), (0, 1, 2, 4), (0, 1, 2, 3))]
    assert err < TOL, (err, np.unravel_index(int(dlt.argmax()), dlt.shape), "z", bad[0], "y", bad[1], "x", bad[2])


# (4, 8, 32): one column, two items -- every voxel a border voxel in z, first / interior / last in y and x;
# (6, 16, 64): 2 x 2 columns, three items -- column-interior halos, an interior item; N = 3: an odd number of samples
@pytest.mark.parametrize("shape,pitch,split,hashed", [
    ((1, 4, 8, 32), 32, 1, 1), ((1, 4, 8, 32), 64, 0, 0), ((3, 6, 16, 64), 64, 1, 1), ((3, 6, 16, 64), 32, 0, 0),
    ((2, 4, 8, 32), 64, 1, 0), ((2, 6, 16, 64), 32, 0, 1)])
def test_composed_up_half_matches_oracle_float_and_planar(shape, pitch, split, hashed, vxcfg):
    c = Case(shape, pitch, split)
    got = c.run(composed=True, hashed=hashed, planar=False)
    _check(c, got, hashed)
    pl = c.run(composed=True, hashed=hashed, planar=True)
    # the planar tensor is the fp16 split of the float one: equal after the float values went through the same split
    want = _presplit(got.contiguous()).view(torch.float16).view(-1, 2, 4).float()
    want = (want[:, 0] + want[:, 1] / 2048.0).reshape(got.shape)
    assert torch.equal(pl, want), (pl - want).abs().max().item()


def test_composed_up_half_when_a_workgroup_walks_columns_of_two_samples(vxcfg):
    """more columns than compute units: a workgroup's second column belongs to another sample, and its first item reads the zero
    plane the previous column left in the rolling slots"""
    props = torch.cuda.get_device_properties(0)
    n = props.multi_processor_count // 4 + 1                      # (6, 16, 64): four columns per sample
    c = Case((n, 6, 16, 64), 32, 1)
    _check(c, c.run(composed=True, hashed=1, planar=False), 1)


def test_refusals_and_the_route(vxcfg):
    """composed weights only with partial sums and a dense float / planar output; the instance's name does not change"""
    lib = _lib.load()
    c = Case((1, 4, 8, 32), 32, 1)
    out = torch.zeros((1, 4, 8, 32, 16), dtype=torch.float32, device=K.dev())
    a = c.args(out, composed=True, hashed=1, planar=False)                        # no acc_in
    with pytest.raises(_lib.VxError):
        _lib.check(lib.vx_conv3d_k3(C.byref(a), _lib.stream_ptr()), "vx_conv3d_k3")
    a.acc_in, a.acc_pitch, a.out_split = out.data_ptr(), 16, 1
    with pytest.raises(_lib.VxError):
        _lib.check(lib.vx_conv3d_k3(C.byref(a), _lib.stream_ptr()), "vx_conv3d_k3")


def test_evaluated_path_keeps_the_parent_builds_bits(vxcfg):
    """up_fused = NULL runs the evaluated bodies: the same bits as the parent commit's library (values_amd/libvalues_amd_base.so, as
    tools/ab_build.sh builds it), float and planar output"""
    path = os.path.join(ROOT, "values_amd", "libvalues_amd_base.so")
    if not os.path.exists(path):
        pytest.skip("no parent build (tools/ab_build.sh)")
    base = C.CDLL(path)
    base.vx_conv3d_k3.restype = C.c_int
    base.vx_conv3d_k3.argtypes = [C.POINTER(_lib.ConvArgs), C.c_void_p]
    c = Case((3, 6, 16, 64), 32, 1)
    for planar in (False, True):
        new = c.run(composed=False, hashed=1, planar=planar)
        old = c.run(composed=False, hashed=1, planar=planar, lib=base)
        assert torch.equal(new, old), (planar, (new - old).abs().max().item())
        _check(c, new, 1)


def test_composed_up_half_is_exact_on_the_lattice(vxcfg):
    """tests/conv_lattice.py:upfused_case((1, 6, 16, 64), 32, 16, 0, 16): every composed weight of that lattice is exact in
    hi + lo 2^-11 and the border table in fp32 (asserted here on the packed block), every product and partial sum is exact in fp32
    (their bound is the lattice's own, over absolute values) -- the composed launch reproduces conv(convT(coarse)) bit for bit"""
    shape = (1, 6, 16, 64)
    u = L.upfused_case(shape, 32, 16, 0, 16)
    w1 = torch.cat([u.w.float(), torch.zeros_like(u.w.float())], 1).contiguous()          # the layer's full weight: skip half unused
    part = torch.from_numpy(L.lattice((1, 16) + shape[1:], 977, False)[0]).float()
    c = Case(shape, 32, 1, weights=(w1, u.uw.float().contiguous(), u.ub.float().contiguous()), coarse=u.coarse.float(), part=part)
    from tests.upcompose16_ref import weff_btab
    weff, btab = weff_btab(c.w1, c.uw, c.ub)
    blk = c.fused.cpu()
    halves = blk[:8 * 8 * 2 * 64 * 8 // 2].view(torch.float16).view(8, 8, 2, 4, 16, 8).double()      # [class][tap][hi | lo][g][co][j]
    packed = (halves[:, :, 0] + halves[:, :, 1] / 2048.0).permute(0, 1, 2, 4, 3).reshape(8, 8, 32, 16)   # ci = 8 g + j
    assert torch.equal(packed, weff) and torch.equal(blk[8 * 8 * 2 * 64 * 8 // 2:].double().view(3, 3, 3, 16), btab)
    pre = u.E - u.b.view(1, 16, 1, 1, 1) + part.double()
    got = c.run(composed=True, hashed=0, planar=False, act=_lib.VX_ACT_RELU)
    L.check_equal(K.ncdhw(got).cpu(), torch.relu(pre))


# ---- network level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 16, 64), (32, 48, 128)])
def test_forward_composed_against_evaluated_against_oracle(size, vxcfg):
    """the MC-dropout forward (T = 2, hash dropout) with upscale3 composed -- vx_unet3d_weights.up3_fused, the default -- and
    evaluated (the pointer cleared: vx_config keeps no switch for it) against the float64 oracle on the exported masks, logits and
    maps; the profiled forward's rows (label, kernel) are the same under both"""
    import bench
    from tests import test_gpu_unet3d as U
    from tests.formula import formula_volume
    from values_amd import predict_uncertainty
    T, seed = 2, 4242
    d, h, w = size
    model = U.make_model(do_dropout=True)
    x = torch.from_numpy(formula_volume((1, 1, d, h, w), tag=73))
    wts, _ = model._ensure_packed(K.dev())
    fused = wts.up3_fused
    assert fused
    res, rows = {}, {}
    try:
        for name, ptr in (("composed", fused), ("evaluated", None)):
            wts.up3_fused = ptr
            res[name] = predict_uncertainty([model], x.float().cuda(), n_pred=T, seeds=[seed])
            rows[name] = [(r[0], r[1]) for r in bench.profiled_forward(model, x.float().cuda(), T, seed)]
    finally:
        wts.up3_fused = fused
    assert rows["composed"] == rows["evaluated"]
    assert any(r[0] == "upscale3+expand_2_1(up half)" and r[1].startswith("conv3d_zc16_kernel<16,") for r in rows["composed"]), rows["composed"]
    masks = [m.cpu() for m in model.hash_dropout_masks(seed, T, d, h, w)]
    logits, ref = U._oracle_maps(U.formula_sd_torch(), x, [[m[t:t + 1] for m in masks] for t in range(T)])
    for name in ("composed", "evaluated"):
        err = np.abs(res[name]["logits"][0].cpu().numpy() - logits).max()
        print(name, "max |logits - oracle| = %.3g" % err)
        assert err < U.LOGIT_TOL, (name, err)
        for k in U.KEYS:
            assert np.abs(res[name][k][0].cpu().numpy() - ref[k]).max() < U.MAP_TOL, (name, k)
    print("max |composed - evaluated| logits = %.3g" % (res["composed"]["logits"] - res["evaluated"]["logits"]).abs().max().item())
