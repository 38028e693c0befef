"""GPU: conv3d_deep.hip shares the (tile, output group) pairs of its last, partly filled round among idle workgroups (deep_tail in
values_amd/csrc/conv3d_route.h): 2 / 4 workgroups stage the same pair and each multiplies and stores the column tiles of 4 / 2 of
the eight multiplying waves.  Single-layer launches at batch sizes that put known pairs into the shared round:

  * a sample's output BITS are the same in a whole pair of a main round and in a shared pair, and so are its InstanceNorm statistics
    (every tile writes one partials entry per wave group, shared or not);
  * everything against the float64 conv, at the bound of the deep kernel's own tests (tests/test_gpu_kernels.py: 4e-5 on the same
    formula inputs), hash dropout with the exported masks;
  * nothing is stored past the batch.

The persistent grid is one workgroup per compute unit (vx_cu_count: the device's multiprocessor count, the number torch reports);
a case whose batch does not give the stated rounds on the device at hand skips."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests.formula import formula_tensor
from tests.test_gpu_kernels import _finalize, _hash_mask, _pack_deep, cl, dev, ncdhw
from values_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 4e-5          # the deep kernel's bound against the float64 conv (tests/test_gpu_kernels.py, DEEP_CASES: same inputs' scale)
FILL = -77.0
SEED, LAYER = 77, 13


def grid():
    return torch.cuda.get_device_properties(0).multi_processor_count


def tail_of(P, G, cap=4):
    """(F, r, S): the rule deep_tail states (tests/test_deep_tail_route_cpu.py checks the header against it)"""
    Fr, r = divmod(P, G)
    S = next((s for s in (4, 2) if r and s <= cap and r * s <= G), 1)
    return Fr, r, S


def need(P, G, cap, want):
    got = tail_of(P, G, cap)
    if got != want:
        pytest.skip(f"{P} pairs on {G} workgroups give (F, r, S) = {got}, the case needs {want}")


def pairs(n, shape, cout):
    d, h, w = shape
    return (-(-n // 4) if d * h * w == 64 else n) * (cout // 32)      # (4^3: four samples per tile; 8^3: one)


def launch(xd, cin, cout, wp, bd, n, shape, epi, guard=0):
    """one vx_conv3d_k3 launch on a dense channels-last device input of n samples; the output buffer holds `guard` more samples.
    -> (out (n + guard, D, H, W, Cout), statistics partials or None, kernel name)"""
    lib = _lib.load()
    d, h, w = shape
    a = _lib.ConvArgs()
    a.w_family = lib.vx_conv3d_k3_family(cin, cout)
    out = torch.full((n + guard, d, h, w, cout), FILL, dtype=torch.float32, device=dev())
    a.in_ = xd.data_ptr(); a.w_packed = wp.data_ptr(); a.bias = bd.data_ptr(); a.out = out.data_ptr()
    a.in_pitch, a.out_pitch, a.out_coff = cin, cout, 0
    a.N, a.D, a.H, a.W, a.Cin, a.Cout = n, d, h, w, cin, cout
    st = None
    if epi == "stats":
        st = torch.full((n, lib.vx_conv3d_k3_tiles_for(d, h, w, cout), cout, 2), 5.0, dtype=torch.float32, device=dev())
        a.stats_partial = st.data_ptr()
    else:
        a.act = _lib.VX_ACT_LRELU
        if epi == "lrelu_hash":
            a.drop_mode, a.drop_seed, a.drop_layer = _lib.VX_DROP_HASH, SEED, LAYER
    _lib.check(lib.vx_conv3d_k3(C.byref(a), _lib.stream_ptr()), "vx_conv3d_k3")
    torch.cuda.synchronize()
    kn = lib.vx_last_kernel_name().decode()
    assert kn.startswith("conv3d_deep_kernel<"), kn
    return out, st, kn


def want_of(ref, epi, n, cout, shape):
    """the float64 result of an epilogue from the float64 conv `ref` (N, C, D, H, W)"""
    if epi == "stats":
        return ref
    act = F.leaky_relu(ref, 0.01)
    return act * _hash_mask(SEED, LAYER, n, cout, *shape) * 2.0 if epi == "lrelu_hash" else act


def check_stats_are_the_sums(st, got):
    ssum = st.double().sum(1).cpu()
    torch.testing.assert_close(ssum[..., 0], got.double().sum((2, 3, 4)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(ssum[..., 1], (got.double() ** 2).sum((2, 3, 4)), rtol=1e-5, atol=1e-3)


class Layer:
    """inputs, packed weights and the float64 conv of one (Cin, Cout, shape, N) case -- computed once, never changed"""

    def __init__(self, cin, cout, shape, n, seed, dup=None):
        self.cin, self.cout, self.shape, self.n = cin, cout, shape, n
        x = torch.from_numpy(formula_tensor((n, cin) + shape, seed, scale=1.5)).float()
        if dup:                                       # sample 0 (a pair of the first main round) again in the last tile's samples
            x[n - dup:] = x[0]
        self.wt, self.b, self.wp, self.bd = _pack_deep(cin, cout, seed + 1)
        self.x = x
        self.xd = cl(x).to(dev())
        self.ref = F.conv3d(x.double(), self.wt.double(), self.b.double(), padding=1)

    def run(self, epi, guard=0):
        return launch(self.xd, self.cin, self.cout, self.wp, self.bd, self.n, self.shape, epi, guard)

    def finalize(self, st):
        d, h, w = self.shape
        return _finalize(st, st.shape[0], st.shape[1], self.cout, d * h * w)


@pytest.fixture(scope="module")
def case1():
    """4^3, 16 -> 128, N = 4 (G / 4 + G / 16): F = 1, r = G / 4, S = 4"""
    G = grid()
    if G % 16:
        pytest.skip(f"{G} workgroups: no batch with r = G / 4")
    return Layer(16, 128, (4, 4, 4), 4 * (G // 4 + G // 16), 831, dup=4)


@pytest.fixture(scope="module")
def case2():
    """8^3, 16 -> 64, N = G / 2 + G / 4: P = 2 N, F = 1, r = G / 2, S = 2"""
    G = grid()
    if G % 4:
        pytest.skip(f"{G} workgroups: no batch with r = G / 2")
    return Layer(16, 64, (8, 8, 8), G // 2 + G // 4, 841, dup=1)


@pytest.mark.parametrize("epi", ["lrelu", "lrelu_hash"])
def test_four_way_shared_pairs_at_4cubed(case1, epi):
    L, G = case1, grid()
    need(pairs(L.n, L.shape, L.cout), G, 4, (1, G // 4, 4))
    out, _, _ = L.run(epi)
    got = ncdhw(out).cpu()
    if epi == "lrelu":                                # sample 0 of tile 0 (main round) and its four copies in the last tile (shared)
        for i in range(L.n - 4, L.n):
            assert torch.equal(out[i], out[0]), i
    err = (got.double() - want_of(L.ref, epi, L.n, L.cout, L.shape)).abs().max().item()
    print(f"case 1 {epi}: max|d| = {err:.3e}")
    assert err < TOL, err


@pytest.mark.parametrize("epi", ["stats", "lrelu"])
def test_two_way_shared_pairs_at_8cubed(case2, epi):
    L, G = case2, grid()
    need(pairs(L.n, L.shape, L.cout), G, 2 if epi == "stats" else 4, (1, G // 2, 2))
    out, st, _ = L.run(epi)
    got = ncdhw(out).cpu()
    assert torch.equal(out[L.n - 1], out[0])          # the main-round copy and the shared copy of one sample: the same bits
    err = (got.double() - want_of(L.ref, epi, L.n, L.cout, L.shape)).abs().max().item()
    print(f"case 2 {epi}: max|d| = {err:.3e}")
    assert err < TOL, err
    if epi == "stats":
        check_stats_are_the_sums(st, got)
        assert torch.equal(st[L.n - 1], st[0])
        mean, rstd = L.finalize(st)
        assert torch.equal(mean[L.n - 1], mean[0]) and torch.equal(rstd[L.n - 1], rstd[0])


@pytest.mark.parametrize("cin,cout,shape,n,guard", [(16, 64, (8, 8, 8), 2, 2), (16, 128, (4, 4, 4), 5, 4)])
def test_every_pair_shared_and_nothing_stored_past_the_batch(cin, cout, shape, n, guard):
    """F = 0: no main round at all; at 4^3 the last four-sample tile holds one sample, and its three masked samples would land
    in the guard rows behind the output"""
    G = grid()
    P = pairs(n, shape, cout)
    if tail_of(P, G)[0] != 0 or tail_of(P, G)[2] == 1:
        pytest.skip(f"{P} pairs on {G} workgroups are not all shared")
    L = Layer(cin, cout, shape, n, 851)
    for epi in ("lrelu", "lrelu_hash") + (("stats",) if shape == (8, 8, 8) else ()):
        out, st, _ = L.run(epi, guard)
        assert (out[n:] == FILL).all(), epi
        got = ncdhw(out[:n]).cpu()
        err = (got.double() - want_of(L.ref, epi, n, cout, shape)).abs().max().item()
        print(f"case 3 {shape} {epi}: max|d| = {err:.3e}")
        assert err < TOL, (epi, err)
        if st is not None:
            check_stats_are_the_sums(st, got)


def test_batch_independence_through_a_shared_pair(case2):
    """the property test_conv3d_deep_is_batch_independent guards, through the split: one sample alone (F = 0, its two pairs shared
    four ways / two ways with statistics), first of case 2's batch (whole pairs) and last of it (pairs shared two ways)"""
    L, G = case2, grid()
    need(pairs(L.n, L.shape, L.cout), G, 4, (1, G // 2, 2))
    x1 = L.xd[L.n - 1:].contiguous()
    for epi in ("lrelu", "stats"):
        big, stb, knb = L.run(epi)
        one, st1, kn1 = launch(x1, L.cin, L.cout, L.wp, L.bd, 1, L.shape, epi)
        assert kn1 == knb
        assert torch.equal(one[0], big[L.n - 1]) and torch.equal(one[0], big[0]), epi
        if epi == "stats":
            assert torch.equal(st1[0], stb[L.n - 1]) and torch.equal(st1[0], stb[0])
            mb, rb = L.finalize(stb)
            m1, r1 = L.finalize(st1)
            for i in (0, L.n - 1):
                assert torch.equal(m1[0], mb[i]) and torch.equal(r1[0], rb[i]), i


# ---- launches that share nothing: r > G / 2 and r = 0 -------------------------------------------------------------------------
def _unshared_cases(G):
    return [("rest_above_half", G // 2 + G // 4 + 1), ("no_rest", G // 2)]      # 8^3, 16 -> 64: P = 2 N


def _unshared_outputs():
    """{case: {epilogue: output}} of the launches of _unshared_cases, with the library of this process"""
    res = {}
    for name, n in _unshared_cases(grid()):
        L = Layer(16, 64, (8, 8, 8), n, 861)
        res[name] = {epi: L.run(epi)[0].cpu() for epi in ("stats", "lrelu", "lrelu_hash")}
        res[name]["layer"] = L
    return res


def test_launches_without_a_shared_round_behave_as_before(tmp_path):
    """r > G / 2 (S = 1) and r = 0: against the float64 conv; and where VX_LIB_PATH names another build of the library (the A/B
    build of the parent revision), the outputs of this process' library and of the tree's own in a child process are the same bits"""
    G = grid()
    for name, n in _unshared_cases(G):
        Fr, r, S = tail_of(2 * n, G)
        if S != 1 or (name == "no_rest") != (r == 0):
            pytest.skip(f"{2 * n} pairs on {G} workgroups: (F, r, S) = {(Fr, r, S)}")
    mine = _unshared_outputs()
    for name, outs in mine.items():
        L = outs.pop("layer")
        for epi, out in outs.items():
            err = (ncdhw(out).double() - want_of(L.ref, epi, L.n, L.cout, L.shape)).abs().max().item()
            print(f"case 5 {name} {epi}: max|d| = {err:.3e}")
            assert err < TOL, (name, epi, err)
    other = os.environ.get("VX_LIB_PATH")
    if not other:
        return
    # this process runs the library VX_LIB_PATH names; a fresh child without it runs the tree's own
    dump = str(tmp_path / "unshared.pt")
    env = {k: v for k, v in os.environ.items() if k != "VX_LIB_PATH"}
    code = ("import torch; from tests import test_gpu_deep_tail as t; r = t._unshared_outputs(); "
            "[o.pop('layer') for o in r.values()]; torch.save(r, %r)" % dump)
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, timeout=300)
    theirs = torch.load(dump)
    for name, outs in mine.items():
        for epi, out in outs.items():
            assert torch.equal(out, theirs[name][epi]), (name, epi)
