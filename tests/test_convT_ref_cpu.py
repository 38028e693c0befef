"""CPU: tests/convT_ref.py, the float64 reference and the tolerance tests/test_gpu_convT_matrix.py holds vx_convT_k2s2 to, checked
without a GPU -- the up-convolution against F.conv_transpose3d, the layouts, the hash mask's element index, an emulation of either
arithmetic inside the bound on every case of the matrix, and six single faults outside it.  No element is left out of any
comparison."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import convT_ref as ref
from tests import convT_route_cases as rc
from tests.ops2d_ref import hash_keep_mask

BY_ID = {c["id"]: c for c in rc.LAYER_CASES}


@pytest.fixture(scope="module")
def lib():
    from values_amd import _lib
    return _lib.load()


def family(lib, vxcfg, case, mode):
    vxcfg.set(conv_fp32=mode)
    code, name, _, _ = rc.dry_run(lib, rc.layer_args(case, rc.dummy_ptr))
    assert code == 0, case["id"]
    return ref.family_of(name)


def test_only_64_and_128_channel_routes_depend_on_the_conv_mode(lib, vxcfg):
    """the premise of convT_route_cases.matrix_params: every other case is one launch under both modes"""
    for case in rc.LAYER_CASES:
        names = []
        for mode in (0, 1):
            vxcfg.set(conv_fp32=mode)
            names.append(rc.dry_run(lib, rc.layer_args(case, rc.dummy_ptr))[1])
        assert (names[0] != names[1]) == (case["cin"] in (64, 128)), (case["id"], names)
    assert len({(c["id"], m) for c, m in rc.matrix_params()}) == len(rc.matrix_params()) >= len(rc.LAYER_CASES)


@pytest.mark.parametrize("cin,cout", [(16, 8), (64, 32)])
@pytest.mark.parametrize("vol", [(2, 3, 5, 6), (1, 3, 5, 7)])
def test_expected_without_epilogue_is_conv_transpose3d(cin, cout, vol):
    case = rc._case("t", cin, cout, vol)
    x, w, b, _ = (t.double() if t is not None else None for t in rc.host_inputs(case))
    E, keep, S = ref.expected(case, x, w, b)
    want = F.conv_transpose3d(x.permute(0, 4, 1, 2, 3), w, b, stride=2)
    assert E.shape == want.shape and bool(keep.all())
    assert float(((E - want).abs() / want.abs().clamp_min(1e-3)).max()) < 1e-12
    assert float((S - F.conv_transpose3d(x.abs().permute(0, 4, 1, 2, 3), w.abs(), None, stride=2)).abs().max()) < 1e-12


@pytest.mark.parametrize("vol,cout", [((2, 3, 5, 6), 8), ((1, 3, 5, 7), 16)])
def test_layouts_round_trip_and_their_write_sets_are_disjoint(vol, cout):
    n, d, h, w = vol
    vals = torch.arange(n * cout * 8 * d * h * w, dtype=torch.float64).reshape(n, cout, 2 * d, 2 * h, 2 * w)
    for xb in (x for x in (1, 2, 4) if (2 * w) % x == 0):
        sets = []
        for half in (0, 1):
            case = rc._case("t", 16, cout, vol, xblk=xb, half=half)
            off = ref.offsets(case).reshape(-1)
            assert len(torch.unique(off)) == off.numel() and int(off.min()) >= 0 and int(off.max()) < ref.buffer_floats(case)
            buf = ref.scatter(case, vals)
            assert torch.equal(ref.gather(case, buf), vals)
            # the definition, through a view of the buffer: [N][2D][2H][2W / xb][2][xb][Cout]
            v = buf.view(n, 2 * d, 2 * h, (2 * w) // xb, 2, xb, cout)
            assert torch.equal(v[:, :, :, :, half].reshape(n, 2 * d, 2 * h, 2 * w, cout).permute(0, 4, 1, 2, 3), vals)
            assert bool((v[:, :, :, :, 1 - half] == ref.SENTINEL).all())
            sets.append(off)
        both = torch.cat(sets)
        assert len(torch.unique(both)) == both.numel() == ref.buffer_floats(case)        # disjoint, and together the whole buffer
    for coff, extra in ((0, 0), (0, 4), (4, 4), (4, 8)):
        case = rc._case("t", 16, cout, vol, out_coff=coff, out_extra=extra)
        off = ref.offsets(case).reshape(-1)
        assert len(torch.unique(off)) == off.numel()
        buf = ref.scatter(case, vals)
        assert torch.equal(ref.gather(case, buf), vals)
        v = buf.view(n, 2 * d, 2 * h, 2 * w, cout + extra)
        assert torch.equal(v[..., coff:coff + cout].permute(0, 4, 1, 2, 3), vals)
        rest = torch.ones(cout + extra, dtype=torch.bool)
        rest[coff:coff + cout] = False
        assert bool((v[..., rest] == ref.SENTINEL).all())                                  # the rest of the pitch is not in the set
        written = torch.zeros(ref.buffer_floats(case), dtype=torch.bool)
        written[off] = True
        wv = written.view(n, 2 * d, 2 * h, 2 * w, cout + extra)
        assert bool(wv[..., coff:coff + cout].all()) and not bool(wv[..., rest].any())


def test_hash_mask_element_index():
    """the reshaped stream equals, element for element, bit e of the sample's stream at e = ((oz OH + oy) OW + ox) Cout + co"""
    case = rc._case("t", 16, 8, (3, 2, 3, 5), act=rc.ACT_RELU, drop=rc.DROP_HASH)
    n, d, h, w = case["vol"]
    co = case["cout"]
    for seed_dev, drop_seed in ((0, ref.DROP_SEED), (5, ref.DROP_SEED), (0x30, 0xFFFFFFF0)):
        keep = ref.keep_mask(case, n, seed_dev=seed_dev, drop_seed=drop_seed)
        flat = hash_keep_mask((drop_seed + seed_dev) % (1 << 32), ref.DROP_LAYER, n, 8 * d * h * w * co)
        count = 0
        for s in range(n):
            for oz in range(2 * d):
                for oy in range(2 * h):
                    for ox in range(2 * w):
                        for c in range(co):
                            e = ((oz * 2 * h + oy) * 2 * w + ox) * co + c
                            assert bool(keep[s, c, oz, oy, ox]) == bool(flat[s, e])
                            count += 1
        assert count == keep.numel()
    # a later chunk of the launch's samples is keyed by the samples' own indices
    assert torch.equal(ref.keep_mask(case, 2, sample0=1), ref.keep_mask(case, 3)[1:])
    assert not torch.equal(ref.keep_mask(case, 1, sample0=1), ref.keep_mask(case, 1))


# ---- the emulations against the bound -------------------------------------------------------------------------------------------------
def emulated(case, fam, n0=0, n1=None):
    """(got, E, tol, keep) of samples n0 .. n1 of a case: the emulation of the family's arithmetic, the reference and its tolerance"""
    x, w, b, mask = rc.host_inputs(case)
    assert float(x.abs().max()) <= 2 and float(w.abs().max()) <= 2        # the premise of the split bound
    n1 = case["vol"][0] if n1 is None else n1
    E, keep, S = ref.expected(case, x[n0:n1], w, b, mask, sample0=n0)
    tol = ref.tolerance(case, S, b, fam, keep)
    got = (ref.emulate_split if fam == "s16" else ref.emulate_fp32)(case, x[n0:n1], w, b, keep)
    return got, E, tol, keep


def test_emulations_of_every_matrix_case_stay_inside_the_bound(lib, vxcfg):
    """A sequential float32 fmaf chain (fp32 families) and the split-fp16 scheme as the kernel forms it (hi / lo operands, exact
    products, three float32 sums per 32 channels) lie within tolerance() on the inputs of every case of the matrix, every element
    compared.  Worst |emulation - E| / tol over the matrix: fp32 0.262, split 0.018 (its bound is mostly the dropped lo x lo term, a worst case
    random signs never reach)."""
    worst, done = {}, set()
    for case, mode in rc.matrix_params():
        fam = family(lib, vxcfg, case, mode)
        arith = "s16" if fam == "s16" else "fp32"
        key = (arith, case["cin"], case["cout"], case["vol"], case["act"], case["drop"])      # the layout does not enter the values
        if key in done:
            continue
        done.add(key)
        n = case["vol"][0]
        step = 1 if n * 8 * case["vol"][1] * case["vol"][2] * case["vol"][3] * case["cout"] > (1 << 22) else n
        for n0 in range(0, n, step):
            got, E, tol, _ = emulated(case, fam, n0, n0 + step)
            ratio, first = ref.compare(got, E, tol)
            assert first is None, ref.describe(case, first, got, E, tol, n0)
            worst[arith] = max(worst.get(arith, 0.0), ratio)
    print("worst emulation / tolerance:", worst)
    assert set(worst) == {"fp32", "s16"} and all(0.0 < r <= 1.0 for r in worst.values())


# ---- single faults --------------------------------------------------------------------------------------------------------------------
FAULT_BASES = {"fp32": "epi:16->8:2x3x5x6", "s16": "epi:64->32:2x3x5x6"}


@functools.lru_cache(maxsize=None)
def _emulated_by_id(cid, fam):
    return emulated(BY_ID[cid], fam)


def _block(v, vol):
    """the slices of input voxel v's 2x2x2 output block in an NCDHW tensor"""
    _, d, h, w = vol
    x, y, z, n = v % w, v // w % h, v // (w * h) % d, v // (w * h * d)
    return n, slice(None), slice(2 * z, 2 * z + 2), slice(2 * y, 2 * y + 2), slice(2 * x, 2 * x + 2)


def _fault(name, arith):
    """(case, faulty output, E, tol): one single fault injected into the emulation's output"""
    base = FAULT_BASES[arith]
    fam = "s16" if arith == "s16" else "mfma"
    tag = {"key": ":hash", "half": ":xblk2h1"}.get(name, ":none")
    case = BY_ID[base + tag]
    got, E, tol, keep = _emulated_by_id(case["id"], fam)
    assert ref.compare(got, E, tol)[1] is None
    bad = got.clone()
    nvox = int(np.prod(case["vol"]))
    if name == "dx":                     # the two dx columns of every voxel swapped
        bad = got.view(*got.shape[:4], -1, 2).flip(-1).reshape(got.shape)
    elif name == "quad":                 # one 16-byte piece holds the channels four further on
        bad[1, 0:4, 3, 4, 5] = got[1, 4:8, 3, 4, 5]
    elif name == "block":                # one voxel's block written to its neighbour's place
        bad[_block(101, case["vol"])] = got[_block(100, case["vol"])]
    elif name == "key":                  # the dropout key of sample n + 1
        x, w, b, mask = rc.host_inputs(case)
        wrong = ref.keep_mask(case, case["vol"][0], sample0=1)
        emu = ref.emulate_split if arith == "s16" else ref.emulate_fp32
        bad = emu(case, x, w, b, wrong)
    elif name == "half":                 # written into the other half of the concat buffer
        other = dict(case, half=1 - case["half"])
        bad = ref.gather(case, ref.scatter(other, got))
    elif name == "tile":                 # the last column tile of 16 input voxels never stored
        for v in range((nvox - 1) // 16 * 16, nvox):
            bad[_block(v, case["vol"])] = ref.SENTINEL
    return case, bad, E, tol


@pytest.mark.parametrize("arith", ["fp32", "s16"])
@pytest.mark.parametrize("name", ["dx", "quad", "block", "key", "half", "tile"])
def test_bound_catches_a_single_fault(name, arith):
    case, bad, E, tol = _fault(name, arith)
    ratio, first = ref.compare(bad, E, tol)
    assert first is not None and ratio > 1.0, (name, arith, ratio)
    assert ref.describe(case, first, bad, E, tol).startswith(case["id"] + ": first bad (n, co, oz, oy, ox) = ")
