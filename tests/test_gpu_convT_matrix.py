"""GPU: the VALUES of every vx_convT_k2s2 launch of tests/convT_route_cases.py against the float64 restatement tests/convT_ref.py --
all four kernel families, every epilogue, layout and edge the route cases reach, under both conv modes where the route depends on
the mode.  Per case: the output is prefilled with -77 and bracketed by guard rows, the input's pitch padding holds NaN; after ONE
launch the kernel name is the dry run's, every element the launch may write is within the derived tolerance of the reference (dropped
elements are 0), and every other float of the buffer and the guards still holds the bits of -77.  The reference is evaluated on the
device in float64 with plain torch, a sample at a time above 20 MB.  Then the device seed word and the range word, per family."""
import pytest
import torch

from tests import convT_ref as ref
from tests import convT_route_cases as rc

pytestmark = pytest.mark.gpu
PARAMS = rc.matrix_params()
BY_ID = {c["id"]: c for c in rc.LAYER_CASES}
CHUNK_BYTES = 20 * 10 ** 6


@pytest.fixture(scope="module")
def lib():
    from values_amd import _lib
    return _lib.load()


def _bits(t):
    return t.view(torch.int32)


def _sentinel_bits(dev):
    return _bits(torch.tensor([ref.SENTINEL], dtype=torch.float32, device=dev))


def check_launch(case, buf, fam, seed_dev=0, drop_seed=ref.DROP_SEED):
    """values, zeros and untouched bytes of the launch whose result is in buf -> the worst |got - E| / tol"""
    ci, n = case["cin"], case["vol"][0]
    flat = buf.out.reshape(-1)
    dev = flat.device
    step = 1 if flat.numel() * 4 > CHUNK_BYTES else n
    written = torch.zeros(flat.numel(), dtype=torch.bool, device=dev)
    worst = 0.0
    for n0 in range(0, n, step):
        E, keep, S = ref.expected(case, buf.x[n0:n0 + step, ..., :ci], buf.w, buf.b, buf.mask, seed_dev, n0, drop_seed)
        tol = ref.tolerance(case, S, buf.b, fam, keep)
        off = ref.offsets(case, n0, n0 + step, dev)
        got = flat[off]
        ratio, first = ref.compare(got, E, tol)
        assert first is None, ref.describe(case, first, got, E, tol, n0)
        if case["drop"] != ref.DROP_NONE:
            assert bool((got[~keep] == 0).all())
        written[off.reshape(-1)] = True
        worst = max(worst, ratio)
    assert int(written.sum()) == n * case["cout"] * 8 * case["vol"][1] * case["vol"][2] * case["vol"][3]
    # bit for bit -77: both guards, and inside the buffer whatever is not in the write set (pitch padding, the out_coff gap, the
    # other half of a concat buffer)
    sent, g, whole = _sentinel_bits(dev), buf.guard, _bits(buf.whole)
    assert g >= 2 * case["vol"][3] * case["cout"]
    assert bool((whole[:g] == sent).all()), case["id"] + ": guard before the buffer written"
    assert bool((whole[g + flat.numel():] == sent).all()), case["id"] + ": guard after the buffer written"
    assert whole.numel() == flat.numel() + 2 * g
    inside = _bits(flat)[~written]
    assert inside.numel() == flat.numel() - int(written.sum()) and bool((inside == sent).all()), case["id"] + ": wrote outside its set"
    return worst


@pytest.mark.parametrize("case,mode", PARAMS, ids=["%s-%s" % (c["id"], "fp32" if m else "split16") for c, m in PARAMS])
def test_launch_matches_the_float64_reference(case, mode, lib, vxcfg):
    vxcfg.set(conv_fp32=mode)
    buf = rc.LayerBuffers(lib, case, guard=True)
    assert float(buf.x[..., :case["cin"]].abs().max()) <= 2 and float(buf.w.abs().max()) <= 2          # the premise of the split bound
    if case["in_extra"]:
        assert bool(torch.isnan(buf.x[..., case["cin"]:]).all())
    code, dry, _, _ = rc.dry_run(lib, rc.layer_args(case, buf.ptr))
    assert code == 0, (case["id"], lib.vx_last_error_string())
    assert buf.launch() == dry, case["id"]
    fam = ref.family_of(dry)
    worst = check_launch(case, buf, fam)
    print("RATIO %s %s %.4f" % (fam, case["id"], worst))


# ---- the device seed word -------------------------------------------------------------------------------------------------------------
SEED_CASES = {"mfma": "epi:16->8:2x3x5x6:hash", "s16": "epi:64->32:2x3x5x6:hash", "rows": "rowsnd:16->8:2x2x2x23171:hash",
              "generic": "epi:8->8:2x2x2x2:hash"}


@pytest.mark.parametrize("fam", sorted(SEED_CASES))
def test_seed_dev_is_added_to_drop_seed(fam, lib, vxcfg):
    """drop_seed = s with the device word w is, bit for bit, drop_seed = s + w (mod 2^32) without one, and not drop_seed = s"""
    vxcfg.set(conv_fp32=0)
    case = BY_ID[SEED_CASES[fam]]
    s, w = 0xFFFFFFF0, 0x35            # the sum wraps
    buf = rc.LayerBuffers(lib, case, guard=True)
    assert ref.family_of(buf.launch(drop_seed=s, seed_dev=w)) == fam
    with_word = buf.whole.clone()
    check_launch(case, buf, fam, seed_dev=w, drop_seed=s)
    buf.launch(drop_seed=(s + w) % (1 << 32))
    assert torch.equal(_bits(buf.whole), _bits(with_word))
    buf.launch(drop_seed=s)
    assert not torch.equal(_bits(buf.whole), _bits(with_word))
    check_launch(case, buf, fam, drop_seed=s)


# ---- the range word -------------------------------------------------------------------------------------------------------------------
RANGE_CASES = {"mfma": ("epi:16->8:2x3x5x6:none", "epi:16->8:2x3x5x6:hash"), "s16": ("epi:64->32:2x3x5x6:none", "epi:64->32:2x3x5x6:hash"),
               "rows": ("bound:16->8:2x2x2x23171", "rowsnd:16->8:2x2x2x23171:hash", "rowsnd:32->16:2x2x2x23171")}
RANGE_SCALE = 6.0e4                    # inputs stay below 65504, the split-fp16 kernel's contract


def _stored_max(case, buf):
    return ref.gather(case, buf.out).abs().max()


@pytest.mark.parametrize("fam,cid", [(f, c) for f in sorted(RANGE_CASES) for c in RANGE_CASES[f]])
def test_range_word_is_the_largest_stored_magnitude(fam, cid, lib, vxcfg):
    """outputs past 32768: the word holds exactly the float bits of max |stored value|, taken after activation and dropout; an
    ordinary tensor leaves it 0.  Cin 16 / 32 also where the route is the row-streaming kernel"""
    vxcfg.set(conv_fp32=0)
    case = BY_ID[cid]
    buf = rc.LayerBuffers(lib, case, guard=True, scale=RANGE_SCALE)
    E = torch.cat([ref.expected(case, buf.x[n0:n0 + 1, ..., :case["cin"]], buf.w, buf.b, buf.mask, sample0=n0)[0].abs().amax().view(1)
                   for n0 in range(case["vol"][0])]).max()
    assert float(E) > 40000.0                                      # the premise, from the reference
    assert ref.family_of(buf.launch()) == fam
    top = _stored_max(case, buf)
    assert float(top) >= 32768.0 and abs(float(top) - float(E)) <= 1e-3 * float(E)
    assert int(buf.range.item()) == int(_bits(top.view(1)).item()), (cid, buf.range.view(torch.float32).item(), float(top))
    small = rc.LayerBuffers(lib, case, guard=True)
    assert ref.family_of(small.launch()) == fam
    assert float(_stored_max(case, small)) < 32768.0 and int(small.range.item()) == 0


def test_range_word_is_left_alone_by_the_generic_kernel(lib, vxcfg):
    """48 -> 8 runs on the generic kernel only, which does not record the range (include/values_amd.h, vx_convT_args.range_flag)"""
    vxcfg.set(conv_fp32=0)
    case = rc._case("range", 48, 8, (2, 2, 2, 2))
    buf = rc.LayerBuffers(lib, case, guard=True, scale=RANGE_SCALE)
    for init in (0, 123):
        assert ref.family_of(buf.launch(range_init=init)) == "generic"
        assert float(_stored_max(case, buf)) >= 32768.0 and int(buf.range.item()) == init
    check_launch(case, buf, "generic")
