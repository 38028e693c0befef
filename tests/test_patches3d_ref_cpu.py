"""CPU: tests/patches3d_ref.py, the restatements tests/test_gpu_patches3d_matrix.py compares the kernels of patches3d.hip
and vx_softmax_accumulate with, against the reference's recorded accumulation (accum_24.npz) and against compose_case
(itself pinned to the reference's concat_data); and the properties of that file's inputs the GPU tests rely on."""
import numpy as np
import pytest

from tests import dataset3d_trees as trees
from tests import patches3d_ref as pr
from tests.formula import formula_tensor
from tests.helpers import load_npz


def test_accumulate_ref_equals_the_reference_concat_data():
    """accum_24.npz: the reference's DataCarrier3D.concat_data over a 24^3 image, patch 16, overlap 0.5 (count up to 8),
    recorded in float32: 2e-6 on sums of up to 8 addends in [0, 1] is the fixture's own precision (8 * 2^-24 * a few)"""
    from oracle.predict_oracle import crop_indices
    g = load_npz("accum_24.npz")
    size, patch, T = 24, 16, 3
    crops = crop_indices((size,) * 3, patch, 0.5)
    fake = np.abs(formula_tensor((len(crops), T, 2, patch, patch, patch), tag=55, scale=1.0))
    fake = fake / fake.sum(axis=2, keepdims=True)                        # softmax(log p) == p
    sums, counts = pr.accumulate_ref(np.log(fake), [(c[0][0], c[1][0], c[2][0]) for c in crops], (size,) * 3, T, 2)
    assert sums.dtype == np.float64 and counts.dtype == np.int64
    np.testing.assert_allclose(sums, g["softmax_sum"], atol=2e-6, rtol=0)
    np.testing.assert_array_equal(counts, g["num_predictions"][0])
    assert counts.max() == 8 and counts.min() == 1
    # one image index per patch: the same patches split over two images give each image its own
    image = [b % 2 for b in range(len(crops))]
    s2, c2 = pr.accumulate_ref(np.log(fake), [(c[0][0], c[1][0], c[2][0]) for c in crops], [(size,) * 3] * 2, T, 2, image=image)
    np.testing.assert_allclose(s2[0] + s2[1], sums, atol=1e-14, rtol=0)
    np.testing.assert_array_equal(c2[0] + c2[1], counts)
    assert c2[0].sum() == c2[1].sum() == counts.sum() // 2


@pytest.mark.parametrize("name", list(trees.CASES))
def test_composite_ref_equals_compose_case(name):
    from values_amd import crop_indices
    from values_amd.dataset3d import compose_case
    shape, _, overlap = trees.CASES[name]
    crops = crop_indices(shape, trees.PATCH, overlap)
    labels = [trees.label(name, r) for r in range(3)]
    want = compose_case(trees.image(name), labels, crops)
    cnt = pr.count_map_of(shape, crops)
    got = pr.composite_ref(trees.image(name), labels, cnt)
    np.testing.assert_array_equal(cnt, want["num_predictions"])
    for k in ("data", "gt_seg", "gt"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert got["n_bad"] == 0


def test_composite_ref_wraps_and_counts_as_numpy_does():
    cnt = np.array([3, 1, 0, 12, 2])
    lab32 = np.array([2 ** 31 - 1, -1, 300, -1, 7], dtype=np.int32)
    lab64 = np.array([2 ** 32 + 7, 5, -1, 255, 256], dtype=np.int64)
    got = pr.composite_ref(np.array([1.5, np.nan, np.inf, -np.inf, 2.0]), [lab32, lab64], cnt)
    seg = np.zeros((2, 5), dtype=np.intc)
    with np.errstate(over="ignore"):
        for v in range(5):
            for _ in range(cnt[v]):
                seg[:, v] += np.array([lab32[v], lab64[v]]).astype(np.intc)      # the intc additions, made
    assert seg[0, 0] == 2 ** 31 - 3                                              # 3 (2^31 - 1) wrapped
    np.testing.assert_array_equal(got["gt_seg"], seg / np.clip(cnt, 1, None))
    np.testing.assert_array_equal(got["gt"], (seg / np.clip(cnt, 1, None)).astype(np.intc))
    assert got["gt_seg"][1, 0] == 7.0                                            # astype(intc) of 2^32 + 7 ...
    assert got["n_bad"] == 4 + 3                                                 # ... which is counted all the same; so is count 0
    np.testing.assert_array_equal(got["data"], [1.5, np.nan, 0.0, -np.inf, 2.0])


@pytest.mark.parametrize("C", range(2, 9))
def test_hot_logits_are_exactly_one_hot_in_float32(C):
    assert np.exp(np.float32(-200)) == 0.0
    P = (3, 5, 7)
    lg = pr.hot_logits(4, 3, C, P)
    assert lg.dtype == np.float32 and lg.shape == (4, 3, C) + P
    p = pr.softmax_f32(lg, 2)
    h = pr.hot_class(4, 3, C, P)
    want = (np.arange(C).reshape(1, 1, C, 1, 1, 1) == h[:, :, None]).astype(np.float32)
    assert np.array_equal(p, want) and (p.sum(2) == 1).all()
    assert len(np.unique(h)) == C


NONCUBIC = [P for P in pr.PATCHES if len(set(P)) > 1]


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("P", NONCUBIC)
def test_placement_cases_can_see_a_transposed_decode(P, overlap, multi):
    assert len(NONCUBIC) == 3
    dims, patches = pr.placement(P, overlap, multi)
    T = pr.placement_T(P)
    image, origins = [i for i, _ in patches], [o for _, o in patches]
    for C in (c for c in range(2, 9) if P in pr.placement_patches(c)):
        lg = pr.hot_logits(len(patches), T, C, P)
        sums, counts = pr.accumulate_ref(lg, origins, dims, T, C, image=image)
        for swap in ("01", "12"):
            other, c2 = pr.accumulate_ref(lg, origins, dims, T, C, image=image, decode=swap)
            assert all(np.array_equal(a, b) for a, b in zip(counts, c2))
            # image 0 alone is what the K14 route runs; float32 is what the GPU test compares
            assert not np.array_equal(sums[0].astype(np.float32), other[0].astype(np.float32)), (P, C, swap)


@pytest.mark.parametrize("P", pr.PATCHES)
def test_placement_cases_are_what_the_issue_asks_for(P):
    for overlap in (0, 1):
        dims, patches = pr.placement(P, overlap, True)
        assert len(dims) == 3 and len(set(dims)) == 3 and all(d[2] % 2 == 1 for d in dims)
        zero = [o for i, o in patches if i == 0]
        assert {o[2] % 4 for o in zero} == {0, 1, 2, 3}
        X, Y, Z = dims[0]
        for a in range(3):                                   # a crop past the image on axis a only
            assert any(o[a] + P[a] > dims[0][a] and all(o[b] + P[b] <= dims[0][b] for b in range(3) if b != a) for o in zero), a
        assert [i for i, _ in patches][:3] == [0, 1, 2]       # the patches of the images are interleaved
        lg = np.zeros((len(patches), 1, 2) + P, dtype=np.float32)
        _, counts = pr.accumulate_ref(lg, [o for _, o in patches], dims, 1, 2, image=[i for i, _ in patches])
        if overlap:
            assert counts[0].max() >= 12 and counts[1].max() == 3
        else:
            assert all(c.max() == 1 for c in counts)          # disjoint: the plain read-modify-write form may run them


@pytest.mark.parametrize("C", [2, 5, 8])
def test_numeric_bound_holds_for_the_float32_emulation(C):
    """the bound of the GPU numeric case is not too tight: a float32 numpy run of the kernel's expressions stays inside"""
    P, T = (3, 5, 7), 3
    dims, patches = pr.placement(P, 1, True)
    image, origins = [i for i, _ in patches], [o for _, o in patches]
    lg = pr.numeric_logits(len(patches), T, C, P, seed=100 + C)
    assert (lg.max(2) - lg.min(2)).max() > 100 and (lg.max(2) == lg.min(2)).any()
    sums, counts = pr.accumulate_ref(lg, origins, dims, T, C, image=image)
    got = pr.accumulate_f32(lg, origins, dims, image=image)
    worst = 0.0
    for s, c, g in zip(sums, counts, got):
        bound = pr.numeric_bound(c, C)
        diff = np.abs(g.astype(np.float64) - s)
        assert (diff <= bound[None, None]).all()
        worst = max(worst, float((diff / np.maximum(bound, 1e-300)[None, None]).max()))
    print(f"accumulate numeric C{C}: float32 emulation max |diff| / bound = {worst:.3f}")
    assert counts[0].max() >= 12


def test_gather_ref_converts_the_planted_values_as_astype_does():
    f64 = pr.gather_specials("float64")
    got = pr.gather_ref(f64.reshape(1, 1, -1), (0, 0, 0), (1, 1, len(f64)))[0, 0]
    assert got[0] != 0 and got[0] < 2.0 ** -126                                   # 1e-40 stays a denormal
    assert got[1] == 0 and got[2] == 2.0 ** -148                                  # ties to even at the bottom
    assert got[3] == np.inf and got[4] == -np.inf
    assert not np.signbit(got[5]) and np.signbit(got[6]) and got[6] == 0 and np.isnan(got[7])
    assert got[10] == 1 and got[11] == np.float32(1 + 2.0 ** -22) and got[12] == -1
    u32 = pr.gather_ref(pr.gather_specials("uint32").reshape(1, 1, -1), (0, 0, 0), (1, 1, 3))[0, 0]
    assert u32.tolist() == [2.0 ** 24, 2.0 ** 24 + 4, 2.0 ** 32]
    i32 = pr.gather_ref(pr.gather_specials("int32").reshape(1, 1, -1), (0, 0, 0), (1, 1, 4))[0, 0]
    assert i32.tolist() == [2.0 ** 31, -2.0 ** 31, -2.0 ** 24, 2.0 ** 24 + 4]
