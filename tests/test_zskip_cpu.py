"""ace_zero_pattern_order (host only): the stable order of the points by
their pattern of exact zeros in the basis and the slice masks of its
64-point blocks -- what ace_model_set_data computes once per fit for the
pair kernels' slice skip.  Every expectation is recomputed
here with numpy from the definition."""
import numpy as np
import pytest

from additivecausalexpansion_amd.synthetic import make_problem


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.lib()
    return pkg


def np_masks(Z, perm):
    """bit j of word k: some point of perm[64 k : 64 k + 64] has Z[:, j] != 0;
    a last block that is not full: every bit."""
    n, ZS = Z.shape
    nz = (Z[perm] != 0)
    out = np.zeros((n + 63) // 64, dtype=np.uint32)
    for k in range(out.size):
        blk = nz[64 * k:64 * k + 64]
        bits = np.ones(ZS, bool) if blk.shape[0] < 64 else blk.any(axis=0)
        out[k] = sum(1 << j for j in range(ZS) if bits[j])
    return out


def runs(keys):
    """the distinct consecutive values of a sequence"""
    r = [keys[0]]
    for k in keys[1:]:
        if k != r[-1]:
            r.append(k)
    return r


def check_order(Z, perm):
    """perm is a permutation, sorted by the pattern's size, equal patterns
    contiguous and in input order."""
    n = Z.shape[0]
    assert sorted(perm.tolist()) == list(range(n))
    keys = [tuple(r) for r in (Z[perm] != 0)]
    size = [sum(k) for k in keys]
    assert size == sorted(size)
    groups = runs(keys)
    assert len(groups) == len(set(keys)), "a pattern is split into two runs"
    for g in groups:
        idx = [int(perm[i]) for i in range(n) if keys[i] == g]
        assert idx == sorted(idx), "equal patterns must keep their input order"
    return groups


def test_no_exact_zeros_gives_identity_and_full_masks(A):
    rng = np.random.default_rng(0)
    Z = np.asfortranarray(rng.normal(size=(300, 5)))
    assert not np.any(Z == 0)
    perm, mask = A.zero_pattern_order(Z)
    assert np.array_equal(perm, np.arange(300))
    assert mask.dtype == np.uint32 and mask.size == 5 and np.all(mask == 31)
    # B <= 3 in make_problem: z and z^2 have no exact zero either (n even: the
    # median that centres z is then no sample point)
    for B in (2, 3):
        Zb = make_problem(258, 2, B, seed=5)[2]
        perm, mask = A.zero_pattern_order(Zb)
        assert np.array_equal(perm, np.arange(258)) and np.all(mask == (1 << (B - 1)) - 1)


def test_spline_basis_groups_are_contiguous_sparsest_first_and_stable(A):
    """make_problem's basis at n = 1000, B = 10: nine columns that are exactly
    zero on 0, 0, 1/8, .. 7/8 of the points.  The first two columns are never
    zero, so the nine columns give eight distinct (nested) patterns, with 2 ..
    9 nonzero columns, 125 points each."""
    Z = make_problem(1000, 3, 10, seed=1000)[2]
    assert Z.shape == (1000, 9)
    assert np.array_equal((Z == 0).mean(axis=0), [0, 0, .125, .25, .375, .5, .625, .75, .875])
    perm, mask = A.zero_pattern_order(Z)
    groups = check_order(Z, perm)
    assert [sum(g) for g in groups] == [2, 3, 4, 5, 6, 7, 8, 9]
    assert all(g == tuple([True] * k + [False] * (9 - k)) for g, k in zip(groups, range(2, 10)))
    assert np.array_equal(mask, np_masks(Z, perm))
    # n = 1000 is not a multiple of 64: the last block counts as fully active,
    # the first holds the sparsest pattern alone
    assert mask[-1] == (1 << 9) - 1 and mask[0] == 0b11


@pytest.mark.parametrize("n", [64, 200, 1000, 1031])
def test_masks_match_numpy_on_scattered_zeros(A, n):
    rng = np.random.default_rng(n)
    Z = rng.normal(size=(n, 7))
    Z[rng.random(Z.shape) < 0.3] = 0.0
    Z[:40, 3] = 0.0  # with some luck for the sort: a block-sized run of one column
    Z = np.asfortranarray(Z)
    perm, mask = A.zero_pattern_order(Z)
    check_order(Z, perm)
    assert np.array_equal(mask, np_masks(Z, perm))


def test_negative_zero_counts_as_zero(A):
    rng = np.random.default_rng(3)
    Z = rng.normal(size=(256, 3))
    Z[:128, 2] = 0.0
    Zs = Z.copy()
    Zs[:128:2, 2] = -0.0
    assert np.signbit(Zs[0, 2]) and not np.signbit(Zs[1, 2])
    pa, ma = A.zero_pattern_order(np.asfortranarray(Z))
    pb, mb = A.zero_pattern_order(np.asfortranarray(Zs))
    assert np.array_equal(pa, pb) and np.array_equal(ma, mb)
    assert np.array_equal(pa, np.arange(256))  # the zero rows already lead
    assert ma.tolist() == [0b011, 0b011, 0b111, 0b111]


def test_column_that_is_zero_everywhere(A):
    rng = np.random.default_rng(4)
    Z = rng.normal(size=(192, 4))
    Z[:, 1] = 0.0
    perm, mask = A.zero_pattern_order(np.asfortranarray(Z))
    assert np.array_equal(perm, np.arange(192))  # one pattern: the identity
    assert np.all(mask == 0b1101)


def test_more_than_32_columns_returns_no_mask(A):
    rng = np.random.default_rng(5)
    Z = rng.normal(size=(130, 33))  # B - 1 = 33
    Z[rng.random(Z.shape) < 0.5] = 0.0
    Z = np.asfortranarray(Z)
    perm, mask = A.zero_pattern_order(Z)
    assert mask is None
    check_order(Z, perm)
    # 32 columns still fit a word
    perm, mask = A.zero_pattern_order(np.asfortranarray(Z[:, :32]))
    assert mask is not None and np.array_equal(mask, np_masks(Z[:, :32], perm))
