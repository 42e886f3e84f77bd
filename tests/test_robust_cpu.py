"""CPU checks of robust_treatment's host side: ace_robust_levels
(native.robust_levels) against a Python restatement of the R formulas
(R/robust_treatment.R:83-84, 94 with R's default type-7 quantile), bit for
bit, and the block-sum identity the GPU tests' reference uses."""
import numpy as np
import pytest

from robust_ref import indicator, levels_ref, step_post


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.lib()
    return pkg


def _same(A, var, n_steps):
    thr, level = A.robust_levels(var, n_steps)
    rthr, rlevel = levels_ref(var, n_steps)
    assert thr.shape == (n_steps + 1,) and level.dtype == np.int32
    assert np.array_equal(thr, rthr), (thr, rthr)
    assert np.array_equal(level, rlevel)
    return thr, level


@pytest.mark.parametrize("nx,n_steps", [(150, 5), (257, 5), (260, 5), (1000, 31), (37, 1), (64, 7),
                                        (5, 31)])
def test_levels_random_inputs_bitwise(A, nx, n_steps):
    rng = np.random.default_rng(nx + n_steps)
    var = rng.gamma(2.0, 1e-3, size=nx)
    thr, level = _same(A, var, n_steps)
    assert np.all(np.diff(thr) >= 0) and thr[0] == var.min() and thr[-1] == var.max()
    assert level.min() == 0 and level.max() <= n_steps
    # numpy's default quantile is the same type-7 definition
    q = np.quantile(var, np.minimum(np.arange(n_steps + 1) * (1.0 / n_steps), 1.0))
    assert np.allclose(thr, q, rtol=1e-14, atol=0)


def test_levels_with_ties(A):
    rng = np.random.default_rng(3)
    var = np.round(rng.uniform(0, 1, size=200), 1)  # 11 distinct values
    _same(A, var, 5)
    _same(A, np.full(40, 0.25), 4)  # all equal: every threshold 0.25, every level 0
    thr, level = A.robust_levels(np.full(40, 0.25), 4)
    assert np.all(thr == 0.25) and np.all(level == 0)


@pytest.mark.parametrize("nx,n_steps", [(151, 5), (97, 4), (11, 10), (1, 5), (1, 1)])
def test_levels_integer_index_and_single_point(A, nx, n_steps):
    """(nx - 1) / n_steps an integer: the quantile index lands on an order
    statistic (up to the rounding of i * (1 / n_steps)); nx = 1."""
    rng = np.random.default_rng(nx)
    var = rng.uniform(0.1, 2.0, size=nx)
    thr, level = _same(A, var, n_steps)
    if nx == 1:
        assert np.all(thr == var[0]) and level[0] == 0


def test_levels_counts_are_nested(A):
    rng = np.random.default_rng(9)
    var = rng.uniform(size=333)
    thr, level = _same(A, var, 6)
    for t in range(7):
        assert np.array_equal(level <= t, var <= thr[t])


def test_levels_nonfinite_and_bad_steps(A):
    var = np.array([0.1, np.nan, 0.3])
    with pytest.raises(A.AceError, match="NONFINITE"):
        A.robust_levels(var, 3)
    with pytest.raises(A.AceError, match="NONFINITE"):
        A.robust_levels(np.array([0.1, np.inf]), 3)
    for bad in (0, 32, -1):
        with pytest.raises(A.AceError, match="ARG"):
            A.robust_levels(np.array([0.1, 0.2, 0.3]), bad)


def test_block_sum_reference_identity():
    """Prefix sums of E^T C E (label = 2 level + treated) are the subset sums
    C[keep][:, keep].sum() the reference forms per step -- numpy alone."""
    rng = np.random.default_rng(17)
    nx, n_steps = 90, 5
    M = rng.normal(size=(nx, nx + 5))
    C = M @ M.T  # SPD
    var = rng.uniform(size=nx)
    zx = (np.arange(nx) % 3 == 0)
    thr, level = levels_ref(var, n_steps)
    G = 2 * (n_steps + 1)
    E = indicator(2 * level + zx, G)
    assert np.array_equal(E.sum(axis=1), np.ones(nx))
    gcov = E.T @ C @ E
    scale = np.abs(C).sum()
    for t in range(n_steps + 1):
        keep = var <= thr[t]
        ate, att, atu = step_post(gcov, t)
        for got, sel in ((ate, keep), (att, keep & zx), (atu, keep & ~zx)):
            assert abs(got - C[np.ix_(sel, sel)].sum()) <= 1e-13 * scale
    # a label of -1 drops the point from every group
    lab = (2 * level + zx).copy()
    lab[::7] = -1
    E2 = indicator(lab, G)
    assert np.array_equal(E2.sum(axis=1), (lab >= 0).astype(float))
