"""Host-only contraction of a coefficient posterior (ace_coef_contract)
against numpy.einsum: the tails of pred_cpp / pred_marginal_cpp
(src/pred_cpp.cpp:20-29, 70-78) on every (covariate point, weight row) pair.
Agreement to 1e-14 relative to the terms summed: the summation order is the
only difference."""
import numpy as np
import pytest

TOL = 1e-14


@pytest.fixture(scope="module")
def N():
    from additivecausalexpansion_amd import native
    return native


def _inputs(nx, B, nz, seed, negative=False):
    rng = np.random.default_rng(seed)
    mean = rng.normal(size=(nx, B))
    G = rng.normal(size=(nx, B, B))
    cov = np.einsum("cij,ckj->cik", G, G)  # symmetric positive semidefinite
    if negative:
        cov = -cov
    W = rng.normal(size=(nz, B))
    return mean, cov, W


def _ref(mean, cov, W, offset, scale, shift, noise):
    a = np.einsum("jb,cb->cj", W, mean)
    q = np.einsum("jb,cbd,jd->cj", W, cov, W)
    # the magnitude of the terms each sum is formed from
    ta = np.einsum("jb,cb->cj", np.abs(W), np.abs(mean)) + abs(shift)
    tq = np.einsum("jb,cbd,jd->cj", np.abs(W), np.abs(cov), np.abs(W)) + abs(noise)
    mp = offset + scale * (a + shift)
    var = scale ** 2 * np.abs(q + noise)
    sd = np.sqrt(var)
    ci = np.stack([mp - 1.96 * sd, mp + 1.96 * sd], axis=2)
    return mp, ci, var, abs(offset) + scale * ta, scale ** 2 * tq


@pytest.mark.parametrize("nx,B,nz", [(7, 5, 4), (3, 1, 6), (9, 17, 1), (1, 1, 1), (40, 10, 13)])
@pytest.mark.parametrize("negative", [False, True])
def test_contract_matches_einsum(N, nx, B, nz, negative):
    mean, cov, W = _inputs(nx, B, nz, seed=nx + 10 * B, negative=negative)
    for offset, scale, shift, noise in ((0.3, 1.7, 0.13, 0.05), (0.0, 2.125, 0.0, 0.0)):
        got = N.coef_contract(mean, cov, W, offset, scale, shift, noise)
        mp, ci, var, tm, tv = _ref(mean, cov, W, offset, scale, shift, noise)
        assert got["map"].shape == (nx, nz) and got["var"].shape == (nx, nz)
        assert got["ci"].shape == (nx, nz, 2)
        assert np.all(np.abs(got["map"] - mp) <= TOL * tm)
        assert np.all(np.abs(got["var"] - var) <= TOL * tv)
        # ci = map -+ 1.96 sd; sd = sqrt(var) carries half of var's relative error
        sd = np.sqrt(var)
        assert np.all(np.abs(got["ci"] - ci) <= TOL * (tm + 1.96 * sd)[:, :, None]
                      + 1.96 * TOL * (tv / np.maximum(sd, 1e-300))[:, :, None])
        assert np.all(got["var"] >= 0)


def test_contract_abs_of_a_negative_form(N):
    """|W^T cov W + noise| (src/pred_cpp.cpp:26): a negative form gives the
    variance of its magnitude, not NaN."""
    mean = np.zeros((2, 2))
    cov = np.zeros((2, 2, 2))
    cov[:, 0, 0] = [-4.0, 1.0]
    cov[:, 1, 1] = [1.0, -9.0]
    W = np.array([[1.0, 0.0], [0.0, 1.0]])
    got = N.coef_contract(mean, cov, W, 0.0, 2.0, 0.0, 0.0)
    assert np.array_equal(got["var"], 4.0 * np.array([[4.0, 1.0], [1.0, 9.0]]))
    cov[1, 1, 1] = -12.0
    got = N.coef_contract(mean, cov, W, 0.0, 1.0, 0.0, 3.0)  # noise inside the |.|
    assert np.array_equal(got["var"], np.array([[1.0, 4.0], [4.0, 9.0]]))
    assert np.array_equal(got["ci"][:, :, 1], 1.96 * np.sqrt(got["var"]))
    assert np.array_equal(got["ci"][:, :, 0], -got["ci"][:, :, 1])


def test_contract_layout_is_expand_grid(N):
    """Output index c + nx j (X fastest), ci as an (nx nz) x 2 matrix."""
    nx, B, nz = 4, 3, 5
    mean, cov, W = _inputs(nx, B, nz, seed=3)
    got = N.coef_contract(mean, cov, W, 0.1, 1.3, 0.2, 0.01)
    flat = np.ravel(got["map"], order="F")
    ci2 = got["ci"].reshape((nx * nz, 2), order="F")
    for j in range(nz):
        one = N.coef_contract(mean, cov, W[j:j + 1], 0.1, 1.3, 0.2, 0.01)
        assert np.array_equal(flat[nx * j:nx * (j + 1)], one["map"][:, 0])
        assert np.array_equal(ci2[nx * j:nx * (j + 1)], one["ci"][:, 0, :])


def test_contract_rejects_bad_shapes(N):
    import additivecausalexpansion_amd as A
    with pytest.raises(A.AceError):
        N.coef_contract(np.zeros(3), np.zeros((3, 1, 1)), np.zeros((1, 1)))
