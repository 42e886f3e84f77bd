"""CPU checks of the host contraction of a group-summed coefficient posterior
(ace_coef_group_contract / native.coef_group_contract) against a numpy
restatement: map = offset + scale (W_j . gmean_g / |g| + shift), var =
scale^2 |W_j^T C_gg W_j| / |g|^2, ci = map -+ 1.96 sqrt(var) and the signed
cov[g, j, j'] = scale^2 W_j^T C_gg W_j' / |g|^2.  The sums are a few terms of
order one in another association than numpy's, so the results are held to
1e-12 relative (plus 1e-13 of the largest entry where a quadratic form
cancels)."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.lib()
    return pkg


def _posterior(G, B, seed, empty=None):
    rng = np.random.default_rng(seed)
    gmean = rng.normal(size=(G, B))
    M = rng.normal(size=(G * B, G * B + 3))
    gcov = (M @ M.T).reshape((G, B, G, B), order="F")     # index g + G b on both sides
    # an indefinite block too (Q6): flip one group's sign
    gcov[G - 1, :, G - 1, :] *= -1.0
    gcount = rng.integers(1, 40, size=G).astype(np.int64)
    if empty is not None:
        gcount[empty] = 0
    return gmean, gcov, gcount


def _restate(gmean, gcov, gcount, W, offset, scale, shift):
    G, B = gmean.shape
    nz = W.shape[0]
    mp, var = np.empty((G, nz)), np.empty((G, nz))
    cov = np.empty((G, nz, nz))
    with np.errstate(divide="ignore", invalid="ignore"):
        for g in range(G):
            C = gcov[g, :, g, :]
            cnt = float(gcount[g])
            mp[g] = offset + scale * (W @ gmean[g] / cnt + shift)
            cov[g] = scale ** 2 * (W @ C @ W.T) / cnt ** 2
            var[g] = scale ** 2 * np.abs(np.einsum("jb,bc,jc->j", W, C, W)) / cnt ** 2
    sd = np.sqrt(var)
    return mp, np.stack([mp - 1.96 * sd, mp + 1.96 * sd], axis=2), var, cov


@pytest.mark.parametrize("nz", [1, 7])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("G", [1, 4])
def test_contract_matches_numpy(A, G, B, nz):
    gmean, gcov, gcount = _posterior(G, B, seed=10 * G + B)
    W = np.random.default_rng(nz).normal(size=(nz, B))
    offset, scale, shift = 0.3, 1.7, -0.2
    got = A.coef_group_contract(gmean, gcov, gcount, W, offset, scale, shift, return_cov=True)
    mp, ci, var, cov = _restate(gmean, gcov, gcount, W, offset, scale, shift)
    assert got["map"].shape == (G, nz) and got["ci"].shape == (G, nz, 2)
    assert got["cov"].shape == (G, nz, nz)
    big = np.max(np.abs(cov))
    assert np.allclose(got["map"], mp, rtol=1e-12, atol=1e-13)
    assert np.allclose(got["var"], var, rtol=1e-12, atol=1e-13 * big)
    assert np.allclose(got["cov"], cov, rtol=1e-12, atol=1e-13 * big)
    assert np.allclose(got["ci"], ci, rtol=1e-12, atol=1e-13 * (1 + np.sqrt(big)))
    # symmetric in (j, j') bit for bit; its diagonal is var where that is nonnegative
    assert np.array_equal(got["cov"], got["cov"].transpose(0, 2, 1))
    d = np.einsum("gjj->gj", got["cov"])
    pos = d >= 0
    assert (~pos).any() and (G == 1 or pos.any())  # both signs occur (the flipped block)
    assert np.allclose(d[pos], got["var"][pos], rtol=1e-12, atol=1e-13 * big)
    assert np.allclose(-d[~pos], got["var"][~pos], rtol=1e-12, atol=1e-13 * big)
    # without cov the other outputs are the same bits
    plain = A.coef_group_contract(gmean, gcov, gcount, W, offset, scale, shift)
    assert "cov" not in plain
    for k in ("map", "ci", "var"):
        assert np.array_equal(plain[k], got[k])


@pytest.mark.parametrize("B", [1, 5])
def test_empty_group_gives_nan(A, B):
    G, nz = 3, 4
    gmean, gcov, gcount = _posterior(G, B, seed=3, empty=1)
    gmean[1] = 0.0                     # what a device pass returns for an empty group
    gcov[1] = 0.0
    gcov[:, :, 1, :] = 0.0
    W = np.random.default_rng(8).normal(size=(nz, B))
    got = A.coef_group_contract(gmean, gcov, gcount, W, 0.0, 2.0, 0.0, return_cov=True)
    for k in ("map", "var", "ci", "cov"):
        assert np.all(np.isnan(got[k][1])), k
        assert np.all(np.isfinite(got[k][[0, 2]])), k
    mp, ci, var, cov = _restate(gmean, gcov, gcount, W, 0.0, 2.0, 0.0)
    assert np.allclose(got["map"], mp, rtol=1e-12, atol=1e-13, equal_nan=True)
    assert np.allclose(got["var"], var, rtol=1e-12, atol=1e-13 * np.nanmax(np.abs(cov)),
                       equal_nan=True)


def test_bad_arguments_raise(A):
    gmean, gcov, gcount = _posterior(2, 3, seed=1)
    with pytest.raises(A.AceError):
        A.coef_group_contract(gmean, gcov, gcount[:1], np.ones((2, 3)))
    with pytest.raises(A.AceError):
        A.coef_group_contract(gmean[0], gcov, gcount, np.ones((2, 3)))
