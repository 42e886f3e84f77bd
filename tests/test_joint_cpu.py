"""CPU checks of the joint-posterior referee (tests/joint_ref.py): its
diagonal is the oracle's pred_cpp / pred_marginal_cpp variance, and the
inputs of tests/test_joint_gpu.py are as definite as its factor tests need
(or, for the failure case, as indefinite).  No GPU here."""
import numpy as np
import pytest

import joint_ref as J

KERNELS = ["SE", "Matern32"]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", list(J.CASES))
@pytest.mark.parametrize("marginal", [False, True])
def test_referee_diagonal_is_the_oracle_variance(kernel, case, marginal):
    r = J.joint(case, kernel, marginal)
    orc = r["oracle"]
    d = np.diag(r["cov"])
    # the oracle: (scale sqrt|d|)^2; these states are definite, so |d| = d
    assert np.all(d > 0)
    assert np.all(np.abs(d - orc["var"]) <= 1e-13 * np.diag(r["terms"]))
    assert np.all(np.abs(r["map"] - orc["map"]) <= 1e-13 * (1 + np.abs(orc["map"])))
    # the reference's matrix is symmetric up to the rounding of its products
    assert np.max(np.abs(r["cov"] - r["cov"].T)) <= 1e-12 * np.max(r["terms"])


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", list(J.CASES))
@pytest.mark.parametrize("marginal", [False, True])
def test_factor_inputs_are_safely_definite(kernel, case, marginal):
    """lambda_min(ref) + jitter >= 100 COV_TOL max(terms): the device's C,
    within COV_TOL terms of the referee's, is then definite with a margin, so
    info == 0 is a property of the inputs and not of the rounding."""
    r = J.joint(case, kernel, marginal)
    lmin = np.linalg.eigvalsh(r["cov"])[0]
    jit = J.jitter_of(kernel, marginal)
    need = 100 * J.COV_TOL * np.max(r["terms"])
    assert lmin + jit >= need, (lmin, jit, need)
    if not marginal:
        assert lmin >= r["scale"] ** 2 * r["es"] * (1 - 1e-9)  # the noise floor
    L = J.factor(r["cov"], jit)
    assert J.factor_residual_ratio(L, r["cov"] + jit * np.eye(L.shape[0])) <= J.FACTOR_MARGIN


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("marginal", [False, True])
def test_q6_mix_is_strongly_indefinite(kernel, marginal):
    """Kernels at theta + 0.02 against the inverse at theta (Q6): C at 300 / 70
    has eigenvalues far below zero, out of reach of any jitter of the size of
    rounding -- the deterministic failure case of the GPU tests."""
    r = J.joint("300/70", kernel, marginal, mix=True)
    lmin = np.linalg.eigvalsh(r["cov"])[0]
    assert lmin < -0.5
    with pytest.raises(np.linalg.LinAlgError):
        J.factor(r["cov"], 1e-5)


def test_states_are_read_only():
    r = J.joint("130/9", "SE", False)
    with pytest.raises(ValueError):
        r["cov"][0, 0] = 0.0
