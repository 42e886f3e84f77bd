"""GPU tests of the coefficient posterior (ace_model_coef_posterior) and the
response surfaces contracted from it (ace_model_predict_surface,
train.response_surface).

The reference is the oracle alone: Kc = cross(X2, X, ones, Z, theta)
["elements"] (the cross kernels with the test basis factor taken out),
m = Kc inv (y - mu), P = Kc inv Kc^T, and for the surfaces pred_cpp /
pred_marginal_cpp (src/pred_cpp.cpp:8-83) on the expanded grid.  pred_cpp's
outputs of a test row depend on that row alone (only the diagonal of
K_xx - tmp K_xX^T is used), so the grid is fed to it one treatment value at
a time: nz calls with nx rows, the same numbers as one call with nx nz rows.

Scales.  cov_c = diag(e^lambda) - P_c cancels terms as large as the prior
and the explained part, so its entries are held to COEF_TOL of
T_c[b,b'] = delta_bb' e^lambda_b + sqrt(P_c[b,b] P_c[b',b']); a surface
variance scale^2 |beta^T cov_c beta + noise| to SURF_TOL of
T = scale^2 (sum_b beta_b^2 e^lambda_b + (sum_b |beta_b| sqrt(P_c[b,b]))^2 +
noise).  Both bounds are set at <= 5x the largest error measured against the
oracle (profiles/coef_error_table.txt: cov 8.7e-10 of T_c, surface variances
3.9e-10 of T, both at n = 700, B = 10; VAR_TOL = 1.5e-9 of
tests/test_predict_gpu.py is the comparable figure for the same
cancellation).  The error is the resident inverse's against the oracle's
under the Q6 theta mix: the triangular and full-product forms, and sharded
against single models, differ by 4e-13 of the same scales.
"""
import os

import numpy as np

from conftest import record_error, run_child
import pytest
from test_gpu import close
from test_predict_gpu import _fit_state

pytestmark = pytest.mark.gpu

COEF_TOL = 4e-9
SURF_TOL = 1.5e-9

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(300, 3, 5, 70), (700, 20, 10, 257), (130, 1, 1, 9), (200, 2, 17, 33)]
KERNELS = ["SE", "Matern32"]
MEAN_Y, STD_Y, STD_Z = 0.3, 1.7, 0.8


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.default_context()
    return pkg


@pytest.fixture(scope="module")
def O():
    from oracle import ace_oracle
    return ace_oracle


_CASES = {}


def _case(A, O, kernel, n, p, B, nx):
    """The fitted model (Q6 theta mix), the test points and the oracle's m, P
    of one case, computed once and shared by the tests (never modified)."""
    key = (kernel, n, p, B, nx)
    if key in _CASES:
        return _CASES[key]
    from additivecausalexpansion_amd.synthetic import make_problem
    m, y, X, Z, th, sy, inv = _fit_state(O, kernel, n, p, B, seed=n, A=A)
    _, X2, _, _, _ = make_problem(nx, p, B, seed=n + 1)
    _, _, Z3, _, _ = make_problem(50, p, B, seed=n + 2)  # basis rows of the surfaces
    ones = np.ones((nx, max(B - 1, 0)), order="F")
    Kc = O.KERNELS[kernel][1](X2, X, ones, Z, th)["elements"]  # nx x n x B
    Kf = np.ascontiguousarray(Kc.transpose(0, 2, 1))           # nx x B x n
    TK = Kf @ inv
    c = dict(m=m, y=y, X=X, Z=Z, th=th, inv=inv, X2=X2, Z3=np.asfortranarray(Z3), Kc=Kc,
             mean=TK @ (y - th[1]), P=TK @ Kf.transpose(0, 2, 1), lam=th[2:2 + B].copy(),
             kernel=kernel, B=B, nx=nx)
    c["cov"] = np.eye(B)[None] * np.exp(c["lam"])[None, :, None] - c["P"]
    Pd = np.einsum("cbb->cb", c["P"])
    assert Pd.min() > 0  # the inverse is positive definite whatever the theta mix
    c["Pd"] = Pd
    c["Tc"] = np.eye(B)[None] * np.exp(c["lam"])[None, :, None] + np.sqrt(Pd[:, :, None] * Pd[:, None, :])
    _CASES[key] = c
    return c


def _coef_check(c, got, label, tol=COEF_TOL):
    err = float(np.max(np.abs(got["cov"] - c["cov"]) / c["Tc"]))
    record_error(f"{label}: max |err| / T_c", err, tol)
    return err


def _betas(B, Zrows, marginal):
    nz = Zrows.shape[0]
    if B == 1:
        return np.ones((nz, 1))
    return np.column_stack([np.zeros(nz) if marginal else np.ones(nz), Zrows])


def _surface_scale(c, beta, scale, noise):
    """T (nx x nz) of the module docstring."""
    prior = (beta ** 2) @ np.exp(c["lam"])                      # nz
    expl = (np.sqrt(c["Pd"]) @ np.abs(beta).T) ** 2             # nx x nz
    return scale ** 2 * (prior[None, :] + expl + noise)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,p,B,nx", CASES)
def test_coef_posterior_matches_oracle(A, O, kernel, n, p, B, nx):
    c = _case(A, O, kernel, n, p, B, nx)
    got = c["m"].coef_posterior(c["th"], c["X2"])
    assert got["mean"].shape == (nx, B) and got["cov"].shape == (nx, B, B)
    close(got["mean"], c["mean"])
    err = _coef_check(c, got, "coef cov")
    assert np.array_equal(got["cov"], got["cov"].transpose(0, 2, 1))
    again = c["m"].coef_posterior(c["th"], c["X2"])
    assert np.array_equal(again["mean"], got["mean"]) and np.array_equal(again["cov"], got["cov"])
    assert err <= COEF_TOL, err


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,p,B,nx", CASES)
def test_surface_matches_pred_cpp_on_the_grid(A, O, kernel, n, p, B, nx):
    c = _case(A, O, kernel, n, p, B, nx)
    sym, cross = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    th = c["th"]
    worst = 0.0
    for nz in (1, 7):
        Zb = np.asfortranarray(c["Z3"][:nz])
        got = c["m"].predict_surface(th, c["X2"], Zb, False, MEAN_Y, STD_Y, STD_Z)
        assert got["map"].shape == (nx, nz) and got["ci"].shape == (nx, nz, 2)
        ref = {k: [] for k in ("map", "ci", "var")}
        lowest = np.inf
        T = _surface_scale(c, _betas(B, Zb, False), STD_Y, np.exp(th[0]))
        for j in range(nz):
            Z2 = np.asfortranarray(np.repeat(Zb[j:j + 1], nx, axis=0))
            r = O.pred_cpp(c["y"], th[0], th[1], c["inv"], cross(c["X2"], c["X"], Z2, c["Z"], th)["full"],
                           sym(c["X2"], Z2, th)["full"], MEAN_Y, STD_Y)
            for k in ref:
                ref[k].append(r[k])
            lowest = min(lowest, float(np.min(r["var"] / T[:, j])))
        assert lowest > 1e-6  # the variances are not lost in T: the check below is not vacuous
        close(got["map"], np.stack(ref["map"], axis=1))
        close(got["ci"], np.stack(ref["ci"], axis=1), 1e-6, 1e-8)
        err = float(np.max(np.abs(got["var"] - np.stack(ref["var"], axis=1)) / T))
        record_error("surface var: max |err| / T", err, SURF_TOL)
        worst = max(worst, err)
    assert worst <= SURF_TOL, worst


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,p,B,nx", [CASES[0], CASES[2]])
def test_marginal_surface_matches_pred_marginal_cpp_on_the_grid(A, O, kernel, n, p, B, nx):
    c = _case(A, O, kernel, n, p, B, nx)
    sym, cross = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    th = c["th"]
    worst = 0.0
    for nz in (1, 7):
        dZ = np.asfortranarray(c["Z3"][:nz] * 0.7 + 0.1)  # a stand-in derivative basis
        got = c["m"].predict_surface(th, c["X2"], dZ, True, MEAN_Y, STD_Y, STD_Z)
        T = _surface_scale(c, _betas(B, dZ, True), STD_Y / STD_Z, 0.0)
        ref = {k: [] for k in ("map", "ci", "var")}
        for j in range(nz):
            Z2 = np.asfortranarray(np.repeat(dZ[j:j + 1], nx, axis=0))
            r = O.pred_marginal_cpp(c["y"], np.zeros(nx), th[0], th[1], c["inv"],
                                    cross(c["X2"], c["X"], Z2, c["Z"], th)["elements"],
                                    sym(c["X2"], Z2, th)["elements"], MEAN_Y, STD_Y, STD_Z, False)
            for k in ref:
                ref[k].append(r[k])
        close(got["map"], np.stack(ref["map"], axis=1))
        close(got["ci"], np.stack(ref["ci"], axis=1), 1e-6, 1e-8)
        err = float(np.max(np.abs(got["var"] - np.stack(ref["var"], axis=1)) / T))
        record_error("marginal surface var: max |err| / T", err, SURF_TOL)
        worst = max(worst, err)
    assert worst <= SURF_TOL, worst


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,p,B,nx", CASES)
def test_slice_kernel_rows_against_kernmat_cross(A, O, kernel, n, p, B, nx):
    """The slice kernel's rows against ace_kernmat_cross with a test side of
    ones.  The ABI cannot restrict that entry point to one slice of several,
    so for B > 1 the slices are added in ascending order and compared with its
    sum to 1e-14 of the terms (the sum fuses each slice's last product into
    the addition, the slices round it first); B = 1 is one slice: bit for bit."""
    from additivecausalexpansion_amd import native
    from additivecausalexpansion_amd._lib import KIND
    c = _case(A, O, kernel, n, p, B, nx)
    Kc = c["m"].coef_cross(c["th"], c["X2"])
    assert Kc.shape == (nx, n, B)
    close(Kc, c["Kc"])
    ones = np.ones((nx, max(B - 1, 0)), order="F")
    full = native._kernmat_cross(KIND[kernel], c["X2"], c["X"], ones, c["Z"], c["th"],
                                 elements=False)["full"]
    if B == 1:
        assert np.array_equal(Kc[:, :, 0], full)
        return
    acc = np.zeros((nx, n))
    for b in range(B):
        acc = acc + Kc[:, :, b]
    terms = np.sum(np.abs(Kc), axis=2)
    err = float(np.max(np.abs(acc - full) / terms))
    record_error("slice sum vs kernmat_cross: max |err| / sum |K_b|", err, 1e-14)
    assert err <= 1e-14, err


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r})
import additivecausalexpansion_amd as A
from additivecausalexpansion_amd.synthetic import make_problem
n, p, B, nx = 300, 3, 5, 70
y, X, Z, th0, sy = make_problem(n, p, B, seed=n)   # _fit_state's model and theta mix
m = A.DeviceModel({kernel!r}, n, p, B)
m.set_data(y, X, Z, sy)
m.para_update(2, th0.copy())
th = th0 + 0.02
th[1] = 0.13
_, X2, _, _, _ = make_problem(nx, p, B, seed=n + 1)
g = m.coef_posterior(th, X2)
np.savez({out!r}, mean=g["mean"], cov=g["cov"])
"""
_CHILD_OUT = {}


def _child(tmp_path_factory, kernel, **env):
    key = (kernel,) + tuple(sorted(env.items()))
    if key not in _CHILD_OUT:
        out = str(tmp_path_factory.mktemp("coef") / "g.npz")
        run_child(_CHILD.format(root=ROOT, kernel=kernel, out=out), env=dict(os.environ, **env),
                  timeout=100)
        with np.load(out) as f:
            _CHILD_OUT[key] = {k: f[k] for k in f.files}
    return _CHILD_OUT[key]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("chunk", [7, 64])
def test_chunking_does_not_change_a_bit(A, O, tmp_path_factory, kernel, chunk):
    """ACE_COEF_CHUNK = 7 (ten chunks of nx = 70) and 64 (one full chunk and a
    ragged one) against the unchunked pass of this process."""
    c = _case(A, O, kernel, *CASES[0])
    here = c["m"].coef_posterior(c["th"], c["X2"])
    got = _child(tmp_path_factory, kernel, ACE_COEF_CHUNK=str(chunk))
    assert np.array_equal(got["mean"], here["mean"])
    assert np.array_equal(got["cov"], here["cov"])


@pytest.mark.parametrize("kernel", KERNELS)
def test_full_product_agrees_with_triangular(A, O, tmp_path_factory, kernel):
    """ACE_PRED_TRI=0: T' = A^-1 Kc^T by the full symmetric product."""
    c = _case(A, O, kernel, *CASES[0])
    here = c["m"].coef_posterior(c["th"], c["X2"])
    got = _child(tmp_path_factory, kernel, ACE_PRED_TRI="0")
    close(got["mean"], here["mean"])
    assert np.array_equal(got["cov"], got["cov"].transpose(0, 2, 1))
    err = float(np.max(np.abs(got["cov"] - here["cov"]) / c["Tc"]))
    record_error("coef cov, full product vs triangular: max |diff| / T_c", err, COEF_TOL)
    assert err <= COEF_TOL, err
    assert _coef_check(c, got, "coef cov (ACE_PRED_TRI=0)") <= COEF_TOL


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_agrees_with_single(A, O, kernel, world):
    n, p, B, nx = CASES[0]
    c = _case(A, O, kernel, n, p, B, nx)
    here = c["m"].coef_posterior(c["th"], c["X2"])
    sh, *_ = _fit_state(O, kernel, n, p, B, seed=n, sharded=True, world=world, A=A)
    got = sh.coef_posterior(c["th"], c["X2"])
    close(got["mean"], here["mean"])
    assert np.array_equal(got["cov"], got["cov"].transpose(0, 2, 1))
    err = float(np.max(np.abs(got["cov"] - here["cov"]) / c["Tc"]))
    record_error("coef cov, sharded vs single: max |diff| / T_c", err, COEF_TOL)
    assert err <= COEF_TOL, err
    assert _coef_check(c, got, "coef cov (sharded)") <= COEF_TOL


@pytest.mark.parametrize("kernel", KERNELS)
def test_surface_agrees_with_device_predict_on_the_grid(A, O, kernel):
    n, p, B, nx = CASES[0]
    c = _case(A, O, kernel, n, p, B, nx)
    th, nz = c["th"], 7
    Zb = np.asfortranarray(c["Z3"][:nz])
    Xg = np.asfortranarray(np.tile(c["X2"], (nz, 1)))          # expand.grid: X fastest
    Zg = np.asfortranarray(np.repeat(Zb, nx, axis=0))
    got = c["m"].predict_surface(th, c["X2"], Zb, False, MEAN_Y, STD_Y, STD_Z)
    ref = c["m"].predict(th, Xg, Zg, MEAN_Y, STD_Y)
    close(np.ravel(got["map"], order="F"), ref["map"])
    close(got["ci"].reshape((nx * nz, 2), order="F"), ref["ci"], 1e-6, 1e-8)
    T = _surface_scale(c, _betas(B, Zb, False), STD_Y, np.exp(th[0]))
    err = float(np.max(np.abs(got["var"] - ref["var"].reshape((nx, nz), order="F")) / T))
    record_error("surface var vs device predict: max |diff| / T", err, 2 * SURF_TOL)
    assert err <= 2 * SURF_TOL, err
    dZ = np.asfortranarray(Zb * 0.7 + 0.1)
    got = c["m"].predict_surface(th, c["X2"], dZ, True, MEAN_Y, STD_Y, STD_Z)
    ref = c["m"].predict_marginal(th, Xg, np.asfortranarray(np.repeat(dZ, nx, axis=0)), None,
                                  STD_Y, STD_Z, False)
    close(np.ravel(got["map"], order="F"), ref["map"])
    T = _surface_scale(c, _betas(B, dZ, True), STD_Y / STD_Z, 0.0)
    err = float(np.max(np.abs(got["var"] - ref["var"].reshape((nx, nz), order="F")) / T))
    record_error("marginal surface var vs device predict_marginal: max |diff| / T", err, 2 * SURF_TOL)
    assert err <= 2 * SURF_TOL, err


def test_coef_before_para_update_raises(A):
    from additivecausalexpansion_amd.synthetic import make_problem
    y, X, Z, th, sy = make_problem(100, 2, 3, seed=1)
    m = A.DeviceModel("SE", 100, 2, 3)
    m.set_data(y, X, Z, sy)
    with pytest.raises(A.AceError, match="ARG"):
        m.coef_posterior(th, X[:5])
    with pytest.raises(A.AceError, match="ARG"):
        m.predict_surface(th, X[:5], Z[:3], False, 0.0, 1.0, 1.0)


def _fit_scale(fit, beta, scale, noise, coef):
    lam = fit["Kernel"].parameters[2:2 + beta.shape[1]]
    Pd = np.abs(np.exp(lam)[None, :] - np.einsum("cbb->cb", coef["cov"]))
    prior = (beta ** 2) @ np.exp(lam)
    return scale ** 2 * (prior[None, :] + (np.sqrt(Pd) @ np.abs(beta).T) ** 2 + noise)


def _check_response_surface(A, fit, newX, newZ, marginal):
    nx, nz = newX.shape[0], len(newZ)
    got = A.response_surface(fit, newX, newZ, marginal=marginal)
    Xg = np.tile(newX, (nz, 1))                                # expand.grid(X, Z), X fastest
    Zg = np.repeat(np.asarray(newZ, dtype=float), nx)
    ref = A.predict_ace(fit, Xg, Zg, marginal=marginal)
    assert got["map"].shape == (nx, nz)
    close(np.ravel(got["map"], order="F"), ref["map"])
    close(got["ci"].reshape((nx * nz, 2), order="F"), ref["ci"], 1e-6, 1e-8)
    # the scale T from the fit's own coefficient posterior (P_bb = e^lambda_b - cov_bb)
    mom = fit["moments"]
    px = newX.shape[1]
    zn = (np.asarray(newZ, dtype=float).reshape(-1, 1) - mom[1 + px, 0]) / mom[1 + px, 1]
    tb = fit["Basis"].testbasis(np.asfortranarray(zn))
    theta = fit["Kernel"].parameters
    B = fit["Basis"].dim()
    beta = _betas(B, np.asarray(tb["dB"] if marginal else tb["B"]), marginal)
    scale = mom[0, 1] / mom[1 + px, 1] if marginal else mom[0, 1]
    T = _fit_scale(fit, beta, scale, 0.0 if marginal else np.exp(theta[0]),
                   A.coef_posterior(fit, newX))
    err = float(np.max(np.abs(got["var"] - ref["var"].reshape((nx, nz), order="F")) / T))
    record_error("response_surface var vs predict_ace: max |diff| / T", err, 2 * SURF_TOL)
    assert err <= 2 * SURF_TOL, err


def test_response_surface_matches_predict_ace_continuous(A):
    from additivecausalexpansion_amd.synthetic import readme_data
    y, X, Z = readme_data(seed=5, n=200)
    fit = A.ace_train(y, X, Z, kernel="SE", basis="ns", n_knots=2, maxiter=8, verbose=False,
                      native_loop=True)
    rng = np.random.default_rng(7)
    newX = np.column_stack([rng.uniform(1, 2, 23), rng.uniform(-1, 1, 23)])
    newZ = np.quantile(np.ravel(Z), [0.1, 0.3, 0.5, 0.7, 0.9])
    _check_response_surface(A, fit, newX, newZ, False)
    _check_response_surface(A, fit, newX, newZ, True)
    g = A.coef_posterior(fit)
    assert g["mean"].shape == (200, fit["Basis"].dim())


def test_response_surface_matches_predict_ace_binary(A):
    from test_robust_gpu import _binary_example
    y, X, Z = _binary_example(n=200)
    fit = A.ace_train(y, X, Z, kernel="Matern32", optimizer="Nadam", learning_rate=0.001,
                      maxiter=5, verbose=False, native_loop=True)
    newX = X[:31] + 0.25
    _check_response_surface(A, fit, newX, [0.0, 1.0], False)
    _check_response_surface(A, fit, newX, [0.0, 1.0], True)
