"""GPU tests of the group-summed coefficient posterior (ace_model_coef_groups)
and the average dose-response curves contracted from it
(ace_model_average_response, train.average_coef_posterior / average_response).

The reference is the oracle alone, on the models and test points of
tests/test_coef_gpu.py: Kc = cross(X2, X, ones, Z, theta)["elements"],
k_b = sym(X2, ones, theta)["elements"], the indicator E of the labels and
  s_{g,b} = Kc_b^T E_g,  gmean = S^T inv (y - mu),  Q_inv = S^T inv S,
  Q_xx,b = E^T k_b E,  gcov = blockdiag_b(Q_xx,b) - Q_inv
with the oracle's inverse (index g + G b).

Scale.  gcov cancels the prior sums against the explained part, so an entry is
held to GROUP_TOL of
  T[(g,b),(h,b')] = delta_bb' sum_{c in g, c' in h} |k_b(x_c, x_c')|
                    + sqrt(Q_inv[(g,b),(g,b)] Q_inv[(h,b'),(h,b')]),
the Cauchy-Schwarz size of the cancelled terms; an empty group has T = 0 and
must give exact zeros.  GROUP_TOL is set at <= 5x the largest error measured
against the oracle (profiles/coef_groups_error_table.txt: 8.7e-10 of T at
n = 200, B = 17 with SE, 4.1e-10 with Matern32, 3.3e-10 at n = 300 and 6e-12
or less on the other two cases, the same to two digits for every labeling of
a case; the bound is 4.6x the largest).  COEF_TOL = 4e-9
(tests/test_coef_gpu.py, 8.7e-10 measured on the same case) and
COV_TOL = 1.5e-9 (tests/test_robust_gpu.py) are the project's bounds for the
same cancellation against the same inverse: the error is the resident
inverse's against the oracle's, not the new kernel's.

Identities against existing device calls are held to the sum of the two
calls' bounds against the oracle, each on its own scale.

G B > 2048 cannot be reached through the ABI: B <= 32 and G <= 64 give at most
2048, so the limit is tested at the boundary (G = 64, B = 32 succeeds) and
G = 65 stands for the rejection.
"""
import os

import numpy as np

from conftest import record_error, run_child
import pytest
from test_coef_gpu import CASES, COEF_TOL, KERNELS, MEAN_Y, STD_Y, STD_Z, _case, _fit_scale
from test_coef_gpu import _betas as _beta_rows
from test_gpu import close
from test_predict_gpu import _fit_state
from test_robust_gpu import COV_TOL

pytestmark = pytest.mark.gpu

GROUP_TOL = 4e-9

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELINGS = ["one", "four", "seventeen", "empty", "straddle"]


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.default_context()
    return pkg


@pytest.fixture(scope="module")
def O():
    from oracle import ace_oracle
    return ace_oracle


def _labels(name, nx):
    """(G, label) of the labelings the tests use, seeded by nx."""
    rng = np.random.default_rng(1000 + nx)
    if name == "one":
        return 1, np.zeros(nx, dtype=np.int32)
    if name == "four":                      # random, about one point in six in no group
        lab = rng.integers(0, 4, nx)
        lab[rng.random(nx) < 0.17] = -1
        return 4, lab.astype(np.int32)
    if name == "seventeen":                 # two fragments, the second with one live column
        return 17, rng.integers(0, 17, nx).astype(np.int32)
    if name == "empty":                     # group 1 of three has no point
        return 3, (2 * rng.integers(0, 2, nx)).astype(np.int32)
    if name == "straddle":                  # group 0: ten points across the tile boundary at 64
        lab = np.ones(nx, dtype=np.int32)
        lo = max(0, min(60, nx - 10))
        lab[lo:lo + 10] = 0
        return 2, lab
    raise KeyError(name)


_REF = {}


def _slice_kernels(O, c):
    """k_b on the test points (nx x nx x B), once per case."""
    if "kxx" not in c:
        nx, B = c["nx"], c["B"]
        ones = np.ones((nx, max(B - 1, 0)), order="F")
        c["kxx"] = O.KERNELS[c["kernel"]][0](c["X2"], ones, c["th"])["elements"]
    return c["kxx"]


def _reference(O, c, name):
    """The oracle's gmean, Q_xx, Q_inv, gcov and the scale T of one labeling."""
    key = (c["kernel"], c["nx"], c["B"], c["X"].shape, name)
    if key in _REF:
        return _REF[key]
    nx, B = c["nx"], c["B"]
    G, lab = _labels(name, nx)
    E = (lab[:, None] == np.arange(G)[None, :]).astype(float)           # nx x G
    kxx = _slice_kernels(O, c)
    S = np.einsum("cqb,cg->qgb", c["Kc"], E).reshape((-1, G * B), order="F")  # column g + G b
    U = c["inv"] @ S
    Qinv = S.T @ U
    gmean = (U.T @ (c["y"] - c["th"][1])).reshape((G, B), order="F")
    Qxx = np.einsum("cg,cdb,dh->gbh", E, kxx, E)
    Qabs = np.einsum("cg,cdb,dh->gbh", E, np.abs(kxx), E)
    prior = np.zeros((G, B, G, B))
    pabs = np.zeros((G, B, G, B))
    for b in range(B):
        prior[:, b, :, b] = Qxx[:, b, :]
        pabs[:, b, :, b] = Qabs[:, b, :]
    Q4 = Qinv.reshape((G, B, G, B), order="F")
    d = np.diag(Qinv).copy()
    count = E.sum(axis=0).astype(np.int64)
    live = np.repeat(count[:, None] > 0, B, axis=1).ravel(order="F")
    assert np.all(d[live] > 0)      # the inverse is positive definite whatever the theta mix
    assert np.all(d[~live] == 0)
    T = pabs + np.sqrt(np.outer(d, d)).reshape((G, B, G, B), order="F")
    r = dict(G=G, label=lab, E=E, gmean=gmean, gcov=prior - Q4, Qinv=Q4, T=T, count=count)
    _REF[key] = r
    return r


def _ratio(got, ref, T):
    """max |got - ref| / T; where T is 0 (an empty group) both must be 0."""
    zero = T == 0
    assert np.all(got[zero] == 0) and np.all(ref[zero] == 0)
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got - ref)[~zero] / T[~zero]))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,p,B,nx", CASES)
def test_coef_groups_match_oracle(A, O, kernel, n, p, B, nx):
    c = _case(A, O, kernel, n, p, B, nx)
    worst = 0.0
    for name in LABELINGS:
        r = _reference(O, c, name)
        G = r["G"]
        got = c["m"].coef_groups(c["th"], c["X2"], G, r["label"])
        assert got["gmean"].shape == (G, B) and got["gcov"].shape == (G, B, G, B)
        assert np.array_equal(got["gcount"], r["count"])
        close(got["gmean"], r["gmean"])
        err = _ratio(got["gcov"], r["gcov"], r["T"])
        print(f"{kernel} n={n} B={B} nx={nx} {name}: max |gcov - ref| / T = {err:.3e}")
        record_error(f"group cov ({name}): max |err| / T", err, GROUP_TOL)
        worst = max(worst, err)
        # exactly symmetric, and the same bits on a second call
        M = got["gcov"].reshape((G * B, G * B), order="F")
        assert np.array_equal(M, M.T)
        again = c["m"].coef_groups(c["th"], c["X2"], G, r["label"])
        for k in ("gmean", "gcov", "gcount"):
            assert np.array_equal(again[k], got[k]), (name, k)
    assert worst <= GROUP_TOL, worst


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["four", "seventeen"])
def test_group_permutation_permutes_exactly(A, O, kernel, name):
    c = _case(A, O, kernel, *CASES[0])
    G, lab = _labels(name, c["nx"])
    perm = np.random.default_rng(5).permutation(G)       # group g becomes perm[g]
    lab2 = np.where(lab >= 0, perm[np.maximum(lab, 0)], -1).astype(np.int32)
    a = c["m"].coef_groups(c["th"], c["X2"], G, lab)
    b = c["m"].coef_groups(c["th"], c["X2"], G, lab2)
    assert np.array_equal(b["gmean"][perm], a["gmean"])
    assert np.array_equal(b["gcount"][perm], a["gcount"])
    assert np.array_equal(b["gcov"][perm][:, :, perm], a["gcov"])


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,p,B,nx", [CASES[2], CASES[3]])
def test_singleton_groups_are_coef_posterior(A, O, kernel, n, p, B, nx):
    """G = nx <= 64, label[c] = c: the diagonal blocks are coef_posterior's
    cov_c and gmean its mean, each within its own bound of the oracle."""
    c = _case(A, O, kernel, n, p, B, nx)
    got = c["m"].coef_groups(c["th"], c["X2"], nx, np.arange(nx, dtype=np.int32))
    ref = c["m"].coef_posterior(c["th"], c["X2"])
    close(got["gmean"], ref["mean"])
    blocks = np.stack([got["gcov"][g, :, g, :] for g in range(nx)])
    err = float(np.max(np.abs(blocks - ref["cov"]) / c["Tc"]))
    record_error("singleton blocks vs coef_posterior: max |diff| / T_c", err, COEF_TOL + GROUP_TOL)
    assert err <= COEF_TOL + GROUP_TOL, err
    assert np.array_equal(got["gcount"], np.ones(nx, dtype=np.int64))


def _betas(B, row, marginal):
    if B == 1:
        return np.ones(1)
    return np.concatenate([[0.0 if marginal else 1.0], row])


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,p,B,nx", CASES)
def test_constant_row_gives_marginal_group_sums(A, O, kernel, n, p, B, nx):
    """One dZ2 row d for all points: sum_{b,b'>=1} d_b d_b' gcov[(g,b),(h,b')]
    is predict_marginal_groups' gcov[g,h], and std_y / std_Z sum_b d_b
    gmean[g,b] its gsum."""
    c = _case(A, O, kernel, n, p, B, nx)
    r = _reference(O, c, "four")
    G = r["G"]
    d = np.asarray(c["Z3"][0] * 0.7 + 0.1)                       # a stand-in derivative row
    beta = _betas(B, d, True)
    dZ2 = np.asfortranarray(np.repeat(d[None, :], nx, axis=0))
    got = c["m"].coef_groups(c["th"], c["X2"], G, r["label"])
    old = c["m"].predict_marginal_groups(c["th"], c["X2"], dZ2, STD_Y, STD_Z, G, r["label"])
    mine = np.einsum("b,gbhc,c->gh", beta, got["gcov"], beta)
    # the old path's scale (tests/test_robust_gpu.py): group sums of |Km_xx| + |Km_xX inv Km_xX^T|
    KmX = np.einsum("cqb,b->cq", c["Kc"], beta)
    Kmxx = np.einsum("cdb,b->cd", _slice_kernels(O, c), beta ** 2)
    Tm = r["E"].T @ (np.abs(Kmxx) + np.abs(KmX @ c["inv"] @ KmX.T)) @ r["E"]
    Tg = np.einsum("b,gbhc,c->gh", np.abs(beta), r["T"], np.abs(beta))
    ratio = _ratio(mine, old["gcov"], COV_TOL * Tm + GROUP_TOL * Tg)
    record_error("constant row vs predict_marginal_groups: max |diff| / bound", ratio, 1.0)
    assert ratio <= 1.0, ratio
    close(STD_Y / STD_Z * (got["gmean"] @ beta), old["gsum"])
    assert np.array_equal(got["gcount"], old["gcount"])


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,p,B,nx", [CASES[0], CASES[2]])
def test_block_sums_of_predict_joint(A, O, kernel, n, p, B, nx):
    """predict_joint(noise=False) at one treatment value: the block sums of its
    covariance are std_y^2 beta^T gcov beta."""
    import joint_ref as J
    c = _case(A, O, kernel, n, p, B, nx)
    r = _reference(O, c, "four")
    G = r["G"]
    z = np.asarray(c["Z3"][1])
    beta = _betas(B, z, False)
    Z2 = np.asfortranarray(np.repeat(z[None, :], nx, axis=0))
    got = c["m"].coef_groups(c["th"], c["X2"], G, r["label"])
    jt = c["m"].predict_joint(c["th"], c["X2"], Z2, MEAN_Y, STD_Y, noise=False, return_cov=True)
    mine = STD_Y ** 2 * np.einsum("b,gbhc,c->gh", beta, got["gcov"], beta)
    old = r["E"].T @ jt["cov"] @ r["E"]
    # predict_joint's scale (tests/joint_ref.py): scale^2 (|K_xx|_ij + sqrt(q_i q_j))
    KX = np.einsum("cqb,b->cq", c["Kc"], beta)
    Kxx = np.einsum("cdb,b->cd", _slice_kernels(O, c), beta ** 2)
    q = np.abs(np.sum((KX @ c["inv"]) * KX, axis=1))
    terms = STD_Y ** 2 * (np.abs(Kxx) + np.sqrt(np.outer(q, q)))
    Tg = STD_Y ** 2 * np.einsum("b,gbhc,c->gh", np.abs(beta), r["T"], np.abs(beta))
    ratio = _ratio(mine, old, J.COV_TOL * (r["E"].T @ terms @ r["E"]) + GROUP_TOL * Tg)
    record_error("block sums of predict_joint: max |diff| / bound", ratio, 1.0)
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,p,B,nx", [CASES[0], CASES[2]])
def test_average_response_is_the_contraction(A, O, kernel, n, p, B, nx):
    """ace_model_average_response against coef_groups + coef_group_contract
    (the same pass and the same host routine: bit for bit), both modes, with
    an empty group's NaN."""
    c = _case(A, O, kernel, n, p, B, nx)
    G, lab = _labels("empty", nx)
    g = c["m"].coef_groups(c["th"], c["X2"], G, lab)
    for marginal in (False, True):
        for nz in (1, 7):
            Zb = np.asfortranarray(c["Z3"][:nz])
            W = np.stack([_betas(B, Zb[j], marginal) for j in range(nz)])
            got = c["m"].average_response(c["th"], c["X2"], G, lab, Zb, marginal, MEAN_Y, STD_Y,
                                          STD_Z, return_cov=True)
            ref = (A.coef_group_contract(g["gmean"], g["gcov"], g["gcount"], W, 0.0,
                                         STD_Y / STD_Z, 0.0, return_cov=True) if marginal else
                   A.coef_group_contract(g["gmean"], g["gcov"], g["gcount"], W, MEAN_Y, STD_Y,
                                         c["th"][1], return_cov=True))
            assert got["map"].shape == (G, nz) and got["cov"].shape == (G, nz, nz)
            for k in ("map", "ci", "var", "cov"):
                assert np.array_equal(got[k], ref[k], equal_nan=True), (marginal, nz, k)
            assert np.all(np.isnan(got["map"][1])) and np.all(np.isfinite(got["map"][[0, 2]]))


_CHILD = """
import sys, numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import additivecausalexpansion_amd as A
from additivecausalexpansion_amd.synthetic import make_problem
from test_coef_groups_gpu import _labels
n, p, B, nx = 300, 3, 5, 70
y, X, Z, th0, sy = make_problem(n, p, B, seed=n)   # _fit_state's model and theta mix
m = A.DeviceModel({kernel!r}, n, p, B)
m.set_data(y, X, Z, sy)
m.para_update(2, th0.copy())
th = th0 + 0.02
th[1] = 0.13
_, X2, _, _, _ = make_problem(nx, p, B, seed=n + 1)
out = {{}}
for name in ("four", "seventeen"):
    G, lab = _labels(name, nx)
    g = m.coef_groups(th, X2, G, lab)
    out[name + "_gmean"], out[name + "_gcov"] = g["gmean"], g["gcov"]
np.savez({out!r}, **out)
"""
_CHILD_OUT = {}


def _child(tmp_path_factory, kernel, slices):
    """The child's outputs with ACE_GROUP_SLICES = slices (None: unset)."""
    key = (kernel, slices)
    if key not in _CHILD_OUT:
        out = str(tmp_path_factory.mktemp("groups") / "g.npz")
        code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), kernel=kernel, out=out)
        env = {k: v for k, v in os.environ.items() if k != "ACE_GROUP_SLICES"}
        if slices is not None:
            env["ACE_GROUP_SLICES"] = str(slices)
        run_child(code, env=env, timeout=100)
        with np.load(out) as f:
            _CHILD_OUT[key] = {k: f[k] for k in f.files}
    return _CHILD_OUT[key]


@pytest.mark.parametrize("kernel", KERNELS)
def test_slices_per_pass_do_not_change_a_bit(A, O, tmp_path_factory, kernel):
    """ACE_GROUP_SLICES = 1 (B passes of one slice) and the default (all five
    slices in one pass for G = 4; two per pass for G = 17), one fresh process
    per setting, and this process."""
    c = _case(A, O, kernel, *CASES[0])
    one = _child(tmp_path_factory, kernel, 1)
    dflt = _child(tmp_path_factory, kernel, None)
    for name in ("four", "seventeen"):
        G, lab = _labels(name, c["nx"])
        here = c["m"].coef_groups(c["th"], c["X2"], G, lab)
        for k in ("gmean", "gcov"):
            assert np.array_equal(one[f"{name}_{k}"], dflt[f"{name}_{k}"]), (name, k)
            assert np.array_equal(here[k], dflt[f"{name}_{k}"]), (name, k)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_agrees_with_single(A, O, kernel, world):
    n, p, B, nx = CASES[0]
    c = _case(A, O, kernel, n, p, B, nx)
    sh, *_ = _fit_state(O, kernel, n, p, B, seed=n, sharded=True, world=world, A=A)
    for name in ("four", "seventeen"):
        r = _reference(O, c, name)
        here = c["m"].coef_groups(c["th"], c["X2"], r["G"], r["label"])
        got = sh.coef_groups(c["th"], c["X2"], r["G"], r["label"])
        close(got["gmean"], here["gmean"])
        M = got["gcov"].reshape((r["G"] * B,) * 2, order="F")
        assert np.array_equal(M, M.T)
        err = _ratio(got["gcov"], here["gcov"], r["T"])
        record_error(f"group cov ({name}), sharded vs single: max |diff| / T", err, GROUP_TOL)
        assert err <= GROUP_TOL, err
        err = _ratio(got["gcov"], r["gcov"], r["T"])
        record_error(f"group cov ({name}, sharded): max |err| / T", err, GROUP_TOL)
        assert err <= GROUP_TOL, err


def test_error_paths_leave_the_model_usable(A):
    from additivecausalexpansion_amd.synthetic import make_problem
    n, p, B, nx = 100, 2, 3, 20
    y, X, Z, th, sy = make_problem(n, p, B, seed=1)
    m = A.DeviceModel("SE", n, p, B)
    m.set_data(y, X, Z, sy)
    lab = (np.arange(nx) % 2).astype(np.int32)
    with pytest.raises(A.AceError, match="ARG"):            # before the first para_update
        m.coef_groups(th, X[:nx], 2, lab)
    with pytest.raises(A.AceError, match="ARG"):
        m.average_response(th, X[:nx], 2, lab, Z[:3], False, 0.0, 1.0, 1.0)
    m.para_update(1, th.copy())
    good = m.coef_groups(th, X[:nx], 2, lab)
    for G, bad in ((0, lab), (65, lab), (2, np.where(np.arange(nx) == 7, 2, lab).astype(np.int32)),
                   (2, np.where(np.arange(nx) == 3, -2, lab).astype(np.int32))):
        with pytest.raises(A.AceError, match="ARG"):
            m.coef_groups(th, X[:nx], G, bad)
        with pytest.raises(A.AceError, match="ARG"):
            m.average_response(th, X[:nx], G, bad, Z[:3], True, 0.0, 1.0, 1.0)
        again = m.coef_groups(th, X[:nx], 2, lab)            # a following valid call succeeds
        assert np.array_equal(again["gcov"], good["gcov"])
    with pytest.raises(A.AceError):                          # one label per point
        m.coef_groups(th, X[:nx], 2, lab[:-1])


def test_largest_group_basis_product_runs(A):
    """G = 64 and B = 32: G B = 2048, the limit, with every fragment live."""
    from additivecausalexpansion_amd.synthetic import make_problem
    n, p, B, nx = 100, 1, 32, 130
    y, X, Z, th, sy = make_problem(n, p, B, seed=3)
    m = A.DeviceModel("Matern32", n, p, B)
    m.set_data(y, X, Z, sy)
    m.para_update(1, th.copy())
    _, X2, _, _, _ = make_problem(nx, p, B, seed=4)
    lab = (np.arange(nx) % 64).astype(np.int32)
    g = m.coef_groups(th, X2, 64, lab)
    assert g["gcov"].shape == (64, 32, 64, 32) and np.all(np.isfinite(g["gcov"]))
    assert np.array_equal(g["gcount"], np.bincount(lab, minlength=64))
    # against the pointwise posterior: a group's sums over its own points
    ref = m.coef_posterior(th, X2)
    close(g["gmean"], np.stack([ref["mean"][lab == h].sum(axis=0) for h in range(64)]))


def _device_average_treatments(A, O, kernel):
    """mix=False (theta_T = theta_{T-1}): every posterior form is nonnegative."""
    n, p, B, nx = 400, 3, 2, 150
    m, y, X, Z, th, sy, inv = _fit_state(O, kernel, n, p, B, seed=7, A=A, mix=False)
    from additivecausalexpansion_amd.synthetic import make_problem
    _, X2, _, _, _ = make_problem(nx, p, B, seed=77)
    return m, th, X2, nx


@pytest.mark.parametrize("kernel", KERNELS)
def test_binary_special_case_is_ate_att_atu(A, O, kernel):
    """B = 2, beta' = (0, d): the groups of a 0 / 1 treatment column give
    predict_marginal's ATT and ATU, one group of all its ATE.  std_Z = 1, as
    a binary treatment has it (it is not rescaled): pred_marginal_cpp's
    averages take their sd as std_y sqrt(post) / n without std_Z
    (src/pred_cpp.cpp:89-126), the average curves scale by std_y / std_Z
    throughout."""
    m, th, X2, nx = _device_average_treatments(A, O, kernel)
    zx = (np.arange(nx) % 3 == 0).astype(float)
    d = 0.7
    dZ2 = np.full((nx, 1), d, order="F")
    old = m.predict_marginal(th, X2, dZ2, zx, STD_Y, 1.0, True)
    two = m.average_response(th, X2, 2, zx.astype(np.int32), np.array([[d]]), True, MEAN_Y, STD_Y,
                             1.0)
    one = m.average_response(th, X2, 1, np.zeros(nx, dtype=np.int32), np.array([[d]]), True,
                             MEAN_Y, STD_Y, 1.0)
    # the forms' scale from the call's own sums: |prior| + explained per group
    g = m.coef_groups(th, X2, 2, zx.astype(np.int32))
    for key, r, gi in (("ate", one, 0), ("att", two, 1), ("atu", two, 0)):
        o = old[key]
        assert np.isfinite(o["var"]) and o["var"] >= 0
        close(r["map"][gi, 0], o["map"], 1e-6, 0.0)
        # the scale of an average's variance: |k_1| <= e^lambda_1 bounds the
        # prior sum over |g|^2 pairs by |g|^2 e^lambda_1, and with
        # theta_T = theta_{T-1} the explained part is no larger than the prior
        T = STD_Y ** 2 * d * d * 2 * np.exp(th[3])
        err = abs(r["var"][gi, 0] - o["var"]) / T
        record_error(f"binary {key} var vs predict_marginal: |diff| / T", err, COV_TOL + GROUP_TOL)
        assert err <= COV_TOL + GROUP_TOL, (key, err)
        tol = 1e-6 * abs(o["map"]) + 1.96 * (COV_TOL + GROUP_TOL) * T / np.sqrt(o["var"])
        assert np.all(np.abs(r["ci"][gi, 0] - o["ci"]) <= tol), key
    assert g["gcount"][1] == zx.sum()


def test_python_average_response_binary(A):
    """train.average_response(marginal=True) with groups = Z on a binary fit:
    predict_ace's ATT / ATU, and its ATE with one group."""
    from test_robust_gpu import _binary_example
    y, X, Z = _binary_example(n=200)
    # learning rate 0.001: theta_T stays close enough to the resident
    # inverse's theta_{T-1} (Q6) that the forms are positive
    # (tests/test_robust_gpu.py test_python_robust_treatment_matches_predict_loop)
    fit = A.ace_train(y, X, Z, kernel="SE", optimizer="Nadam", learning_rate=0.001, maxiter=5,
                      verbose=False, native_loop=True)
    old = A.predict_ace(fit, marginal=True, return_average_treatments=True)
    zt = np.ravel(fit["train_data"]["Z"])
    two = A.average_response(fit, [1.0], groups=zt, marginal=True)
    one = A.average_response(fit, [1.0], marginal=True)
    assert list(two["groups"]) == [0.0, 1.0] and list(two["count"]) == [int((zt == 0).sum()),
                                                                       int((zt == 1).sum())]
    assert one["map"].shape == (1, 1) and two["ci"].shape == (2, 1, 2)
    K = fit["Kernel"]
    mom = fit["moments"]
    Xtr = fit["train_data"]["X"]
    tb = fit["Basis"].testbasis(fit["train_data"]["Z"])
    KmX = A.kernmat_SE_cpp(Xtr, Xtr, tb["dB"], fit["Basis"].B, K.parameters)["elements"][:, :, 1:].sum(axis=2)
    Kxx = A.kernmat_SE_symmetric_cpp(Xtr, tb["dB"], K.parameters)["elements"][:, :, 1:].sum(axis=2)
    Tm = np.abs(Kxx) + np.abs(KmX @ K._model.inverse() @ KmX.T)
    # pred_marginal_cpp's averages take their sd without std_Z (1 for a binary
    # treatment that is not rescaled; src/pred_cpp.cpp:89-126)
    sy, sz = float(mom[0, 1]), float(mom[3, 1])
    for key, r, gi, sel in (("ate", one, 0, np.ones(zt.size, bool)), ("att", two, 1, zt == 1),
                            ("atu", two, 0, zt == 0)):
        o = old[key]
        assert np.isfinite(o["var"]), key
        close(r["map"][gi, 0], o["map"], 1e-6, 0.0)
        e = sy ** 2 / sel.sum() ** 2 * (COV_TOL + GROUP_TOL) * Tm[np.ix_(sel, sel)].sum()
        v = r["var"][gi, 0] * sz ** 2
        assert abs(v - o["var"]) <= e, (key, v, o["var"], e)
    avg = A.average_coef_posterior(fit, groups=zt)
    assert avg["mean"].shape == (2, 2) and avg["cov"].shape == (2, 2, 2, 2)
    assert list(avg["count"]) == list(two["count"])


def test_python_average_response_continuous(A):
    """Every point its own group: average_response is response_surface; and
    the average curve of a group is the mean of its points' curves."""
    from additivecausalexpansion_amd.synthetic import readme_data
    y, X, Z = readme_data(seed=5, n=200)
    fit = A.ace_train(y, X, Z, kernel="SE", basis="ns", n_knots=2, maxiter=8, verbose=False,
                      native_loop=True)
    rng = np.random.default_rng(7)
    nx = 23
    newX = np.column_stack([rng.uniform(1, 2, nx), rng.uniform(-1, 1, nx)])
    newZ = np.quantile(np.ravel(Z), [0.1, 0.3, 0.5, 0.7, 0.9])
    for marginal in (True, False):
        surf = A.response_surface(fit, newX, newZ, marginal=marginal)
        got = A.average_response(fit, newZ, newX=newX, groups=np.arange(nx), marginal=marginal,
                                 return_cov=True)
        assert got["map"].shape == (nx, 5) and got["cov"].shape == (nx, 5, 5)
        close(got["map"], surf["map"])
        if marginal:                         # response_surface adds the noise term otherwise
            # both contract B x B blocks that are each within their bound of
            # the oracle's, on the surface scale of tests/test_coef_gpu.py
            mom = fit["moments"]
            zn = (newZ.reshape(-1, 1) - mom[3, 0]) / mom[3, 1]
            tb = fit["Basis"].testbasis(np.asfortranarray(zn))
            beta = _beta_rows(fit["Basis"].dim(), np.asarray(tb["dB"]), True)
            T = _fit_scale(fit, beta, mom[0, 1] / mom[3, 1], 0.0, A.coef_posterior(fit, newX))
            err = float(np.max(np.abs(got["var"] - surf["var"]) / T))
            record_error("average_response (singletons) var vs response_surface: max |diff| / T",
                         err, COEF_TOL + GROUP_TOL)
            assert err <= COEF_TOL + GROUP_TOL, err
    half = (np.arange(nx) % 2).astype(int)
    grp = A.average_response(fit, newZ, newX=newX, groups=half)
    surf = A.response_surface(fit, newX, newZ)
    close(grp["map"], np.stack([surf["map"][half == h].mean(axis=0) for h in (0, 1)]))
    assert list(grp["count"]) == [12, 11]
    insample = A.average_response(fit, newZ)
    assert insample["map"].shape == (1, 5) and insample["count"][0] == 200
