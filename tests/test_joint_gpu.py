"""GPU tests of the joint posterior at the test points
(ace_model_predict_joint, ace_potrf_lower, posterior_draws): covariance,
Cholesky factor and draws against the numpy referee (tests/joint_ref.py),
whose diagonal tests/test_joint_cpu.py ties to the oracle's pred_cpp /
pred_marginal_cpp.

Every device state is produced once, by a child process (run_child) that
saves what the calls returned; the tests of a state assert on that file.

Bounds.  cov: COV_TOL of the Cauchy-Schwarz size of the cancelled terms,
scale^2 (|K_xx|_ij + sqrt(q_i q_j) [+ e^sigma on i = j]); measured 5.2e-10 at
most over all states (profiles/joint_error_table.txt), bound 1.5e-9 = 2.9x.
Factor: |L L^T - (cov + jitter I)|_ij <= FACTOR_MARGIN gamma_{nx+1}
sqrt(c'_ii c'_jj) (Higham's bound for a substitution-based Cholesky), the
product in long double from the device's own L and cov; measured 0.23 at
most, margin 1.  Draws: the rounding of one dot product of length nx and
one addition (measured 0.87 of it; the results are bitwise reproducible).
"""
import os

import numpy as np
import pytest

import joint_ref as J
from conftest import ROOT, record_error, run_child
from test_gpu import close
from test_predict_gpu import CI_TOL, VAR_TOL

pytestmark = pytest.mark.gpu

KERNELS = ["SE", "Matern32"]
CASES = list(J.CASES)
S_SEEDED = 33

_PRE = f"""
import sys
sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]
import numpy as np
import additivecausalexpansion_amd as A
import joint_ref as J


def model(s, kernel, **kw):
    m = A.DeviceModel(kernel, s["n"], s["p"], s["B"], **kw)
    m.set_data(s["y"], s["X"], s["Z"], s["sy"])
    m.para_update(2, s["th_prev"].copy())   # resident inverse at theta_(T-1)
    return m


def joint(m, s, marg, **kw):
    return m.predict_joint(s["th"], s["X2"], s["dZ2"] if marg else s["Z2"], J.MEAN_Y, J.STD_Y,
                           marginal=marg, std_Z=J.STD_Z, **kw)
"""

_STATE = _PRE + """
kernel, case, out = {kernel!r}, {case!r}, {out!r}
s = J.problem(case, kernel)
m = model(s, kernel)
nx = s["nx"]
xi = np.random.default_rng(7).standard_normal((nx, {S}))
res = {{}}
for marg in (False, True):
    k = "m_" if marg else "p_"
    jit = J.jitter_of(kernel, marg)
    a = joint(m, s, marg, jitter=jit, xi=xi, return_cov=True, return_factor=True)
    b = joint(m, s, marg, jitter=jit, xi=xi, return_cov=True, return_factor=True)
    e = joint(m, s, marg, jitter=jit, xi=np.eye(nx), return_factor=True)
    # S = 0, xi = None and NULL outputs
    n0 = joint(m, s, marg, jitter=jit)
    n1 = joint(m, s, marg, jitter=jit, xi=np.empty((nx, 0)), return_cov=True)
    assert set(n0) == {{"map", "info"}} and n1["draws"].shape == (nx, 0)
    assert n0["info"] == 0 and n1["info"] == 0
    assert np.array_equal(n0["map"], a["map"]) and np.array_equal(n1["cov"], a["cov"])
    if marg:
        pv = m.predict_marginal(s["th"], s["X2"], s["dZ2"], None, J.STD_Y, J.STD_Z, False)
    else:
        pv = m.predict(s["th"], s["X2"], s["Z2"], J.MEAN_Y, J.STD_Y)
    for name in ("map", "cov", "L", "draws"):
        res[k + name] = a[name]
        res[k + name + "_same"] = np.array(np.array_equal(a[name], b[name]))
    res[k + "info"] = np.array([a["info"], b["info"], e["info"]])
    res[k + "L_eye"], res[k + "draws_eye"] = e["L"], e["draws"]
    res[k + "pmap"], res[k + "pvar"] = pv["map"], pv["var"]
res["xi"] = xi
np.savez(out, **res)
"""


@pytest.fixture(scope="module")
def device_state(tmp_path_factory):
    cache = {}

    def get(kernel, case):
        if (kernel, case) not in cache:
            out = str(tmp_path_factory.mktemp("joint") / "state.npz")
            run_child(_STATE.format(kernel=kernel, case=case, out=out, S=S_SEEDED), timeout=100)
            with np.load(out) as f:
                cache[(kernel, case)] = {k: f[k] for k in f.files}
        return cache[(kernel, case)]
    return get


def _check_cov(got, ref, label):
    err = np.abs(got - ref["cov"]) / ref["terms"]
    print(f"{label}: max |cov - ref| / terms = {err.max():.3e} (COV_TOL {J.COV_TOL:g})")
    record_error("joint cov: max |err| / terms", err.max(), J.COV_TOL)
    assert np.all(err <= J.COV_TOL)


# ------------------------------------------------------------------ 1. covariance
@pytest.mark.parametrize("marginal", [False, True])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_covariance_matches_oracle(device_state, kernel, case, marginal):
    d = device_state(kernel, case)
    ref = J.joint(case, kernel, marginal)
    k = "m_" if marginal else "p_"
    cov = d[k + "cov"]
    _check_cov(cov, ref, f"{kernel} {case} marginal={marginal}")
    assert np.array_equal(cov, cov.T)  # bitwise
    # the diagonal against predict / predict_marginal's var, the map against theirs
    dterms = np.diag(ref["terms"])
    derr = np.abs(np.diag(cov) - d[k + "pvar"]) / dterms
    record_error("joint diag(cov) vs predict var: max |err| / terms", derr.max(), VAR_TOL)
    assert np.all(derr <= VAR_TOL)
    close(d[k + "map"], d[k + "pmap"], check="joint map vs predict map")
    close(d[k + "map"], ref["map"], check="joint map vs oracle")


# ------------------------------------------------------------------ 2. factor
@pytest.mark.parametrize("marginal", [False, True])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_factor_through_the_model(device_state, kernel, case, marginal):
    d = device_state(kernel, case)
    k = "m_" if marginal else "p_"
    L, cov = d[k + "L"], d[k + "cov"]
    assert np.all(d[k + "info"] == 0)
    assert np.all(np.triu(L, 1) == 0.0)
    assert np.all(np.diag(L) > 0)
    jit = J.jitter_of(kernel, marginal)
    ratio = J.factor_residual_ratio(L, cov + jit * np.eye(L.shape[0]))
    print(f"{kernel} {case} marginal={marginal}: factor residual / gamma bound = {ratio:.3e}")
    record_error("joint factor: max |L L^T - C'| / (gamma_{nx+1} sqrt(c_ii c_jj))", ratio,
                 J.FACTOR_MARGIN)
    assert ratio <= J.FACTOR_MARGIN


# ------------------------------------------------------------------ 3. draws
@pytest.mark.parametrize("marginal", [False, True])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_draws(device_state, kernel, case, marginal):
    d = device_state(kernel, case)
    k = "m_" if marginal else "p_"
    mp, L, xi = d[k + "map"], d[k + "L"], d["xi"]
    nx = mp.size
    # Xi = I: column j is map + L[:, j], one rounding
    Le = d[k + "L_eye"]
    assert np.array_equal(Le, L)
    err = np.abs((d[k + "draws_eye"] - mp[:, None]) - Le)
    assert np.all(err <= 2 * np.spacing(np.abs(mp)[:, None] + np.abs(Le)))
    # a seeded normal Xi against numpy's product, taken in long double
    ref = mp[:, None] + L.astype(np.longdouble) @ xi.astype(np.longdouble)
    bound = J.gamma(nx) * (np.abs(L) @ np.abs(xi)) + J.U * np.abs(mp)[:, None]
    derr = np.abs(d[k + "draws"] - ref).astype(float)
    record_error("joint draws: max |err| / (gamma_nx |L||Xi| + u |map|)", np.max(derr / bound), 1.0)
    assert np.all(derr <= bound)
    # two identical calls: bitwise equal
    for name in ("map", "cov", "L", "draws"):
        assert bool(d[k + name + "_same"]), name


# ------------------------------------------------------------------ 4. averages
_AVG = _PRE + """
from additivecausalexpansion_amd.synthetic import readme_data
y, X, Z = readme_data(n=300)
Zb = (Z > np.median(Z)).astype(float)
# learning rate 0.001: the five steps leave theta_T close enough to the
# resident inverse's theta_(T-1) (Q6) for the marginal covariance to be used
fit = A.ace_train(y, X, Zb, kernel={kernel!r}, optimizer="Nadam", learning_rate=0.001, maxiter=5,
                  verbose=False, native_loop=True)
pa = A.predict_ace(fit, marginal=True, return_average_treatments=True)
K, mom = fit["Kernel"], fit["moments"]
tb = fit["Basis"].testbasis(fit["train_data"]["Z"])
c = K.predict_joint(fit["train_data"]["y"], fit["train_data"]["X"], fit["Basis"].B,
                    fit["train_data"]["X"], tb["dB"], mom[0, 0], mom[0, 1], marginal=True,
                    std_Z=mom[3:4, 1], return_cov=True)["cov"]
lmin = float(np.linalg.eigvalsh(c)[0])
print("lambda_min", lmin, "mean diag", float(np.mean(np.diag(c))))
jitter = {jitter}
r = A.posterior_draws(fit, marginal=True, n_draws=40, seed=3, jitter=jitter,
                      return_average_treatments=True, return_cov=True)
assert np.array_equal(r["cov"], c)
# Q6, far from the inverse's theta: strongly indefinite, and the error says so
bad = dict(fit)
Kb = type(K).__new__(type(K))
Kb.__dict__.update(K.__dict__)
Kb.parameters = K.parameters + 0.02
bad["Kernel"] = Kb
msg = ""
try:
    A.posterior_draws(bad, n_draws=2)
except A.AceError as e:
    msg = str(e)
np.savez({out!r}, draws=r["draws"], map=r["map"], cov=r["cov"], ate=r["ate"], att=r["att"],
         atu=r["atu"], zx=np.ravel(tb["B"]), lmin=lmin, msg=np.array(msg),
         **{{"pa_" + k + "_" + f: np.asarray(pa[k][f]) for k in ("ate", "att", "atu")
            for f in ("map", "var")}})
"""


@pytest.mark.parametrize("kernel", KERNELS)
def test_average_treatment_draws(tmp_path, kernel):
    """ate / att / atu of posterior_draws are the weighted column means of the
    draws, and the ATE's variance w^T cov w / nx^2 is predict_ace's.  Matern32
    runs with the default jitter.  SE passes an explicit one: under Q6
    (inverse at theta_{T-1}, kernels at theta_T) this fit's SE marginal
    covariance, mean diagonal 19.4, has lambda_min = -3.9e-9 (the child
    prints it) -- inside the rounding of C itself, COV_TOL terms ~ 1e-7, and
    below the default 1e-10 mean(diag) = 1.9e-9.  1e-6 is 10x that rounding."""
    out = str(tmp_path / "avg.npz")
    jitter = "1e-6" if kernel == "SE" else "None"
    r = run_child(_AVG.format(kernel=kernel, out=out, jitter=jitter), timeout=100)
    print(r.stdout[-300:])
    with np.load(out) as f:
        d = {k: f[k] for k in f.files}
    D, zx = d["draws"], d["zx"]
    nx = D.shape[0]
    assert set(np.unique(zx)) == {0.0, 1.0}
    for key, w in (("ate", np.ones(nx)), ("att", zx), ("atu", (zx == 0).astype(float))):
        ref = (w @ D) / w.sum()
        tol = 1e-13 * (np.abs(w) @ np.abs(D))
        assert np.all(np.abs(d[key] - ref) <= tol), key
        assert d[key].shape == (D.shape[1],)
    v = np.ones(nx) @ d["cov"] @ np.ones(nx) / nx ** 2
    sd = np.sqrt(abs(float(d["pa_ate_var"])))
    # predict_ace's interval half-width 1.96 sd against the covariance's
    assert abs(1.96 * np.sqrt(abs(v)) - 1.96 * sd) <= CI_TOL * (abs(float(d["pa_ate_map"])) + 1.96 * sd)
    assert "jitter" in str(d["msg"]) and "pivot" in str(d["msg"])


# ------------------------------------------------------------------ 5. failure path
_FAIL = _PRE + """
kernel, out = {kernel!r}, {out!r}
bad = J.problem("300/70", kernel, True)     # kernels at theta + 0.02 (Q6)
good = J.problem("300/70", kernel, False)
m = model(bad, kernel)
nx = bad["nx"]
xi = np.random.default_rng(1).standard_normal((nx, 5))
res = {{}}
for marg in (False, True):
    k = "m_" if marg else "p_"
    f = joint(m, bad, marg, xi=xi, return_cov=True, return_factor=True)
    g = joint(m, good, marg, jitter=J.jitter_of(kernel, marg), xi=xi, return_factor=True)
    res[k + "info"] = np.array([f["info"], g["info"]])
    for name in ("map", "cov", "L", "draws"):
        res[k + name] = f[name]
    res[k + "gL"], res[k + "gdraws"] = g["L"], g["draws"]
np.savez(out, **res)
"""


@pytest.mark.parametrize("kernel", KERNELS)
def test_failure_path_is_deterministic_and_does_not_leak(tmp_path, kernel):
    out = str(tmp_path / "fail.npz")
    run_child(_FAIL.format(kernel=kernel, out=out), timeout=100)
    with np.load(out) as f:
        d = {k: f[k] for k in f.files}
    for marginal in (False, True):
        k = "m_" if marginal else "p_"
        ref = J.joint("300/70", kernel, marginal, mix=True)
        nx = ref["map"].size
        bad_info, good_info = d[k + "info"]
        assert 1 <= bad_info <= nx
        close(d[k + "map"], ref["map"], check="joint map vs oracle (Q6 mix)")
        _check_cov(d[k + "cov"], ref, f"{kernel} 300/70 mix marginal={marginal}")
        assert np.all(np.isnan(d[k + "L"])) and np.all(np.isnan(d[k + "draws"]))
        # the next call on the same model: the flag does not leak
        assert good_info == 0
        assert np.all(np.isfinite(d[k + "gL"])) and np.all(np.isfinite(d[k + "gdraws"]))


# ------------------------------------------------------------------ 6. the factor alone
_POTRF = _PRE + """
res = {{}}
rng = np.random.default_rng(11)
for n in (1, 63, 64, 65, 129, 200, 1000):
    G = rng.standard_normal((n, n))
    M = G @ G.T + np.eye(n)
    L, info = A.potrf_lower(M)
    res[f"spd_{{n}}_A"], res[f"spd_{{n}}_L"], res[f"spd_{{n}}_info"] = M, L, np.array(info)
for n in (65, 200):
    for at in (0, 63, 64, n - 1):
        dg = np.ones(n)
        dg[at] = -1.0
        L, info = A.potrf_lower(np.diag(dg))
        res[f"neg_{{n}}_{{at}}"] = np.array([info, int(np.all(np.isnan(L)))])
n = 130
G = rng.standard_normal((n, n))
M = G @ G.T + np.eye(n)
for (i, j) in ((0, 0), (70, 3), (129, 64), (100, 100)):
    Mn = M.copy()
    Mn[i, j] = np.nan
    res[f"nan_{{i}}_{{j}}"] = np.array(A.potrf_lower(Mn)[1])
Mu = M.copy()
Mu[3, 70] = np.nan                      # above the diagonal: never read
res["nan_upper"] = np.array(A.potrf_lower(Mu)[1])
# lda > n: rows n.. of the buffer are not the matrix
buf = np.full((n + 7, n), np.nan, order="F")
buf[:n] = M
res["lda_L"], res["lda_info"] = (lambda r: (r[0], np.array(r[1])))(A.potrf_lower(buf, lda=n + 7))
res["lda_ref"] = A.potrf_lower(M)[0]
L, info = A.potrf_lower(M, jitter=0.5)
res["jit_A"], res["jit_L"] = M + 0.5 * np.eye(n), L
np.savez({out!r}, **res)
"""


@pytest.fixture(scope="module")
def potrf_state(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("potrf") / "potrf.npz")
    run_child(_POTRF.format(out=out), timeout=100)
    with np.load(out) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 200, 1000])
def test_potrf_lower_spd(potrf_state, n):
    A_, L = potrf_state[f"spd_{n}_A"], potrf_state[f"spd_{n}_L"]
    assert int(potrf_state[f"spd_{n}_info"]) == 0
    assert np.all(np.triu(L, 1) == 0.0) and np.all(np.diag(L) > 0)
    ratio = J.factor_residual_ratio(L, A_)
    record_error("potrf_lower: max |L L^T - A| / (gamma_{n+1} sqrt(a_ii a_jj))", ratio,
                 J.FACTOR_MARGIN)
    assert ratio <= J.FACTOR_MARGIN


def test_potrf_lower_failures_and_layout(potrf_state):
    d = potrf_state
    for n in (65, 200):
        for at in (0, 63, 64, n - 1):
            info, allnan = d[f"neg_{n}_{at}"]
            assert info == at + 1 and allnan == 1, (n, at, info)
    # a NaN at (i, j), i >= j, first reaches a pivot at row i
    for (i, j) in ((0, 0), (70, 3), (129, 64), (100, 100)):
        assert int(d[f"nan_{i}_{j}"]) == i + 1, (i, j)
    assert int(d["nan_upper"]) == 0
    assert int(d["lda_info"]) == 0 and np.array_equal(d["lda_L"], d["lda_ref"])
    assert J.factor_residual_ratio(d["jit_L"], d["jit_A"]) <= J.FACTOR_MARGIN


# ------------------------------------------------------------------ 7. refusals
_REFUSE = _PRE + """
s = J.problem("130/9", "SE")
msgs = {{}}


def attempt(name, f):
    try:
        f()
        msgs[name] = "no error"
    except A.AceError as e:
        msgs[name] = str(e)


s2 = J.problem("300/70", "SE")
sh = model(s2, "SE", world=2, sharded=True)
attempt("sharded", lambda: joint(sh, s2, False))
m = model(s, "SE")
big = 8193
attempt("nx", lambda: m.predict_joint(s["th"], np.zeros((big, s["p"])), np.zeros((big, 0)),
                                      0.0, 1.0))
attempt("S", lambda: joint(m, s, False, xi=np.zeros((s["nx"], 4097))))
attempt("jitter", lambda: joint(m, s, False, jitter=-1e-12))
attempt("jitter_nan", lambda: joint(m, s, False, jitter=float("nan")))
fresh = A.DeviceModel("SE", s["n"], s["p"], s["B"])
fresh.set_data(s["y"], s["X"], s["Z"], s["sy"])
attempt("no_inverse", lambda: joint(fresh, s, False))
attempt("ok", lambda: joint(m, s, False))
import json
open({out!r}, "w").write(json.dumps(msgs))
"""


def test_refusals(tmp_path):
    import json
    out = str(tmp_path / "refuse.json")
    run_child(_REFUSE.format(out=out), timeout=100)
    msgs = json.load(open(out))
    assert msgs["ok"] == "no error"
    for k in ("sharded", "nx", "S"):
        assert msgs[k].startswith("ACE_ERR_UNSUPPORTED"), (k, msgs[k])
    for k in ("jitter", "jitter_nan", "no_inverse"):
        assert msgs[k].startswith("ACE_ERR_ARG"), (k, msgs[k])
    assert "para_update" in msgs["no_inverse"]
