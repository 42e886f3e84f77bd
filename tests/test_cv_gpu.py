"""GPU tests of cross-validation from the resident inverse (ace_model_cv,
ace_cv_from_inverse, cross_validate) against the numpy referee
(tests/cv_ref.py), which conditions explicitly on the remaining rows and never
uses the inverse identity; tests/test_cv_cpu.py ties the two together and
shows every fold's block SPD, so a status != 0 here is a defect.

Every device state is produced once, by a child process (run_child) that
saves what the calls returned; the tests of a state assert on that file.

Bounds.  Every array is held with close() at the project's RTOL = 1e-6, and
its error max |got - ref| / max |ref| with the file's own CV_TOL_*: at most 5x
the largest value measured on an MI355X over all cases, kernels, fold sets and
both dispatches (profiles/cv_error_table.txt):
    measured  map 9.1e-13, var 2.6e-12, resid 3.0e-12, lpd 2.4e-12, mahal 3.5e-12
              (all at SE 300/70, where the referee's own solves differ from the
              identity in numpy by 1.0e-12: tests/test_cv_cpu.py)
    CV_TOL    map 4.5e-12, var 1.3e-11, resid 1.5e-11, lpd 1.2e-11, mahal 1.7e-11;
the host-buffer entry point against numpy on a well-conditioned random SPD
matrix: 1.7e-15 measured, CV_TOL_HOST 8.5e-15.
"""
import os

import numpy as np
import pytest

import cv_ref as C
import joint_ref as J
import zskip_cases as ZC
from conftest import ROOT, record_error, run_child
from test_gpu import close

pytestmark = pytest.mark.gpu

KERNELS = ["SE", "Matern32"]
KEYS = ("map", "var", "resid", "lpd", "mahal")
CV_TOL = {"map": 4.5e-12, "var": 1.3e-11, "resid": 1.5e-11, "lpd": 1.2e-11, "mahal": 1.7e-11}
CV_TOL_HOST = 8.5e-15
N_OTHERS = 40
PERM_CASES = ["SE-p3-spline-n200", "Matern32-p20-scattered-n200"]


def hold(got, ref, key, label, tol=None):
    """close() at RTOL, then the measured error against the file's own bound."""
    tol = CV_TOL[key] if tol is None else tol
    close(got, ref, check=f"cv {key}")
    err = float(np.abs(np.asarray(got) - ref).max() / np.abs(ref).max())
    print(f"{label} {key}: max |err| / max |ref| = {err:.3e} (bound {tol:g})")
    record_error(f"cv {key}: max |err| / max |ref|", err, tol)
    assert err <= tol, (label, key, err)


_PRE = f"""
import os, sys
sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]
import numpy as np
import additivecausalexpansion_amd as A
import cv_ref as C
import joint_ref as J
KEYS = ("map", "var", "resid", "lpd", "mahal", "status")


def put(res, tag, r):
    for k in KEYS:
        res[tag + "/" + k] = r[k]


def same(a, b):
    return np.array(all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS))


def one(r, f):
    # fold f's part of a result, as a dict
    o = r["off"]
    out = dict((k, r[k][o[f]:o[f + 1]]) for k in ("map", "var", "resid"))
    out.update((k, r[k][f:f + 1]) for k in ("lpd", "mahal", "status"))
    return out
"""

_STATE = _PRE + """
kernel, case, out = {kernel!r}, {case!r}, {out!r}
s = J.problem(case, kernel)
n = s["n"]
m = A.DeviceModel(kernel, n, s["p"], s["B"])
m.set_data(s["y"], s["X"], s["Z"], s["sy"])
m.para_update(2, s["th_prev"].copy())   # resident inverse at theta_(T-1)
cv = lambda folds: m.cv(s["th"], folds, C.MEAN_Y, C.STD_Y)
sets = C.fold_sets(n)
res = {{}}
for name in C.sets_of(case):
    a = cv(sets[name])
    put(res, name, a)
    res[name + "/again"] = same(a, cv(sets[name]))
    os.environ["ACE_CV_WG_MAX"] = "16"   # read per call: folds above 16 take the sweep
    b = cv(sets[name])
    del os.environ["ACE_CV_WG_MAX"]
    put(res, name + "/sweep", b)
    os.environ["ACE_CV_WG_MAX"] = "16"
    res[name + "/sweep/again"] = same(b, cv(sets[name]))
    del os.environ["ACE_CV_WG_MAX"]
# leave-one-out as a list next to one fold of two rows: the workgroup kernel
lst = cv(sets["loo"] + [np.array([0, 1])])
for k in ("map", "var", "resid"):
    res["loolist/" + k] = lst[k][:n]
for k in ("lpd", "mahal", "status"):
    res["loolist/" + k] = lst[k][:n]
# one fold alone, first and last among {others} others, reversed, shuffled
rng = np.random.default_rng(5)
F = sets["descending"][0]
others = [rng.permutation(n)[:int(rng.integers(2, 60))] for _ in range({others})]
alone = one(cv([F]), 0)
res["indep/first"] = same(alone, one(cv([F] + others), 0))
res["indep/last"] = same(alone, one(cv(others + [F]), {others}))
rev = one(cv([F[::-1].copy()]), 0)
for k in ("map", "var", "resid"):
    rev[k] = rev[k][::-1]
res["indep/reversed"] = same(alone, rev)
sh = rng.permutation(F.size)
shf = one(cv([F[sh]]), 0)
back = np.argsort(sh)
for k in ("map", "var", "resid"):
    shf[k] = shf[k][back]
res["indep/shuffled"] = same(alone, shf)
# NULL outputs are accepted
from additivecausalexpansion_amd._lib import check, lib, ptr
from additivecausalexpansion_amd.native import iptr, pack_folds
nf, off, idx = pack_folds(sets["mixed"])
th = np.ascontiguousarray(s["th"])
check(lib().ace_model_cv(m.handle, ptr(th), nf, iptr(off), iptr(idx), 0.0, 1.0, None, None, None,
                         None, None, None), m.ctx.handle)
# malformed folds are refused, a model without an inverse too
errs = []
for bad in ([np.array([0, n])], [np.array([3, 3])], [np.array([1]), np.array([], dtype=int)]):
    try:
        cv(bad)
        errs.append("")
    except A.AceError as e:
        errs.append(str(e))
m2 = A.DeviceModel(kernel, n, s["p"], s["B"])
m2.set_data(s["y"], s["X"], s["Z"], s["sy"])
try:
    m2.cv(s["th"], sets["mixed"], 0.0, 1.0)
    errs.append("")
except A.AceError as e:
    errs.append(str(e))
res["errors"] = np.array(errs)
np.savez(out, **res)
"""


@pytest.fixture(scope="module")
def device_state(tmp_path_factory):
    cache = {}

    def get(kernel, case):
        if (kernel, case) not in cache:
            out = str(tmp_path_factory.mktemp("cv") / "state.npz")
            run_child(_STATE.format(kernel=kernel, case=case, out=out, others=N_OTHERS),
                      timeout=100)
            with np.load(out) as f:
                cache[(kernel, case)] = {k: f[k] for k in f.files}
        return cache[(kernel, case)]
    return get


# ------------------------------------------------------------ 4. against the referee
@pytest.mark.parametrize("case", C.CASES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_matches_explicit_conditioning(device_state, kernel, case):
    d = device_state(kernel, case)
    for name in C.sets_of(case):
        ref = C.reference(case, kernel, name)
        assert np.all(d[name + "/status"] == 0), name
        for k in KEYS:
            hold(d[f"{name}/{k}"], ref[k], k, f"{kernel} {case} {name}")


# ------------------------------------------------------------ 5. the three paths agree
@pytest.mark.parametrize("case", C.CASES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_paths_agree(device_state, kernel, case):
    d = device_state(kernel, case)
    for name in C.sets_of(case):
        ref = C.reference(case, kernel, name)
        assert np.all(d[name + "/sweep/status"] == 0), name
        for k in KEYS:
            hold(d[f"{name}/sweep/{k}"], ref[k], k, f"{kernel} {case} {name} (sweep above 16)")
            close(d[f"{name}/sweep/{k}"], d[f"{name}/{k}"], check=f"cv {k}: sweep vs default")
    ref = C.reference(case, kernel, "loo")
    assert np.all(d["loolist/status"] == 0)
    for k in KEYS:
        hold(d[f"loolist/{k}"], ref[k], k, f"{kernel} {case} loo as a list")
        close(d[f"loolist/{k}"], d[f"loo/{k}"], check=f"cv {k}: loo list vs k_cv_loo")


def test_default_dispatch_reaches_the_sweep():
    """513 rows is the smallest fold the whole-chip sweep takes by itself."""
    sizes = [f.size for f in C.fold_sets(700)["split513"]]
    assert sizes == [513, 187]


# ------------------------------------------------------------ 6. determinism, independence
@pytest.mark.parametrize("case", C.CASES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_bitwise_reproducible_and_independent(device_state, kernel, case):
    d = device_state(kernel, case)
    for name in C.sets_of(case):
        assert bool(d[name + "/again"]), name
        assert bool(d[name + "/sweep/again"]), name
    for k in ("first", "last", "reversed", "shuffled"):
        assert bool(d["indep/" + k]), k


@pytest.mark.parametrize("kernel", KERNELS)
def test_refusals(device_state, kernel):
    e = device_state(kernel, "130/9")["errors"]
    assert "out of range" in e[0] and "ACE_ERR_ARG" in e[0]
    assert "appears twice" in e[1]
    assert "is empty" in e[2]
    assert "ACE_ERR_UNSUPPORTED" in e[3] and "no resident inverse" in e[3]


# ------------------------------------------------------------ 7. permuted device order
_PERM = _PRE + """
import zskip_cases as ZC
out = {out!r}
res = {{}}
for case in ZC.cases():
    if case[0] not in {names!r}:
        continue
    name, kernel, n, p, B = case[:5]
    y, X, Z, th, sy = ZC.build(case)
    m = A.DeviceModel(kernel, n, p, B)
    m.set_data(y, X, Z, sy)
    m.para_update(2, th.copy())
    folds = np.split(np.random.default_rng(9).permutation(n)[:198], 6)   # 33 rows each
    put(res, name, m.cv(th, folds, C.MEAN_Y, C.STD_Y))
np.savez(out, **res)
"""


@pytest.fixture(scope="module")
def perm_state(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cvperm") / "state.npz")
    run_child(_PERM.format(out=out, names=PERM_CASES), env=dict(os.environ, ACE_ZSKIP="2"),
              timeout=100)
    with np.load(out) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("name", PERM_CASES)
def test_permuted_device_order(perm_state, name):
    import additivecausalexpansion_amd as A
    from oracle import ace_oracle as O
    case = [c for c in ZC.cases() if c[0] == name][0]
    kernel, n = case[1], case[2]
    y, X, Z, th, sy = ZC.build(case)
    perm, _ = A.zero_pattern_order(Z)
    assert not np.array_equal(perm, np.arange(n))  # the device order differs from the caller's
    Am = O.KERNELS[kernel][0](X, Z, th)["full"] + np.exp(th[0]) * np.eye(n)
    folds = np.split(np.random.default_rng(9).permutation(n)[:198], 6)
    ref = C.pack([C.condition(0.5 * (Am + Am.T), np.ravel(y), th[1], F) for F in folds])
    assert np.all(perm_state[name + "/status"] == 0)
    for k in KEYS:
        hold(perm_state[f"{name}/{k}"], ref[k], k, name)


# ------------------------------------------------------------ 8. the host-buffer entry point
HOST_SIZES = (1, 16, 17, 130)
BAD = 2  # the fold whose block is made indefinite

_HOST = _PRE + """
out = {out!r}
rng = np.random.default_rng(3)
n = 200
M = rng.normal(size=(n, n))
P = M @ M.T / n + np.eye(n)
al = rng.normal(size=n)
perm = rng.permutation(n)
cuts = np.cumsum({sizes!r})
folds = np.split(perm[:cuts[-1]], cuts[:-1])
res = dict(P=P, al=al, perm=perm)
g = A.cv_from_inverse(P, al, folds)
for k in ("resid", "var", "logdet", "mahal", "status"):
    res["good/" + k] = g[k]
Pb = P.copy()
Fb = folds[{bad}]
Pb[Fb, Fb] = -Pb[Fb, Fb]
b = A.cv_from_inverse(Pb, al, folds)   # returns ACE_OK: no exception
for k in ("resid", "var", "logdet", "mahal", "status"):
    res["bad/" + k] = b[k]
# an upper triangle of NaN is never read; a leading dimension above n
Pu = np.tril(P) + np.triu(np.full((n, n), np.nan), 1)
u = A.cv_from_inverse(Pu, al, folds)
res["upper_same"] = np.array(all(np.array_equal(u[k], g[k]) for k in ("resid", "var", "logdet")))
np.savez(out, **res)
"""


@pytest.fixture(scope="module")
def host_state(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cvhost") / "state.npz")
    run_child(_HOST.format(out=out, sizes=list(HOST_SIZES), bad=BAD), timeout=100)
    with np.load(out) as f:
        return {k: f[k] for k in f.files}


def _host_folds(d):
    cuts = np.cumsum(HOST_SIZES)
    return np.split(d["perm"][:cuts[-1]], cuts[:-1])


def test_host_entry_point_matches_numpy(host_state):
    d = host_state
    P, al = d["P"], d["al"]
    folds = _host_folds(d)
    assert np.all(d["good/status"] == 0)
    Bs = [P[np.ix_(F, F)] for F in folds]
    ref = {"resid": np.concatenate([np.linalg.solve(B, al[F]) for B, F in zip(Bs, folds)]),
           "var": np.concatenate([np.diag(np.linalg.inv(B)) for B in Bs]),
           "logdet": np.array([np.linalg.slogdet(B)[1] for B in Bs]),
           "mahal": np.array([al[F] @ np.linalg.solve(B, al[F]) for B, F in zip(Bs, folds)])}
    for k, r in ref.items():
        hold(d["good/" + k], r, k, "cv_from_inverse", tol=CV_TOL_HOST)
    assert bool(d["upper_same"])


def test_indefinite_fold_fails_alone(host_state):
    d = host_state
    off = np.concatenate([[0], np.cumsum(HOST_SIZES)])
    st = d["bad/status"]
    # rows sorted: the first pivot is a negated diagonal entry
    assert st[BAD] == 1 and np.all(np.delete(st, BAD) == 0)
    for k in ("resid", "var"):
        sl = slice(off[BAD], off[BAD + 1])
        assert np.all(np.isnan(d["bad/" + k][sl]))
        keep = np.ones(off[-1], dtype=bool)
        keep[sl] = False
        assert np.array_equal(d["bad/" + k][keep], d["good/" + k][keep])  # bitwise
    for k in ("logdet", "mahal"):
        assert np.isnan(d["bad/" + k][BAD])
        assert np.array_equal(np.delete(d["bad/" + k], BAD), np.delete(d["good/" + k], BAD))


# ------------------------------------------------------------ 9. the public function
_PUBLIC = _PRE + """
from additivecausalexpansion_amd.synthetic import readme_data, make_problem
out = {out!r}
y, X, Z = readme_data(seed=5, n=200)
fit = A.ace_train(y, X, Z, kernel="SE", basis="ns", n_knots=2, maxiter=6, verbose=False,
                  native_loop=True)
K, mom = fit["Kernel"], fit["moments"]
n = 200
groups = np.arange(n) % 7
res = dict(y=np.ravel(y), groups=groups)
for tag, kw, fl in (
        ("k5", dict(folds=5), np.array_split(np.random.default_rng(0).permutation(n), 5)),
        ("loo", dict(folds="loo"), [np.array([i]) for i in range(n)]),
        ("grp", dict(groups=groups), [np.flatnonzero(groups == g) for g in range(7)]),
        ("ovl", dict(folds=[np.arange(30), np.arange(20, 50)]), [np.arange(30), np.arange(20, 50)])):
    r = A.cross_validate(fit, **kw)
    for k, v in r.items():
        res[tag + "/" + k] = np.asarray(v)
    d = K._model.cv(K.parameters, fl, mom[0, 0], mom[0, 1])
    put(res, tag + "/dev", d)
    res[tag + "/idx"] = np.concatenate(fl)
# errors: a sharded model (one simulated rank), an inverse that is not resident
errs = []
ys, Xs, Zs, th, sy = make_problem(300, 3, 4, seed=8)
Ks = A.KernelClass_SE_R6(3, 4, th, sy)
Ks.use_model(A.DeviceModel("SE", 300, 3, 4, world=1, rank=0, sharded=True), ys, Xs, Zs)
Ks.para_update(2, ys, Xs, Zs, A.optNadam(Ks, 0.01, 0.9, 0.999, True, 1.0), verbose=False)
class Bs:
    B = Zs
fs = dict(Kernel=Ks, train_data=dict(y=ys, X=Xs), Basis=Bs, moments=np.array([[0.0, 1.0]]))
Kn = A.KernelClass_SE_R6(3, 4, th, sy)
Kn.getinv_kernel(Xs, Zs)
for f in (fs, dict(fs, Kernel=Kn)):
    try:
        A.cross_validate(f, folds=3)
        errs.append("")
    except A.AceError as e:
        errs.append(str(e))
res["errors"] = np.array(errs)
np.savez(out, **res)
"""


@pytest.fixture(scope="module")
def public_state(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cvpub") / "state.npz")
    run_child(_PUBLIC.format(out=out), timeout=100)
    with np.load(out) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("tag", ["k5", "loo", "grp"])
def test_cross_validate_equals_device_model(public_state, tag):
    d = public_state
    idx = d[tag + "/idx"]
    n = 200
    for k in ("map", "var", "resid"):
        assert d[f"{tag}/{k}"].shape == (n,)
        assert np.array_equal(d[f"{tag}/{k}"][idx], d[f"{tag}/dev/{k}"])
    for k in ("lpd", "mahal", "status"):
        assert np.array_equal(d[f"{tag}/{k}"], d[f"{tag}/dev/{k}"])
    mp, var, res = d[tag + "/map"], d[tag + "/var"], d[tag + "/resid"]
    assert np.all(np.isfinite(mp)) and np.all(var > 0)   # every row is in a fold here
    assert np.all(d[tag + "/fold"] >= 0) and np.array_equal(np.bincount(d[tag + "/fold"]), d[tag + "/size"])
    sd = np.sqrt(var)
    assert np.array_equal(d[tag + "/ci"], np.column_stack([mp - 1.96 * sd, mp + 1.96 * sd]))
    assert np.array_equal(d[tag + "/z"], res / sd)
    assert float(d[tag + "/elpd"]) == float(np.sum(d[tag + "/lpd"]))
    assert float(d[tag + "/rmse"]) == float(np.sqrt(np.mean(res[idx] ** 2)))  # fold after fold
    # resid is the held-out y minus its prediction, in original units
    y = d["y"]
    assert np.allclose(y - mp, res, rtol=0, atol=1e-9 * np.abs(y).max())
    inside = (y >= d[tag + "/ci"][:, 0]) & (y <= d[tag + "/ci"][:, 1])
    assert abs(float(d[tag + "/coverage"]) - inside.mean()) <= 1.0 / n + 1e-12
    if tag == "grp":
        assert np.array_equal(d["grp/fold"], d["groups"])


def test_cross_validate_overlapping_folds_are_packed(public_state):
    d = public_state
    assert "ovl/fold" not in d and d["ovl/map"].shape == (60,)
    assert np.array_equal(d["ovl/off"], [0, 30, 60])
    for k in ("map", "var", "resid", "lpd"):
        assert np.array_equal(d["ovl/" + k], d["ovl/dev/" + k])


def test_cross_validate_refuses_what_it_cannot_do(public_state):
    e = public_state["errors"]
    assert "sharded" in e[0] and "ACE_ERR_UNSUPPORTED" in e[0]
    assert "device-resident inverse" in e[1]
