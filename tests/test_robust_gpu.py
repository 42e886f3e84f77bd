"""GPU tests of the grouped posterior sums (ace_model_predict_marginal_groups)
and of robust_treatment built on them (ace_model_robust_treatment,
R/robust_treatment.R:67-128), against the oracle: pred_marginal_cpp is called
once per retained subset, which is the reference's own call sequence.

gcov = E^T (Km_xx - Km_xX A^-1 Km_xX^T) E cancels two terms up to cond x
larger than the result, so it is held entrywise to COV_TOL of
T_gh = sum_{i in g, j in h} (|Km_xx| + |Km_xX A^-1 Km_xX^T|)_ij, the same
convention as VAR_TOL of test_predict_gpu (1.5e-9 for the same cancellation).
COV_TOL = 1.5e-9 is 4.2x the largest max |err| / T measured over this file's
cases, 3.57e-10 (Matern32, n = 400, B = 6, G = 17; the per-step variances
reach 3.4e-10 of their terms, the other grouped cases 1e-10 and below; every
figure in profiles/robust_error_table.txt).

The robust_treatment cases are chosen (and checked on the CPU from the
oracle alone, see _preconditions) so that no discard threshold lies within
the variance's own tolerance of a test point's variance -- then the retained
sets of the device and of the oracle are the same sets -- and so that every
posterior form is well above COV_TOL of its terms.
"""
import numpy as np

from conftest import record_error
import pytest
from robust_ref import indicator, levels_ref, step_post
from test_gpu import close
from test_predict_gpu import VAR_TOL, _fit_state, _test_points

pytestmark = pytest.mark.gpu

COV_TOL = 1.5e-9
MEAN_Y, STD_Y, STD_Z = 0.3, 1.7, 0.8
N_STEPS = 5
KEYS = ("ate", "att", "atu")


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.default_context()
    return pkg


@pytest.fixture(scope="module")
def O():
    from oracle import ace_oracle
    return ace_oracle


# --------------------------------------------------------------------------
# shared references: one per (kernel, shape), computed once, never modified
# --------------------------------------------------------------------------
_CASES = {}


def oracle_case(O, kernel, n, p, B, nx, insample=False, model=None):
    """Oracle quantities of one case (no GPU): the marginal kernels, the
    posterior covariance C, the cancelled terms Tm, the per-point prediction
    and the variance terms of test_predict_gpu._var_terms."""
    from additivecausalexpansion_amd.synthetic import make_problem
    y, X, Z, th, sy = make_problem(n, p, B, seed=5 + B)
    th = th.copy()
    inv = O.invkernel_cpp(O.KERNELS[kernel][0](X, Z, th)["full"], th[0])["inv"]
    th[1] = 0.13
    if insample:
        X2, Z2 = X, Z
    else:
        X2, Z2 = _test_points(p, B, nx, seed=77)
    dZ2 = np.asfortranarray(Z2 * 0.7 + 0.1)
    zx = (np.arange(nx) % 3 == 0).astype(float)
    sym, cross = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    Km_xX = cross(X2, X, dZ2, Z, th)["elements"]
    Km_xx = sym(X2, dZ2, th)["elements"]
    sl = slice(1, B) if B > 1 else slice(0, 1)
    KmX = Km_xX[:, :, sl].sum(axis=2)
    Kxx = Km_xx[:, :, sl].sum(axis=2)
    P = KmX @ inv @ KmX.T
    ref = O.pred_marginal_cpp(y, zx, th[0], th[1], inv, Km_xX, Km_xx, MEAN_Y, STD_Y, STD_Z, False)
    terms = (STD_Y / STD_Z) ** 2 * (np.abs(np.diag(Kxx)) + np.abs(np.diag(P)))
    return dict(y=y, X=X, Z=Z, th=th, inv=inv, X2=X2, dZ2=dZ2, zx=zx, Km_xX=Km_xX, Km_xx=Km_xx,
                C=Kxx - P, Tm=np.abs(Kxx) + np.abs(P), ref=ref, terms=terms, nx=nx)


def case(A, O, kernel, n, p, B, nx, insample=False):
    key = (kernel, n, p, B, nx, insample)
    if key not in _CASES:
        c = oracle_case(O, kernel, n, p, B, nx, insample)
        m, y, X, Z, th, sy, inv = _fit_state(O, kernel, n, p, B, seed=5 + B, A=A, mix=False)
        assert np.array_equal(th, c["th"]) and np.array_equal(X, c["X"])
        c["m"] = m
        _CASES[key] = c
    return _CASES[key]


def robust_ref(O, c, n_steps=N_STEPS):
    """The reference's loop (R/robust_treatment.R:83-128) on the oracle:
    thresholds and levels from the oracle's variances, then
    pred_marginal_cpp on every retained subset."""
    if "robust" in c:
        return c["robust"]
    var = c["ref"]["var"]
    thr, level = levels_ref(var, n_steps)
    zx = c["zx"]
    steps = []
    for t in range(n_steps + 1):
        keep = var <= thr[t]
        assert np.array_equal(keep, level <= t)
        r = O.pred_marginal_cpp(c["y"], zx[keep], c["th"][0], c["th"][1], c["inv"],
                                c["Km_xX"][keep], c["Km_xx"][keep][:, keep], MEAN_Y, STD_Y, STD_Z,
                                True)
        sel = {"ate": keep, "att": keep & (zx == 1), "atu": keep & (zx == 0)}
        steps.append({"keep": keep, "ref": r,
                      "count": {k: int(s.sum()) for k, s in sel.items()},
                      "T": {k: c["Tm"][np.ix_(s, s)].sum() for k, s in sel.items()},
                      "post": {k: c["C"][np.ix_(s, s)].sum() for k, s in sel.items()}})
    c["robust"] = dict(thr=thr, level=level, steps=steps)
    return c["robust"]


def _preconditions(c, rr, n_steps=N_STEPS):
    """From the oracle alone.  (a) every cut is at least 20 VAR_TOL max(terms)
    away from the nearest variance on either side (at the two extremes the
    threshold is an order statistic itself: the gap to the next one inside);
    (b) every non-empty posterior form is at least 100 COV_TOL of its terms."""
    var, thr = c["ref"]["var"], rr["thr"]
    x = np.sort(var)
    need = 20 * VAR_TOL * np.max(c["terms"])
    margins = []
    for t in range(n_steps + 1):
        if t == 0:
            gap = x[1] - thr[0]
        elif t == n_steps:
            gap = thr[t] - x[-2]
        else:
            gap = np.min(np.abs(var - thr[t]))
        margins.append(gap)
        assert gap >= need, (t, gap, need)
    ratios = []
    for t, s in enumerate(rr["steps"]):
        for k in KEYS:
            if s["count"][k] > 0:
                ratios.append(s["post"][k] / s["T"][k])
                assert s["post"][k] >= 100 * COV_TOL * s["T"][k], (t, k, s["post"][k], s["T"][k])
    return min(margins) / np.max(c["terms"]), min(ratios)


def _avg_bounds(step, k):
    """e (variance bound) and the ci bound's sd term for one (step, estimand)."""
    m = step["count"][k]
    e = STD_Y ** 2 / m ** 2 * COV_TOL * step["T"][k]
    sd_ref = np.sqrt(step["ref"][k]["var"])
    return e, sd_ref


def _check_avg(got_map, got_ci, got_var, step, k, what):
    ref = step["ref"][k]
    if step["count"][k] == 0:
        assert np.isnan(got_var) and np.isnan(ref["var"]), what
        assert np.all(np.isnan(got_ci)) and np.all(np.isnan(ref["ci"])), what
        return
    if np.isnan(ref["map"]):  # ATU's map with an empty treated group (NaN * 0)
        assert np.isnan(got_map), what
    else:
        close(got_map, ref["map"], 1e-6, 0.0)
    e, sd_ref = _avg_bounds(step, k)
    record_error(f"robust {k} var: |err| / (std_y^2 / m^2 T)",
                 abs(got_var - ref["var"]) / (e / COV_TOL), COV_TOL)
    assert abs(got_var - ref["var"]) <= e, (what, got_var, ref["var"], e)
    if np.isnan(ref["map"]):
        assert np.all(np.isnan(got_ci)) and np.all(np.isnan(ref["ci"])), what
    else:
        tol = 1e-6 * abs(ref["map"]) + 2 * e / sd_ref
        assert np.all(np.abs(np.ravel(got_ci) - ref["ci"]) <= tol), (what, got_ci, ref["ci"], tol)


# --------------------------------------------------------------------------
# 1. grouped primitive vs oracle
# --------------------------------------------------------------------------
def _labels(nx, G):
    i = np.arange(nx)
    if G == 1:
        return np.zeros(nx, dtype=np.int32)
    if G == 3:
        return (i % 4 - 1).astype(np.int32)
    if G == 17:
        return (i % 17).astype(np.int32)
    lab = (i % 64).astype(np.int32)
    lab[(lab == 5) | (lab == 40)] = -1   # empty groups
    lab[(lab == 7) & (i != 7)] = -1      # exactly one point in group 7
    return lab


def _check_gcov(got, c, label, G, what):
    E = indicator(label, G)
    ref = E.T @ c["C"] @ E
    T = E.T @ c["Tm"] @ E
    live = T > 0
    err = np.abs(got - ref)
    assert np.all(got[~live] == 0)  # empty groups
    worst = np.max(err[live] / T[live]) if np.any(live) else 0.0
    record_error(f"{what}: max |err| / T", worst, COV_TOL)
    print(f"{what}: max |gcov err| / T = {worst:.3e}")
    assert np.all(err <= COV_TOL * T), (what, worst)
    assert np.all(np.abs(got - got.T) <= COV_TOL * T), what
    return T


@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
@pytest.mark.parametrize("n,p,B,nx,G", [(130, 1, 1, 9, 1), (400, 3, 2, 150, 3),
                                        (700, 20, 10, 257, 64), (400, 3, 6, 150, 17),
                                        (70, 50, 32, 65, 17)])
def test_grouped_sums_match_oracle(A, O, kernel, n, p, B, nx, G):
    """The last shape (PM = 64, B = 32) is k_group_mm's largest request of
    dynamic LDS, 149248 B for SE."""
    c = case(A, O, kernel, n, p, B, nx)
    m = c["m"]
    label = _labels(nx, G)
    if G == 64:
        assert np.sum(label == 7) == 1 and not np.any(label == 5) and np.any(label == -1)
    got = m.predict_marginal_groups(c["th"], c["X2"], c["dZ2"], STD_Y, STD_Z, G, label)
    _check_gcov(got["gcov"], c, label, G, f"groups {kernel} n={n} G={G}")
    E = indicator(label, G)
    assert np.array_equal(got["gcount"], E.sum(axis=0).astype(np.int64))
    close(got["gsum"], E.T @ c["ref"]["map"], 1e-6, 1e-9)
    plain = m.predict_marginal(c["th"], c["X2"], c["dZ2"], c["zx"], STD_Y, STD_Z, False)
    for k in ("map", "ci", "var"):
        assert np.array_equal(got[k], plain[k]), k
    close(got["map"], c["ref"]["map"])


# --------------------------------------------------------------------------
# 2. / 3. robust_treatment vs oracle and vs the existing path
# --------------------------------------------------------------------------
ROBUST_SHAPES = [(400, 3, 2, 150, False), (400, 3, 6, 150, False), (700, 20, 10, 257, False),
                 (260, 3, 2, 260, True)]


@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
@pytest.mark.parametrize("n,p,B,nx,insample", ROBUST_SHAPES)
def test_robust_treatment_matches_oracle(A, O, kernel, n, p, B, nx, insample):
    c = case(A, O, kernel, n, p, B, nx, insample)
    rr = robust_ref(O, c)
    margin, ratio = _preconditions(c, rr)
    print(f"preconditions: margin / max(terms) = {margin:.3e}, min post / T = {ratio:.3e}")
    got = c["m"].robust_treatment(c["th"], c["X2"], c["dZ2"], c["zx"], STD_Y, STD_Z, N_STEPS)
    c["got_robust"] = got
    assert np.array_equal(got["level"], rr["level"])
    assert np.all(np.abs(got["thresholds"] - rr["thr"]) <= VAR_TOL * np.max(c["terms"]))
    close(got["map"], c["ref"]["map"])
    for t, step in enumerate(rr["steps"]):
        cnt = step["count"]
        assert list(got["counts"][:, t]) == [cnt["ate"], cnt["att"], cnt["atu"]]
        for j, k in enumerate(KEYS):
            a = got["avg"][4 * j:4 * j + 4, t]
            _check_avg(a[0], a[1:3], a[3], step, k, (kernel, n, t, k))
            assert np.array_equal(got[k]["map"][t], a[0], equal_nan=True) and np.array_equal(
                got[k]["var"][t], a[3], equal_nan=True)
    # step 0 keeps the one point of smallest variance: the group it is not in
    # is empty, with NaN (0 / 0) in both; the other's variance is finite (with
    # an empty treated group ATU's map is NaN * 0 in both)
    s0 = rr["steps"][0]
    assert s0["count"]["ate"] == 1 and s0["count"]["att"] + s0["count"]["atu"] == 1
    empty, full = (1, 2) if s0["count"]["att"] == 0 else (2, 1)
    assert np.isnan(got["avg"][4 * empty + 3, 0]) and np.isnan(s0["ref"][KEYS[empty]]["var"])
    assert np.isfinite(got["avg"][4 * full + 3, 0]) and np.isfinite(s0["ref"][KEYS[full]]["var"])
    if empty == 1:
        assert np.isnan(got["avg"][4, 0]) and np.isnan(s0["ref"]["att"]["map"])
    assert got["counts"][0, -1] == nx


@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
@pytest.mark.parametrize("n,p,B,nx,insample", ROBUST_SHAPES)
def test_robust_treatment_matches_existing_path(A, O, kernel, n, p, B, nx, insample):
    """The reference's literal loop through the pre-existing
    predict_marginal(..., calculate_ate=True) on every retained subset."""
    c = case(A, O, kernel, n, p, B, nx, insample)
    rr = robust_ref(O, c)
    m = c["m"]
    got = c.get("got_robust") or m.robust_treatment(c["th"], c["X2"], c["dZ2"], c["zx"], STD_Y,
                                                    STD_Z, N_STEPS)
    for t, step in enumerate(rr["steps"]):
        keep = got["level"] <= t
        old = m.predict_marginal(c["th"], c["X2"][keep], c["dZ2"][keep], c["zx"][keep], STD_Y,
                                 STD_Z, True)
        for j, k in enumerate(KEYS):
            a = got["avg"][4 * j:4 * j + 4, t]
            o = old[k]
            if step["count"][k] == 0:
                assert np.isnan(a[3]) and np.isnan(o["var"])
                continue
            if np.isnan(o["map"]):
                assert np.isnan(a[0])
            else:
                close(a[0], o["map"], 1e-6, 0.0)
            e, sd_ref = _avg_bounds(step, k)
            assert abs(a[3] - o["var"]) <= e, (t, k, a[3], o["var"], e)
            if np.isnan(o["map"]):
                assert np.all(np.isnan(a[1:3])) and np.all(np.isnan(o["ci"])), (t, k)
            else:
                tol = 1e-6 * abs(o["map"]) + 2 * e / sd_ref
                assert np.all(np.abs(a[1:3] - o["ci"]) <= tol), (t, k)


# --------------------------------------------------------------------------
# 4. other step counts, argument errors
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [1, 31])
def test_robust_treatment_other_step_counts(A, O, n_steps):
    c = case(A, O, "SE", 400, 3, 2, 150)
    got = c["m"].robust_treatment(c["th"], c["X2"], c["dZ2"], c["zx"], STD_Y, STD_Z, n_steps)
    assert got["avg"].shape == (12, n_steps + 1) and got["counts"].shape == (3, n_steps + 1)
    thr, level = A.robust_levels(got["var"], n_steps)
    assert np.array_equal(level, got["level"]) and np.array_equal(thr, got["thresholds"])
    for t in range(n_steps + 1):
        keep = got["level"] <= t
        assert list(got["counts"][:, t]) == [keep.sum(), (keep & (c["zx"] == 1)).sum(),
                                             (keep & (c["zx"] == 0)).sum()]
    assert got["counts"][0, -1] == 150 and got["counts"][0, 0] >= 1
    full = c["m"].predict_marginal(c["th"], c["X2"], c["dZ2"], c["zx"], STD_Y, STD_Z, True)
    close(got["avg"][0, -1], full["ate"]["map"], 1e-6, 0.0)


def test_robust_treatment_argument_errors(A, O):
    c = case(A, O, "SE", 400, 3, 2, 150)
    m, th, X2, dZ2, zx = c["m"], c["th"], c["X2"], c["dZ2"], c["zx"]
    for bad in (0, 32):
        with pytest.raises(A.AceError, match="ARG"):
            m.robust_treatment(th, X2, dZ2, zx, STD_Y, STD_Z, bad)
    z2 = zx.copy()
    z2[3] = 0.5
    with pytest.raises(A.AceError, match="ARG"):
        m.robust_treatment(th, X2, dZ2, z2, STD_Y, STD_Z, 5)
    lab = np.zeros(150, dtype=np.int32)
    for G in (0, 65):
        with pytest.raises(A.AceError, match="ARG"):
            m.predict_marginal_groups(th, X2, dZ2, STD_Y, STD_Z, G, lab)
    lab[10] = 4
    with pytest.raises(A.AceError, match="ARG"):
        m.predict_marginal_groups(th, X2, dZ2, STD_Y, STD_Z, 4, lab)
    lab[10] = -2
    with pytest.raises(A.AceError, match="ARG"):
        m.predict_marginal_groups(th, X2, dZ2, STD_Y, STD_Z, 4, lab)
    fresh = A.DeviceModel("SE", 400, 3, 2)
    fresh.set_data(c["y"], c["X"], c["Z"], 1.0)
    with pytest.raises(A.AceError, match="ARG"):
        fresh.robust_treatment(th, X2, dZ2, zx, STD_Y, STD_Z, 5)
    with pytest.raises(A.AceError, match="ARG"):
        fresh.predict_marginal_groups(th, X2, dZ2, STD_Y, STD_Z, 1, np.zeros(150, dtype=np.int32))


# --------------------------------------------------------------------------
# 5. determinism
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
def test_grouped_sums_are_bitwise_reproducible(A, O, kernel):
    c = case(A, O, kernel, 700, 20, 10, 257)
    m = c["m"]
    label = _labels(257, 64)
    a = m.predict_marginal_groups(c["th"], c["X2"], c["dZ2"], STD_Y, STD_Z, 64, label)
    b = m.predict_marginal_groups(c["th"], c["X2"], c["dZ2"], STD_Y, STD_Z, 64, label)
    assert np.array_equal(a["gcov"], b["gcov"])
    r1 = m.robust_treatment(c["th"], c["X2"], c["dZ2"], c["zx"], STD_Y, STD_Z, N_STEPS)
    r2 = m.robust_treatment(c["th"], c["X2"], c["dZ2"], c["zx"], STD_Y, STD_Z, N_STEPS)
    assert np.array_equal(r1["avg"], r2["avg"], equal_nan=True)


# --------------------------------------------------------------------------
# 6. chunking: S accumulated over two K_xX chunks
# --------------------------------------------------------------------------
def test_grouped_sums_two_chunks(A, O):
    kernel, n, p, B, nx, G = "SE", 333, 2, 1, 8192 + 77, 4
    m, y, X, Z, th, sy, inv = _fit_state(O, kernel, n, p, B, seed=5 + B, A=A, mix=False)
    X2, Z2 = _test_points(p, B, nx, seed=77)
    dZ2 = np.asfortranarray(Z2 * 0.7 + 0.1)
    label = (np.arange(nx) % 5 - 1).astype(np.int32)
    cross = O.KERNELS[kernel][1]
    E = indicator(label, G)
    KmX = cross(X2, X, dZ2, Z, th)["full"]  # B = 1: slice 0 is the marginal kernel
    W = KmX @ inv
    ref = np.zeros((G, G))
    T = np.zeros((G, G))
    for i0 in range(0, nx, 1024):  # row blocks: no nx x nx array on the host
        blk = slice(i0, min(i0 + 1024, nx))
        Kb = cross(X2[blk], X2, dZ2[blk], dZ2, th)["full"]
        Pb = W[blk] @ KmX.T
        ref += E[blk].T @ ((Kb - Pb) @ E)
        T += E[blk].T @ ((np.abs(Kb) + np.abs(Pb)) @ E)
    got = m.predict_marginal_groups(th, X2, dZ2, STD_Y, STD_Z, G, label)
    err = np.abs(got["gcov"] - ref)
    record_error("groups two chunks: max |err| / T", np.max(err / T), COV_TOL)
    print(f"two chunks: max |gcov err| / T = {np.max(err / T):.3e}")
    assert np.all(err <= COV_TOL * T)
    assert np.array_equal(got["gcount"], E.sum(axis=0).astype(np.int64))
    close(got["gsum"], E.T @ (STD_Y * (W @ (y - th[1])) / STD_Z), 1e-6, 1e-9)


# --------------------------------------------------------------------------
# 7. sharded models
# --------------------------------------------------------------------------
def test_sharded_robust_treatment_matches_single(A, O):
    kernel, n, p, B, nx = "Matern32", 1100, 4, 5, 300
    single, y, X, Z, th, sy, inv = _fit_state(O, kernel, n, p, B, seed=21, A=A, mix=False)
    sh, *_ = _fit_state(O, kernel, n, p, B, seed=21, sharded=True, world=3, A=A, mix=False)
    X2, Z2 = _test_points(p, B, nx, seed=22)
    dZ2 = np.asfortranarray(Z2 * 0.7 + 0.1)
    zx = (np.arange(nx) % 3 == 0).astype(float)
    a = single.robust_treatment(th, X2, dZ2, zx, STD_Y, STD_Z, N_STEPS)
    b = sh.robust_treatment(th, X2, dZ2, zx, STD_Y, STD_Z, N_STEPS)
    assert np.array_equal(a["level"], b["level"]) and np.array_equal(a["counts"], b["counts"])
    G = 2 * (N_STEPS + 1)
    label = (2 * a["level"] + zx).astype(np.int32)
    ga = single.predict_marginal_groups(th, X2, dZ2, STD_Y, STD_Z, G, label)
    gb = sh.predict_marginal_groups(th, X2, dZ2, STD_Y, STD_Z, G, label)
    sym, cross = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    KmX = cross(X2, X, dZ2, Z, th)["elements"][:, :, 1:].sum(axis=2)
    Kxx = sym(X2, dZ2, th)["elements"][:, :, 1:].sum(axis=2)
    E = indicator(label, G)
    T = E.T @ (np.abs(Kxx) + np.abs(KmX @ inv @ KmX.T)) @ E
    err = np.abs(gb["gcov"] - ga["gcov"])
    record_error("groups sharded vs single: max |err| / T", np.max(err[T > 0] / T[T > 0]), COV_TOL)
    assert np.all(err <= COV_TOL * T)
    # the per-step variances follow from gcov by the same prefix sums
    for t in range(N_STEPS + 1):
        for j, post in enumerate(step_post(gb["gcov"], t)):
            cnt = b["counts"][j, t]
            if cnt > 0:
                assert np.isclose(b["avg"][4 * j + 3, t], (STD_Y * np.sqrt(post) / cnt) ** 2,
                                  rtol=1e-12, atol=0)


def test_sharded_rccl_world1_robust_treatment(A, O):
    from additivecausalexpansion_amd.synthetic import make_problem
    kernel, n, p, B, nx = "SE", 700, 3, 4, 120
    y, X, Z, th0, sy = make_problem(n, p, B, seed=8)
    sh = A.DeviceModel(kernel, n, p, B, world=1, rank=0, unique_id=A.comm_unique_id(),
                       sharded=True)
    sh.set_data(y, X, Z, sy)
    sh.para_update(2, th0.copy())
    single = A.DeviceModel(kernel, n, p, B)
    single.set_data(y, X, Z, sy)
    single.para_update(2, th0.copy())
    X2, Z2 = _test_points(p, B, nx, seed=9)
    dZ2 = np.asfortranarray(Z2 * 0.7 + 0.1)
    zx = (np.arange(nx) % 3 == 0).astype(float)
    label = (np.arange(nx) % 4).astype(np.int32)
    c0 = sh.comm_calls()["allreduce"]
    plain = sh.predict_marginal(th0, X2, dZ2, zx, STD_Y, STD_Z, False)
    c1 = sh.comm_calls()["allreduce"]
    g = sh.predict_marginal_groups(th0, X2, dZ2, STD_Y, STD_Z, 4, label)
    c2 = sh.comm_calls()["allreduce"]
    sh.robust_treatment(th0, X2, dZ2, zx, STD_Y, STD_Z, N_STEPS)
    c3 = sh.comm_calls()["allreduce"]
    # the grouped pass adds its own all-reduce (Q_inv) to the pipeline's
    assert c2 - c1 > c1 - c0 > 0 and c3 - c2 == c2 - c1
    assert np.array_equal(g["map"], plain["map"])
    gs = single.predict_marginal_groups(th0, X2, dZ2, STD_Y, STD_Z, 4, label)
    scale = np.max(np.abs(gs["gcov"]))
    assert np.max(np.abs(g["gcov"] - gs["gcov"])) <= 1e-6 * scale


# --------------------------------------------------------------------------
# 8. Python level: ace_train -> robust_treatment
# --------------------------------------------------------------------------
def _binary_example(n=300, seed=1231):
    """The data shape of the reference's robust_treatment example
    (R/robust_treatment.R:21-47): binary Z, one confounder, one exogenous
    variable."""
    rng = np.random.default_rng(seed)
    Z = (rng.random(n) < 0.3).astype(float)
    x = np.where(Z == 1, rng.normal(30, 10, n), rng.normal(20, 10, n))
    e = rng.random(n)
    y0 = 72 + 3 * (x > 0) * np.sqrt(np.abs(x))
    y1 = 90 + np.exp(0.06 * e)
    y = np.where(Z == 1, rng.normal(y1, 1), rng.normal(y0, 1))
    return y, np.column_stack([x, e]), Z.reshape(n, 1)


def test_python_robust_treatment_matches_predict_loop(A):
    y, X, Z = _binary_example()
    # learning rate 0.001: the five steps leave theta_T close enough to the
    # resident inverse's theta_{T-1} (Q6) that every posterior form is
    # positive; at the example's 0.005 nearly all are negative, NaN in both
    # paths, and nothing would be compared (checked for this seed)
    fit = A.ace_train(y, X, Z, kernel="SE", optimizer="Nadam", learning_rate=0.001, maxiter=5,
                      verbose=False, native_loop=True)
    res = A.robust_treatment(fit, n_steps=5)
    idx = res["idx"]
    n = 300
    assert idx.shape == (n, 6) and idx.dtype == bool and np.all(idx[:, -1])
    assert np.all(idx[:, :-1] <= idx[:, 1:])  # nested
    assert res["ate"].shape == (6, 7) and res["att"].shape == (6, 4) and res["atu"].shape == (6, 4)
    Xtr, Ztr = fit["train_data"]["X"], fit["train_data"]["Z"]
    full = A.predict_ace(fit, marginal=True)
    assert np.array_equal(idx, full["var"][:, None] <= res["thresholds"][None, :])
    K = fit["Kernel"]
    mom = fit["moments"]
    sy = mom[0, 1]
    for t in range(6):
        keep = idx[:, t]
        old = A.predict_ace(fit, newX=Xtr[keep], newZ=Ztr[keep], marginal=True,
                            return_average_treatments=True, normalize=False)
        zk = Ztr[keep, 0]
        assert res["ate"][t, 4] == keep.sum() and res["ate"][t, 5] == zk.sum()
        assert res["ate"][t, 6] == keep.sum() - zk.sum()
        # T of the subset from the library's own kernels (the same bound as
        # test_robust_treatment_matches_existing_path)
        tb = fit["Basis"].testbasis(Ztr[keep])
        KmX = A.kernmat_SE_cpp(Xtr[keep], Xtr, tb["dB"], fit["Basis"].B,
                               K.parameters)["elements"][:, :, 1:].sum(axis=2)
        Kxx = A.kernmat_SE_symmetric_cpp(Xtr[keep], tb["dB"],
                                         K.parameters)["elements"][:, :, 1:].sum(axis=2)
        Tm = np.abs(Kxx) + np.abs(KmX @ K._model.inverse() @ KmX.T)
        for tab, k, sel in ((res["ate"], "ate", np.ones(keep.sum(), bool)),
                            (res["att"], "att", zk == 1), (res["atu"], "atu", zk == 0)):
            if sel.sum() == 0:
                assert np.all(np.isnan(tab[t, :4]))
                continue
            o = old[k]
            e = sy ** 2 / sel.sum() ** 2 * COV_TOL * Tm[np.ix_(sel, sel)].sum()
            if np.isnan(o["map"]):
                assert np.isnan(tab[t, 0])
            else:
                close(tab[t, 0], o["map"], 1e-6, 0.0)
            assert np.isfinite(o["var"]), (t, k)  # every form positive (learning rate above)
            assert abs(tab[t, 3] - o["var"]) <= e, (t, k, tab[t, 3], o["var"], e)
            if not np.isnan(o["map"]):
                tol = 1e-6 * abs(o["map"]) + 2 * e / np.sqrt(o["var"])
                assert np.all(np.abs(tab[t, 1:3] - o["ci"]) <= tol), (t, k)
    oos = A.robust_treatment(fit, newX=X[:50], n_steps=3)
    assert oos["ate"].shape == (4, 5) and "att" not in oos and oos["idx"].shape == (50, 4)
    assert oos["ate"][-1, 4] == 50 and np.all(np.isfinite(oos["ate"][:, :4]))


def test_python_robust_treatment_needs_binary_treatment(A):
    from additivecausalexpansion_amd.synthetic import readme_data
    y, X, Z = readme_data(n=120)
    fit = A.ace_train(y, X, Z, kernel="SE", maxiter=3, verbose=False, native_loop=True)
    with pytest.raises(A.AceError, match="binary"):
        A.robust_treatment(fit, n_steps=5)
