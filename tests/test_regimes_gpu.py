"""The pair kernels across input regimes (tests/regimes.py) against the
extended-precision referee.

a. MFMA family, elementwise: K of k_cross_mm (the expansion form
   r2 = s(r) + s(c) - 2 G on the matrix cores, the hand-written exp / sqrt)
   within `k_bound` per element -- a bound derived from the arithmetic, not
   from any device result (tests/regimes.py; tests/test_regimes_cpu.py shows
   fp64 arithmetic of the same form uses at most 0.49 of it).  This is the
   test that holds the "bounded by eps * (s_b(r) + s_b(c))" sentence of the
   kernel file's header.
b. VALU family (the public kernmat_* calls with the cube) on the same inputs,
   `full` and every slice, under the same bound.
c. The fused model (k_asm_mm, sweep, k_grad_mm) in every model regime:
   gradient, statistics and mu within the project's contract of the referee,
   and the gradient also against the referee's gradient evaluated with the
   device's own inverse (which isolates k_grad_mm and the K it recomputes
   from the inverse's error).
d. The test-side kernels (k_cross_mm inside predict, k_group_mm inside
   predict_marginal_groups) on duplicated, in-range and far extrapolated test
   points, against the oracle's prediction chain with the tolerances of
   tests/test_predict_gpu.py and tests/test_robust_gpu.py.
Every case has n <= 130.
"""
import functools

import numpy as np
import pytest

import regimes as R
from conftest import record_error
from referee_ld import LD, grad_from_inverse
from test_predict_gpu import VAR_TOL, _var_terms
from test_regimes_cpu import contract_used, referee, used
from test_robust_gpu import _check_gcov

pytestmark = pytest.mark.gpu

KERNELS = ["SE", "Matern32"]
B = 3
# every regime at p = 3 (PM = 4); four of them again at p = 20 (PM = 20: the
# 4x4x4 tail path) and p = 40 (PM = 48: row operand read from memory)
K_CASES = [(name, 3) for name in R.REGIMES] + [(name, p) for p in (20, 40)
                                                for name in ("base", "dups", "ramp30", "zext")]


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.default_context()
    return pkg


@functools.lru_cache(maxsize=None)
def k_reference(name, kernel, p):
    """The two K problems of one regime with their referee values and bounds
    (full and per slice), computed once and shared; never modified."""
    _, X, Z, th, _ = R.regime(name, 130, p, B, 5)
    out = []
    cases = [(X, X, Z, Z, th), R.cross_points(name, p, B)]
    if name == "zext":  # slice 0 switched off: the other slices' exact zeros show in the full K
        off = th.copy()
        off[2] = -2000.0
        cases.append((X, X, Z, Z, off))
    for X1, X2, Z1, Z2, t in cases:
        out.append((X1, X2, Z1, Z2, t) + R.k_bound(kernel, X1, X2, Z1, Z2, t, slices=True))
    return out


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name,p", K_CASES)
def test_mfma_pair_arithmetic_within_bound(A, name, p, kernel):
    from additivecausalexpansion_amd import native
    from additivecausalexpansion_amd._lib import KIND
    for which, (X1, X2, Z1, Z2, th, Kref, bound, Kb, _) in zip(("self", "cross", "self, slice 0 off"),
                                                              k_reference(name, kernel, p)):
        K = native._kernmat_cross(KIND[kernel], X1, X2, Z1, Z2, th, elements=False)["full"]
        frac = used(K, Kref, bound)  # asserts finite, and exactly 0 where the referee is
        if th[2] == -2000.0:  # exp(-2000 - r2) is 0 in fp64: K is the sum of the z slices
            dead = np.all(Kb[1:] == 0, axis=0)
            assert np.any(dead) and np.all(K[dead] == 0)
        print(f"mfma {name} {kernel} p={p} {which}: {frac:.3g} of the K bound")
        record_error(f"regime K bound used, MFMA family ({which})", frac, 1.0)
        assert frac <= 1.0, (which, frac)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name,p", K_CASES)
def test_valu_pair_arithmetic_within_bound(A, name, p, kernel):
    cross = A.kernmat_SE_cpp if kernel == "SE" else A.kernmat_Matern32_cpp
    sym = A.kernmat_SE_symmetric_cpp if kernel == "SE" else A.kernmat_Matern32_symmetric_cpp
    (X, _, Z, _, th, Kref, bound, Kb, bb), (X1, X2, Z1, Z2, th2, Kref2, bound2, Kb2, bb2) = \
        k_reference(name, kernel, p)[:2]
    for which, got, ref in (("symmetric", sym(X, Z, th), (Kref, bound, Kb, bb)),
                            ("self", cross(X, X, Z, Z, th), (Kref, bound, Kb, bb)),
                            ("cross", cross(X1, X2, Z1, Z2, th2), (Kref2, bound2, Kb2, bb2))):
        frac = used(got["full"], ref[0], ref[1])
        fs = max(used(got["elements"][:, :, b], ref[2][b], ref[3][b]) for b in range(B))
        print(f"valu {name} {kernel} p={p} {which}: full {frac:.3g}, slices {fs:.3g} of the K bound")
        record_error(f"regime K bound used, VALU family ({which})", max(frac, fs), 1.0)
        assert frac <= 1.0 and fs <= 1.0, (which, frac, fs)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("p", [3, 20])
@pytest.mark.parametrize("name", R.MODEL_REGIMES)
def test_fused_model_meets_contract(A, name, p, kernel):
    """n = 130: two diagonal tiles, one strictly lower tile, a ragged edge."""
    n = 130
    r = referee(kernel, name, n, p, B)
    y, X, Z, th, sy = (r[k] for k in ("y", "X", "Z", "th", "sy"))
    m = A.DeviceModel(kernel, n, p, B)
    m.set_data(y, X, Z, sy)
    g, st, mu = m.para_update(1, th.copy())
    inv = m.inverse()
    m.close()
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(st)) and np.isfinite(mu)
    assert np.all(np.isfinite(inv))
    ug, us = contract_used(g, r["g"]), contract_used(st, r["st"])
    um = contract_used([mu], [r["mu"]], 1e-9)
    # the referee's gradient from the device's own inverse: what is left is
    # k_grad_mm's error (and that of the K it recomputes)
    g_own, _, _ = grad_from_inverse(kernel, y, X, Z, th, sy, inv, r["logdet"], 1, r["Kb"])
    uo = contract_used(g, g_own)
    print(f"model {name} {kernel} p={p}: gradient {ug:.3g} (referee's inverse) {uo:.3g} (own inverse), "
          f"stats {us:.3g}, mu {um:.3g} of the contract")
    record_error("regime gradient contract used (referee's inverse)", ug, 1.0)
    record_error("regime gradient contract used (device's own inverse)", uo, 1.0)
    record_error("regime stats contract used", us, 1.0)
    record_error("regime mu contract used", um, 1.0)
    assert ug <= 1.0 and uo <= 1.0 and us <= 1.0 and um <= 1.0, (ug, uo, us, um)


MEAN_Y, STD_Y, STD_Z = 0.3, 1.7, 0.8
NX = 70


@functools.lru_cache(maxsize=None)
def predict_case(name, kernel):
    """Training data of a regime (n = 130, p = 3), the oracle's inverse at
    theta, and 70 test points: one third exact copies of training rows, one
    third in range, one third training rows shifted by 50."""
    from oracle import ace_oracle as O
    n, p = 130, 3
    y, X, Z, th, sy = R.regime(name, n, p, B, 9)
    _, X2, Z2, _, _ = R.regime(name, NX, p, B, 10)
    X2 = np.array(X2, order="F")
    kind = np.arange(NX) % 3  # 0 copy, 1 in range, 2 shifted
    src = (7 * np.arange(NX)) % n
    X2[kind == 0] = X[src[kind == 0]]
    X2[kind == 2] = X[src[kind == 2]] + 50.0
    sym, cross = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    inv = O.invkernel_cpp(sym(X, Z, th)["full"], th[0])["inv"]
    th_now = th.copy()
    th_now[1] = 0.13
    alpha = inv @ (y - th_now[1])
    Kb_xX, _ = R.kernel_slices_ld(kernel, X2, X, Z2, Z, th_now)
    Kb_xx, _ = R.kernel_slices_ld(kernel, X2, X2, Z2, Z2, th_now)
    return dict(y=y, X=X, Z=Z, th=th, sy=sy, X2=X2, Z2=Z2, th_now=th_now, inv=inv, alpha=alpha,
                far=kind == 2, cross=cross(X2, X, Z2, Z, th_now), sym=sym(X2, Z2, th_now),
                Kb_xX=Kb_xX, kxx_b=np.array([np.diag(k) for k in Kb_xx]))


def _fitted(A, c, kernel):
    m = A.DeviceModel(kernel, 130, 3, B)
    m.set_data(c["y"], c["X"], c["Z"], c["sy"])
    m.para_update(2, c["th"].copy())  # the resident inverse at theta
    return m


def _far_map_slack(c, K_far, scale):
    """|map - prior mean| <= scale sum_c |K_xX,rc| |alpha_c| in exact arithmetic."""
    return scale * (np.abs(K_far) @ np.abs(c["alpha"]).astype(LD)).astype(np.float64)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["dups", "binary", "zext_m"])
def test_predict_on_copied_and_far_points(A, name, kernel):
    from oracle import ace_oracle as O
    c = predict_case(name, kernel)
    th = c["th_now"]
    m = _fitted(A, c, kernel)
    got = m.predict(th, c["X2"], c["Z2"], MEAN_Y, STD_Y)
    m.close()
    from test_gpu import close
    ref = O.pred_cpp(c["y"], th[0], th[1], c["inv"], c["cross"]["full"], c["sym"]["full"], MEAN_Y, STD_Y)
    assert all(np.all(np.isfinite(got[k])) for k in ("map", "ci", "var"))
    close(got["map"], ref["map"])
    close(got["ci"], ref["ci"], 1e-6, 1e-8)
    terms = _var_terms(O, kernel, c["X2"], c["Z2"], th, STD_Y, c["inv"], c["cross"]["full"], np.exp(th[0]))
    ev = np.max(np.abs(got["var"] - ref["var"]) / terms)
    print(f"predict {name} {kernel}: var {ev:.3g} of its terms (VAR_TOL {VAR_TOL:g})")
    record_error("regime predict var: max |err| / terms", ev, VAR_TOL)
    assert np.all(np.abs(got["var"] - ref["var"]) <= VAR_TOL * terms)
    # far test points: the posterior is the prior
    far = c["far"]
    prior_var = (STD_Y ** 2 * (c["kxx_b"].sum(axis=0)[far] + np.exp(LD(th[0])))).astype(np.float64)
    prior_map = MEAN_Y + STD_Y * th[1]
    slack = _far_map_slack(c, c["Kb_xX"].sum(axis=0)[far], STD_Y)
    print(f"predict {name} {kernel} far: var {np.max(np.abs(got['var'][far] - prior_var) / prior_var):.3g} "
          f"map {np.max(np.abs(got['map'][far] - prior_map)) / abs(prior_map):.3g} relative to the prior "
          f"(exact deviation of the map <= {slack.max() / abs(prior_map):.3g})")
    assert np.all(np.abs(got["var"][far] - prior_var) <= 1e-12 * prior_var)
    assert np.all(np.abs(got["map"][far] - prior_map) <= 1e-12 * abs(prior_map) + slack)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["dups", "binary", "zext_m"])
def test_grouped_marginal_on_copied_and_far_points(A, name, kernel):
    from oracle import ace_oracle as O
    from test_gpu import close
    c = predict_case(name, kernel)
    th = c["th_now"]
    dZ2 = c["Z2"]  # the test-side basis itself as the derivative basis: keeps its edge values
    G = 3
    label = (np.arange(NX) % 4 - 1).astype(np.int32)
    m = _fitted(A, c, kernel)
    got = m.predict_marginal_groups(th, c["X2"], dZ2, STD_Y, STD_Z, G, label)
    m.close()
    Km_xX, Km_xx = c["cross"]["elements"], c["sym"]["elements"]
    ref = O.pred_marginal_cpp(c["y"], None, th[0], th[1], c["inv"], Km_xX, Km_xx, MEAN_Y, STD_Y, STD_Z,
                              False)
    KmX = Km_xX[:, :, 1:].sum(axis=2)
    Kxx = Km_xx[:, :, 1:].sum(axis=2)
    P = KmX @ c["inv"] @ KmX.T
    assert all(np.all(np.isfinite(got[k])) for k in ("map", "ci", "var", "gsum", "gcov"))
    close(got["map"], ref["map"])
    terms = (STD_Y / STD_Z) ** 2 * (np.abs(np.diag(Kxx)) + np.abs(np.diag(P)))
    live = terms > 0
    assert np.all(got["var"][~live] == 0)
    ev = np.max(np.abs(got["var"] - ref["var"])[live] / terms[live])
    print(f"groups {name} {kernel}: var {ev:.3g} of its terms (VAR_TOL {VAR_TOL:g})")
    record_error("regime marginal var: max |err| / terms", ev, VAR_TOL)
    assert np.all(np.abs(got["var"] - ref["var"]) <= VAR_TOL * terms)
    _check_gcov(got["gcov"], dict(C=Kxx - P, Tm=np.abs(Kxx) + np.abs(P)), label, G,
                f"regime groups {name} {kernel}")
    far = c["far"]
    prior_var = ((STD_Y / STD_Z) ** 2 * c["kxx_b"][1:].sum(axis=0)[far]).astype(np.float64)
    slack = _far_map_slack(c, c["Kb_xX"][1:].sum(axis=0)[far], STD_Y / STD_Z)
    print(f"groups {name} {kernel} far: var "
          f"{np.max(np.abs(got['var'][far] - prior_var) / np.where(prior_var > 0, prior_var, 1)):.3g} "
          f"relative to the prior, |map| {np.max(np.abs(got['map'][far])):.3g} "
          f"(exact |map| <= {slack.max():.3g})")
    assert np.all(np.abs(got["var"][far] - prior_var) <= 1e-12 * prior_var)
    # (1.001: alpha above is the oracle's, the device's differs at the inverse's 1e-9)
    assert np.all(np.abs(got["map"][far]) <= 1.001 * slack)
