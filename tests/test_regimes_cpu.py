"""The conditions under which tests/test_regimes_gpu.py means something,
checked without a GPU.

1. The per-element K bound of tests/regimes.py (`k_bound`) is attainable by
   fp64 arithmetic: the fp64 oracle (direct differences) and a numpy fp64
   restatement of the kernels' expansion form (s_r + s_c - 2 G, clamp,
   diagonal forced) both stay inside it, in every regime, for both kernels,
   at p = 1, 3 and 20.  Measured here: at most 0.49 of the bound.
2. In every model regime the fp64 oracle's gradient, statistics and mu meet
   the project's contract (`close`: 1e-6 |ref| + 1e-9 max|ref|; mu with 1e-9
   absolute more, as tests/test_shard_gpu.py holds it for standardised y)
   against the extended-precision referee.  The regimes are therefore well
   enough conditioned that a device failure there is the device's.
"""
import numpy as np
import pytest

import regimes as R
from referee_ld import LD, _chol_inverse, _kernel_slices, grad_from_inverse, para_update_ld

SQRT3 = 1.7320508075688772
KERNELS = ["SE", "Matern32"]


def _sign(x):
    return (x > 0).astype(np.float64) - (x < 0).astype(np.float64)


def k_expansion_fp64(kernel, X1, X2, Z1, Z2, theta, sym, clamp=True):
    """K in fp64 in the MFMA family's form (csrc/ace_pairs_mm.hip): r2_b =
    s_b(r) + s_b(c) - 2 sum_i w_bi x_ri x_ci, clamped at 0 (Matern32: 1e-300),
    on the diagonal of a symmetric problem forced to 0; then the reference's
    SE sign / log|z| form or Matern32 product.  clamp=False leaves r2 as the
    expansion gives it (the mutant of test_regimes_reach_the_clamp)."""
    n1, p = X1.shape
    n2 = X2.shape[0]
    Z1 = np.asarray(Z1).reshape(n1, -1)
    Z2 = np.asarray(Z2).reshape(n2, -1)
    B = Z1.shape[1] + 1
    K = np.zeros((n1, n2))
    for b in range(B):
        w = np.exp(-theta[[1 + b + B * (i + 1) for i in range(p)]])
        s1 = (X1 * X1) @ w
        s2 = (X2 * X2) @ w
        r2 = (s1[:, None] + s2[None, :]) - 2.0 * ((X1 * w) @ X2.T)
        if clamp:
            r2 = np.maximum(r2, 0.0 if kernel == "SE" else 1e-300)
        if sym and clamp:
            np.fill_diagonal(r2, 0.0 if kernel == "SE" else 1e-300)
        z1 = Z1[:, b - 1] if b else np.ones(n1)
        z2 = Z2[:, b - 1] if b else np.ones(n2)
        if kernel == "SE":
            with np.errstate(divide="ignore", invalid="ignore"):
                k = (_sign(z1)[:, None] * _sign(z2)[None, :]) * np.exp(
                    ((theta[2 + b] - r2) + np.log(np.abs(z1))[:, None]) + np.log(np.abs(z2))[None, :])
            k[(z1 == 0)[:, None] | (z2 == 0)[None, :]] = 0.0
        else:
            with np.errstate(invalid="ignore"):
                t = np.sqrt(r2)
            k = (((1.0 + SQRT3 * t) * np.exp(theta[2 + b] - SQRT3 * t)) * z1[:, None]) * z2[None, :]
        K += k
    return K


def used(K, Kref, bound):
    """Largest |K - K_ref| / bound; where the bound is 0, K must be exactly 0."""
    K = np.asarray(K)
    assert np.all(np.isfinite(K))
    z = bound == 0
    assert np.all(K[z] == 0)
    err = np.abs(K.astype(LD) - Kref)
    return float(np.max(np.where(z, 0, err / np.where(z, 1, bound))))


def test_two_sided_slices_are_the_referees():
    _, X, Z, th, _ = R.regime("base", 40, 3, 3, 1)
    Kb, _ = R.kernel_slices_ld("Matern32", X, X, Z, Z, th)
    assert np.array_equal(Kb, _kernel_slices("Matern32", X, Z, th))


def test_regimes_are_what_they_say():
    _, X, _, _, _ = R.regime("dups", 130, 3, 3, 0)
    assert np.array_equal(X[64:128], X[:64]) and not np.array_equal(X[128], X[0])
    _, X, _, _, _ = R.regime("dups", 70, 3, 3, 0)
    assert np.array_equal(X[35:70], X[:35])
    _, Xu, _, _, _ = R.regime("neardup_ulp", 130, 3, 3, 0)
    assert np.all(Xu[64:128] != Xu[:64]) and np.all(np.abs(Xu[64:128] - Xu[:64]) <= 2.3e-16)
    _, X, _, th, _ = R.regime("binary", 130, 3, 3, 0)
    assert set(np.unique(X)) == {0.0, 1.0} and np.all(X[:, 2] == 0) and np.all(th[5:] == 0)
    _, _, Z, _, _ = R.regime("zext", 130, 3, 3, 0)
    for v in R.ZEXT + R.ZEXT_MODEL:
        Z = R.regime("zext" if v in R.ZEXT else "zext_m", 130, 3, 3, 0)[2]
        assert np.any((Z == v) & (np.signbit(Z) == np.signbit(v)))
    X1, X2, _, _, _ = R.cross_points("base", 3, 3)
    assert np.array_equal(X1[0], X2[0]) and np.array_equal(X1[2], X2[6] + 50.0)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("p", [1, 3, 20])
@pytest.mark.parametrize("name", R.REGIMES)
def test_k_bound_holds_fp64_arithmetic(name, p, kernel):
    from oracle import ace_oracle as O
    cross = O.KERNELS[kernel][1]
    _, X, Z, th, _ = R.regime(name, 70, p, 3, 5)
    cases = [(X, X, Z, Z, th, True), R.cross_points(name, p, 3) + (False,)]
    for X1, X2, Z1, Z2, t, sym in cases:
        Kref, bound = R.k_bound(kernel, X1, X2, Z1, Z2, t)
        u_or = used(cross(X1, X2, Z1, Z2, t)["full"], Kref, bound)
        u_ex = used(k_expansion_fp64(kernel, X1, X2, Z1, Z2, t, sym), Kref, bound)
        print(f"{name} {kernel} p={p} sym={sym}: oracle {u_or:.3g}, expansion {u_ex:.3g} of the K bound")
        assert u_or <= 1.0 and u_ex <= 1.0, (u_or, u_ex)


def test_regimes_reach_the_clamp():
    """Without the clamp the expansion's r2 goes negative on duplicated rows
    and Matern32's square root is NaN: `dups` would catch a kernel that lost it."""
    X1, X2, Z1, Z2, th = R.cross_points("dups", 20, 3)
    K = k_expansion_fp64("Matern32", X1, X2, Z1, Z2, th, False, clamp=False)
    assert np.any(np.isnan(K))


def contract_used(a, ref, extra_abs=0.0):
    """Fraction of `close`'s bound 1e-6 |ref| + 1e-9 max|ref| (+ extra_abs) used."""
    a = np.asarray(a, dtype=LD).ravel()
    ref = np.asarray(ref, dtype=LD).ravel()
    assert np.all(np.isfinite(a.astype(np.float64)))
    bound = LD(1e-6) * np.abs(ref) + LD(1e-9) * np.max(np.abs(ref)) + LD(extra_abs)
    return float(np.max(np.abs(a - ref) / bound))


_REF = {}


def referee(kernel, name, n, p, B, seed=9):
    """One regime's problem and its para_update_ld (iteration 1) with the
    pieces grad_from_inverse needs (the slices Kb, A^-1, log det A), computed once
    and shared; never modified."""
    key = (kernel, name, n, p, B, seed)
    if key not in _REF:
        y, X, Z, th, sy = R.regime(name, n, p, B, seed)
        Kb = _kernel_slices(kernel, X, Z, th)
        A = Kb.sum(axis=0) + np.exp(LD(th[0])) * np.eye(n, dtype=LD)
        inv, logdet = _chol_inverse(A)
        g, st, mu = grad_from_inverse(kernel, y, X, Z, th, sy, inv, logdet, 1, Kb)
        _REF[key] = dict(y=y, X=X, Z=Z, th=th, sy=sy, Kb=Kb, inv=inv, logdet=logdet, g=g, st=st, mu=mu)
    return _REF[key]


def test_shared_referee_is_para_update_ld():
    r = referee("SE", "base", 130, 3, 3)
    g, st, mu = para_update_ld("SE", r["y"], r["X"], r["Z"], r["th"], r["sy"])
    assert np.array_equal(g, r["g"]) and np.array_equal(st, r["st"]) and mu == r["mu"]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", R.MODEL_REGIMES)
def test_oracle_meets_contract_in_every_model_regime(name, kernel):
    from oracle import ace_oracle as O
    n, p, B = 130, 3, 3
    r = referee(kernel, name, n, p, B)
    y, X, Z, th, sy, g_ref, st_ref, mu_ref = (r[k] for k in ("y", "X", "Z", "th", "sy", "g", "st", "mu"))
    sym, _, grad = O.KERNELS[kernel]
    t = th.copy()
    K = sym(X, Z, t)
    inv = O.invkernel_cpp(K["full"], t[0])
    t[1] = O.mu_solution_cpp(y, inv["inv"])
    st = np.zeros(2)
    g = grad(y, X, Z, K["full"], K["elements"], inv["inv"], inv["eigenval"], t, st, B, sy)
    ug, us = contract_used(g, g_ref), contract_used(st, st_ref)
    um = contract_used([t[1]], [mu_ref], 1e-9)
    print(f"{name} {kernel}: oracle uses {ug:.3g} (gradient) {us:.3g} (stats) {um:.3g} (mu) of the contract")
    assert max(ug, us, um) <= 1.0
