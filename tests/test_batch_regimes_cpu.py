"""The conditions under which tests/test_batch_regimes_gpu.py and the
not-positive-definite cases of tests/test_batch_gpu.py mean something, checked
without a GPU.

1. For every (kernel, regime, p) that goes through k_batch_eval against the
   referee (batch_cases.REGIME_CASES, n = 130, B = 3), fp64 arithmetic meets
   the tight bound the device is held to: the fp64 oracle chain, and the
   referee's formulas fed with the inverse and log-determinant of a pivot-free
   fp64 Gauss-Jordan sweep (the batch kernel's algorithm at block width 1),
   each use at most CPU_CAP of the contract for gradient, stats and mu.
   CPU_CAP is three times the worst fraction this file prints.
2. The singular models of batch_cases.singular_cases are singular by
   construction, not by rounding: the chosen row of the fp64 oracle's
   K + e^theta0 I is exactly zero, diagonal included, and everything else of
   the model is the healthy model's.
"""
import numpy as np
import pytest

import batch_cases as C
from referee_ld import grad_from_inverse
from test_regimes_cpu import contract_used, referee

KERNELS = ["SE", "Matern32"]
CASES = [(p, name) for p, names in C.REGIME_CASES for name in names]


def test_gauss_jordan_fp64_inverts():
    rng = np.random.default_rng(3)
    G = rng.normal(size=(37, 37))
    A = G @ G.T + 37 * np.eye(37)
    inv, logdet = C.gauss_jordan_fp64(A)
    assert np.allclose(inv @ A, np.eye(37), rtol=0, atol=1e-12)
    assert np.allclose(inv, inv.T, rtol=1e-12, atol=0)
    assert logdet == pytest.approx(np.linalg.slogdet(A)[1], rel=1e-13)


def test_cpu_cap_is_three_times_the_worst_measured():
    assert C.CPU_CAP == 3 * C.CPU_WORST and C.TIGHT == 10 * C.CPU_CAP
    assert 3e-4 <= C.CPU_CAP <= 3e-3  # "near 1e-3": far below the contract's 1.0


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("p,name", CASES)
def test_fp64_of_the_batch_kernels_form_meets_the_tight_bound(p, name, kernel):
    from oracle import ace_oracle as O
    r = referee(kernel, name, C.N_REG, p, C.B_REG)
    y, X, Z, th, sy, g_ref, st_ref, mu_ref = (r[k] for k in ("y", "X", "Z", "th", "sy", "g", "st", "mu"))
    sym, _, grad = O.KERNELS[kernel]
    t = th.copy()
    K = sym(X, Z, t)
    inv = O.invkernel_cpp(K["full"], t[0])
    t[1] = O.mu_solution_cpp(y, inv["inv"])
    st = np.zeros(2)
    g = grad(y, X, Z, K["full"], K["elements"], inv["inv"], inv["eigenval"], t, st, C.B_REG, sy)
    orc = (contract_used(g, g_ref), contract_used(st, st_ref), contract_used([t[1]], [mu_ref], 1e-9))
    # the batch kernel's inverse and log-determinant in fp64, the rest the referee's
    A = np.array(K["full"])
    A[np.diag_indices_from(A)] += np.exp(th[0])
    inv_gj, logdet_gj = C.gauss_jordan_fp64(A)
    g2, st2, mu2 = grad_from_inverse(kernel, y, X, Z, th, sy, inv_gj, logdet_gj, 1, r["Kb"])
    gj = (contract_used(g2, g_ref), contract_used(st2, st_ref), contract_used([mu2], [mu_ref], 1e-9))
    ui = contract_used(inv_gj, r["inv"])
    print(f"batch cpu {name} {kernel} p={p}: oracle {orc[0]:.3g} {orc[1]:.3g} {orc[2]:.3g}, "
          f"gauss-jordan {gj[0]:.3g} {gj[1]:.3g} {gj[2]:.3g} (gradient, stats, mu), "
          f"gauss-jordan inverse {ui:.3g} of the contract; worst {max(orc + gj):.3g}")
    assert max(orc + gj) <= C.CPU_CAP, (orc, gj)
    assert ui <= 1.0


@pytest.mark.parametrize("kernel", KERNELS)
def test_singular_models_are_singular_by_construction(kernel):
    from oracle import ace_oracle as O
    sym = O.KERNELS[kernel][0]
    for (y, X, Z, th, sy), (ys, Xs, Zs, ths, sys_), ths2, row in C.singular_cases():
        assert ths is ths2
        A = np.array(sym(Xs, Zs, ths)["full"], dtype=np.float64)
        A[np.diag_indices_from(A)] += np.exp(ths[0])
        assert np.exp(ths[0]) == 0.0
        assert np.all(A[row, :] == 0.0) and np.all(A[:, row] == 0.0) and A[row, row] == 0.0
        other = np.delete(np.arange(y.size), row)
        assert np.all(np.diag(A)[other] > 0.0)  # no other row is dead
        # everything else is the healthy model
        assert np.array_equal(ys, y) and np.array_equal(Xs, X) and sys_ == sy
        assert np.array_equal(Zs[other], Z[other]) and np.all(Zs[row] == 0.0) and np.any(Z[row] != 0.0)
        keep = np.delete(np.arange(th.size), [0, 2])
        assert np.array_equal(ths[keep], th[keep]) and ths[0] == -2000.0 and ths[2] == -2000.0
