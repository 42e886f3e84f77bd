"""The batched engine (k_batch_eval: its own kernel evaluation, its 16-wide
pivot-free Gauss-Jordan sweep, its gradient pass) in the input regimes of
tests/regimes.py against the extended-precision referee.

One BatchModel per (kernel, p) of batch_cases.REGIME_CASES with B = 3 and
n = 130 (nine 16-blocks, the last ragged, plus the right-hand-side block);
each of its models is one model regime.  Per model, after para_update(1, .):
  * everything is finite;
  * gradient, stats and mu use at most 1.0 of the project's contract
    (test_regimes_cpu.contract_used; mu with 1e-9 absolute more), and at most
    TIGHT = 10 CPU_CAP of it: CPU_CAP is what fp64 arithmetic of the kernel's
    form needs (tests/test_batch_regimes_cpu.py), the factor 10 allows for the
    device's exp / log / sqrt, fma contraction and the blocked accumulation
    order.  The contract alone leaves four orders of magnitude over what fp64
    needs here and would not notice a kernel that is subtly wrong;
  * the gradient against the referee's gradient evaluated with the model's own
    inverse (which isolates the gradient pass and the K it recomputes from the
    sweep's error), under the same two bounds;
  * the inverse against the referee's under the contract.
Bitwise: a model alone equals itself inside the thirteen-model batch; with
slice 0 switched off the zext_m model's exact zeros leave everything finite.
"""
import numpy as np
import pytest

import batch_cases as C
import regimes as R
from conftest import record_error
from referee_ld import grad_from_inverse
from test_regimes_cpu import contract_used, referee

pytestmark = pytest.mark.gpu

KERNELS = ["SE", "Matern32"]
N, B = C.N_REG, C.B_REG
NAMES = dict(C.REGIME_CASES)
CASES = [(p, name) for p, names in C.REGIME_CASES for name in names]


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.default_context()
    return pkg


def _run(A, kernel, p, names, thetas=None):
    bm = A.BatchModel(kernel, len(names), N, p, B)
    rs = [referee(kernel, name, N, p, B) for name in names]
    for j, r in enumerate(rs):
        bm.set_data(j, r["y"], r["X"], r["Z"], r["sy"])
    th = np.asfortranarray(np.column_stack([r["th"] for r in rs] if thetas is None else thetas))
    g, st, mu = bm.para_update(1, th)
    invs = [bm.inverse(j) for j in range(len(names))]
    bm.close()
    return th, g, st, mu, invs


_runs = {}


def batch_run(A, kernel, p):
    """para_update(1, .) of the (kernel, p) batch, run once and shared; never modified."""
    if (kernel, p) not in _runs:
        _runs[(kernel, p)] = _run(A, kernel, p, NAMES[p])
    return _runs[(kernel, p)]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("p,name", CASES)
def test_batch_model_meets_contract_and_tight_bound(A, p, name, kernel):
    j = NAMES[p].index(name)
    th, g, st, mu, invs = batch_run(A, kernel, p)
    g, st, mu, inv = g[:, j], st[:, j], mu[j], invs[j]
    r = referee(kernel, name, N, p, B)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(st)) and np.isfinite(mu)
    assert np.all(np.isfinite(inv)) and th[1, j] == mu
    ug, us = contract_used(g, r["g"]), contract_used(st, r["st"])
    um = contract_used([mu], [r["mu"]], 1e-9)
    g_own, _, _ = grad_from_inverse(kernel, r["y"], r["X"], r["Z"], r["th"], r["sy"], inv, r["logdet"], 1,
                                    r["Kb"])
    uo = contract_used(g, g_own)
    ui = contract_used(inv, r["inv"])
    print(f"batch regime {name} {kernel} p={p}: gradient {ug:.3g} (referee's inverse) {uo:.3g} (own "
          f"inverse), stats {us:.3g}, mu {um:.3g}, inverse {ui:.3g} of the contract (tight bound "
          f"{C.TIGHT:.3g})")
    for what, u in (("gradient (referee's inverse)", ug), ("gradient (own inverse)", uo), ("stats", us),
                    ("mu", um)):
        record_error(f"batch regime {what} contract used, {kernel}", u, 1.0)
        record_error(f"batch regime {what} tight bound used, {kernel}", u / C.TIGHT, 1.0)
    record_error(f"batch regime inverse contract used, {kernel}", ui, 1.0)
    assert max(ug, uo, us, um, ui) <= 1.0, (ug, uo, us, um, ui)
    assert max(ug, uo, us, um) <= C.TIGHT, (ug, uo, us, um)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("p", [3, 40])
@pytest.mark.parametrize("name", ["zext_m", "dups"])
def test_batch_regime_model_alone_is_bitwise_the_batched_one(A, name, p, kernel):
    j = NAMES[p].index(name)
    th, g, st, mu, invs = batch_run(A, kernel, p)
    th1, g1, st1, mu1, inv1 = _run(A, kernel, p, [name])
    assert np.array_equal(g1[:, 0], g[:, j]) and np.array_equal(st1[:, 0], st[:, j])
    assert mu1[0] == mu[j] and np.array_equal(th1[:, 0], th[:, j])
    assert np.array_equal(inv1[0], invs[j])


@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_zext_m_with_slice_0_off_stays_finite(A, kernel):
    """exp(-2000 - r2) is 0 in fp64: A is the z slices plus 0.1 I, and the z
    slices are exactly 0 on the rows and columns of a z of +-0."""
    r = referee(kernel, "zext_m", N, 3, B)
    th = r["th"].copy()
    assert abs(th[0] - np.log(0.1)) < 1e-15
    th[2] = -2000.0
    _, g, st, mu, invs = _run(A, kernel, 3, ["zext_m"], thetas=[th])
    assert np.all(np.isfinite(invs[0])) and np.all(np.isfinite(g)) and invs[0].shape == (N, N)
