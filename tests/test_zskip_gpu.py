"""The pair kernels' slice skip and the zero-pattern point order (ACE_ZSKIP,
DESIGN.md §14) on the fused model.

Every case of tests/zskip_cases.py is evaluated once per setting of the
switch, in a child process each (the switch is read once per process):
  * ACE_ZSKIP=1 against 0, bit for bit: the skip changes no bit of the
    gradients, both statistics, mu, the inverse, apply_inverse or coef_cross
    -- with the carried Matern factor refreshed above a skipped slice
    (craft3), a skipped slice between two active ones (craft2), signed
    zeros, padding blocks (n = 200) and both forms of the gradient's partials;
  * ACE_ZSKIP=2 against the fp64 oracle with tests/test_gpu.py's tolerances
    (n <= 200) and against the extended-precision referee with
    tests/test_referee_gpu.py's (n = 2600);
  * ACE_ZSKIP=2 against 0 for the outputs indexed by training point
    (inverse, apply_inverse, coef_cross) in the caller's order, to the
    inverse tolerance of tests/test_gpu.py -- a missing un-permute is O(1);
  * a Z without exact zeros: ACE_ZSKIP=2 equals 0 bit for bit.
"""
import os

import numpy as np
import pytest

from conftest import golden, run_child
from test_gpu import close
from test_referee_gpu import GRAD_FLOOR, GRAD_REL, MU_TOL, STATS_TOL
import zskip_cases as ZC

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = ZC.cases()
SMALL = [c for c in CASES if c[2] <= 200]
KEYS = ("g1", "st1", "mu1", "g2", "st2", "mu2", "inv", "apply", "cross")

_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import zskip_cases as ZC
ZC.run_all({out!r})
ZC.run_referee({ref!r})
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{mode: (results of every case, results of the referee fixture)}"""
    d = tmp_path_factory.mktemp("zskip")
    out = {}
    for mode in ("0", "1", "2"):
        a, r = str(d / f"all{mode}.npz"), str(d / f"ref{mode}.npz")
        run_child(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=a, ref=r),
                  env=dict(os.environ, ACE_ZSKIP=mode), timeout=240)
        with np.load(a) as f, np.load(r) as g:
            out[mode] = ({k: f[k] for k in f.files}, {k: g[k] for k in g.files})
    return out


@pytest.fixture(scope="module")
def O():
    from oracle import ace_oracle
    return ace_oracle


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_skip_alone_is_bitwise_exact(runs, case):
    a, b = runs["0"][0], runs["1"][0]
    for k in KEYS:
        x, y = a[f"{case[0]}/{k}"], b[f"{case[0]}/{k}"]
        assert np.all(np.isfinite(x)), k
        assert np.array_equal(x, y), (k, float(np.max(np.abs(x - y))))


def test_skip_alone_is_bitwise_exact_on_referee_fixture(runs):
    a, b = runs["0"][1], runs["1"][1]
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_reordered_matches_oracle(runs, O, case):
    """test_gpu.test_model_para_update_matches_oracle's chain and bounds."""
    name, kernel, n, p, B = case[:5]
    r = runs["2"][0]
    y, X, Z, th, sy = ZC.build(case)
    sym, _, grad = O.KERNELS[kernel]
    for it in (1, 2):
        t_ref = th + 0.01 * (it - 1)
        Kl = sym(X, Z, t_ref)
        inv = O.invkernel_cpp(Kl["full"], t_ref[0])
        mu_sol = O.mu_solution_cpp(y, inv["inv"])
        if it == 1:
            t_ref[1] = mu_sol
        st_ref = np.zeros(2)
        g_ref = grad(y, X, Z, Kl["full"], Kl["elements"], inv["inv"], inv["eigenval"], t_ref,
                     st_ref, B, sy)
        mu = r[f"{name}/mu{it}"]
        assert mu[0] == pytest.approx(t_ref[1], rel=1e-8, abs=1e-12)
        assert mu[1] == pytest.approx(mu_sol, rel=1e-8)
        close(r[f"{name}/g{it}"], g_ref)
        close(r[f"{name}/st{it}"], st_ref)
        if it == 1:
            close(r[f"{name}/inv"], inv["inv"], 1e-9, 1e-9)


@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
def test_reordered_matches_referee_n2600(runs, kernel):
    """test_referee_gpu's bounds on its n = 2600 fixture (11 sweep steps)."""
    d = golden(ZC.REFEREE)
    ld = lambda key: d[key + "_hi"].astype(np.longdouble) + d[key + "_lo"]  # noqa: E731
    r = runs["2"][1]
    g_ref, st_ref, mu_ref = ld(kernel + "_g"), ld(kernel + "_st"), ld(kernel + "_mu")[0]
    err = np.abs(np.asarray(r[kernel + "/g"], dtype=np.longdouble) - g_ref)
    bound = GRAD_REL * np.abs(g_ref) + GRAD_FLOOR * np.max(np.abs(g_ref))
    print(f"{kernel}: gradient max err / bound {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound), float(np.max(err / bound))
    es = float(np.max(np.abs(np.asarray(r[kernel + "/st"], dtype=np.longdouble) - st_ref)
                      / np.abs(st_ref)))
    assert es <= STATS_TOL, es
    em = float(abs(np.longdouble(r[kernel + "/mu"][0]) - mu_ref) / abs(mu_ref))
    assert em <= MU_TOL, em


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reordered_point_indexed_outputs_come_back_in_caller_order(runs, case):
    a, b = runs["0"][0], runs["2"][0]
    for k in ("inv", "apply", "cross"):
        close(b[f"{case[0]}/{k}"], a[f"{case[0]}/{k}"], 1e-9, 1e-9)
    # and everything else to the parity tolerance (the reorder changes rounding)
    for k in ("g1", "st1", "g2", "st2"):
        close(b[f"{case[0]}/{k}"], a[f"{case[0]}/{k}"])


def test_reorder_is_the_identity_without_exact_zeros(runs):
    a, b = runs["0"][0], runs["2"][0]
    names = [c[0] for c in CASES if c[5] == "nozeros"]
    assert len(names) == 4
    for nm in names:
        for k in KEYS:
            assert np.array_equal(a[f"{nm}/{k}"], b[f"{nm}/{k}"]), (nm, k)
