"""GPU tests of the two-sided 64 x 64 tile that k_cross_mm, k_cross_slices_mm
and k_group_mm share (ace_pairs_mm.hip), at the smallest shapes where its
pieces take different paths: ragged tile edges on both sides, the row operand
in registers (PM <= 32) and read through a pointer (PM = 48), no basis rows
staged (B = 1) and the fewest (B = 2), one and two blocks of group columns,
and dynamic LDS above 64 KB (the launch's attribute path).

Slice 0 of the slice kernel is held bit for bit against the cross kernel:
with a test basis of zeros every later slice of ace_kernmat_cross adds a zero
of either sign to slice 0 (SE selects 0 for z = 0, Matern's product is 0), so
its sum is slice 0 as k_cross_mm forms it, 0 + k_0 with z = 1, log|z| = 0 on
both sides -- the slice kernel's expression.  Both are also held to the
oracle, so the shared tile cannot be wrong in both the same way unnoticed.
The grouped sums use test_robust_gpu's oracle helper and COV_TOL.
"""
import numpy as np

import pytest
from test_gpu import close
from test_predict_gpu import _fit_state
from test_robust_gpu import COV_TOL, STD_Y, STD_Z, _check_gcov, _labels, case

pytestmark = pytest.mark.gpu

# (kernel, n, p, B, nx): p = 3 -> PM = 4, p = 40 -> PM = 48, p = 50 -> PM = 64
CROSS_CASES = [
    ("SE", 70, 3, 2, 65), ("Matern32", 70, 3, 2, 65),     # RowX in registers, ragged both ways
    ("SE", 130, 40, 1, 9), ("Matern32", 130, 40, 1, 9),   # RowX from a pointer, no Z rows
    ("SE", 130, 40, 2, 9), ("Matern32", 70, 3, 1, 65),    # the other B of each
    ("SE", 70, 50, 32, 65),                               # 145 KB of dynamic LDS
]


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.default_context()
    return pkg


@pytest.fixture(scope="module")
def O():
    from oracle import ace_oracle
    return ace_oracle


@pytest.mark.parametrize("kernel,n,p,B,nx", CROSS_CASES)
def test_slice_zero_is_the_cross_kernel_bit_for_bit(A, O, kernel, n, p, B, nx):
    from additivecausalexpansion_amd import native
    from additivecausalexpansion_amd._lib import KIND
    from additivecausalexpansion_amd.synthetic import make_problem
    m, y, X, Z, th, sy, inv = _fit_state(O, kernel, n, p, B, seed=n + p, A=A)
    th[2 + B:] += np.log(3.0 / p)  # r2 of order 1 at every p: the kernels far from underflow
    _, X2, _, _, _ = make_problem(nx, p, B, seed=n + p + 1)
    Kc = m.coef_cross(th, X2)
    assert Kc.shape == (nx, n, B)
    ones = np.ones((nx, B - 1), order="F")
    close(Kc, O.KERNELS[kernel][1](X2, X, ones, Z, th)["elements"])
    zeros = np.zeros((nx, B - 1), order="F")
    full = native._kernmat_cross(KIND[kernel], X2, X, zeros, Z, th, elements=False)["full"]
    assert np.array_equal(Kc[:, :, 0], full)
    # and with the basis factors on both sides, the cross kernel's own sum
    _, _, Z2, _, _ = make_problem(nx, p, B, seed=n + p + 1)
    full = native._kernmat_cross(KIND[kernel], X2, X, Z2, Z, th, elements=False)["full"]
    close(full, O.KERNELS[kernel][1](X2, X, Z2, Z, th)["full"])


@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
@pytest.mark.parametrize("p,G", [(3, 1), (3, 17), (40, 17)])
def test_grouped_sums_one_and_two_column_blocks(A, O, kernel, p, G):
    """G = 1 (one block of 16 group columns) and G = 17 (two) on 130 points:
    two full tiles and a 2-point edge on both sides of the square."""
    n, B, nx = 130, 2, 130
    c = case(A, O, kernel, n, p, B, nx)
    label = _labels(nx, G)
    got = c["m"].predict_marginal_groups(c["th"], c["X2"], c["dZ2"], STD_Y, STD_Z, G, label)
    _check_gcov(got["gcov"], c, label, G, f"cross tile groups {kernel} p={p} G={G}")
    again = c["m"].predict_marginal_groups(c["th"], c["X2"], c["dZ2"], STD_Y, STD_Z, G, label)
    assert np.array_equal(got["gcov"], again["gcov"])
