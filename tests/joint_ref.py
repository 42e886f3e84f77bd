"""The numpy referee of the joint posterior at the test points
(ace_model_predict_joint): the matrix pred_cpp / pred_marginal_cpp form in
full before they take diag() (src/pred_cpp.cpp:22, :72), from the oracle's
kernel functions and invkernel_cpp; the factor is numpy.linalg.cholesky and
the draws are m + L Xi.  Shared by tests/test_joint_cpu.py (which checks the
referee against the oracle and the inputs' definiteness) and
tests/test_joint_gpu.py; every state is computed once and never modified."""
import functools

import numpy as np

MEAN_Y, STD_Y, STD_Z = 0.3, 1.7, 0.8
U = 2.0 ** -53

# n, p, B, nx, seed of the problem, seed of the test points: the states of
# tests/test_predict_gpu.py (_fit_state's recipe)
CASES = {
    "300/70": (300, 3, 5, 70, 300, 301),
    "700/257": (700, 20, 10, 257, 700, 701),   # four full 64-tiles and a ragged one; PM = 20
    "130/9": (130, 1, 1, 9, 130, 131),         # less than one tile; B = 1 marginal
    "400/150": (400, 3, 6, 150, 11, 77),
}

# Measured on an MI355X against this referee (profiles/joint_error_table.txt):
# the largest |cov - ref| / terms over all states was 5.2e-10 (Matern32 400/150,
# with noise); the bound is 2.9x that, the bound the diagonal already has
# (VAR_TOL of tests/test_predict_gpu.py, the same cancellation).
COV_TOL = 1.5e-9
# The factor's residual against gamma_{nx+1} sqrt(c'_ii c'_jj): the largest
# ratio measured was 0.23 (Matern32 130/9), so Higham's bound holds as it
# stands, margin c = 1.
FACTOR_MARGIN = 1.0


def gamma(k):
    return k * U / (1.0 - k * U)


def jitter_of(kernel, marginal):
    """The jitter of the factor tests: the SE marginal covariance's smallest
    eigenvalue reaches 5e-13, below the rounding of C itself."""
    return 1e-5 if (marginal and kernel == "SE") else 0.0


@functools.lru_cache(maxsize=None)
def problem(case, kernel, mix=False):
    """_fit_state's recipe without the device: data, theta_{T-1} (the
    inverse's), theta_T (the kernels'), the oracle's inverse, test points and
    the stand-in derivative basis."""
    from additivecausalexpansion_amd.synthetic import make_problem
    from oracle import ace_oracle as O
    n, p, B, nx, seed, seed2 = CASES[case]
    y, X, Z, th, sy = make_problem(n, p, B, seed=seed)
    th_now = th + 0.02 if mix else th.copy()
    th_now[1] = 0.13
    inv = O.invkernel_cpp(O.KERNELS[kernel][0](X, Z, th)["full"], th[0])["inv"]
    _, X2, Z2, _, _ = make_problem(nx, p, B, seed=seed2)
    dZ2 = np.asfortranarray(Z2 * 0.7 + 0.1)
    out = dict(n=n, p=p, B=B, nx=nx, y=y, X=X, Z=Z, th_prev=th, th=th_now, sy=sy, inv=inv,
               X2=X2, Z2=Z2, dZ2=dZ2)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def joint(case, kernel, marginal, mix=False, noise=True):
    """map, cov and the size of the cancelled terms (the Cauchy-Schwarz bound
    |K_xx|_ij + sqrt(q_i q_j) [+ e^sigma on the diagonal], scaled), plus the
    oracle's own pred_cpp / pred_marginal_cpp output."""
    from oracle import ace_oracle as O
    s = problem(case, kernel, mix)
    sym, cross = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    th, inv, y, B = s["th"], s["inv"], s["y"], s["B"]
    if not marginal:
        K_xX = cross(s["X2"], s["X"], s["Z2"], s["Z"], th)["full"]
        K_xx = sym(s["X2"], s["Z2"], th)["full"]
        orc = O.pred_cpp(y, th[0], th[1], inv, K_xX, K_xx, MEAN_Y, STD_Y)
        es = np.exp(th[0]) if noise else 0.0
        scale = STD_Y
        tmp = K_xX @ inv
        mp = MEAN_Y + STD_Y * (tmp @ (np.ravel(y) - th[1]) + th[1])
    else:
        Ke_xX = cross(s["X2"], s["X"], s["dZ2"], s["Z"], th)["elements"]
        Ke_xx = sym(s["X2"], s["dZ2"], th)["elements"]
        zx = (np.arange(s["nx"]) % 3 == 0).astype(float)
        orc = O.pred_marginal_cpp(y, zx, th[0], th[1], inv, Ke_xX, Ke_xx, MEAN_Y, STD_Y, STD_Z,
                                  False)
        sl = slice(1, B) if B > 1 else slice(0, 1)
        K_xX = Ke_xX[:, :, sl].sum(axis=2)
        K_xx = Ke_xx[:, :, sl].sum(axis=2)
        es = 0.0
        scale = STD_Y / STD_Z
        tmp = K_xX @ inv
        mp = STD_Y * (tmp @ (np.ravel(y) - th[1])) / STD_Z
    Kp = K_xx - tmp @ K_xX.T
    nx = s["nx"]
    cov = scale ** 2 * (Kp + es * np.eye(nx))
    q = np.abs(np.sum(tmp * K_xX, axis=1))
    terms = scale ** 2 * (np.abs(K_xx) + np.sqrt(np.outer(q, q)) + es * np.eye(nx))
    out = dict(map=mp, cov=cov, terms=terms, oracle=orc, scale=scale, es=es)
    for v in (mp, cov, terms):
        v.setflags(write=False)
    return out


def factor(cov, jitter=0.0):
    return np.linalg.cholesky(cov + jitter * np.eye(cov.shape[0]))


def draws(mp, L, xi):
    return mp[:, None] + L @ xi


def factor_residual_ratio(L, A):
    """max over i >= j of |L L^T - A|_ij / (gamma_{n+1} sqrt(a_ii a_jj)), the
    product in long double from the given L and A (Higham, Accuracy and
    Stability of Numerical Algorithms, Theorem 10.3 with |L||L^T|_ij <=
    sqrt(a_ii a_jj) / (1 - gamma_{n+1}))."""
    n = A.shape[0]
    Ll = L.astype(np.longdouble)
    R = np.abs(Ll @ Ll.T - A.astype(np.longdouble))
    d = np.sqrt(np.diag(A).astype(np.longdouble))
    # (the factor reads A's lower triangle)
    return float(np.max(np.tril(R / (gamma(n + 1) * np.outer(d, d)))))
