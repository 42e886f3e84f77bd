"""Inputs of tests/test_zskip_gpu.py and the child script that evaluates them
under one ACE_ZSKIP setting (the switch is read once per process).  TEST
INFRASTRUCTURE ONLY.

A case is (name, kernel, n, p, B, zkind, seed).  Z kinds:
  spline     make_problem's natural-cubic-spline basis, points in random
             order (columns exactly zero on 0, 0, 1/(B-2), 2/(B-2), ...)
  sorted     the same with the points sorted by treatment, so that the GIVEN
             order already has homogeneous 64-point blocks (ACE_ZSKIP=1 skips)
  signed     `sorted` with every other exact zero written as -0.0
  nozeros    normal deviates
  scattered  normal deviates, 30 % exact zeros at random (non-nested patterns)
  craft3     Matern's carried factor: column 3 zero on the first 128 of 192
             points, columns 1 and 2 nonzero -- whole tiles skip slice 3 above
             an active slice 2
  craft2     the mirror: column 2 zero on those points, column 3 not -- a
             skipped slice between two active ones
"""
import numpy as np

from additivecausalexpansion_amd.synthetic import make_problem

NX, KV = 37, 3  # test points of coef_cross, right-hand sides of apply_inverse


def cases():
    out = []
    for kernel in ("SE", "Matern32"):
        for p in (3, 20):  # p = 20: the 4-feature tail of GEMM2 on 4x4x4 MFMAs
            for zk, B in (("spline", 6), ("sorted", 6), ("signed", 6), ("nozeros", 4),
                          ("scattered", 5)):
                out.append((f"{kernel}-p{p}-{zk}-n200", kernel, 200, p, B, zk, 11))
            # the two-buffer form of the gradient's partials (B (8 (p + 1) + 256) 8 > 40 KB)
            if p == 20:
                out.append((f"{kernel}-p20-sorted-B13-n200", kernel, 200, 20, 13, "sorted", 12))
            out.append((f"{kernel}-p{p}-craft3-n192", kernel, 192, p, 4, "craft3", 13))
            out.append((f"{kernel}-p{p}-craft2-n192", kernel, 192, p, 4, "craft2", 14))
        out.append((f"{kernel}-p3-sorted-n192", kernel, 192, 3, 6, "sorted", 15))
    # several sweep groups, a multi-tile gradient list
    out.append(("Matern32-p20-sorted-n2600", "Matern32", 2600, 20, 10, "sorted", 16))
    out.append(("SE-p3-sorted-n2600", "SE", 2600, 3, 6, "sorted", 17))
    out.append(("Matern32-p3-scattered-n2600", "Matern32", 2600, 3, 5, "scattered", 18))
    return out


def build(case):
    """(y, X, Z, theta, std_y) of a case."""
    _, _, n, p, B, zk, seed = case
    y, X, Z, th, sy = make_problem(n, p, B, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    if zk in ("sorted", "signed"):
        o = np.argsort(Z[:, 0], kind="stable")  # column 0 is the treatment
        y, X, Z = y[o], np.asfortranarray(X[o]), np.asfortranarray(Z[o])
        if zk == "signed":
            r, c = np.nonzero(Z == 0)
            Z[r[::2], c[::2]] = -0.0
    elif zk == "nozeros":
        Z = np.asfortranarray(rng.normal(size=(n, B - 1)))
    elif zk == "scattered":
        Z = rng.normal(size=(n, B - 1))
        Z[rng.random(Z.shape) < 0.3] = 0.0
        Z = np.asfortranarray(Z)
    elif zk in ("craft3", "craft2"):
        Z = rng.normal(size=(n, B - 1))
        Z[np.abs(Z) < 0.05] = 0.05
        Z[:128, 2 if zk == "craft3" else 1] = 0.0
        Z = np.asfortranarray(Z)
    elif zk != "spline":
        raise ValueError(zk)
    return y, X, Z, th, sy


def side_inputs(case):
    """(X2 for coef_cross, V for apply_inverse) of a case"""
    _, _, n, p, _, _, seed = case
    rng = np.random.default_rng(2000 + seed)
    return (np.asfortranarray(rng.uniform(-1, 1, size=(NX, p))),
            np.asfortranarray(rng.normal(size=(n, KV))))


REFEREE = "referee_p20_n2600"  # tests/golden: make_problem(2600, 20, .) in random order


def referee_inputs():
    """(fixture, y, X, Z, theta, std_y) of the n = 2600 referee fixture, as
    tests/test_referee_gpu.py regenerates them"""
    import os
    import sys
    from conftest import golden
    d = golden(REFEREE)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_referee import input_digest
    n_, p_, B_, seed = (int(v) for v in d["gen"])
    y, X, Z, th, sy = make_problem(n_, p_, B_, seed=seed)
    assert input_digest(y, X, Z, th, sy) == str(d["input_sha256"][0]), "generator drift"
    return d, y, X, Z, th, sy


def run_referee(out_path):
    """One para_update of the referee fixture per kernel under the process's
    ACE_ZSKIP."""
    import additivecausalexpansion_amd as A
    _, y, X, Z, th, sy = referee_inputs()
    res = {}
    for kernel in ("SE", "Matern32"):
        m = A.DeviceModel(kernel, X.shape[0], X.shape[1], Z.shape[1] + 1)
        m.set_data(y, X, Z, sy)
        g, st, mu = m.para_update(1, th.copy())
        m.close()
        res[kernel + "/g"], res[kernel + "/st"], res[kernel + "/mu"] = g, st, np.array([mu])
    np.savez(out_path, **res)


def run_all(out_path, names=None):
    """Evaluates every case (or those named) on the GPU under the process's
    ACE_ZSKIP and saves the results: two para_updates (gradient, statistics,
    mu), the inverse, apply_inverse and coef_cross, all in the caller's point
    order."""
    import additivecausalexpansion_amd as A
    res = {}
    for case in cases():
        name, kernel, n, p, B = case[:5]
        if names is not None and name not in names:
            continue
        y, X, Z, th, sy = build(case)
        X2, V = side_inputs(case)
        m = A.DeviceModel(kernel, n, p, B)
        m.set_data(y, X, Z, sy)
        for it in (1, 2):  # iteration 1 at theta (mu solved first), 2 at theta + 0.01
            t = th + 0.01 * (it - 1)
            g, st, mu = m.para_update(it, t)
            res[f"{name}/g{it}"], res[f"{name}/st{it}"] = g, st
            res[f"{name}/mu{it}"] = np.array([t[1], mu])
            if it == 1:
                res[f"{name}/inv"] = m.inverse()
        res[f"{name}/apply"] = m.apply_inverse(V)
        res[f"{name}/cross"] = m.coef_cross(th, X2)
        m.close()
    np.savez(out_path, **res)
