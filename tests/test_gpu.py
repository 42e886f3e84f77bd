"""GPU parity tests: every C-ABI entry point against the oracle, on the
committed golden fixtures and on live oracle runs, plus size-independent
properties at larger n.  All calls go through libace_hip.so (the HIP path);
there is no fallback.

Tolerances (north_star: "within 1e-6 relative fp64"):
  * assembly (pure pair arithmetic, FMA vs separate mul/add and ocml vs
    glibc exp/log/sqrt): |K - K_ref| <= 1e-12 * max|K_ref|
  * inverse (Gauss-Jordan sweep vs eigendecomposition, ~cond * eps):
    |inv - inv_ref| <= 1e-9 * max|inv_ref|
  * gradients, stats, predictions: |v - v_ref| <= 1e-6 |v_ref| + 1e-9 max|v_ref|
"""
import math

import numpy as np

from conftest import run_child
import pytest
from conftest import golden, golden_names, record_error

pytestmark = pytest.mark.gpu

RTOL = 1e-6


def close(a, b, rtol=RTOL, atol_rel=1e-9, check="close"):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    scale = np.abs(b).max() if b.size else 0.0
    bound = rtol * np.abs(b) + atol_rel * scale
    ok = np.abs(a - b) <= bound
    if b.size and np.all(np.isfinite(a)) and np.all(np.isfinite(b)):
        # the fraction of the bound the worst element uses (1 = at the bound)
        with np.errstate(divide="ignore", invalid="ignore"):
            use = np.where(bound > 0, np.abs(a - b) / bound, np.where(a == b, 0.0, np.inf))
        record_error(f"{check} (rtol {rtol:g}, atol {atol_rel:g} max|ref|): bound used",
                     float(use.max()), 1.0)
    if not np.all(ok):
        i = np.argmax(np.abs(a - b) - rtol * np.abs(b))
        raise AssertionError(f"mismatch at {np.unravel_index(i, b.shape)}: {a.flat[i]} vs "
                             f"{b.flat[i]} (max abs err {np.abs(a - b).max():.3e}, scale {scale:.3e})")


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.default_context()
    return pkg


@pytest.fixture(scope="module")
def O():
    from oracle import ace_oracle
    return ace_oracle


def kern_fns(A, kernel):
    if kernel == "SE":
        return A.kernmat_SE_symmetric_cpp, A.kernmat_SE_cpp, A.grad_SE_cpp
    return A.kernmat_Matern32_symmetric_cpp, A.kernmat_Matern32_cpp, A.grad_Matern_cpp


# ------------------------------------------------------------------ MFMA layout
def test_gemm_mfma_layout_asymmetric(A):
    """A=I and asymmetric B through the MFMA GEMM (pred_cpp's tmp = K_xX inv):
    catches a transposed C/D fragment map."""
    rng = np.random.default_rng(0)
    nX, nx = 37, 150
    Bm = rng.normal(size=(nX, nX))
    inv = Bm  # not symmetric on purpose
    KxX = rng.normal(size=(nx, nX))
    y = rng.normal(size=nX)
    out = A.pred_cpp(y, -1.0, 0.2, inv, KxX, np.eye(nx) * 3.0, 0.5, 2.0)
    tmp = KxX @ inv
    close(out["map"], 0.5 + 2.0 * (tmp @ (y - 0.2) + 0.2), 1e-12, 1e-12)
    d = 3.0 - np.sum(tmp * KxX, axis=1) + math.exp(-1.0)
    close(out["var"], (2.0 * np.sqrt(np.abs(d))) ** 2, 1e-11, 1e-12)


# ------------------------------------------------------------------ assembly
@pytest.mark.parametrize("name", golden_names("asm_"))
def test_assembly_golden(A, name):
    d = golden(name)
    kernel = "SE" if "_SE_" in name else "Matern32"
    sym, cross, _ = kern_fns(A, kernel)
    ks = sym(d["X"], d["Z"], d["theta"])
    close(ks["full"], d["sym_full"], 1e-12, 1e-12)
    assert np.array_equal(ks["full"], ks["full"].T)  # mirrored exactly
    kc = cross(d["X2"], d["X"], d["Z2"], d["Z"], d["theta"])
    close(kc["full"], d["cross_full"], 1e-12, 1e-12)
    if "sym_elements" in d:
        close(ks["elements"], d["sym_elements"], 1e-12, 1e-12)
        close(kc["elements"], d["cross_elements"], 1e-12, 1e-12)
        # exact zeros of the basis give exact zeros (Q7 branch)
        zr = d["Z"] == 0
        for b in range(1, ks["elements"].shape[2]):
            assert np.all(ks["elements"][zr[:, b - 1], :, b] == 0)


@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
@pytest.mark.parametrize("p", [1, 4, 8, 11, 20, 23, 31, 40, 57, 64])
def test_assembly_every_feature_bucket(A, O, kernel, p):
    rng = np.random.default_rng(p)
    n, B = 70, 3
    X = rng.uniform(-1, 1, (n, p))
    Z = rng.normal(size=(n, B - 1))
    Z[rng.random((n, B - 1)) < 0.3] = 0
    th = np.concatenate([[-1.0, 0.0], rng.normal(0, .3, B), rng.normal(1.0, .3, B * p)])
    sym = kern_fns(A, kernel)[0]
    close(sym(X, Z, th)["full"], O.KERNELS[kernel][0](X, Z, th)["full"], 1e-12, 1e-12)


@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
@pytest.mark.parametrize("p,B", [(50, 16), (64, 32), (20, 10)])
def test_assembly_large_shapes_cube_and_cross(A, O, kernel, p, B):
    """Symmetric and cross kernels with their n x n x B cubes at the largest
    feature / basis counts (the ABI modes run the all-VALU assembly)."""
    rng = np.random.default_rng(p + B)
    n1, n2 = 70, 45
    X1, X2 = rng.uniform(-1, 1, (n1, p)), rng.uniform(-1, 1, (n2, p))
    Z1, Z2 = rng.normal(size=(n1, B - 1)), rng.normal(size=(n2, B - 1))
    Z1[rng.random((n1, B - 1)) < 0.3] = 0
    Z2[rng.random((n2, B - 1)) < 0.3] = 0
    th = np.concatenate([[-1.0, 0.0], rng.normal(0, .3, B), rng.normal(2.5, .3, B * p)])
    sym, cross, _ = kern_fns(A, kernel)
    osym, ocross = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    r, ref = sym(X1, Z1, th), osym(X1, Z1, th)
    close(r["full"], ref["full"], 1e-12, 1e-12)
    close(r["elements"], ref["elements"], 1e-12, 1e-12)
    r, ref = cross(X1, X2, Z1, Z2, th), ocross(X1, X2, Z1, Z2, th)
    close(r["full"], ref["full"], 1e-12, 1e-12)
    close(r["elements"], ref["elements"], 1e-12, 1e-12)


def test_assembly_unsupported_shape_raises(A):
    with pytest.raises(A.AceError):
        A.kernmat_SE_symmetric_cpp(np.zeros((5, 65)), np.zeros((5, 1)), np.zeros(2 + 2 * 66))


# ------------------------------------------------------------------ inverse
@pytest.mark.parametrize("name", golden_names("grad_"))
def test_invkernel_golden(A, name):
    d = golden(name)
    r = A.invkernel_cpp(d["Kfull"], d["theta"][0])
    close(r["inv"], d["inv"], 1e-9, 1e-9)
    assert np.sum(np.log(r["eigenval"])) == pytest.approx(float(d["logdet"]), rel=1e-10, abs=1e-9)


@pytest.mark.parametrize("n", [1, 2, 63, 255, 256, 257, 700, 1500])
def test_invkernel_sizes(A, O, n):
    """Edge sizes around the 64/128/256 blockings (padding + AUG rows)."""
    from additivecausalexpansion_amd.synthetic import make_problem
    y, X, Z, th, _ = make_problem(max(n, 3), 3, 4, seed=n)
    X, Z = X[:n], Z[:n]
    K = O.kernmat_SE_symmetric_cpp(X, Z, th)["full"]
    r = A.invkernel_cpp(K, th[0])
    ref = O.invkernel_cpp(K, th[0])
    close(r["inv"], ref["inv"], 1e-9, 1e-9)
    assert np.sum(np.log(r["eigenval"])) == pytest.approx(np.sum(np.log(ref["eigenval"])),
                                                          rel=1e-10, abs=1e-9)


def test_invkernel_not_positive_definite_gives_nan(A):
    K = -np.eye(10)
    r = A.invkernel_cpp(K, -5.0)
    assert np.all(np.isnan(r["inv"]))
    assert np.any(r["eigenval"] <= 0)


# ------------------------------------------------------------------ gradient + stats
@pytest.mark.parametrize("name", golden_names("grad_"))
@pytest.mark.parametrize("with_cube", [True, False])
def test_grad_golden(A, O, name, with_cube):
    d = golden(name)
    kernel = "SE" if "_SE_" in name else "Matern32"
    sym, _, grad = kern_fns(A, kernel)
    B = d["Z"].shape[1] + 1
    cube = O.KERNELS[kernel][0](d["X"], d["Z"], d["theta"])["elements"] if with_cube else None
    ev = np.exp(np.full(d["y"].shape[0], float(d["logdet"]) / d["y"].shape[0]))
    stats = np.zeros(2)
    g = grad(d["y"], d["X"], d["Z"], d["Kfull"], cube, d["inv"], ev, d["theta"], stats, B,
             float(d["std_y"]))
    close(g, d["grad"])
    close(stats, d["stats"])
    st2 = A.stats_cpp(d["y"], d["Kfull"], d["inv"], ev, d["theta"][1], float(d["std_y"]))
    close(st2, d["stats_cpp"])
    assert A.mu_solution_cpp(d["y"], d["inv"]) == pytest.approx(float(d["mu"]), rel=1e-9)


@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
@pytest.mark.parametrize("p", [48, 64])
@pytest.mark.parametrize("with_cube", [True, False])
def test_grad_abi_large_p(A, O, kernel, p, with_cube):
    """ABI gradient at the largest feature buckets, with and without the K
    cube (above PM = 48 the MFMA kernel recomputes K_b instead of reading the
    cube; the all-VALU kernels are only used up to PM = 48)."""
    from additivecausalexpansion_amd.synthetic import make_problem
    n, B = 150, 5
    y, X, Z, th, sy = make_problem(n, p, B, seed=11)
    sym, _, grad = O.KERNELS[kernel]
    Kl = sym(X, Z, th)
    inv = O.invkernel_cpp(Kl["full"], th[0])
    st_ref = np.zeros(2)
    g_ref = grad(y, X, Z, Kl["full"], Kl["elements"], inv["inv"], inv["eigenval"], th.copy(),
                 st_ref, B, sy)
    _, _, gdev = kern_fns(A, kernel)
    st = np.zeros(2)
    g = gdev(y, X, Z, Kl["full"], Kl["elements"] if with_cube else None, inv["inv"],
             inv["eigenval"], th.copy(), st, B, sy)
    close(g, g_ref)
    close(st, st_ref)


# ------------------------------------------------------------------ prediction
@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
def test_pred_golden(A, kernel):
    d = golden(f"pred_{kernel}")
    th = d["theta"]
    pr = A.pred_cpp(d["y"], th[0], th[1], d["inv"], d["K_xX"], d["K_xx"], 0.3, 1.9)
    close(pr["map"], d["map"])
    close(pr["var"], d["var"])
    close(pr["ci"], d["ci"])
    pm = A.pred_marginal_cpp(d["y"], d["Z2"], th[0], th[1], d["inv"], d["cube_xX"], d["cube_xx"],
                             0.3, 1.9, 0.8, True)
    close(pm["map"], d["m_map"])
    close(pm["var"], d["m_var"])
    got = np.concatenate([[pm[k]["map"], pm[k]["ci"][0], pm[k]["ci"][1], pm[k]["var"]]
                          for k in ("ate", "att", "atu")])
    close(got, d["avg"])
    pm2 = A.pred_marginal_cpp(d["y"], d["Z2"], th[0], th[1], d["inv"], d["cube_xX"],
                              d["cube_xx"], 0.3, 1.9, 0.8, False)
    assert "ate" not in pm2


# ------------------------------------------------------------------ fused model
@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
@pytest.mark.parametrize("n,p,B", [(300, 2, 5), (513, 3, 4), (1000, 20, 10), (130, 1, 2),
                                   (600, 32, 5), (700, 40, 6), (300, 64, 3), (200, 50, 32)])
def test_model_para_update_matches_oracle(A, O, kernel, n, p, B):
    """One device-resident para_update (kernel + sweep + fused gradient) vs the
    oracle's kernmat_sym -> invkernel -> grad chain, at iter 1 (mu first) and 2.
    Every case runs the MFMA-expansion pair kernels (both gradient workgroup
    shapes, diagonal and strictly lower tiles, per-slice and double-buffered
    partials); (200, 50, 32) is the largest per-tile LDS staging (PM = 64,
    B = 32: above 64 KB, one workgroup per CU)."""
    from additivecausalexpansion_amd.synthetic import make_problem
    y, X, Z, th, sy = make_problem(n, p, B, seed=7)
    m = A.DeviceModel(kernel, n, p, B)
    m.set_data(y, X, Z, sy)
    sym, _, grad = O.KERNELS[kernel]
    for it in (1, 2):
        t_dev = th.copy()
        g, st, mu_post = m.para_update(it, t_dev)
        t_ref = th.copy()
        Kl = sym(X, Z, t_ref)
        inv = O.invkernel_cpp(Kl["full"], t_ref[0])
        if it == 1:
            t_ref[1] = O.mu_solution_cpp(y, inv["inv"])
        st_ref = np.zeros(2)
        g_ref = grad(y, X, Z, Kl["full"], Kl["elements"], inv["inv"], inv["eigenval"], t_ref,
                     st_ref, B, sy)
        assert t_dev[1] == pytest.approx(t_ref[1], rel=1e-8, abs=1e-12)
        close(g, g_ref)
        close(st, st_ref)
        assert mu_post == pytest.approx(O.mu_solution_cpp(y, inv["inv"]), rel=1e-8)
        if it == 1:
            close(m.inverse(), inv["inv"], 1e-9, 1e-9)
        th = th + 0.01


def test_model_train_stats_keeps_inverse(A, O):
    from additivecausalexpansion_amd.synthetic import make_problem
    y, X, Z, th, sy = make_problem(400, 3, 4, seed=3)
    m = A.DeviceModel("SE", 400, 3, 4)
    m.set_data(y, X, Z, sy)
    m.para_update(2, th.copy())
    inv1 = m.inverse()
    th2 = th + 0.05
    st = m.train_stats(th2)
    K = O.kernmat_SE_symmetric_cpp(X, Z, th2)["full"]
    inv = O.invkernel_cpp(K, th2[0])
    close(st, O.stats_cpp(y, K, inv["inv"], inv["eigenval"], th2[1], sy))
    assert np.array_equal(m.inverse(), inv1)  # Q6: predict keeps the para_update inverse


# ------------------------------------------------------------------ training loop
@pytest.mark.parametrize("kernel", ["SE", "Matern32"])
def test_training_trajectory_matches_golden(A, kernel):
    """README config (n=300, d=2, ns n.knots=2, Nadam lr 0.01), 20 iterations of
    ace.train through the R6 mirror on the device-resident path.

    (1) anchored: each iteration's native work (para_update at the golden
        theta_{it-1}) must reproduce the golden stats and raw gradient to 1e-6;
    (2) free run: the whole loop (device gradients -> host norm clip + Nadam ->
        mu overwrite) must track the golden trajectory.  Nadam divides by
        sqrt(v), so last-bit differences in small gradient components are
        amplified along the loop: theta is held to 1e-5 relative, stats to 1e-6;
    (3) prediction at the golden theta_T with the golden theta_{T-1} inverse
        (Q6).  That mix makes the reference's variance |K_xx - q + e^s| a
        cancellation of terms ~1e3 x larger than the result, so its tolerance is
        1e-6 of the cancelled terms (std_y^2 (K_xx,rr + q_r)), not of the result.
    """
    d = golden(f"traj_{kernel}")
    y, X, Bm = d["y"], np.asfortranarray(d["X"]), np.asfortranarray(d["basis"])
    B = Bm.shape[1] + 1
    sy, my = float(d["moments"][0, 1]), float(d["moments"][0, 0])
    Kc = A.KernelClass_SE_R6 if kernel == "SE" else A.KernelClass_Matern32_R6
    # (1) anchored
    m = A.DeviceModel(kernel, 300, 2, B)
    m.set_data(y, X, Bm, sy)
    for it in range(1, 21):
        th = (d["theta0"] if it == 1 else d["thetas"][it - 2]).copy()
        g, st, _ = m.para_update(it, th)
        close(st, d["stats"][it - 1])
        close(g, d["grads"][it - 1])
    # (2) free run
    k = Kc(2, B, d["theta0"], sy)
    opt = A.set_optimizer("Nadam", k, 0.01, 0.0, 0.9, 0.999, True, 1.0)
    for it in range(1, 21):
        st = k.para_update(it, y, X, Bm, opt, verbose=False)
        close(st, d["stats"][it - 1], 1e-6, 1e-9)
        close(k.parameters, d["thetas"][it - 1], 1e-5, 1e-9)
    # (3) prediction (Q6: inverse of theta_{T-1}, kernels at theta_T)
    k.parameters = d["thetas"][18].copy()
    k.para_update(20, y, X, Bm, A.set_optimizer("GD", k, 0.0, 0.0, 0.9, 0.999, False, 1.0),
                  verbose=False)
    k.parameters = d["thetas"][19].copy()
    pr = k.predict(y, X, Bm, X, Bm, my, sy)
    close(pr["map"], d["pred_map"], 1e-6, 1e-9)
    sym = A.kernmat_SE_symmetric_cpp if kernel == "SE" else A.kernmat_Matern32_symmetric_cpp
    kxx = np.diag(sym(X, Bm, d["thetas"][19])["full"])
    terms = sy ** 2 * (2 * np.abs(kxx) + abs(np.exp(d["thetas"][19][0])))
    assert np.all(np.abs(pr["var"] - d["pred_var"]) <= 1e-6 * terms), \
        np.max(np.abs(pr["var"] - d["pred_var"]) / terms)


def test_ace_train_and_predict_end_to_end(A):
    from additivecausalexpansion_amd.synthetic import readme_data
    y, X, Z = readme_data(seed=5, n=200)
    fit = A.ace_train(y, X, Z, kernel="SE", basis="cubic", n_knots=2, maxiter=30, verbose=False)
    ev = fit["train_stats"]["stats"][1]
    assert np.all(np.isfinite(ev)) and ev[-1] > ev[0]
    pr = A.predict_ace(fit)
    assert pr["map"].shape == (200,) and np.all(pr["var"] > 0)
    pm = A.predict_ace(fit, marginal=True)
    assert pm["map"].shape == (200,)
    # binary treatment: ATE / ATT / ATU
    rng = np.random.default_rng(1)
    zb = (rng.random(200) < 0.5).astype(float)
    yb = X[:, 0] + 2 * zb + rng.normal(0, .3, 200)
    fb = A.ace_train(yb, X, zb, maxiter=15, verbose=False)
    out = A.predict_ace(fb, marginal=True, return_average_treatments=True)
    assert set(out) >= {"ate", "att", "atu"}


@pytest.mark.parametrize("optimizer,kernel", [("Nadam", "SE"), ("Adam", "Matern32"),
                                              ("NAG", "SE")])
def test_native_training_loop_matches_python_loop(A, optimizer, kernel):
    """ace_model_train (the R loop of R/main_ace.R:213-235 fused on the
    device, tests/test_train_gpu.py) and the host-driven Python mirror of the
    loop (native para_update + host optimizer) follow the same trajectory to
    the training tolerances, with the same stopping iteration.  (The golden
    trajectory check of the device loop is in tests/test_train_gpu.py.)"""
    from additivecausalexpansion_amd.synthetic import readme_data
    y, X, Z = readme_data(seed=9, n=250)
    kw = dict(kernel=kernel, basis="cubic", n_knots=2, optimizer=optimizer, maxiter=40,
              tol=1e-3, learning_rate=0.02, momentum=0.5, norm_clip=True, verbose=False)
    f_py = A.ace_train(y, X, Z, **kw)
    f_nat = A.ace_train(y, X, Z, native_loop=True, **kw)
    s_nat, s_py = f_nat["train_stats"]["stats"], f_py["train_stats"]["stats"]
    assert s_nat.shape == s_py.shape
    close(s_nat, s_py, 1e-6, 1e-9)
    assert f_nat["train_stats"]["convergence"] == f_py["train_stats"]["convergence"]
    # the two loops round their tables (device vs host exp) and the clip norm
    # (block vs sequential sum) differently; 40 optimizer steps amplify that
    # to a few 1e-5 of a parameter (NAG has no sqrt(v) normalisation)
    close(f_nat["Kernel"].parameters, f_py["Kernel"].parameters, 1e-4, 1e-9)
    p_nat, p_py = A.predict_ace(f_nat), A.predict_ace(f_py)
    close(p_nat["map"], p_py["map"], 1e-5, 1e-6)


def test_native_training_loop_nonfinite_stops(A):
    """A learning rate that blows the hyperparameters up ends in the
    optimizer's stop() (R/optimizer_classes.R:26-29) -> ACE_ERR_NONFINITE."""
    from additivecausalexpansion_amd.synthetic import make_problem
    y, X, Z, th, sy = make_problem(200, 2, 3, seed=2)
    m = A.DeviceModel("SE", 200, 2, 3)
    m.set_data(y, X, Z, sy)
    th = th.copy()
    th[0] = 800.0  # e^800 overflows: non-finite stats and gradient
    with pytest.raises(A.AceError, match="NONFINITE"):
        m.train(th, "Nadam", maxiter=5)


def test_interrupt_poll_stops_training(A):
    """ace_set_interrupt_poll: the poll runs before every para_update; a true
    return stops ace_model_train with ACE_ERR_INTERRUPTED (R's interrupt,
    Rcpp::checkUserInterrupt in the reference's loops)."""
    from additivecausalexpansion_amd.synthetic import make_problem
    y, X, Z, th, sy = make_problem(200, 2, 3, seed=4)
    ctx = A.Context(0)
    calls = []
    ctx.set_interrupt_poll(lambda: calls.append(1) or len(calls) > 3)
    m = A.DeviceModel("SE", 200, 2, 3, ctx=ctx)
    m.set_data(y, X, Z, sy)
    with pytest.raises(A.AceError, match="INTERRUPTED"):
        m.train(th.copy(), "Nadam", maxiter=50)
    assert len(calls) == 4  # three iterations ran, the fourth poll stopped the loop
    ctx.set_interrupt_poll(None)
    m.para_update(1, th.copy())  # no poll any more


# ------------------------------------------------------------------ full-size properties
def test_sweep_large_residual_and_logdet(A):
    """n = 4096 (C1 size): ||A A^-1 - I|| small and logdet vs LAPACK slogdet."""
    from additivecausalexpansion_amd.synthetic import make_problem
    y, X, Z, th, sy = make_problem(4096, 10, 6, seed=1)
    K = A.kernmat_SE_symmetric_cpp(X, Z, th)["full"]
    r = A.invkernel_cpp(K, th[0])
    Am = K + math.exp(th[0]) * np.eye(4096)
    R = Am @ r["inv"] - np.eye(4096)
    assert np.abs(R).max() < 1e-8
    s, ld = np.linalg.slogdet(Am)
    assert s > 0 and np.sum(np.log(r["eigenval"])) == pytest.approx(ld, rel=1e-10)


_ORDER_SNIPPET = """
import sys, numpy as np
sys.path.insert(0, {root!r})
import additivecausalexpansion_amd as A
d = np.load({inp!r})
r = A.invkernel_cpp(d["K"], float(d["s"]))
np.save({out!r}, r["inv"])
"""


def test_update_tile_order_is_bitwise_neutral(A, tmp_path):
    """The XCD super-block tile order of k_update (ACE_UPD_ORDER=S, default
    4) only changes which workgroup runs a tile, never its arithmetic: the
    inverse is bit-identical to the row-major grid (S = 0) and to S = 2."""
    import os
    import subprocess
    import sys
    from additivecausalexpansion_amd.synthetic import make_problem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = 1500  # 6 sweep steps, 13 x 13 tiles: padding entries in every order
    y, X, Z, th, _ = make_problem(n, 4, 5, seed=7)
    K = A.kernmat_SE_symmetric_cpp(X, Z, th)["full"]
    inp = str(tmp_path / "k.npz")
    np.savez(inp, K=K, s=th[0])
    outs = {}
    for S in ("0", "2", "4"):
        out = str(tmp_path / f"inv{S}.npy")
        env = dict(os.environ, ACE_UPD_ORDER=S)
        run_child(_ORDER_SNIPPET.format(root=root, inp=inp, out=out), env=env, timeout=100)
        outs[S] = np.load(out)
    assert np.array_equal(outs["0"], outs["4"]) and np.array_equal(outs["2"], outs["4"])
    mine = A.invkernel_cpp(K, th[0])["inv"]  # this process: default order
    assert np.array_equal(mine, outs["4"])


# the n > 8192 production regime (Z = 4, the plain bulk grid, Q beside the
# rest of the lookahead), selected at sizes that take seconds
LARGE_N_REGIME = {"ACE_GROUP": "4", "ACE_BULK_RESERVE": "0", "ACE_QFIRST": "0"}


@pytest.mark.parametrize("n", [300, 900, 1100, 1500, 2600])
def test_sweep_schedules_are_bitwise_neutral(A, tmp_path, n):
    """The default schedule (run_sweep_heads: Z sweep steps per bulk launch,
    head / tail lookahead) runs every element's MFMA chain over the same k
    order as the one-step reference schedule (ACE_PAIR=0, `single`): the
    inverse is bit-identical.  n = 1100: 5 steps, 1500: 6, 2600: 11, so the
    groups are 2+2+1 / 3+2 / 4+1, 2+2+2 / 3+3 / 4+2 and 2 x 5 + 1 / 3+3+3+2 /
    4+4+3 at Z = 2 / 3 / 4 (ACE_GROUP); n = 300: 2 steps, one group at every
    Z; n = 900: 4 steps, 2+2 / 3+1 / 4, so the default Z = 3 ends on a group of
    a single step in the small-n regime.  `default` is the small-n regime:
    Z = 3, the bulk launches as a persistent queue that leaves 1 CU per
    engine to the chains, and with it the head launches on 32 x 32 pieces,
    each panel's four sub-steps in one k_panel_split4 launch and the last
    tail panel GEMM on the head stream; the same at Z = 2 and 4, with 2 CUs
    reserved, and with the plain grid instead (ACE_BULK_RESERVE=0: 64 x 64
    head pieces, four k_panel_split launches, k_panel_gemm_t tails).  The
    next group's Q launch runs before (default at these n) or beside
    (ACE_QFIRST=0) the bulk launch and the rest of the cross; the fused
    chains run alone on their CUs (extra LDS, ACE_CHAIN_XLDS, default) or
    share them (0).  `large_n_regime` is exactly what n > 8192 runs, and
    `large_n_regime3` the same at Z = 3."""
    import os
    from additivecausalexpansion_amd.synthetic import make_problem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    y, X, Z, th, _ = make_problem(n, 4, 5, seed=23)
    K = A.kernmat_SE_symmetric_cpp(X, Z, th)["full"]
    inp = str(tmp_path / "k.npz")
    np.savez(inp, K=K, s=th[0])
    outs = {}
    variants = {"single": {"ACE_PAIR": "0"}, "default": {},
                "heads2": {"ACE_GROUP": "2"},
                "heads3": {"ACE_GROUP": "3"},
                "heads4": {"ACE_GROUP": "4"},
                "heads4_unreserved": {"ACE_BULK_RESERVE": "0"},
                "heads4_reserve2": {"ACE_BULK_RESERVE": "2"},
                "heads4_q_beside": {"ACE_QFIRST": "0"},
                "heads4_q_beside_unreserved": {"ACE_QFIRST": "0", "ACE_BULK_RESERVE": "0"},
                "chain_xlds_off": {"ACE_CHAIN_XLDS": "0"},
                "large_n_regime": LARGE_N_REGIME,
                "large_n_regime3": {**LARGE_N_REGIME, "ACE_GROUP": "3"}}
    for name, ev in variants.items():
        out = str(tmp_path / f"inv_{name}.npy")
        env = dict(os.environ, **ev)
        run_child(_ORDER_SNIPPET.format(root=root, inp=inp, out=out), env=env, timeout=100)
        outs[name] = np.load(out)
    for name in variants:
        assert np.array_equal(outs["single"], outs[name]), name


_MODEL_SNIPPET = """
import sys, numpy as np
sys.path.insert(0, {root!r})
import additivecausalexpansion_amd as A
from additivecausalexpansion_amd.synthetic import make_problem
y, X, Z, th, sy = make_problem({n}, 6, 4, seed=31)
m = A.DeviceModel("Matern32", {n}, 6, 4)
m.set_data(y, X, Z, sy)
outs = []
for it in (1, 2):
    g, st, mu = m.para_update(it, th)
    outs += [g, st, np.array([mu])]
    th = th + 0.01 * g / max(1.0, float(np.abs(g).max()))
np.save({out!r}, np.concatenate(outs))
"""


@pytest.mark.parametrize("n", [2000, 2600])
def test_model_schedules_are_bitwise_neutral(tmp_path, n):
    """The fused model's para_update gives the same gradient and stats bit
    for bit, over two evaluations, under the one-step reference schedule
    (ACE_PAIR=0, the baseline) and the head / tail schedule at two, three and
    four steps per bulk launch, with no override at all (at these n: Z = 3 on
    three streams with the small-n bulk queue) and under exactly what
    n > 8192 runs (LARGE_N_REGIME).  n = 2000: 8 steps; 2600: 11 (a last
    single step).  Also the no-override schedule under the smaller stream
    budgets (ACE_STREAMS=2: the tail path on the panel stream; 1: everything
    on the main stream), which run the same launch graph serialised in host
    order."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    variants = {"single": {"ACE_PAIR": "0"}, "default": {},
                "heads4": {"ACE_GROUP": "4"}, "heads3": {"ACE_GROUP": "3"},
                "heads2": {"ACE_GROUP": "2"}, "large_n_regime": LARGE_N_REGIME,
                "streams2": {"ACE_STREAMS": "2"}, "streams1": {"ACE_STREAMS": "1"}}
    outs = {}
    for v, ev in variants.items():
        out = str(tmp_path / f"m{v}.npy")
        run_child(_MODEL_SNIPPET.format(root=root, n=n, out=out), env=dict(os.environ, **ev),
                  timeout=100)
        outs[v] = np.load(out)
    assert np.all(np.isfinite(outs["single"]))
    for v in ("default", "heads4", "heads3", "heads2", "large_n_regime"):
        assert np.array_equal(outs["single"], outs[v]), v
    # the no-override schedule on two streams and on one
    assert np.array_equal(outs["default"], outs["streams2"])
    assert np.array_equal(outs["default"], outs["streams1"])


_MODEL_SNIPPET_K = _MODEL_SNIPPET.replace('"Matern32"', '{kernel!r}')


@pytest.mark.parametrize("kernel,n", [("Matern32", 2000), ("SE", 2600)])
def test_persistent_assembly_is_bitwise_neutral(tmp_path, kernel, n):
    """The assembly's second part as a persistent tile queue that leaves one
    CU per shader engine to the first group's lookahead (default:
    ACE_ASM_PERSIST=1, the tail path beside the head path and a filler launch
    joining the queue afterwards) assembles every tile exactly as the plain
    grid does: gradient, stats and mu bit for bit against ACE_ASM_PERSIST=0,
    over two evaluations (the queue reset per evaluation), and under the
    other switches and the one-stream budget."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    variants = {"plain": {"ACE_ASM_PERSIST": "0"}, "default": {},
                "tail_after": {"ACE_ASM_TAIL": "0", "ACE_ASM_FILL": "0"},
                "tail_split": {"ACE_ASM_TAIL": "2"},
                "two_per_engine": {"ACE_ASM_PERSIST": "2"},
                "one_stream": {"ACE_STREAMS": "1"}}
    outs = {}
    for name, ev in variants.items():
        out = str(tmp_path / f"p_{name}.npy")
        run_child(_MODEL_SNIPPET_K.format(root=root, n=n, out=out, kernel=kernel),
                  env=dict(os.environ, **ev), timeout=100)
        outs[name] = np.load(out)
    assert np.all(np.isfinite(outs["plain"]))
    for name in variants:
        assert np.array_equal(outs["plain"], outs[name]), name
