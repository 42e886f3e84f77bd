"""The batched engine (ace_batch_*, csrc/ace_batch.hip): many small models,
one workgroup per model.  Checked against the oracle and against the
single-model device path at the project's bound (test_gpu.close, RTOL 1e-6,
atol 1e-9 max|ref|), plus what one-workgroup-per-model promises: a model's
outputs are bitwise independent of M, of its position and of its neighbours
(a non-finite neighbour included), and every model stops on its own."""
import numpy as np
import pytest

import batch_cases as C
from conftest import golden
from test_gpu import close

pytestmark = pytest.mark.gpu

KERNELS = ["SE", "Matern32"]
RAGGED_N = (7, 16, 17, 64, 65, 130)  # the 16-wide fragment, the 64-wide wave, the tails
NONFINITE = 5  # ACE_ERR_NONFINITE


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.default_context()
    return pkg


@pytest.fixture(scope="module")
def O():
    from oracle import ace_oracle
    return ace_oracle


def _problems(ns, p, B, seed0=0):
    return C.problems(ns, p, B, seed0)


def _batch(A, kernel, probs, p, B, nmax=None, order=None):
    order = list(range(len(probs))) if order is None else order
    bm = A.BatchModel(kernel, len(order), nmax or max(probs[j][0].size for j in order), p, B)
    for pos, j in enumerate(order):
        y, X, Z, _, sy = probs[j]
        bm.set_data(pos, y, X, Z, sy)
    return bm


def _theta_of(prob, it):
    """The model's theta of iteration it: make_problem's (the one
    test_predict_gpu._fit_state evaluates at) at iter 1; at iter 2 a random
    one within the ranges of tests/golden/make_golden.py, seeded by the
    model alone so that it does not depend on the model's place in a batch."""
    y, X, Z, th, _ = prob
    if it == 1:
        return th.copy()
    n, p, B = y.size, X.shape[1], Z.shape[1] + 1
    rng = np.random.default_rng(1000 + 64 * n + p + 7 * B)
    return np.concatenate([[np.log(rng.uniform(0.05, 0.5)), rng.normal(0, 0.2)],
                           rng.normal(0, 0.4, B), rng.normal(0.5, 0.8, B * p)])


def _theta(probs, order=None, it=1):
    order = list(range(len(probs))) if order is None else order
    return np.asfortranarray(np.column_stack([_theta_of(probs[j], it) for j in order]))


def _oracle_update(O, kernel, it, prob, th, B):
    y, X, Z, _, sy = prob
    sym, _, grad = O.KERNELS[kernel]
    t = th.copy()
    Kl = sym(X, Z, t)
    inv = O.invkernel_cpp(Kl["full"], t[0])
    mu = O.mu_solution_cpp(y, inv["inv"])
    if it == 1:
        t[1] = mu
    st = np.zeros(2)
    g = grad(y, X, Z, Kl["full"], Kl["elements"], inv["inv"], inv["eigenval"], t, st, B, sy)
    return g, st, mu, inv["inv"], t


_ragged_cache = {}


def _ragged(A, kernel):
    """The ragged batch's para_update at iter 1 and 2, computed once per
    kernel and shared (read-only) by the tests that compare against it."""
    if kernel not in _ragged_cache:
        probs = _problems(RAGGED_N, 3, 5)
        bm = _batch(A, kernel, probs, 3, 5)
        res = []
        for it in (1, 2):
            th = _theta(probs, it=it)
            g, st, mu = bm.para_update(it, th)
            res.append((th, g, st, mu, [bm.inverse(j) for j in range(len(probs))]))
        bm.close()
        _ragged_cache[kernel] = (probs, res)
    return _ragged_cache[kernel]


# ------------------------------------------------------------------ 1. evaluation
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ns,p,B", [
    (RAGGED_N, 3, 5), ((33, 33), 1, 1), ((97, 97), 20, 10), ((300, 300), 2, 5), ((512, 512), 2, 2),
    ((130,), 8, 3), ((97,), 16, 2),  # p equals its feature bucket: no zero padding
    ((70, 45), 64, 2),               # PM = 64 unpadded: both passes of the length-scale sums
    ((50,), 2, 32),                  # B at its maximum, ZS = 31
    # 256 threads: the second trip of the assembly and gradient row loops at
    # n = 257 (one live lane in the fifth wave), the assembly's third at n = 512
    # (528 rows with the right-hand sides)
    ((257, 300, 512), 20, 3),
    ((272, 511), 33, 2),             # PM = 64 at 256 threads; n a multiple of 16, and 511
])
def test_batch_para_update_matches_oracle_and_device_model(A, O, kernel, ns, p, B):
    """Every model of the batch against the oracle's kernmat_sym -> invkernel ->
    grad chain and against DeviceModel.para_update, at iter 1 (mu first) and 2."""
    if ns == RAGGED_N:
        probs, res = _ragged(A, kernel)
        bm = None
    else:
        probs = _problems(ns, p, B)
        bm = _batch(A, kernel, probs, p, B)
    for it in (1, 2):
        if bm is None:
            th, g, st, mu, invs = res[it - 1]
        else:
            th = _theta(probs, it=it)
            g, st, mu = bm.para_update(it, th)
            invs = [bm.inverse(j) for j in range(len(probs))]
        for j, prob in enumerate(probs):
            th_in = _theta_of(prob, it)
            g_ref, st_ref, mu_ref, inv_ref, t_ref = _oracle_update(O, kernel, it, prob, th_in, B)
            assert th[1, j] == pytest.approx(t_ref[1], rel=1e-8, abs=1e-12)
            close(g[:, j], g_ref, check="batch grad vs oracle")
            close(st[:, j], st_ref, check="batch stats vs oracle")
            assert mu[j] == pytest.approx(mu_ref, rel=1e-8, abs=1e-12)
            close(invs[j], inv_ref, check="batch inverse vs oracle")
            m = A.DeviceModel(kernel, prob[0].size, p, B)
            m.set_data(prob[0], prob[1], prob[2], prob[4])
            t_dev = th_in.copy()
            g_dev, st_dev, mu_dev = m.para_update(it, t_dev)
            m.close()
            close(g[:, j], g_dev, check="batch grad vs DeviceModel")
            close(st[:, j], st_dev, check="batch stats vs DeviceModel")
            assert mu[j] == pytest.approx(mu_dev, rel=1e-8, abs=1e-12)
    if bm is not None:
        bm.close()


# ------------------------------------------------------------------ 2. independence
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_model_is_bitwise_independent_of_batch_and_position(A, kernel):
    probs, res = _ragged(A, kernel)
    th0, g0, st0, mu0, inv0 = res[1]
    M = len(probs)
    # alone, in a batch of one sized for the model itself
    for j in range(M):
        bm = _batch(A, kernel, probs, 3, 5, order=[j])
        g, st, mu = bm.para_update(2, _theta(probs, [j], it=2))
        assert np.array_equal(g[:, 0], g0[:, j]) and np.array_equal(st[:, 0], st0[:, j])
        assert mu[0] == mu0[j]
        assert np.array_equal(bm.inverse(0), inv0[j])
        bm.close()
    # at another position (the batch reversed), and on a repeated call
    order = list(range(M))[::-1]
    bm = _batch(A, kernel, probs, 3, 5, order=order)
    for _ in range(2):
        g, st, mu = bm.para_update(2, _theta(probs, order, it=2))
        for pos, j in enumerate(order):
            assert np.array_equal(g[:, pos], g0[:, j]) and np.array_equal(st[:, pos], st0[:, j])
            assert mu[pos] == mu0[j]
            assert np.array_equal(bm.inverse(pos), inv0[j])
    bm.close()


# ------------------------------------------------------------------ 3. M > CUs
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_more_workgroups_than_cus(A, kernel):
    prob = _problems((7,), 1, 2)[0]
    M = 300
    bm = _batch(A, kernel, [prob], 1, 2, order=[0] * M)
    g, st, mu = bm.para_update(1, _theta([prob], [0] * M))
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(st))
    for j in range(1, M):
        assert np.array_equal(g[:, j], g[:, 0]) and np.array_equal(st[:, j], st[:, 0])
        assert mu[j] == mu[0]
    assert np.array_equal(bm.inverse(M - 1), bm.inverse(0))
    bm.close()


# ------------------------------------------------------------------ 4. non-finite
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_nonfinite_model_does_not_leak(A, kernel):
    probs, res = _ragged(A, kernel)
    th0, g0, st0, mu0, inv0 = res[1]
    M, bad = len(probs), 3
    bm = _batch(A, kernel, probs, 3, 5)
    th = _theta(probs, it=2)
    th[2, bad] = np.nan
    g, st, mu = bm.para_update(2, th)
    assert not np.any(np.isfinite(g[:, bad])) and not np.any(np.isfinite(st[:, bad]))
    for j in range(M):
        if j == bad:
            continue
        assert np.array_equal(g[:, j], g0[:, j]) and np.array_equal(st[:, j], st0[:, j])
        assert mu[j] == mu0[j]
        assert np.array_equal(bm.inverse(j), inv0[j])
    # train: the model's status is ACE_ERR_NONFINITE and its theta is kept (but
    # theta[1], the iteration-1 mean_solution assigned before the optimizer)
    th = _theta(probs)
    th[2, bad] = np.nan
    before = th.copy()
    stats, its, conv, status = bm.train(th, "Nadam", maxiter=5, tol=-1.0)
    assert status[bad] == NONFINITE and its[bad] == 1 and not conv[bad]
    keep = np.delete(np.arange(th.shape[0]), 1)
    assert np.array_equal(th[keep, bad], before[keep, bad], equal_nan=True)
    clean = _batch(A, kernel, probs, 3, 5)
    th_c = _theta(probs)
    stats_c, its_c, _, status_c = clean.train(th_c, "Nadam", maxiter=5, tol=-1.0)
    assert np.all(status_c == 0)
    for j in range(M):
        if j == bad:
            continue
        assert status[j] == 0 and its[j] == 5
        assert np.array_equal(th[:, j], th_c[:, j])
        assert np.array_equal(stats[:, :, j], stats_c[:, :, j])
    clean.close()
    bm.close()


# ------------------------------------------------------------------ 5. golden trajectories
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_train_matches_golden_trajectory(A, kernel):
    """README config (n = 300, Nadam 0.01, 20 iterations, tol = -1): the golden
    dataset twice and once with y negated; bounds of
    test_train_gpu.test_device_loop_matches_golden_trajectory."""
    d = golden(f"traj_{kernel}")
    y, X, Bm = d["y"], np.asfortranarray(d["X"]), np.asfortranarray(d["basis"])
    B = Bm.shape[1] + 1
    sy = float(d["moments"][0, 1])
    bm = A.BatchModel(kernel, 3, 300, 2, B)
    for j, yy in enumerate((y, y, -y)):
        bm.set_data(j, yy, X, Bm, sy)
    th = np.asfortranarray(np.column_stack([d["theta0"]] * 3))
    stats, its, conv, status = bm.train(th, "Nadam", 0.01, 0.0, 0.9, 0.999, True, 1.0,
                                        maxiter=20, tol=-1.0)
    bm.close()
    assert np.all(its == 20) and not np.any(conv) and np.all(status == 0)
    assert np.array_equal(stats[:, :, 0], stats[:, :, 1]) and np.array_equal(th[:, 0], th[:, 1])
    close(stats[:, 1:21, 0].T, d["stats"], 1e-6, 1e-9, check="batch train stats vs golden")
    close(th[:, 0], d["thetas"][19], 1e-5, 1e-9, check="batch train theta vs golden")
    assert np.all(stats[:, 0, :] == 0.0)
    m = A.DeviceModel(kernel, 300, 2, B)
    m.set_data(-y, X, Bm, sy)
    th2 = d["theta0"].copy()
    stats2, it2, _ = m.train(th2, "Nadam", 0.01, 0.0, 0.9, 0.999, True, 1.0, maxiter=20, tol=-1.0)
    m.close()
    assert it2 == 20
    close(stats[:, 1:22, 2], stats2[:, 1:22], 1e-6, 1e-9, check="batch train stats vs DeviceModel")
    close(th[:, 2], th2, 1e-5, 1e-9, check="batch train theta vs DeviceModel")


# ------------------------------------------------------------------ 6. per-model stopping
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_models_stop_on_their_own(A, O, kernel):
    """Nadam 0.05, tol 0.9, maxiter 30: the oracle's evidence steps of the three
    models (n = 60, 90, 130) fall below 0.9 at iterations 8, 15 or 16 and 22 or
    25, each with the neighbouring steps at least 0.01 away from the tolerance."""
    from additivecausalexpansion_amd.synthetic import make_problem
    tol, maxiter, lr = 0.9, 30, 0.05
    probs = [make_problem(n, 2, 3, seed=s) for n, s in ((60, 1), (90, 2), (130, 3))]
    stops, inv_ref = [], []
    for y, X, Z, th, sy in probs:
        opt = O.OracleOptimizer("Nadam", th.size, lr)
        _, st, _, _ = O.train_trajectory(kernel, y, X, Z, th, sy, maxiter, opt)
        ev = np.concatenate([[0.0], st[:, 1]])
        step = np.abs(np.diff(ev))
        T = next(it for it in range(4, maxiter + 1) if step[it - 1] < tol)
        stops.append(T)
        opt = O.OracleOptimizer("Nadam", th.size, lr)
        inv_ref.append(O.train_trajectory(kernel, y, X, Z, th, sy, T, opt)[3])  # at theta_{T-1}
    assert min(abs(a - b) for i, a in enumerate(stops) for b in stops[i + 1:]) >= 2, stops
    bm = _batch(A, kernel, probs, 2, 3)
    th = _theta(probs)
    stats, its, conv, status = bm.train(th, "Nadam", lr, maxiter=maxiter, tol=tol)
    assert list(its) == stops and np.all(conv) and np.all(status == 0)
    for j in range(3):
        one = _batch(A, kernel, probs, 2, 3, order=[j])
        th1 = _theta(probs, [j])
        stats1, its1, conv1, status1 = one.train(th1, "Nadam", lr, maxiter=maxiter, tol=tol)
        assert its1[0] == its[j] and conv1[0] == conv[j] and status1[0] == 0
        assert np.array_equal(th1[:, 0], th[:, j])
        assert np.array_equal(stats1[:, :, 0], stats[:, :, j])
        assert np.all(stats[:, its[j] + 2:, j] == 0.0)
        assert np.array_equal(one.inverse(0), bm.inverse(j))
        one.close()
        close(bm.inverse(j), inv_ref[j], 1e-6, 1e-9, check="batch inverse at theta_{T-1} vs oracle")
    bm.close()


# ------------------------------------------------------------------ 7. end to end
@pytest.mark.parametrize("kernel", KERNELS)
def test_train_batch_end_to_end_matches_ace_train(A, kernel):
    from additivecausalexpansion_amd.synthetic import readme_data
    data = [readme_data(seed=21 + j, n=n) for j, n in enumerate((300, 240, 270))]
    kw = dict(kernel=kernel, basis="cubic", n_knots=2, optimizer="Nadam", maxiter=25, tol=1e-4,
              learning_rate=0.01, verbose=False)
    fits = A.ace_train_batch([d[0] for d in data], [d[1] for d in data], [d[2] for d in data], **kw)
    assert len(fits) == 3
    for (y, X, Z), fit in zip(data, fits):
        ref = A.ace_train(y, X, Z, native_loop=True, **kw)
        assert fit["train_stats"]["stats"].shape == ref["train_stats"]["stats"].shape
        assert not fit["Kernel"]._inv_from_model
        pr, pr_ref = A.predict_ace(fit), A.predict_ace(ref)
        close(pr["map"], pr_ref["map"], 1e-4, 1e-6, check="batch fit predict map")
        close(pr["ci"], pr_ref["ci"], 1e-4, 1e-6, check="batch fit predict ci")
        pm = A.predict_ace(fit, marginal=True, return_average_treatments=True)
        pm_ref = A.predict_ace(ref, marginal=True, return_average_treatments=True)
        close(pm["map"], pm_ref["map"], 1e-4, 1e-6, check="batch fit marginal map")
        close(pm["ci"], pm_ref["ci"], 1e-4, 1e-6, check="batch fit marginal ci")


# ------------------------------------------------------------------ 8. argument errors
def test_batch_argument_errors(A):
    from additivecausalexpansion_amd.synthetic import make_problem
    with pytest.raises(A.AceError, match="ACE_ERR_UNSUPPORTED"):
        A.BatchModel("SE", 2, 513, 2, 3)
    with pytest.raises(A.AceError, match="ACE_ERR_UNSUPPORTED"):
        A.BatchModel("SE", 2, 100, 65, 3)
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        A.BatchModel("SE", 0, 100, 2, 3)
    bm = A.BatchModel("SE", 2, 40, 2, 3)
    y, X, Z, th, sy = make_problem(41, 2, 3, seed=1)
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        bm.set_data(0, y, X, Z, sy)  # n_j = nmax + 1
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        bm.set_data(2, y[:40], X[:40], Z[:40], sy)  # j = M
    bm.set_data(0, y[:40], X[:40], Z[:40], sy)
    th2 = np.asfortranarray(np.column_stack([th, th]))
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        bm.para_update(1, th2)  # model 1 has no data
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        bm.inverse(0)  # no para_update yet
    bm.set_data(1, y[:20], X[:20], Z[:20], sy)
    g, st, mu = bm.para_update(1, th2)
    assert np.all(np.isfinite(g)) and bm.inverse(1).shape == (20, 20)
    bm.close()


# ------------------------------------------------------------------ 9. slot reuse
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_slot_reused_for_a_smaller_model(A, kernel):
    """A slot given new, smaller data after a larger model runs over that
    model's leftovers in the scratch matrix: they must not reach its results."""
    big, small, other = _problems((130, 40, 97), 3, 5)
    th_of = lambda *ps: np.asfortranarray(np.column_stack([q[3] for q in ps]))  # noqa: E731
    bm = A.BatchModel(kernel, 2, 130, 3, 5)
    bm.set_data(0, big[0], big[1], big[2], big[4])
    bm.set_data(1, other[0], other[1], other[2], other[4])
    g1, st1, mu1 = bm.para_update(1, th_of(big, other))
    inv1 = bm.inverse(1)
    assert np.all(np.isfinite(g1)) and bm.inverse(0).shape == (130, 130)
    bm.set_data(0, small[0], small[1], small[2], small[4])
    g2, st2, mu2 = bm.para_update(1, th_of(small, other))
    fresh = A.BatchModel(kernel, 1, 130, 3, 5)
    fresh.set_data(0, small[0], small[1], small[2], small[4])
    gf, stf, muf = fresh.para_update(1, th_of(small))
    assert np.all(np.isfinite(gf)) and np.all(np.isfinite(stf))
    assert np.array_equal(g2[:, 0], gf[:, 0]) and np.array_equal(st2[:, 0], stf[:, 0])
    assert mu2[0] == muf[0]
    assert np.array_equal(bm.inverse(0), fresh.inverse(0)) and bm.inverse(0).shape == (40, 40)
    assert np.array_equal(g2[:, 1], g1[:, 1]) and np.array_equal(st2[:, 1], st1[:, 1])
    assert mu2[1] == mu1[1] and np.array_equal(bm.inverse(1), inv1)
    fresh.close()
    bm.close()


# ------------------------------------------------------------------ 10. not positive definite
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_not_positive_definite_model_gets_nan_and_does_not_leak(A, kernel):
    """Three models with an exactly zero pivot (batch_cases.singular_cases;
    tests/test_batch_regimes_cpu.py shows the row of A is exactly zero) -- in
    the first 16-block, in a later one and in the ragged last one -- between
    two healthy models.  The kernel's own pivot test has to fire: nothing in
    theta or the data is non-finite."""
    ragged, res = _ragged(A, kernel)
    healthy = [RAGGED_N.index(n) for n in C.HEALTHY_N]
    sing = [c[1] for c in C.singular_cases()]
    probs = [sing[0], ragged[healthy[0]], sing[1], ragged[healthy[1]], sing[2]]
    bad, good = (0, 2, 4), (1, 3)
    th_all = lambda: np.asfortranarray(np.column_stack([q[3] for q in probs]))  # noqa: E731
    bm = _batch(A, kernel, probs, 3, 5)
    th = th_all()
    assert np.all(np.isfinite(th))
    g, st, mu = bm.para_update(1, th)
    for j in bad:
        assert not np.any(np.isfinite(g[:, j])) and not np.any(np.isfinite(st[:, j]))
        assert not np.isfinite(mu[j])
    # the healthy ones as in the ragged batch, which holds no singular model
    _, g0, st0, mu0, inv0 = res[0]
    for j, j0 in zip(good, healthy):
        assert np.all(np.isfinite(g[:, j]))
        assert np.array_equal(g[:, j], g0[:, j0]) and np.array_equal(st[:, j], st0[:, j0])
        assert mu[j] == mu0[j0] and th[1, j] == mu0[j0]
        assert np.array_equal(bm.inverse(j), inv0[j0])
    # train: status ACE_ERR_NONFINITE at iteration 1, theta kept (but theta[1],
    # the iteration-1 mean_solution assigned before the optimizer)
    th = th_all()
    before = th.copy()
    stats, its, conv, status = bm.train(th, "Nadam", maxiter=5, tol=-1.0)
    keep = np.delete(np.arange(th.shape[0]), 1)
    for j in bad:
        assert status[j] == NONFINITE and its[j] == 1 and not conv[j]
        assert np.array_equal(th[keep, j], before[keep, j])
    clean = _batch(A, kernel, [probs[j] for j in good], 3, 5)
    th_c = np.asfortranarray(before[:, list(good)])
    stats_c, its_c, _, status_c = clean.train(th_c, "Nadam", maxiter=5, tol=-1.0)
    assert np.all(status_c == 0) and np.all(its_c == 5)
    for k, j in enumerate(good):
        assert status[j] == 0 and its[j] == 5
        assert np.array_equal(th[:, j], th_c[:, k])
        assert np.array_equal(stats[:, :, j], stats_c[:, :, k])
    clean.close()
    bm.close()
    # the single-model path promises the same
    y, X, Z, ths, sy = sing[2]
    m = A.DeviceModel(kernel, y.size, 3, 5)
    m.set_data(y, X, Z, sy)
    g1, st1, mu1 = m.para_update(1, ths.copy())
    m.close()
    assert not np.any(np.isfinite(g1)) and not np.any(np.isfinite(st1)) and not np.isfinite(mu1)


# ------------------------------------------------------------------ 11. the other optimizers, the clip
_opt_oracle = {}


def _oracle_trajectory(O, kernel, name):
    """The oracle's trajectories of one configuration, computed once."""
    if (kernel, name) not in _opt_oracle:
        _, oname, lr, mom, clip, clip_at = C.OPT_CONFIGS[name]
        out = []
        for y, X, Z, th, sy in C.opt_problems(name):
            opt = O.OracleOptimizer(oname, th.size, lr, momentum=mom, norm_clip=clip, clip_at=clip_at)
            out.append(O.train_trajectory(kernel, y, X, Z, th, sy, C.OPT_ITERS, opt)[:3])
        _opt_oracle[(kernel, name)] = out
    return _opt_oracle[(kernel, name)]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", list(C.OPT_CONFIGS))
def test_batch_step_optimizers_and_clip(A, O, kernel, name):
    """k_batch_step's Nesterov and Adam branches, the clip switched off, and
    Q5 (||g|| > clip_at rescales to unit norm) at clip_at = 0.3, against the
    oracle's trajectory and DeviceModel.train with the bounds of
    test_batch_train_matches_golden_trajectory."""
    pname, _, lr, mom, clip, clip_at = C.OPT_CONFIGS[name]
    probs = C.opt_problems(name)
    T = C.OPT_ITERS
    ref = _oracle_trajectory(O, kernel, name)
    if clip_at != 1.0:
        # Q5 differs from a rescale to clip_at only where clip_at < ||g|| <= 1
        norms = np.array([np.linalg.norm(r[2], axis=1) for r in ref])
        print(f"{name} {kernel}: the oracle's ||g|| per model and iteration\n{norms}")
        assert np.all(np.any((norms > clip_at) & (norms <= 1.0), axis=1)), norms
    args = (pname, lr, mom, 0.9, 0.999, clip, clip_at)
    bm = _batch(A, kernel, probs, C.OPT_P, C.OPT_B)
    th = _theta(probs)
    stats, its, conv, status = bm.train(th, *args, maxiter=T, tol=-1.0)
    bm.close()
    assert np.all(its == T) and not np.any(conv) and np.all(status == 0)
    for j, (y, X, Z, th0, sy) in enumerate(probs):
        thetas, st_ref, _ = ref[j]
        close(stats[:, 1:T + 1, j].T, st_ref, 1e-6, 1e-9, check=f"batch {name} stats vs oracle")
        close(th[:, j], thetas[T - 1], 1e-5, 1e-9, check=f"batch {name} theta vs oracle")
        m = A.DeviceModel(kernel, y.size, C.OPT_P, C.OPT_B)
        m.set_data(y, X, Z, sy)
        th2 = th0.copy()
        stats2, it2, _ = m.train(th2, *args, maxiter=T, tol=-1.0)
        m.close()
        assert it2 == T
        close(stats[:, 1:T + 1, j], stats2[:, 1:T + 1], 1e-6, 1e-9, check=f"batch {name} stats vs DeviceModel")
        close(th[:, j], th2, 1e-5, 1e-9, check=f"batch {name} theta vs DeviceModel")
        one = _batch(A, kernel, probs, C.OPT_P, C.OPT_B, order=[j])
        th1 = _theta(probs, [j])
        stats1, its1, _, status1 = one.train(th1, *args, maxiter=T, tol=-1.0)
        one.close()
        assert its1[0] == its[j] and status1[0] == 0
        assert np.array_equal(th1[:, 0], th[:, j]) and np.array_equal(stats1[:, :, 0], stats[:, :, j])
