"""Batched prediction (ace_predict_batch / ace_predict_marginal_batch /
ace_set_inverse_batch, csrc/ace_batch_predict.hip): every model of a batch
against the oracle's pred_cpp / pred_marginal_cpp fed the oracle's own kernels
and inverse, and against the single-model device path, at
test_predict_gpu's bounds; plus what one-workgroup-per-model promises: a
model's outputs are bitwise independent of M, of its position, of nmax and of
its neighbours (a not-positive-definite neighbour included).

Conventions: tests/batch_predict_cases.py (test_predict_gpu._fit_state's).
"""
import numpy as np
import pytest

import batch_cases as C
import batch_predict_cases as PC
from conftest import record_error
from test_gpu import close
from test_predict_gpu import CI_TOL, VAR_TOL, _check_avg_edge

pytestmark = pytest.mark.gpu

KERNELS = list(PC.KERNELS)
KEYS = ("map", "ci", "var")


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.default_context()
    return pkg


@pytest.fixture(scope="module")
def O():
    from oracle import ace_oracle
    return ace_oracle


def _resident(A, kernel, ms, p, B, nmax=None, it=2):
    """A batch holding the models' data and, resident, their inverses at
    make_problem's theta."""
    bm = A.BatchModel(kernel, len(ms), nmax or max(m[0][0].size for m in ms), p, B)
    for j, (prob, _, _) in enumerate(ms):
        bm.set_data(j, prob[0], prob[1], prob[2], prob[4])
    th = np.asfortranarray(np.column_stack([m[0][3] for m in ms]))
    bm.para_update(it, th)
    return bm


def _thetas(ms, mix=True):
    return np.asfortranarray(np.column_stack([PC.theta_now(m[0][3], mix) for m in ms]))


def _plain(bm, ms, mix=True, j0=0):
    M = len(ms)
    return bm.predict(_thetas(ms, mix), [m[1] for m in ms], [m[2] for m in ms],
                      [PC.mean_y(j0 + j) for j in range(M)], [PC.std_y(j0 + j) for j in range(M)])


def _marginal(bm, ms, cases=None, ate=True, j0=0):
    M = len(ms)
    cases = cases or ["third"] * M
    return bm.predict_marginal(_thetas(ms, mix=False), [m[1] for m in ms],
                               [PC.dbasis(m[2]) for m in ms],
                               [PC.treated(m[1].shape[0], c) for m, c in zip(ms, cases)],
                               [PC.std_y(j0 + j) for j in range(M)],
                               [PC.std_Z(j0 + j) for j in range(M)], ate)


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ("ate", "att", "atu"):
        assert (k in a) == (k in b)
        if k in a:
            for q in KEYS:
                assert np.array_equal(a[k][q], b[k][q], equal_nan=True), (k, q)


def _check_plain(got, ref, terms, what):
    close(got["map"], ref["map"], check=f"batch predict map vs {what}")
    close(got["ci"], ref["ci"], 1e-6, 1e-8, check=f"batch predict ci vs {what}")
    err = np.abs(got["var"] - ref["var"]) / terms
    record_error(f"batch predict var vs {what}: max |err| / terms", np.max(err), VAR_TOL)
    assert np.all(err <= VAR_TOL), (what, np.max(err))


# ------------------------------------------------------------------ 1. plain prediction
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ns,nxs,p,B", PC.PLAIN_CASES)
def test_batch_predict_matches_oracle_and_device_model(A, O, kernel, ns, nxs, p, B):
    ms = PC.models(ns, nxs, p, B)
    bm = _resident(A, kernel, ms, p, B)
    got = _plain(bm, ms)
    bm.close()
    for j, m in enumerate(ms):
        (y, X, Z, th0, sy), X2, Z2 = m
        th = PC.theta_now(th0)
        assert got[j]["map"].shape == (nxs[j],) and got[j]["ci"].shape == (nxs[j], 2)
        ref, terms = PC.oracle_plain(O, kernel, m, th, PC.mean_y(j), PC.std_y(j))
        _check_plain(got[j], ref, terms, "oracle")
        dm = A.DeviceModel(kernel, y.size, p, B)
        dm.set_data(y, X, Z, sy)
        dm.para_update(2, th0.copy())
        dev = dm.predict(th, X2, Z2, PC.mean_y(j), PC.std_y(j))
        dm.close()
        _check_plain(got[j], dev, terms, "DeviceModel")


@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_predict_at_the_largest_lds(A, O, kernel):
    """n = 512, PM = 64, B = 32: the kernel's dynamic LDS at its maximum.  The
    launch must succeed (legal inputs are never unsupported); the reference is
    DeviceModel.predict with the model's own inverse in the variance terms
    (the oracle's n = 512, B = 32 cube would take this test past a few seconds)."""
    ns, nxs, p, B = PC.MAX_LDS_CASE
    m = PC.models(ns, nxs, p, B)[0]
    (y, X, Z, th0, sy), X2, Z2 = m
    bm = _resident(A, kernel, [m], p, B)
    got = _plain(bm, [m])[0]
    bm.close()
    th = PC.theta_now(th0)
    dm = A.DeviceModel(kernel, y.size, p, B)
    dm.set_data(y, X, Z, sy)
    dm.para_update(2, th0.copy())
    dev = dm.predict(th, X2, Z2, PC.mean_y(0), PC.std_y(0))
    inv = dm.inverse()
    dm.close()
    sym, cross = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    K_xX = cross(X2, X, Z2, Z, th)["full"]
    q = np.abs(np.sum((K_xX @ inv) * K_xX, axis=1))
    terms = PC.std_y(0) ** 2 * (np.abs(np.diag(sym(X2, Z2, th)["full"])) + q + np.exp(th[0]))
    _check_plain(got, dev, terms, "DeviceModel (largest LDS)")


# ------------------------------------------------------------------ 2. marginal with ATE
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("B", PC.ATE_BS)
def test_batch_predict_marginal_ate_matches_oracle_and_device_model(A, O, kernel, B):
    p = PC.ATE_P
    ms = PC.models(PC.ATE_NS, PC.ATE_NXS, p, B, PC.ATE_SEED0)
    bm = _resident(A, kernel, ms, p, B)
    got = _marginal(bm, ms)
    plain = _marginal(bm, ms, ate=False)
    bm.close()
    for j, m in enumerate(ms):
        (y, X, Z, th0, sy), X2, Z2 = m
        th = PC.theta_now(th0, mix=False)
        zx = PC.treated(X2.shape[0])
        ref, terms = PC.oracle_marginal(O, kernel, m, th, zx, PC.std_y(j), PC.std_Z(j))
        dm = A.DeviceModel(kernel, y.size, p, B)
        dm.set_data(y, X, Z, sy)
        dm.para_update(2, th0.copy())
        dev = dm.predict_marginal(th, X2, PC.dbasis(Z2), zx, PC.std_y(j), PC.std_Z(j), True)
        dm.close()
        for what, r in (("oracle", ref), ("DeviceModel", dev)):
            close(got[j]["map"], r["map"], check=f"batch marginal map vs {what}")
            err = np.abs(got[j]["var"] - r["var"]) / terms
            record_error(f"batch marginal var vs {what}: max |err| / terms", np.max(err), VAR_TOL)
            assert np.all(err <= VAR_TOL), (what, np.max(err))
            for k in ("ate", "att", "atu"):
                close(got[j][k]["map"], r[k]["map"], check=f"batch {k} map vs {what}")
                close(got[j][k]["var"], r[k]["var"], 1e-6, 1e-10, check=f"batch {k} var vs {what}")
                sd = np.sqrt(abs(ref[k]["var"]))
                scale = abs(ref[k]["map"]) + 1.96 * sd
                e = np.max(np.abs(got[j][k]["ci"] - r[k]["ci"]))
                record_error(f"batch {k} ci vs {what}: max |err| / (|map| + 1.96 sd)", e / scale, CI_TOL)
                assert e <= CI_TOL * scale, (what, k, got[j][k]["ci"], r[k]["ci"])
        assert "ate" not in plain[j]
        _same(plain[j], {q: got[j][q] for q in KEYS})


# ------------------------------------------------------------------ 3. empty groups
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_predict_marginal_empty_groups(A, O, kernel):
    p, B = PC.ATE_P, PC.EDGE_B
    ms = PC.models(PC.ATE_NS, PC.ATE_NXS, p, B, PC.ATE_SEED0)
    cases = ["none_treated", "all_treated", "third"]
    bm = _resident(A, kernel, ms, p, B)
    got = _marginal(bm, ms, cases)
    ordinary = _marginal(bm, ms)
    bm.close()
    for j in (0, 1):
        th = PC.theta_now(ms[j][0][3], mix=False)
        zx = PC.treated(PC.ATE_NXS[j], cases[j])
        ref, _ = PC.oracle_marginal(O, kernel, ms[j], th, zx, PC.std_y(j), PC.std_Z(j))
        close(got[j]["map"], ref["map"])
        _check_avg_edge(got[j], ref, cases[j])
    _same(got[2], ordinary[2])


# ------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_predict_is_bitwise_independent_of_batch_and_position(A, kernel):
    p, B = PC.ATE_P, PC.EDGE_B
    ms = PC.models(PC.ATE_NS, PC.ATE_NXS, p, B, PC.ATE_SEED0)
    big = PC.models((200, 40), (35, 5), p, B, seed0=50)
    me = ms[1]

    def run(group, pos, nmax=None):
        bm = _resident(A, kernel, group, p, B, nmax=nmax)
        outs = []
        for _ in range(2):  # the same call twice
            M = len(group)
            pl = bm.predict(_thetas(group), [m[1] for m in group], [m[2] for m in group],
                            [PC.mean_y(1)] * M, [PC.std_y(1)] * M)
            mg = bm.predict_marginal(_thetas(group, mix=False), [m[1] for m in group],
                                     [PC.dbasis(m[2]) for m in group],
                                     [PC.treated(m[1].shape[0]) for m in group],
                                     [PC.std_y(1)] * M, [PC.std_Z(1)] * M, True)
            outs.append((pl[pos], mg[pos]))
        bm.close()
        _same(outs[0][0], outs[1][0])
        _same(outs[0][1], outs[1][1])
        return outs[0]

    alone = run([me], 0)
    assert np.all(np.isfinite(alone[0]["var"])) and np.isfinite(alone[1]["ate"]["var"])
    for group, pos, nmax in (([me, ms[0], ms[2]], 0, None), ([big[0], ms[2], me, big[1], ms[0]], 2, 256)):
        other = run(group, pos, nmax)
        _same(other[0], alone[0])
        _same(other[1], alone[1])


# ------------------------------------------------------------------ 5. M > CUs
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_predict_more_workgroups_than_cus(A, kernel):
    m = PC.models((33,), (9,), 2, 3)[0]
    one = _resident(A, kernel, [m], 2, 3)
    ref = _plain(one, [m])[0]
    one.close()
    M = 300
    bm = _resident(A, kernel, [m] * M, 2, 3)
    got = bm.predict(_thetas([m] * M), [m[1]] * M, [m[2]] * M, PC.mean_y(0), PC.std_y(0))
    bm.close()
    assert np.all(np.isfinite(ref["var"]))
    for j in range(M):
        _same(got[j], ref)


# ------------------------------------------------------------------ 6. not positive definite
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_predict_not_positive_definite_neighbour(A, kernel):
    p, B = C.SING_P, C.SING_B
    sing = [c[1] for c in C.singular_cases()]
    healthy = C.problems(C.HEALTHY_N, p, B)
    probs = [sing[0], healthy[0], sing[1], healthy[1], sing[2]]
    bad, good = (0, 2, 4), (1, 3)
    from additivecausalexpansion_amd.synthetic import make_problem
    ms = [(q, *(np.asfortranarray(v[:5 + 6 * j]) for v in make_problem(40, p, B, seed=300 + j)[1:3]))
          for j, q in enumerate(probs)]
    bm = _resident(A, kernel, ms, p, B, it=1)
    th = _thetas(ms)
    args = ([m[1] for m in ms], [m[2] for m in ms], 0.2, 1.3)
    got = bm.predict(th, *args)
    zxs = [PC.treated(m[1].shape[0]) for m in ms]
    mg = bm.predict_marginal(th, args[0], [PC.dbasis(m[2]) for m in ms], zxs, 1.3, 0.9, True)
    for j in bad:
        for k in KEYS:
            assert np.all(np.isnan(got[j][k])) and np.all(np.isnan(mg[j][k])), (j, k)
        for k in ("ate", "att", "atu"):
            assert all(np.all(np.isnan(mg[j][k][q])) for q in KEYS), (j, k)
    clean = _resident(A, kernel, [ms[j] for j in good], p, B, it=1)
    sub = lambda v: [v[j] for j in good]  # noqa: E731
    got_c = clean.predict(np.asfortranarray(th[:, list(good)]), sub(args[0]), sub(args[1]), 0.2, 1.3)
    mg_c = clean.predict_marginal(np.asfortranarray(th[:, list(good)]), sub(args[0]),
                                  [PC.dbasis(m[2]) for m in sub(ms)], sub(zxs), 1.3, 0.9, True)
    clean.close()
    for k, j in enumerate(good):
        assert np.all(np.isfinite(got[j]["var"]))
        _same(got[j], got_c[k])
        _same(mg[j], mg_c[k])
    # a valid inverse installed in a singular model's slot clears its mark
    bm.set_inverse(0, np.eye(ms[0][0][0].size))
    again = bm.predict(th, *args)
    bm.close()
    assert all(np.all(np.isfinite(again[0][k])) for k in KEYS)
    assert np.all(np.isnan(again[2]["map"]))
    for j in good:
        _same(again[j], got[j])


# ------------------------------------------------------------------ 7. set_inverse
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_set_inverse_round_trip_and_oracle_inverse(A, O, kernel):
    ns, nxs, p, B = PC.PLAIN_CASES[0]
    ms = PC.models(ns, nxs, p, B)
    bm = _resident(A, kernel, ms, p, B)
    before = _plain(bm, ms)
    mg_before = _marginal(bm, ms)
    for j in range(len(ms)):
        bm.set_inverse(j, bm.inverse(j))
    after = _plain(bm, ms)
    mg_after = _marginal(bm, ms)
    bm.close()
    for j in range(len(ms)):
        _same(after[j], before[j])
        _same(mg_after[j], mg_before[j])
    fresh = A.BatchModel(kernel, len(ms), max(ns), p, B)
    for j, (prob, _, _) in enumerate(ms):
        fresh.set_data(j, prob[0], prob[1], prob[2], prob[4])
        fresh.set_inverse(j, PC.oracle_inverse(O, kernel, prob))
    got = _plain(fresh, ms)
    fresh.close()
    for j, m in enumerate(ms):
        ref, terms = PC.oracle_plain(O, kernel, m, PC.theta_now(m[0][3]), PC.mean_y(j), PC.std_y(j))
        _check_plain(got[j], ref, terms, "oracle (installed inverse)")


# ------------------------------------------------------------------ 8. after train
@pytest.mark.parametrize("kernel", KERNELS)
def test_predict_ace_batch_after_train_matches_predict_ace(A, kernel):
    from additivecausalexpansion_amd.synthetic import readme_data
    from additivecausalexpansion_amd.train import _prepare
    data = [readme_data(seed=21 + j, n=n) for j, n in enumerate((300, 240, 270))]
    kw = dict(kernel=kernel, basis="cubic", n_knots=2, optimizer="Nadam", maxiter=25, tol=1e-4,
              learning_rate=0.01, verbose=False)
    fits = A.ace_train_batch([d[0] for d in data], [d[1] for d in data], [d[2] for d in data], **kw)
    refs = [A.ace_train(y, X, Z, native_loop=True, **kw) for y, X, Z in data]
    got = A.predict_ace_batch(fits)
    gm = A.predict_ace_batch(fits, marginal=True, return_average_treatments=True)
    for j, (fit, ref) in enumerate(zip(fits, refs)):
        for what, f in (("predict_ace on the batch fit", fit), ("predict_ace on ace_train's fit", ref)):
            pr = A.predict_ace(f)
            pm = A.predict_ace(f, marginal=True, return_average_treatments=True)
            for k in ("map", "ci"):  # (close records the share of the bound that is used)
                close(got[j][k], pr[k], 1e-4, 1e-6, check=f"predict_ace_batch {k} vs {what}")
                close(gm[j][k], pm[k], 1e-4, 1e-6, check=f"predict_ace_batch marginal {k} vs {what}")
    # fits of ace_train (the inverse read from their device models) batch as well
    got_r = A.predict_ace_batch(refs)
    for j, ref in enumerate(refs):
        close(got_r[j]["map"], A.predict_ace(ref)["map"], 1e-4, 1e-6)
    # out of sample, one treatment value for all points
    rng = np.random.default_rng(9)
    newXs = [np.column_stack([rng.uniform(1, 2, 11 + j), rng.uniform(-1, 1, 11 + j)]) for j in range(3)]
    out = A.predict_ace_batch(fits, newXs=newXs, newZs=1)
    for j, fit in enumerate(fits):
        pr = A.predict_ace(fit, newX=newXs[j], newZ=1)
        close(out[j]["map"], pr["map"], 1e-4, 1e-6, check="predict_ace_batch out of sample map")
        close(out[j]["ci"], pr["ci"], 1e-4, 1e-6, check="predict_ace_batch out of sample ci")
    # BatchModel.predict right after train uses each model's own last
    # para_update: the inverses ace_train_batch read from an equal batch
    prep = [_prepare(y, X, Z, None, "cubic", 2, None, 20.0, False) for y, X, Z in data]
    px, B = prep[0][3], prep[0][6].dim()
    bm = A.BatchModel(kernel, 3, 300, px, B)
    theta = np.empty((2 + B * (px + 1), 3), order="F")
    for j, q in enumerate(prep):
        bm.set_data(j, q[0], q[1], q[6].B, q[4][0, 1])
        theta[:, j] = q[7]
    stats, its, conv, status = bm.train(theta, "Nadam", 0.01, maxiter=25, tol=1e-4)
    assert np.all(status == 0)
    direct = bm.predict(theta, [q[1] for q in prep], [q[6].testbasis(q[2])["B"] for q in prep],
                        [q[4][0, 0] for q in prep], [q[4][0, 1] for q in prep])
    bm.close()
    for j in range(3):
        assert np.array_equal(theta[:, j], fits[j]["Kernel"].parameters)
        _same(direct[j], got[j])


@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_predict_after_models_stopped_on_their_own(A, kernel):
    """test_batch_gpu.test_batch_models_stop_on_their_own's configuration (the
    three models stop at different iterations before maxiter): prediction right
    after train uses every model's inverse of its own last para_update -- the
    one a batch of that model alone ends with, and the one inverse(j) reports
    (which that test holds to the oracle's at theta_{T-1})."""
    from additivecausalexpansion_amd.synthetic import make_problem
    tol, maxiter, lr, p, B = 0.9, 30, 0.05, 2, 3
    probs = [make_problem(n, p, B, seed=s) for n, s in ((60, 1), (90, 2), (130, 3))]
    ms = [(q, *(np.asfortranarray(v[:12 + 5 * j]) for v in make_problem(40, p, B, seed=400 + j)[1:3]))
          for j, q in enumerate(probs)]

    def trained(group):
        bm = A.BatchModel(kernel, len(group), max(m[0][0].size for m in group), p, B)
        for j, (q, _, _) in enumerate(group):
            bm.set_data(j, q[0], q[1], q[2], q[4])
        th = np.asfortranarray(np.column_stack([m[0][3] for m in group]))
        _, its, conv, status = bm.train(th, "Nadam", lr, maxiter=maxiter, tol=tol)
        assert np.all(status == 0) and np.all(conv)
        M = len(group)
        pl = bm.predict(th, [m[1] for m in group], [m[2] for m in group], 0.2, 1.3)
        mg = bm.predict_marginal(th, [m[1] for m in group], [PC.dbasis(m[2]) for m in group],
                                 [PC.treated(m[1].shape[0]) for m in group], 1.3, 0.9, True)
        invs = [bm.inverse(j) for j in range(M)]
        bm.close()
        return th, its, pl, mg, invs

    th, its, pl, mg, invs = trained(ms)
    assert len(set(its)) == 3 and max(its) < maxiter, its
    for j, m in enumerate(ms):
        th1, its1, pl1, mg1, _ = trained([m])
        assert its1[0] == its[j] and np.array_equal(th1[:, 0], th[:, j])
        assert np.all(np.isfinite(pl[j]["var"]))
        _same(pl1[0], pl[j])
        _same(mg1[0], mg[j])
    fresh = A.BatchModel(kernel, 3, 130, p, B)
    for j, (q, _, _) in enumerate(ms):
        fresh.set_data(j, q[0], q[1], q[2], q[4])
        fresh.set_inverse(j, invs[j])
    again = fresh.predict(th, [m[1] for m in ms], [m[2] for m in ms], 0.2, 1.3)
    fresh.close()
    for j in range(3):
        _same(again[j], pl[j])


# ------------------------------------------------------------------ 9. argument errors
def test_batch_predict_argument_errors(A):
    ms = PC.models((40, 20), (5, 6), 2, 3)
    bm = A.BatchModel("SE", 2, 40, 2, 3)
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        bm.set_inverse(0, np.eye(40))  # before set_data
    for j, (prob, _, _) in enumerate(ms):
        bm.set_data(j, prob[0], prob[1], prob[2], prob[4])
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        _plain(bm, ms)  # neither a para_update nor a set_inverse
    bm.set_inverse(0, np.eye(40))
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        _plain(bm, ms)  # model 1 still has none
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        bm.set_inverse(2, np.eye(20))  # j = M
    bm.para_update(2, np.asfortranarray(np.column_stack([m[0][3] for m in ms])))
    assert np.all(np.isfinite(_plain(bm, ms)[1]["var"]))
    empty = [ms[0], (ms[1][0], ms[1][1][:0], ms[1][2][:0])]
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        _plain(bm, empty)  # off with an empty model
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        _plain(bm, ms[:1])  # a wrong M
    with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
        bm.predict_marginal(_thetas(ms), [m[1] for m in ms], [m[2] for m in ms],
                            [np.full(5, 0.5), np.zeros(6)], 1.0, 1.0, True)  # Z_x not binary
    bm.close()
