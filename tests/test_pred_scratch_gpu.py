"""The retained prediction scratch (csrc/ace_predict.cpp, with_pred_scratch)
carries no state from one kind of call to the next: on one context and one
model, each of predict, coef_posterior, predict_joint,
predict_marginal_groups and predict again returns, bit for bit, what the same
call returns on a fresh context and model, although each finds the buffers
the one before it left (sized and filled for other shapes)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KERNEL, N, P, B = "SE", 333, 2, 3


def _points(nx, seed):
    from additivecausalexpansion_amd.synthetic import make_problem
    _, X2, Z2, _, _ = make_problem(nx, P, B, seed=seed)
    return X2, np.asfortranarray(Z2)


def _calls():
    Xa, Za = _points(90, 6)
    Xb, Zb = _points(257, 7)
    Xc, Zc = _points(40, 8)
    dZb = np.asfortranarray(Zb * 0.7 + 0.1)
    label = (np.arange(257) % 4).astype(np.int32)
    xi = np.random.default_rng(7).standard_normal((40, 5))
    predict = ("predict", lambda m, th: m.predict(th, Xa, Za, 0.3, 1.7))
    return [
        predict,
        ("coef_posterior", lambda m, th: m.coef_posterior(th, Xb)),
        ("predict_joint", lambda m, th: m.predict_joint(th, Xc, Zc, 0.3, 1.7, jitter=1e-8, xi=xi,
                                                        return_cov=True, return_factor=True)),
        ("predict_marginal_groups",
         lambda m, th: m.predict_marginal_groups(th, Xb, dZb, 1.7, 0.8, 4, label)),
        predict,
    ]


def test_scratch_carries_no_state_between_call_kinds():
    import additivecausalexpansion_amd as A
    from additivecausalexpansion_amd.synthetic import make_problem
    y, X, Z, th, sy = make_problem(N, P, B, seed=5)

    def fitted():
        ctx = A.Context()
        m = A.DeviceModel(KERNEL, N, P, B, ctx=ctx)
        m.set_data(y, X, Z, sy)
        m.para_update(2, th.copy())
        return ctx, m

    ctx, m = fitted()
    differing = []
    for step, (name, call) in enumerate(_calls()):
        got = call(m, th)
        fctx, fm = fitted()
        want = call(fm, th)
        fm.close()
        fctx.close()
        assert sorted(got) == sorted(want)
        for k in sorted(want):
            a = np.ravel(np.asarray(got[k], dtype=np.float64))
            b = np.ravel(np.asarray(want[k], dtype=np.float64))
            assert np.all(np.isfinite(b)), (step, name, k)
            if a.shape != b.shape or not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
                differing.append((step, name, k, float(np.max(np.abs(a - b)))))
    m.close()
    ctx.close()
    assert not differing, differing
