#!/usr/bin/env python3
"""Bitwise comparison of two builds of libace_hip.so on the fused model:
two para_update evaluations (gradient, stats, mu) at a C2-shaped problem,
each build in its own process (ACE_LIB_PATH).  Used for bit-identical A/B
switches.  usage: python tools/cmp_libs.py libA.so libB.so [n] [kernel] [what];
CMP_ENV_B="K=V ..." sets environment switches for the second run only.  what =
para_update (default), or cross: predict, coef_cross and predict_marginal_groups
of one fitted model with p = 20, B = 10 at nx = 257 test points (the two-sided
tile kernels; n = 700 is the shape the tests use), or formulas: every output
of every entry point that evaluates a formula of csrc/ace_formulas.h (fused
para_update / train_stats, the device training loop under each optimizer with
the clip firing and off, host-buffer and handle grad / stats, the batched
para_update / train / predict / predict_marginal with ATE, and one ragged batch of n = 16,
17, 33 and 512), both kernels,
compared bit for bit per output at fixed small shapes (n and kernel are not
read), or predict: in the same style, every output of the prediction host
paths (csrc/ace_predict.cpp) and of the handle path's pred_cpp /
pred_marginal_cpp, both kernels at n = 333, p = 2, B = 3 and n = 700, p = 20,
B = 10 with 257 test points (8269 for the two-chunk cases), one simulated
sharded model, and the coefficient paths once more in a process with
ACE_COEF_CHUNK=7; run it as is and with ACE_PRED_TRI=0 in the environment
(both builds then take the full symmetric product), or cv: every output array
of DeviceModel.cv, status included, both kernels, one fitted model at n = 700,
p = 2, B = 3: one call with folds of 1, 15, 16, 17, 33, 64, 100 and 512 rows,
an all-one-row call, and the first call again with ACE_CV_WG_MAX=16."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNIP = """
import sys, numpy as np
sys.path.insert(0, {root!r})
import additivecausalexpansion_amd as A
from additivecausalexpansion_amd.synthetic import make_problem
y, X, Z, th, sy = make_problem({n}, 20, 10, seed=5)
m = A.DeviceModel({kernel!r}, {n}, 20, 10)
m.set_data(y, X, Z, sy)
outs = []
for it in (1, 2):
    g, st, mu = m.para_update(it, th)
    outs += [g, st, np.array([mu])]
    th = th + 0.01 * g / max(1.0, float(np.abs(g).max()))
np.save({out!r}, np.concatenate(outs))
"""
SNIP_CROSS = """
import sys, numpy as np
sys.path.insert(0, {root!r})
import additivecausalexpansion_amd as A
from additivecausalexpansion_amd.synthetic import make_problem
nx = 257
y, X, Z, th, sy = make_problem({n}, 20, 10, seed=5)
m = A.DeviceModel({kernel!r}, {n}, 20, 10)
m.set_data(y, X, Z, sy)
m.para_update(2, th.copy())
th = th + 0.02
th[1] = 0.13
_, X2, Z2, _, _ = make_problem(nx, 20, 10, seed=6)
dZ2 = np.asfortranarray(Z2 * 0.7 + 0.1)
pr = m.predict(th, X2, Z2, 0.3, 1.7)
g = m.predict_marginal_groups(th, X2, dZ2, 1.7, 0.8, 17, (np.arange(nx) % 17).astype(np.int32))
outs = [pr["map"], pr["var"], m.coef_cross(th, X2), g["gcov"], g["gsum"], g["map"], g["var"]]
np.save({out!r}, np.concatenate([np.ravel(o) for o in outs]))
"""
# Shapes: the smallest at which every branch of the shared functions is taken
# (exact zeros in Z on either side of a pair for the Q7 rules, n_j and nx_j on
# either side of a 16-row block / a 32-point pass, the PM = 4 and PM = 64
# buckets, B = 1 and B > 1, each optimizer, the clip firing and off).
SNIP_FORMULAS = """
import sys, numpy as np
sys.path.insert(0, {root!r})
import additivecausalexpansion_amd as A
from additivecausalexpansion_amd import native as N
from additivecausalexpansion_amd.model import BatchModel
from additivecausalexpansion_amd.synthetic import make_problem
out = {{}}
# Every device object lives inside run(): a handle left at script level is
# released at interpreter exit after the context it belongs to (the script's
# globals form a cycle with its functions, and the collector finalises the
# older context first), and ace_dmat_free then writes into the freed context.
def run():
    def put(name, *arrs):
        for i, a in enumerate(arrs):
            out[name + "/" + str(i)] = np.ravel(np.asarray(a, dtype=np.float64))
    def problem(n, p, B, seed):
        y, X, Z, th, sy = make_problem(n, p, B, seed=seed)
        Z = np.array(Z, order="F")
        if B > 1:
            Z[3::7, 0] = 0.0   # exact zeros: the Q7 rules
            Z[5::11, :] = 0.0
        return y, X, Z, th + 0.05 * np.sin(np.arange(th.size)), sy
    OPTS = [(o, c) for o in ("NAG", "Adam", "Nadam") for c in (True, False)]
    for kernel in ("SE", "Matern32"):
        # fused model: para_update, train_stats, the inverse
        y, X, Z, th, sy = problem(97, 2, 5, 1)
        m = A.DeviceModel(kernel, 97, 2, 5)
        m.set_data(y, X, Z, sy)
        t = th.copy()
        for it in (1, 2):
            g, st, mu = m.para_update(it, t)
            put(kernel + "/fused/it" + str(it), g, st, [mu], t)
            t = t + 0.01 * g / max(1.0, float(np.abs(g).max()))
        put(kernel + "/fused/inverse", m.inverse())
        put(kernel + "/fused/train_stats", m.train_stats(t))
        m.close()
        # the device training loop
        y, X, Z, th, sy = problem(60, 3, 4, 2)
        for opt, clip in OPTS:
            m = A.DeviceModel(kernel, 60, 3, 4)
            m.set_data(y, X, Z, sy)
            t = th.copy()
            stats, iters, conv = m.train(t, optimizer=opt, learning_rate=0.003, momentum=0.9,
                                         norm_clip=clip, clip_at=0.5, maxiter=6)
            put(kernel + "/train/" + opt + "/clip" + str(int(clip)), t, stats, [iters, conv], m.inverse())
            m.close()
        # host buffers and handles: grad, stats
        y, X, Z, th, sy = problem(97, 2, 5, 3)
        sym = N.kernmat_SE_symmetric_cpp if kernel == "SE" else N.kernmat_Matern32_symmetric_cpp
        grad = N.grad_SE_cpp if kernel == "SE" else N.grad_Matern_cpp
        for dev in (False, True):
            K = sym(X, Z, th, device=dev)
            inv = N.invkernel_cpp(K["full"], th[0])
            mu = N.mu_solution_cpp(y, inv["inv"])
            t = th.copy()
            t[1] = mu
            st = np.zeros(2)
            g = grad(y, X, Z, K["full"], K["elements"], inv["inv"], inv["eigenval"], t, st, 5, sy)
            st2 = N.stats_cpp(y, K["full"], inv["inv"], inv["eigenval"], mu, sy)
            put(kernel + "/abi/dev" + str(int(dev)), g, st, st2, [mu], inv["eigenval"])
        # the batched engine
        ns, nxs = (15, 16, 33), (1, 32, 33)
        for p, B in ((3, 1), (3, 4), (33, 1), (33, 4)):
            tag = kernel + "/batch/p" + str(p) + "B" + str(B)
            probs = [problem(n, p, B, 10 + j) for j, n in enumerate(ns)]
            th0 = np.asfortranarray(np.column_stack([q[3] for q in probs]))
            def model():
                bm = BatchModel(kernel, 3, 33, p, B)
                for j, q in enumerate(probs):
                    bm.set_data(j, q[0], q[1], q[2], q[4])
                return bm
            bm = model()
            T = th0.copy(order="F")
            for it in (1, 2):
                g, st, mu = bm.para_update(it, T)
                put(tag + "/it" + str(it), g, st, mu, T)
                T = np.asfortranarray(T + 0.01 * g / max(1.0, float(np.abs(g).max())))
            put(tag + "/inverse", *[bm.inverse(j) for j in range(3)])
            tests = [problem(40, p, B, 20 + j) for j in range(3)]
            X2s = [np.asfortranarray(q[1][:nx]) for q, nx in zip(tests, nxs)]
            Z2s = [np.asfortranarray(q[2][:nx]) for q, nx in zip(tests, nxs)]
            for q in Z2s:
                if B > 1:
                    q[1::5, -1] = 0.0
            pr = bm.predict(T, X2s, Z2s, [0.3, -0.2, 0.1], [1.7, 0.9, 1.1])
            put(tag + "/predict", *[r[k] for r in pr for k in ("map", "ci", "var")])
            dZ2s = [np.asfortranarray(q * 0.7 + 0.1) for q in Z2s]
            for q in dZ2s:
                if B > 1:
                    q[1::5, -1] = 0.0
            zxs = [(np.arange(nx) % 3 == 0).astype(np.float64) for nx in nxs]
            for ate in (False, True):
                pm = bm.predict_marginal(T, X2s, dZ2s, zxs, [1.7, 0.9, 1.1], [0.8, 1.2, 1.0],
                                         calculate_ate=ate)
                put(tag + "/marginal/ate" + str(int(ate)), *[r[k] for r in pm for k in ("map", "ci", "var")])
                if ate:
                    put(tag + "/marginal/avg", *[r[g][k] for r in pm for g in ("ate", "att", "atu")
                                                 for k in ("map", "ci", "var")])
            bm.close()
            for opt, clip in OPTS:
                bm = model()
                T = th0.copy(order="F")
                stats, iters, conv, status = bm.train(T, optimizer=opt, learning_rate=0.003, momentum=0.9,
                                                      norm_clip=clip, clip_at=0.5, maxiter=6)
                put(tag + "/train/" + opt + "/clip" + str(int(clip)), T, stats, iters, conv, status,
                    *[bm.inverse(j) for j in range(3)])
                bm.close()
        # one ragged batch over the workgroup sweep's block edges and its row limit
        nr = (16, 17, 33, 512)
        probs = [problem(n, 3, 4, 30 + j) for j, n in enumerate(nr)]
        bm = BatchModel(kernel, len(nr), max(nr), 3, 4)
        for j, q in enumerate(probs):
            bm.set_data(j, q[0], q[1], q[2], q[4])
        T = np.asfortranarray(np.column_stack([q[3] for q in probs]))
        for it in (1, 2):
            g, st, mu = bm.para_update(it, T)
            put(kernel + "/batch/ragged/it" + str(it), g, st, mu, T)
            T = np.asfortranarray(T + 0.01 * g / max(1.0, float(np.abs(g).max())))
        put(kernel + "/batch/ragged/inverse", *[bm.inverse(j) for j in range(len(nr))])
        bm.close()
run()
np.savez({out!r}, **out)
"""
# Cross-validation from the resident inverse (csrc/ace_cv.hip): one fitted
# model per kernel; folds on the workgroup sweep's block edges, at an odd tile
# count (where its 2 x 2 turn clamps) and at 512 rows (LDS above 64 KB); the
# elementwise class; and the first call again with every fold above 16 rows
# sent through the whole-chip sweep.
SNIP_CV = """
import os, sys, numpy as np
sys.path.insert(0, {root!r})
import additivecausalexpansion_amd as A
from additivecausalexpansion_amd.synthetic import make_problem
out = {{}}
def run():
    n, p, B = 700, 2, 3
    rng = np.random.default_rng(11)
    folds = [np.sort(rng.permutation(n)[:m]) for m in (1, 15, 16, 17, 33, 64, 100, 512)]
    for kernel in ("SE", "Matern32"):
        y, X, Z, th, sy = make_problem(n, p, B, seed=5)
        m = A.DeviceModel(kernel, n, p, B)
        m.set_data(y, X, Z, sy)
        m.para_update(2, th.copy())
        def put(name, res):
            for k in sorted(res):
                out[kernel + "/" + name + "/" + k] = np.ravel(np.asarray(res[k]))
        put("folds", m.cv(th, folds, 0.3, sy))
        put("loo", m.cv(th, [np.array([i]) for i in range(n)], 0.3, sy))
        os.environ["ACE_CV_WG_MAX"] = "16"  # read per call
        put("folds_wg16", m.cv(th, folds, 0.3, sy))
        del os.environ["ACE_CV_WG_MAX"]
        m.close()
run()
np.savez({out!r}, **out)
"""
# Every output of every entry point that goes through csrc/ace_predict.cpp's
# host paths, and the handle path's two callers of its pipeline.  The part
# named by CMP_PART runs: "all", or "coef7" -- the coefficient paths alone, in
# a process started with ACE_COEF_CHUNK=7 so that their chunk loops run (the
# library reads the switch once per process).
SNIP_PREDICT = """
import os, sys, numpy as np
sys.path.insert(0, {root!r})
import additivecausalexpansion_amd as A
from additivecausalexpansion_amd import native as N
from additivecausalexpansion_amd.synthetic import make_problem
out = {{}}
part = os.environ.get("CMP_PART", "all")
NX, NX2, G = 257, 8192 + 77, 17
def run():
    def put(name, res, keys=None):
        if not isinstance(res, dict):
            res = {{"": res}}
        for k in sorted(keys or res):
            v = res[k]
            if isinstance(v, dict):  # ate / att / atu
                v = np.concatenate([np.ravel(v[q]) for q in ("map", "ci", "var")])
            out[part + "/" + name + ("/" + k if k else "")] = np.ravel(np.asarray(v, dtype=np.float64))
    def points(nx, p, B, seed):
        _, X2, Z2, _, _ = make_problem(nx, p, B, seed=seed)
        Z2 = np.asfortranarray(Z2)
        return X2, Z2, np.asfortranarray(Z2 * 0.7 + 0.1), (np.arange(nx) % 3 == 0).astype(np.float64)
    def fitted(kernel, n, p, B, **kw):
        y, X, Z, th, sy = make_problem(n, p, B, seed=5)
        m = A.DeviceModel(kernel, n, p, B, **kw)
        m.set_data(y, X, Z, sy)
        m.para_update(2, th.copy())   # the resident inverse is at th
        mix = th + 0.02               # kernels at another theta (Q6)
        mix[1] = 0.13
        return m, y, X, Z, th, mix, sy
    for kernel in ("SE", "Matern32"):
        for n, p, B in ((333, 2, 3), (700, 20, 10)):
            tag = kernel + "/n" + str(n)
            m, y, X, Z, th, mix, sy = fitted(kernel, n, p, B)
            X2, Z2, dZ2, zx = points(NX, p, B, 6)
            put(tag + "/coef_posterior", m.coef_posterior(mix, X2))
            put(tag + "/coef_cross", m.coef_cross(mix, X2))
            for marg in (False, True):
                put(tag + "/surface/marginal" + str(int(marg)),
                    m.predict_surface(mix, X2, (dZ2 if marg else Z2)[:9], marg, 0.3, 1.7, 0.8))
            if part == "coef7":
                m.close()
                continue
            put(tag + "/predict", m.predict(mix, X2, Z2, 0.3, 1.7))
            put(tag + "/marginal/ate0", m.predict_marginal(mix, X2, dZ2, None, 1.7, 0.8, False))
            put(tag + "/marginal/ate1", m.predict_marginal(th, X2, dZ2, zx, 1.7, 0.8, True))
            lab = (np.arange(NX) % G).astype(np.int32)
            lab[5::13] = -1
            put(tag + "/groups", m.predict_marginal_groups(mix, X2, dZ2, 1.7, 0.8, G, lab))
            put(tag + "/robust", m.robust_treatment(th, X2, dZ2, zx, 1.7, 0.8, n_steps=3),
                ("map", "ci", "var", "thresholds", "level", "avg", "counts"))
            xi = np.asfortranarray(np.random.default_rng(7).standard_normal((NX, 5)))
            for marg in (False, True):
                put(tag + "/joint/marginal" + str(int(marg)),
                    m.predict_joint(th, X2, dZ2 if marg else Z2, 0.3, 1.7, marginal=marg, std_Z=0.8,
                                    jitter=1e-8, xi=xi, return_cov=True, return_factor=True))
            put(tag + "/apply_inverse",
                m.apply_inverse(np.random.default_rng(8).standard_normal((n, 3))))
            if n == 333:  # two chunks; the grouped pass reuses the last one's scratch
                X2b, Z2b, dZ2b, _ = points(NX2, p, B, 9)
                put(tag + "/predict/two_chunks", m.predict(mix, X2b, Z2b, 0.3, 1.7))
                put(tag + "/groups/two_chunks",
                    m.predict_marginal_groups(mix, X2b, dZ2b, 1.7, 0.8, G,
                                              (np.arange(NX2) % G).astype(np.int32)))
            m.close()
            # the handle path: pred_cpp / pred_marginal_cpp over DMat handles
            cross = N.kernmat_SE_cpp if kernel == "SE" else N.kernmat_Matern32_cpp
            sym = N.kernmat_SE_symmetric_cpp if kernel == "SE" else N.kernmat_Matern32_symmetric_cpp
            inv = N.invkernel_cpp(sym(X, Z, th, device=True)["full"], th[0])["inv"]
            put(tag + "/handles/pred",
                N.pred_cpp(y, th[0], 0.13, inv, cross(X2, X, Z2, Z, th, device=True)["full"],
                           sym(X2, Z2, th, device=True)["full"], 0.3, 1.7))
            put(tag + "/handles/marginal",
                N.pred_marginal_cpp(y, zx, th[0], 0.13, inv,
                                    cross(X2, X, dZ2, Z, th, device=True)["elements"],
                                    sym(X2, dZ2, th, device=True)["elements"], 0.0, 1.7, 0.8, True))
    if part == "all":  # one simulated sharded model
        m, y, X, Z, th, mix, sy = fitted("Matern32", 700, 20, 10, world=3, sharded=True)
        X2, Z2, dZ2, zx = points(NX, 20, 10, 6)
        put("sharded/predict", m.predict(mix, X2, Z2, 0.3, 1.7))
        put("sharded/marginal/ate1", m.predict_marginal(th, X2, dZ2, zx, 1.7, 0.8, True))
        m.close()
run()
np.savez({out!r}, **out)
"""
SNIPS = {"para_update": SNIP, "cross": SNIP_CROSS, "formulas": SNIP_FORMULAS,
         "predict": SNIP_PREDICT, "cv": SNIP_CV}
# the processes each build runs in for a mode: (extra environment, ...)
PARTS = {"predict": ({"CMP_PART": "all"}, {"CMP_PART": "coef7", "ACE_COEF_CHUNK": "7"})}
NAMED = ("formulas", "predict", "cv")  # named outputs in an npz, a verdict per output


def bits_equal(a, b):
    """Equal bit for bit (a NaN equals only the same NaN)."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    a, b = sys.argv[1], sys.argv[2]
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    kernel = sys.argv[4] if len(sys.argv) > 4 else "Matern32"
    what = sys.argv[5] if len(sys.argv) > 5 else "para_update"
    res = []
    with tempfile.TemporaryDirectory() as d:
        for i, lib in enumerate((a, b)):
            got = {}
            for j, extra in enumerate(PARTS.get(what, ({},))):
                out = os.path.join(d, f"o{i}_{j}." + ("npz" if what in NAMED else "npy"))
                env = dict(os.environ, ACE_LIB_PATH=os.path.abspath(lib), **extra)
                if i == 1 and os.environ.get("CMP_ENV_B"):  # "K=V ..." for the second run only
                    env.update(kv.split("=", 1) for kv in os.environ["CMP_ENV_B"].split())
                subprocess.run([sys.executable, "-c",
                                SNIPS[what].format(root=ROOT, n=n, kernel=kernel, out=out)],
                               env=env, check=True, timeout=300)
                if what in NAMED:
                    got.update(np.load(out))
            res.append(got if what in NAMED else np.load(out))
    if what in NAMED:
        keys = sorted(set(res[0]) | set(res[1]))
        diff = [k for k in keys if k not in res[0] or k not in res[1]
                or not bits_equal(res[0][k], res[1][k])]
        for k in keys:
            v = res[1].get(k)
            print(f"{k}: {'DIFFERS' if k in diff else 'bit-identical'} "
                  f"({0 if v is None else v.size} values, "
                  f"{0 if v is None else int(np.sum(~np.isfinite(v)))} non-finite)")
        nval = sum(v.size for v in res[1].values())
        print(f"{what}: {len(keys) - len(diff)} of {len(keys)} outputs bit-identical "
              f"({nval} values); differing: {diff if diff else 'none'}")
        sys.exit(0 if not diff else 1)
    same = np.array_equal(res[0], res[1])
    rel = float(np.max(np.abs(res[0] - res[1]) / np.maximum(np.abs(res[0]), 1e-300)))
    print(f"{what} n={n} {kernel}: bit-identical={same} max rel diff={rel:.3e} finite={bool(np.all(np.isfinite(res[1])))}")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
