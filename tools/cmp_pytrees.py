#!/usr/bin/env python3
"""Bitwise comparison of two trees of the Python layer on one libace_hip.so:
every leaf of every result of the public API, each tree in its own fresh
process (sys.path[0] = the tree, ACE_LIB_PATH = the one library).  For a
refactor of the Python layer that must not move a bit, a dtype, a shape or a
memory order.

usage: python tools/cmp_pytrees.py TREE_A TREE_B [--host-only | --time [ROUNDS]]
       [--lib PATH]   (default: TREE_B's additivecausalexpansion_amd/libace_hip.so)

Default: both kernels, the smallest shapes that reach every branch --
ace_train (Python loop and native loop, maxiter 6, n = 130, p = 2, binary Z
with the linear basis and continuous Z with ns and 2 knots), predict_ace in
the four newX / newZ cases (marginal off / on, ATE for the binary fit, 37 test
points), posterior_draws, cross_validate (K-fold, loo, groups, overlapping
folds), robust_treatment, coef_posterior, response_surface,
average_coef_posterior, average_response, the batched pair (M = 3, n = 16,
17, 33), the reference call surface with host buffers and with handles at
n = 70, potrf_lower and cv_from_inverse (both open a context) -- plus
everything --host-only runs.
--host-only: the routines that need no GPU (optimizers, norm_clip_cpp,
normalize_*, ncs_basis*, coef_contract, coef_group_contract, robust_levels,
zero_pattern_order).
Each leaf is compared by Python type, dtype, shape, contiguity flags and raw
bytes; exit status 1 and the leaf's name on any difference.

--time: Python overhead per call instead.  ROUNDS (default 5) fresh processes
per tree, alternating; each warms up, then times 2000 DeviceModel.para_update
(2, theta) calls at n = 64, p = 2, B = 3 and 200 predict calls at 37 test
points in blocks, and reports its median block.  Prints every process's
median, and each tree's median and range of those."""
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

CHILD = r"""
import json, os, sys, time
import numpy as np
tree, mode, out_path = sys.argv[1:4]
sys.path[0] = tree
import additivecausalexpansion_amd as A
from additivecausalexpansion_amd import native as N
from additivecausalexpansion_amd.synthetic import make_problem
assert os.path.dirname(os.path.dirname(os.path.abspath(A.__file__))) == os.path.abspath(tree)
out, meta = {}, {}


def put(name, v):
    if callable(v):  # a call that may refuse its input: the message is the leaf
        try:
            v = v()
        except A.AceError as e:
            v = "AceError: " + str(e)
    if isinstance(v, dict):
        meta[name] = type(v).__name__ + " " + " ".join(map(str, v))  # the keys, in order
        for k in v:
            put(name + "/" + str(k), v[k])
    elif isinstance(v, (list, tuple)):
        meta[name] = type(v).__name__ + " " + str(len(v))
        for i, x in enumerate(v):
            put(name + "/" + str(i), x)
    elif v is None or isinstance(v, str):
        meta[name] = repr(v)
    elif hasattr(v, "parameters") and hasattr(v, "invKmatn"):  # a kernel object
        put(name, {"kernel": v.kernel, "p": v.p, "B": v.B, "parameters": v.parameters,
                   "from_model": v._inv_from_model, "invKmatn": np.asarray(v.invKmatn)})
    elif hasattr(v, "testbasis"):  # a basis object
        put(name, {"B": v.B, "dB": v.dB, "myknots": getattr(v, "myknots", None)})
    else:
        a = np.asarray(v)
        out[name] = a
        meta[name] = "%s c=%d f=%d" % (type(v).__name__, a.flags.c_contiguous, a.flags.f_contiguous)


def raw_data(n, p, binary, seed):
    # raw (y, X, Z) in make_problem's style: y = sin(3 x1) + x2 z + noise
    rng = np.random.default_rng(seed)
    X = 3.0 + 2.0 * rng.uniform(-1.0, 1.0, size=(n, p))
    z = (rng.uniform(size=n) < 0.4).astype(np.float64) if binary else 5.0 + 2.0 * rng.normal(size=n)
    y = 10.0 + np.sin(3 * X[:, 0]) + X[:, 1] * z + rng.normal(scale=0.1, size=n)
    return y, X, z


def host_only():
    rng = np.random.default_rng(1)
    g0 = rng.normal(size=7)
    for name, step in (("Nesterov", lambda s, it: N.Nesterov_cpp(0.01, 0.9, s["nu"], s["g"], s["para"])),
                       ("Adam", lambda s, it: N.Adam_cpp(it, 0.01, 0.9, 0.999, 1e-8, s["m"], s["v"], s["g"], s["para"])),
                       ("Nadam", lambda s, it: N.Nadam_cpp(it, 0.01, 0.9, 0.999, 1e-8, s["m"], s["v"], s["g"], s["para"]))):
        s = {"nu": np.zeros(7), "m": np.zeros(7), "v": np.zeros(7), "para": np.linspace(-1, 1, 7)}
        for it in (1, 2, 3):
            s["g"] = g0 * it
            put("host/%s/it%d/ok" % (name, it), step(s, it))
            put("host/%s/it%d/state" % (name, it), {k: a.copy() for k, a in s.items()})
    for flag in (True, False):
        g = 3.0 * g0
        put("host/norm_clip/%d/ret" % flag, N.norm_clip_cpp(flag, g, 1.0))
        put("host/norm_clip/%d/grads" % flag, g)
    y, X, z = raw_data(23, 2, False, 2)
    yv, Xf, Zf = y.copy(), np.asfortranarray(X), np.asfortranarray(z.reshape(-1, 1))
    mom = N.normalize_train(yv, Xf, Zf)
    put("host/normalize_train", {"mom": mom, "y": yv, "X": Xf, "Z": Zf})
    X2, Z2 = np.asfortranarray(X[:9] + 0.1), np.asfortranarray(z[:9].reshape(-1, 1) - 0.2)
    put("host/normalize_test/ret", N.normalize_test(X2, Z2, mom))
    put("host/normalize_test", {"X": X2, "Z": Z2})
    kn = np.array([-0.4, 0.1, 0.5, -1.0, 1.0])
    for x in (np.linspace(-1, 1, 11), [0.3, -0.2], np.linspace(-1, 1, 6).reshape(2, 3)):
        put("host/ncs/%d" % np.size(x), {"B": N.ncs_basis(x, kn), "dB": N.ncs_basis_deriv(x, kn)})
    nx, B, nz, G = 6, 3, 4, 3
    mean = rng.normal(size=(nx, B))
    Lc = rng.normal(size=(nx, B, B))
    cov = np.einsum("cij,ckj->cik", Lc, Lc)
    W = rng.normal(size=(nz, B))
    put("host/coef_contract", N.coef_contract(mean, cov, W, 0.3, 1.7, 0.1, 0.01))
    put("host/coef_contract/vectorW", N.coef_contract(mean, cov, W[0], 0.3, 1.7))
    Lg = rng.normal(size=(G * B, G * B))
    gcov = (Lg @ Lg.T).reshape(G, B, G, B, order="F")
    for rc in (False, True):
        put("host/coef_group_contract/%d" % rc,
            N.coef_group_contract(mean[:G], gcov, [4, 0, 2], W, 0.3, 1.7, 0.1, return_cov=rc))
    put("host/robust_levels", N.robust_levels(rng.uniform(size=37), 5))
    Zp = rng.normal(size=(130, 3))
    Zp[::3, 0] = 0.0
    Zp[1::5, 2] = 0.0
    put("host/zero_pattern_order", N.zero_pattern_order(Zp))
    put("host/zero_pattern_order/wide", N.zero_pattern_order(np.ones((5, 33))))


def factor_and_folds():
    # potrf_lower and cv_from_inverse open a context of their own: they need a GPU
    L0 = np.random.default_rng(2).normal(size=(9, 9))
    S = L0 @ L0.T + 9.0 * np.eye(9)
    put("potrf", N.potrf_lower(S, 1e-9))
    put("potrf/lda", N.potrf_lower(np.vstack([S[:5, :5], np.zeros((2, 5))]), lda=7))
    put("potrf/indefinite", N.potrf_lower(-S))
    put("cv_from_inverse", N.cv_from_inverse(S, np.arange(9.0), [[0, 3], [8], np.arange(2, 7)]))
    put("cv_from_inverse/empty_fold", lambda: N.cv_from_inverse(S, np.arange(9.0), [[0, 3], []]))


def call_surface(kernel):
    sym = N.kernmat_SE_symmetric_cpp if kernel == "SE" else N.kernmat_Matern32_symmetric_cpp
    cross = N.kernmat_SE_cpp if kernel == "SE" else N.kernmat_Matern32_cpp
    grad = N.grad_SE_cpp if kernel == "SE" else N.grad_Matern_cpp
    n, p, B, nx = 70, 2, 3, 37
    y, X, Z, th, sy = make_problem(n, p, B, seed=5)
    _, X2, Z2, _, _ = make_problem(nx, p, B, seed=6)
    dZ2 = np.asfortranarray(Z2 * 0.7 + 0.1)
    zx = (np.arange(nx) % 3 == 0).astype(np.float64)
    for dev in (False, True):
        tag = "%s/abi/dev%d" % (kernel, dev)
        K = sym(X, Z, th, device=dev)
        put(tag + "/kernmat_sym", {k: np.asarray(v) for k, v in K.items()})
        inv = N.invkernel_cpp(K["full"], th[0])
        put(tag + "/invkernel", {"eigenval": inv["eigenval"], "inv": np.asarray(inv["inv"])})
        mu = N.mu_solution_cpp(y, inv["inv"])
        put(tag + "/mu_solution", mu)
        t = th.copy()
        t[1] = mu
        st = np.zeros(2)
        put(tag + "/grad", grad(y, X, Z, K["full"], K["elements"], inv["inv"], inv["eigenval"], t, st, B, sy))
        put(tag + "/grad/stats", st)
        put(tag + "/stats", N.stats_cpp(y, K["full"], inv["inv"], inv["eigenval"], np.array([mu]), sy))
        KxX = cross(X2, X, Z2, Z, t, device=dev)
        put(tag + "/kernmat_cross", {k: np.asarray(v) for k, v in KxX.items()})
        put(tag + "/pred", N.pred_cpp(y, t[0], mu, inv["inv"], KxX["full"], sym(X2, Z2, t, device=dev)["full"], 0.3, sy))
        for ate in (False, True):
            put(tag + "/pred_marginal/ate%d" % ate,
                N.pred_marginal_cpp(y, zx, t[0], mu, inv["inv"],
                                    cross(X2, X, dZ2, Z, t, device=dev)["elements"],
                                    sym(X2, dZ2, t, device=dev)["elements"], 0.3, sy, np.array([0.8]), ate))
        del K, inv, KxX


def fits_and_queries(kernel):
    n, p, nx = 130, 2, 37
    for basis, binary in (("linear", True), ("ns", False)):
        y, X, z = raw_data(n, p, binary, 3)
        _, X2, z2 = raw_data(nx, p, binary, 4)
        for loop in (False, True):
            tag = "%s/%s/native%d" % (kernel, basis, loop)
            fit = A.ace_train(y, X, z, kernel=kernel, basis=basis, n_knots=2, maxiter=6, verbose=False,
                              native_loop=loop)
            put(tag + "/fit", fit)
            for case, (nX, nZ) in {"none": (None, None), "Z": (None, np.resize(z2, n)),
                                   "Zlevel": (None, 1.0), "X": (X2, None), "XZ": (X2, z2),
                                   "XZlevel": (X2, 1.0)}.items():
                for marg in (False, True):
                    put("%s/predict/%s/marginal%d" % (tag, case, marg),
                        A.predict_ace(fit, nX, nZ, marginal=marg, return_average_treatments=True))
            put(tag + "/predict/raw", A.predict_ace(fit, X2, z2, normalize=False))
            if loop:
                continue  # the queries below read the same state either way
            for marg in (False, True):
                put("%s/draws/marginal%d" % (tag, marg),
                    lambda: A.posterior_draws(fit, X2, z2, marginal=marg, n_draws=5, return_cov=True,
                                              return_average_treatments=True))
            put(tag + "/draws/xi", lambda: A.posterior_draws(fit, X2, z2, xi=np.ones(nx), jitter=1e-6))
            over = [np.arange(0, 40), np.arange(30, 70), np.arange(60, 100)]  # equal sizes
            for name, kw in (("k4", {"folds": 4}), ("loo", {"folds": "loo"}),
                             ("groups", {"groups": np.arange(n) % 7}), ("overlap", {"folds": over})):
                put(tag + "/cv/" + name, lambda: A.cross_validate(fit, **kw))
            put(tag + "/robust/insample", lambda: A.robust_treatment(fit))
            put(tag + "/robust/newX", lambda: A.robust_treatment(fit, X2, n_steps=3))
            put(tag + "/coef_posterior", A.coef_posterior(fit, X2))
            put(tag + "/coef_posterior/train", A.coef_posterior(fit))
            zg = np.array([0.0, 1.0]) if binary else np.linspace(2.0, 8.0, 5)
            for marg in (False, True):
                put("%s/surface/marginal%d" % (tag, marg), A.response_surface(fit, X2, zg, marginal=marg))
            g3 = np.arange(nx) % 3
            put(tag + "/average_coef", A.average_coef_posterior(fit, X2, groups=g3))
            put(tag + "/average_coef/all", A.average_coef_posterior(fit))
            for marg in (False, True):
                put("%s/average_response/marginal%d" % (tag, marg),
                    A.average_response(fit, zg, X2, groups=g3, marginal=marg, return_cov=True))
            put(tag + "/average_response/all", A.average_response(fit, zg))
            del fit


def batch(kernel):
    ns = (16, 17, 33)
    data = [raw_data(m, 2, True, 20 + j) for j, m in enumerate(ns)]
    tests = [raw_data(5 + j, 2, True, 30 + j) for j in range(3)]
    fits = A.ace_train_batch([d[0] for d in data], [d[1] for d in data], [d[2] for d in data],
                             kernel=kernel, maxiter=6)
    put(kernel + "/batch/fits", fits)
    for marg in (False, True):
        put("%s/batch/predict/marginal%d" % (kernel, marg),
            A.predict_ace_batch(fits, [t[1] for t in tests], [t[2] for t in tests], marginal=marg,
                                return_average_treatments=True))
    put(kernel + "/batch/predict/insample", A.predict_ace_batch(fits))
    put(kernel + "/batch/predict/level", A.predict_ace_batch(fits, None, 1.0, marginal=True))


def timing():
    n, p, B, nx = 64, 2, 3, 37
    y, X, Z, th, sy = make_problem(n, p, B, seed=5)
    _, X2, Z2, _, _ = make_problem(nx, p, B, seed=6)
    m = A.DeviceModel("SE", n, p, B)
    m.set_data(y, X, Z, sy)
    res = {}
    for name, calls, block, f in (("para_update_us", 2000, 100, lambda: m.para_update(2, th)),
                                  ("predict_us", 200, 20, lambda: m.predict(th, X2, Z2, 0.3, sy))):
        for _ in range(2 * block):  # warm-up: code objects, pools, the caches of ctypes
            f()
        ts = []
        for _ in range(calls // block):
            t0 = time.perf_counter()  # each call ends in a device synchronise and a host copy
            for _ in range(block):
                f()
            ts.append((time.perf_counter() - t0) / block * 1e6)
        res[name] = sorted(ts)[len(ts) // 2]
    m.close()
    return res


def run():
    if mode == "time":
        return timing()
    host_only()
    if mode == "all":
        factor_and_folds()
        for kernel in ("SE", "Matern32"):
            call_surface(kernel)
            fits_and_queries(kernel)
            batch(kernel)


res = run()
if mode == "time":
    json.dump(res, open(out_path, "w"))
else:
    np.savez(out_path, __meta__=np.array(json.dumps(meta)), **out)
"""


def child(tree, mode, out, lib, timeout):
    env = dict(os.environ, ACE_LIB_PATH=os.path.abspath(lib))
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(tree), mode, out], env=env,
                       timeout=timeout)
    if r.returncode:  # not a verdict: exit status 2
        print(f"the child of tree {tree} ({mode}) exited {r.returncode}", file=sys.stderr)
        sys.exit(2)


def compare(tree_a, tree_b, mode, lib):
    got = []
    with tempfile.TemporaryDirectory() as d:
        for i, tree in enumerate((tree_a, tree_b)):
            out = os.path.join(d, f"tree{i}.npz")
            child(tree, mode, out, lib, 600)
            with np.load(out) as f:
                got.append(({k: f[k] for k in f.files if k != "__meta__"},
                            json.loads(str(f["__meta__"]))))
    (la, ma), (lb, mb) = got
    diff = [k for k in sorted(set(ma) | set(mb)) if ma.get(k) != mb.get(k)]
    for k in sorted(set(la) | set(lb)):
        a, b = la.get(k), lb.get(k)
        if k not in diff and (a is None or b is None or a.dtype != b.dtype or a.shape != b.shape
                              or a.tobytes() != b.tobytes()):
            diff.append(k)
    for k in diff:
        print(f"DIFFERS {k}: A {ma.get(k)} {None if k not in la else (la[k].dtype, la[k].shape)}"
              f" | B {mb.get(k)} {None if k not in lb else (lb[k].dtype, lb[k].shape)}")
    nval = sum(v.size for v in lb.values())
    print(f"{mode}: {len(mb)} leaves ({len(lb)} arrays, {nval} values), "
          f"{len(diff)} differing: {diff if diff else 'none'}")
    return 1 if diff else 0


def timing(tree_a, tree_b, rounds, lib):
    res = {"A": [], "B": []}
    with tempfile.TemporaryDirectory() as d:
        for r in range(rounds):
            pair = (("A", tree_a), ("B", tree_b))
            for name, tree in pair[::-1] if r % 2 else pair:  # neither tree always goes first
                out = os.path.join(d, "t.json")
                child(tree, "time", out, lib, 300)
                res[name].append(json.load(open(out)))
                print(f"round {r} tree {name}: " +
                      ", ".join(f"{k} {v:.2f}" for k, v in res[name][-1].items()), flush=True)
    for key in res["A"][0]:
        a, b = ([x[key] for x in res[t]] for t in ("A", "B"))
        inside = min(a) <= statistics.median(b) <= max(a)
        print(f"{key}: A median {statistics.median(a):.2f} range [{min(a):.2f}, {max(a):.2f}] | "
              f"B median {statistics.median(b):.2f} range [{min(b):.2f}, {max(b):.2f}] | "
              f"B's median inside A's range: {inside}")
    return 0


def main():
    args = sys.argv[1:]
    lib = None
    if "--lib" in args:
        i = args.index("--lib")
        lib = args[i + 1]
        del args[i:i + 2]
    tree_a, tree_b, rest = args[0], args[1], args[2:]
    lib = lib or os.path.join(tree_b, "additivecausalexpansion_amd", "libace_hip.so")
    if rest[:1] == ["--time"]:
        sys.exit(timing(tree_a, tree_b, int(rest[1]) if len(rest) > 1 else 5, lib))
    sys.exit(compare(tree_a, tree_b, "host" if rest[:1] == ["--host-only"] else "all", lib))


if __name__ == "__main__":
    main()
