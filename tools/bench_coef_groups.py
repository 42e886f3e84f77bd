#!/usr/bin/env python
"""Times DeviceModel.average_response against the only route to an average
marginal curve without it, on the same tree, and prints one JSON line.

Default: configuration C2 in-sample (n = nx = 16384, p = 20, B = 10,
Matern32), G = 4 groups, nz = 16 treatment values, after one para_update.
  average    one average_response(marginal): one grouped coefficient pass
             (G B right-hand sides) and the host contraction
  loop       nz calls of predict_marginal_groups, each with one constant dZ2
             row: a full marginal pass per treatment value
  one_pass   (reported beside them) a single predict_marginal_groups call
Every call ends in the library's bounded stream sync, so host wall time
around a call is its device time plus the host tail.  average and one_pass
are timed in alternation (--runs 15), the loop on its own (--loop-runs 3: it
is nz passes); medians and the spread are reported.  The two routes' results
are compared: the loop's gcov[g, g] against beta^T gcov_gg beta.

    python tools/bench_coef_groups.py [--config C2] [--nx N] [--groups 4] [--nz 16]
    rocprofv3 --kernel-trace --stats -- python tools/bench_coef_groups.py --runs 1 --loop-runs 0
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "runs": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--nx", type=int, default=0, help="test points (default: in-sample, nx = n)")
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--nz", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--loop-runs", type=int, default=3)
    a = ap.parse_args()
    import additivecausalexpansion_amd as A
    from additivecausalexpansion_amd.synthetic import CONFIGS, make_problem
    n, p, B, kernel = CONFIGS[a.config]
    y, X, Z, th, sy = make_problem(n, p, B, seed=0)
    m = A.DeviceModel(kernel, n, p, B)
    m.set_data(y, X, Z, sy)
    m.para_update(2, th.copy())
    if a.nx:
        _, X2, Z2, _, _ = make_problem(a.nx, p, B, seed=1)
    else:
        X2, Z2 = X, Z
    nx, G, nz = X2.shape[0], a.groups, a.nz
    label = (np.arange(nx) % G).astype(np.int32)
    dZ = np.asfortranarray(0.7 * Z2[:nz] + 0.1)              # nz derivative rows
    out = {"config": a.config, "kernel": kernel, "n": n, "p": p, "B": B, "nx": nx, "G": G,
           "nz": nz}
    res = {}

    def average():
        res["a"] = m.average_response(th, X2, G, label, dZ, True, 0.0, sy, 0.8)

    def one_pass(j=0):
        row = np.asfortranarray(np.repeat(dZ[j:j + 1], nx, axis=0))
        return m.predict_marginal_groups(th, X2, row, sy, 0.8, G, label)

    def loop():
        res["l"] = [one_pass(j) for j in range(nz)]

    for _ in range(a.warmup):
        average()
        one_pass()
    ta, tp = [], []
    for _ in range(a.runs):
        for fn, acc in ((average, ta), (one_pass, tp)):
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e3)
    out["average"] = stats(ta)
    out["one_pass"] = stats(tp)
    if a.loop_runs > 0:
        tl = []
        for _ in range(a.loop_runs):
            t0 = time.perf_counter()
            loop()
            tl.append((time.perf_counter() - t0) * 1e3)
        out["loop"] = stats(tl)
        out["loop_over_average"] = out["loop"]["median_ms"] / out["average"]["median_ms"]
        # the same quantities by both routes: group variances and means
        sc = (sy / 0.8) ** 2
        cnt = np.bincount(label, minlength=G).astype(float)
        v_loop = np.array([[sc * abs(r["gcov"][g, g]) / cnt[g] ** 2 for r in res["l"]]
                           for g in range(G)])
        m_loop = np.array([[r["gsum"][g] / cnt[g] for r in res["l"]] for g in range(G)])
        out["max_rel_var_diff"] = float(np.max(np.abs(res["a"]["var"] - v_loop) / v_loop))
        out["max_rel_map_diff"] = float(np.max(np.abs(res["a"]["map"] - m_loop) /
                                               np.max(np.abs(m_loop))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
