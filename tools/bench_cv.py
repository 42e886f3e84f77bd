#!/usr/bin/env python
"""Times cross-validation from the resident inverse (DeviceModel.cv, DESIGN
§18) on one model after one para_update, on the same tree, and prints one JSON
line.

Default: configuration C2 (n = 16384, p = 20, B = 10, Matern32).
  loo       leave-one-out, n folds of one row        (k_cv_loo)
  wg32      32 folds of 512 rows                     (k_cv_gather + k_cv_fold)
  k10       10 random folds of n / 10 rows           (the whole-chip sweep, fold after fold)
timed in alternation with
  update    one para_update of the model (what every refit costs at least), and
  holdout   the refit-free alternative without this feature: a DeviceModel on
            the other rows of one of the 10 folds at the same theta (set_data,
            one para_update for its inverse) and predict of the fold's rows;
            one fold is timed and `holdout_x10_ms` scales it to the ten.
Every call ends in the library's bounded stream sync, so host wall time around
a call is its device time plus the host tail (fold packing and the scatter
included).  2 warm-ups and 5 runs each by default; medians and ranges are
reported, and each set's work count, the sum of m^3 over its folds.

    python tools/bench_cv.py [--config C2] [--runs 5]
    rocprofv3 --kernel-trace --stats -- python tools/bench_cv.py --runs 1 --warmup 1
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def summary(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "runs": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-holdout", action="store_true")
    a = ap.parse_args()
    import additivecausalexpansion_amd as A
    from additivecausalexpansion_amd.synthetic import CONFIGS, make_problem
    n, p, B, kernel = CONFIGS[a.config]
    y, X, Z, th, sy = make_problem(n, p, B, seed=0)
    m = A.DeviceModel(kernel, n, p, B)
    m.set_data(y, X, Z, sy)
    m.para_update(2, th.copy())
    perm = np.random.default_rng(0).permutation(n)
    sets = {"loo": [np.array([i]) for i in range(n)],
            "wg32": np.array_split(perm, max(1, n // 512)),
            "k10": np.array_split(perm, 10)}
    F = sets["k10"][0]
    R = np.setdiff1d(np.arange(n), F)
    yR, XR, ZR = np.ravel(y)[R].copy(), np.asfortranarray(X[R]), np.asfortranarray(Z[R])
    XF, ZF = np.asfortranarray(X[F]), np.asfortranarray(Z[F])

    def holdout():
        h = A.DeviceModel(kernel, R.size, p, B)
        h.set_data(yR, XR, ZR, sy)
        h.para_update(2, th.copy())
        r = h.predict(th, XF, ZF, 0.0, sy)
        h.close()
        return r

    calls = {k: (lambda f=f: m.cv(th, f, 0.0, sy)) for k, f in sets.items()}
    calls["update"] = lambda: m.para_update(2, th.copy())
    if not a.no_holdout:
        calls["holdout"] = holdout
    last = {}
    for _ in range(a.warmup):
        for k, f in calls.items():
            last[k] = f()
    times = {k: [] for k in calls}
    for _ in range(a.runs):
        for k, f in calls.items():
            t0 = time.perf_counter()
            last[k] = f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    out = {"config": a.config, "n": n, "p": p, "B": B, "kernel": kernel}
    for k in calls:
        out[k] = summary(times[k])
    for k, f in sets.items():
        out[k]["folds"] = len(f)
        out[k]["work_m3"] = float(sum(float(g.size) ** 3 for g in f))
        out[k]["status_max"] = int(np.abs(last[k]["status"]).max())
        out[k]["elpd"] = float(np.sum(last[k]["lpd"]))
    if "holdout" in calls:
        out["holdout_x10_ms"] = 10 * out["holdout"]["median_ms"]
        # the two answers to the same question: fold 0 of k10 held out
        o = last["k10"]["off"]
        d = np.abs(last["k10"]["map"][o[0]:o[1]] - last["holdout"]["map"])
        out["k10_vs_holdout_max_abs_diff_map"] = float(d.max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
