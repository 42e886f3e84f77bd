#!/usr/bin/env python
"""Times DeviceModel.predict_surface against DeviceModel.predict on the
expanded grid, on the same tree, and prints one JSON line.

Default: configuration C2 (n = 16384, p = 20, B = 10, Matern32) after one
para_update; nx = 64 covariate points x nz = 64 treatment values.
  surface   predict_surface: one coefficient pass (nx B = 640 right-hand
            sides through the resident inverse) and the host contraction
  predict   predict on the nx nz = 4096 rows of expand.grid(X, Z)
Every call ends in the library's bounded stream sync, so host wall time
around a call is its device time plus the host tail.  2 warm-ups and 15
calls each by default, timed in alternation; medians and ranges are reported,
and the largest difference of the two results as a check.

    python tools/bench_surface.py [--config C2] [--nx 64] [--nz 64] [--runs 15]
    rocprofv3 --kernel-trace --stats -- python tools/bench_surface.py --runs 1
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
    ap.add_argument("--nx", type=int, default=64)
    ap.add_argument("--nz", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=15)
    a = ap.parse_args()
    import additivecausalexpansion_amd as A
    from additivecausalexpansion_amd.synthetic import CONFIGS, make_problem
    n, p, B, kernel = CONFIGS[a.config]
    y, X, Z, th, sy = make_problem(n, p, B, seed=0)
    m = A.DeviceModel(kernel, n, p, B)
    m.set_data(y, X, Z, sy)
    m.para_update(2, th.copy())
    _, X2, _, _, _ = make_problem(a.nx, p, B, seed=1)
    _, _, Zb, _, _ = make_problem(max(a.nz, 64), p, B, seed=2)
    Zb = np.asfortranarray(Zb[:a.nz])
    Xg = np.asfortranarray(np.tile(X2, (a.nz, 1)))      # expand.grid: X fastest
    Zg = np.asfortranarray(np.repeat(Zb, a.nx, axis=0))
    surface = lambda: m.predict_surface(th, X2, Zb, False, 0.0, sy, 1.0)  # noqa: E731
    predict = lambda: m.predict(th, Xg, Zg, 0.0, sy)                      # noqa: E731
    for _ in range(a.warmup):
        s, g = surface(), predict()
    ts, tp = [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        s = surface()
        t1 = time.perf_counter()
        g = predict()
        t2 = time.perf_counter()
        ts.append((t1 - t0) * 1e3)
        tp.append((t2 - t1) * 1e3)
    dmap = float(np.max(np.abs(np.ravel(s["map"], order="F") - g["map"])) / np.max(np.abs(g["map"])))
    dvar = float(np.max(np.abs(np.ravel(s["var"], order="F") - g["var"])) / np.max(np.abs(g["var"])))
    print(json.dumps({"config": a.config, "n": n, "p": p, "B": B, "kernel": kernel, "nx": a.nx,
                      "nz": a.nz, "columns_surface": a.nx * B, "columns_predict": a.nx * a.nz,
                      "surface": summary(ts), "predict": summary(tp),
                      "speedup_median": statistics.median(tp) / statistics.median(ts),
                      "max_rel_diff_map": dmap, "max_rel_diff_var": dvar}))


if __name__ == "__main__":
    main()
