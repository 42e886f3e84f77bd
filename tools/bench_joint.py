#!/usr/bin/env python
"""Times one DeviceModel.predict_joint (covariance, factor and draws) against
one DeviceModel.predict at the same size, on the same tree, and prints one
JSON line.

Default: configuration C2 (n = 16384, p = 20, B = 10, Matern32) after one
para_update; nx = 4096 test points, 1000 draws.
  joint     predict_joint with cov, L and 1000 draws returned (K_xX, the full
            A^-1 K_xX^T product, K_xx, k_post_cov, the blocked Cholesky, the
            draw product, and the three nx x nx / nx x S downloads)
  device    the same call with nothing but map returned to the host beyond
            the draws' flag: cov and L stay on the device (xi still goes up)
  predict   predict (the triangular product, diag(K_xx) only)
Every call ends in the library's bounded stream sync, so host wall time
around a call is its device time plus the host tail.  2 warm-ups and 10
calls each by default, timed in alternation; medians and ranges are reported.
The factor's work is nx^3 / 3 flops in 3 nx / 64 dependent launches.

    python tools/bench_joint.py [--config C2] [--nx 4096] [--draws 1000] [--runs 10]
    rocprofv3 --kernel-trace --stats -- python tools/bench_joint.py --runs 1 --warmup 1
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
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    import additivecausalexpansion_amd as A
    from additivecausalexpansion_amd.synthetic import CONFIGS, make_problem
    n, p, B, kernel = CONFIGS[a.config]
    y, X, Z, th, sy = make_problem(n, p, B, seed=0)
    m = A.DeviceModel(kernel, n, p, B)
    m.set_data(y, X, Z, sy)
    m.para_update(2, th.copy())
    _, X2, Z2, _, _ = make_problem(a.nx, p, B, seed=1)
    xi = np.asfortranarray(np.random.default_rng(0).standard_normal((a.nx, a.draws)))
    joint = lambda: m.predict_joint(th, X2, Z2, 0.0, sy, xi=xi, return_cov=True,  # noqa: E731
                                    return_factor=True)
    device = lambda: m.predict_joint(th, X2, Z2, 0.0, sy, xi=xi[:, :1])            # noqa: E731
    predict = lambda: m.predict(th, X2, Z2, 0.0, sy)                               # noqa: E731
    for _ in range(a.warmup):
        j, d, g = joint(), device(), predict()
    tj, td, tp = [], [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        j = joint()
        t1 = time.perf_counter()
        d = device()
        t2 = time.perf_counter()
        g = predict()
        t3 = time.perf_counter()
        tj.append((t1 - t0) * 1e3)
        td.append((t2 - t1) * 1e3)
        tp.append((t3 - t2) * 1e3)
    dvar = float(np.max(np.abs(np.diag(j["cov"]) - g["var"])) / np.max(np.abs(g["var"])))
    print(json.dumps({"config": a.config, "n": n, "p": p, "B": B, "kernel": kernel, "nx": a.nx,
                      "draws": a.draws, "info": j["info"], "joint": summary(tj),
                      "device": summary(td), "predict": summary(tp),
                      "factor_flops": a.nx ** 3 / 3, "factor_launches": 3 * ((a.nx + 63) // 64) - 2,
                      "max_rel_diff_diag_var": dvar}))


if __name__ == "__main__":
    main()
