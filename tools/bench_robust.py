#!/usr/bin/env python
"""Times DeviceModel.robust_treatment against its two baselines on the same
tree and prints one JSON line.

Default: configuration C2 in-sample (n = nx = 16384, p = 20, B = 10,
Matern32, n_steps = 5), after one para_update.
  robust     robust_treatment (one marginal pass, the levels, one grouped pass)
  marginal   (i)  one predict_marginal without ATE at the same nx
  sequence   (ii) the reference's sequence through the pre-existing API: one
             marginal call plus n_steps + 1 predict_marginal(..., True) calls
             on the nested subsets
Every call ends in the library's bounded stream sync, so host wall time
around a call is its device time plus the host tail.  --warmup >= 2 and
--runs 15 by default, robust and marginal timed in alternation; the median
and the spread are reported.

    python tools/bench_robust.py [--config C2] [--nx N] [--steps 5] [--runs 15]
    rocprofv3 --kernel-trace --stats -- python tools/bench_robust.py --runs 1 --no-sequence
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--nx", type=int, default=0, help="test points (default: in-sample, nx = n)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--no-sequence", action="store_true", help="skip baseline (ii)")
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
    nx = X2.shape[0]
    dZ2 = np.asfortranarray(0.7 * Z2 + 0.1)
    zx = (np.arange(nx) % 3 == 0).astype(float)
    out = {"config": a.config, "kernel": kernel, "n": n, "p": p, "B": B, "nx": nx,
           "n_steps": a.steps}
    res = {}

    def robust():
        res["r"] = m.robust_treatment(th, X2, dZ2, zx, sy, 0.8, a.steps)

    def marginal():
        m.predict_marginal(th, X2, dZ2, zx, sy, 0.8, False)

    # the two are timed in alternation, so that clock and allocator drift
    # falls on both alike
    for _ in range(a.warmup):
        robust()
        marginal()
    tr, tm = [], []
    for _ in range(a.runs):
        for fn, acc in ((robust, tr), (marginal, tm)):
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e3)
    for key, t in (("robust", tr), ("marginal", tm)):
        out[key] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
                    "runs": a.runs}
    out["robust_minus_marginal_ms"] = statistics.median([x - y for x, y in zip(tr, tm)])
    out["robust_over_marginal"] = out["robust"]["median_ms"] / out["marginal"]["median_ms"]
    if not a.no_sequence:
        level = res["r"]["level"]

        def sequence():
            m.predict_marginal(th, X2, dZ2, zx, sy, 0.8, False)
            for t in range(a.steps + 1):
                keep = level <= t
                m.predict_marginal(th, X2[keep], dZ2[keep], zx[keep], sy, 0.8, True)

        out["sequence"] = timed(sequence, a.warmup, a.runs)
        out["sequence_over_robust"] = out["sequence"]["median_ms"] / out["robust"]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
