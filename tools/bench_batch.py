#!/usr/bin/env python
"""Times one BatchModel.para_update over M small models against M sequential
DeviceModel.para_update calls of the same size, and prints a table plus one
JSON line per row.

README config by default (p = 2, B = 5, both kernels), n = 300 and 512,
M in {1, 16, 256, 1024}.
  batch       one ace_batch_para_update of M models (theta up, one launch,
              results down, one bounded sync)
  sequential  M ace_model_para_update calls on one DeviceModel of the same n
              (each ends in its own bounded sync, as a loop over fits does)
Both end in the library's stream sync, so host wall time around them is
device time plus the host tail.  The two are timed in alternation after
--warmup rounds; the median and min-max of --runs rounds are reported, and
ratio = sequential / batch per round (median).

    python tools/bench_batch.py [--n 300 512] [--M 1 16 256 1024] [--runs 7]
    rocprofv3 --kernel-trace --stats -- python tools/bench_batch.py --n 300 --M 256 --runs 1 --warmup 1
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
    ap.add_argument("--n", type=int, nargs="+", default=[300, 512])
    ap.add_argument("--M", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--p", type=int, default=2)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--kernels", nargs="+", default=["SE", "Matern32"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    import additivecausalexpansion_amd as A
    from additivecausalexpansion_amd.synthetic import make_problem
    rows = []
    for kernel in a.kernels:
        for n in a.n:
            probs = [make_problem(n, a.p, a.B, seed=s) for s in range(8)]
            y, X, Z, th, sy = probs[0]
            dm = A.DeviceModel(kernel, n, a.p, a.B)
            dm.set_data(y, X, Z, sy)
            for M in a.M:
                bm = A.BatchModel(kernel, M, n, a.p, a.B)
                for j in range(M):
                    q = probs[j % len(probs)]
                    bm.set_data(j, q[0], q[1], q[2], q[4])
                theta = np.asfortranarray(np.column_stack([th] * M))

                def batch():
                    bm.para_update(2, theta)

                def sequential():
                    for _ in range(M):
                        dm.para_update(2, th)

                for _ in range(a.warmup):
                    batch()
                    sequential()
                tb, ts = [], []
                for _ in range(a.runs):
                    for fn, acc in ((batch, tb), (sequential, ts)):
                        t0 = time.perf_counter()
                        fn()
                        acc.append((time.perf_counter() - t0) * 1e3)
                bm.close()
                row = {"kernel": kernel, "n": n, "p": a.p, "B": a.B, "M": M,
                       "batch": summary(tb), "sequential": summary(ts),
                       "sequential_per_eval_ms": statistics.median(ts) / M,
                       "batch_per_model_ms": statistics.median(tb) / M,
                       "ratio": statistics.median([s / b for s, b in zip(ts, tb)])}
                rows.append(row)
                print(json.dumps(row), flush=True)
            dm.close()
    print()
    print(f"{'kernel':9s} {'n':>4s} {'M':>5s} {'batch ms (min-max)':>28s} "
          f"{'sequential ms (min-max)':>32s} {'seq/eval ms':>12s} {'ratio':>8s}")
    for r in rows:
        b, s = r["batch"], r["sequential"]
        print(f"{r['kernel']:9s} {r['n']:4d} {r['M']:5d} "
              f"{b['median_ms']:10.3f} ({b['min_ms']:.3f}-{b['max_ms']:.3f})".ljust(48) +
              f"{s['median_ms']:12.3f} ({s['min_ms']:.3f}-{s['max_ms']:.3f})".ljust(36) +
              f"{r['sequential_per_eval_ms']:10.4f} {r['ratio']:8.1f}")


if __name__ == "__main__":
    main()
