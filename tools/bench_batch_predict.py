#!/usr/bin/env python
"""Times posterior prediction of M small fits in one batched call against the
same M predictions one after another, and prints a table plus one JSON line
per row.

README config by default (n = 300, p = 2, B = 5, both kernels), M in
{1, 16, 256}, two modes: in-sample marginal prediction with ATE/ATT/ATU, and
plain prediction at nx = n.  Every fit holds its inverse on the host, as
ace_train_batch returns it.
  batch       what predict_ace_batch does: one BatchModel, set_data and
              set_inverse per fit, one ace_predict_batch /
              ace_predict_marginal_batch call, close
  launch      the batched call alone, on a batch that already holds the data
              and the inverses (BatchModel.predict after BatchModel.train)
  sequential  M predictions through the host-buffer path predict_ace takes on
              an ace_train_batch fit (kernel matrices, then pred_cpp /
              pred_marginal_cpp with the n x n inverse uploaded per call)
  resident    M DeviceModel.predict / predict_marginal calls on single models
              that hold their inverse on the device (8 models, taken in turn)
The legs are timed in alternation after --warmup rounds; the median and
min-max of --runs rounds are reported, ratio = sequential / batch and
resident / batch per round (median).

    python tools/bench_batch_predict.py [--n 300] [--M 1 16 256] [--runs 7]
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
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--M", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--p", type=int, default=2)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--kernels", nargs="+", default=["SE", "Matern32"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    import additivecausalexpansion_amd as A
    n, p, B = a.n, a.p, a.B
    from additivecausalexpansion_amd.synthetic import make_problem
    Kc = {"SE": A.KernelClass_SE_R6, "Matern32": A.KernelClass_Matern32_R6}
    rows = []
    for kernel in a.kernels:
        probs = [make_problem(n, p, B, seed=s) for s in range(8)]
        th = probs[0][3].copy()
        th[1] = 0.13
        zx = (np.arange(n) % 3 == 0).astype(float)
        singles, invs = [], []
        for y, X, Z, th0, sy in probs:
            dm = A.DeviceModel(kernel, n, p, B)
            dm.set_data(y, X, Z, sy)
            dm.para_update(2, th0.copy())
            singles.append(dm)
            invs.append(dm.inverse())
        for M in a.M:
            idx = [j % len(probs) for j in range(M)]
            theta = np.asfortranarray(np.column_stack([th] * M))
            X2s = [probs[i][1] for i in idx]
            Z2s = [probs[i][2] for i in idx]
            dZs = [np.asfortranarray(probs[i][2] * 0.7 + 0.1) for i in idx]
            kerns = []
            for i in idx:  # a fit's kernel object with its inverse on the host
                K = Kc[kernel](p, B, th, probs[i][4])
                K._inv = invs[i]
                kerns.append(K)

            def fill(bm):
                for j, i in enumerate(idx):
                    bm.set_data(j, probs[i][0], probs[i][1], probs[i][2], probs[i][4])
                    bm.set_inverse(j, invs[i])

            held = A.BatchModel(kernel, M, n, p, B)
            fill(held)
            for mode in ("marginal+ate", "plain"):
                marg = mode != "plain"

                def call(bm):
                    if marg:
                        return bm.predict_marginal(theta, X2s, dZs, [zx] * M, 1.7, 0.8, True)
                    return bm.predict(theta, X2s, Z2s, 0.3, 1.7)

                def batch():
                    bm = A.BatchModel(kernel, M, n, p, B)
                    fill(bm)
                    call(bm)
                    bm.close()

                def launch():
                    call(held)

                def sequential():
                    for j, i in enumerate(idx):
                        y, X, Z = probs[i][:3]
                        if marg:
                            kerns[j].predict_marginal(y, X, Z, X, zx, dZs[j], 0.3, 1.7, 0.8, True)
                        else:
                            kerns[j].predict(y, X, Z, X, Z, 0.3, 1.7)

                def resident():
                    for j, i in enumerate(idx):
                        if marg:
                            singles[i].predict_marginal(th, X2s[j], dZs[j], zx, 1.7, 0.8, True)
                        else:
                            singles[i].predict(th, X2s[j], Z2s[j], 0.3, 1.7)

                legs = (("batch", batch), ("launch", launch), ("sequential", sequential),
                        ("resident", resident))
                for _ in range(a.warmup):
                    for _, fn in legs:
                        fn()
                t = {k: [] for k, _ in legs}
                for _ in range(a.runs):
                    for k, fn in legs:
                        t0 = time.perf_counter()
                        fn()
                        t[k].append((time.perf_counter() - t0) * 1e3)
                row = {"kernel": kernel, "mode": mode, "n": n, "p": p, "B": B, "M": M}
                for k, _ in legs:
                    row[k] = summary(t[k])
                for k in ("sequential", "resident"):
                    row[k + "_over_batch"] = statistics.median(
                        [s / b for s, b in zip(t[k], t["batch"])])
                rows.append(row)
                print(json.dumps(row), flush=True)
            held.close()
        for dm in singles:
            dm.close()
    print()
    print(f"{'kernel':9s} {'mode':13s} {'M':>4s}  {'batch ms (min-max)':26s} {'launch ms (min-max)':26s} "
          f"{'sequential ms (min-max)':30s} {'resident ms (min-max)':30s} {'seq/batch':>9s} {'res/batch':>9s}")

    def cell(s, w):
        return f"{s['median_ms']:.3f} ({s['min_ms']:.3f}-{s['max_ms']:.3f})".ljust(w)
    for r in rows:
        print(f"{r['kernel']:9s} {r['mode']:13s} {r['M']:4d}  " + cell(r["batch"], 27) +
              cell(r["launch"], 27) + cell(r["sequential"], 31) + cell(r["resident"], 31) +
              f"{r['sequential_over_batch']:9.1f} {r['resident_over_batch']:9.1f}")


if __name__ == "__main__":
    main()
