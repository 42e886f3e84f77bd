"""Reference restatements shared by tests/test_robust_cpu.py and
tests/test_robust_gpu.py: the discard levels of R/robust_treatment.R:83-84, 94
(R's default type-7 quantile) and the block-sum identity the device's grouped
posterior sums rest on.  numpy / Python floats only."""
import math

import numpy as np


def levels_ref(var, n_steps):
    """thresholds (n_steps + 1) and level (first step t with var <= thr[t])
    with R's arithmetic: probs = min(i * (1 / n_steps), 1),
    index = 1 + (nx - 1) p, q = x_(lo), and where index > lo and x_(hi) != q,
    q = (1 - h) q + h x_(hi) with h = index - lo."""
    var = np.ravel(np.asarray(var, dtype=np.float64))
    nx = var.size
    x = np.sort(var)
    by = 1.0 / n_steps
    thr = np.empty(n_steps + 1)
    for i in range(n_steps + 1):
        p = min(i * by, 1.0)
        index = 1 + float(nx - 1) * p
        lo, hi = math.floor(index), math.ceil(index)
        q = float(x[lo - 1])
        xh = float(x[hi - 1])
        if index > lo and xh != q:
            h = index - lo
            q = (1 - h) * q + h * xh
        thr[i] = q
    first = np.full(nx, n_steps, dtype=np.int32)
    done = np.zeros(nx, dtype=bool)
    for t in range(n_steps):
        hit = (var <= thr[t]) & ~done
        first[hit] = t
        done |= hit
    return thr, first


def indicator(label, G):
    """E (nx x G): E[i, g] = (label[i] == g); label -1 is in no group."""
    label = np.ravel(label)
    E = np.zeros((label.size, G))
    ok = label >= 0
    E[np.nonzero(ok)[0], label[ok]] = 1.0
    return E


def step_post(gcov, t):
    """The three posterior forms (ATE, ATT, ATU) of step t from
    gcov = E^T C E with label = 2 level + treated: prefix sums over the groups
    of levels <= t."""
    g1 = 2 * (t + 1)
    blk = gcov[:g1, :g1]
    return blk.sum(), blk[1::2, 1::2].sum(), blk[0::2, 0::2].sum()
