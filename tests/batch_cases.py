"""Cases and helpers shared by the batched engine's tests
(tests/test_batch_gpu.py, tests/test_batch_regimes_cpu.py,
tests/test_batch_regimes_gpu.py) -- TEST INFRASTRUCTURE ONLY, plain numpy.

* `REGIME_CASES`: the (p, model regimes) that go through k_batch_eval against
  the extended-precision referee, one BatchModel per (kernel, p), n = 130 and
  B = 3 (nine 16-blocks, the last ragged, plus the right-hand-side block).
* `gauss_jordan_fp64`: the batch kernel's inverse algorithm at block width 1.
* `CPU_CAP`: what fp64 arithmetic of that form was measured to need of the
  project's contract (see there), and `TIGHT` = 10 CPU_CAP, the bound the
  device is held to besides the contract itself.
* `singular_cases`: models that are not positive definite by construction.
"""
import numpy as np

import regimes as R

N_REG, B_REG = 130, 3
SOME = ("base", "dups", "binary", "long", "zext_m")
# p -> regimes.  PM is k_batch_eval's feature bucket (4 / 8 / 16 / 32 / 64):
#   3: PM = 4;  40: PM = 64, padded, the two-pass gradient;  8, 16: p equals
#   the bucket (16: the last 512-thread one);  17: PM = 32;  64: PM = 64 unpadded
REGIME_CASES = ((3, R.MODEL_REGIMES), (40, R.MODEL_REGIMES), (8, SOME), (16, SOME), (17, SOME),
                (64, SOME))

# Largest fraction of the contract (tests/test_regimes_cpu.contract_used) that
# fp64 arithmetic used against the referee over exactly REGIME_CASES, both
# kernels, gradient / stats / mu, printed by tests/test_batch_regimes_cpu.py:
#   the fp64 oracle chain                           3.43e-4 (SE, zext_m, p = 8, gradient)
#   grad_from_inverse on gauss_jordan_fp64's result 3.07e-5 (SE, zext_m, p = 3, gradient)
# CPU_CAP is three times the worst of them (3.43e-4 rounded up in its last
# digit).  Nothing here comes from a device.
CPU_WORST = 3.44e-4
CPU_CAP = 3 * CPU_WORST
TIGHT = 10 * CPU_CAP


def gauss_jordan_fp64(A):
    """(A^-1, sum of the log pivots) of a symmetric A by the pivot-free
    symmetric Gauss-Jordan sweep in numpy fp64: csrc/ace_batch.hip's algorithm
    at a block width of one.  After step k the swept matrix holds -1 / piv at
    (k, k), column k / piv in row and column k, and the Schur update elsewhere;
    after the last step it is -A^-1."""
    S = np.array(A, dtype=np.float64)
    n = S.shape[0]
    logdet = 0.0
    for k in range(n):
        piv = S[k, k]
        logdet += np.log(piv)
        col = S[:, k].copy()
        w = col / piv
        S -= np.outer(w, col)
        S[:, k] = w
        S[k, :] = w
        S[k, k] = -1.0 / piv
    return -S, logdet


def problems(ns, p, B, seed0=0):
    from additivecausalexpansion_amd.synthetic import make_problem
    return [make_problem(n, p, B, seed=seed0 + 11 * j + n) for j, n in enumerate(ns)]


# ---- not positive definite by construction --------------------------------
SING_P, SING_B = 3, 5
# (rows of the model, the row of Z set to zero): the first 16-block (the
# in-block scalar steps), a later block (reached through the MFMA updates),
# the ragged last block
SING_ROWS = ((130, 3), (64, 37), (45, 44))
HEALTHY_N = (17, 65)


def singular_cases():
    """[(healthy problem, singular problem, singular theta, row)] for SING_ROWS.
    The singular model is the healthy one with row `row` of Z zeroed and
    theta[0] = theta[2] = -2000: e^theta0 and slice 0 (amplitude e^-2000) are
    exactly 0 in fp64 and every z slice is exactly 0 along that row, so row
    and column `row` of A are exactly zero and so is the pivot met there,
    however the steps before it round (a zero row stays zero under the sweep's
    updates: its multiplier column is zero)."""
    out = []
    for n, row in SING_ROWS:
        y, X, Z, th, sy = problems((n,), SING_P, SING_B)[0]
        Zs = np.array(Z, order="F")
        Zs[row, :] = 0.0
        ths = th.copy()
        ths[0] = -2000.0
        ths[2] = -2000.0
        out.append(((y, X, Z, th, sy), (y, X, Zs, ths, sy), ths, row))
    return out


# ---- the optimizers of k_batch_step ------------------------------------------
OPT_P, OPT_B, OPT_ITERS = 2, 3, 8
OPT_SEEDS = ((40, 1), (60, 2), (90, 3))  # (n, make_problem's seed)
# name -> (the package's optimizer name, the oracle's, lr, momentum, norm_clip, clip_at)
OPT_CONFIGS = {
    "nesterov": ("NAG", "Nesterov", 0.01, 0.9, True, 1.0),
    "adam": ("Adam", "Adam", 0.03, 0.0, True, 1.0),
    "adam-noclip": ("Adam", "Adam", 0.03, 0.0, False, 1.0),
    "nadam-clip0.3": ("Nadam", "Nadam", 0.01, 0.0, True, 0.3),
}


def opt_problems(name):
    """The three make_problem models of the optimizer test and their start
    theta: make_problem's, except for the clip_at = 0.3 configuration.

    That configuration is there for Q5 (a gradient longer than clip_at is
    rescaled to UNIT norm, not to clip_at), which shows only at an iteration
    with clip_at < ||g|| <= 1.  From make_problem's theta no such iteration
    exists: the oracle's ||g|| starts at 10.7 .. 32 (seeds 1 .. 5 of every n,
    both kernels) and grows from there (to 1e3 after 400 iterations at lr 0.01,
    past 1e14 after 1200 at lr 0.05: the noise term runs toward zero), so
    neither a seed nor an iteration count reaches the band.  The start is
    therefore moved next to a stationary point that exists in closed form: with
    all amplitudes at e^-7 the model is almost pure noise, A ~ e^theta0 I,
    g_0 ~ -0.5 (n - e^-theta0 |y|^2) with |y|^2 = n - 1 (y is standardised),
    and theta0 = log((n - 1) / n) - log(1 + 1.2 / n) puts g_0 near +0.6 with
    every other component below 0.1.  The oracle's ||g|| at iteration 1 is then
    0.54 / 0.51 / 0.41 (SE) and 0.53 / 0.49 / 0.36 (Matern32) for n = 40 / 60 /
    90, and below 0.3 (no clip at all) from iteration 2 or 3 on; the test
    asserts the band on the oracle's side before it looks at the device."""
    from additivecausalexpansion_amd.synthetic import make_problem
    probs = []
    for n, seed in OPT_SEEDS:
        y, X, Z, th, sy = make_problem(n, OPT_P, OPT_B, seed=seed)
        th = th.copy()
        if name == "nadam-clip0.3":
            th[2:2 + OPT_B] = -7.0
            th[0] = np.log((n - 1) / n) - np.log1p(1.2 / n)
        probs.append((y, X, Z, th, sy))
    return probs
