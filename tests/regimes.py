"""Input regimes for the pair kernels and the a-priori bound their K is held
to -- TEST INFRASTRUCTURE ONLY (plain numpy, no GPU).

Every other numerical test draws X ~ U(-1, 1), length-scale parameters in
about [0, 3], amplitudes near 0 and z of order 1, and scales its tolerance by
max|ref|.  The hot-path kernels (csrc/ace_pairs_mm.hip) replace the
reference's arithmetic by forms whose error depends on the data: r2 by a Gram
expansion on the matrix cores, hand-written exp / sqrt, the SE sign / log|z|
form.  `regime` produces the data on which those forms can fail -- all of it
data the package itself produces (normalize_train maps binary columns to
{0, 1}, normalize_test extrapolates, the optimiser moves length scales and
amplitudes over many units, the C ABI accepts unnormalised X).

`k_bound` gives, per element, the extended-precision K (referee_ld's
mathematics, extended to two point sets) and a bound on what fp64 arithmetic
of the kernels' form may miss it by.

Derivation of the bound
-----------------------
Notation: u = 2^-53; PM the compiled feature bucket (>= p; the zero padding
adds exact zeros); w_bi = exp(-theta_L); s_b(x) = sum_i w_bi x_i^2;
S_b = s_b(r) + s_b(c); lambda_b the slice's amplitude parameter.

r2.  The MFMA family forms r2_b = s_b(r) + s_b(c) - 2 G, G = sum_i w_bi x_ri
x_ci.  Each of s_b(r), s_b(c) and G is a PM-term fp64 sum of products
(relative error (PM + 2) u of the sum of the terms' magnitudes, first order:
PM - 1 additions, the product, the rounded weight), and 2 sum_i |w x_r x_c|
<= S_b, so the three sums miss by at most (PM + 2) u (S_b + S_b); the two
final additions add 2 u S_b each at most.  Hence
    |r2_b - r2_b,exact| <= delta_b = 2 (PM + 4) u S_b,
the "eps * (s_b(r) + s_b(c))" of the kernel file's header with its constant.
The direct-difference form (the fp64 oracle, the all-VALU family) misses r2
by at most (PM + 4) u r2 (difference, square, weight, PM-term sum), and
r2 <= 2 S_b, so delta_b covers it too.  A clamp of a negative r2 to 0 (or to
1e-300, which gives the same K in double) only moves r2 toward the exact
value, which is >= 0.

SE.  K_b = sign(z_r) sign(z_c) exp(((lambda_b - r2_b) + log|z_r|) + log|z_c|).
An error d in the exponent is a relative error e^d - 1 ~ d of K_b.  The
exponent carries delta_b from r2, u |log|z|| from each fp64 log, and one
rounding of each of the three partial sums, each at most
M_b = |lambda_b| + r2_b + |log|z_r|| + |log|z_c|| in magnitude: 5 u M_b
together.  The exponential itself is good to about 1.5 u (table entry,
polynomial, the product), the sum over slices adds (B - 1) u of sum|K_b|
(B <= 3 in the tests).  With slack 8 u (1 + M_b):
    bound_b = |K_b| (delta_b + 8 u (1 + M_b)).
Matern32.  K_b = z_r z_c (1 + sqrt3 t) exp(lambda_b - sqrt3 t), t = sqrt(r2_b).
dK_b/dr2 = -1.5 z_r z_c exp(lambda_b - sqrt3 t), largest in magnitude at the
low end of [r2 - delta_b, r2 + delta_b]; with t- = sqrt(max(r2_b - delta_b, 0))
the r2 error moves K_b by at most |z_r z_c| 1.5 exp(lambda_b - sqrt3 t-) delta_b.
The exponent lambda_b - sqrt3 t has partial sums at most |lambda_b| + sqrt3 t,
the square root, the product sqrt3 t, 1 + sqrt3 t, the exponential and the
two z products one rounding each:
    bound_b = |z_r z_c| 1.5 exp(lambda_b - sqrt3 t-) delta_b
              + |K_b| 8 u (1 + |lambda_b| + sqrt3 t)
              + 2^-1074 ((1 + sqrt3 t) |z_r z_c| + max(|z_r|, |z_c|)).
The last term was not in the first form of this bound; it was added from
the arithmetic when the fp64 oracle itself missed the bound without it
(short, p = 20: 23 times), before any device result existed.  Matern32
multiplies an exponential that may be denormal -- rounded to a multiple of
2^-1074, not to a relative u -- by (1 + sqrt3 t) ~ 740 at the underflow
boundary and by z_r z_c, and the reference's product order (e z_lo) z_hi
multiplies the rounding of a denormal e z_lo by |z_hi|.  (SE multiplies its
exponential by a sign only.)
Both.  bound = sum_b bound_b + 2^-1070: a result below 2^-1022 is rounded a
second time, to a multiple of 2^-1074, in every slice and in their sum (16
such steps cover B <= 3 slices with the exponential's own ldexp rounding and
the products).  The per-slice bound is bound_b + 2^-1070 for the same
reason.  Where z_r or z_c is +-0 the reference's K_b is exactly 0 (SE: the
explicit select; Matern32: the product), so K_b,ref = 0 and the slice's
bound is exactly 0: such a slice must come out as 0, not as something small.
(In the sum over slices, slice 0 has z = 1 and is never such; the tests
switch it off with lambda_0 = -2000, where it is 0 in fp64, to see the other
slices' zeros in the full K.)

No constant above was fitted to a device result.  tests/test_regimes_cpu.py
shows the bound is attainable by fp64 arithmetic of both forms (the oracle's
direct differences and a numpy restatement of the expansion).
"""
from __future__ import annotations

import functools

import numpy as np

from referee_ld import LD

U = 2.0 ** -53
TINY = 2.0 ** -1070
DENORM_ULP = 2.0 ** -1074
# csrc/ace_internal.h PM_BUCKETS: the feature counts the pair kernels are compiled for
BUCKETS = (4, 8, 12, 16, 20, 24, 32, 48, 64)

REGIMES = ("base", "dups", "neardup", "neardup_ulp", "binary", "short", "long", "ramp30", "ramp450",
           "offset1", "offset100", "amp_hi", "amp_lo", "zext", "zext_m")
# amp_hi (amplitudes e^6 against sigma = 0.1: cond(A) ~ 4e3 n) and zext (below)
# are for the K check only
MODEL_REGIMES = tuple(r for r in REGIMES if r not in ("amp_hi", "zext"))

# zext: the values planted in Z, cycled along a fixed stride of its (row-major)
# entries, so every value meets every other in both columns.
ZEXT = (1e-160, -1e-300, 5e-324, 1e150, 0.0, -0.0)
ZEXT_STRIDE = 7
# zext_m, the model's form of zext, SOFTENED: 1e150 -> 1e2.  With z = 1e150 K
# has entries 1e300 and the fp64 oracle's eigendecomposition returns NaN (from
# z = 1e8 on); at 1e6 and 1e4 its gradient misses the contract against the
# referee by 1e5 and 1.8 times (cond(A) ~ z^2 n / sigma).  At 1e2 it uses
# 6.4e-5 of it, the level of the other regimes.  The small values and the
# zeros stay.  zext itself (1e150) remains for the K checks.
ZEXT_MODEL = (1e-160, -1e-300, 5e-324, 1e2, 0.0, -0.0)


def pm_bucket(p):
    return next(b for b in BUCKETS if p <= b)


def _set_L(theta, B, L):
    theta[2 + B:] = L


def regime(name, n, p, B, seed):
    """(y, X, Z, theta, std_y) of make_problem(n, p, B, seed) (theta_0 =
    log 0.1), modified as the regime says."""
    from additivecausalexpansion_amd.synthetic import make_problem
    y, X, Z, th, sy = make_problem(n, p, B, seed=seed)
    y, X, Z, th = y.copy(), np.array(X, order="F"), np.array(Z, order="F"), th.copy()
    rng = np.random.default_rng(seed + 7919)
    if name == "base":
        pass
    elif name in ("dups", "neardup", "neardup_ulp"):
        # equal points in different 64-tiles; n < 128: the second half copies
        # the first (same tile).  z is left alone: equal covariates, other basis
        h = 64 if n >= 128 else n // 2
        src = X[:h].copy()
        if name == "neardup":
            src = src * (1 + 1e-9)
        elif name == "neardup_ulp":
            src = np.nextafter(src, np.inf)
        X[h:2 * h] = src
    elif name == "binary":
        X[:] = rng.integers(0, 2, size=(n, p)).astype(np.float64)
        if p > 1:  # a constant column after normalize_train (p = 1: kept, or all points are one)
            X[:, p - 1] = 0.0
        _set_L(th, B, 0.0)
    elif name == "short":
        _set_L(th, B, -6.0)
    elif name == "long":
        _set_L(th, B, 8.0)
    elif name in ("ramp30", "ramp450"):
        X[:, 0] = np.linspace(0.0, 30.0 if name == "ramp30" else 450.0, n)
        _set_L(th, B, 0.0)
    elif name == "offset1":
        X += 1.5
    elif name == "offset100":
        X += 100.0
    elif name == "amp_hi":
        th[2:2 + B] = 6.0
    elif name == "amp_lo":
        th[2:2 + B] = -30.0
    elif name in ("zext", "zext_m"):
        Zc = np.ascontiguousarray(Z)
        flat = Zc.reshape(-1)
        idx = np.arange(3, flat.size, ZEXT_STRIDE)
        flat[idx] = np.resize(np.array(ZEXT if name == "zext" else ZEXT_MODEL), idx.size)
        Z = np.asfortranarray(Zc)
    else:
        raise KeyError(name)
    return y, np.asfortranarray(X), np.asfortranarray(Z), th, sy


def kernel_slices_ld(kernel, X1, X2, Z1, Z2, theta):
    """referee_ld._kernel_slices for two point sets: (B, n1, n2) in longdouble."""
    X1 = np.asarray(X1, dtype=np.float64)
    X2 = np.asarray(X2, dtype=np.float64)
    n1, p = X1.shape
    n2 = X2.shape[0]
    Z1 = np.asarray(Z1, dtype=np.float64).reshape(n1, -1)
    Z2 = np.asarray(Z2, dtype=np.float64).reshape(n2, -1)
    B = Z1.shape[1] + 1
    X1, X2 = X1.astype(LD), X2.astype(LD)
    th = np.asarray(theta, dtype=np.float64).astype(LD)
    K = np.empty((B, n1, n2), dtype=LD)
    R2 = np.empty((B, n1, n2), dtype=LD)
    for b in range(B):
        r2 = np.zeros((n1, n2), dtype=LD)
        for i in range(p):
            d = X1[:, i][:, None] - X2[:, i][None, :]
            r2 += d * d * np.exp(-th[1 + b + B * (i + 1)])
        if kernel == "SE":
            k = np.exp(th[2 + b] - r2)
        else:
            t = np.sqrt(r2)
            s3 = np.sqrt(LD(3))
            k = (1 + s3 * t) * np.exp(th[2 + b] - s3 * t)
        if b >= 1:
            k = k * Z1[:, b - 1].astype(LD)[:, None] * Z2[:, b - 1].astype(LD)[None, :]
        K[b], R2[b] = k, r2
    return K, R2


def k_bound(kernel, X1, X2, Z1, Z2, theta, slices=False):
    """(K_ref, bound), both (n1, n2) longdouble: the extended-precision K and
    the per-element bound of the module docstring.  slices=True: (K_ref,
    bound, Kb_ref, bound_b) with the (B, n1, n2) slices and their bounds."""
    X1 = np.asarray(X1, dtype=np.float64)
    X2 = np.asarray(X2, dtype=np.float64)
    n1, p = X1.shape
    n2 = X2.shape[0]
    Z1 = np.asarray(Z1, dtype=np.float64).reshape(n1, -1)
    Z2 = np.asarray(Z2, dtype=np.float64).reshape(n2, -1)
    B = Z1.shape[1] + 1
    th = np.asarray(theta, dtype=np.float64).astype(LD)
    Kb, R2 = kernel_slices_ld(kernel, X1, X2, Z1, Z2, theta)
    PM = pm_bucket(p)
    u = LD(U)
    s3 = np.sqrt(LD(3))
    bound = np.zeros_like(Kb)
    with np.errstate(divide="ignore"):
        for b in range(B):
            w = np.exp(-th[[1 + b + B * (i + 1) for i in range(p)]])
            s1 = (X1.astype(LD) ** 2) @ w
            s2 = (X2.astype(LD) ** 2) @ w
            delta = 2 * (PM + 4) * u * (s1[:, None] + s2[None, :])
            lam = th[2 + b]
            if b >= 1:
                z1, z2 = Z1[:, b - 1].astype(LD), Z2[:, b - 1].astype(LD)
            else:
                z1, z2 = np.ones(n1, dtype=LD), np.ones(n2, dtype=LD)
            zero = (z1 == 0)[:, None] | (z2 == 0)[None, :]
            l1 = np.abs(np.log(np.abs(np.where(z1 == 0, 1, z1))))
            l2 = np.abs(np.log(np.abs(np.where(z2 == 0, 1, z2))))
            if kernel == "SE":
                M = np.abs(lam) + R2[b] + l1[:, None] + l2[None, :]
                bb = np.abs(Kb[b]) * (delta + 8 * u * (1 + M))
            else:
                t = np.sqrt(R2[b])
                tm = np.sqrt(np.maximum(R2[b] - delta, 0))
                zz = np.abs(z1)[:, None] * np.abs(z2)[None, :]
                zmax = np.maximum(np.abs(z1)[:, None], np.abs(z2)[None, :])
                bb = zz * LD(1.5) * np.exp(lam - s3 * tm) * delta \
                    + np.abs(Kb[b]) * 8 * u * (1 + np.abs(lam) + s3 * t) \
                    + LD(DENORM_ULP) * ((1 + s3 * t) * zz + zmax)
            assert np.all(Kb[b][zero] == 0)
            bound[b] = np.where(zero, 0, bb)
    full = (Kb.sum(axis=0), bound.sum(axis=0) + LD(TINY))
    return full + (Kb, np.where(Kb == 0, 0, bound + LD(TINY))) if slices else full


@functools.lru_cache(maxsize=None)
def cross_points(name, p, B, n1=70, n2=45, seed=3):
    """The 70 x 45 cross case of a regime: X2 / Z2 the regime's n2 points;
    rows of X1 are in turn an exact copy of a row of X2, that row shifted by
    5, shifted by 50 (extrapolation after normalize_test), and a fresh point
    of the regime."""
    _, X2, Z2, th, _ = regime(name, n2, p, B, seed)
    _, X1, Z1, _, _ = regime(name, n1, p, B, seed + 1)
    X1 = np.array(X1, order="F")
    for r in range(n1):
        k = r % 4
        if k < 3:
            X1[r] = X2[(3 * r) % n2] + (0.0, 5.0, 50.0)[k]
    return X1, X2, Z1, Z2, th
