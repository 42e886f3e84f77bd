// ace_formulas.h -- the model's arithmetic, each formula stated once for the
// host and for every kernel.  The Q-numbered rules, where the reference's
// behaviour is matched on purpose, live here and nowhere else: the Q1 index
// rule (tab_weight), the Q5 clip predicate (clip_on), the Q7 zero rules
// (kval) and the Q8 optimizer updates (opt_update).  Two statements stay
// outside on purpose: the MFMA pair kernels' branch-free slice value with its
// table exponentials (kval_nb, ace_pairs_mm.hip), and the host ABI optimizers
// (ace_nadam and the others, ace_host.cpp), which mirror the reference's own
// spelling; clip_on and opt_update are called by the two step kernels only.
// Callers keep their own table layouts, reduction orders and NaN handling.
// exp / sqrt / log are unqualified, so host and device each get their own.
// The device-only helpers of the kernels (d4, the wave and workgroup sums)
// follow below.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/ace_hip.h"

namespace ace {

constexpr double SQRT3 = 1.7320508075688772;

__host__ __device__ __forceinline__ double sgn(double x) {
  return (double)((0.0 < x) - (x < 0.0));
}

// One slice value K_b for a pair, following the reference expressions:
//  SE  (src/kernel_SE_cpp.cpp:96, 119 / 39, 53): slice 0 exp(lam - r2);
//      b>=1: sign(z_lo) sign(z_hi) exp(((lam - r2) + log|z_lo|) + log|z_hi|),
//      0 if either z is exactly 0 (Q7).
//  Matern32 (src/kernel_Matern_cpp.cpp:217-227 / 79-86): t = sqrt(r2),
//      e = (1 + sqrt3 t) exp(lam - sqrt3 t); b>=1: (e z_lo) z_hi, 0 if
//      z_lo == 0 (and, in the cross kernel, if z_hi == 0).
// "lo" is the first operand of the reference's product: the smaller index
// of a symmetric pair (upper-triangle loop), the X1/Z1 side of a cross pair.
template <int KIND, bool CROSS>
__host__ __device__ __forceinline__ double kval(int b, double r2, double lam, double zlo,
                                                double zhi, double lzlo, double lzhi) {
  if (KIND == 0) {
    if (b == 0) return exp(lam - r2);
    if (zlo == 0.0 || zhi == 0.0) return 0.0;
    return (sgn(zlo) * sgn(zhi)) * exp(((lam - r2) + lzlo) + lzhi);
  } else {
    const double t = sqrt(r2);
    const double e = (1.0 + SQRT3 * t) * exp(lam - SQRT3 * t);
    if (b == 0) return e;
    if (zlo == 0.0) return 0.0;
    if (CROSS && zhi == 0.0) return 0.0;
    return (e * zlo) * zhi;
  }
}

// Theta-table weight of slice b, feature i (Q1): the kernel reads its length
// scale one feature further on than the gradient entry that differentiates it.
__host__ __device__ __forceinline__ double tab_weight(const double *th, int B, int b, int i,
                                                      bool grad) {
  return exp(-th[grad ? 2 + B + b + B * i : 1 + b + B * (i + 1)]);
}

// Element j of the P-gradient from the device sums (P = 2 + B (p + 1)).
//   gsum[b*(PM+1)+i] : sum T K_b d_i^2 (SE) / sum T K_b/(1+sqrt(3 r~2)) d_i^2 (Matern)
//   gsum[b*(PM+1)+PM]: sum T K_b ; gsum[B*(PM+1)] : trace T
// theta[1] is not read (its mu_solution overwrite may come before or after).
__host__ __device__ __forceinline__ double grad_entry(int kind, int B, int PM, const double *th,
                                                      const double *gsum, double sum_alpha,
                                                      int j) {
  if (j == 0) return -0.5 * gsum[B * (PM + 1)] * exp(th[0]);  // sigma_gradient
  if (j == 1) return kind == ACE_KERNEL_SE ? sum_alpha : 0.0;
  if (j < 2 + B) return -0.5 * gsum[(j - 2) * (PM + 1) + PM];
  const int q = j - 2 - B, b = q % B, i = q / B;
  const double sum = gsum[b * (PM + 1) + i], w = tab_weight(th, B, b, i, true);
  return kind == ACE_KERNEL_SE ? -0.5 * (sum * w) : -0.25 * 9 * sum * w;
}

// The two train stats: the RMSE on the response's scale from e2 = sum of the
// squared residuals, and the log evidence from log det and quad = y^T alpha.
__host__ __device__ __forceinline__ void train_stats(double std_y, double n, double e2,
                                                     double logdet, double quad, double *s0,
                                                     double *s1) {
  *s0 = std_y * sqrt(e2) / sqrt(n);
  *s1 = -0.5 * (n * log(2.0 * M_PI) + logdet + quad);
}

// Optim$update's settings, embedded in the step kernels' arguments.
struct OptCfg {
  int optimizer;  // ace_optimizer
  double lr, momentum, beta1, beta2;
  int clip;
  double clip_at, tol;
};
inline OptCfg opt_cfg(int optimizer, double lr, double momentum, double beta1, double beta2,
                      int clip, double clip_at, double tol) {
  return OptCfg{optimizer, lr, momentum, beta1, beta2, clip, clip_at, tol};
}

// Norm clip (src/utilities_cpp.cpp:121-129, Q5): whether a gradient of norm L2
// is divided by it.
__host__ __device__ __forceinline__ bool clip_on(const OptCfg &c, double L2) {
  return c.clip && (L2 > c.clip_at) && isfinite(L2) && (L2 != 0);
}

// One element's optimizer step (src/optimizer_cpp.cpp:8-63, Q8) at iteration
// it, c1 = 1 - beta1^it, c2 = 1 - beta2^it, for gradient element gj and theta
// element th: updates the moments m1[j], m2[j] and returns the new theta.
// Nadam's step uses the updated first moment (Q8).  (The moments come as array
// and index so that each branch forms only the addresses it uses.)
__host__ __device__ __forceinline__ double opt_update(const OptCfg &c, double c1, double c2,
                                                      double gj, double th, double *m1,
                                                      double *m2, int j) {
  const double b1 = c.beta1, b2 = c.beta2, eps = 1e-8;
  if (c.optimizer == ACE_OPT_NESTEROV) {
    m1[j] = c.momentum * m1[j] + c.lr * gj;
    th = th + m1[j];
  } else if (c.optimizer == ACE_OPT_NADAM) {
    m1[j] = b1 * m1[j] + (1 - b1) * gj;
    m2[j] = b2 * m2[j] + (1 - b2) * (gj * gj);
    th = th + c.lr * ((b1 * m1[j] + (1 - b1) * gj) / c1) / (sqrt(m2[j] / c2) + eps);
  } else {
    m1[j] = (b1 * m1[j]) + (1 - b1) * gj;
    m2[j] = b2 * m2[j] + (1 - b2) * (gj * gj);
    th = th + c.lr * (m1[j] / c1) / (sqrt(m2[j] / c2) + eps);
  }
  return th;
}

#ifdef __HIPCC__
// ---- device-only helpers -----------------------------------------------------
typedef double d4 __attribute__((ext_vector_type(4)));

// xor-shuffle sum over the 64 lanes of a wave; every lane gets it
__device__ __forceinline__ double wsum64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the NW per-wave partials at sh[q stride], added in a fixed order
template <int NW>
__device__ __forceinline__ double wave_parts(const double *sh, int stride) {
  double r = (sh[0] + sh[stride]) + (sh[2 * stride] + sh[3 * stride]);
  if (NW == 8)
    r += (sh[4 * stride] + sh[5 * stride]) + (sh[6 * stride] + sh[7 * stride]);
  return r;
}

// sum over a workgroup of NW waves in a fixed order; every thread gets it.
// sh: NW doubles
template <int NW>
__device__ __forceinline__ double block_sum(double v, double *sh) {
  v = wsum64(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = wave_parts<NW>(sh, 1);
  __syncthreads();
  return r;
}
#endif  // __HIPCC__

}  // namespace ace
