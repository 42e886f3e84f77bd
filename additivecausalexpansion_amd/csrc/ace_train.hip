// ace_train.hip -- the per-iteration host tail of ace.train on the device, so
// that the training loop (R/main_ace.R:213-235) enqueues iteration after
// iteration without a host round trip.
//
//   k_make_tab   : the theta tables of make_tab (ace_common.h) from the
//                  device theta, plus exp(theta[0]) for the diagonal;
//   k_train_step : para_update's gradient and stats, the norm clip, the
//                  optimizer, the mu overwrite (R/kernel_SE_R6.R:45,58) and
//                  the convergence test (R/main_ace.R:221-226), one workgroup.
//
// The arithmetic is that of ace_formulas.h (tab_weight, grad_entry,
// train_stats, clip_on, opt_update), shared with the host and the batched
// engine; this file keeps the table layout and the order of the sums.
#include "../../include/ace_hip.h"
#include "ace_internal.h"

namespace ace {

__global__ void k_make_tab(const double *__restrict__ th, int B, int p, int PM,
                           double *__restrict__ tab) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int nk = B * PM;
  if (e < 2 * nk) {
    const int gi = e >= nk;  // 0: kernel weights (Q1 index), 1: gradient weights
    const int q = e - gi * nk;
    const int b = q / PM, i = q - b * PM;
    double v = 0.0;
    if (i < p) v = tab_weight(th, B, b, i, gi);
    tab[e] = v;
  } else if (e < 2 * nk + B) {
    tab[e] = th[2 + (e - 2 * nk)];
  } else if (e == 2 * nk + B) {
    tab[e] = exp(th[0]);
  }
}

hipError_t launch_make_tab(const double *theta, int B, int p, int PM, double *tab,
                           hipStream_t st) {
  const int total = 2 * B * PM + B + 1;
  hipLaunchKernelGGL(k_make_tab, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, theta,
                     B, p, PM, tab);
  return hipGetLastError();
}

namespace {

// block sum of 1024 threads, every thread gets the result; the 16 partials
// are added in sequence (that order is part of the training loop's results)
__device__ __forceinline__ double bsum(double v, double *sh) {
  v = wsum64(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  double r = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q) r += sh[q];
  __syncthreads();
  return r;
}

}  // namespace

__global__ __launch_bounds__(1024) void k_train_step(TrainCfg c, int it,
                                                     const double *__restrict__ gsum,
                                                     const double *__restrict__ sums,
                                                     const double *__restrict__ scal,
                                                     const int *__restrict__ flag,
                                                     double *__restrict__ st,
                                                     double *__restrict__ hist,
                                                     int *__restrict__ ctl) {
  __shared__ double sh[16];
  if (ctl[1] != 0) return;  // stopped at an earlier iteration: this one is discarded
  const int P = c.P, B = c.B, PM = c.PM, tid = threadIdx.x;
  double *th = st, *m1 = st + P, *m2 = st + 2 * P, *g = st + 3 * P, *prev = st + 4 * P;
  // the theta this iteration's evaluation ran at: the host re-runs it into
  // the resident inverse when later, discarded iterations overwrote it
  // (Q6: predict uses invKmatn of the last para_update, R/kernel_SE_R6.R:37)
  for (int j = tid; j < P; j += 1024) prev[j] = th[j];
  __syncthreads();
  const double kNaN = __builtin_nan("");
  const double mu = scal[3];
  const bool bad = *flag != 0;  // not positive definite: non-finite outputs
  // theta[1] <- mu_solution at iter 1 happens before the gradient in
  // para_update, but grad_entry does not read theta[1]
  for (int j = tid; j < P; j += 1024) {
    const double v = grad_entry(c.kind, B, PM, th, gsum, sums[2], j);
    g[j] = bad ? kNaN : v;
  }
  double s0, s1;
  train_stats(c.std_y, (double)c.n, sums[0], sums[3], sums[1], &s0, &s1);
  if (bad) s0 = s1 = kNaN;
  if (tid == 0) {
    hist[2 * it] = s0;
    hist[2 * it + 1] = s1;
    if (it == 1) th[1] = mu;  // mean_solution before the gradient (R/kernel_SE_R6.R:45)
  }
  __syncthreads();
  // Optim$update: norm clip, then the finite test and the step
  double ss = 0.0, nf = 0.0;
  for (int j = tid; j < P; j += 1024) {
    ss += g[j] * g[j];
    nf += isfinite(g[j]) ? 0.0 : 1.0;
  }
  ss = bsum(ss, sh);
  nf = bsum(nf, sh);
  const double L2 = sqrt(ss);
  const bool clip = clip_on(c.opt, L2);
  if (nf > 0.0) {  // the optimizer classes' stop(): theta stays as it was
    if (tid == 0) {
      ctl[0] = it;
      ctl[1] = 2;
    }
    return;
  }
  const double c1 = 1 - pow(c.opt.beta1, (double)it), c2 = 1 - pow(c.opt.beta2, (double)it);
  for (int j = tid; j < P; j += 1024) {
    const double gj = clip ? g[j] / L2 : g[j];
    th[j] = opt_update(c.opt, c1, c2, gj, th[j], m1, m2, j);
  }
  __syncthreads();
  if (tid == 0) {
    th[1] = mu;  // private$mean_solution(y) with this iteration's inverse
    const double change = fabs(s1 - hist[2 * (it - 1) + 1]);
    ctl[0] = it;
    if (change < c.opt.tol && it > 3) ctl[1] = 1;
  }
}

hipError_t launch_train_step(const TrainCfg &c, int it, const double *gsum, const double *sums,
                             const double *scal, const int *flag, double *st, double *hist,
                             int *ctl, hipStream_t stream) {
  hipLaunchKernelGGL(k_train_step, dim3(1), dim3(1024), 0, stream, c, it, gsum, sums, scal, flag,
                     st, hist, ctl);
  return hipGetLastError();
}

}  // namespace ace
