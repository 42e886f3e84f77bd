// ace_batch.hip -- many small models at once: one workgroup runs one model's
// whole para_update.
//
//   k_batch_eval<KIND, PM> : theta tables, assembly of A = sum_b K_b + e^theta0 I,
//                            in-place SPD inverse + log-determinant with the
//                            right-hand sides [y, 1] carried along, alpha, the
//                            gradient sums, and the composed gradient / stats;
//   k_batch_step           : the training loop's per-iteration tail (clip,
//                            optimizer, mu overwrite, stop tests), one wave
//                            per model.
//
// The arithmetic is that of ace_formulas.h (kval, tab_weight, grad_entry,
// train_stats, clip_on, opt_update), shared with the host and the single-model
// kernels; this file keeps the LDS layouts and the order of every sum.
//
// Workgroup j touches model j's data and scratch only: no grid barrier, no
// flag polling, no atomics -- a launch needs no co-residency and never waits
// on another workgroup.  Every loop is bounded by n_j, p and B.  Every
// reduction runs in a fixed order, so a model's outputs depend neither on M
// nor on its position in the batch.
//
// The inverse is the symmetric Gauss-Jordan sweep of ace_sweep.hip at a block
// width of one MFMA fragment: for pivot block K (16 indices)
//   P = A[:, K] (all rows, from the lower triangle and its mirror), D = A[K, K]
//   N = sweep(D) = -D^-1 (16 scalar steps in LDS; the pivots give log det A)
//   W = P D^-1;  A[i, j] -= W_i P_j^T for i, j outside K  (v_mfma_f64_16x16x4_f64,
//   W and P staged in LDS);  A[:, K] = W;  A[K, K] = N.
// After the last block the n x n part holds -A^-1 (lower), the two rows under
// it (A^-1 [y, 1])^T and their corner -[y, 1]^T A^-1 [y, 1].  k_cv_fold
// (ace_cv.hip) holds the same loop with one statement changed (it records the
// first bad pivot's index): a correction to either belongs in both.  Their
// geometry and LDS map are stated once, in ace_wg_geom.h.
#include "../../include/ace_hip.h"
#include "ace_batch.h"
#include "ace_internal.h"

namespace ace {

// LDS: the sweep's map (ace_wg_geom.h).  The region behind its fixed head is
// used twice: by the sweep as the panels P and W, before and after it as the
// theta tables (wk | wg | lam | e^theta0), alpha, the gradient sums and a
// reduction pad.
size_t batch_lds_bytes(int nmax, int B, int PM) {
  const size_t sweep = (size_t)wg_sweep_lds_bytes(nmax);
  const size_t rest = (size_t)(2 * B * PM + B + 1) + (size_t)nmax + (size_t)(B * (PM + 1) + 1) +
                      (size_t)(batch_threads(PM) / 64) * (PM + 1) + 8;
  return std::max(sweep, (WG_L_REG + rest) * sizeof(double));
}

template <int KIND, int PM>
__global__ __launch_bounds__(batch_threads(PM)) void k_batch_eval(BatchView a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int GC = PM > 32 ? 32 : PM;  // length-scale sums per gradient pass
  constexpr int NTHR = batch_threads(PM), NW = NTHR / 64;
  const int j = blockIdx.x;
  if (a.ctl) {
    const int stop = a.ctl[2 * j + 1];
    if ((a.skip == 1 && stop != 0) || (a.skip == 2 && stop == 2)) return;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = a.n[j], B = a.B, p = a.p, ZS = a.ZS;
  const int npad = (n + BT - 1) / BT * BT, Nt = npad + BT, nt = Nt / BT;
  const int64_t ld = a.ld;
  const int pitch = wg_pitch(a.nmax);
  const double *__restrict__ X = a.X + (int64_t)j * a.nmax * PM;
  const double *__restrict__ Z = a.Z + (int64_t)j * a.nmax * ZS;
  const double *__restrict__ LZ = a.LZ + (int64_t)j * a.nmax * ZS;
  const double *__restrict__ y = a.y + (int64_t)j * a.nmax;
  const double *__restrict__ th = a.theta + (int64_t)j * a.ldt;
  double *A = a.A + (int64_t)j * ld * ld;
  double *out = a.out + (int64_t)j * a.ldo;

  double *sScal = lds + WG_L_SCAL, *sD = lds + WG_L_D, *reg = lds + WG_L_REG;
  double *sP = reg, *sW = reg + BT * pitch;
  const int nk = B * PM;
  double *sWk = reg, *sWg = reg + nk, *sLam = reg + 2 * nk;  // e^theta0 at sLam[B]
  double *sAl = sLam + B + 1, *sG = sAl + a.nmax;
  double *sRed = sG + (B * (PM + 1) + 1), *sSum = sRed + NW * (PM + 1);

  // ---- theta tables (make_tab / k_make_tab) --------------------------------
  auto tables = [&]() {
    for (int e = tid; e < 2 * nk + B + 1; e += NTHR) {
      double v = 0.0;
      if (e < 2 * nk) {
        const int gi = e >= nk, q = e - gi * nk, b = q / PM, i = q - b * PM;
        if (i < p) v = tab_weight(th, B, b, i, gi);
      } else if (e < 2 * nk + B) {
        v = th[2 + (e - 2 * nk)];
      } else {
        v = exp(th[0]);
      }
      reg[e] = v;
    }
    __syncthreads();
  };
  tables();

  // ---- assembly: lane = row r, columns c <= r in a wave-uniform loop --------
  for (int h = 0; NTHR * h < Nt; ++h) {  // (the right-hand-side rows can lie past 512)
    const int wbase = NTHR * h + 64 * wv;
    if (wbase >= Nt) continue;
    const int r = wbase + lane;
    const bool rin = r < n;
    double xr[PM];
#pragma unroll
    for (int i = 0; i < PM; ++i) xr[i] = rin ? X[(int64_t)r * PM + i] : 0.0;
    const int cend = min(wbase + 63, Nt - 1);
    for (int c = 0; c <= cend; ++c) {
      if (r >= Nt || c > r) continue;
      double v;
      if (rin) {  // c <= r < n: c is the reference's first operand
        double kf = 0.0;
        for (int b = 0; b < B; ++b) {
          double r2 = 0.0;
#pragma unroll
          for (int i = 0; i < PM; ++i) {
            const double d = xr[i] - X[(int64_t)c * PM + i];
            r2 = fma(d * d, sWk[b * PM + i], r2);
          }
          double zr = 0.0, zc = 0.0, lzr = 0.0, lzc = 0.0;
          if (b > 0) {
            zr = Z[(int64_t)r * ZS + b - 1];
            zc = Z[(int64_t)c * ZS + b - 1];
            if (KIND == 0) {
              lzr = LZ[(int64_t)r * ZS + b - 1];
              lzc = LZ[(int64_t)c * ZS + b - 1];
            }
          }
          kf += kval<KIND, false>(b, r2, sLam[b], zc, zr, lzc, lzr);  // c: the smaller index
        }
        v = (r == c) ? kf + sLam[B] : kf;
      } else if (r < npad) {
        v = (r == c) ? 1.0 : 0.0;  // identity padding
      } else if (c < n) {
        v = (r == npad) ? y[c] : (r == npad + 1 ? 1.0 : 0.0);  // right-hand sides
      } else {
        v = 0.0;
      }
      A[r + (int64_t)c * ld] = v;
    }
  }
  __syncthreads();

  // ---- sweep ----------------------------------------------------------------
  const int lr = lane & 15, lk = lane >> 4;
  // this thread's element of the pivot block (the first 256 threads hold one)
  const bool dth = tid < BT * BT;
  const int da = dth ? tid >> 4 : 0, db = tid & 15;
  double logdet = 0.0;                     // thread 0's
  int bad = 0;
  const int nb2 = (nt + 1) / 2;
  for (int kt = 0; kt < npad / BT; ++kt) {
    const int k0 = kt * BT;
    // the panel: sP[k][i] = A(i, k0 + k) for every row i
    for (int i = tid; i < Nt; i += NTHR) {
#pragma unroll
      for (int k = 0; k < BT; ++k) {
        const int c = k0 + k;
        sP[k * pitch + i] = (i >= c) ? A[i + (int64_t)c * ld] : A[c + (int64_t)i * ld];
      }
    }
    // the pivot block, swept in registers; row / column s goes through LDS
    double d = 0.0;
    if (dth) {
      const int r = k0 + da, c = k0 + db;
      d = (r >= c) ? A[r + (int64_t)c * ld] : A[c + (int64_t)r * ld];
    }
#pragma unroll 1
    for (int s = 0; s < BT; ++s) {
      double *buf = sD + (s & 1) * BT * WG_DP;
      if (dth && (da == s || db == s)) buf[da * WG_DP + db] = d;
      __syncthreads();
      const double piv = buf[s * WG_DP + s];
      const double das = buf[da * WG_DP + s], dsb = buf[s * WG_DP + db];
      const double rp = 1.0 / piv;
      if (tid == 0) {
        logdet += log(piv);
        if (!(piv > 0.0) || !isfinite(piv)) bad = 1;
      }
      if (da == s && db == s) d = -rp;
      else if (da == s) d = dsb * rp;
      else if (db == s) d = das * rp;
      else d = d - (das * dsb) * rp;
    }
    __syncthreads();
    if (dth) sD[da * WG_DP + db] = d;  // N = -D^-1
    if (dth && da >= db) A[(k0 + da) + (int64_t)(k0 + db) * ld] = d;
    __syncthreads();
    // W = P D^-1 = -P N: to A's column block (and its mirror), -W to LDS
    for (int i = tid; i < Nt; i += NTHR) {
      if (i >= k0 && i < k0 + BT) {
#pragma unroll
        for (int k = 0; k < BT; ++k) {
          sP[k * pitch + i] = 0.0;
          sW[k * pitch + i] = 0.0;
        }
        continue;
      }
      double pr[BT];
#pragma unroll
      for (int l = 0; l < BT; ++l) pr[l] = sP[l * pitch + i];
#pragma unroll
      for (int k = 0; k < BT; ++k) {
        double s = 0.0;
#pragma unroll
        for (int l = 0; l < BT; ++l) s = fma(pr[l], sD[l * WG_DP + k], s);
        sW[k * pitch + i] = s;  // -W
        if (i > k0) A[i + (int64_t)(k0 + k) * ld] = -s;
        else A[(k0 + k) + (int64_t)i * ld] = -s;
      }
    }
    __syncthreads();
    // A[i, j] += (-W_i) P_j^T over the lower 16-tiles outside K, 2 x 2 tiles a
    // turn.  The fragment is the transposed tile (rows = j, columns = i), so a
    // lane's four results lie in four columns of A at 16 adjacent rows.
    int turn = 0;
    for (int I2 = 0; I2 < nb2; ++I2) {
      for (int J2 = 0; J2 <= I2; ++J2, ++turn) {
        if (turn % NW != wv) continue;
        bool ok[2][2];
        d4 acc[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int v = 0; v < 2; ++v) {
            const int I = 2 * I2 + u, J = 2 * J2 + v;
            ok[u][v] = I < nt && J <= I && I != kt && J != kt;
            if (ok[u][v]) {
#pragma unroll
              for (int q = 0; q < 4; ++q)
                acc[u][v][q] = A[(I * BT + lr) + (int64_t)(J * BT + lk + 4 * q) * ld];
            }
          }
#pragma unroll
        for (int q4 = 0; q4 < BT / 4; ++q4) {
          double wi[2], pj[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            // (a tile past nt is clamped: its products are not used)
            const int I = min(2 * I2 + u, nt - 1), J = min(2 * J2 + u, nt - 1);
            wi[u] = sW[(4 * q4 + lk) * pitch + I * BT + lr];
            pj[u] = sP[(4 * q4 + lk) * pitch + J * BT + lr];
          }
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v)
              if (ok[u][v])
                acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(pj[v], wi[u], acc[u][v], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int v = 0; v < 2; ++v)
            if (ok[u][v]) {
              const int I = 2 * I2 + u, J = 2 * J2 + v;
#pragma unroll
              for (int q = 0; q < 4; ++q)
                A[(I * BT + lr) + (int64_t)(J * BT + lk + 4 * q) * ld] = acc[u][v][q];
            }
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    sScal[0] = logdet;
    sScal[1] = (double)bad;
  }
  tables();  // the panels overwrote them (also the barrier for sScal)

  // ---- alpha, mu_solution (Q4) and the sums of the stats ---------------------
  const double yK1 = -A[(npad + 1) + (int64_t)npad * ld];
  const double oK1 = -A[(npad + 1) + (int64_t)(npad + 1) * ld];
  const double mu = 0.5 * yK1 / oK1;
  const double mu_eff = a.use_mu ? mu : th[1];
  const double esig = sLam[B];
  double e2 = 0.0, ya = 0.0, sa = 0.0;
  for (int i = tid; i < n; i += NTHR) {
    const double al = A[npad + (int64_t)i * ld] - mu_eff * A[(npad + 1) + (int64_t)i * ld];
    sAl[i] = al;
    const double e = esig * al;  // ybar - Kfull alpha = e^theta0 alpha
    e2 += e * e;
    ya += y[i] * al;  // Q3: y, not y - mu
    sa += al;
  }
  for (int e = tid; e < B * (PM + 1) + 1; e += NTHR) sG[e] = 0.0;
  e2 = block_sum<NW>(e2, sSum);
  ya = block_sum<NW>(ya, sSum);
  sa = block_sum<NW>(sa, sSum);

  // ---- gradient sums: T = A^-1 - alpha alpha^T over the lower pairs ---------
  for (int h = 0; NTHR * h < n; ++h) {  // (block-uniform)
    const int wbase = NTHR * h + 64 * wv;
    const int r = wbase + lane;
    const bool rin = r < n;
    double xr[PM];
#pragma unroll
    for (int i = 0; i < PM; ++i) xr[i] = rin ? X[(int64_t)r * PM + i] : 0.0;
    const double ar = rin ? sAl[r] : 0.0;
    const int cend = wbase < n ? min(wbase + 63, n - 1) : -1;  // a wave past n: no pairs
    // the length-scale sums GC features at a time (GC = 32 at PM = 64, where
    // x_r and 64 running sums together would not fit the register file)
    for (int b = 0; b < B; ++b) {
      double zr = 0.0, lzr = 0.0;
      if (b > 0 && rin) {
        zr = Z[(int64_t)r * ZS + b - 1];
        if (KIND == 0) lzr = LZ[(int64_t)r * ZS + b - 1];
      }
      const double lam = sLam[b];
#pragma unroll 1
      for (int i0 = 0; i0 < PM; i0 += GC) {
        double g[GC];
#pragma unroll
        for (int i = 0; i < GC; ++i) g[i] = 0.0;
        double gl = 0.0, tr = 0.0;
        for (int c = 0; c <= cend; ++c) {
          if (!rin || c > r) continue;
          double t = -A[r + (int64_t)c * ld] - ar * sAl[c];
          if (c == r) tr += t;
          else t *= 2.0;
          double r2 = 0.0, rt2 = 0.0;
#pragma unroll
          for (int i = 0; i < PM; ++i) {
            const double dd = xr[i] - X[(int64_t)c * PM + i];
            const double d2 = dd * dd;
            r2 = fma(d2, sWk[b * PM + i], r2);
            if (KIND == 1) rt2 = fma(d2, sWg[b * PM + i], rt2);  // Q2: gradient-indexed
          }
          double zc = 0.0, lzc = 0.0;
          if (b > 0) {
            zc = Z[(int64_t)c * ZS + b - 1];
            if (KIND == 0) lzc = LZ[(int64_t)c * ZS + b - 1];
          }
          const double kb = kval<KIND, false>(b, r2, lam, zc, zr, lzc, lzr);
          gl = fma(t, kb, gl);
          const double U = KIND == 0 ? t * kb : t * (kb / (1.0 + sqrt(3.0 * rt2)));
          if (GC == PM) {
#pragma unroll
            for (int i = 0; i < GC; ++i) {
              const double dd = xr[i] - X[(int64_t)c * PM + i];
              g[i] = fma(U, dd * dd, g[i]);
            }
          } else if (i0 == 0) {
#pragma unroll
            for (int i = 0; i < GC; ++i) {
              const double dd = xr[i] - X[(int64_t)c * PM + i];
              g[i] = fma(U, dd * dd, g[i]);
            }
          } else {
#pragma unroll
            for (int i = 0; i < GC; ++i) {
              const double dd = xr[(PM - GC) + i] - X[(int64_t)c * PM + (PM - GC) + i];
              g[i] = fma(U, dd * dd, g[i]);
            }
          }
        }
        // fixed-order reduction: lanes of a wave, then the waves
#pragma unroll
        for (int i = 0; i < GC; ++i) {
          const double v = wsum64(g[i]);
          if (lane == 0) sRed[wv * (PM + 1) + i0 + i] = v;
        }
        if (i0 == 0) {
          const double v = wsum64(gl);
          if (lane == 0) sRed[wv * (PM + 1) + PM] = v;
          const double w = wsum64(tr);
          if (lane == 0) sSum[wv] = w;
        }
      }
      __syncthreads();
      if (tid <= PM)
        sG[b * (PM + 1) + tid] += wave_parts<NW>(sRed + tid, PM + 1);
      if (tid == 0 && b == 0) sG[B * (PM + 1)] += wave_parts<NW>(sSum, 1);
      __syncthreads();
    }
  }
  __syncthreads();

  // ---- the gradient and the stats -------------------------------------------
  const double kNaN = __builtin_nan("");
  const bool flag = sScal[1] != 0.0;
  const int P = a.P;
  for (int q = tid; q < P; q += NTHR) {
    const double v = grad_entry(KIND, B, PM, th, sG, sa, q);  // KIND: an ace_kernel_kind
    out[q] = flag ? kNaN : v;
  }
  if (tid == 0) {
    double s0, s1;
    train_stats(a.std_y[j], (double)n, e2, sScal[0], ya, &s0, &s1);
    out[P] = flag ? kNaN : s0;
    out[P + 1] = flag ? kNaN : s1;
    out[P + 2] = flag ? kNaN : mu;
    out[P + 3] = flag ? 1.0 : 0.0;
  }
}

// ---------------------------------------------------------------------------
// One wave per model: norm clip (clip_on), the optimizer (opt_update), the mu
// overwrite, the stats history, the convergence test and the non-finite stop,
// as k_train_step.  A stopped model is left alone from then on.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_batch_step(BatchStepCfg c, int it,
                                                   const double *__restrict__ outp, int64_t ldo,
                                                   double *__restrict__ stp,
                                                   double *__restrict__ histp, int64_t ldh,
                                                   int *__restrict__ ctlp) {
  const int j = blockIdx.x, tid = threadIdx.x, P = c.P;
  int *ctl = ctlp + 2 * j;
  if (ctl[1] != 0) return;
  const double *g = outp + (int64_t)j * ldo;
  double *th = stp + (int64_t)j * 3 * P, *m1 = th + P, *m2 = th + 2 * P;
  double *hist = histp + (int64_t)j * ldh;
  const double s1 = g[P + 1], mu = g[P + 2];
  double ss = 0.0, nf = 0.0;
  for (int q = tid; q < P; q += 64) {
    ss += g[q] * g[q];
    nf += isfinite(g[q]) ? 0.0 : 1.0;
  }
  ss = wsum64(ss);
  nf = wsum64(nf);
  const double prev = hist[2 * (it - 1) + 1];
  if (tid == 0) {
    hist[2 * it] = g[P];
    hist[2 * it + 1] = s1;
  }
  const double L2 = sqrt(ss);
  const bool clip = clip_on(c.opt, L2);
  if (nf > 0.0) {  // the optimizer classes' stop(): theta stays as it was
    if (tid == 0) {
      if (it == 1) th[1] = mu;  // assigned before the optimizer runs
      ctl[0] = it;
      ctl[1] = 2;
    }
    return;
  }
  const double c1 = 1 - pow(c.opt.beta1, (double)it), c2 = 1 - pow(c.opt.beta2, (double)it);
  for (int q = tid; q < P; q += 64) {
    const double gj = clip ? g[q] / L2 : g[q];
    // theta[1] <- mu at iteration 1 comes before the step (R/kernel_SE_R6.R:45)
    const double t = opt_update(c.opt, c1, c2, gj, (it == 1 && q == 1) ? mu : th[q], m1, m2, q);
    th[q] = (q == 1) ? mu : t;  // private$mean_solution(y) with this iteration's inverse
  }
  if (tid == 0) {
    ctl[0] = it;
    if (fabs(s1 - prev) < c.opt.tol && it > 3) ctl[1] = 1;
  }
}

int batch_pm_bucket(int p) {
  for (int b : {4, 8, 16, 32, 64})
    if (p <= b) return b;
  return -1;
}

template <int KIND, int PM>
static hipError_t eval_pm(const BatchView &v, hipStream_t st) {
  return launch_lds(k_batch_eval<KIND, PM>, dim3((unsigned)v.M), dim3(batch_threads(PM)),
                    batch_lds_bytes(v.nmax, v.B, PM), st, v);
}

hipError_t launch_batch_eval(int kind, const BatchView &v, hipStream_t st) {
  if (v.M <= 0) return hipSuccess;
  if (v.nmax > BATCH_NMAX || batch_lds_bytes(v.nmax, v.B, v.PM) > LDS_MAX)
    return hipErrorInvalidValue;
  switch (v.PM) {
#define ACE_CASE(Q) \
  case Q:           \
    return kind == 0 ? eval_pm<0, Q>(v, st) : eval_pm<1, Q>(v, st);
    ACE_CASE(4) ACE_CASE(8) ACE_CASE(16) ACE_CASE(32) ACE_CASE(64)
#undef ACE_CASE
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_batch_step(const BatchStepCfg &c, int it, const double *out, int64_t ldo,
                             double *st, double *hist, int64_t ldh, int *ctl, hipStream_t stream) {
  hipLaunchKernelGGL(k_batch_step, dim3((unsigned)c.M), dim3(64), 0, stream, c, it, out, ldo, st,
                     hist, ldh, ctl);
  return hipGetLastError();
}

}  // namespace ace
