// ace_cv.hip -- cross-validation from a resident inverse.
//
// With S = A^-1 in HBM and alpha = S (y - mu 1), a held-out index set F needs
// only the block B_F = S[F, F] and alpha_F:
//   r_F = B_F^-1 alpha_F = y_F - E[y_F | y_-F],  C_F = B_F^-1,
//   lpd_F = -1/2 alpha_F^T r_F + 1/2 log det B_F - (m/2) log 2 pi.
//
//   k_cv_gather    : B_F, alpha_F and the padding into a fold's working matrix
//                    (a workgroup fold's scratch, or a SweepWork's A);
//   k_cv_fold      : one workgroup per fold of up to CV_WG_MAX rows: the
//                    symmetric Gauss-Jordan sweep of [[B_F, alpha_F], [alpha_F^T, 0]]
//                    over its first npad pivots, which leaves -B_F^-1,
//                    B_F^-1 alpha_F and the corner -alpha_F^T B_F^-1 alpha_F;
//                    the pivots give log det B_F;
//   k_cv_loo       : every fold has one row -- one pass over the diagonal;
//   k_cv_sweep_out : the same outputs read out of a whole-chip sweep's
//                    SweepWork (folds above CV_WG_MAX).
//
// Workgroup f of k_cv_fold touches fold f's matrix and outputs only: no grid
// barrier, no flag polling, no atomics; every loop is bounded by the fold's
// size and every sum runs in a fixed order, so a fold's results depend
// neither on the other folds nor on its place in the call.  A bad pivot does
// not leave the loop (every barrier is reached); the fold's outputs are
// overwritten with NaN at the end.
//
// The sweep is the one of k_batch_eval (ace_batch.hip) at a block width of one
// MFMA fragment: for pivot block K (16 indices)
//   P = A[:, K] (all rows, read through the lower triangle), D = A[K, K],
//   N = sweep(D) = -D^-1 (16 scalar steps through LDS),
//   W = P D^-1;  A[i, j] -= W_i P_j^T outside K (v_mfma_f64_16x16x4_f64, W and
//   P staged in LDS);  A[:, K] = W;  A[K, K] = N.
// The loop is k_batch_eval's with one statement changed (the first bad
// pivot's index is recorded, not a flag): a correction to either belongs in
// both.  The working matrix's rows, the LDS map and its size are
// ace_wg_geom.h's, as the plan (ace_cv_plan.cpp) and the batched engine use
// them.
#include "ace_cv.h"
#include "ace_internal.h"

namespace ace {

namespace {

constexpr int FOLD_THREADS = 512;  // eight waves

// One swept fold's outputs, by every thread of its NTHR-thread workgroup: A
// (ld) holds -B_F^-1 in its leading block, B_F^-1 alpha_F in row npad and the
// corner -alpha_F^T B_F^-1 alpha_F.  status != 0: NaN in their place.
template <int NTHR>
__device__ __forceinline__ void fold_out(const double *A, int64_t ld, int64_t npad, const CvDesc &d,
                                         const CvRes &res, double logdet, int status) {
  const double kNaN = __builtin_nan("");
  const bool fail = status != 0;
  for (int64_t k = threadIdx.x; k < d.m; k += NTHR) {
    res.r[d.off + k] = fail ? kNaN : A[npad + k * ld];
    res.v[d.off + k] = fail ? kNaN : -A[k + k * ld];
  }
  if (threadIdx.x == 0) {
    res.logdet[d.fold] = fail ? kNaN : logdet;
    res.mahal[d.fold] = fail ? kNaN : -A[npad + npad * ld];
    res.status[d.fold] = status;
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// blockIdx.x = fold of the list, blockIdx.y = column c of its working matrix;
// the threads walk the rows.  With the fold's rows ascending, column c's
// entries at a >= c come from one source column, read downwards.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cv_gather(CvSrc s, const CvDesc *__restrict__ desc,
                                                   double *__restrict__ W, int64_t npad_sweep,
                                                   double *__restrict__ af) {
  const CvDesc d = desc[blockIdx.x];
  const int64_t c = blockIdx.y, ld = d.ld, m = d.m;
  if (c >= ld) return;
  const bool full = npad_sweep > 0;
  const int64_t npad = full ? npad_sweep : ld - BT;
  double *__restrict__ A = W + d.scratch;
  const int64_t *__restrict__ rows = s.rows + d.off;
  const int64_t rc = c < m ? rows[c] : 0;
  for (int64_t a = threadIdx.x; a < ld; a += 256) {
    if (a < c && (!full || c >= npad)) continue;  // the upper part is not used
    double v = 0.0;
    if (a < m && c < m) {
      const int64_t ra = rows[a];
      const int64_t hi = ra > rc ? ra : rc, lo = ra > rc ? rc : ra;
      v = s.sgn * s.P[hi + lo * s.ldp];
    } else if (a < npad && c < npad) {
      v = (a == c) ? 1.0 : 0.0;  // identity padding
    } else if (a == npad && c < m) {
      v = s.alpha[rc];  // the right-hand side
      if (af) af[c] = v;
    }
    A[a + c * ld] = v;
  }
}

hipError_t launch_cv_gather(const CvSrc &s, const CvDesc *desc, int64_t nd, int64_t ldmax,
                            double *W, int64_t npad_sweep, double *af, hipStream_t st) {
  if (nd <= 0) return hipSuccess;
  if (ldmax > 65535 || nd > 2147483647LL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cv_gather, dim3((unsigned)nd, (unsigned)ldmax), dim3(256), 0, st, s, desc,
                     W, npad_sweep, af);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(FOLD_THREADS) void k_cv_fold(const CvDesc *__restrict__ desc,
                                                          double *__restrict__ Wm, CvRes res,
                                                          int pitch) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int NTHR = FOLD_THREADS, NW = NTHR / 64;
  const CvDesc dsc = desc[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Nt = (int)dsc.ld, npad = Nt - BT, nt = Nt / BT;
  const int64_t ld = dsc.ld;
  double *A = Wm + dsc.scratch;
  double *sScal = lds + WG_L_SCAL, *sD = lds + WG_L_D;
  double *sP = lds + WG_L_REG, *sW = sP + BT * pitch;

  const int lr = lane & 15, lk = lane >> 4;
  // this thread's element of the pivot block (the first 256 threads hold one)
  const bool dth = tid < BT * BT;
  const int da = dth ? tid >> 4 : 0, db = tid & 15;
  double logdet = 0.0;  // thread 0's
  int bad = 0;          // thread 0's: 1-based index of the first bad pivot
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
        if (bad == 0 && (!(piv > 0.0) || !isfinite(piv))) bad = k0 + s + 1;
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
  __syncthreads();
  fold_out<NTHR>(A, ld, npad, dsc, res, sScal[0], (int)sScal[1]);
}

hipError_t launch_cv_fold(const CvDesc *desc, int64_t nd, int64_t mmax, double *W, CvRes res,
                          hipStream_t st) {
  if (nd <= 0) return hipSuccess;
  if (mmax < 1 || mmax > CV_WG_MAX || nd > 2147483647LL) return hipErrorInvalidValue;
  const size_t lds = (size_t)wg_sweep_lds_bytes(mmax);
  if (lds > LDS_MAX) return hipErrorInvalidValue;
  return launch_lds(k_cv_fold, dim3((unsigned)nd), dim3(FOLD_THREADS), lds, st, desc, W, res,
                    (int)wg_pitch(mmax));
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cv_loo(CvSrc s, int64_t nf, CvRes res) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int64_t row = s.rows[f];
  const double p = s.sgn * s.P[row + row * s.ldp], al = s.alpha[row];
  const bool fail = !(p > 0.0) || !isfinite(p);
  const double kNaN = __builtin_nan("");
  const double r = al / p;
  res.r[f] = fail ? kNaN : r;
  res.v[f] = fail ? kNaN : 1.0 / p;
  res.logdet[f] = fail ? kNaN : log(p);
  res.mahal[f] = fail ? kNaN : al * r;
  res.status[f] = fail ? 1 : 0;
}

hipError_t launch_cv_loo(const CvSrc &s, int64_t nf, CvRes res, hipStream_t st) {
  if (nf <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_cv_loo, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, s, nf, res);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// One workgroup: thread t takes the pivots t, t + 256, ...; the partial sums
// of log and the first bad index meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void k_cv_sweep_out(const double *__restrict__ A, int64_t ld,
                                                      int64_t npad, const double *__restrict__ piv,
                                                      const int *__restrict__ flag,
                                                      const CvDesc *__restrict__ desc, CvRes res) {
  __shared__ double sSum[4];
  __shared__ int sBad[256];
  const CvDesc d = desc[0];
  const int tid = threadIdx.x;
  double ls = 0.0;
  int bad = 0;
  for (int64_t k = tid; k < npad; k += 256) {
    const double p = piv[k];
    if (k < d.m) ls += log(p);
    if (bad == 0 && (!(p > 0.0) || !isfinite(p))) bad = (int)(k + 1);
  }
  sBad[tid] = bad;
  ls = block_sum<4>(ls, sSum);  // (its barriers also publish sBad)
  int first = 0;
  for (int t = 0; t < 256; ++t) {
    const int b = sBad[t];
    if (b != 0 && (first == 0 || b < first)) first = b;
  }
  const int fl = *flag;
  fold_out<256>(A, ld, npad, d, res, ls, first != 0 ? first : (fl != 0 ? -fl : 0));
}

hipError_t launch_cv_sweep_out(const double *A, int64_t ld, int64_t npad, const double *piv,
                               const int *flag, const CvDesc *desc, CvRes res, hipStream_t st) {
  hipLaunchKernelGGL(k_cv_sweep_out, dim3(1), dim3(256), 0, st, A, ld, npad, piv, flag, desc, res);
  return hipGetLastError();
}

}  // namespace ace
