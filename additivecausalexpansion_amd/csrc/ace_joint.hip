// ace_joint.hip -- the joint posterior at the test points (ace_predict.cpp,
// ace_model_predict_joint): the covariance C = K_xx - K_xX A^-1 K_xX^T, its
// lower Cholesky factor, and the shift of the draws m 1^T + L Xi.
//
// The reference forms this matrix in full (src/pred_cpp.cpp:22, :72) and
// keeps its diagonal and three quadratic forms; here it is an output.
//
//   k_post_cov      lower 64 x 64 tiles of C from K_xX (nx x n) and
//                   T' = A^-1 K_xX^T (n x nx), K = n, on
//                   v_mfma_f64_16x16x4_f64; every accumulator starts from its
//                   K_xx entries, the entries r >= c are kept and mirrored
//   k_potrf_diag    step k of the blocked right-looking Cholesky (NB = 64):
//                   the diagonal block, one wave, rows in registers
//   k_potrf_solve   the rows below by forward substitution against L_kk in
//                   LDS, one lane per row (no inverted diagonal block)
//   k_potrf_update  the trailing C_IJ -= P_I P_J^T on the lower tiles (the
//                   tile body of k_post_cov with K = 64)
//
// Every sum has a fixed order and nothing is atomic: bitwise reproducible.
// A pivot that is <= 0 or not finite writes its 1-based index to the device
// flag; every later launch of the factor reads the flag first and returns, so
// the first writer is the first bad pivot and no workgroup waits on another.
#include <algorithm>

#include "ace_internal.h"

namespace ace {

constexpr int JT = 64, JBK = 16, JLD = JT + 16;  // tile, k-chunk, LDS pitch (= 16 mod 32)

// acc (rows R0 + 32 wr + 16 ri + lr, columns C0 + 32 wc + 16 ci + lk + 4 j)
// += sum over k < K of (-A[r][k]) B[k][c], 256 threads, BK = 16 chunks through
// double-buffered LDS with a register prefetch (the staging of k_trmm_lower).
// A[r][k] = A[r + k lda], r < nr.  BT: B[k][c] = B[c + k ldb] (the panel of the
// factor's update), else B[k + c ldb]; c < nc.
template <bool BT>
__device__ __forceinline__ void joint_tile(const double *__restrict__ A, int64_t lda, int64_t nr,
                                           const double *__restrict__ B, int64_t ldb, int64_t nc,
                                           int64_t R0, int64_t C0, int64_t K, d4 (&acc)[2][2]) {
  __shared__ __attribute__((aligned(16))) double sA[2][JBK][JLD];  // [k][r - R0], negated
  __shared__ __attribute__((aligned(16))) double sB[2][JBK][JLD];  // [k][c - C0]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4, wr = wv & 1, wc = wv >> 1;
  const int ak = tid >> 4, am = (tid & 15) * 4;  // chunk row ak, 4 consecutive rows / columns
  const int bc = tid >> 2, bk = (tid & 3) * 4;   // !BT: column bc, 4 consecutive k
  double ra[4], rb[4];
  auto load = [&](int64_t kk) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t r = R0 + am + e, k = kk + ak;
      ra[e] = (r < nr && k < K) ? -A[r + k * lda] : 0.0;
    }
    if (BT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t c = C0 + am + e, k = kk + ak;
        rb[e] = (c < nc && k < K) ? B[c + k * ldb] : 0.0;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t c = C0 + bc, k = kk + bk + e;
        rb[e] = (c < nc && k < K) ? B[k + c * ldb] : 0.0;
      }
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sA[buf][ak][am + e] = ra[e];
      if (BT)
        sB[buf][ak][am + e] = rb[e];
      else
        sB[buf][bk + e][bc] = rb[e];
    }
  };
  if (K > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  int buf = 0;
  for (int64_t kk = 0; kk < K; kk += JBK) {
    const bool more = kk + JBK < K;
    if (more) load(kk + JBK);
#pragma unroll
    for (int q4 = 0; q4 < JBK / 4; ++q4) {
      double a[2], b[2];
#pragma unroll
      for (int ci = 0; ci < 2; ++ci) a[ci] = sB[buf][4 * q4 + lk][32 * wc + 16 * ci + lr];
#pragma unroll
      for (int ri = 0; ri < 2; ++ri) b[ri] = sA[buf][4 * q4 + lk][32 * wr + 16 * ri + lr];
#pragma unroll
      for (int ci = 0; ci < 2; ++ci)
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
          acc[ci][ri] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ci], b[ri], acc[ci][ri], 0, 0, 0);
    }
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
}

// C (nx x nx, ldc) = scale (K_xx - K_xX T' + noise I): lower tiles (blockIdx.y
// >= blockIdx.x), entries r >= c, each written to (r, c) and (c, r)
__global__ __launch_bounds__(256) void k_post_cov(const double *__restrict__ Kx, int64_t ldk,
                                                  const double *__restrict__ T, int64_t ldt,
                                                  int64_t n, const double *__restrict__ Kxx,
                                                  int64_t ldx, int64_t nx, double noise,
                                                  double scale, double *__restrict__ C,
                                                  int64_t ldc) {
  if (blockIdx.x > blockIdx.y) return;
  const int64_t R0 = (int64_t)blockIdx.y * JT, C0 = (int64_t)blockIdx.x * JT;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4, wr = wv & 1, wc = wv >> 1;
  d4 acc[2][2];
#pragma unroll
  for (int ci = 0; ci < 2; ++ci)
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
      const int64_t r = R0 + 32 * wr + 16 * ri + lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t c = C0 + 32 * wc + 16 * ci + lk + 4 * j;
        acc[ci][ri][j] = (r < nx && c < nx) ? Kxx[r + c * ldx] : 0.0;
      }
    }
  joint_tile<false>(Kx, ldk, nx, T, ldt, nx, R0, C0, n, acc);
#pragma unroll
  for (int ci = 0; ci < 2; ++ci)
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
      const int64_t r = R0 + 32 * wr + 16 * ri + lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t c = C0 + 32 * wc + 16 * ci + lk + 4 * j;
        if (r < nx && c <= r) {
          const double v = scale * (r == c ? acc[ci][ri][j] + noise : acc[ci][ri][j]);
          C[r + c * ldc] = v;
          if (r != c) C[c + r * ldc] = v;
        }
      }
    }
}

hipError_t launch_post_cov(const double *Kx, int64_t ldk, const double *T, int64_t ldt, int64_t n,
                           const double *Kxx, int64_t ldx, int64_t nx, double noise, double scale,
                           double *C, int64_t ldc, hipStream_t st) {
  if (nx <= 0) return hipSuccess;
  const unsigned nt = (unsigned)((nx + JT - 1) / JT);
  hipLaunchKernelGGL(k_post_cov, dim3(nt, nt), dim3(256), 0, st, Kx, ldk, T, ldt, n, Kxx, ldx, nx,
                     noise, scale, C, ldc);
  return hipGetLastError();
}

// ---------------------------------------------------------------- factor
// L = tril(C) + jitter I, exact zeros above the diagonal
__global__ void k_potrf_init(const double *__restrict__ C, int64_t ldc, int64_t n, double jitter,
                             double *__restrict__ L, int64_t ldl) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (r >= n) return;
  L[r + c * ldl] = r > c ? C[r + c * ldc] : (r == c ? C[r + c * ldc] + jitter : 0.0);
}

// The diagonal block of step j0 / 64 (jb = min(64, n - j0) rows), factored by
// one wave with lane t holding row t in registers (identity rows and columns
// beyond jb): column j is divided by sqrt(pivot) and taken off the columns to
// its right (right-looking); the pivot and the column's entries reach the
// other lanes as wave-uniform lane reads, so the 64 steps need neither LDS nor
// a barrier.  (A first version kept the block in LDS and updated it in place:
// 120 us per block, every update waiting for the previous one's LDS round
// trip.)  Entries right of a lane's diagonal are scratch and never stored.
__device__ __forceinline__ double lane_read(double v, int lane) {  // lane: a constant
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(64) void k_potrf_diag(double *__restrict__ L, int64_t ld, int64_t n,
                                                   int64_t j0, int *__restrict__ flag) {
  if (*flag != 0) return;
  const int t = threadIdx.x;
  const int jb = (int)(n - j0 < JT ? n - j0 : JT);
  double x[JT];
#pragma unroll
  for (int c = 0; c < JT; ++c)
    x[c] = (t < jb && c <= t) ? L[(j0 + t) + (j0 + c) * ld] : (t == c ? 1.0 : 0.0);
  int bad = 0;  // 1-based column of the first bad pivot (the same in every lane)
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    double d = lane_read(x[j], j);
    if (!(d > 0.0) || !isfinite(d)) {  // straight-line: the steps go on with a stand-in
      if (bad == 0) bad = j + 1;
      d = 1.0;
    }
    const double ljj = sqrt(d);
    const double l = t > j ? x[j] / ljj : 0.0;
    x[j] = t == j ? ljj : l;
#pragma unroll
    for (int c = j + 1; c < JT; ++c) x[c] = fma(-l, lane_read(l, c), x[c]);
  }
  if (bad != 0) {  // nothing is stored: the later launches return on the flag
    if (t == 0) *flag = (int)(j0 + bad);
    return;
  }
  if (t < jb) {
#pragma unroll
    for (int c = 0; c < JT; ++c)
      if (c <= t) L[(j0 + t) + (j0 + c) * ld] = x[c];
  }
}

// Rows below a full diagonal block (j0 + 64 < n): x L_kk^T = a by forward
// substitution, one lane per row with the row in registers, L_kk in LDS
// (every lane reads the same entry: a broadcast).  Column-oriented: x_k is
// final after k updates and is then taken off every later entry, so the
// updates of one k are independent of each other.
__global__ __launch_bounds__(64) void k_potrf_solve(double *__restrict__ L, int64_t ld, int64_t n,
                                                    int64_t j0, const int *__restrict__ flag) {
  __shared__ double sD[JT][JT + 1];
  if (*flag != 0) return;
  const int t = threadIdx.x;
  for (int c = 0; c < JT; ++c) sD[t][c] = c <= t ? L[(j0 + t) + (j0 + c) * ld] : 0.0;
  __syncthreads();
  const int64_t i = j0 + JT + (int64_t)blockIdx.x * JT + t;
  if (i >= n) return;
  double x[JT];
#pragma unroll
  for (int j = 0; j < JT; ++j) x[j] = L[i + (j0 + j) * ld];
#pragma unroll
  for (int k = 0; k < JT; ++k) {
    x[k] = x[k] / sD[k][k];
#pragma unroll
    for (int j = k + 1; j < JT; ++j) x[j] = fma(-x[k], sD[j][k], x[j]);
  }
#pragma unroll
  for (int j = 0; j < JT; ++j) L[i + (j0 + j) * ld] = x[j];
}

// Trailing update of step j0 / 64: L_IJ -= P_I P_J^T over the lower tiles of
// rows and columns >= j0 + 64, P = L[:, j0 .. j0 + 63]; diagonal tiles keep
// r >= c only (the strict upper triangle stays zero).
__global__ __launch_bounds__(256) void k_potrf_update(double *__restrict__ L, int64_t ld, int64_t n,
                                                      int64_t j0, const int *__restrict__ flag) {
  if (blockIdx.x > blockIdx.y) return;
  if (*flag != 0) return;
  const int64_t R0 = j0 + JT + (int64_t)blockIdx.y * JT, C0 = j0 + JT + (int64_t)blockIdx.x * JT;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4, wr = wv & 1, wc = wv >> 1;
  d4 acc[2][2];
#pragma unroll
  for (int ci = 0; ci < 2; ++ci)
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
      const int64_t r = R0 + 32 * wr + 16 * ri + lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t c = C0 + 32 * wc + 16 * ci + lk + 4 * j;
        acc[ci][ri][j] = (r < n && c <= r) ? L[r + c * ld] : 0.0;
      }
    }
  const double *P = L + j0 * ld;
  joint_tile<true>(P, ld, n, P, ld, n, R0, C0, JT, acc);
#pragma unroll
  for (int ci = 0; ci < 2; ++ci)
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
      const int64_t r = R0 + 32 * wr + 16 * ri + lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t c = C0 + 32 * wc + 16 * ci + lk + 4 * j;
        if (r < n && c <= r) L[r + c * ld] = acc[ci][ri][j];
      }
    }
}

hipError_t launch_potrf_lower(const double *C, int64_t ldc, int64_t n, double jitter, double *L,
                              int64_t ldl, int *flag, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_potrf_init, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, st,
                     C, ldc, n, jitter, L, ldl);
  for (int64_t j0 = 0; j0 < n; j0 += JT) {
    hipLaunchKernelGGL(k_potrf_diag, dim3(1), dim3(64), 0, st, L, ldl, n, j0, flag);
    const int64_t below = n - j0 - JT;
    if (below <= 0) break;
    const unsigned nt = (unsigned)((below + JT - 1) / JT);
    hipLaunchKernelGGL(k_potrf_solve, dim3(nt), dim3(64), 0, st, L, ldl, n, j0, flag);
    hipLaunchKernelGGL(k_potrf_update, dim3(nt, nt), dim3(256), 0, st, L, ldl, n, j0, flag);
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------- draws
// D (nx x S, ld nx) += m 1^T
__global__ void k_add_col(const double *__restrict__ m, int64_t nx, double *__restrict__ D) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < nx) D[r + (int64_t)blockIdx.y * nx] += m[r];
}

hipError_t launch_draws(const double *L, int64_t ldl, int64_t nx, const double *xi, int64_t S,
                        const double *m, double *D, hipStream_t st) {
  if (nx <= 0 || S <= 0) return hipSuccess;
  const hipError_t e = launch_gemm_nn(nx, S, nx, L, ldl, xi, nx, D, nx, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_add_col, dim3((unsigned)((nx + 255) / 256), (unsigned)S), dim3(256), 0, st, m,
                     nx, D);
  return hipGetLastError();
}

}  // namespace ace
