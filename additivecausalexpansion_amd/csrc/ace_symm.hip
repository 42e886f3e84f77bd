// ace_symm.hip -- products with the resident inverse (device-resident
// prediction, ace_model_apply_inverse).
//
// After a para_update the swept matrix A holds -A^-1 in its lower triangle
// (single GPU: the whole naug x naug array; sharded: the rank's NB-wide
// column blocks, block-cyclic).  The reference multiplies by the explicit
// inverse in pred_cpp (src/pred_cpp.cpp:19, 69: tmp = K_xX * invK_XX); here
// the product is taken straight from the lower storage:
//
//   Out (n x k) = scale * S V,   S = the symmetric n x n matrix whose lower
//   triangle is stored in A, V = an n x k operand given either directly
//   (col-major, ld ldv) or as the transpose of a k x n col-major matrix
//   (VT: V[p][c] = M[c + p * ldv], the K_xX of prediction, so that
//   Out = S K_xX^T = (K_xX S)^T).
//
// Sharded: each rank adds only the entries of S it stores -- S[q][p] for
// p >= q from its own column blocks p and, mirrored, S[q][p] = A[p][q] for
// q < p from its own column blocks q -- so the sum over ranks of the
// partial products is S V.  A 16-wide k-chunk of the product touches only
// one column block, so a chunk the rank does not own is skipped whole
// (block-uniform: the barriers stay uniform), and each rank does 1/G of the
// MFMA work.
//
// 256 threads, 128 (rows) x 64 (columns) output tile, 4 waves of 32 x 64
// (2 x 4 v_mfma_f64_16x16x4_f64 fragments), BK = 16 k-chunks staged
// through LDS with a register prefetch of the next chunk.
#include <algorithm>
#include <cstdlib>

#include "ace_internal.h"

namespace ace {

constexpr int SR = 128, SC = 64, SBK = 16;
constexpr int SLS = SR + 16;  // LDS pitch of the S stage
constexpr int SLV = SC + 16;  // LDS pitch of the V stage

// TRI (single GPU): Out = scale L V with L the STRICTLY lower part of the
// stored matrix (row q, column p < q) -- the k-chunks below the tile's rows
// and the masked diagonal block only, so half of k_symm's MFMA work on
// average and only coalesced column loads (prediction's variance, see
// k_pred_cols_tri).
template <bool VT, bool TRI>
__global__ __launch_bounds__(256) void k_symm(const double *__restrict__ A, int64_t ld, int64_t n,
                                              int G, int rank, const double *__restrict__ V,
                                              int64_t ldv, int64_t k, double scale,
                                              double *__restrict__ out, int64_t ldo) {
  __shared__ __attribute__((aligned(16))) double sS[2][SBK][SLS];
  __shared__ __attribute__((aligned(16))) double sV[2][SBK][SLV];
  const int64_t R0 = (int64_t)blockIdx.y * SR, C0 = (int64_t)blockIdx.x * SC;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const bool rowown = owns_col(R0, G, rank);  // the tile's rows lie in one NB block
  // S staging: lower chunks read 128 consecutive rows of one column (thread:
  // row sm .. sm + 7 of column si), upper chunks 16 consecutive rows of one
  // column of the mirror (thread: column tq of the mirror, rows 8 tj ..)
  const int si = tid >> 4, sm = (tid & 15) * 8;
  const int tq = tid >> 1, tj = (tid & 1) * 8;
  // V staging: 4 doubles per thread
  const int vi = tid >> 4, vc = (tid & 15) * 4;    // VT:  k-row vi, columns vc..vc+3
  const int vci = tid >> 2, vpi = (tid & 3) * 4;   // !VT: column vci, k-rows vpi..vpi+3
  double rs[8], rv[4];
  // chunk class of k-chunk kk: 0 skip, 1 lower (all p < q), 2 upper (all
  // p > q), 3 mixed (the chunk crosses the tile's rows: same NB block)
  auto cls = [&](int64_t kk) -> int {
    if (TRI) return kk + SBK <= R0 ? 1 : (kk < R0 + SR ? 4 : 0);
    if (kk + SBK <= R0) return owns_col(kk, G, rank) ? 1 : 0;
    if (kk >= R0 + SR) return rowown ? 2 : 0;
    return rowown ? 3 : 0;
  };
  auto load = [&](int64_t kk, int c) {
    if (c == 1) {
      const int64_t p = kk + si;
      const double *col = A + lcol(p, G) * ld;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t q = R0 + sm + e;
        rs[e] = (q < n && p < n) ? col[q] : 0.0;
      }
    } else if (c == 2) {
      const int64_t q = R0 + tq;
      const double *col = A + lcol(q, G) * ld;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t p = kk + tj + e;
        rs[e] = (q < n && p < n) ? col[p] : 0.0;
      }
    } else if (c == 4) {  // TRI diagonal block: row q, column p < q only
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t p = kk + si, q = R0 + sm + e;
        rs[e] = (q < n && p < n && q > p) ? A[q + p * ld] : 0.0;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t p = kk + si, q = R0 + sm + e;
        double v = 0.0;
        if (q < n && p < n) v = (q >= p) ? A[q + lcol(p, G) * ld] : A[p + lcol(q, G) * ld];
        rs[e] = v;
      }
    }
    if (!VT) {  // V[p + c ldv]: 4 consecutive p of one column per thread
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t p = kk + vpi + e, c = C0 + vci;
        rv[e] = (p < n && c < k) ? V[p + c * ldv] : 0.0;
      }
    } else {    // V[c + p ldv]: 4 consecutive c of one k-row per thread
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t p = kk + vi, c = C0 + vc + e;
        rv[e] = (p < n && c < k) ? V[c + p * ldv] : 0.0;
      }
    }
  };
  auto store = [&](int buf, int c) {
    if (c == 2) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sS[buf][tj + e][tq] = rs[e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) sS[buf][si][sm + e] = rs[e];
    }
    if (!VT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) sV[buf][vpi + e][vci] = rv[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) sV[buf][vi][vc + e] = rv[e];
    }
  };
  d4 acc[4][2];
#pragma unroll
  for (int ci = 0; ci < 4; ++ci)
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) acc[ci][ri] = d4{0.0, 0.0, 0.0, 0.0};
  // the owned chunks, in order; cur / nxt chunk and their classes
  const int64_t kend = TRI ? (n < R0 + SR ? n : R0 + SR) : n;
  int64_t kk = 0;
  int c = 0;
  while (kk < kend && (c = cls(kk)) == 0) kk += SBK;
  if (kk < kend) {
    load(kk, c);
    store(0, c);
  }
  __syncthreads();
  int buf = 0;
  while (kk < kend) {
    int64_t kn = kk + SBK;
    int cn = 0;
    while (kn < kend && (cn = cls(kn)) == 0) kn += SBK;
    if (kn < kend) load(kn, cn);
#pragma unroll
    for (int q4 = 0; q4 < SBK / 4; ++q4) {
      double a[4], b[2];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) a[ci] = sV[buf][4 * q4 + lk][16 * ci + lr];
#pragma unroll
      for (int ri = 0; ri < 2; ++ri) b[ri] = sS[buf][4 * q4 + lk][32 * w + 16 * ri + lr];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci)
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
          acc[ci][ri] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ci], b[ri], acc[ci][ri], 0, 0, 0);
    }
    if (kn < kend) store(buf ^ 1, cn);
    __syncthreads();
    buf ^= 1;
    kk = kn;
    c = cn;
  }
#pragma unroll
  for (int ci = 0; ci < 4; ++ci)
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
      const int64_t q = R0 + 32 * w + 16 * ri + lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t cc = C0 + 16 * ci + lk + 4 * j;
        if (q < n && cc < k) out[q + cc * ldo] = scale * acc[ci][ri][j];
      }
    }
}

hipError_t launch_symm(const double *A, int64_t ld, int64_t n, int G, int rank, const double *V,
                       int64_t ldv, bool vt, int64_t k, double scale, double *out, int64_t ldo,
                       hipStream_t st) {
  if (n <= 0 || k <= 0) return hipSuccess;
  const dim3 grid((unsigned)((k + SC - 1) / SC), (unsigned)((n + SR - 1) / SR));
  if (vt)
    hipLaunchKernelGGL((k_symm<true, false>), grid, dim3(256), 0, st, A, ld, n, G, rank, V, ldv, k,
                       scale, out, ldo);
  else
    hipLaunchKernelGGL((k_symm<false, false>), grid, dim3(256), 0, st, A, ld, n, G, rank, V, ldv, k,
                       scale, out, ldo);
  return hipGetLastError();
}

// The triangular product on the sweep update's tile machinery (ACE_TRMM_BIG,
// default): 512 threads, 128 x 128 output tiles (8 waves of 64 x 32), BK =
// 16 chunks through double-buffered LDS with a register prefetch.  Row tiles
// are taken bottom-up (blockIdx.y = 0 is the last row tile, the longest k
// range), so the cheap tiles form the launch's tail.
constexpr int TT = 128, TBK = 16, TLD = TT + 16;
__global__ __launch_bounds__(512, 2) void k_trmm_lower(const double *__restrict__ A, int64_t ld,
                                                       int64_t n, const double *__restrict__ V,
                                                       int64_t ldv, int64_t k, double scale,
                                                       double *__restrict__ out, int64_t ldo) {
  __shared__ __attribute__((aligned(16))) double sS[2][TBK][TLD];  // [p][q - R0]
  __shared__ __attribute__((aligned(16))) double sV[2][TBK][TLD];  // [p][c - C0]
  const int64_t nrt = (n + TT - 1) / TT;
  const int64_t R0 = (nrt - 1 - (int64_t)blockIdx.y) * TT, C0 = (int64_t)blockIdx.x * TT;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int wr = wv & 1, wc = wv >> 1;  // rows 64 wr.., columns 32 wc..
  const int sp = tid >> 5, sm = (tid & 31) * 4;  // staging: chunk row sp, 4 consecutive entries
  const int64_t kend = n < R0 + TT ? n : R0 + TT;
  double rs[4], rv[4];
  auto load = [&](int64_t kk) {
    const int64_t p = kk + sp;
    const bool diag = kk + TBK > R0;  // the chunk reaches the tile's rows: keep p < q only
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t q = R0 + sm + e, c = C0 + sm + e;
      rs[e] = (p < n && q < n && (!diag || q > p)) ? A[q + p * ld] : 0.0;
      rv[e] = (p < n && c < k) ? V[c + p * ldv] : 0.0;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sS[buf][sp][sm + e] = rs[e];
      sV[buf][sp][sm + e] = rv[e];
    }
  };
  d4 acc[2][4];
#pragma unroll
  for (int ci = 0; ci < 2; ++ci)
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) acc[ci][ri] = d4{0.0, 0.0, 0.0, 0.0};
  if (kend > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  int buf = 0;
  for (int64_t kk = 0; kk < kend; kk += TBK) {
    const bool more = kk + TBK < kend;
    if (more) load(kk + TBK);
#pragma unroll
    for (int q4 = 0; q4 < TBK / 4; ++q4) {
      double a[2], b[4];
#pragma unroll
      for (int ci = 0; ci < 2; ++ci) a[ci] = sV[buf][4 * q4 + lk][32 * wc + 16 * ci + lr];
#pragma unroll
      for (int ri = 0; ri < 4; ++ri) b[ri] = sS[buf][4 * q4 + lk][64 * wr + 16 * ri + lr];
#pragma unroll
      for (int ci = 0; ci < 2; ++ci)
#pragma unroll
        for (int ri = 0; ri < 4; ++ri)
          acc[ci][ri] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ci], b[ri], acc[ci][ri], 0, 0, 0);
    }
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
#pragma unroll
  for (int ci = 0; ci < 2; ++ci)
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) {
      const int64_t q = R0 + 64 * wr + 16 * ri + lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t c = C0 + 32 * wc + 16 * ci + lk + 4 * j;
        if (q < n && c < k) out[q + c * ldo] = scale * acc[ci][ri][j];
      }
    }
}

static bool trmm_big() {
  static const bool v = env_int("ACE_TRMM_BIG", 1) != 0;
  return v;
}

hipError_t launch_trmm_lower(const double *A, int64_t ld, int64_t n, const double *V, int64_t ldv,
                             int64_t k, double scale, double *out, int64_t ldo, hipStream_t st) {
  if (n <= 0 || k <= 0) return hipSuccess;
  if (trmm_big()) {
    const dim3 grid((unsigned)((k + TT - 1) / TT), (unsigned)((n + TT - 1) / TT));
    hipLaunchKernelGGL(k_trmm_lower, grid, dim3(512), 0, st, A, ld, n, V, ldv, k, scale, out, ldo);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)((k + SC - 1) / SC), (unsigned)((n + SR - 1) / SR));
  hipLaunchKernelGGL((k_symm<true, true>), grid, dim3(256), 0, st, A, ld, n, 1, 0, V, ldv, k, scale,
                     out, ldo);
  return hipGetLastError();
}

// ---------------------------------------------------------------- prediction sums
// For each test point c < nx (T' = S K_xX^T, n x nx, ld ldt; K = K_xX,
// nx x n, ld ldk):  a[c] = sum_q T'[q][c] w[q]   (tmp (y - mu), src/pred_cpp.cpp:20)
//                   d[c] = sum_q T'[q][c] K[c][q] (diag(tmp K_xX^T), :22)
// One workgroup per test point; T' column reads are contiguous.
__global__ __launch_bounds__(256) void k_pred_cols(const double *__restrict__ T, int64_t ldt,
                                                   const double *__restrict__ K, int64_t ldk,
                                                   int64_t n, const double *__restrict__ w,
                                                   double *__restrict__ a, double *__restrict__ d) {
  __shared__ double sh[2][4];
  const int64_t c = blockIdx.x;
  const double *tc = T + c * ldt;
  double sa = 0.0, sd = 0.0;
  for (int64_t q = threadIdx.x; q < n; q += 256) {
    const double t = tc[q];
    sa = fma(t, w[q], sa);
    sd = fma(t, K[c + q * ldk], sd);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sa += __shfl_xor(sa, o, 64);
    sd += __shfl_xor(sd, o, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    sh[0][wv] = sa;
    sh[1][wv] = sd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a[c] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
    d[c] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
  }
}

hipError_t launch_pred_cols(const double *T, int64_t ldt, const double *K, int64_t ldk, int64_t n,
                            int64_t nx, const double *w, double *a, double *d, hipStream_t st) {
  if (nx <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pred_cols, dim3((unsigned)nx), dim3(256), 0, st, T, ldt, K, ldk, n, w, a,
                     d);
  return hipGetLastError();
}

// Triangular form (single GPU): with S = L + L^T + D (L strictly lower),
// Y = L K^T (n x nx, ld ldt) from launch_trmm_lower and s = S w:
//   a[c] = sum_q K[c][q] s[q]
//   d[c] = (K S K^T)[c][c] = sum_q K[c][q] (2 Y[q][c] + D[q] K[c][q])
__global__ __launch_bounds__(256) void k_pred_cols_tri(const double *__restrict__ Y, int64_t ldt,
                                                       const double *__restrict__ K, int64_t ldk,
                                                       int64_t n, const double *__restrict__ sv,
                                                       const double *__restrict__ D,
                                                       double *__restrict__ a,
                                                       double *__restrict__ d) {
  __shared__ double sh[2][4];
  const int64_t c = blockIdx.x;
  const double *yc = Y + c * ldt;
  double sa = 0.0, sd = 0.0;
  for (int64_t q = threadIdx.x; q < n; q += 256) {
    const double kq = K[c + q * ldk];
    sa = fma(kq, sv[q], sa);
    sd = fma(kq, fma(D[q], kq, 2.0 * yc[q]), sd);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sa += __shfl_xor(sa, o, 64);
    sd += __shfl_xor(sd, o, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    sh[0][wv] = sa;
    sh[1][wv] = sd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a[c] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
    d[c] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
  }
}

hipError_t launch_pred_cols_tri(const double *Y, int64_t ldt, const double *K, int64_t ldk,
                                int64_t n, int64_t nx, const double *sv, const double *D, double *a,
                                double *d, hipStream_t st) {
  if (nx <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pred_cols_tri, dim3((unsigned)nx), dim3(256), 0, st, Y, ldt, K, ldk, n, sv,
                     D, a, d);
  return hipGetLastError();
}

// ---------------------------------------------------------------- coefficient Gram
// Per test point c of a chunk of ncx (the coefficient posterior,
// ace_predict.cpp): with Kc the (ncx B) x n per-slice cross kernels (row
// c + ncx b, ld ldk) and W the n x (ncx B) product with the resident inverse
// (column c + ncx b, ld ldw),
//   M_c[b][b'] = sum_q Kc[c,b][q] Wt[q][c,b'],  m_c[b] = sum_q (..)[q] v[q]
// TRI:  Wt = Y + 1/2 D o Kc^T (Y = L Kc^T, L strictly lower), v = S w summed
//       against Kc; then P_c = M_c + M_c^T = Kc_c S Kc_c^T -- k_pred_cols_tri's
//       identity for b != b'
// full: Wt = T' = S Kc^T, v = w summed against T'; P_c = (M_c + M_c^T) / 2
// A batched tall-skinny GEMM (M = N = B, K = n) on v_mfma_f64_16x16x4_f64:
// B padded to 16 NBK with zeros, NBK^2 accumulator blocks per point.  A
// workgroup takes GC = 16 adjacent test points (wave w the points 4 w ..
// 4 w + 3) and the training points [js qs, (js + 1) qs); each GQ = 8 step
// stages Kc as runs of 16 adjacent c and W as runs of 8 adjacent q in LDS,
// so no load strides by a leading dimension (k_pred_cols reads K[c + q ld]).
// qs and the number of ranges depend on n alone (coef_gram_split), the
// ranges' partials are added in ascending js by k_coef_finish: no atomics,
// and a point's bits do not depend on the chunk it arrives in.
// Memory-bound by construction: Kc and W are read once, 2 ncx B n doubles,
// for 2 ncx B^2 n flops (DESIGN §13 has the measured rate).
// ----------------------------------------------------------------
constexpr int GC = 16, GQ = 8, GKP = GQ * GC + 1, GWP = GQ + 1;

template <bool TRI, int NBK>
__global__ __launch_bounds__(256) void k_coef_gram(const double *__restrict__ Kc, int64_t ldk,
                                                   const double *__restrict__ W, int64_t ldw,
                                                   int64_t n, int64_t ncx, int B, int64_t qs,
                                                   const double *__restrict__ vec,
                                                   const double *__restrict__ D,
                                                   double *__restrict__ part, int64_t pstride) {
  extern __shared__ __attribute__((aligned(16))) double glds[];
  constexpr int BP = 16 * NBK;
  double *const sK = glds;                 // [b][q][c]: b GKP + q GC + c
  double *const sW = sK + BP * GKP;        // [c][b][q]: (c BP + b) GWP + q
  double *const sV = sW + GC * BP * GWP;   // v[q]
  double *const sD = sV + GQ;              // D[q] / 2
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.x * GC, js = blockIdx.y;
  const int64_t q0 = js * qs, qend = q0 + qs < n ? q0 + qs : n;
  const int mc = tid & 15, mb = tid >> 4;  // the mean's (point, slice mb + 16 bi)
  d4 acc[4][NBK][NBK];
  double macc[NBK];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt)
#pragma unroll
    for (int bi = 0; bi < NBK; ++bi)
#pragma unroll
      for (int bj = 0; bj < NBK; ++bj) acc[pt][bi][bj] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int bi = 0; bi < NBK; ++bi) macc[bi] = 0.0;
  for (int64_t qq = q0; qq < qend; qq += GQ) {
    for (int e = tid; e < BP * GQ * GC; e += 256) {
      const int c = e & (GC - 1), q = (e >> 4) & (GQ - 1), b = e >> 7;
      const bool ok = b < B && c0 + c < ncx && qq + q < qend;
      sK[b * GKP + q * GC + c] = ok ? Kc[(c0 + c) + ncx * b + (qq + q) * ldk] : 0.0;
    }
    for (int e = tid; e < GC * BP * GQ; e += 256) {
      const int q = e & (GQ - 1), cb = e >> 3, b = cb % BP, c = cb / BP;
      const bool ok = b < B && c0 + c < ncx && qq + q < qend;
      sW[cb * GWP + q] = ok ? W[(qq + q) + ((c0 + c) + ncx * b) * ldw] : 0.0;
    }
    if (tid < GQ) {
      const bool ok = qq + tid < qend;
      sV[tid] = ok ? vec[qq + tid] : 0.0;
      sD[tid] = (TRI && ok) ? 0.5 * D[qq + tid] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int bi = 0; bi < NBK; ++bi) {
      const int b = mb + 16 * bi;
#pragma unroll
      for (int q = 0; q < GQ; ++q) {
        const double x = TRI ? sK[b * GKP + q * GC + mc] : sW[(mc * BP + b) * GWP + q];
        macc[bi] = fma(x, sV[q], macc[bi]);
      }
    }
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int c = 4 * w + pt;
#pragma unroll
      for (int ks = 0; ks < GQ / 4; ++ks) {
        const int q = 4 * ks + lk;
        double a[NBK], bop[NBK];
#pragma unroll
        for (int bi = 0; bi < NBK; ++bi) {
          a[bi] = sK[(16 * bi + lr) * GKP + q * GC + c];
          const double y = sW[(c * BP + 16 * bi + lr) * GWP + q];
          bop[bi] = TRI ? fma(sD[q], a[bi], y) : y;
        }
#pragma unroll
        for (int bi = 0; bi < NBK; ++bi)
#pragma unroll
          for (int bj = 0; bj < NBK; ++bj)
            acc[pt][bi][bj] =
                __builtin_amdgcn_mfma_f64_16x16x4f64(a[bi], bop[bj], acc[pt][bi][bj], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // D register v of lane (lr, lk): M[16 bi + lk + 4 v][16 bj + lr]
  double *const pj = part + js * pstride;
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int64_t c = c0 + 4 * w + pt;
    if (c >= ncx) continue;
#pragma unroll
    for (int bi = 0; bi < NBK; ++bi)
#pragma unroll
      for (int bj = 0; bj < NBK; ++bj)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int b = 16 * bi + lk + 4 * v, b2 = 16 * bj + lr;
          if (b < B && b2 < B) pj[c + ncx * (b + (int64_t)B * b2)] = acc[pt][bi][bj][v];
        }
  }
  if (c0 + mc < ncx) {
#pragma unroll
    for (int bi = 0; bi < NBK; ++bi) {
      const int b = mb + 16 * bi;
      if (b < B) pj[ncx * B * B + (c0 + mc) + ncx * b] = macc[bi];
    }
  }
}

// res = the ranges' partials in ascending js, symmetrised: res[c + ncx (b +
// B b')] = M[b][b'] + M[b'][b] (TRI) or half of it, the same bits for (b, b')
// and (b', b); res[ncx B B + c + ncx b] = m_c[b]
__global__ __launch_bounds__(256) void k_coef_finish(const double *__restrict__ part, int nparts,
                                                     int64_t pstride, int64_t ncx, int B, int tri,
                                                     double *__restrict__ res) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ncov = ncx * B * B;
  if (e >= ncov + ncx * B) return;
  if (e >= ncov) {
    double s = 0.0;
    for (int j = 0; j < nparts; ++j) s += part[j * pstride + e];
    res[e] = s;
    return;
  }
  const int64_t c = e % ncx, bb = e / ncx;
  const int b = (int)(bb % B), b2 = (int)(bb / B);
  const int64_t et = c + ncx * (b2 + (int64_t)B * b);
  double s1 = 0.0, s2 = 0.0;
  for (int j = 0; j < nparts; ++j) {
    s1 += part[j * pstride + e];
    s2 += part[j * pstride + et];
  }
  res[e] = tri ? s1 + s2 : 0.5 * (s1 + s2);
}

// training points per range and the number of ranges: from n alone
int64_t coef_gram_split(int64_t n, int *nparts) {
  const int64_t np = std::min<int64_t>(64, (n + 255) / 256);
  const int64_t qs = ((n + np - 1) / np + GQ - 1) / GQ * GQ;
  *nparts = (int)((n + qs - 1) / qs);
  return qs;
}

int64_t coef_gram_work(int64_t n, int64_t ncx, int B) {
  int np = 0;
  (void)coef_gram_split(n, &np);
  return (int64_t)np * ncx * B * (B + 1);
}

template <bool TRI, int NBK>
static hipError_t coef_gram_launch(const double *Kc, int64_t ldk, const double *W, int64_t ldw,
                                   int64_t n, int64_t ncx, int B, const double *vec,
                                   const double *D, double *part, hipStream_t st) {
  constexpr int BP = 16 * NBK;
  const size_t lds = (size_t)(BP * GKP + GC * BP * GWP + 2 * GQ) * sizeof(double);
  int np = 0;
  const int64_t qs = coef_gram_split(n, &np);
  const dim3 grid((unsigned)((ncx + GC - 1) / GC), (unsigned)np);
  return launch_lds(k_coef_gram<TRI, NBK>, grid, dim3(256), lds, st, Kc, ldk, W, ldw, n, ncx, B, qs,
                    vec, D, part, ncx * B * (B + 1));
}

hipError_t launch_coef_gram(bool tri, const double *Kc, int64_t ldk, const double *W, int64_t ldw,
                            int64_t n, int64_t ncx, int B, const double *vec, const double *D,
                            double *part, double *res, hipStream_t st) {
  if (ncx <= 0 || n <= 0) return hipSuccess;
  if (B < 1 || B > 32) return hipErrorInvalidValue;
  hipError_t e;
  if (B <= 16)
    e = tri ? coef_gram_launch<true, 1>(Kc, ldk, W, ldw, n, ncx, B, vec, D, part, st)
            : coef_gram_launch<false, 1>(Kc, ldk, W, ldw, n, ncx, B, vec, D, part, st);
  else
    e = tri ? coef_gram_launch<true, 2>(Kc, ldk, W, ldw, n, ncx, B, vec, D, part, st)
            : coef_gram_launch<false, 2>(Kc, ldk, W, ldw, n, ncx, B, vec, D, part, st);
  if (e != hipSuccess) return e;
  int np = 0;
  (void)coef_gram_split(n, &np);
  const int64_t tot = ncx * B * (B + 1);
  hipLaunchKernelGGL(k_coef_finish, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, part, np,
                     tot, ncx, B, tri ? 1 : 0, res);
  return hipGetLastError();
}

// D[q] = scale A[q][q] (the diagonal of the stored matrix)
__global__ void k_diag_scaled(const double *__restrict__ A, int64_t ld, int64_t n, double scale,
                              double *__restrict__ D) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) D[q] = scale * A[q + q * ld];
}

hipError_t launch_diag_scaled(const double *A, int64_t ld, int64_t n, double scale, double *D,
                              hipStream_t st) {
  hipLaunchKernelGGL(k_diag_scaled, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, ld, n,
                     scale, D);
  return hipGetLastError();
}

// w = y - mu (the reference's y_X - mu, src/pred_cpp.cpp:20, 70)
__global__ void k_center(const double *__restrict__ y, int64_t n, double mu,
                         double *__restrict__ w) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) w[j] = y[j] - mu;
}

hipError_t launch_center(const double *y, int64_t n, double mu, double *w, hipStream_t st) {
  hipLaunchKernelGGL(k_center, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, y, n, mu, w);
  return hipGetLastError();
}

}  // namespace ace
