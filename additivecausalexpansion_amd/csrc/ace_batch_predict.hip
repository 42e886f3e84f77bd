// ace_batch_predict.hip -- posterior prediction for every model of a batch in
// one launch: one workgroup runs one model's pred_cpp / pred_marginal_cpp
// (DESIGN §16).
//
//   k_batch_predict<KIND, PM> : theta tables, alpha = A^-1 (y - mu) from the
//                               resident inverse, then per tile of 16 BPT test
//                               points the cross rows k_i = K_xX[i, :] in LDS,
//                               a_i = k_i alpha, diag(K_xx), and the quadratic
//                               form q_i = k_i A^-1 k_i^T on
//                               v_mfma_f64_16x16x4_f64; for ATE/ATT/ATU the
//                               posterior covariance of the two group sums.
//
// The rules of k_batch_eval hold: workgroup j touches model j's slots, scratch
// matrix and test points only; no grid barrier, no flag polling, no atomics;
// every loop is bounded by n_j, nx_j, p and B; every reduction runs in a fixed
// order (lanes by xor-shuffle, waves in a fixed tree, tiles in index order), so
// a model's outputs depend neither on M nor on its position nor on nmax.
//
// Of the scratch matrix only the n x n part is read (-A^-1, lower triangle
// and its mirror): an inverse installed from the host behaves like a resident
// one.  The host composes map / ci / var and the 12 averages from a, kd, q and
// gcov with the tails the single-model path uses (ace_common.h).
//
// The arithmetic is that of ace_formulas.h (kval in its cross and symmetric
// forms, tab_weight for the kernel-indexed weights), and the wave and
// workgroup sums are its wsum64 / wave_parts / block_sum; this file keeps the
// LDS layout and the order of every sum.
#include "../../include/ace_hip.h"
#include "ace_batch.h"
#include "ace_internal.h"

namespace ace {

namespace {

// LDS map (doubles): scal[16] | wk[B PM] | lam[B] e^theta0 | alpha[nmax] |
// u[2 nmax] (y - mu first, then the group sums of the cross rows) |
// red[NW 16 BPT] | the BPT test tiles, 16 rows of `pitch` each.
constexpr int PL_HEAD = 16;
constexpr int TP = BT * BPT;  // test points per pass

}  // namespace

size_t batch_predict_lds_bytes(int nmax, int B, int PM) {
  const size_t d = (size_t)PL_HEAD + (size_t)B * PM + B + 1 + 3 * (size_t)nmax +
                   (size_t)(batch_threads(PM) / 64) * TP + (size_t)TP * batch_predict_pitch(nmax);
  return d * sizeof(double);
}

template <int KIND, int PM>
__global__ __launch_bounds__(batch_threads(PM)) void k_batch_predict(BatchPredView a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int NTHR = batch_threads(PM), NW = NTHR / 64;
  const int j = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = a.n[j], B = a.B, p = a.p, ZS = a.ZS, nmax = a.nmax;
  const int npad = (n + BT - 1) / BT * BT;
  const int64_t ld = a.ld;
  const int pitch = batch_predict_pitch(nmax);
  const int64_t o0 = a.off[j];
  const int nx = (int)(a.off[j + 1] - o0);
  const double *__restrict__ X = a.X + (int64_t)j * nmax * PM;
  const double *__restrict__ Z = a.Z + (int64_t)j * nmax * ZS;
  const double *__restrict__ LZ = a.LZ + (int64_t)j * nmax * ZS;
  const double *__restrict__ y = a.y + (int64_t)j * nmax;
  const double *__restrict__ th = a.theta + (int64_t)j * a.ldt;
  const double *__restrict__ A = a.A + (int64_t)j * ld * ld;
  const double *__restrict__ X2 = a.X2 + o0 * PM;
  const double *__restrict__ Z2 = a.Z2 + o0 * ZS;
  const double *__restrict__ LZ2 = a.LZ2 + o0 * ZS;
  const double *__restrict__ zx = a.ate ? a.zx + o0 : nullptr;
  double *oa = a.a + o0, *okd = a.kd + o0, *oq = a.q + o0;

  // a model whose last para_update met a non-positive pivot: NaN, nothing else
  if (a.flag[j] != 0.0) {
    const double kNaN = __builtin_nan("");
    for (int i = tid; i < nx; i += NTHR) {
      oa[i] = kNaN;
      okd[i] = kNaN;
      oq[i] = kNaN;
    }
    if (a.ate && tid < 3) a.gcov[3 * (int64_t)j + tid] = kNaN;
    return;
  }

  const int nk = B * PM;
  double *sWk = lds + PL_HEAD, *sLam = sWk + nk;  // e^theta0 at sLam[B]
  double *sAl = sLam + B + 1, *sU = sAl + nmax;
  double *sRed = sU + 2 * nmax, *sK = sRed + NW * TP;
  // the slices summed: all of them, or the marginal ones (src/pred_cpp.cpp:55-67)
  const int b0 = a.marginal && B > 1 ? 1 : 0;
  const int b1 = a.marginal ? (B > 1 ? B : 1) : B;

  // ---- theta tables (the kernel weights of make_tab; no gradient part) ----------
  for (int e = tid; e < nk + B + 1; e += NTHR) {
    double v = 0.0;
    if (e < nk) {
      const int b = e / PM, i = e - b * PM;
      if (i < p) v = tab_weight(th, B, b, i, false);
    } else if (e < nk + B) {
      v = th[2 + (e - nk)];
    } else {
      v = exp(th[0]);
    }
    sWk[e] = v;
  }
  const double mu = th[1];
  for (int i = tid; i < n; i += NTHR) sU[i] = y[i] - mu;
  __syncthreads();

  // the resident inverse's element (r, c), r, c < n
  auto ainv = [&](int r, int c) -> double {
    return -(r >= c ? A[r + (int64_t)c * ld] : A[c + (int64_t)r * ld]);
  };

  // ---- alpha = A^-1 (y - mu): one row per thread, columns in index order -------
  for (int i = tid; i < n; i += NTHR) {
    double s = 0.0;
    for (int c = 0; c < n; ++c) s = fma(ainv(i, c), sU[c], s);
    sAl[i] = s;
  }
  __syncthreads();
  for (int i = tid; i < 2 * nmax; i += NTHR) sU[i] = 0.0;
  __syncthreads();

  const int lr = lane & 15, lk = lane >> 4;
  const int nch = (npad + 63) / 64;  // 64-column chunks of a cross row

  for (int i0 = 0; i0 < nx; i0 += TP) {
    const int nt = min(TP, nx - i0);
    // ---- cross rows: a wave takes (64 training columns, one test point) -------
    for (int item = wv; item < nch * TP; item += NW) {
      const int ch = item % nch, pt = item / nch;
      const int c = ch * 64 + lane;
      if (c >= npad) continue;
      double kf = 0.0;
      if (c < n && pt < nt) {
        const int64_t r = i0 + pt;
        double d2[PM];
#pragma unroll
        for (int i = 0; i < PM; ++i) {
          const double d = X2[r * PM + i] - X[(int64_t)c * PM + i];
          d2[i] = d * d;
        }
        for (int b = b0; b < b1; ++b) {
          double r2 = 0.0;
#pragma unroll
          for (int i = 0; i < PM; ++i) r2 = fma(d2[i], sWk[b * PM + i], r2);
          double zt = 0.0, zc = 0.0, lzt = 0.0, lzc = 0.0;
          if (b > 0) {
            zt = Z2[r * ZS + b - 1];
            zc = Z[(int64_t)c * ZS + b - 1];
            if (KIND == 0) {
              lzt = LZ2[r * ZS + b - 1];
              lzc = LZ[(int64_t)c * ZS + b - 1];
            }
          }
          // cross form: "lo" is the test point (the X1 / Z1 side of
          // kernmat_*_cpp(X2, X, Z2, Z))
          kf += kval<KIND, true>(b, r2, sLam[b], zt, zc, lzt, lzc);
        }
      }
      sK[pt * pitch + c] = kf;  // (the identity padding's columns: zero)
    }
    __syncthreads();

    // ---- a_i = k_i alpha and diag(K_xx): one wave per test point ---------------
    for (int pt = wv; pt < nt; pt += NW) {
      double s = 0.0;
      for (int c = lane; c < n; c += 64) s = fma(sK[pt * pitch + c], sAl[c], s);
      s = wsum64(s);
      if (lane == 0) {
        const int64_t r = i0 + pt;
        double kd = 0.0;
        for (int b = b0; b < b1; ++b) {
          double z = 0.0, lz = 0.0;
          if (b > 0) {
            z = Z2[r * ZS + b - 1];
            if (KIND == 0) lz = LZ2[r * ZS + b - 1];
          }
          kd += kval<KIND, false>(b, 0.0, sLam[b], z, z, lz, lz);
        }
        oa[r] = s;
        okd[r] = kd;
      }
    }
    // ---- u_g += Km_xX^T e_g, test points in index order ------------------------
    if (a.ate) {
      for (int c = tid; c < n; c += NTHR) {
        double ut = sU[c], uu = sU[nmax + c];
        for (int pt = 0; pt < nt; ++pt) {
          const double k = sK[pt * pitch + c];
          if (zx[i0 + pt] != 0.0) ut += k;
          else uu += k;
        }
        sU[c] = ut;
        sU[nmax + c] = uu;
      }
    }

    // ---- W = K_tile A^-1 on the matrix cores, q_i = sum_c W[i, c] k_i[c] -------
    // A operand: the tile (rows = test points, from LDS); B operand: A^-1
    // (k = row, column tile J); a lane's results: rows lk + 4 q, column lr.
    double qacc[BPT][4];
#pragma unroll
    for (int u = 0; u < BPT; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) qacc[u][q] = 0.0;
    for (int J = wv; J < npad / BT; J += NW) {
      d4 acc[BPT];
#pragma unroll
      for (int u = 0; u < BPT; ++u) acc[u] = d4{0.0, 0.0, 0.0, 0.0};
      const int c = J * BT + lr;
      for (int k0 = 0; k0 < npad; k0 += 4) {
        const int r = k0 + lk;
        const double bv = (r < n && c < n) ? ainv(r, c) : 0.0;
        const double a0 = sK[lr * pitch + r];
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bv, acc[0], 0, 0, 0);
        if (nt > BT) {
          const double a1 = sK[(BT + lr) * pitch + r];
          acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bv, acc[1], 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < BPT; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          qacc[u][q] = fma(acc[u][q], sK[(u * BT + lk + 4 * q) * pitch + c], qacc[u][q]);
    }
#pragma unroll
    for (int u = 0; u < BPT; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // over the 16 lanes of a row (written here, not as a shared template:
        // this form keeps the kernel's machine code as it was)
        double v = qacc[u][q];
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if (lr == 0) sRed[wv * TP + u * BT + lk + 4 * q] = v;
      }
    __syncthreads();
    if (tid < nt) oq[i0 + tid] = wave_parts<NW>(sRed + tid, TP);
    __syncthreads();
  }
  if (!a.ate) return;

  // ---- (a) E^T Km_xx E over the lower test pairs: lane = row r, columns c <= r --
  double tt = 0.0, tu = 0.0, uu = 0.0;
  for (int h = 0; (int64_t)NTHR * h < nx; ++h) {
    const int wbase = NTHR * h + 64 * wv;
    const int r = wbase + lane;
    const bool rin = r < nx;
    double xr[PM];
#pragma unroll
    for (int i = 0; i < PM; ++i) xr[i] = rin ? X2[(int64_t)r * PM + i] : 0.0;
    const bool gr = rin && zx[r] != 0.0;
    const int cend = wbase < nx ? min(wbase + 63, nx - 1) : -1;
    for (int c = 0; c <= cend; ++c) {
      if (!rin || c > r) continue;
      double kf = 0.0;
      for (int b = b0; b < b1; ++b) {
        double r2 = 0.0;
#pragma unroll
        for (int i = 0; i < PM; ++i) {
          const double d = xr[i] - X2[(int64_t)c * PM + i];
          r2 = fma(d * d, sWk[b * PM + i], r2);
        }
        double zr = 0.0, zc = 0.0, lzr = 0.0, lzc = 0.0;
        if (b > 0) {
          zr = Z2[(int64_t)r * ZS + b - 1];
          zc = Z2[(int64_t)c * ZS + b - 1];
          if (KIND == 0) {
            lzr = LZ2[(int64_t)r * ZS + b - 1];
            lzc = LZ2[(int64_t)c * ZS + b - 1];
          }
        }
        kf += kval<KIND, false>(b, r2, sLam[b], zc, zr, lzc, lzr);
      }
      const bool gc = zx[c] != 0.0;
      if (gr != gc) tu += kf;  // once: the host counts the pair's mirror
      else if (gr) tt += (c == r) ? kf : 2.0 * kf;
      else uu += (c == r) ? kf : 2.0 * kf;
    }
  }
  tt = block_sum<NW>(tt, sRed);
  tu = block_sum<NW>(tu, sRed);
  uu = block_sum<NW>(uu, sRed);

  // ---- (c) u_g^T A^-1 u_h: one row per thread, columns in index order ---------
  double dtt = 0.0, dtu = 0.0, duu = 0.0;
  for (int i = tid; i < n; i += NTHR) {
    double st = 0.0, su = 0.0;
    for (int c = 0; c < n; ++c) {
      const double av = ainv(i, c);
      st = fma(av, sU[c], st);
      su = fma(av, sU[nmax + c], su);
    }
    dtt = fma(sU[i], st, dtt);
    dtu = fma(sU[i], su, dtu);
    duu = fma(sU[nmax + i], su, duu);
  }
  dtt = block_sum<NW>(dtt, sRed);
  dtu = block_sum<NW>(dtu, sRed);
  duu = block_sum<NW>(duu, sRed);
  if (tid == 0) {
    double *g = a.gcov + 3 * (int64_t)j;
    g[0] = tt - dtt;
    g[1] = tu - dtu;
    g[2] = uu - duu;
  }
}

template <int KIND, int PM>
static hipError_t predict_pm(const BatchPredView &v, hipStream_t st) {
  return launch_lds(k_batch_predict<KIND, PM>, dim3((unsigned)v.M), dim3(batch_threads(PM)),
                    batch_predict_lds_bytes(v.nmax, v.B, PM), st, v);
}

hipError_t launch_batch_predict(int kind, const BatchPredView &v, hipStream_t st) {
  if (v.M <= 0) return hipSuccess;
  if (v.nmax > BATCH_NMAX || batch_predict_lds_bytes(v.nmax, v.B, v.PM) > LDS_MAX)
    return hipErrorInvalidValue;
  switch (v.PM) {
#define ACE_CASE(Q) \
  case Q:           \
    return kind == 0 ? predict_pm<0, Q>(v, st) : predict_pm<1, Q>(v, st);
    ACE_CASE(4) ACE_CASE(8) ACE_CASE(16) ACE_CASE(32) ACE_CASE(64)
#undef ACE_CASE
    default: return hipErrorInvalidValue;
  }
}

}  // namespace ace
