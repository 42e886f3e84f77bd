// ace_pairs.hip -- the all-VALU pair kernels of the ABI's cube modes, written
// for gfx950, and the dispatch of every pair-kernel entry point.
//
//  * k_assembly : kernel matrix K = sum_b K_b (a1-a4 of SURVEY §8a), symmetric
//                 (mode 1) or cross (mode 2), with the n x n x B cube of the
//                 K_b when `elements` is asked for; mode 1 also without a cube
//                 (prediction's K_xx).
//  * k_grad     : gradient traces -0.5 tr(T dK/dtheta) for every
//                 hyperparameter (a7/a8) with K_b read from a given cube, up
//                 to PM = 48.
//
// Everything else -- the fused model's assembly and gradient, the cube-less
// cross kernels, the grouped sums, the gradient above PM = 48 -- runs on the
// MFMA expansion (ace_pairs_mm.hip), whose LDS staging fits every supported
// shape (the static proof there).  tests/test_regimes_gpu.py
// test_valu_pair_arithmetic_within_bound holds these kernels to the K bound.
//
// Both kernels walk 64x64 pair tiles with 256 threads: lane = row r, the
// wave id picks 16 columns c = J*64 + wave + 4m, so every column-side
// operand (x_c, z_c, the per-b weight rows) is wave-uniform and is fetched
// with scalar loads, and every store to the column-major matrix is one
// contiguous 512-B segment per wave.  fp64 VALU bound.
#include <algorithm>

#include "ace_internal.h"

namespace ace {

// ---------------------------------------------------------------------------
// Assembly.  MODE 1: symmetric full output (+cube), MODE 2: cross (+cube).
// npad, sig, tiles and G are not read, and the column test below repeats the
// loop's own: both are what keeps these kernels' machine code as it was while
// the fused mode left (an argument less moves the others, a test less changes
// the schedule); dropping them is a change of its own.
// ---------------------------------------------------------------------------
template <int PM, int KIND, int MODE>
__global__ __launch_bounds__(256) void k_assembly(PairSide R, PairSide C, int64_t npad, int B,
                                                  int ZS, TabView tab, double sig,
                                                  double *__restrict__ out, int64_t ld,
                                                  double *__restrict__ cube,
                                                  const Tile *__restrict__ tiles, int G, int b0,
                                                  int b1) {
  static_assert(MODE == 1 || MODE == 2, "the ABI modes");
  const int I = blockIdx.y, J = blockIdx.x;
  if (MODE != 2 && J > I) return;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t r = (int64_t)I * AT + lane;
  if (r >= R.n) return;
  double xr[PM];
#pragma unroll
  for (int i = 0; i < PM; ++i) xr[i] = R.X[r * PM + i];
  const int64_t cubeld = R.n;  // n (sym) or n1 (cross)
  const int64_t slice = (MODE == 2) ? R.n * C.n : R.n * R.n;

  for (int m = 0; m < AT / 4; ++m) {
    const int64_t c = (int64_t)J * AT + wv + 4 * m;  // wave-uniform
    if (c >= C.n) break;
    if (MODE == 1 && I == J && c > r) continue;  // lower half, mirrored below
    if (!(c < C.n)) continue;                    // (never taken, see above)
    double d2[PM];
#pragma unroll
    for (int i = 0; i < PM; ++i) {
      const double d = xr[i] - C.X[c * PM + i];
      d2[i] = d * d;
    }
    const bool rlo = (MODE == 2) || (r < c);  // row is the reference's first operand
    double kf = 0.0;
    for (int b = b0; b < b1; ++b) {  // [0, B), or the marginal slices of prediction
      const double *w = tab.wk + b * PM;
      double r2 = 0.0;
#pragma unroll
      for (int i = 0; i < PM; ++i) r2 = fma(d2[i], w[i], r2);
      double zr = 0.0, zc = 0.0, lzr = 0.0, lzc = 0.0;
      if (b > 0) {
        zr = R.Z[r * ZS + b - 1];
        zc = C.Z[c * ZS + b - 1];
        if (KIND == 0) {
          lzr = R.LZ[r * ZS + b - 1];
          lzc = C.LZ[c * ZS + b - 1];
        }
      }
      const double kb =
          rlo ? kval<KIND, MODE == 2>(b, r2, tab.lam[b], zr, zc, lzr, lzc)
              : kval<KIND, MODE == 2>(b, r2, tab.lam[b], zc, zr, lzc, lzr);
      kf += kb;
      if (cube) {
        cube[r + c * cubeld + b * slice] = kb;
        if (MODE == 1 && c != r) cube[c + r * cubeld + b * slice] = kb;
      }
    }
    out[r + c * ld] = kf;
    if (MODE == 1 && c != r) out[c + r * ld] = kf;
  }
}

// ---------------------------------------------------------------------------
// Gradient traces.  T = w_rc (sA A[r,c] - alpha_r alpha_c) on lower pairs,
// w = 2 off the diagonal, 1 on it (T and dK are symmetric, so the full-matrix
// trace tr(T dK) = sum_rc T_rc dK_rc, src/include/ace_kernel_utils.hpp:23-26).
// Per b: lambda sum   sum T K_b                       (src/kernel_SE_cpp.cpp:224-227)
//        length sums  sum T K_b d_i^2                 (SE, 161-188)
//                     sum T K_b/(1+sqrt(3 r~2)) d_i^2 (Matern32, kernel_Matern 340-377;
//                     r~2 uses the gradient-indexed weights wg)
// One 64x64 lower tile per workgroup; T stays in registers (16 pairs per
// lane) while the b loop runs outermost with PM+1 running sums.  The per-b
// block reduction goes through LDS in [value][thread] order (conflict-free,
// two levels) instead of 6-step cross-lane shuffles per value.
// ---------------------------------------------------------------------------
// Column-side operands (x_c, z_c, weight rows) are wave-uniform: they are
// read through the constant address space so they land in SGPRs via scalar
// loads instead of 64-lane vector loads of one address.
typedef const __attribute__((address_space(4))) double *cdp;

// K_b comes from the cube (kernmat's, for the same theta); Matern32 forms
// r~2_b from the pair's d_i^2 and the gradient-indexed weights of slice b.
template <int PM, int KIND>
__global__ __launch_bounds__(256) void k_grad(PairSide S, int B, int ZS, TabView tab,
                                              const double *__restrict__ A, int64_t ld,
                                              double sA, const double *__restrict__ alpha,
                                              const double *__restrict__ cube,
                                              double *__restrict__ gpart, int64_t ldg,
                                              const Tile *__restrict__ tiles, int G) {
  constexpr int NV = PM + 1;
  constexpr int NM = AT / 4;
  __shared__ double red[NV][64];
  __shared__ double red2[NV][4];
  __shared__ double sT[NM][256];  // T of each lane's pairs
  const int64_t t = blockIdx.x;
  int64_t I, J;
  if (tiles) {  // the rank's own lower tiles, or the model's XCD-dealt order
    const Tile tt = tiles[t];
    I = tt.I;
    J = tt.J;
    if (I < 0) {  // padding of an XCD-dealt list: an all-zero partial row
      for (int64_t e = threadIdx.x; e < ldg; e += 256) gpart[t * ldg + e] = 0.0;
      return;
    }
    A += (lcol(J * AT, G) - J * AT) * ld;
  } else {
    I = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    while (I * (I + 1) / 2 > t) --I;
    J = t - I * (I + 1) / 2;
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t n = S.n;
  const int64_t r = I * AT + lane;
  const bool rvalid = r < n;
  const int64_t rr = rvalid ? r : 0;
  const int64_t c0 = J * AT + wv;  // columns c0 + 4m (rows of X exist up to a multiple of 64)
  cdp Xc = (cdp)S.X;
  cdp WG = (cdp)tab.wg;

  double xr[PM];
#pragma unroll
  for (int i = 0; i < PM; ++i) xr[i] = S.X[rr * PM + i];
  const double ar = rvalid ? alpha[rr] : 0.0;

  unsigned valid = 0;
  double tr = 0.0;
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    const int64_t c = c0 + 4 * m;
    const bool v = rvalid && c < n && !(I == J && c > r);
    double tv = 0.0;
    if (v) {
      tv = sA * A[r + c * ld] - ar * alpha[c];
      if (c == r) tr += tv;
      else tv *= 2.0;
      valid |= 1u << m;
    }
    sT[m][tid] = tv;  // each lane only ever reads its own column of sT
  }

  for (int b = B - 1; b >= 0; --b) {
    double g[PM];
#pragma unroll
    for (int i = 0; i < PM; ++i) g[i] = 0.0;
    double gl = 0.0;
    cdp wg = WG + b * PM;
#pragma unroll 1
    for (int m = 0; m < NM; ++m) {
      const int64_t c = c0 + 4 * m;
      double d2[PM];
#pragma unroll
      for (int i = 0; i < PM; ++i) {
        const double d = xr[i] - Xc[c * PM + i];
        d2[i] = d * d;
      }
      const double kb = ((valid >> m) & 1u) ? cube[r + c * n + (int64_t)b * n * n] : 0.0;
      double rt2 = 0.0;
      if (KIND == 1) {
#pragma unroll
        for (int i = 0; i < PM; ++i) rt2 = fma(d2[i], wg[i], rt2);
      }
      const double tm = sT[m][tid];
      gl = fma(tm, kb, gl);
      double U;
      if (KIND == 0) U = tm * kb;
      else U = tm * (kb / (1.0 + sqrt(3.0 * rt2)));
#pragma unroll
      for (int i = 0; i < PM; ++i) g[i] = fma(U, d2[i], g[i]);
    }
    // block reduction: two xor-shuffle steps fold each wave to 16 lanes, the
    // 64 survivors go to LDS in [value][slot] order, 4 x 16 -> 4 -> 1
#pragma unroll
    for (int i = 0; i < PM; ++i) {
      double v = g[i];
      v += __shfl_xor(v, 32, 64);
      v += __shfl_xor(v, 16, 64);
      if (lane < 16) red[i][wv * 16 + lane] = v;
    }
    {
      double v = gl;
      v += __shfl_xor(v, 32, 64);
      v += __shfl_xor(v, 16, 64);
      if (lane < 16) red[PM][wv * 16 + lane] = v;
    }
    __syncthreads();
    if (tid < NV * 4) {
      const int i = tid % NV, sg = tid / NV;
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) s += red[i][16 * sg + k];
      red2[i][sg] = s;
    }
    __syncthreads();
    if (tid < NV) {
      const double s = (red2[tid][0] + red2[tid][1]) + (red2[tid][2] + red2[tid][3]);
      gpart[t * ldg + (int64_t)b * NV + tid] = s;
    }
  }
  // trace of T (diagonal pairs)
  {
    double v = tr;
    v += __shfl_xor(v, 32, 64);
    v += __shfl_xor(v, 16, 64);
    if (lane < 16) red[0][wv * 16 + lane] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < 64; ++k) s += red[0][k];
    gpart[t * ldg + (int64_t)B * NV] = s;
  }
}

// ---------------------------------------------------------------------------
// Diagonal of a symmetric kernel matrix over slices [b0, b1): r2 = 0 on the
// diagonal, so K_b(r, r) is the reference expression at r2 = 0 with both z
// operands z_r (kernmat_*_symmetric_cpp's r == c entries; prediction needs
// only diag(K_xx), src/pred_cpp.cpp:22-28, 71-77).
// ---------------------------------------------------------------------------
template <int KIND>
__global__ void k_kdiag(PairSide S, int ZS, TabView tab, int b0, int b1, double *__restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= S.n) return;
  double s = 0.0;
  for (int b = b0; b < b1; ++b) {
    double z = 0.0, lz = 0.0;
    if (b > 0) {
      z = S.Z[r * ZS + b - 1];
      if (KIND == 0) lz = S.LZ[r * ZS + b - 1];
    }
    s += kval<KIND, false>(b, 0.0, tab.lam[b], z, z, lz, lz);
  }
  out[r] = s;
}

hipError_t launch_kdiag(int kind, PairSide S, int ZS, TabView tab, int b0, int b1, double *out,
                        hipStream_t st) {
  if (S.n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((S.n + 255) / 256));
  if (kind == 0) hipLaunchKernelGGL(k_kdiag<0>, grid, dim3(256), 0, st, S, ZS, tab, b0, b1, out);
  else hipLaunchKernelGGL(k_kdiag<1>, grid, dim3(256), 0, st, S, ZS, tab, b0, b1, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Dispatch over the compiled feature-count buckets.
// ---------------------------------------------------------------------------
int pm_bucket(int p) {
  for (int b : PM_BUCKETS)
    if (p <= b) return b;
  return -1;
}

int64_t grad_ntiles(int64_t n) {
  const int64_t nt = (n + AT - 1) / AT;
  return nt * (nt + 1) / 2;
}

template <int PM>
static hipError_t asm_pm(int mode, int kind, PairSide R, PairSide C, int B, int ZS, TabView tab,
                         double *out, int64_t ld, double *cube, hipStream_t st, int b0, int b1) {
  dim3 blk(256);
  dim3 grid;
  if (mode == 1) {
    const unsigned nt = (unsigned)((R.n + AT - 1) / AT);
    grid = dim3(nt, nt);
  } else {
    grid = dim3((unsigned)((C.n + AT - 1) / AT), (unsigned)((R.n + AT - 1) / AT));
  }
#define ACE_ASM(K, M)                                                                         \
  hipLaunchKernelGGL((k_assembly<PM, K, M>), grid, blk, 0, st, R, C, (int64_t)0, B, ZS, tab, 0.0, \
                     out, ld, cube, (const Tile *)nullptr, 1, b0, b1)
  if (kind == 0) {
    if (mode == 1) ACE_ASM(0, 1);
    else ACE_ASM(0, 2);
  } else {
    if (mode == 1) ACE_ASM(1, 1);
    else ACE_ASM(1, 2);
  }
#undef ACE_ASM
  return hipGetLastError();
}

int zskip_mode(int64_t n) {
  static const int v = env_set("ACE_ZSKIP") ? std::max(0, std::min(2, env_int("ACE_ZSKIP", 2))) : -1;
  return v >= 0 ? v : (n > 8192 ? 2 : 1);
}

// The ABI's kernel matrices.  Cross without a cube: k_cross_mm; everything
// else (a cube to fill, or the symmetric full output): k_assembly.
hipError_t launch_assembly(int mode, int kind, int PM, PairSide R, PairSide C, int B, int ZS,
                           TabView tab, double *out, int64_t ld, double *cube, hipStream_t st,
                           int b0, int b1) {
  if (mode != 1 && mode != 2) return hipErrorInvalidValue;
  if (b1 < 0) b1 = B;
  if (mode == 2 && !cube) return launch_cross_mm(kind, PM, R, C, B, ZS, tab, b0, b1, out, ld, st);
  switch (PM) {
#define ACE_CASE(P) \
  case P:           \
    return asm_pm<P>(mode, kind, R, C, B, ZS, tab, out, ld, cube, st, b0, b1);
    ACE_CASE(4) ACE_CASE(8) ACE_CASE(12) ACE_CASE(16) ACE_CASE(20) ACE_CASE(24)
    ACE_CASE(32) ACE_CASE(48) ACE_CASE(64)
#undef ACE_CASE
    default: return hipErrorInvalidValue;
  }
}

template <int PM>
static hipError_t grad_pm(int kind, PairSide S, int B, int ZS, TabView tab, const double *A,
                          int64_t ld, double sA, const double *alpha, const double *cube,
                          double *gpart, hipStream_t st, const Tile *tiles, int64_t ntiles,
                          int G) {
  const int64_t nsuper = tiles ? ntiles : grad_ntiles(S.n);
  if (nsuper == 0) return hipSuccess;
  const int64_t ldg = grad_part_cols(PM, B);
  dim3 grid((unsigned)nsuper), blk(256);
#define ACE_G(K)                                                                               \
  hipLaunchKernelGGL((k_grad<PM, K>), grid, blk, 0, st, S, B, ZS, tab, A, ld, sA, alpha, cube, \
                     gpart, ldg, tiles, G)
  if (kind == 0) ACE_G(0);
  else ACE_G(1);
#undef ACE_G
  return hipGetLastError();
}

int grad_order_block() {
  // 4: gradient HBM reads 1.52 -> 1.21 GB per C2 evaluation against the
  // 1.07 GB lower triangle (the per-tile X / Z staging stays in each XCD's
  // L2), time-neutral (profiles/r02_grad_ab.txt)
  static const int v = std::max(0, env_int("ACE_GRAD_ORDER", 4));
  return v;
}

hipError_t launch_grad(int kind, int PM, PairSide S, int B, int ZS, TabView tab,
                       const double *A, int64_t ld, double sA, const double *alpha,
                       const double *cube, double *gpart, hipStream_t st,
                       const Tile *tiles, int64_t ntiles, int G, int64_t ndiag) {
  // A cube given and PM <= 48: k_grad reads K_b from it.  Else the MFMA
  // kernel, which recomputes K_b (the cube is kernmat's K_b for the same
  // theta, so the traces are the same): k_grad's per-lane p-long arrays and
  // static LDS outgrow their budget at PM = 64 (it returned wrong traces
  // there), so it has no instantiation above PM = 48.
  if (!cube || PM > 48)
    return launch_grad_mm(kind, PM, S, B, ZS, tab, A, ld, sA, alpha, gpart, st, tiles, ntiles,
                          G, ndiag);
  switch (PM) {
#define ACE_CASE(P) \
  case P:           \
    return grad_pm<P>(kind, S, B, ZS, tab, A, ld, sA, alpha, cube, gpart, st, tiles, ntiles, G);
    ACE_CASE(4) ACE_CASE(8) ACE_CASE(12) ACE_CASE(16) ACE_CASE(20) ACE_CASE(24)
    ACE_CASE(32) ACE_CASE(48)
#undef ACE_CASE
    default: return hipErrorInvalidValue;
  }
}

}  // namespace ace
