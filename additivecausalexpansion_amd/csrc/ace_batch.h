// ace_batch.h -- shared between the batched kernels (ace_batch.hip) and their
// host side (ace_batch.cpp): many small models, one workgroup per model.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ace_formulas.h"
#include "ace_wg_geom.h"

namespace ace {

constexpr int BATCH_NMAX = WG_NMAX;  // rows of the largest model one workgroup takes

// Feature-count buckets of k_batch_eval (its own, coarser than pm_bucket's).
int batch_pm_bucket(int p);
// A model's scratch matrix has wg_rows(nmax) rows (= leading dimension); the
// first two rows of its last block carry the right-hand sides y and 1.
// threads of the batch kernels: eight waves where the per-lane feature arrays leave
// room for them (two waves per SIMD hide the scratch matrix's latency), four above
__host__ __device__ constexpr int batch_threads(int PM) { return PM <= 16 ? 512 : 256; }
// dynamic LDS of k_batch_eval in bytes
size_t batch_lds_bytes(int nmax, int B, int PM);

// Per model j: n[j] rows; y, X (row-major n x PM), Z / LZ (row-major n x ZS)
// at stride nmax rows; scratch matrix A + j ld ld (column-major, lower
// triangle used).  theta of model j at theta + j ldt.  out + j ldo: grad (P),
// stats (2), mu_solution, flag.  ctl (null: every model runs) holds {last
// iteration done, stop} per model; skip = 1 leaves out models with stop != 0,
// skip = 2 those with stop == 2.
struct BatchView {
  int M, nmax, p, B, PM, ZS, P;
  int64_t ld;
  const int *n;
  const double *y, *X, *Z, *LZ, *std_y;
  double *A;
  const double *theta;
  int64_t ldt;
  double *out;
  int64_t ldo;
  const int *ctl;
  int skip, use_mu;
};
hipError_t launch_batch_eval(int kind, const BatchView &v, hipStream_t st);

struct BatchStepCfg {
  OptCfg opt;
  int P, M;
};
// ace_model_train's per-iteration tail per model: st + j 3 P = [theta | m1 | m2], hist + j ldh
// the model's stats matrix, ctl as above, out as k_batch_eval left it.
hipError_t launch_batch_step(const BatchStepCfg &c, int it, const double *out, int64_t ldo,
                             double *st, double *hist, int64_t ldh, int *ctl, hipStream_t stream);

// ---- prediction (ace_batch_predict.hip) ------------------------
constexpr int BPT = 2;  // 16-point test tiles a workgroup holds in LDS at a time
// LDS pitch of a test tile's cross rows (2 mod 32 doubles: the 32 lanes of a
// half wave, 16 test points x 2 training columns, read 32 different banks)
__host__ __device__ constexpr int batch_predict_pitch(int nmax) {
  return (nmax + BT - 1) / BT * BT + ((nmax + BT - 1) / BT % 2 ? 18 : 2);
}
// dynamic LDS of k_batch_predict in bytes
size_t batch_predict_lds_bytes(int nmax, int B, int PM);

// Model j: the training slots and scratch matrix of BatchView (the n x n part
// of A holds -A^-1, lower triangle), flag[j] != 0: not positive definite.
// Test points off[j] .. off[j + 1] - 1 of the packed test side: X2 row-major
// x PM, Z2 / LZ2 row-major x ZS (the basis, or its derivative when marginal),
// zx the binary treatment (ate).  Out, per test point: a = k alpha,
// kd = K_xx(i, i), q = k A^-1 k^T; per model gcov[3] = the posterior
// covariance of the group sums (treated-treated, treated-untreated,
// untreated-untreated).
struct BatchPredView {
  int M, nmax, p, B, PM, ZS, marginal, ate;
  int64_t ld;
  const int *n;
  const double *y, *X, *Z, *LZ;
  const double *A, *flag;
  const double *theta;
  int64_t ldt;
  const int64_t *off;
  const double *X2, *Z2, *LZ2, *zx;
  double *a, *kd, *q, *gcov;
};
hipError_t launch_batch_predict(int kind, const BatchPredView &v, hipStream_t st);

}  // namespace ace
