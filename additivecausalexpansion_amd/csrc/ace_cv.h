// ace_cv.h -- cross-validation from a resident inverse: the
// kernels of ace_cv.hip as the host core (ace_cv.cpp) launches them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ace_cv_plan.h"

namespace ace {

// One fold on the device: rows[off .. off + m) are its device rows
// (ascending), its working matrix is W + scratch with leading dimension ld,
// and its per-fold outputs go to index `fold`.
struct CvDesc {
  int64_t off, m, ld, scratch, fold;
};

// The source matrix: S = sgn * P, symmetric, of which the lower triangle of P
// (ldp) is read; alpha = S (y - mu 1).
struct CvSrc {
  const double *P;
  int64_t ldp;
  double sgn;
  const double *alpha;
  const int64_t *rows;
};

// Per-fold results.  r, v: packed like rows (the fold's sorted order);
// logdet, mahal, status: one per fold id.  A fold whose status is not 0 has
// NaN in r, v, logdet and mahal.
struct CvRes {
  double *r, *v, *logdet, *mahal;
  int *status;
};

// Fold desc[j], j < nd, into its working matrix: +S[F, F] in the leading
// m x m block, unit diagonal on the padding, alpha_F in row npad of the
// columns k < m, zeros in the rest of the right-hand-side block.
// npad_sweep == 0: the workgroup layout (npad = ld - BT); the lower
// triangle alone is written and k_cv_fold reads through it.  npad_sweep > 0:
// a SweepWork's A (ld = naug): both triangles of the npad x npad block from
// the same source element (exactly symmetric) and every AUG row; af
// (optional, one fold) also receives alpha_F packed.  ldmax: the largest ld
// among the nd folds.
hipError_t launch_cv_gather(const CvSrc &s, const CvDesc *desc, int64_t nd, int64_t ldmax,
                            double *W, int64_t npad_sweep, double *af, hipStream_t st);
// One workgroup per fold desc[j], m <= CV_WG_MAX: the symmetric Gauss-Jordan
// sweep of the gathered matrix over its first npad pivots.  mmax: the largest
// m among them (LDS pitch).
hipError_t launch_cv_fold(const CvDesc *desc, int64_t nd, int64_t mmax, double *W, CvRes res,
                          hipStream_t st);
// Every fold has one row: r = alpha / S_ii, v = 1 / S_ii, logdet = log S_ii
hipError_t launch_cv_loo(const CvSrc &s, int64_t nf, CvRes res, hipStream_t st);
// One fold's results out of a swept SweepWork (A, ld, npad, its pivots and
// flag).  status: the first bad pivot (1-based), or -flag when the sweep
// failed without one.
hipError_t launch_cv_sweep_out(const double *A, int64_t ld, int64_t npad, const double *piv,
                               const int *flag, const CvDesc *desc, CvRes res, hipStream_t st);

}  // namespace ace
