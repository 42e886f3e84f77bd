// ace_cv_plan.h -- host-only planning of one cross-validation call (DESIGN
// §18): fold validation, the map from the caller's rows to device rows, the
// order inside a fold, the three execution classes and each fold's scratch.
// No HIP header, so tests/cv_plan_check.cpp checks it with a host compiler
// alone.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "ace_wg_geom.h"

namespace ace {

// largest fold one workgroup takes (k_cv_fold): the workgroup sweep's bound
constexpr int CV_WG_MAX = WG_NMAX;

// A workgroup fold's working matrix: m padded to BT plus one BT block whose
// first row carries the right-hand side alpha_F; column-major, ld = rows =
// wg_rows(m).  k_cv_fold's dynamic LDS is the sweep's, wg_sweep_lds_bytes of
// the call's largest m.

enum CvClass : int {
  CV_LOO = 0,    // every fold of the call has one row: elementwise (k_cv_loo)
  CV_WG = 1,     // one workgroup per fold (k_cv_gather + k_cv_fold)
  CV_SWEEP = 2,  // the whole-chip sweep, one fold after another
};

struct CvFold {
  int64_t off = 0;      // first entry in rows / scatter (the caller's off[f])
  int64_t m = 0;        // rows held out
  int cls = CV_WG;
  int64_t mpad = 0;     // CV_WG: m padded to BT
  int64_t ld = 0;       // CV_WG: wg_rows(m)
  int64_t scratch = 0;  // CV_WG: first double of the fold's working matrix
};

struct CvPlan {
  int64_t n = 0, nf = 0, total = 0;  // total = off[nf]
  // device rows, ascending inside each fold; entry off + k came from the
  // caller's position off + scatter[off + k] of that fold
  std::vector<int64_t> rows, scatter;
  std::vector<CvFold> folds;
  std::vector<int64_t> wg, sweep;  // fold ids by class, in the caller's order
  int64_t wg_doubles = 0;          // the workgroup folds' scratch in all
  int64_t wg_mmax = 0;             // their largest m (sizes the LDS)
  int64_t lds_bytes = 0;
  double work = 0.0;               // sum over folds of m^3
};

// Plans the folds idx[off[f] .. off[f + 1]) of n rows.  perm (null: the
// identity): the device's point k is the caller's perm[k].  wg_max: folds above
// it take the sweep (clamped to 1 .. CV_WG_MAX).  Returns "" and fills *out,
// or the reason the fold list is refused.
std::string cv_plan(int64_t n, int64_t nf, const int64_t *off, const int64_t *idx,
                    const int64_t *perm, int wg_max, CvPlan *out);

}  // namespace ace
