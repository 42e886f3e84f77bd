// ace_cv_plan.cpp -- see ace_cv_plan.h.
#include "ace_cv_plan.h"

#include <algorithm>
#include <numeric>

namespace ace {

std::string cv_plan(int64_t n, int64_t nf, const int64_t *off, const int64_t *idx,
                    const int64_t *perm, int wg_max, CvPlan *out) {
  if (n < 1 || nf < 1 || !off || !idx || !out) return "cv: bad shape / null argument";
  if (off[0] != 0) return "cv: off[0] must be 0";
  for (int64_t f = 0; f < nf; ++f) {
    if (off[f + 1] < off[f])
      return "cv: off must be non-decreasing (fold " + std::to_string(f) + ")";
    if (off[f + 1] == off[f]) return "cv: fold " + std::to_string(f) + " is empty";
  }
  const int64_t total = off[nf];
  for (int64_t k = 0; k < total; ++k)
    if (idx[k] < 0 || idx[k] >= n)
      return "cv: index " + std::to_string(idx[k]) + " out of range [0, " + std::to_string(n) + ")";
  wg_max = std::max(1, std::min(wg_max, CV_WG_MAX));

  CvPlan &p = *out;
  p = CvPlan();
  p.n = n;
  p.nf = nf;
  p.total = total;
  // the caller's row -> the device row (the inverse of perm)
  std::vector<int64_t> dev;
  if (perm) {
    dev.assign((size_t)n, -1);
    for (int64_t k = 0; k < n; ++k) {
      if (perm[k] < 0 || perm[k] >= n || dev[(size_t)perm[k]] >= 0)
        return "cv: perm is not a permutation";
      dev[(size_t)perm[k]] = k;
    }
  }
  p.rows.resize((size_t)total);
  p.scatter.resize((size_t)total);
  p.folds.resize((size_t)nf);
  bool all_one = true;
  std::vector<int64_t> ord;
  for (int64_t f = 0; f < nf; ++f) {
    CvFold &c = p.folds[(size_t)f];
    c.off = off[f];
    c.m = off[f + 1] - off[f];
    all_one = all_one && c.m == 1;
    ord.resize((size_t)c.m);
    std::iota(ord.begin(), ord.end(), (int64_t)0);
    auto row = [&](int64_t k) { return perm ? dev[(size_t)idx[c.off + k]] : idx[c.off + k]; };
    std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return row(a) < row(b); });
    for (int64_t k = 0; k < c.m; ++k) {
      p.rows[(size_t)(c.off + k)] = row(ord[(size_t)k]);
      p.scatter[(size_t)(c.off + k)] = ord[(size_t)k];
      if (k > 0 && p.rows[(size_t)(c.off + k)] == p.rows[(size_t)(c.off + k - 1)])
        return "cv: index " + std::to_string(idx[c.off + ord[(size_t)k]]) + " appears twice in fold " +
               std::to_string(f);
    }
    p.work += (double)c.m * (double)c.m * (double)c.m;
  }
  for (int64_t f = 0; f < nf; ++f) {
    CvFold &c = p.folds[(size_t)f];
    if (all_one) {
      c.cls = CV_LOO;
    } else if (c.m <= wg_max) {
      c.cls = CV_WG;
      c.mpad = (c.m + BT - 1) / BT * BT;
      c.ld = wg_rows(c.m);
      c.scratch = p.wg_doubles;
      p.wg_doubles += c.ld * c.ld;
      p.wg_mmax = std::max(p.wg_mmax, c.m);
      p.wg.push_back(f);
    } else {
      c.cls = CV_SWEEP;
      p.sweep.push_back(f);
    }
  }
  p.lds_bytes = p.wg.empty() ? 0 : wg_sweep_lds_bytes(p.wg_mmax);
  return "";
}

}  // namespace ace
