// cv_plan_check.cpp -- stand-alone check of the cross-validation plan
// (csrc/ace_cv_plan.cpp), built by tests/test_cv_cpu.py with a host compiler
// under AddressSanitizer + UBSan: malformed fold lists, the perm round trip,
// the class thresholds, the scratch layout and the work count.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "ace_cv_plan.h"

using namespace ace;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      ++fails;                                                    \
    }                                                             \
  } while (0)

static std::string plan(int64_t n, const std::vector<int64_t> &off, const std::vector<int64_t> &idx,
                        const int64_t *perm, int wg_max, CvPlan *p) {
  return cv_plan(n, (int64_t)off.size() - 1, off.data(), idx.data(), perm, wg_max, p);
}

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

int main() {
  CvPlan p;
  // ---- malformed lists ------------------------------------------------------
  CHECK(has(plan(10, {0, 2}, {3, 10}, nullptr, 512, &p), "out of range"));
  CHECK(has(plan(10, {0, 2}, {-1, 3}, nullptr, 512, &p), "out of range"));
  CHECK(has(plan(10, {0, 3}, {3, 4, 3}, nullptr, 512, &p), "appears twice in fold 0"));
  CHECK(has(plan(10, {0, 2, 2, 3}, {1, 2, 3}, nullptr, 512, &p), "fold 1 is empty"));
  CHECK(has(plan(10, {0, 2, 1}, {1, 2, 3}, nullptr, 512, &p), "non-decreasing"));
  CHECK(has(plan(10, {1, 2}, {1, 2}, nullptr, 512, &p), "off[0]"));
  {  // a duplicate through the perm, and a perm that is none
    const std::vector<int64_t> bad = {0, 1, 1, 3};
    CHECK(has(plan(4, {0, 2}, {0, 1}, bad.data(), 512, &p), "not a permutation"));
  }
  // the same index in two folds is fine (overlap), and folds need not cover
  CHECK(plan(10, {0, 2, 4}, {1, 2, 2, 3}, nullptr, 512, &p).empty());
  CHECK(p.nf == 2 && p.total == 4 && p.wg.size() == 2);

  // ---- perm round trip ------------------------------------------------------
  std::mt19937_64 rng(7);
  for (int trial = 0; trial < 20; ++trial) {
    const int64_t n = 50 + 37 * trial;
    std::vector<int64_t> perm((size_t)n), src((size_t)n);
    std::iota(perm.begin(), perm.end(), (int64_t)0);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::iota(src.begin(), src.end(), (int64_t)0);
    std::shuffle(src.begin(), src.end(), rng);
    // three folds: ragged pieces of a shuffled index list
    const int64_t c1 = n / 5, c2 = n / 2 + trial;
    const std::vector<int64_t> off = {0, c1, c2, n};
    CHECK(plan(n, off, src, trial % 2 ? perm.data() : nullptr, 512, &p).empty());
    for (int f = 0; f < 3; ++f) {
      const CvFold &c = p.folds[(size_t)f];
      CHECK(c.off == off[(size_t)f] && c.m == off[(size_t)f + 1] - off[(size_t)f]);
      std::vector<char> seen((size_t)c.m, 0);
      for (int64_t k = 0; k < c.m; ++k) {
        const int64_t row = p.rows[(size_t)(c.off + k)], sc = p.scatter[(size_t)(c.off + k)];
        CHECK(row >= 0 && row < n && sc >= 0 && sc < c.m);
        if (k > 0) CHECK(row > p.rows[(size_t)(c.off + k - 1)]);  // ascending
        // the device's point `row` is the caller's perm[row]: the index the
        // caller gave at position sc of the fold
        const int64_t caller = trial % 2 ? perm[(size_t)row] : row;
        CHECK(caller == src[(size_t)(c.off + sc)]);
        CHECK(!seen[(size_t)sc]);
        seen[(size_t)sc] = 1;
      }
    }
  }

  // ---- classes at 1, 512, 513; LOO; ACE_CV_WG_MAX ----------------------------
  {
    const int64_t n = 1100;
    std::vector<int64_t> idx, off = {0};
    for (int64_t m : {1, 512, 513, 16, 17}) {
      for (int64_t k = 0; k < m; ++k) idx.push_back(k + 3);
      off.push_back((int64_t)idx.size());
    }
    CHECK(plan(n, off, idx, nullptr, 512, &p).empty());
    CHECK(p.folds[0].cls == CV_WG && p.folds[1].cls == CV_WG && p.folds[2].cls == CV_SWEEP);
    CHECK(p.folds[3].cls == CV_WG && p.folds[4].cls == CV_WG);
    CHECK(p.wg.size() == 4 && p.sweep.size() == 1 && p.sweep[0] == 2 && p.wg_mmax == 512);
    CHECK(p.folds[0].ld == 32 && p.folds[1].ld == 528 && p.folds[3].ld == 32 && p.folds[4].ld == 48);
    CHECK(p.folds[1].mpad == 512 && p.folds[4].mpad == 32);
    CHECK(p.lds_bytes == wg_sweep_lds_bytes(512) && p.lds_bytes <= LDS_MAX);
    // scratch: disjoint, in order, ld^2 each
    int64_t end = 0;
    for (const int64_t f : p.wg) {
      const CvFold &c = p.folds[(size_t)f];
      CHECK(c.scratch == end && c.ld == wg_rows(c.m));
      end = c.scratch + c.ld * c.ld;
    }
    CHECK(end == p.wg_doubles);
    const double w = 1.0 + 512.0 * 512 * 512 + 513.0 * 513 * 513 + 16.0 * 16 * 16 + 17.0 * 17 * 17;
    CHECK(p.work == w);
    // a lower threshold sends 17 and above to the sweep; out-of-range values clamp
    CHECK(plan(n, off, idx, nullptr, 16, &p).empty());
    CHECK(p.wg.size() == 2 && p.sweep.size() == 3 && p.folds[4].cls == CV_SWEEP);
    CHECK(plan(n, off, idx, nullptr, 100000, &p).empty());
    CHECK(p.folds[1].cls == CV_WG && p.folds[2].cls == CV_SWEEP);
    CHECK(plan(n, off, idx, nullptr, 0, &p).empty());
    CHECK(p.folds[0].cls == CV_WG && p.folds[3].cls == CV_SWEEP);
  }
  {  // every fold of one row: the elementwise class, no scratch
    const std::vector<int64_t> off = {0, 1, 2, 3}, idx = {4, 0, 2};
    CHECK(plan(5, off, idx, nullptr, 512, &p).empty());
    CHECK(p.folds[0].cls == CV_LOO && p.folds[2].cls == CV_LOO && p.wg.empty() && p.sweep.empty());
    CHECK(p.wg_doubles == 0 && p.lds_bytes == 0 && p.work == 3.0);
    CHECK(p.rows[0] == 4 && p.rows[1] == 0 && p.rows[2] == 2);
    // one fold of two rows among them: the workgroup class for all
    CHECK(plan(5, {0, 1, 2, 4}, {4, 0, 2, 1}, nullptr, 512, &p).empty());
    CHECK(p.folds[0].cls == CV_WG && p.wg.size() == 3);
  }
  // the pitch keeps the two 16-lane groups of a half wave on different banks
  for (int64_t m = 1; m <= 512; ++m) CHECK(wg_pitch(m) % 32 == 16 && wg_pitch(m) >= wg_rows(m));

  if (fails) {
    std::printf("cv_plan_check: %d FAILED\n", fails);
    return 1;
  }
  std::printf("cv_plan_check: OK\n");
  return 0;
}
