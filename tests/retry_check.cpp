// Stand-alone check of the retained-scratch policy's control flow
// (csrc/ace_retry.h, the function ace_predict.cpp's with_pred_scratch runs):
// fake bodies, and counts of what ran.  Built and run by
// tests/test_retry_cpu.py with a host compiler and AddressSanitizer + UBSan;
// needs no GPU and no HIP header.
#include <stdio.h>

#include "ace_retry.h"

using namespace ace_host;

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      ++failures;                                 \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
    }                                             \
  } while (0)

struct Fail {
  int code;
};
constexpr int OOM = -4, OTHER = -3;

// One run of the policy: the body's attempt k (from 0) throws Fail{plan[k]}
// when plan[k] != 0.  Records how often each part ran and what came out.
struct Run {
  int bodies = 0, recoveries = 0, trims = 0;
  int thrown = 0;               // the code that left retry_once_on (0: none)
  bool recovered_first = true;  // the recovery ran before the second attempt
  explicit Run(const int (&plan)[2]) {
    try {
      retry_once_on<Fail>(
          OOM,
          [&] {
            const int k = bodies++;
            if (k == 1 && recoveries != 1) recovered_first = false;
            if (k < 2 && plan[k] != 0) throw Fail{plan[k]};
          },
          [&] { ++recoveries; }, [&] { ++trims; });
    } catch (const Fail &f) {
      thrown = f.code;
    }
  }
};

int main() {
  {  // success first time: recovery not called, trim called once
    const Run r({0, 0});
    CHECK(r.bodies == 1 && r.recoveries == 0 && r.trims == 1 && r.thrown == 0,
          "success: bodies %d recoveries %d trims %d thrown %d", r.bodies, r.recoveries, r.trims,
          r.thrown);
  }
  {  // OOM then success: recovery once, body twice, trim once
    const Run r({OOM, 0});
    CHECK(r.bodies == 2 && r.recoveries == 1 && r.trims == 1 && r.thrown == 0 && r.recovered_first,
          "OOM then success: bodies %d recoveries %d trims %d thrown %d", r.bodies, r.recoveries,
          r.trims, r.thrown);
  }
  {  // OOM twice: the second failure propagates, body exactly twice, no trim
    const Run r({OOM, OOM});
    CHECK(r.bodies == 2 && r.recoveries == 1 && r.trims == 0 && r.thrown == OOM,
          "OOM twice: bodies %d recoveries %d trims %d thrown %d", r.bodies, r.recoveries, r.trims,
          r.thrown);
  }
  {  // OOM, then another failure: that one propagates too, no third attempt
    const Run r({OOM, OTHER});
    CHECK(r.bodies == 2 && r.recoveries == 1 && r.trims == 0 && r.thrown == OTHER,
          "OOM then other: bodies %d recoveries %d trims %d thrown %d", r.bodies, r.recoveries,
          r.trims, r.thrown);
  }
  {  // a non-OOM failure: propagates at once, recovery not called, no trim
    const Run r({OTHER, 0});
    CHECK(r.bodies == 1 && r.recoveries == 0 && r.trims == 0 && r.thrown == OTHER,
          "other failure: bodies %d recoveries %d trims %d thrown %d", r.bodies, r.recoveries,
          r.trims, r.thrown);
  }
  {  // a failure of the recovery itself propagates; no second attempt, no trim
    int bodies = 0, trims = 0, thrown = 0;
    try {
      retry_once_on<Fail>(
          OOM,
          [&] {
            ++bodies;
            throw Fail{OOM};
          },
          [&] { throw Fail{OTHER}; }, [&] { ++trims; });
    } catch (const Fail &f) {
      thrown = f.code;
    }
    CHECK(bodies == 1 && trims == 0 && thrown == OTHER, "failing recovery: bodies %d trims %d thrown %d",
          bodies, trims, thrown);
  }
  if (failures) {
    printf("retry_check: %d FAILURES\n", failures);
    return 1;
  }
  printf("retry_check: OK\n");
  return 0;
}
