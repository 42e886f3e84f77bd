// ace_retry.h -- the control flow of a call that works in scratch retained
// between calls (ace_predict.cpp's with_pred_scratch): run the body; if it
// fails with `code` (out of device memory), recover -- free what was retained
// -- and run the body once more; after a run that succeeded, trim what is
// kept.  A second failure propagates, any other failure propagates at once
// without the recovery, and neither is followed by the trim.  The body must
// write its outputs only at its end.  No HIP header: the policy is built and
// checked by a host compiler alone (tests/retry_check.cpp), and the library
// runs this same function.
#pragma once

namespace ace_host {

// Failure: the exception type, with an int member `code`.
template <class Failure, class Body, class Recover, class Trim>
void retry_once_on(int code, Body &&body, Recover &&recover, Trim &&trim) {
  try {
    body();
  } catch (const Failure &f) {
    if (f.code != code) throw;
    recover();
    body();
  }
  trim();
}

}  // namespace ace_host
