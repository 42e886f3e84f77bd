// ace_wg_geom.h -- the geometry of the workgroup-level SPD sweep, stated once
// for its two users, k_batch_eval (ace_batch.hip) and k_cv_fold
// (ace_cv.hip), and for their host sides.
// Plain C++, no HIP header: the cross-validation plan and its stand-alone
// check build with a host compiler alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define ACE_HD __host__ __device__
#else
#define ACE_HD
#endif

namespace ace {

// LDS a gfx950 workgroup can use, and what a kernel gets without asking
// (launch_lds, ace_internal.h)
constexpr size_t LDS_MAX = 160 * 1024, LDS_DEFAULT = 64 * 1024;

constexpr int BT = 16;        // pivot block = MFMA fragment width
constexpr int WG_NMAX = 512;  // rows of the largest matrix one workgroup sweeps

// rows (= leading dimension) of a working matrix: n padded to BT, plus one BT
// block whose first rows carry the right-hand sides
template <class T>
ACE_HD constexpr T wg_rows(T n) {
  return (n + BT - 1) / BT * BT + BT;
}
// LDS pitch of a pivot panel (16 mod 32 doubles: the two 16-lane groups of a
// half wave read different banks)
template <class T>
ACE_HD constexpr T wg_pitch(T nmax) {
  return wg_rows(nmax) % 32 == 16 ? wg_rows(nmax) : wg_rows(nmax) + 16;
}

// LDS map of the sweep (doubles).  Fixed head: scal[16], the pivot block
// D[2][BT][WG_DP].  Behind it (WG_L_REG) the panels P and W, BT x pitch each,
// k-major; a kernel may use that region for something else outside the sweep.
constexpr int WG_DP = BT + 1;  // pitch of the pivot block
constexpr int WG_L_SCAL = 0, WG_L_D = 16, WG_L_REG = WG_L_D + 2 * BT * WG_DP;
// head and panels in bytes
constexpr int64_t wg_sweep_lds_bytes(int64_t nmax) {
  return (WG_L_REG + 2 * BT * wg_pitch(nmax)) * (int64_t)sizeof(double);
}

}  // namespace ace
