// ace_internal.h -- shared declarations between the HIP kernel sources
// (ace_pairs*.hip, ace_sweep.hip, ace_util.hip, ace_symm.hip, ace_joint.hip,
// ace_train.hip, ace_batch*.hip, ace_cv.hip) and the host orchestration (ace_api.cpp, ace_shard.cpp,
// ace_predict.cpp, ace_dmat.cpp).  The sweep's host-only planning is
// ace_sweep_plan.h.
#pragma once
#include <algorithm>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "ace_formulas.h"
#include "ace_sweep_plan.h"
#include "ace_wg_geom.h"

namespace ace {

// One launch with `lds` bytes of dynamic LDS (up to LDS_MAX; a shape whose
// request can exceed it is refused by its launcher).  Above LDS_DEFAULT a
// kernel has to be allowed the size first: the attribute is set at every such
// launch, with no record kept, so it holds on whichever device is current.
template <class... P, class... A>
hipError_t launch_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st,
                      A... args) {
  if (lds > LDS_DEFAULT) {
    const hipError_t e = hipFuncSetAttribute((const void *)kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<P>(args)...);
  return hipGetLastError();
}

// Environment switches (ACE_*): the integer value of `name`, dflt when unset.
// Every switch is read once per process, as
//   static const T v = <expression of env_int("ACE_X", dflt)>;
// (the initialisation of a function-local static is thread-safe).
inline int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}
// whether `name` is set at all (switches whose default depends on the size)
inline bool env_set(const char *name) { return getenv(name) != nullptr; }
// Host syncs of the device training loops (ace_model_train, ace_batch_train):
// the stop words are read back every ACE_TRAIN_SYNC iterations (default 4).
inline int train_sync_every() {
  static const int v = std::max(1, env_int("ACE_TRAIN_SYNC", 4));
  return v;
}

// (AT, the assembly / gradient pair tile: ace_sweep_plan.h)
constexpr int PMAX = 64;   // largest supported covariate count p
constexpr int BMAX = 32;   // largest supported component count B

// Feature-count buckets the pair kernels are compiled for.
constexpr int PM_BUCKETS[] = {4, 8, 12, 16, 20, 24, 32, 48, PMAX};
int pm_bucket(int p);  // smallest compiled bucket >= p, or -1

// ---- column sharding ---------------------------------------------------------
// The sharded model (ace_shard.cpp) distributes A by NB-wide column blocks,
// block-cyclic over G ranks: block j lives on rank j % G, as local block
// j / G of a naug-row, column-major local array (same ld, same row index).
// Every kernel that touches A maps a global column through lcol(); G == 1 is
// the identity, which is the single-GPU layout.
__host__ __device__ __forceinline__ int64_t lcol(int64_t c, int G) {
  return G == 1 ? c : (c / NB / G) * NB + c % NB;
}

// Per-theta tables, b-major: wk[b*PM+i] = tab_weight(theta, B, b, i, false)
// (kernel index, Q1), wg[b*PM+i] = tab_weight(theta, B, b, i, true) (gradient
// index), lam[b] = theta[2+b].  Total 2*B*PM + B doubles.
struct TabView {
  const double *wk, *wg, *lam;
  // device exp(theta[0]) (the device-fused training loop's theta lives in
  // HBM); null: the kernels' host `sig` argument
  const double *sig = nullptr;
  // slice norms s_b(x_p) = sum_i w_bi x_pi^2 of every point, norms[b ldn + p]
  // (launch_slice_norms: b < B the kernel weights, b = B the Matern
  // gradient's last-slice weights); null: each pair tile computes its own
  const double *norms = nullptr;
  int64_t ldn = 0;
};

// Row-side / column-side operand of a pair kernel (row-major, padded).
struct PairSide {
  const double *X;   // nrows x PM
  const double *Z;   // nrows x ZS   (basis columns 1..B-1)
  const double *LZ;  // nrows x ZS   log|z| (SE only; may be null for Matern)
  int64_t n;         // valid rows
  // slice masks of the 64-point blocks (ace_zero_pattern_order; the fused
  // model's training side only): bit b - 1 of mask[k] is clear when z_b is
  // exactly zero on every point of block k, so a pair tile whose row or
  // column block has it clear skips slice b.  Null: every slice
  // of every tile runs.  Read by the MFMA assembly and gradient tiles alone.
  const uint32_t *mask = nullptr;
};

// ACE_ZSKIP for a model of n points: 2 the fused model groups its points by
// zero pattern and the pair tiles skip all-zero slices, 1 skip only (given
// order), 0 neither.  Unset: 2 above n = 8192, else 1 -- the reorder changes
// rounding, and up to that size the model's inverse stays bit-identical to
// the handle path's (which keeps the given order), as
// tests/test_r6_handles_gpu.py holds it.
int zskip_mode(int64_t n);

// ---- assembly --------------------------------------------------------------
// The ABI's kernel matrices (the fused model's assembly is
// launch_assembly_mm below):
// mode 1: symmetric output -- full n x n Kfull (ld = n) + optional cube.
// mode 2: cross output -- n1 x n2 Kfull + optional cube.
// b0 / b1 (no cube): sum only slices [b0, b1) -- the marginal kernels of
// prediction (src/pred_cpp.cpp:55-67); b1 < 0 means B.
hipError_t launch_assembly(int mode, int kind, int PM, PairSide rows, PairSide cols, int B, int ZS,
                           TabView tab, double *out, int64_t ld, double *cube, hipStream_t st,
                           int b0 = 0, int b1 = -1);
// out[r] = sum over b in [b0, b1) of K_b(r, r) (symmetric kernel diagonal)
hipError_t launch_kdiag(int kind, PairSide S, int ZS, TabView tab, int b0, int b1, double *out,
                        hipStream_t st);

// The fused model's assembly (ace_pairs_mm.hip): lower 64-tiles of the
// npad x npad block of A (ld), value K + sig on the diagonal, identity on
// padding rows / columns; kcopy, if non-null, receives the lower Kfull (same
// ld).  tiles: a rank's own lower tiles (ntiles of them, G ranks).
// part (without a tile list): 0 all tiles, 1 the first sweep group's panels'
// columns, 2 the rest -- 1 then 2 lets the sweep's first group of pivot
// chains and lookahead crosses run while part 2 runs; 3 part 2's diagonal
// tiles alone (beside launch_assembly_persist).
hipError_t launch_assembly_mm(int kind, int PM, PairSide S, int64_t npad, int B, int ZS,
                              TabView tab, double sig, double *out, int64_t ld,
                              double *kcopy, hipStream_t st, const Tile *tiles,
                              int64_t ntiles, int G, int part = 0);
// the assembly's second part (part 2 above) as a persistent work queue
// that leaves `reserve` CU ids of shader engine 0 of every XCD free (queue:
// two device ints, reset here on the stream)
hipError_t launch_assembly_persist(int kind, int PM, PairSide S, int64_t npad, int B, int ZS,
                                   TabView tab, double sig, double *out, int64_t ld,
                                   hipStream_t st, int *queue, int reserve, int fill = 0);
// workgroup slots of one CU for the persistent assembly (0 if unknown)
int assembly_persist_per_cu(int kind, int PM, int B);
// mode 2 without a cube on the MFMA r2 expansion (k_cross_mm): R.n x C.n, ld
hipError_t launch_cross_mm(int kind, int PM, PairSide R, PairSide C, int B, int ZS, TabView tab,
                           int b0, int b1, double *out, int64_t ld, hipStream_t st);
// Per-slice cross kernels without the row side's basis factor
// (k_cross_slices_mm): slice b of row r at out[(r + R.n b) + c ld], b < B;
// each element as launch_cross_mm gives it for slices [b, b + 1) and a row
// side of ones.  R.Z / R.LZ are not read.
hipError_t launch_cross_slices_mm(int kind, int PM, PairSide R, PairSide C, int B, int ZS,
                                  TabView tab, double *out, int64_t ld, hipStream_t st);
// Grouped test-kernel sums (k_group_mm): R (S.n x G, ld S.n) = Km E for the
// marginal kernel Km of slices [b0, b1) on the points S and the indicator
// E[c][h] = (label[c] == h), labels in [-1, G), 1 <= G <= 64; Km is never
// stored.  part: group_sums_parts(S.n) * S.n * G doubles of partial sums,
// reduced in a fixed order (bitwise reproducible).
int group_sums_parts(int64_t n);
hipError_t launch_group_sums(int kind, int PM, PairSide S, int B, int ZS, TabView tab, int b0,
                             int b1, const int *label, int G, double *part, double *R,
                             hipStream_t st);
// Per-slice grouped sums over two point sets (k_group_slices_mm): out (R.n x
// (G B), ld R.n), column block b = K_b(R, C) E for every slice b < B, with
// K_b(r, c) = k_b(x_r, x_c) beta_b(z_r) -- the row side's basis factor (1 for
// slice 0), none on the column side, whose Z / LZ are not read -- and E the
// indicator of the C.n labels in [-1, G), 1 <= G <= 64.  part:
// group_slices_parts(R.n, C.n) * R.n * G * B doubles of partial sums, reduced
// in a fixed order (bitwise reproducible, whatever ACE_GROUP_SLICES).
int group_slices_parts(int64_t nrows, int64_t ncols);
hipError_t launch_group_slices(int kind, int PM, PairSide R, PairSide C, int B, int ZS,
                               TabView tab, const int *label, int G, double *part, double *out,
                               hipStream_t st);
hipError_t launch_grad_mm(int kind, int PM, PairSide S, int B, int ZS, TabView tab,
                          const double *A, int64_t ld, double sA, const double *alpha,
                          double *gpart, hipStream_t st, const Tile *tiles, int64_t ntiles, int G,
                          int64_t ndiag);

// ---- gradient --------------------------------------------------------------
// T = sA * A[r,c] - alpha_r alpha_c over the lower 64x64 tiles of [0,n)
// (grad_ntiles(n) of them).
// gpart: tile-major partial sums, one contiguous row of grad_part_cols(PM, B)
//        doubles per tile: [b*(PM+1) + i] (i < PM: length-scale sums,
//        i == PM: lambda sums), then [B*(PM+1)] the trace of T.  Each tile's
//        workgroup writes one contiguous run (launch_tile_sums reduces).
// cube (if non-null, ld n): up to PM = 48 K_b is read from it (k_grad);
// without one, or above, the MFMA kernel recomputes K_b (launch_grad_mm).
// tiles: the rank's list; ndiag >= 0 says its first ndiag entries are the
// diagonal tiles (lets the MFMA kernel run them separately).
__host__ __device__ constexpr int grad_part_cols(int PM, int B) { return B * (PM + 1) + 1; }
hipError_t launch_grad(int kind, int PM, PairSide side, int B, int ZS,
                       TabView tab, const double *A, int64_t ld, double sA,
                       const double *alpha, const double *cube, double *gpart, hipStream_t st,
                       const Tile *tiles = nullptr, int64_t ntiles = 0, int G = 1,
                       int64_t ndiag = -1);
int64_t grad_ntiles(int64_t n);
// super-block size of the fused model's XCD-dealt gradient tile order (0:
// row-major grid); ACE_GRAD_ORDER=S overrides (A/B switch)
int grad_order_block();
// out[j] = sum_t part[t * ncols + j], j < ncols (deterministic order); work
// needs tile_sums_work(ncols) doubles.
hipError_t launch_tile_sums(const double *part, int64_t ntiles, int ncols, double *work,
                            double *out, hipStream_t st);
int64_t tile_sums_work(int ncols);

// ---- sweep -----------------------------------------------------------------
// doubles of the SW buffer: SW[2] (SUB x SUB, ping-pong by sub-step), then
// k_panel_split's three NB x SUB chunk buffers
constexpr int64_t SW_DOUBLES = 2 * (int64_t)SUB * SUB + 3 * (int64_t)NB * SUB;
struct SweepBufs {
  double *A;      // Naug x Naug, col-major, ld = Naug, lower triangle used
  int64_t ld;     // Naug
  int64_t npad;   // multiple of NB
  double *P[8];   // Naug x NB : -panel (negated copy), slot k % 2Z (one-step schedule: k & 1)
  double *W[8];   // Naug x NB : panel being swept, same slots; [2] .. null unless used
  int Z = 2;      // steps per bulk launch (sweep_group_n()); gorder / htiles follow it
  double *SW;     // SW_DOUBLES: 2 SUB x SUB sub-pivot inverses + split-panel chunks
  double *S[2];   // SUB x NB col-major: pivot rows before their sub-sweep (ping-pong)
  double *piv;    // npad pivots
  int *flag;      // set to 1 on a non-positive / non-finite pivot
  const Tile *order = nullptr;  // k_update tile order (xcd_update_order), or row-major
  int64_t norder = 0;
  // the one-step schedule's lookahead cross (cross_update_tiles): device list
  // of every step's cross tiles, host offsets (steps + 1)
  const Tile *xtiles = nullptr;
  const int64_t *xoff = nullptr;
  const Tile *gorder = nullptr;  // per-group bulk orders (pair_bulk_orders), glen each
  const Tile *htiles = nullptr;  // group_head_tiles lists (run_sweep_heads), offsets hoff
  const int64_t *hoff = nullptr;
  int64_t glen = 0;
  // small n: the bulk work queues and launch counters (bq_layout) and the CUs
  // per shader engine the bulk launches leave to the chains
  int *bq = nullptr;
  int breserve = 0;
};
// CUs per shader engine a small-n bulk launch leaves to the panel chains:
// ACE_BULK_RESERVE (0 .. 2) overrides; default 1 up to n = ACE_BULK_RESERVE_N,
// none above (there the bulk launches are the critical path)
int bulk_reserve(int64_t naug);
// small n: a group's first head launch before the rest of its lookahead
// (ACE_QFIRST overrides)
bool q_first(int64_t naug);
// Several sweep steps per bulk update launch (run_sweep_heads, default);
// ACE_PAIR=0 selects the one-step reference schedule.
bool pair_steps();
// Steps per bulk launch: ACE_GROUP = 2 .. 4 (default 4); sweep_group_n: for a
// model of naug rows (3 at small n unless ACE_GROUP is set)
int sweep_group();
int sweep_group_n(int64_t naug);
// super-block size S of the update tile orders (xcd_update_order; 0: row-major
// grid); ACE_UPD_ORDER=S overrides (diagnostic A/B switch)
int update_order_block();
// Lookahead streams and events of one sweep.  side: the panel chains (one-step
// schedule) / the head path; side2: the tail path; either may alias the main
// stream (ACE_STREAMS).  ev: the events SweepEvents{steps, Z} names (SweepWork::ensure).
struct SweepSync {
  hipStream_t side;
  hipStream_t side2 = nullptr;
  hipEvent_t *ev;
  int nev;
  bool ready_recorded = false;  // caller already recorded SweepEvents::ready()
  // caller recorded SweepEvents::tail_after() on the main stream after the
  // whole assembly: the first group's tail path waits for it when the
  // assembly's second part leaves CUs to the head path (ACE_ASM_PERSIST);
  // false: it waits for ready()
  bool tail_after_recorded = false;
  // called on side2 after group 0's tail path, before its completion event
  // (ACE_ASM_FILL: the persistent assembly's filler launch)
  hipError_t (*fill)(void *, hipStream_t) = nullptr;
  bool tail_split = false;  // group 0's tail path after its whole head path
  void *fill_arg = nullptr;
};
// Optional timing of the dominant update launches (k_update<false>): event
// pairs in ev, executed GEMM flops per timed launch in flops[].
struct SweepTiming {
  hipEvent_t *ev;
  int nev;
  int *used;
  double *flops;
};
// Runs every step; A's K block ends holding -A^-1 (lower), the AUG rows hold
// (A^-1 R)^T and the corner -R^T A^-1 R.
hipError_t run_sweep(const SweepBufs &b, hipStream_t st, const SweepSync *sync,
                     const SweepTiming *timing);

// ---- sharded sweep (one rank's view; ace_shard.cpp drives the steps) --------
// Step k on rank r:  pack -> [exchange: broadcast `low` from rank k%G,
// all-gather recv slot r -> recv] -> unpack + pivot chain (panel k on every
// rank, the chain run redundantly, W for the rows r consumes) -> updates.
// The one-step schedule (ACE_PAIR=0, or one step): shard_pack, one exchange,
// shard_unpack_chain, shard_update_cross / shard_update_main per step.  The
// head schedule (default): shard_update_group launches of Z steps that also
// pack the next panel, the exchange and the unpack split into the group's
// head rows and the rest (shard_*_part), shard_chain and shard_pgemm.
struct ShardSweep {
  double *A;          // local column blocks, naug x (nloc * NB), ld = naug
  int64_t ld;         // naug
  int64_t npad;
  int G, r;
  double *P[8], *W[8];  // naug x NB: Pn = -panel (all rows), W (own rows); slot k % (2 Z)
  double *SW;
  double *S[2];
  double *piv;        // npad pivots (every rank records all of them)
  int *flag;
  double *low;        // (naug - k0) x NB broadcast block
  double *recv;       // G x shard_row_slots(k, G) x NB x NB; slot r holds the own
                      // row pieces (the in-place all-gather operand)
  const Tile *tiles;  // own 128-tiles (row-major lower), device
  int64_t ntiles;
};
hipError_t shard_pack(const ShardSweep &b, int k, hipStream_t st);
hipError_t shard_unpack_chain(const ShardSweep &b, int k, int buf, hipStream_t st);
// cross tiles of block k+1 with panel k (buffer buf)
hipError_t shard_update_cross(const ShardSweep &b, int k, int buf, hipStream_t st);
// every own tile except the cross of block kx (kx < 0: none)
hipError_t shard_update_main(const ShardSweep &b, int k, int buf, int kx, hipStream_t st);
// npan steps from block kb in one launch (k_update_multi<true>; one panel:
// k_update), panels in slots (kb + j) % nslot, skipping blocks [kx0, kx1),
// on a tile list; kpack >= 0: the launch also writes the exchange buffers of
// step kpack (what shard_pack(kpack) would copy; G > 1) and the rank's own
// rows of panel kpack (slot kpack % nslot)
hipError_t shard_update_group(const ShardSweep &b, int kb, int npan, int nslot, int kx0, int kx1,
                              const Tile *tiles, int64_t nt, hipStream_t st, int kpack = -1,
                              double *lowp = nullptr, int64_t lr0 = 0, int64_t hh = -1);
// the head schedule's pieces (run_sweep_sharded_heads): a row range of the
// owner's column block (+ row pieces) into an exchange buffer; a row range of
// panel k from one; the pivot sub-steps alone; the head or tail panel GEMM
hipError_t shard_pack_part(const ShardSweep &b, int k, int64_t i_lo, int64_t i_hi, double *low,
                           int64_t lr0, int64_t hh, bool rows, hipStream_t st);
hipError_t shard_unpack_part(const ShardSweep &b, int k, int buf, int64_t i_lo, int64_t i_hi,
                             const double *low, int64_t lr0, int64_t hh, bool own_done,
                             hipStream_t st);
hipError_t shard_chain(const ShardSweep &b, int k, int buf, hipStream_t st);
hipError_t shard_pgemm(const ShardSweep &b, int k, int buf, int rt_lo, int rt_hi, bool head,
                       hipStream_t st);

// ---- small helpers -----------------------------------------------------------
// AUG rows of columns j < n: row 0 = y (zeros if y is null), row 1 = 1
// z0[0..n0) and z1[0..n1) (device ints, may be null) are zeroed by the same
// launch: the evaluation's flag and queue resets without fill launches
hipError_t launch_aug_init(double *A, int64_t ld, int64_t npad, int64_t n,
                           const double *y, hipStream_t st, int G = 1, int rank = 0,
                           int *z0 = nullptr, int n0 = 0, int *z1 = nullptr, int n1 = 0);
// out[0] = sum_j y_j (A^-1 1)_j (AUG row 1), out[1] = 1^T A^-1 1 (corner)
hipError_t launch_aug_dot(const double *A, int64_t ld, int64_t npad, int64_t n, const double *y,
                          double *out, hipStream_t st);
// sharded: vec = [u | v | yKy, yK1, 1K1] of the rank's own columns (zeros elsewhere)
hipError_t launch_aug_extract(const double *A, int64_t ld, int64_t npad, int G,
                              int rank, double *vec, hipStream_t st);
hipError_t launch_alpha_from_vec(const double *vec, int64_t npad, int64_t n,
                                 double theta1, int use_mu_solution, double *alpha,
                                 double *scal, hipStream_t st);
hipError_t launch_add(const double *x, double *y, int64_t count, hipStream_t st);
// alpha = u - mu_eff * v, u/v read from A's AUG rows; mu_eff = theta1 (or
// *theta1p, a device scalar, when given), or 0.5*yK1/1K1 when
// use_mu_solution; writes scal[0..2] = {yKy, yK1, 1K1}, scal[3] =
// mu_solution, scal[4] = mu_eff.
hipError_t launch_alpha_from_aug(const double *A, int64_t ld, int64_t npad,
                                 int64_t n, double theta1, int use_mu_solution,
                                 double *alpha, double *scal, hipStream_t st,
                                 const double *theta1p = nullptr);
hipError_t launch_colsum(const double *in, int64_t nrows, int ncols,
                         double *out, hipStream_t st);
// sums[0] = sum (ybar - s)^2, sums[1] = sum y*alpha, sums[2] = sum alpha,
// sums[3] = sum log(piv[0..npiv)), with ybar = y - *mu (device scalar).
// s == nullptr: ybar - s = sig * alpha (fused model, A = Kfull + sig I);
// sigp (device scalar) replaces sig when given; flag (device int) is copied
// to sums[4] when given, so that one read-back carries it.
hipError_t launch_final_sums(const double *y, const double *mu, const double *alpha,
                             const double *s, double sig, int64_t n, const double *piv,
                             int64_t npiv, double *sums, hipStream_t st,
                             const double *sigp = nullptr, const int *flag = nullptr);
// ---- device-fused training loop (ace_train.hip) -----------------------------
// theta tables of make_tab (ace_common.h) from a device theta, plus
// tab[2 B PM + B] = exp(theta[0]) (TabView::sig)
// the TabView::norms table: NS = B (+ 1 for the Matern gradient) rows of np
// points (ld np) from X (np x PM row-major), with mm_stage's arithmetic
hipError_t launch_slice_norms(const double *X, int PM, int64_t np, int B, int NS,
                              const double *wk, const double *wlast, double *norms,
                              hipStream_t st);
hipError_t launch_make_tab(const double *theta, int B, int p, int PM, double *tab,
                           hipStream_t st);
struct TrainCfg {
  OptCfg opt;
  int P, B, p, PM, kind;
  int64_t n;
  double std_y;
};
// One iteration's host-side tail of ace_model_train on the device (one
// workgroup): compose_grad + stats of para_update, norm clip, optimizer step,
// the mu overwrite and the convergence test.  st = [theta | m1 | m2 | g |
// prev] (5 P; prev = the theta the iteration's evaluation ran at), hist = the
// stats matrix (2 x (maxiter + 2)), ctl = {last iteration done, stop: 0
// running / 1 converged / 2 non-finite gradient}.  Once ctl[1] is set, later
// launches change nothing.
hipError_t launch_train_step(const TrainCfg &c, int it, const double *gsum, const double *sums,
                             const double *scal, const int *flag, double *st, double *hist,
                             int *ctl, hipStream_t stream);
// y = M x for M (m x k, col-major ld) ; y = M^T x
hipError_t launch_gemv(const double *M, int64_t ld, int64_t m, int64_t k,
                       const double *x, double *y, hipStream_t st);
hipError_t launch_gemv_t(const double *M, int64_t ld, int64_t m, int64_t k,
                         const double *x, double *y, hipStream_t st);
// C (m x n) = A (m x k) * B (k x n), col-major, fp64 MFMA.
hipError_t launch_gemm_nn(int64_t m, int64_t n, int64_t k, const double *A,
                          int64_t lda, const double *B, int64_t ldb, double *C,
                          int64_t ldc, hipStream_t st);
// C (m x n) = A^T B (+ C when accumulate) for A (k x m) and B (k x n),
// col-major, fp64 MFMA, k split over workgroups and summed in a fixed order;
// work: gemm_tn_work(m, n, k) doubles.
int64_t gemm_tn_work(int64_t m, int64_t n, int64_t k);
hipError_t launch_gemm_tn(int64_t m, int64_t n, int64_t k, const double *A, int64_t lda,
                          const double *B, int64_t ldb, double *C, int64_t ldc, bool accumulate,
                          double *work, hipStream_t st);
// E (nx x G, ld nx): E[i][g] = (label[i] == g)
hipError_t launch_label_matrix(const int *label, int64_t nx, int G, double *E, hipStream_t st);
// Copies scale * A (lower) into a full symmetric n x n matrix (ld_out).
hipError_t launch_sym_from_lower(const double *A, int64_t ld, int64_t n,
                                 double scale, double *out, int64_t ld_out,
                                 hipStream_t st);
// Same from block-cyclic column storage: global column c of A lives in
// slot (c / NB) % G (slot_elems doubles each) at local column lcol(c, G).
hipError_t launch_sym_from_cyclic(const double *A, int64_t ld, int64_t n, int G,
                                  int64_t slot_elems, double scale, double *out,
                                  int64_t ld_out, hipStream_t st);
// dst[0:npad, 0:npad] (ld_dst) = src (n x n, ld n) + diag I, identity padding
hipError_t launch_prepare_A(const double *src, int64_t n, double diag,
                            double *dst, int64_t ld_dst, int64_t npad,
                            hipStream_t st);
hipError_t launch_fill(double *p, int64_t count, double v, hipStream_t st);
// Sum over b>=1 of cube slices (or slice 0 when B == 1): out m x n.
hipError_t launch_marginal_sum(const double *cube, int64_t m, int64_t n,
                               int B, double *out, hipStream_t st);
// Prediction rows: for r < nx: a = sum_c T[r,c] w[c]; q = sum_c T[r,c] K[r,c]
hipError_t launch_pred_rows(const double *T, const double *K, int64_t ld,
                            int64_t nx, int64_t nX, const double *w,
                            double *a, double *q, hipStream_t st);
// q[j] = w_j^T M w_j for three weight vectors packed in W (n x 3)
hipError_t launch_quad3(const double *M, int64_t ld, int64_t n,
                        const double *W, double *q, hipStream_t st);
hipError_t launch_log_abs(const double *Z, double *LZ, int64_t count,
                          hipStream_t st);

// ---- products with the resident inverse (ace_symm.hip) -----------------------
// out (n x k, ldo) = scale * S V, S = symmetric matrix with lower triangle in
// A (ld; block-cyclic columns for G > 1: only the rank's stored entries are
// used, so the ranks' outputs sum to S V).  vt: V[p][c] = V[c + p ldv].
hipError_t launch_symm(const double *A, int64_t ld, int64_t n, int G, int rank, const double *V,
                       int64_t ldv, bool vt, int64_t k, double scale, double *out, int64_t ldo,
                       hipStream_t st);
// a[c] = sum_q T[q + c ldt] w[q], d[c] = sum_q T[q + c ldt] K[c + q ldk], c < nx
hipError_t launch_pred_cols(const double *T, int64_t ldt, const double *K, int64_t ldk, int64_t n,
                            int64_t nx, const double *w, double *a, double *d, hipStream_t st);
// single GPU: out (n x k, ldo) = scale * L V^T, L the strictly lower part of
// the stored matrix, V given as k x n (V[p][c] = V[c + p ldv])
hipError_t launch_trmm_lower(const double *A, int64_t ld, int64_t n, const double *V, int64_t ldv,
                             int64_t k, double scale, double *out, int64_t ldo, hipStream_t st);
// a[c] = sum_q K[c][q] s[q], d[c] = sum_q K[c][q] (2 Y[q][c] + D[q] K[c][q])
hipError_t launch_pred_cols_tri(const double *Y, int64_t ldt, const double *K, int64_t ldk,
                                int64_t n, int64_t nx, const double *sv, const double *D, double *a,
                                double *d, hipStream_t st);
// Coefficient Gram sums of a chunk of ncx test points (k_coef_gram): Kc the
// (ncx B) x n per-slice cross kernels (row c + ncx b, ld ldk), W the n x
// (ncx B) product with the inverse (ld ldw): Y = L Kc^T with D, vec = S w
// (tri), or T' = S Kc^T with vec = w.  res (ncx B (B + 1)):
// res[c + ncx (b + B b')] = (Kc_c S Kc_c^T)[b][b'], exactly symmetric, then
// res[ncx B B + c + ncx b] = Kc_c S w.  part: coef_gram_work(n, ncx, B)
// doubles.  The training points are split by n alone and the partials added
// in a fixed order: bitwise reproducible, whatever the chunking.
int64_t coef_gram_work(int64_t n, int64_t ncx, int B);
hipError_t launch_coef_gram(bool tri, const double *Kc, int64_t ldk, const double *W, int64_t ldw,
                            int64_t n, int64_t ncx, int B, const double *vec, const double *D,
                            double *part, double *res, hipStream_t st);
// D[q] = scale * A[q + q ld], q < n
hipError_t launch_diag_scaled(const double *A, int64_t ld, int64_t n, double scale, double *D,
                              hipStream_t st);
// w = y - mu
hipError_t launch_center(const double *y, int64_t n, double mu, double *w, hipStream_t st);

// ---- joint posterior at the test points (ace_joint.hip) ----------------------
// C (nx x nx, ldc) = scale (Kxx - Kx T + noise I) for Kx (nx x n, ldk) and
// T (n x nx, ldt): lower 64-tiles on the fp64 MFMA, mirrored, so C is exactly
// symmetric; Kxx is read at r >= c and on the diagonal tiles
hipError_t launch_post_cov(const double *Kx, int64_t ldk, const double *T, int64_t ldt, int64_t n,
                           const double *Kxx, int64_t ldx, int64_t nx, double noise, double scale,
                           double *C, int64_t ldc, hipStream_t st);
// L (n x n, ldl) = the lower Cholesky factor of tril(C) + jitter I, zeros
// above the diagonal; blocked right-looking, NB = 64, no host sync.  *flag
// (device int, reset here): 0, or the 1-based index of the first pivot that
// is <= 0 or not finite -- L is then unfinished.
hipError_t launch_potrf_lower(const double *C, int64_t ldc, int64_t n, double jitter, double *L,
                              int64_t ldl, int *flag, hipStream_t st);
// D (nx x S, ld nx) = m 1^T + L xi for xi (nx x S, ld nx)
hipError_t launch_draws(const double *L, int64_t ldl, int64_t nx, const double *xi, int64_t S,
                        const double *m, double *D, hipStream_t st);

}  // namespace ace
