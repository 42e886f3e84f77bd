// ace_sweep_plan.h -- the sweep's host-only planning: blocking, tile lists,
// the work of a launch on a tile, the named lookahead events, the small-n
// rules, for the single-GPU sweep and the sharded one (ace_shard.cpp).  Pure
// functions of (naug or n, steps, Z, S, G, r) and no HIP header, so
// tests/sweep_plan_check.cpp checks them with a host compiler alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

namespace ace {

// Sweep (Gauss-Jordan SPD inversion) blocking; see DESIGN.md §3.
#ifndef ACE_NB
#define ACE_NB 256
#endif
constexpr int NB = ACE_NB;  // outer pivot block = panel width
constexpr int SUB = 64;    // inner pivot block, eliminated inside LDS
constexpr int UT = 128;    // update tile (MFMA f64 16x16x4, 4 waves x 64x64)
constexpr int AUG = 128;   // augmented right-hand-side rows (y, 1) appended to A
constexpr int AT = 64;     // assembly / gradient pair tile
// GEMM flops of one full update tile against one panel
constexpr double TILE_FLOPS = 2.0 * UT * UT * NB;

// Column sharding (ace_internal.h): block j of NB columns lives on rank j % G.
// The one function here that the kernels call too.
#ifdef __HIPCC__
__host__ __device__
#endif
inline __attribute__((always_inline)) bool owns_col(int64_t c, int G, int r) {
  return G == 1 || (c / NB) % G == r;
}
// columns of rank r's local array: its column blocks, the AUG block included
inline int64_t ncols_local(int64_t naug, int G, int r) { return ((naug + NB - 1) / NB - r + G - 1) / G * NB; }
// NB x NB row pieces A[k, j < k] a rank contributes to step k's all-gather
// (ShardSweep::recv: G slots of this many)
inline int shard_row_slots(int k, int G) { return (k + G - 1) / G; }

// A pair / update tile (row tile I, column tile J) of a per-rank tile list.
// Entries with I < 0 are padding of an XCD-dealt order.
struct Tile {
  int I, J;
};

// ---- the work of one update launch on one tile ------------------------------
// I or J in the NB blocks [k0, k1) (k0 < 0: no blocks): the cross a launch skips
inline bool in_blocks(const Tile &t, int k0, int k1) {
  constexpr int KT = NB / UT;
  return k0 >= 0 && ((t.I >= k0 * KT && t.I < k1 * KT) || (t.J >= k0 * KT && t.J < k1 * KT));
}
// k_update_multi's rule (k_update's with npan = 1), stated here once: a launch
// of npan panels from row tile ta0 (block ta0 / KT) that skips the cross of
// blocks [kx0, kx1).  A tile in group block jm starts from W_jm and takes the
// later panels; any other tile takes every panel.  Returns the first group
// panel the tile takes: 0 for all of them, npan for none (a tile of the last
// group block is a copy; a tile of the skipped cross is not touched).
inline int tile_first_panel(const Tile &t, int64_t ta0, int npan, int kx0, int kx1) {
  constexpr int KT = NB / UT;
  if (in_blocks(t, kx0, kx1)) return npan;
  const int64_t di = t.I - ta0, dj = t.J - ta0;
  const int bi = (di >= 0 && di < npan * KT) ? (int)(di / KT) : -1;
  const int bj = (dj >= 0 && dj < npan * KT) ? (int)(dj / KT) : -1;
  return std::max(bi, bj) + 1;
}
// a tile of the AUG row block (the last of nT) computes 16 of its 128 rows
inline double tile_rows(const Tile &t, int64_t nT) { return t.I == nT - 1 ? 16.0 / UT : 1.0; }
// GEMM tiles of that launch on one tile, in units of one full tile x NB
inline double tile_work(const Tile &t, int64_t nT, int64_t ta0, int npan, int kx0, int kx1) {
  return tile_rows(t, nT) * (npan - tile_first_panel(t, ta0, npan, kx0, kx1));
}
// ... on a tile list
double tile_list_work(const std::vector<Tile> &tl, int64_t nT, int64_t ta0, int npan, int kx0,
                      int kx1);
// ... of one k_update launch of step k0 / NB over every lower tile outside the
// cross of block kx (look: inside it)
double update_gemm_tiles(int64_t naug, int64_t k0, int kx, bool look);
// ... of one launch of npan steps from block ka0 / NB over every lower tile
double update_gemm_tiles_group(int64_t naug, int64_t ka0, int npan, int kx0, int kx1);
// every GEMM flop of one sweep, whatever the schedule: each step's update of
// every lower tile outside its block (bulk + lookahead crosses) and its panel
// GEMM W_i = Pn_i W_kk
double sweep_flops(int64_t naug, int64_t npad);

// ---- tile lists ---------------------------------------------------------------
// own lower tiles of size T over [0, ntile*T) in row-major order
std::vector<Tile> own_tiles(int64_t ntile, int T, int G, int r);
// k_update tile order: the tiles of `tl` grouped into S x S super-blocks of
// 128-tiles that are dealt whole to the 8 XCDs; list index b runs on XCD
// b % 8 (dispatch is round-robin).  Entries with I < 0 are padding.
std::vector<Tile> xcd_update_order(const std::vector<Tile> &tl, int S,
                                   const std::function<double(const Tile &)> &cost = nullptr);
// The lower 128-tiles with I or J in block k+1, for k = 0 .. steps-2,
// concatenated (each step's list dealt to the XCDs in S x S super-blocks like
// the bulk order, S = 0: row-major); off[k] .. off[k+1] is step k's range.
std::vector<Tile> cross_update_tiles(int64_t naug, int steps, int S, std::vector<int64_t> &off);
// per group of Z steps, the bulk order with each XCD's cheap tiles last:
// ngroups lists of *len entries (sharded: rank r's own tiles of G)
std::vector<Tile> pair_bulk_orders(int64_t naug, int steps, int S, int64_t *len, int G, int r,
                                   int Z);
// Head / tail lists of the group schedule's lookahead (run_sweep_heads):
// 2Z lists per group at off[G 2Z + m] (see ace_sweep_plan.cpp).
std::vector<Tile> group_head_tiles(int64_t naug, int steps, int Z, int S,
                                   std::vector<int64_t> &off);
// ... restricted to rank r's own tiles (column block owned), in the same
// order and without the padding: the sharded head schedule's lists
std::vector<Tile> rank_head_tiles(int64_t naug, int steps, int Z, int S, int G, int r,
                                  std::vector<int64_t> &off);
// Rank r's assembly list: its lower AT-tiles of [0, npad), the first group's
// panels' columns (J < Z NB / AT) first, *nfirst of them (the sweep's first
// lookahead runs under the rest of the assembly)
std::vector<Tile> rank_asm_tiles(int64_t npad, int Z, int G, int r, int64_t *nfirst);
// Rank r's gradient list: its lower AT-tiles of [0, n), the *ndiag diagonal
// ones first (the gradient kernel runs them separately)
std::vector<Tile> rank_grad_tiles(int64_t n, int G, int r, int64_t *ndiag);
// The single-GPU gradient order: the *ndiag diagonal AT-tiles of [0, n), then
// the strictly lower ones dealt to the XCDs in S x S super-blocks.  mask (one
// word per AT-block, PairSide::mask; may be null): a tile's cost is its
// active slices (grouped points: up to B times apart), and each XCD's cheap
// tiles end its share of the launch.
std::vector<Tile> grad_tile_order(int64_t n, int S, const uint32_t *mask, int64_t *ndiag);

// ---- the pair kernels' work of a timed evaluation -----------------------------
// point pairs of a list of lower AT-tiles, every tile counted whole
double tile_list_pairs(const std::vector<Tile> &tl);
// algorithmic flops of the assembly and of the gradient over
// `pairs` point pairs with B components and p covariates
inline double asm_flops(double pairs, double B, double p) { return pairs * B * (3 * p + 3); }
inline double grad_flops(double pairs, double B, double p, bool matern) {
  return pairs * (4 * B * p + 2 * p) + (matern ? pairs * B * p : 0);
}

// ---- the lookahead events of one sweep (SweepSync::ev) ------------------------
// One name per event; every name is an index of its own below count() (the
// schedules' correctness rests on that; events carry no state between sweeps).
struct SweepEvents {
  int steps, Z;
  int groups() const { return (steps + Z - 1) / Z; }
  int ready() const { return 0; }       // the sweep's inputs (main stream)
  int tail_after() const { return 1; }  // the whole assembly (assemble_and_sweep)
  int filler() const { return 2; }      // group 0's tail path + the assembly's filler launch
  // bulk launch g, for g >= -1 (-1: the main stream's work before the sweep)
  int bulk_done(int g) const { return 4 + g; }
  // group g: its head path (side), its tail path (side2, after the head
  // path), its Q launch, its last T launch (small n: before the last tail GEMM)
  int head_done(int g) const { return group0() + 4 * g; }
  int tail_done(int g) const { return group0() + 4 * g + 1; }
  int q_done(int g) const { return group0() + 4 * g + 2; }
  int last_tail(int g) const { return group0() + 4 * g + 3; }
  // panel k: its pivot sub-steps, its head GEMM
  int substeps_done(int k) const { return panel0() + 2 * k; }
  int head_gemm_done(int k) const { return panel0() + 2 * k + 1; }
  // the one-step schedule: panel k swept (side), the main stream's work
  // before bulk k (bulk k - 1 and what preceded the sweep)
  int step_panel_done(int k) const { return step0() + 2 * k; }
  int step_bulk_before(int k) const { return step0() + 2 * k + 1; }
  // the sharded head schedule: the main stream before bulk g (bulk g - 1 and
  // group g's head and tail paths done)
  int bulk_before(int g) const { return before0() + g; }
  int count() const { return before0() + groups(); }

 private:
  int group0() const { return 4 + groups(); }
  int panel0() const { return group0() + 4 * groups(); }
  int step0() const { return panel0() + 2 * steps; }
  int before0() const { return step0() + 2 * steps; }
};

// ---- the small-n regime ---------------------------------------------------------
// n up to ACE_BULK_RESERVE_N: the chains, not the bulk launches, are the
// critical path (run_sweep_heads).  The defaults of sweep_group_n,
// bulk_reserve and q_first (ace_internal.h) for a model of naug rows:
#ifndef ACE_BULK_RESERVE_N
#define ACE_BULK_RESERVE_N 8192
#endif
inline bool small_n(int64_t naug) { return naug <= ACE_BULK_RESERVE_N + AUG; }
inline int default_group(int64_t naug) { return small_n(naug) ? 3 : 4; }
inline int default_bulk_reserve(int64_t naug) { return small_n(naug) ? 1 : 0; }
inline bool default_q_first(int64_t naug) { return small_n(naug); }
// SweepBufs::bq for a sweep of `steps` steps in groups of Z: per group a bulk
// work queue of BQ_INTS ints (k_update_multi_r, zeroed per sweep), from fctr
// on two counters per step (k_panel_split4's grid barrier and exits), from
// qctr on one per step (k_update_q4's D_0 pieces).  The counters are zero
// between launches: each launch's last workgroup resets them.
constexpr int BQ_INTS = 2 + 64;
struct BqLayout {
  int64_t fctr, qctr, ints;
};
inline BqLayout bq_layout(int steps, int Z) {
  const int64_t q = (int64_t)((steps + Z - 1) / Z) * BQ_INTS;
  return BqLayout{q, q + 2 * steps, q + 3 * steps};
}

}  // namespace ace
