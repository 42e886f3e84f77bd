// ace_sweep_plan.cpp -- the sweep's tile lists and work counts (host only, no HIP)
#include "ace_sweep_plan.h"

#include <map>

namespace ace {

double tile_list_work(const std::vector<Tile> &tl, int64_t nT, int64_t ta0, int npan, int kx0,
                      int kx1) {
  double cnt = 0.0;
  for (const Tile &t : tl)
    if (t.I >= 0) cnt += tile_work(t, nT, ta0, npan, kx0, kx1);  // (I < 0: padding)
  return cnt;
}

// The same loop over the whole lower triangle, without building a list: the
// timed schedules count between two launches.
double update_gemm_tiles(int64_t naug, int64_t k0, int kx, bool look) {
  const int nT = (int)(naug / UT);
  double cnt = 0.0;
  for (int I = 0; I < nT; ++I)
    for (int J = 0; J <= I; ++J)
      if (const Tile t{I, J}; in_blocks(t, kx, kx + 1) == look) cnt += tile_work(t, nT, k0 / UT, 1, -1, -1);
  return cnt;
}

double update_gemm_tiles_group(int64_t naug, int64_t ka0, int npan, int kx0, int kx1) {
  const int nT = (int)(naug / UT);
  double cnt = 0.0;
  for (int I = 0; I < nT; ++I)
    for (int J = 0; J <= I; ++J) cnt += tile_work(Tile{I, J}, nT, ka0 / UT, npan, kx0, kx1);
  return cnt;
}

double sweep_flops(int64_t naug, int64_t npad) {
  thread_local int64_t cn = -1, cp = -1;
  thread_local double cf = 0.0;
  if (naug == cn && npad == cp) return cf;
  double f = 0.0;
  for (int64_t k0 = 0; k0 < npad; k0 += NB)
    f += update_gemm_tiles(naug, k0, -1, false) * TILE_FLOPS +
         2.0 * (double)(naug - NB) * NB * NB;
  cn = naug;
  cp = npad;
  cf = f;
  return f;
}

// The one-step schedule's lookahead cross on k_update's 128-tiles: -0.2 ms
// per C2 evaluation against the 64-tile k_update_x (same box, 2 rounds: 81.03
// / 81.26 vs 81.25 / 81.49 ms)
std::vector<Tile> cross_update_tiles(int64_t naug, int steps, int S, std::vector<int64_t> &off) {
  const std::vector<Tile> lower = own_tiles(naug / UT, UT, 1, 0);
  std::vector<Tile> all;
  off.assign(1, 0);
  for (int k = 0; k + 1 < steps; ++k) {
    std::vector<Tile> t;
    for (const Tile &x : lower)
      if (in_blocks(x, k + 1, k + 2)) t.push_back(x);
    const std::vector<Tile> o = S > 0 ? xcd_update_order(t, S) : t;
    all.insert(all.end(), o.begin(), o.end());
    off.push_back((int64_t)all.size());
  }
  return all;
}

std::vector<Tile> pair_bulk_orders(int64_t naug, int steps, int S, int64_t *len, int G, int r,
                                   int Z) {
  const int64_t nT = naug / UT;
  constexpr int KT = NB / UT;
  const int ng = (steps + Z - 1) / Z;
  const std::vector<Tile> base = own_tiles(nT, UT, G, r);
  std::vector<Tile> all;
  std::vector<std::vector<Tile>> lists;
  *len = 0;
  for (int g = 0; g < ng; ++g) {
    const int z = std::min(Z, steps - Z * g);
    const int64_t ta0 = (int64_t)Z * g * KT;
    const bool more = g + 1 < ng;
    const int kx0 = more ? Z * (g + 1) : -1, kx1 = more ? std::min(Z * (g + 1) + Z, steps) : -1;
    // the panels the tile runs; a copy costs a little, a skipped tile nothing
    auto cost = [&](const Tile &t) -> double {
      const double w = tile_work(t, nT, ta0, z, kx0, kx1);
      return w > 0.0 ? w : in_blocks(t, kx0, kx1) ? 0.0 : 0.05;
    };
    // each XCD's cheap tiles last: -0.15 ms per C2 evaluation once the side
    // chain is off the critical path (profiles/r02_chain_ab.txt)
    lists.push_back(xcd_update_order(base, std::max(1, S), cost));
    *len = std::max<int64_t>(*len, (int64_t)lists.back().size());
  }
  // one length for every group (padding: whole rows of 8, so the XCD dealing
  // of each list stands)
  for (auto &o : lists) {
    o.resize((size_t)*len, Tile{-1, -1});
    all.insert(all.end(), o.begin(), o.end());
  }
  return all;
}

// Head / tail split of the group schedule's lookahead (run_sweep_heads).
// Group G (blocks [kb, kb + z)), lists at off[G 2Z + m] (m = 0, 1 unused for G = 0):
//   m = 0          Q: the lower tiles with I and J in the group's blocks
//   m = 1          the rest of the group's cross (I or J in the group, not in Q)
//   m = 2 + i      Q_{i+1}: the tiles of Q with J in block kb + i + 1 or later
//                  (panel kb + i is applied to them as soon as it is final), i < z - 1
//   m = z + j      T_j: the tiles with I or J in block kb + j minus the head
//                  H_j = {J in block kb + j, I in blocks [kb + j, kb + z)}, 1 <= j < z
// Every list is XCD-dealt like the cross lists.
std::vector<Tile> group_head_tiles(int64_t naug, int steps, int Z, int S,
                                   std::vector<int64_t> &off) {
  const std::vector<Tile> lower = own_tiles(naug / UT, UT, 1, 0);
  constexpr int KT = NB / UT;
  const int ng = (steps + Z - 1) / Z;
  std::vector<Tile> all;
  off.assign((size_t)ng * 2 * Z + 1, 0);
  for (int G = 0; G < ng; ++G) {
    const int kb = Z * G, z = std::min(Z, steps - kb);
    std::vector<std::vector<Tile>> L((size_t)2 * Z);  // (group 0 uses only m >= 2)
    for (const Tile &t : lower) {
      const int bi = t.I / KT - kb, bj = t.J / KT - kb;  // relative blocks
      const bool ii = bi >= 0 && bi < z, ij = bj >= 0 && bj < z;
      if (ii && ij) {
        L[0].push_back(t);
        for (int i = 0; i + 1 < z; ++i)
          if (bj >= i + 1) L[(size_t)(2 + i)].push_back(t);
      } else if (ii || ij) {
        L[1].push_back(t);
      }
      for (int j = 1; j < z; ++j) {
        if (bi != j && bj != j) continue;
        const bool head = bj == j && bi >= j && bi < z;
        if (!head) L[(size_t)(z + j)].push_back(t);
      }
    }
    for (int m = 0; m < 2 * Z; ++m) {
      const std::vector<Tile> o = S > 0 ? xcd_update_order(L[(size_t)m], S) : L[(size_t)m];
      all.insert(all.end(), o.begin(), o.end());
      off[(size_t)G * 2 * Z + m + 1] = (int64_t)all.size();
    }
  }
  return all;
}

std::vector<Tile> rank_head_tiles(int64_t naug, int steps, int Z, int S, int G, int r,
                                  std::vector<int64_t> &off) {
  std::vector<int64_t> all_off;
  const std::vector<Tile> all = group_head_tiles(naug, steps, Z, S, all_off);
  std::vector<Tile> mine;
  off.assign(all_off.size(), 0);
  for (size_t m = 0; m + 1 < all_off.size(); ++m) {
    for (int64_t i = all_off[m]; i < all_off[m + 1]; ++i)
      if (const Tile &t = all[(size_t)i]; t.I >= 0 && owns_col((int64_t)t.J * UT, G, r)) mine.push_back(t);
    off[m + 1] = (int64_t)mine.size();
  }
  return mine;
}

std::vector<Tile> rank_asm_tiles(int64_t npad, int Z, int G, int r, int64_t *nfirst) {
  std::vector<Tile> t = own_tiles(npad / AT, AT, G, r);
  *nfirst = std::stable_partition(t.begin(), t.end(), [&](const Tile &x) { return x.J < Z * NB / AT; }) - t.begin();
  return t;
}

std::vector<Tile> rank_grad_tiles(int64_t n, int G, int r, int64_t *ndiag) {
  std::vector<Tile> t = own_tiles((n + AT - 1) / AT, AT, G, r);
  *ndiag = std::stable_partition(t.begin(), t.end(), [](const Tile &x) { return x.I == x.J; }) - t.begin();
  return t;
}

std::vector<Tile> grad_tile_order(int64_t n, int S, const uint32_t *mask, int64_t *ndiag) {
  const int64_t ntr = (n + AT - 1) / AT;
  std::vector<Tile> lst, low;
  for (int64_t I = 0; I < ntr; ++I)
    for (int64_t J = 0; J <= I; ++J) (J == I ? lst : low).push_back(Tile{(int)I, (int)J});
  std::function<double(const Tile &)> cost;
  if (mask)
    cost = [mask](const Tile &t) { return 1.0 + __builtin_popcount(mask[t.I] & mask[t.J]); };
  const std::vector<Tile> o = xcd_update_order(low, S, cost);
  lst.insert(lst.end(), o.begin(), o.end());
  *ndiag = ntr;
  return lst;
}

double tile_list_pairs(const std::vector<Tile> &tl) {
  double pairs = 0.0;
  for (const Tile &t : tl)
    if (t.I >= 0) pairs += t.I == t.J ? AT * (AT + 1) / 2 : AT * AT;  // (I < 0: padding)
  return pairs;
}

std::vector<Tile> own_tiles(int64_t ntile, int T, int G, int r) {
  std::vector<Tile> t;
  for (int64_t I = 0; I < ntile; ++I)
    for (int64_t J = 0; J <= I; ++J)
      if (owns_col(J * T, G, r)) t.push_back(Tile{(int)I, (int)J});
  return t;
}

std::vector<Tile> xcd_update_order(const std::vector<Tile> &tl, int S,
                                   const std::function<double(const Tile &)> &cost) {
  // super-blocks (I / S, J / S) in row-major order; each goes whole to the
  // XCD with the fewest tiles so far, so an XCD's in-flight tiles share few
  // row / column panel blocks in its L2 (about -1 % per update launch at C2
  // against every-eighth-tile dealing, profiles/r01_pairs_ab.txt)
  constexpr int X = 8;
  std::vector<std::vector<Tile>> q(X);
  std::map<std::pair<int, int>, std::vector<Tile>> sb;
  for (const Tile &t : tl) sb[{t.I / S, t.J / S}].push_back(t);
  for (auto &kv : sb) {
    int x = 0;
    for (int i = 1; i < X; ++i)
      if (q[i].size() < q[x].size()) x = i;
    q[x].insert(q[x].end(), kv.second.begin(), kv.second.end());
  }
  if (cost)  // each XCD's dearest tiles first: its launch tail is the cheap ones
    for (auto &v : q)
      std::stable_sort(v.begin(), v.end(),
                       [&](const Tile &a, const Tile &b) { return cost(a) > cost(b); });
  size_t len = 0;
  for (auto &v : q) len = std::max(len, v.size());
  std::vector<Tile> out(len * X, Tile{-1, -1});
  for (int x = 0; x < X; ++x)
    for (size_t i = 0; i < q[x].size(); ++i) out[i * X + x] = q[x][i];
  return out;
}

}  // namespace ace
