// Stand-alone check of the sweep's host-only planning (csrc/ace_sweep_plan.*):
// the event names, the tile lists of both schedules on one GPU and sharded
// over ranks, the tile-work rule, the pair kernels' work counts and the
// small-n layout rules.  Built and run by tests/test_sweep_plan_cpu.py
// with a host compiler and AddressSanitizer + UBSan; needs no GPU.
#include <stdio.h>

#include <map>
#include <set>
#include <string>
#include <utility>

#include "ace_sweep_plan.h"

using namespace ace;

static int failures = 0;
#define CHECK(cond, ...)                           \
  do {                                             \
    if (!(cond)) {                                 \
      if (++failures <= 20) {                      \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                       \
        printf("\n");                              \
      }                                            \
    }                                              \
  } while (0)

constexpr int KT = NB / UT;
constexpr int S_DEFAULT = 2;       // update_order_block()'s default
constexpr int S_GRAD_DEFAULT = 4;  // grad_order_block()'s default

// ---- 1. events: every name an index of its own below count() ----------------
static void check_events(int steps, int Z) {
  const SweepEvents E{steps, Z};
  std::multiset<int> seen;
  auto add = [&](int i) {
    CHECK(i >= 0 && i < E.count(), "event %d outside [0, %d) at steps %d Z %d", i, E.count(), steps, Z);
    seen.insert(i);
  };
  add(E.ready());
  add(E.tail_after());
  add(E.filler());
  for (int g = -1; g < E.groups(); ++g) add(E.bulk_done(g));
  for (int g = 0; g < E.groups(); ++g) {
    add(E.head_done(g));
    add(E.tail_done(g));
    add(E.q_done(g));
    add(E.last_tail(g));
    add(E.bulk_before(g));
  }
  for (int k = 0; k < steps; ++k) {
    add(E.substeps_done(k));
    add(E.head_gemm_done(k));
    add(E.step_panel_done(k));
    add(E.step_bulk_before(k));
  }
  for (int i : seen) CHECK(seen.count(i) == 1, "event %d named twice at steps %d Z %d", i, steps, Z);
}

// ---- 2, 3. the launches of a schedule, walked as the host issues them --------
struct Walk {
  int64_t nT;
  int steps;
  std::map<std::pair<int, int>, std::vector<int>> took;  // tile -> times it took panel k
  double work;
  // a launch of npan panels from block kb on a list, skipping blocks [kx0, kx1)
  void launch(const Tile *tl, int64_t n, int kb, int npan, int kx0, int kx1) {
    const std::vector<Tile> v(tl, tl + n);
    for (const Tile &t : v) {
      if (t.I < 0) continue;  // padding
      CHECK(t.J >= 0 && t.J <= t.I && t.I < nT, "tile (%d, %d) outside the lower triangle", t.I, t.J);
      std::vector<int> &c = took[{t.I, t.J}];
      c.resize((size_t)steps, 0);
      for (int j = tile_first_panel(t, (int64_t)kb * KT, npan, kx0, kx1); j < npan; ++j) ++c[(size_t)(kb + j)];
    }
    work += tile_list_work(v, nT, (int64_t)kb * KT, npan, kx0, kx1);
  }
  // every lower tile outside panel k's block row and column took it once, no
  // tile a panel of its own block; the work is the sweep's
  void verify(const char *what, int Z) {
    for (int I = 0; I < nT; ++I)
      for (int J = 0; J <= I; ++J) {
        std::vector<int> &c = took[{I, J}];
        c.resize((size_t)steps, 0);
        for (int k = 0; k < steps; ++k) {
          const int want = in_blocks(Tile{I, J}, k, k + 1) ? 0 : 1;
          CHECK(c[(size_t)k] == want, "%s steps %d Z %d: tile (%d, %d) took panel %d %d times, not %d", what,
                steps, Z, I, J, k, c[(size_t)k], want);
        }
      }
    double all = 0.0;
    for (int k = 0; k < steps; ++k) all += update_gemm_tiles(nT * UT, (int64_t)k * NB, -1, false);
    CHECK(work == all, "%s steps %d Z %d: work %.4f, the sweep's %.4f", what, steps, Z, work, all);
  }
};

static void check_head_schedule(int steps, int Z) {
  const int64_t naug = (int64_t)steps * NB + AUG;
  const int ng = (steps + Z - 1) / Z;
  auto zsize = [&](int g) { return std::min(Z, steps - Z * g); };
  std::vector<int64_t> hoff;
  int64_t glen = 0;
  const std::vector<Tile> h = group_head_tiles(naug, steps, Z, S_DEFAULT, hoff);
  const std::vector<Tile> o = pair_bulk_orders(naug, steps, S_DEFAULT, &glen, 1, 0, Z);
  CHECK((int64_t)hoff.size() == (int64_t)ng * 2 * Z + 1 && hoff.back() == (int64_t)h.size(), "head offsets");
  CHECK((int64_t)o.size() == glen * ng, "bulk orders: %zu entries, not %d x %lld", o.size(), ng, (long long)glen);
  Walk w{naug / UT, steps, {}, 0.0};
  auto list = [&](int G, int m, int kb, int npan) {
    const int64_t i = (int64_t)G * 2 * Z + m;
    w.launch(h.data() + hoff[(size_t)i], hoff[(size_t)i + 1] - hoff[(size_t)i], kb, npan, -1, -1);
  };
  auto produce_q = [&](int G) {  // (group 0: k_gather, no update)
    if (G > 0) list(G, 0, Z * (G - 1), zsize(G - 1));
  };
  auto produce = [&](int G) {
    const int kb = Z * G, zb = zsize(G);
    if (G > 0) list(G, 1, Z * (G - 1), zsize(G - 1));  // the rest of the cross
    for (int j = 0; j + 1 < zb; ++j) {
      list(G, 2 + j, kb + j, 1);       // panel kb + j on Q_{j+1}
      list(G, zb + j + 1, kb, j + 1);  // T_{j+1}
    }
  };
  produce_q(0);
  produce(0);
  for (int g = 0; g < ng; ++g) {
    const bool more = g + 1 < ng;
    const int kx0 = more ? Z * (g + 1) : -1, kx1 = more ? Z * (g + 1) + zsize(g + 1) : -1;
    if (more) produce_q(g + 1);
    w.launch(o.data() + (int64_t)g * glen, glen, Z * g, zsize(g), kx0, kx1);
    if (more) produce(g + 1);
  }
  w.verify("head schedule", Z);
}

static void check_step_schedule(int steps) {
  const int64_t naug = (int64_t)steps * NB + AUG, nT = naug / UT;
  std::vector<int64_t> xoff;
  const std::vector<Tile> x = cross_update_tiles(naug, steps, S_DEFAULT, xoff);
  const std::vector<Tile> order = xcd_update_order(own_tiles(nT, UT, 1, 0), S_DEFAULT);
  CHECK((int)xoff.size() == std::max(steps, 1) && xoff.back() == (int64_t)x.size(), "cross offsets");
  Walk w{nT, steps, {}, 0.0};
  for (int k = 0; k < steps; ++k) {
    const bool more = k + 1 < steps;
    if (more) w.launch(x.data() + xoff[(size_t)k], xoff[(size_t)k + 1] - xoff[(size_t)k], k, 1, -1, -1);
    w.launch(order.data(), (int64_t)order.size(), k, 1, more ? k + 1 : -1, more ? k + 2 : -1);
  }
  w.verify("one-step schedule", 1);
}

// G ranks: each group's bulk lists hold every lower tile once, on the rank
// that owns its column, and their work sums to the whole triangle's
static void check_ranks(int steps, int Z, int G) {
  const int64_t naug = (int64_t)steps * NB + AUG, nT = naug / UT;
  const int ng = (steps + Z - 1) / Z;
  std::vector<double> work((size_t)ng, 0.0);
  std::vector<std::map<std::pair<int, int>, int>> seen((size_t)ng);
  for (int r = 0; r < G; ++r) {
    int64_t glen = 0;
    const std::vector<Tile> o = pair_bulk_orders(naug, steps, S_DEFAULT, &glen, G, r, Z);
    CHECK((int64_t)o.size() == glen * ng && glen % 8 == 0, "rank %d of %d: bulk order sizes", r, G);
    for (int g = 0; g < ng; ++g) {
      const bool more = g + 1 < ng;
      const int kx0 = more ? Z * (g + 1) : -1, kx1 = more ? std::min(Z * (g + 2), steps) : -1;
      const std::vector<Tile> v(o.begin() + g * glen, o.begin() + (g + 1) * glen);
      for (const Tile &t : v)
        if (t.I >= 0) {
          CHECK(owns_col((int64_t)t.J * UT, G, r), "rank %d of %d lists tile (%d, %d)", r, G, t.I, t.J);
          ++seen[(size_t)g][{t.I, t.J}];
        }
      work[(size_t)g] += tile_list_work(v, nT, (int64_t)Z * g * KT, std::min(Z, steps - Z * g), kx0, kx1);
    }
  }
  for (int g = 0; g < ng; ++g) {
    const bool more = g + 1 < ng;
    const int kx0 = more ? Z * (g + 1) : -1, kx1 = more ? std::min(Z * (g + 2), steps) : -1;
    CHECK((int64_t)seen[(size_t)g].size() == nT * (nT + 1) / 2, "G %d group %d: %zu tiles listed", G, g,
          seen[(size_t)g].size());
    for (auto &kv : seen[(size_t)g]) CHECK(kv.second == 1, "G %d group %d: a tile listed twice", G, g);
    const double all = update_gemm_tiles_group(naug, (int64_t)Z * g * NB, std::min(Z, steps - Z * g), kx0, kx1);
    CHECK(work[(size_t)g] == all, "steps %d Z %d G %d group %d: ranks' work %.4f, whole %.4f", steps, Z, G, g,
          work[(size_t)g], all);
  }
}

// ---- 3b. the sharded schedules (ace_shard.cpp), every rank walked in turn -----
// a rank's launch: as Walk::launch, and every tile's column block is the rank's
static void rank_launch(Walk &w, int G, int r, const Tile *tl, int64_t n, int kb, int npan, int kx0, int kx1) {
  for (int64_t i = 0; i < n; ++i)
    CHECK(tl[i].I < 0 || owns_col((int64_t)tl[i].J * UT, G, r), "rank %d of %d launches on tile (%d, %d)", r, G,
          tl[i].I, tl[i].J);
  w.launch(tl, n, kb, npan, kx0, kx1);
}
// a rank's bulk list (RankState::hupd)
static std::vector<Tile> rank_bulk_tiles(int64_t nT, int G, int r) {
  return xcd_update_order(own_tiles(nT, UT, G, r), S_DEFAULT);
}

// run_sweep_sharded_heads
static void check_sharded_head_schedule(int steps, int Z, int G) {
  const int64_t naug = (int64_t)steps * NB + AUG, nT = naug / UT;
  const int ng = (steps + Z - 1) / Z;
  auto zsize = [&](int g) { return std::min(Z, steps - Z * g); };
  std::vector<int64_t> aoff;
  const std::vector<Tile> all = group_head_tiles(naug, steps, Z, S_DEFAULT, aoff);
  Walk w{nT, steps, {}, 0.0};
  for (int r = 0; r < G; ++r) {
    std::vector<int64_t> hoff;
    const std::vector<Tile> h = rank_head_tiles(naug, steps, Z, S_DEFAULT, G, r, hoff);
    // the single-GPU lists restricted to the rank, in the same order
    CHECK(hoff.size() == aoff.size() && hoff.back() == (int64_t)h.size(), "rank %d of %d: head offsets", r, G);
    for (size_t m = 0; m + 1 < aoff.size() && m + 1 < hoff.size(); ++m) {
      int64_t at = hoff[m];
      for (int64_t i = aoff[m]; i < aoff[m + 1]; ++i) {
        const Tile &t = all[(size_t)i];
        if (t.I < 0 || !owns_col((int64_t)t.J * UT, G, r)) continue;
        CHECK(at < hoff[m + 1] && h[(size_t)at].I == t.I && h[(size_t)at].J == t.J,
              "steps %d Z %d rank %d of %d: head list %zu differs at tile (%d, %d)", steps, Z, r, G, m, t.I, t.J);
        ++at;
      }
      CHECK(at == hoff[m + 1], "steps %d Z %d rank %d of %d: head list %zu has extra tiles", steps, Z, r, G, m);
    }
    const std::vector<Tile> bulk = rank_bulk_tiles(nT, G, r);
    auto list = [&](int g, int m, int kb, int npan) {
      const int64_t i = (int64_t)g * 2 * Z + m;
      rank_launch(w, G, r, h.data() + hoff[(size_t)i], hoff[(size_t)i + 1] - hoff[(size_t)i], kb, npan, -1, -1);
    };
    auto produce = [&](int g) {
      const int kb = Z * g, zb = zsize(g);
      if (g > 0) {
        list(g, 0, Z * (g - 1), zsize(g - 1));  // Q
        list(g, 1, Z * (g - 1), zsize(g - 1));  // the rest of the cross
      }
      for (int j = 0; j + 1 < zb; ++j) {
        list(g, 2 + j, kb + j, 1);       // panel kb + j on Q_{j+1}
        list(g, zb + j + 1, kb, j + 1);  // T_{j+1}
      }
    };
    produce(0);
    for (int g = 0; g < ng; ++g) {
      const bool more = g + 1 < ng;
      const int kx0 = more ? Z * (g + 1) : -1, kx1 = more ? Z * (g + 1) + zsize(g + 1) : -1;
      rank_launch(w, G, r, bulk.data(), (int64_t)bulk.size(), Z * g, zsize(g), kx0, kx1);
      if (more) produce(g + 1);
    }
  }
  char what[64];
  snprintf(what, sizeof what, "sharded head schedule, %d ranks", G);
  w.verify(what, Z);
}

// run_sweep_sharded_steps: the cross launch is a grid over the block's rows
// and columns whose workgroups keep to the rank's columns (k_update_x)
static void check_sharded_step_schedule(int steps, int G) {
  const int64_t naug = (int64_t)steps * NB + AUG, nT = naug / UT;
  Walk w{nT, steps, {}, 0.0};
  for (int r = 0; r < G; ++r) {
    const std::vector<Tile> own = own_tiles(nT, UT, G, r), bulk = rank_bulk_tiles(nT, G, r);
    for (int k = 0; k < steps; ++k) {
      const bool more = k + 1 < steps;
      if (more) {
        std::vector<Tile> x;
        for (const Tile &t : own)
          if (in_blocks(t, k + 1, k + 2)) x.push_back(t);
        rank_launch(w, G, r, x.data(), (int64_t)x.size(), k, 1, -1, -1);
      }
      rank_launch(w, G, r, bulk.data(), (int64_t)bulk.size(), k, 1, more ? k + 1 : -1, k + 2);
    }
  }
  char what[64];
  snprintf(what, sizeof what, "sharded one-step schedule, %d ranks", G);
  w.verify(what, 1);
}

// a rank's assembly and gradient lists, and the layout helpers
static void check_rank_lists(int steps, int Z, int G) {
  const int64_t npad = (int64_t)steps * NB, naug = npad + AUG, n = npad - 37;
  const int64_t na = npad / AT, ng = (n + AT - 1) / AT;
  std::set<std::pair<int, int>> seen_a, seen_g;
  int64_t cols = 0;
  for (int r = 0; r < G; ++r) {
    cols += ncols_local(naug, G, r);
    int64_t nfirst = -1, ndiag = -1;
    const std::vector<Tile> ta = rank_asm_tiles(npad, Z, G, r, &nfirst);
    const std::vector<Tile> tg = rank_grad_tiles(n, G, r, &ndiag);
    CHECK(nfirst >= 0 && nfirst <= (int64_t)ta.size() && ndiag >= 0 && ndiag <= (int64_t)tg.size(),
          "rank %d of %d: list counts", r, G);
    for (size_t i = 0; i < ta.size(); ++i) {
      const Tile &t = ta[i];
      CHECK(t.J >= 0 && t.J <= t.I && t.I < na && owns_col((int64_t)t.J * AT, G, r) && seen_a.insert({t.I, t.J}).second,
            "steps %d rank %d of %d: assembly tile (%d, %d)", steps, r, G, t.I, t.J);
      // the first part is exactly the tiles in the first group's columns
      CHECK(((int64_t)i < nfirst) == ((int64_t)t.J * AT < (int64_t)Z * NB),
            "steps %d Z %d rank %d of %d: assembly tile (%d, %d) at %zu, first part %lld", steps, Z, r, G, t.I, t.J,
            i, (long long)nfirst);
    }
    for (size_t i = 0; i < tg.size(); ++i) {
      const Tile &t = tg[i];
      CHECK(t.J >= 0 && t.J <= t.I && t.I < ng && owns_col((int64_t)t.J * AT, G, r) && seen_g.insert({t.I, t.J}).second,
            "steps %d rank %d of %d: gradient tile (%d, %d)", steps, r, G, t.I, t.J);
      CHECK(((int64_t)i < ndiag) == (t.I == t.J), "steps %d rank %d of %d: gradient tile (%d, %d) at %zu, ndiag %lld",
            steps, r, G, t.I, t.J, i, (long long)ndiag);
    }
  }
  CHECK((int64_t)seen_a.size() == na * (na + 1) / 2, "steps %d G %d: %zu assembly tiles", steps, G, seen_a.size());
  CHECK((int64_t)seen_g.size() == ng * (ng + 1) / 2, "steps %d G %d: %zu gradient tiles", steps, G, seen_g.size());
  CHECK(cols == (naug + NB - 1) / NB * NB, "naug %lld G %d: %lld local columns", (long long)naug, G, (long long)cols);
}

// the single-GPU gradient order: the diagonal, then every strictly lower tile once
static std::vector<uint32_t> test_mask(int64_t ntr) {
  std::vector<uint32_t> m((size_t)ntr);
  for (int64_t k = 0; k < ntr; ++k) m[(size_t)k] = (uint32_t)((k * 2654435761u) >> 7) & 0x1ffu;
  return m;
}
static void check_grad_order(int64_t n, int S, bool masked) {
  const int64_t ntr = (n + AT - 1) / AT;
  const std::vector<uint32_t> mk = test_mask(ntr);
  int64_t ndiag = -1;
  const std::vector<Tile> o = grad_tile_order(n, S, masked ? mk.data() : nullptr, &ndiag);
  CHECK(ndiag == ntr && (int64_t)o.size() >= ntr * (ntr + 1) / 2, "gradient order n %lld: counts", (long long)n);
  std::set<std::pair<int, int>> seen;
  for (size_t i = 0; i < o.size(); ++i) {
    const Tile &t = o[i];
    if ((int64_t)i < ndiag) CHECK(t.I == (int)i && t.J == (int)i, "gradient order n %lld: entry %zu", (long long)n, i);
    else if (t.I >= 0)
      CHECK(t.J >= 0 && t.J < t.I && t.I < ntr && seen.insert({t.I, t.J}).second,
            "gradient order n %lld: tile (%d, %d)", (long long)n, t.I, t.J);
  }
  CHECK((int64_t)seen.size() == ntr * (ntr - 1) / 2, "gradient order n %lld: %zu lower tiles", (long long)n, seen.size());
}

// ---- 4. the lists and counters of the commit before the plan moved here ------
static uint64_t fnv(uint64_t h, int64_t v) {
  for (int i = 0; i < 8; ++i) {
    h ^= (uint64_t)(v >> (8 * i)) & 0xff;
    h *= 0x100000001b3ull;
  }
  return h;
}
static uint64_t hash_list(const std::vector<Tile> &t, const std::vector<int64_t> &extra) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (const Tile &x : t) h = fnv(fnv(h, x.I), x.J);
  for (int64_t e : extra) h = fnv(h, e);
  return h;
}

struct Pinned {
  const char *name;
  uint64_t hash;
};
struct PinnedValue {
  const char *name;
  double value;
};
// (values of the parent commit's functions, profiles/sweep_plan_ab.txt)
static const Pinned PINNED[] = {
    {"cross_update_tiles steps=2", 0x81bc9a85e1dd2915ull},
    {"group_head_tiles steps=2 Z=2", 0x550f00e030ee3545ull},
    {"pair_bulk_orders steps=2 Z=2 G=1 r=0", 0x8be950a762ea3315ull},
    {"pair_bulk_orders steps=2 Z=2 G=3 r=0", 0xb72909b0df8ae435ull},
    {"pair_bulk_orders steps=2 Z=2 G=3 r=2", 0x6c93e6a53c14dfddull},
    {"group_head_tiles steps=2 Z=3", 0x1cd711bdbfc52345ull},
    {"pair_bulk_orders steps=2 Z=3 G=1 r=0", 0x8be950a762ea3315ull},
    {"pair_bulk_orders steps=2 Z=3 G=3 r=0", 0xb72909b0df8ae435ull},
    {"pair_bulk_orders steps=2 Z=3 G=3 r=2", 0x6c93e6a53c14dfddull},
    {"group_head_tiles steps=2 Z=4", 0xc96ebaaeb0a79145ull},
    {"pair_bulk_orders steps=2 Z=4 G=1 r=0", 0x8be950a762ea3315ull},
    {"pair_bulk_orders steps=2 Z=4 G=3 r=0", 0xb72909b0df8ae435ull},
    {"pair_bulk_orders steps=2 Z=4 G=3 r=2", 0x6c93e6a53c14dfddull},
    {"cross_update_tiles steps=5", 0xcee06d80f70d6d05ull},
    {"group_head_tiles steps=5 Z=2", 0x317fca771070d9f5ull},
    {"pair_bulk_orders steps=5 Z=2 G=1 r=0", 0x3a355b94247c726dull},
    {"pair_bulk_orders steps=5 Z=2 G=3 r=0", 0x5aa8bbf8df73e685ull},
    {"pair_bulk_orders steps=5 Z=2 G=3 r=2", 0x18fae011f5b0a705ull},
    {"group_head_tiles steps=5 Z=3", 0xe5bcbfd162a280acull},
    {"pair_bulk_orders steps=5 Z=3 G=1 r=0", 0x004875269d70688dull},
    {"pair_bulk_orders steps=5 Z=3 G=3 r=0", 0x588c21e2585d3165ull},
    {"pair_bulk_orders steps=5 Z=3 G=3 r=2", 0x9cf90b856ca46e65ull},
    {"group_head_tiles steps=5 Z=4", 0xb369f38b5d3d574full},
    {"pair_bulk_orders steps=5 Z=4 G=1 r=0", 0x004875269d70688dull},
    {"pair_bulk_orders steps=5 Z=4 G=3 r=0", 0x588c21e2585d3165ull},
    {"pair_bulk_orders steps=5 Z=4 G=3 r=2", 0x9cf90b856ca46e65ull},
    {"cross_update_tiles steps=13", 0x338c69a883b00574ull},
    {"group_head_tiles steps=13 Z=2", 0x2c89d6dca0b58cfeull},
    {"pair_bulk_orders steps=13 Z=2 G=1 r=0", 0xd5946266a5a49b2aull},
    {"pair_bulk_orders steps=13 Z=2 G=3 r=0", 0x0f97eea535c8592dull},
    {"pair_bulk_orders steps=13 Z=2 G=3 r=2", 0x660c0860fcf42b7dull},
    {"group_head_tiles steps=13 Z=3", 0xfee87590747456b3ull},
    {"pair_bulk_orders steps=13 Z=3 G=1 r=0", 0x8e247423f9adb72aull},
    {"pair_bulk_orders steps=13 Z=3 G=3 r=0", 0x6724061999321c8dull},
    {"pair_bulk_orders steps=13 Z=3 G=3 r=2", 0xe92b62883c1c4afdull},
    {"group_head_tiles steps=13 Z=4", 0xa8f11f78f8bda2c5ull},
    {"pair_bulk_orders steps=13 Z=4 G=1 r=0", 0xc5aacad13e65df4aull},
    {"pair_bulk_orders steps=13 Z=4 G=3 r=0", 0xc5b05e6f8ffc3efdull},
    {"pair_bulk_orders steps=13 Z=4 G=3 r=2", 0x387eb5fd1582f63dull},
    {"xcd_update_order steps=13 S=2", 0xede58f8ffde48a85ull},
    {"xcd_update_order steps=13 S=4", 0x8c023ab8212e0085ull},
    // the lists ace_shard.cpp and ace_api.cpp built inline before these
    // functions (profiles/shard_plan_ab.txt)
    {"rank_head_tiles steps=5 Z=2 G=3 r=0", 0xee47bb4e3e91e65full},
    {"rank_asm_tiles steps=5 Z=2 G=3 r=0", 0x23e467b27e77bf4full},
    {"rank_grad_tiles steps=5 Z=2 G=3 r=0", 0x61b771322ec8facdull},
    {"rank_head_tiles steps=7 Z=3 G=4 r=3", 0x6dd8ff935494a117ull},
    {"rank_asm_tiles steps=7 Z=3 G=4 r=3", 0x09a3f10f9f573ec5ull},
    {"rank_grad_tiles steps=7 Z=3 G=4 r=3", 0x83cbd224f5c57241ull},
    {"rank_head_tiles steps=13 Z=4 G=2 r=1", 0x696c56d3c601f4d0ull},
    {"rank_asm_tiles steps=13 Z=4 G=2 r=1", 0xb5bf936d0c2d9536ull},
    {"rank_grad_tiles steps=13 Z=4 G=2 r=1", 0x4fd62174b86d83ddull},
    {"rank_head_tiles steps=8 Z=4 G=8 r=5", 0x590b1709c698db5dull},
    {"rank_asm_tiles steps=8 Z=4 G=8 r=5", 0x5763832f033c9bc5ull},
    {"rank_grad_tiles steps=8 Z=4 G=8 r=5", 0x9912334ff03acf41ull},
    {"grad_tile_order n=1700 mask=0", 0x1a60bbb1e7bb1cceull},
    {"grad_tile_order n=1700 mask=1", 0xda73f24a0eb038ceull},
    {"grad_tile_order n=3301 mask=0", 0x07ea701f2748ed31ull},
    {"grad_tile_order n=3301 mask=1", 0x548c46a9bc8259b1ull},
};
static const PinnedValue PINNED_VALUES[] = {
    {"update_gemm_tiles k=4 kx=5", 255.875},
    {"update_gemm_tiles k=4 kx=5 look", 47.25},
    {"update_gemm_tiles k=12", 303.125},
    {"update_gemm_tiles_group g=1", 418.375},
    {"update_gemm_tiles_group g=4", 303.125},
    {"sweep_flops", 38508953600},
    {"list flops, one step k=4 kx=5 (rank 1 of 3)", 619708416},
    {"list flops, group g=1 (rank 1 of 3)", 1133510656},
    // the pair kernels' work of a timed evaluation at n = 1700, B = 10, p = 20:
    // model_collect_timing, then shard_collect_timing on rank 0 of 3
    {"model assembly flops", 910885500},
    {"model gradient flops SE", 1214514000},
    {"model gradient flops Matern", 1503684000},
    {"shard pairs (rank 0 of 3)", 641376},
    {"shard assembly flops", 404066880},
    {"shard gradient flops SE", 538755840},
    {"shard gradient flops Matern", 667031040},
};

static void check_pinned() {
  std::vector<std::pair<std::string, uint64_t>> got;
  std::vector<int64_t> off;
  char name[96];
  for (int steps : {2, 5, 13})
    for (int Z : {2, 3, 4}) {
      const int64_t naug = (int64_t)steps * NB + AUG;
      if (Z == 2) {
        snprintf(name, sizeof name, "cross_update_tiles steps=%d", steps);
        const std::vector<Tile> x = cross_update_tiles(naug, steps, S_DEFAULT, off);
        got.push_back({name, hash_list(x, off)});
      }
      snprintf(name, sizeof name, "group_head_tiles steps=%d Z=%d", steps, Z);
      const std::vector<Tile> h = group_head_tiles(naug, steps, Z, S_DEFAULT, off);
      got.push_back({name, hash_list(h, off)});
      for (int G : {1, 3})
        for (int r = 0; r < G; r += 2) {
          int64_t len = 0;
          snprintf(name, sizeof name, "pair_bulk_orders steps=%d Z=%d G=%d r=%d", steps, Z, G, r);
          const std::vector<Tile> o = pair_bulk_orders(naug, steps, S_DEFAULT, &len, G, r, Z);
          got.push_back({name, hash_list(o, {len})});
        }
    }
  for (int S : {2, 4}) {
    snprintf(name, sizeof name, "xcd_update_order steps=13 S=%d", S);
    got.push_back({name, hash_list(xcd_update_order(own_tiles((13 * NB + AUG) / UT, UT, 1, 0), S), {})});
  }
  // (7, 3, 4, 3): steps % Z != 0 and a rank without a column of the first group
  struct {
    int steps, Z, G, r;
  } const pts[] = {{5, 2, 3, 0}, {7, 3, 4, 3}, {13, 4, 2, 1}, {8, 4, 8, 5}};
  for (auto &q : pts) {
    const int64_t npad = (int64_t)q.steps * NB, n = npad - 37;
    int64_t cnt = 0;
    snprintf(name, sizeof name, "rank_head_tiles steps=%d Z=%d G=%d r=%d", q.steps, q.Z, q.G, q.r);
    const std::vector<Tile> h = rank_head_tiles(npad + AUG, q.steps, q.Z, S_DEFAULT, q.G, q.r, off);
    got.push_back({name, hash_list(h, off)});
    snprintf(name, sizeof name, "rank_asm_tiles steps=%d Z=%d G=%d r=%d", q.steps, q.Z, q.G, q.r);
    const std::vector<Tile> ta = rank_asm_tiles(npad, q.Z, q.G, q.r, &cnt);
    got.push_back({name, hash_list(ta, {cnt})});
    snprintf(name, sizeof name, "rank_grad_tiles steps=%d Z=%d G=%d r=%d", q.steps, q.Z, q.G, q.r);
    const std::vector<Tile> tg = rank_grad_tiles(n, q.G, q.r, &cnt);
    got.push_back({name, hash_list(tg, {cnt})});
  }
  for (int64_t n : {1700, 3301})
    for (int masked = 0; masked < 2; ++masked) {
      const std::vector<uint32_t> mk = test_mask((n + AT - 1) / AT);
      int64_t ndiag = 0;
      snprintf(name, sizeof name, "grad_tile_order n=%lld mask=%d", (long long)n, masked);
      const std::vector<Tile> o = grad_tile_order(n, S_GRAD_DEFAULT, masked ? mk.data() : nullptr, &ndiag);
      got.push_back({name, hash_list(o, {ndiag})});
    }
  for (auto &g : got) printf("hash %-44s 0x%016llxull\n", g.first.c_str(), (unsigned long long)g.second);
  CHECK(got.size() == sizeof PINNED / sizeof *PINNED, "%zu lists, %zu pinned", got.size(),
        sizeof PINNED / sizeof *PINNED);
  for (size_t i = 0; i < got.size() && i < sizeof PINNED / sizeof *PINNED; ++i)
    CHECK(got[i].first == PINNED[i].name && got[i].second == PINNED[i].hash, "list changed: %s",
          got[i].first.c_str());

  // the five counters: 13 steps, groups of 3
  const int64_t naug = 13 * NB + AUG, nT = naug / UT;
  const std::vector<Tile> own = xcd_update_order(own_tiles(nT, UT, 3, 1), S_DEFAULT);
  const double mpairs = 1700.0 * 1701.0 / 2;
  int64_t nd = 0;
  const double spairs = tile_list_pairs(rank_grad_tiles(1700, 3, 0, &nd));
  const std::pair<const char *, double> vals[] = {
      {"update_gemm_tiles k=4 kx=5", update_gemm_tiles(naug, 4 * NB, 5, false)},
      {"update_gemm_tiles k=4 kx=5 look", update_gemm_tiles(naug, 4 * NB, 5, true)},
      {"update_gemm_tiles k=12", update_gemm_tiles(naug, 12 * NB, -1, false)},
      {"update_gemm_tiles_group g=1", update_gemm_tiles_group(naug, 3 * NB, 3, 6, 9)},
      {"update_gemm_tiles_group g=4", update_gemm_tiles_group(naug, 12 * NB, 1, -1, -1)},
      {"sweep_flops", sweep_flops(naug, 13 * NB)},
      {"list flops, one step k=4 kx=5 (rank 1 of 3)", tile_list_work(own, nT, 4 * KT, 1, 5, 6) * TILE_FLOPS},
      {"list flops, group g=1 (rank 1 of 3)", tile_list_work(own, nT, 3 * KT, 3, 6, 9) * TILE_FLOPS},
      {"model assembly flops", asm_flops(mpairs, 10, 20)},
      {"model gradient flops SE", grad_flops(mpairs, 10, 20, false)},
      {"model gradient flops Matern", grad_flops(mpairs, 10, 20, true)},
      {"shard pairs (rank 0 of 3)", spairs},
      {"shard assembly flops", asm_flops(spairs, 10, 20)},
      {"shard gradient flops SE", grad_flops(spairs, 10, 20, false)},
      {"shard gradient flops Matern", grad_flops(spairs, 10, 20, true)},
  };
  size_t i = 0;
  for (auto &v : vals) {
    printf("value %-44s %.17g\n", v.first, v.second);
    const bool known = i < sizeof PINNED_VALUES / sizeof *PINNED_VALUES;
    CHECK(known && std::string(v.first) == PINNED_VALUES[i].name && v.second == PINNED_VALUES[i].value,
          "counter changed: %s", v.first);
    ++i;
  }
}

// ---- 5. the small-n rules and the queue layout ---------------------------------
static void check_layout() {
  struct {
    int64_t naug;
    int Z, reserve, qfirst;
    int64_t fctr, qctr, ints;
  } const want[] = {{384, 3, 1, 1, 66, 68, 69},
                    {8192 + AUG, 3, 1, 1, 726, 790, 822},
                    {8192 + AUG + NB, 4, 0, 0, 594, 660, 693}};
  for (auto &w : want) {
    const int steps = (int)((w.naug - AUG) / NB), Z = default_group(w.naug);
    const BqLayout q = bq_layout(steps, Z);
    CHECK(Z == w.Z && default_bulk_reserve(w.naug) == w.reserve && (int)default_q_first(w.naug) == w.qfirst,
          "naug %lld: Z %d reserve %d qfirst %d", (long long)w.naug, Z, default_bulk_reserve(w.naug),
          (int)default_q_first(w.naug));
    CHECK(q.fctr == w.fctr && q.qctr == w.qctr && q.ints == w.ints, "naug %lld: bq_layout %lld %lld %lld",
          (long long)w.naug, (long long)q.fctr, (long long)q.qctr, (long long)q.ints);
  }
  static_assert(BQ_INTS == 66, "the bulk queue: next, leavers, 2 x 32 CU claims");
}

int main() {
  static_assert(NB == 256 && UT == 128 && AUG == 128, "the pinned values are for the default blocking");
  for (int steps = 1; steps <= 13; ++steps) {
    check_step_schedule(steps);
    for (int Z = 2; Z <= 4; ++Z) {
      check_events(steps, Z);
      if (steps >= 2) check_head_schedule(steps, Z);
      for (int G = 1; G <= 3; ++G) check_ranks(steps, Z, G);
      for (int G = 1; G <= 4; ++G) {
        if (steps >= 2) check_sharded_head_schedule(steps, Z, G);
        if (Z == 2) check_sharded_step_schedule(steps, G);
        check_rank_lists(steps, Z, G);
      }
    }
  }
  check_sharded_head_schedule(13, 3, 8);
  check_sharded_step_schedule(13, 8);
  check_rank_lists(13, 3, 8);
  for (int64_t n : {1, 64, 65, 1700})
    for (int masked = 0; masked < 2; ++masked) check_grad_order(n, S_GRAD_DEFAULT, masked != 0);
  check_pinned();
  check_layout();
  if (failures) {
    printf("sweep_plan_check: %d FAILED\n", failures);
    return 1;
  }
  printf("sweep_plan_check: OK\n");
  return 0;
}
