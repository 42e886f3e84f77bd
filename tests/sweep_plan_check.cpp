// Stand-alone check of the sweep's host-only planning (csrc/ace_sweep_plan.*):
// the event names, the tile lists of both schedules, the tile-work rule and
// the small-n layout rules.  Built and run by tests/test_sweep_plan_cpu.py
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
constexpr int S_DEFAULT = 2;  // update_order_block()'s default

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
  for (auto &g : got) printf("hash %-44s 0x%016llxull\n", g.first.c_str(), (unsigned long long)g.second);
  CHECK(got.size() == sizeof PINNED / sizeof *PINNED, "%zu lists, %zu pinned", got.size(),
        sizeof PINNED / sizeof *PINNED);
  for (size_t i = 0; i < got.size() && i < sizeof PINNED / sizeof *PINNED; ++i)
    CHECK(got[i].first == PINNED[i].name && got[i].second == PINNED[i].hash, "list changed: %s",
          got[i].first.c_str());

  // the five counters: 13 steps, groups of 3
  const int64_t naug = 13 * NB + AUG, nT = naug / UT;
  const std::vector<Tile> own = xcd_update_order(own_tiles(nT, UT, 3, 1), S_DEFAULT);
  const std::pair<const char *, double> vals[] = {
      {"update_gemm_tiles k=4 kx=5", update_gemm_tiles(naug, 4 * NB, 5, false)},
      {"update_gemm_tiles k=4 kx=5 look", update_gemm_tiles(naug, 4 * NB, 5, true)},
      {"update_gemm_tiles k=12", update_gemm_tiles(naug, 12 * NB, -1, false)},
      {"update_gemm_tiles_group g=1", update_gemm_tiles_group(naug, 3 * NB, 3, 6, 9)},
      {"update_gemm_tiles_group g=4", update_gemm_tiles_group(naug, 12 * NB, 1, -1, -1)},
      {"sweep_flops", sweep_flops(naug, 13 * NB)},
      {"list flops, one step k=4 kx=5 (rank 1 of 3)", tile_list_work(own, nT, 4 * KT, 1, 5, 6) * TILE_FLOPS},
      {"list flops, group g=1 (rank 1 of 3)", tile_list_work(own, nT, 3 * KT, 3, 6, 9) * TILE_FLOPS},
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
    }
  }
  check_pinned();
  check_layout();
  if (failures) {
    printf("sweep_plan_check: %d FAILED\n", failures);
    return 1;
  }
  printf("sweep_plan_check: OK\n");
  return 0;
}
