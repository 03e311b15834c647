// Host check of csrc/gemm_route.h: the routing table of the weight-gradient (TN) products, recorded from the decision code as it
// was before it moved into that header (direct_ok / launch_tn_direct of gemm.hip, 256 CUs), and the first-use state machine under
// threads with a fake check.  Exits non-zero at the first difference.  Built and run by tests/test_gemm_route_cpu.py.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../ubisoft-laforge-zeroeggs_amd/csrc/gemm_route.h"

#define EXPECT(cond, ...)                                            \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "gemm_route_check: %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                  \
      fprintf(stderr, "  [%s]\n", #cond);                            \
      exit(1);                                                       \
    }                                                                \
  } while (0)

namespace {

constexpr int NCU = 256;
const TnRoute DEFAULTS{1, 0, 4, 0};

struct Shape { const char* name; TnShape g; int tx, ty64, ty128, cpb; };      // ty: output tiles along M with the 64 x 64 / 128 x 64 wave tile
const Shape SHAPES[] = {
    {"dW_hh", {3072, 1024, 8160, 1, 3072, 1024}, 8, 24, 12, 510},
    {"dW_ih0", {3072, 2286, 8160, 1, 3072, 2288}, 18, 24, 12, 510},
    {"dW_l2", {1131, 1024, 8160, 1, 1136, 1024}, 8, 9, 5, 510},
    {"dW_l0", {1024, 1262, 8160, 1, 1024, 2286}, 10, 8, 4, 510},
    {"conv_dw", {384, 128, 192, 7, 384, 128}, 1, 3, 2, 12},
    {"conv0_dw", {3402, 512, 208, 5, 1134, 512}, 4, 27, 14, 13},
    {"ragged", {197, 333, 1026, 1, 200, 340}, 3, 2, 1, 65},
    {"tiny", {130, 70, 2048, 1, 131, 73}, 1, 2, 1, 128},
};
const Shape NEVER[] = {      // "lds" under every route: an odd K, fewer than 64 rows
    {"oddK", {128, 128, 1025, 1, 128, 128}, 0, 0, 0, 0},
    {"narrow", {63, 512, 4096, 1, 64, 512}, 0, 0, 0, 0},
};

struct Cell { int big, shield; long nwg; };      // big < 0: the LDS-tiled kernel ("lds")
constexpr Cell LDS{-1, 0, 0};
struct Row { const char* name; TnRoute route; int depth; Cell cell[8]; };
const Row ROWS[] = {
    {"default", {1, 0, 4, 0}, 4, {{0, 0, 512}, {1, 0, 256}, {0, 0, 512}, {0, 0, 512}, {0, 0, 63}, {0, 0, 512}, {0, 0, 97}, {0, 0, 64}}},
    {"engine", {1, 1, 8, 0}, 8, {{0, 1, 256}, {1, 1, 256}, {0, 1, 256}, {0, 1, 256}, {0, 1, 63}, {0, 1, 256}, {0, 1, 97}, {0, 1, 64}}},
    {"engine, world > 1", {1, 1, 8, 32}, 8, {{0, 1, 224}, {1, 1, 224}, {0, 1, 224}, {0, 1, 224}, {0, 1, 63}, {0, 1, 224}, {0, 1, 97}, {0, 1, 64}}},
    {"reserve >= ncu / 2 is ignored", {1, 1, 8, 128}, 8, {{0, 1, 256}, {1, 1, 256}, {0, 1, 256}, {0, 1, 256}, {0, 1, 63}, {0, 1, 256}, {0, 1, 97}, {0, 1, 64}}},
    {"beside", {5, 2, 8, 0}, 8, {LDS, LDS, LDS, LDS, {0, 0, 63}, {0, 0, 512}, {0, 0, 97}, {0, 0, 64}}},
    {"128 x 64 always", {2, 0, 6, 0}, 6, {{1, 0, 256}, {1, 0, 256}, {1, 0, 256}, {1, 0, 256}, {1, 0, 42}, {1, 0, 256}, {1, 0, 48}, {1, 0, 32}}},
    {"64 x 64 always, shield on the big", {3, 2, 4, 0}, 4, {{0, 1, 256}, {0, 1, 256}, {0, 1, 256}, {0, 1, 256}, {0, 0, 63}, {0, 0, 512}, {0, 0, 97}, {0, 0, 64}}},
    {"off", {0, 1, 8, 0}, 8, {LDS, LDS, LDS, LDS, LDS, LDS, LDS, LDS}},
};

void check_table() {
  for (const Row& row : ROWS) {
    for (int i = 0; i < 8; ++i) {
      const Shape& sh = SHAPES[i];
      const Cell& want = row.cell[i];
      const DirectPlan p = direct_plan(row.route, sh.g, NCU, 0);
      EXPECT(p.use == (want.big >= 0), "%s / %s: use = %d", row.name, sh.name, (int)p.use);
      if (!p.use) continue;
      EXPECT(route_selects(row.route, p.big, p.shield), "%s / %s: a variant the warm-up would not check", row.name, sh.name);
      EXPECT(p.big == (want.big != 0) && p.shield == (want.shield != 0) && p.depth == row.depth && p.nwg == want.nwg,
             "%s / %s: %s/%s/%d/%ld", row.name, sh.name, p.big ? "128x64" : "64x64", p.shield ? "shield" : "plain", p.depth, p.nwg);
      EXPECT(p.tx == sh.tx && p.ty == (p.big ? sh.ty128 : sh.ty64) && p.cpb == sh.cpb, "%s / %s: (%d, %d, %d)", row.name, sh.name,
             p.tx, p.ty, p.cpb);
    }
    for (const Shape& sh : NEVER) EXPECT(!direct_plan(row.route, sh.g, NCU, 0).use, "%s / %s: not lds", row.name, sh.name);
  }
  // the variants the warm-up checks for a route: both wave tiles when direct = 1, the one when 2 / 3 / 5; shield on / both / off
  auto selected = [](const TnRoute& r) {
    int bits = 0;
    for (int big = 0; big < 2; ++big)
      for (int shield = 0; shield < 2; ++shield) bits |= route_selects(r, big, shield) << (2 * big + shield);
    return bits;
  };
  EXPECT(selected({1, 1, 8, 0}) == 0b1010 && selected({1, 0, 4, 0}) == 0b0101 && selected({5, 2, 8, 0}) == 0b0011 &&
             selected({2, 0, 6, 0}) == 0b0100 && selected({3, 2, 4, 0}) == 0b0011 && selected({0, 1, 8, 0}) == 0,
         "route_selects");
  const DirectPlan p = direct_plan(TnRoute{3, 0, 6, 0}, SHAPES[0].g, NCU, 3);      // option "gemm_direct_wgs" = 3
  EXPECT(p.use && !p.big && !p.shield && p.depth == 6 && p.nwg == 768, "wgs = 3: %d/%d/%d/%ld", (int)p.big, (int)p.shield, p.depth, p.nwg);
  const int thread_route[4] = {-1, -1, 6, -1};
  const TnRoute r = resolve(thread_route, DEFAULTS);
  EXPECT(r.direct == 1 && r.shield == 0 && r.depth == 6 && r.reserve == 0, "resolve: (%d, %d, %d, %d)", r.direct, r.shield, r.depth, r.reserve);
}

const auto NOT_CAPTURING = [] { return false; };
const auto CAPTURING = [] { return true; };

void check_first_use() {
  const DirectPlan v = direct_variant(false, 8, true), other = direct_variant(true, 4, false);
  {   // two threads meet the same UNCHECKED variant: one check, both go
    DirectFirstUse fu;
    std::atomic<int> checks{0}, gos{0}, ready{0};
    auto body = [&] {
      ready.fetch_add(1);
      while (ready.load() < 2) std::this_thread::yield();
      if (fu.go(v, NOT_CAPTURING, [&](const DirectPlan&) {
            checks.fetch_add(1);
            return DirectCheck::AGREES;
          }))
        gos.fetch_add(1);
    };
    std::thread a(body), b(body);
    a.join();
    b.join();
    EXPECT(checks == 1 && gos == 2, "two threads: %d checks, %d go", checks.load(), gos.load());
    EXPECT(fu.at(false, 8, true) == DIRECT_OK && fu.at(true, 4, false) == DIRECT_UNCHECKED, "two threads: states");
  }
  {   // UNAVAILABLE: refused, still UNCHECKED, nothing disabled, the next call checks again
    DirectFirstUse fu;
    int checks = 0;
    EXPECT(!fu.go(v, NOT_CAPTURING, [&](const DirectPlan&) { ++checks; return DirectCheck::UNAVAILABLE; }), "unavailable: go");
    EXPECT(fu.at(false, 8, true) == DIRECT_UNCHECKED && !fu.disabled, "unavailable: state %d", fu.at(false, 8, true).load());
    EXPECT(fu.go(v, NOT_CAPTURING, [&](const DirectPlan&) { ++checks; return DirectCheck::AGREES; }) && checks == 2, "unavailable: again");
    EXPECT(fu.at(false, 8, true) == DIRECT_OK && !fu.disabled, "unavailable, then agrees: state");
  }
  {   // MISMATCH: BAD, the process-wide disable, every variant refused from then on
    DirectFirstUse fu;
    int checks = 0;
    auto never = [&](const DirectPlan&) { ++checks; return DirectCheck::AGREES; };
    EXPECT(!fu.go(v, NOT_CAPTURING, [&](const DirectPlan&) { return DirectCheck::MISMATCH; }), "mismatch: go");
    EXPECT(fu.at(false, 8, true) == DIRECT_BAD && fu.disabled, "mismatch: state");
    for (int big = 0; big < 2; ++big)
      for (int depth = 4; depth <= 8; depth += 2)
        for (int shield = 0; shield < 2; ++shield) {
          EXPECT(!fu.go(direct_variant(big, depth, shield), NOT_CAPTURING, never), "mismatch: variant %d/%d/%d goes", big, depth, shield);
          EXPECT(!fu.go(direct_variant(big, depth, shield), CAPTURING, never), "mismatch: variant %d/%d/%d goes in a capture", big, depth, shield);
        }
    EXPECT(checks == 0, "mismatch: %d checks after the disable", checks);
    const int none[4] = {-1, -1, -1, -1}, engine[4] = {1, 1, 8, 0};      // ... and every route resolves to "off"
    for (const Shape& sh : SHAPES) {
      EXPECT(!direct_plan(resolve(none, DEFAULTS, fu.disabled), sh.g, NCU, 0).use, "mismatch: %s still planned", sh.name);
      EXPECT(!direct_plan(resolve(engine, DEFAULTS, fu.disabled), sh.g, NCU, 0).use, "mismatch: %s still planned (route)", sh.name);
    }
  }
  {   // a capturing stream: go, unchecked, and the state stays UNCHECKED
    DirectFirstUse fu;
    int checks = 0;
    EXPECT(fu.go(other, CAPTURING, [&](const DirectPlan&) { ++checks; return DirectCheck::MISMATCH; }) && checks == 0, "capture: go");
    EXPECT(fu.at(true, 4, false) == DIRECT_UNCHECKED && !fu.disabled, "capture: state");
  }
  {   // eight threads on the OK fast path
    DirectFirstUse fu;
    std::atomic<int> checks{0};
    std::atomic<long> gos{0};
    auto agrees = [&](const DirectPlan&) { checks.fetch_add(1); return DirectCheck::AGREES; };
    constexpr int THREADS = 8, ITERS = 200000;
    std::vector<std::thread> pool;
    for (int t = 0; t < THREADS; ++t)
      pool.emplace_back([&] {
        long n = 0;
        for (int i = 0; i < ITERS; ++i) n += fu.go(i & 1 ? v : other, NOT_CAPTURING, agrees);
        gos.fetch_add(n);
      });
    for (auto& t : pool) t.join();
    EXPECT(gos == (long)THREADS * ITERS && checks == 2, "fast path: %ld go, %d checks", gos.load(), checks.load());
  }
}

}  // namespace

int main() {
  check_table();
  check_first_use();
  printf("gemm_route_check: ok\n");
  return 0;
}
