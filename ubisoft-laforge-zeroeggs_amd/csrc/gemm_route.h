// Routing of the weight-gradient (TN) products onto the direct stream-K kernel of gemm.hip, as pure host code: which variant a
// product gets, with which grid, and whether that variant may run yet on this process.  No HIP call and no device code in here
// (tests/host/gemm_route_check.cpp compiles it alone); gemm.hip resolves the route once per product, builds ONE plan from it and
// hands that same plan to the first-use check and to the launch.
#pragma once
#include <atomic>
#include <cstdio>
#include <mutex>

// the values of the options "gemm_direct", "gemm_direct_shield", "gemm_direct_depth", "gemm_direct_reserve" for one product
struct TnRoute { int direct, shield, depth, reserve; };
// a calling thread's route (zeggs_gemm_route) over the process-wide options: -1 = the process-wide option.  `disabled`: a variant
// failed its first-use check on this process -- the direct kernel is off whatever a route says.
inline TnRoute resolve(const int (&thread_route)[4], const TnRoute& options, bool disabled = false) {
  auto pick = [](int t, int o) { return t >= 0 ? t : o; };
  return TnRoute{disabled ? 0 : pick(thread_route[0], options.direct), pick(thread_route[1], options.shield),
                 pick(thread_route[2], options.depth), pick(thread_route[3], options.reserve)};
}

// what the decision needs of a GemmArgs: C(m, n) = sum over kbatch segments of sum_k A[k sak + m sam] B[k sbk + n sbn]
struct TnShape {
  int M, N, K, kbatch;
  long sak, sbk;
  long sam = 1, sbn = 1, scn = 1;
};
// Big outputs (384 tiles of 128 x 128 and more) take the coarser tile of both stream-K families: the 128 x 64 wave tile with one workgroup
// per CU here (fewer operand bytes per product; the others 64 x 64 wave tiles, two workgroups per CU: finer grain at the ends of
// the stream-K ranges), the 256 x 128 workgroup tile of the LDS-tiled kernel.
inline bool tn_big_output(int M, int N) { return (long)((M + 127) / 128) * ((N + 127) / 128) >= 384; }

inline int tn_depth(int option) { return option >= 8 ? 8 : option >= 6 ? 6 : 4; }      // the kernel is built for 4 / 6 / 8

struct DirectPlan {
  bool use;           // the direct kernel takes this product (else: the LDS-tiled stream-K kernel)
  bool big, shield;   // 128 x 64 wave tile (else 64 x 64); the variant that owns its SIMDs' register files
  int depth;          // 4 / 6 / 8 k-pairs of operands in flight per wave
  long nwg;           // workgroups of the stream-K grid
  int tx, ty, cpb;    // output tiles along N and M, chunks of 8 k-pairs per batch segment
};
// the grid of a variant (p.big, p.shield set) over a product's shape
inline DirectPlan direct_grid(DirectPlan p, const TnShape& g, int ncu, int wgs_option, int reserve) {
  auto cdiv = [](long a, long b) { return (int)((a + b - 1) / b); };
  p.tx = cdiv(g.N, 128);
  p.ty = cdiv(g.M, p.big ? 256 : 128);
  p.cpb = cdiv(g.K / 2, 8);
  p.nwg = (long)ncu * (p.shield ? 1 : wgs_option > 0 ? wgs_option : (p.big ? 1 : 2));
  // reserve: CUs a shielded product leaves free.  For data-parallel runs: the collective's workgroups live for the whole exchange,
  // and a stream-K product whose equal-share workgroups do not ALL become resident takes twice as long (the stragglers start when
  // the first ones end); with the CUs of the collective left out of the grid nobody waits for anybody.
  // (On one GPU, where nothing else is resident: 8 / 16 / 32 reserved CUs measured 17.13 / 17.17 / 17.02 ms against 17.03.)
  if (p.shield && reserve > 0 && reserve < ncu / 2) p.nwg = ncu - reserve;
  const long total = (long)p.tx * p.ty * p.cpb * g.kbatch;
  if (p.nwg > total / 4) p.nwg = total / 4 > 0 ? total / 4 : 1;      // at least 4 chunks (64 k) per workgroup
  return p;
}
inline DirectPlan direct_plan(const TnRoute& r, const TnShape& g, int ncu, int wgs_option) {
  DirectPlan p{};
  // a big single-segment product: one of the decoder's weight gradients, not one of the encoders' backward chains (batch-reduce
  // convolution weight gradients, small outputs)
  const bool big_single = g.kbatch == 1 && (long)g.M * g.N >= 400000;
  // direct = 5: only the chain products.  They run BESIDE the decoder's resident LDS-tiled stream-K workgroups (101 VGPRs x 4 per
  // SIMD, 135 of 160 KB LDS), where a kernel that needs no LDS and <= 108 VGPRs is the one that still gets a wave per SIMD
  p.use = r.direct != 0 && !(r.direct == 5 && big_single) && g.sam == 1 && g.sbn == 1 && g.scn == 1 && g.K % 2 == 0 && g.K >= 64 &&
          g.M >= 64 && g.N >= 64 && ((long)g.M + g.sak) * 4 < (1L << 31) && ((long)g.N + g.sbk) * 4 < (1L << 31);
  p.big = r.direct == 2 || (r.direct == 1 && tn_big_output(g.M, g.N));      // (3, 5: 64 x 64)
  // shield = 2: only the big single-segment products (on the second queue); the chain products stay the kind that fits in beside
  // other queues' workgroups
  p.shield = r.shield == 1 || (r.shield == 2 && big_single);
  // (deeper than 8 was measured under the shield -- 10 / 12 / 16 pairs: nothing; the wait counter's 6 bits end at (D - 1) x 6 <= 63)
  p.depth = tn_depth(r.depth);
  return direct_grid(p, g, ncu, wgs_option, r.reserve);
}
// whether some product routed by r gets the variant (big, shield) -- what zeggs_gemm_direct_warm checks ahead of time
inline bool route_selects(const TnRoute& r, bool big, bool shield) {
  const bool tile = r.direct == 1 || (r.direct == 2 ? big : r.direct != 0 && !big);
  return tile && (r.shield == 2 || (r.shield == 1) == shield);
}
// a variant by name (the first-use check of one, zeggs_gemm_direct_warm): no grid
inline DirectPlan direct_variant(bool big, int depth, bool shield) {
  DirectPlan p{};
  p.use = true; p.big = big; p.shield = shield; p.depth = tn_depth(depth);
  return p;
}

// First use of a variant on this process.  The kernel's operand loads are inline asm the compiler cannot see into, so a variant is
// CHECKED where it runs before it is trusted.  The outcomes of a check:
//   AGREES       the variant is OK from now on (one acquire load per product, no lock)
//   MISMATCH     the variant is BAD and the direct kernel is disabled for the process
//   UNAVAILABLE  the check itself could not run (an allocation, copy, launch or synchronise call failed): this one product goes
//                to the LDS-tiled kernel, the variant stays UNCHECKED and the next product tries again
enum class DirectCheck { AGREES, MISMATCH, UNAVAILABLE };
enum { DIRECT_UNCHECKED = -1, DIRECT_BAD = 0, DIRECT_OK = 1 };      // what zeggs_gemm_direct_state returns
struct DirectFirstUse {
  std::atomic<int> state[2][3][2];      // [128 x 64 wave tile][depth 4 / 6 / 8][shield]
  std::atomic<bool> disabled{false};
  std::mutex mu;                        // one check at a time; the states only change under it
  DirectFirstUse() {
    for (auto& b : state) for (auto& d : b) for (auto& s : d) s.store(DIRECT_UNCHECKED, std::memory_order_relaxed);
  }
  std::atomic<int>& at(bool big, int depth, bool shield) { return state[big][tn_depth(depth) / 2 - 2][shield]; }
  // true: launch p.  capturing(): the caller's stream is in a capture, where nothing can be checked (the check synchronises) -- the
  // variant runs unchecked and stays UNCHECKED.  check(p) runs the variant once on memory of its own.
  // Cost to know about: capturing() is asked under the lock, after the re-read, so a product captured while its variant is still
  // UNCHECKED takes the mutex on every launch and may wait behind another thread's check (which ends in a device-synchronising
  // free); zeggs_gemm_direct_warm before the capture leaves it the lock-free load.
  template <class Capturing, class Check>
  bool go(const DirectPlan& p, Capturing&& capturing, Check&& check) {
    std::atomic<int>& st = at(p.big, p.depth, p.shield);
    if (st.load(std::memory_order_acquire) == DIRECT_OK) return true;
    std::lock_guard<std::mutex> lock(mu);
    const int now = st.load(std::memory_order_relaxed);
    if (now == DIRECT_OK) return true;
    if (now == DIRECT_BAD || disabled.load(std::memory_order_relaxed)) return false;
    if (capturing()) return true;
    switch (check(p)) {
      case DirectCheck::AGREES: st.store(DIRECT_OK, std::memory_order_release); return true;
      case DirectCheck::UNAVAILABLE: return false;
      case DirectCheck::MISMATCH: break;
    }
    st.store(DIRECT_BAD, std::memory_order_release);
    disabled.store(true, std::memory_order_release);
    fprintf(stderr, "zeggs: the direct TN GEMM kernel is DISABLED for this process (self-test failed: built with another compiler?); "
                    "the LDS-tiled stream-K kernel takes its products\n");
    return false;
  }
};
