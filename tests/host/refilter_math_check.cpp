// Host check of csrc/refilter_math.h, the counting and layout rules of the filter stage of the re-timing output head of live
// serving (csrc/live_refilter.hip):
//   1. the ratio check of a filtered row: what the unfiltered head refuses is refused with its reason, L above 1024 and M above
//      4 L with theirs; H = ceil(Z max(L, M) / L) is Z at or above the server's rate, 10 at 24 from 60 with Z = 4, never above 32;
//   2. the counting rule for every ratio class: nf is monotone and 0 up to H input frames; the frames emitted after n inputs
//      are exactly those whose last tap k + H is below n; nf(n) plus a tail that is never negative is rt_n_out(n), what a final
//      record brings the stream to; the counts of any cut add up;
//   3. the ring: a stream is walked in calls of 1 .. 20 frames (fixed and pseudo-random cuts, with a final record that brings
//      no frame or some), for H = 1 .. 32, max_half = H and 32, every ratio class: every tap of every output reads, through
//      rf_tap_frame and rf_where, a frame of the call that is in the call or a ring slot that holds exactly the frame it wants
//      (the coverage claim: k + H >= n_in, so k - H >= n_in - 2 H); the ring is written behind the outputs, from rf_first_kept on;
//   4. the state: the plain head's row, then the ring, 2 max_half raw frames, rows on 8-byte boundaries; the LDS need is the
//      unfiltered head's.
// With --table it also prints the rule's values for tests/test_live_refilter_cpu.py, which compares them with its own
// restatement.  Exits non-zero at the first difference.  Built and run by that test, once more under the address and
// undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ubisoft-laforge-zeroeggs_amd/csrc/refilter_math.h"

#define EXPECT(cond, ...)                                                 \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "refilter_math_check: %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                       \
      fprintf(stderr, "  [%s]\n", #cond);                                 \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

namespace {

// every allowed class: down by an integer, down by a fraction, NTSC, the server's own rate, up by a fraction, up by an integer,
// the corners L = 1024 and M = 4 L
const long RATIOS[][2] = {{2, 5}, {1, 2}, {500, 1001}, {3, 2}, {2, 1}, {1, 1}, {1, 4}, {5, 12}, {8, 1}, {1024, 1023}, {1023, 1024}, {1024, 4095}, {6, 5}};
const int NRATIOS = sizeof(RATIOS) / sizeof(RATIOS[0]);

void check_ratios() {
  for (int r = 0; r < NRATIOS; ++r) EXPECT(rf_ratio_refused(RATIOS[r][0], RATIOS[r][1]) == 0, "%ld / %ld is refused\n", RATIOS[r][0], RATIOS[r][1]);
  EXPECT(rf_ratio_refused(0, 1) == 1 && rf_ratio_refused(1, 0) == 2 && rf_ratio_refused(2, 4) == 3 && rf_ratio_refused(9, 1) == 4, "the unfiltered reasons\n");
  EXPECT(rf_ratio_refused(1025, 1024) == 5 && rf_ratio_refused(2000, 1001) == 5 && rf_ratio_refused(1024, 1023) == 0, "L above 1024\n");
  EXPECT(rf_ratio_refused(1, 5) == 6 && rf_ratio_refused(2, 9) == 6 && rf_ratio_refused(1, 4) == 0 && rf_ratio_refused(400, 1001) == 0, "M above 4 L\n");
  EXPECT(rf_half(2, 5, 4) == 10 && rf_half(1, 2, 4) == 8 && rf_half(500, 1001, 4) == 9 && rf_half(1, 1, 4) == 4 && rf_half(2, 1, 4) == 4 &&
             rf_half(3, 2, 4) == 4 && rf_half(1, 4, 8) == 32 && rf_half(1, 4, 4) == 16 && rf_half(5, 12, 4) == 10,
         "the half widths DESIGN.md states\n");
  for (int r = 0; r < NRATIOS; ++r)
    for (int Z = 1; Z <= RF_MAX_Z; ++Z) {
      const int H = rf_half(RATIOS[r][0], RATIOS[r][1], Z);
      EXPECT(H >= Z && H <= RF_MAX_HALF && rf_half_fits(RATIOS[r][0], RATIOS[r][1], H) && rf_taps(H) == 2 * H + 1, "%ld / %ld Z %d: H %d\n",
             RATIOS[r][0], RATIOS[r][1], Z, H);
    }
  EXPECT(!rf_half_fits(2, 5, 9) && !rf_half_fits(1, 1, 9) && !rf_half_fits(2, 1, 0) && rf_half_fits(2, 5, 3), "halves that no Z gives\n");
}

void check_counting() {
  for (int r = 0; r < NRATIOS; ++r) {
    const long L = RATIOS[r][0], M = RATIOS[r][1];
    for (int H = 1; H <= RF_MAX_HALF; ++H) {
      long before = 0;
      for (long n = 0; n <= 400; ++n) {
        const long N = rf_n_out(n, L, M, H);
        EXPECT(N >= before && (n > H || N == 0), "%ld / %ld H %d: nf(%ld) = %ld after %ld\n", L, M, H, n, N, before);
        long k, num;
        if (N > 0) {
          rt_position(N - 1, L, M, &k, &num);
          EXPECT(k + H <= n - 1, "%ld / %ld H %d: frame %ld needs input %ld of %ld\n", L, M, H, N - 1, k + H, n);
        }
        rt_position(N, L, M, &k, &num);
        EXPECT(k + H >= n, "%ld / %ld H %d: frame %ld was computable with %ld inputs\n", L, M, H, N, n);
        const long tail = rt_n_out(n, L, M) - N;
        EXPECT(tail >= 0 && rf_emitted(n, L, M, H, 1) == N + tail && rf_emitted(n, L, M, H, 0) == N, "%ld / %ld H %d: tail %ld at %ld\n", L, M, H, tail, n);
        before = N;
      }
    }
  }
  EXPECT(rf_n_out(10, 2, 5, 10) == 0 && rf_n_out(11, 2, 5, 10) == 1 && rf_n_out(48, 2, 5, 10) == 16 && rt_n_out(48, 2, 5) == 19, "24 from 60\n");
  EXPECT(rf_n_out((1L << 40) + 20, 1024, 4095, 32) - rf_n_out(1L << 40, 1024, 4095, 32) <= rt_max_outputs(20, 1024, 4095), "far into a stream\n");
}

// one stream through the ring: frames are their own index; -1 marks a slot never written
void walk(long L, long M, int H, int max_half, const std::vector<int>& cuts, bool final_empty) {
  const int D = rf_ring_frames(max_half);
  std::vector<long> ring(D, -1);
  long n_in = 0, emitted = 0;
  const size_t calls = cuts.size() + (final_empty ? 1 : 0);
  for (size_t c = 0; c < calls; ++c) {
    const long count = c < cuts.size() ? cuts[c] : 0;
    const int final = c + 1 == calls;
    const long n1 = n_in + count, last = n1 - 1;
    const long m1 = rf_emitted(n1, L, M, H, final);
    EXPECT(emitted == rf_n_out(n_in, L, M, H) && m1 >= emitted, "%ld / %ld H %d: counters\n", L, M, H);
    for (long m = emitted; m < m1; ++m) {
      long k, num;
      rt_position(m, L, M, &k, &num);
      EXPECT(k + H >= n_in && k <= last && num >= 0 && num < L, "%ld / %ld H %d: output %ld at %ld with %ld earlier frames\n", L, M, H, m, k, n_in);
      for (int j = 0; j < rf_taps(H); ++j) {
        const long i = rf_tap_frame(k, H, j, last);
        const long want = k - H + j < 0 ? 0 : (k - H + j > last ? last : k - H + j);
        EXPECT(i == want && i >= 0 && i <= last && (final || k - H + j <= last), "%ld / %ld H %d: tap %d of output %ld\n", L, M, H, j, m);
        const long at = rf_where(i, n_in, max_half);
        if (at >= 0) {
          EXPECT(at < count && n_in + at == i, "%ld / %ld H %d: tap %d of output %ld reads frame %ld of a call of %ld\n", L, M, H, j, m, at, count);
        } else {
          const long slot = -1 - at;
          EXPECT(slot >= 0 && slot < D && ring[slot] == i, "%ld / %ld H %d max_half %d: tap %d of output %ld wants frame %ld, slot %ld holds %ld\n", L, M,
                 H, max_half, j, m, i, slot, slot >= 0 && slot < D ? ring[slot] : -2);
        }
      }
    }
    // behind the last pass: the call's frames enter the ring
    for (long f = rf_first_kept(count, max_half); f < count; ++f) ring[rf_slot(n_in + f, max_half)] = n_in + f;
    for (long i = n1 - 1; i >= 0 && i >= n1 - D; --i) EXPECT(ring[rf_slot(i, max_half)] == i, "the ring holds the last %d frames\n", D);
    n_in = n1;
    emitted = m1;
  }
  EXPECT(emitted == rt_n_out(n_in, L, M), "%ld / %ld H %d: a closed stream has %ld frames, not %ld\n", L, M, H, rt_n_out(n_in, L, M), emitted);
}

void check_ring() {
  unsigned long long s = 99;
  for (int r = 0; r < NRATIOS; ++r)
    for (int H = 1; H <= RF_MAX_HALF; ++H)
      for (int max_half : {H, RF_MAX_HALF}) {
        const long L = RATIOS[r][0], M = RATIOS[r][1];
        for (int c = 1; c <= 20; ++c) {
          walk(L, M, H, max_half, std::vector<int>(100 / c + 1, c), true);
          walk(L, M, H, max_half, std::vector<int>(100 / c + 1, c), false);
        }
        std::vector<int> cuts;
        for (int i = 0; i < 40; ++i) {
          s = s * 6364136223846793005ULL + 1442695040888963407ULL;
          cuts.push_back(1 + (int)((s >> 33) % 20));
        }
        walk(L, M, H, max_half, cuts, (s >> 40) & 1);
        walk(L, M, H, max_half, {1}, true);      // a stream of one frame: everything is the tail
        walk(L, M, H, max_half, {3}, false);
      }
  EXPECT(rf_slot(-1, 4) == 7 && rf_slot(0, 4) == 0 && rf_slot(8, 4) == 0 && rf_slot(13, 4) == 5, "slots\n");
  EXPECT(rf_first_kept(20, 4) == 12 && rf_first_kept(8, 4) == 0 && rf_first_kept(0, 4) == 0, "a call longer than the ring\n");
}

void check_state() {
  for (int J : {1, 2, 5, 75, 1024})
    for (int mh : {1, 4, 10, 16, 32}) {
      EXPECT(rf_row_ring_offset(J) == fr_row_bytes(J) && rf_row_ring_offset(J) % 8 == 0 && rf_row_bytes(J, mh) % 8 == 0, "J = %d: row bytes\n", J);
      EXPECT(rf_ring_bytes(J, mh) == 2L * mh * rt_raw_floats(J) * 4, "J = %d: %d raw frames\n", J, 2 * mh);
      EXPECT(rf_row_offset(J, mh, 0) == fr_tables_bytes(J) && rf_row_offset(J, mh, 3) - rf_row_offset(J, mh, 2) == rf_row_bytes(J, mh), "J = %d: rows\n", J);
      EXPECT(rf_state_bytes(64, J, mh) == rf_row_offset(J, mh, 64), "J = %d: state bytes\n", J);
    }
  EXPECT(rf_row_bytes(75, 16) == 120 + 2416 + 32 * 2728 && rf_state_bytes(4, 5, 10) == 64 + 4 * (296 + 20 * 208), "the sizes DESIGN.md states\n");
  EXPECT(rf_pass_frames(75, 20) == rt_pass_frames(75, 20) && rf_lds_bytes(5, 20) == rt_lds_bytes(5, 20) && rf_lds_bytes(75, 20) <= FR_LDS_BYTES, "the LDS\n");
}

void table() {
  for (int r = 0; r < NRATIOS; ++r) {
    const long L = RATIOS[r][0], M = RATIOS[r][1];
    for (int Z : {1, 4, 8}) {
      const int H = rf_half(L, M, Z);
      printf("ratio %ld %ld %d %d |", L, M, Z, H);
      for (long n = 0; n <= 60; ++n) printf(" %ld", rf_n_out(n, L, M, H));
      printf("\n");
    }
  }
  for (int J : {1, 5, 75})
    for (int mh : {4, 10, 16}) printf("state %d %d %ld %ld\n", J, mh, rf_row_bytes(J, mh), rf_state_bytes(64, J, mh));
}

}  // namespace

int main(int argc, char** argv) {
  check_ratios();
  check_counting();
  check_ring();
  check_state();
  if (argc > 1 && strcmp(argv[1], "--table") == 0) table();
  printf("refilter_math_check: ok\n");
  return 0;
}
