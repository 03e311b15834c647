// Host check of csrc/retime_math.h, the counting and layout rules of the re-timing output head of live serving
// (csrc/live_retime.hip):
//   1. the ratio check: the frame rates the head is for (24 .. 480 and the NTSC rates against 60) reduce to the documented L / M
//      and pass; L or M out of 1 .. 4096, a ratio that is not in lowest terms and a ratio above 8 are refused, each with its reason;
//   2. the counting rule for every ratio of the tests: n_out is monotone and n_out(1) = 1; the frames emitted after n inputs are
//      exactly those whose last needed input is below n (the last one emitted needs no input >= n, the next one does); the
//      counts of any cut of the inputs into calls add up to n_out(n); a call of c inputs never emits more than rt_max_outputs(c);
//      position(m) is k + num / L with 0 <= num < L, and num == 0 exactly when m M is a multiple of L;
//   3. the state: the plain head's row, then the raw frame, its four fields tiling 7 + 9J floats, rows on 8-byte boundaries;
//   4. the LDS need: never more than 64 KB, 15 frames a pass for 75 joints as the plain head, and for small skeletons never more
//      frames than the largest ratio can give a record;
//   5. the interpolation weights: for unit quaternions an angle theta apart the weighted sum is a unit quaternion at t theta from
//      the near end; below the small-sine threshold the weights are 1 - t and t; a dot product a rounding above 1 is taken as 1.
// With --table it also prints the rule's values for tests/test_live_retime_cpu.py, which compares them with its own restatement.
// Exits non-zero at the first difference.  Built and run by that test, once more under the address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ubisoft-laforge-zeroeggs_amd/csrc/retime_math.h"

#define EXPECT(cond, ...)                                               \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "retime_math_check: %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                     \
      fprintf(stderr, "  [%s]\n", #cond);                               \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

namespace {

const long RATIOS[][2] = {{1, 1}, {1, 2}, {2, 1}, {3, 2}, {2, 5}, {5, 12}, {500, 1001}, {8, 1}, {1, 7}, {1000, 1001}, {4096, 4095}, {1, 4096}};
const int NRATIOS = sizeof(RATIOS) / sizeof(RATIOS[0]);

void check_ratios() {
  // frame_rate (as a fraction) against 60 frames per second
  const long rates[][4] = {{24, 1, 2, 5},          {25, 1, 5, 12},           {30, 1, 1, 2},           {50, 1, 5, 6},
                           {72, 1, 6, 5},          {90, 1, 3, 2},            {120, 1, 2, 1},          {480, 1, 8, 1},
                           {24000, 1001, 400, 1001}, {30000, 1001, 500, 1001}, {60000, 1001, 1000, 1001}, {120000, 1001, 2000, 1001}};
  for (const auto& r : rates) {
    const long num = r[0], den = r[1] * 60, g = rt_gcd(num, den);
    EXPECT(num / g == r[2] && den / g == r[3], "%ld / %ld fps reduces to %ld / %ld\n", r[0], r[1], num / g, den / g);
    EXPECT(rt_ratio_refused(r[2], r[3]) == 0, "%ld / %ld is refused\n", r[2], r[3]);
  }
  EXPECT(rt_ratio_refused(0, 1) == 1 && rt_ratio_refused(-1, 1) == 1 && rt_ratio_refused(4097, 4096) == 1, "L out of range\n");
  EXPECT(rt_ratio_refused(1, 0) == 2 && rt_ratio_refused(1, 4097) == 2 && rt_ratio_refused(3, -2) == 2, "M out of range\n");
  EXPECT(rt_ratio_refused(2, 4) == 3 && rt_ratio_refused(4096, 2) == 3, "not in lowest terms\n");
  EXPECT(rt_ratio_refused(9, 1) == 4 && rt_ratio_refused(17, 2) == 4 && rt_ratio_refused(8, 1) == 0 && rt_ratio_refused(4095, 512) == 0,
         "above 8\n");
  EXPECT(rt_ratio_refused(4096, 4095) == 0 && rt_ratio_refused(1, 4096) == 0, "the corners\n");
}

void check_counting() {
  for (int r = 0; r < NRATIOS; ++r) {
    const long L = RATIOS[r][0], M = RATIOS[r][1];
    EXPECT(rt_n_out(0, L, M) == 0 && rt_n_out(-3, L, M) == 0 && rt_n_out(1, L, M) == 1, "%ld / %ld: the first frames\n", L, M);
    long before = 0;
    for (long n = 1; n <= 3000; ++n) {
      const long N = rt_n_out(n, L, M);
      EXPECT(N >= before && N - before <= rt_max_outputs(1, L, M), "%ld / %ld: n_out(%ld) = %ld after %ld\n", L, M, n, N, before);
      EXPECT(rt_last_needed(N - 1, L, M) <= n - 1, "%ld / %ld: frame %ld needs input %ld of %ld\n", L, M, N - 1, rt_last_needed(N - 1, L, M), n);
      EXPECT(rt_last_needed(N, L, M) >= n, "%ld / %ld: frame %ld was computable with %ld inputs\n", L, M, N, n);
      before = N;
    }
    for (long m = 0; m <= 3000; ++m) {
      long k, num;
      rt_position(m, L, M, &k, &num);
      EXPECT(num >= 0 && num < L && k * L + num == m * M && (num == 0) == ((m * M) % L == 0), "%ld / %ld: position of %ld\n", L, M, m);
    }
    // cuts: pseudo-random call sizes 0 .. 21 add up, and no call emits more than its bound
    unsigned long long s = 12345 + r;
    long n = 0, total = 0;
    while (n < 5000) {
      s = s * 6364136223846793005ULL + 1442695040888963407ULL;
      const long c = (long)((s >> 33) % 22);
      const long got = rt_n_out(n + c, L, M) - rt_n_out(n, L, M);
      EXPECT(got >= 0 && got <= rt_max_outputs(c, L, M), "%ld / %ld: %ld inputs after %ld emit %ld\n", L, M, c, n, got);
      n += c;
      total += got;
    }
    EXPECT(total == rt_n_out(n, L, M), "%ld / %ld: the cuts add up to %ld, n_out(%ld) = %ld\n", L, M, total, n, rt_n_out(n, L, M));
    // far into a stream: 2^40 inputs at the largest terms stay inside 64 bits
    const long far = 1L << 40;
    EXPECT(rt_n_out(far + 20, L, M) - rt_n_out(far, L, M) <= rt_max_outputs(20, L, M), "%ld / %ld: far\n", L, M);
  }
  EXPECT(rt_max_outputs(20, 8, 1) == 161 && rt_max_outputs(20, 1, 2) == 11 && rt_max_outputs(0, 8, 1) == 0 && rt_max_outputs(1, 1, 7) == 2,
         "rt_max_outputs\n");
}

void check_state() {
  const int Js[] = {1, 2, 5, 75, 1024};
  for (int J : Js) {
    std::vector<int> used(rt_raw_floats(J), 0);
    auto mark = [&](int at, int n) {
      for (int i = 0; i < n; ++i) {
        EXPECT(at + i >= 0 && at + i < (int)used.size(), "J = %d: offset %d of %zu\n", J, at + i, used.size());
        used[at + i] += 1;
      }
    };
    mark(rt_raw_rpos(), 3);
    mark(rt_raw_rrot(), 4);
    for (int j = 0; j < J; ++j) {
      mark(rt_raw_lpos(j), 3);
      mark(rt_raw_ltxy(J, j), 6);
    }
    for (size_t i = 0; i < used.size(); ++i) EXPECT(used[i] == 1, "J = %d: raw float %zu belongs to %d fields\n", J, i, used[i]);
    // the raw lpos | ltxy block is a pose row's, one float earlier: what the kernel's copy relies on
    EXPECT(rt_raw_lpos(0) - 1 == fr_pose_lpos(0) && rt_raw_ltxy(J, J - 1) - 1 == fr_pose_ltxy(J, J - 1), "J = %d: raw against pose\n", J);
    EXPECT(rt_row_raw_offset(J) == fr_row_bytes(J) && rt_row_raw_offset(J) % 8 == 0 && rt_row_bytes(J) % 8 == 0, "J = %d: row bytes\n", J);
    EXPECT(rt_row_bytes(J) >= fr_row_bytes(J) + 4L * rt_raw_floats(J) && rt_row_bytes(J) < fr_row_bytes(J) + 4L * rt_raw_floats(J) + 8, "J = %d\n", J);
    EXPECT(rt_row_offset(J, 0) == fr_tables_bytes(J) && rt_row_offset(J, 3) - rt_row_offset(J, 2) == rt_row_bytes(J), "J = %d: rows\n", J);
    EXPECT(rt_state_bytes(64, J) == rt_row_offset(J, 64), "J = %d: state bytes\n", J);
  }
  EXPECT(rt_state_bytes(4, 5) == 64 + 4 * (296 + 208) && rt_row_bytes(75) == 120 + 2416 + 2728, "the sizes DESIGN.md states\n");
}

void check_lds() {
  EXPECT(rt_pass_frames(75, 20) == 15 && rt_pass_frames(75, 20) == fr_pass_frames(75, 20), "75 joints: 15 frames a pass\n");
  EXPECT(rt_pass_frames(1, 20) == 161 && rt_pass_frames(5, 20) == 161 && rt_pass_frames(5, 1) == 9, "small skeletons: what 8 / 1 can give\n");
  for (int J = 1; J <= FR_MAX_JOINTS; ++J)
    for (int mf : {1, 20, 4096}) {
      if (fr_shape_refused(J, mf) != 0) continue;
      EXPECT(rt_pass_frames(J, mf) >= 1 && rt_lds_bytes(J, mf) <= FR_LDS_BYTES, "J = %d, max_frames = %d: %ld bytes\n", J, mf, rt_lds_bytes(J, mf));
      EXPECT(rt_lds_bytes(J, mf) == rt_pass_frames(J, mf) * 56L * (J + 1), "J = %d: 56 bytes a slot\n", J);
    }
}

void check_weights() {
  const double thetas[] = {1e-7, 1e-3, 0.125, 1.0, 1.5707963267948966};      // half the rotation angle between the two ends
  const double ts[] = {0.5, 1.0 / 3.0, 0.999, 1.0 / 1001.0};
  for (double th : thetas)
    for (double t : ts) {
      // a = (1, 0), b = (cos th, sin th) in the plane they span
      double wa, wb;
      rt_slerp_weights(cos(th), t, &wa, &wb);
      const double x = wa + wb * cos(th), y = wb * sin(th);
      EXPECT(fabs(sqrt(x * x + y * y) - 1.0) < 1e-12, "theta %g, t %g: norm %.17g\n", th, t, sqrt(x * x + y * y));
      EXPECT(fabs(atan2(y, x) - t * th) < 1e-12, "theta %g, t %g: angle %.17g\n", th, t, atan2(y, x));
    }
  double wa, wb;
  rt_slerp_weights(1.0, 0.25, &wa, &wb);
  EXPECT(wa == 0.75 && wb == 0.25, "d = 1\n");
  rt_slerp_weights(1.0 + 1e-15, 0.25, &wa, &wb);
  EXPECT(wa == 0.75 && wb == 0.25, "d above 1\n");
  rt_slerp_weights(cos(5e-9), 0.25, &wa, &wb);      // sine 5e-9 < 1e-8
  EXPECT(wa == 0.75 && wb == 0.25, "below the threshold\n");
  rt_slerp_weights(0.0, 0.5, &wa, &wb);             // a quarter turn of the quaternion: half a turn of the rotation
  EXPECT(fabs(wa - sqrt(0.5)) < 1e-15 && fabs(wb - sqrt(0.5)) < 1e-15, "d = 0\n");
}

void table() {
  for (int r = 0; r < NRATIOS; ++r) {
    const long L = RATIOS[r][0], M = RATIOS[r][1];
    printf("ratio %ld %ld", L, M);
    for (long n = 0; n <= 45; ++n) printf(" %ld", rt_n_out(n, L, M));
    printf(" |");
    for (long m = 0; m <= 30; ++m) {
      long k, num;
      rt_position(m, L, M, &k, &num);
      printf(" %ld:%ld", k, num);
    }
    printf(" | %ld\n", rt_max_outputs(20, L, M));
  }
  for (int J : {1, 5, 75}) printf("state %d %ld %ld %d %ld\n", J, rt_row_bytes(J), rt_state_bytes(64, J), rt_pass_frames(J, 20), rt_lds_bytes(J, 20));
}

}  // namespace

int main(int argc, char** argv) {
  check_ratios();
  check_counting();
  check_state();
  check_lds();
  check_weights();
  if (argc > 1 && strcmp(argv[1], "--table") == 0) table();
  printf("retime_math_check: ok\n");
  return 0;
}
