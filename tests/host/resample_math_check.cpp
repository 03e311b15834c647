// Host check of csrc/resample_math.h, the index rules of the rate converter of live serving (csrc/live_resample.hip):
//   1. the reduced ratio of every supported rate -> 16 kHz, and the refusal of what lies outside (L > 640, M / L > 24);
//   2. rs_ready / rs_total against brute force over the support rule |P_m - k L| < WL, for 3:1, 441:160, 1:2, 441:320, 2:1, 3:2
//      and the pass-through, Z = 4 and 64, n = 0 .. 3000; the tap range of every phase against a scan of the whole table row;
//      the tiles of the kernel: rs_first_tap / rs_last_tap grow with m, and rs_tile_outputs consecutive outputs touch at most
//      RS_SPAN inputs, for every supported decimation at 64 zero crossings;
//   3. the kernel's walk -- per push every output from rs_ready(n) to rs_ready(n + count), every tap either in this push's
//      source or in the ring of the last rs_history inputs, the ring moved only after the push's outputs -- over signals cut into
//      pushes of 1, 2, 7, 95, 96, 1000 samples and a mixed sequence: every ring slot an output reads holds exactly the sample it
//      wants, no source index leaves the push, the outputs are 0, 1, 2, ... without gap, and the final flush ends at rs_total.
// Exits non-zero at the first difference.  Built and run by tests/test_live_resample_cpu.py, once more under the address and
// undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ubisoft-laforge-zeroeggs_amd/csrc/resample_math.h"

#define EXPECT(cond, ...)                                                 \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "resample_math_check: %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                       \
      fprintf(stderr, "  [%s]\n", #cond);                                 \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

namespace {

struct Ratio { int L, M; };
const Ratio RATIOS[] = {{1, 3}, {160, 441}, {2, 1}, {320, 441}, {1, 2}, {2, 3}};
const long PUSHES[] = {1, 2, 7, 95, 96, 1000};

uint64_t rnd(uint64_t* s) {
  *s ^= *s << 13; *s ^= *s >> 7; *s ^= *s << 17;
  return *s;
}

void check_ratios() {
  const struct { long fi; int L, M; } want[] = {{8000, 2, 1}, {11025, 640, 441}, {12000, 4, 3}, {22050, 320, 441}, {24000, 2, 3},
                                                {32000, 1, 2}, {44100, 160, 441}, {48000, 1, 3}, {88200, 80, 441}, {96000, 1, 6},
                                                {192000, 1, 12}, {384000, 1, 24}, {16000, 1, 1}};
  for (const auto& w : want) {
    int L = 0, M = 0;
    EXPECT(rs_ratio(w.fi, 16000, &L, &M) && L == w.L && M == w.M, "%ld Hz: %d / %d\n", w.fi, L, M);
  }
  int L, M;
  EXPECT(!rs_ratio(400000, 16000, &L, &M), "M / L = 25\n");
  EXPECT(!rs_ratio(16001, 16000, &L, &M), "L = 16000\n");
  EXPECT(!rs_ratio(0, 16000, &L, &M) && !rs_ratio(16000, -1, &L, &M), "a rate that is not positive\n");
  EXPECT(rs_wl(64, 1, 3) == 192 && rs_taps(192, 1) == 385 && rs_history(192, 1) == 384, "48 kHz: 385 taps\n");
  EXPECT(rs_wl(64, 2, 1) == 128 && rs_taps(128, 2) == 129 && rs_history(128, 2) == 128, "8 kHz\n");
  EXPECT(rs_taps(0, 1) == 1 && rs_history(0, 1) == 0, "pass-through\n");
}

bool in_support(long m, long k, int L, int M, long WL) {
  const long d = m * (long)M - k * (long)L;
  return WL == 0 ? d == 0 : (d < WL && -d < WL);
}

long check_counts(int L, int M, int Z) {
  const long WL = Z == 0 ? 0 : rs_wl(Z, L, M);
  const int H = rs_half(WL, L), taps = rs_taps(WL, L);
  EXPECT((long)H * L >= WL && (long)(H - 1) * L < WL && taps == 2 * H + 1, "%d / %d: half width %d\n", L, M, H);
  // the tap range of every phase against a scan of the row
  for (int ph = 0; ph < L; ++ph) {
    int j0, j1, lo = -1, hi = -1;
    rs_tap_range(ph, L, WL, &j0, &j1);
    for (int j = 0; j < taps; ++j) {
      const long d = ph + (long)(H - j) * L;      // (P_m - k L) of tap j
      if (WL == 0 ? d == 0 : (d < WL && -d < WL)) { if (lo < 0) lo = j; hi = j; }
    }
    EXPECT(j0 == lo && j1 == hi && j0 >= 0 && j1 < taps, "%d / %d phase %d: taps %d .. %d, scan %d .. %d\n", L, M, ph, j0, j1, lo, hi);
  }
  long m_ready = 0, m_total = 0, checked = 0;
  for (long n = 0; n <= 3000; ++n, ++checked) {
    // brute force: m is ready once its last tap is below n (then so is every tap), and the ready outputs are a prefix
    while (true) {
      long last = (m_ready * M) / L + H + 1;
      while (!in_support(m_ready, last, L, M, WL)) --last;
      if (last >= n) break;
      ++m_ready;
    }
    while (m_total * (long)M < n * (long)L) ++m_total;      // p_m < n
    EXPECT(rs_ready(n, L, M, WL) == m_ready, "%d / %d Z %d: ready(%ld) = %ld, brute force %ld\n", L, M, Z, n, rs_ready(n, L, M, WL), m_ready);
    EXPECT(rs_total(n, L, M) == m_total, "%d / %d: total(%ld) = %ld, brute force %ld\n", L, M, n, rs_total(n, L, M), m_total);
    EXPECT(m_ready <= m_total, "%d / %d: more ready than there are\n", L, M);
  }
  for (long m = 0; m < 500; ++m) {
    const long a = rs_first_tap(m, L, M, WL), b = rs_last_tap(m, L, M, WL);
    EXPECT(in_support(m, a, L, M, WL) && in_support(m, b, L, M, WL) && !in_support(m, a - 1, L, M, WL) && !in_support(m, b + 1, L, M, WL),
           "%d / %d output %ld: taps %ld .. %ld\n", L, M, m, a, b);
  }
  // the tiles: both ends of the support grow with m, and a full tile's span fits the staging area
  const int tile = rs_tile_outputs(L, M, WL);
  EXPECT(tile >= 1 && tile <= RS_THREADS, "%d / %d Z %d: %d outputs per tile\n", L, M, Z, tile);
  for (long m = 0; m < 3000; ++m) {
    EXPECT(rs_first_tap(m + 1, L, M, WL) >= rs_first_tap(m, L, M, WL) && rs_last_tap(m + 1, L, M, WL) >= rs_last_tap(m, L, M, WL),
           "%d / %d output %ld: the support moves backwards\n", L, M, m);
    const long span = rs_last_tap(m + tile - 1, L, M, WL) - rs_first_tap(m, L, M, WL) + 1;
    EXPECT(span >= 1 && span <= RS_SPAN, "%d / %d Z %d tile at %ld: %ld inputs\n", L, M, Z, m, span);
  }
  return checked;
}

// one push of `count` inputs on a row that has n_in inputs and n_out outputs: the reads of the kernel, then the ring update
void walk_push(int L, int M, long WL, long count, bool final, long* n_in_, long* n_out_, std::vector<long>* ring, long* reads) {
  const long n_in = *n_in_, n_out = *n_out_, n1 = n_in + count;
  const int HL = rs_history(WL, L), H = rs_half(WL, L);
  EXPECT(n_out == rs_ready(n_in, L, M, WL), "%d / %d: %ld outputs after %ld inputs\n", L, M, n_out, n_in);
  const long due = (final ? rs_total(n1, L, M) : rs_ready(n1, L, M, WL)) - n_out;
  EXPECT(due >= 0, "%d / %d: %ld outputs due\n", L, M, due);
  for (long i = 0; i < due; ++i) {
    const long m = n_out + i;
    long q; int ph, j0, j1;
    rs_position(m, L, M, &q, &ph);
    rs_tap_range(ph, L, WL, &j0, &j1);
    EXPECT(ph >= 0 && ph < L && q * L + ph == m * (long)M, "%d / %d output %ld: position\n", L, M, m);
    long k = q - H + j0;
    for (int j = j0; j <= j1; ++j, ++k, ++*reads) {
      if (k < 0) continue;
      if (k < n_in) {
        EXPECT(HL > 0 && k >= n_in - HL && (*ring)[(size_t)rs_slot(k, HL)] == k, "%d / %d output %ld: sample %ld is not in the history after %ld\n",
               L, M, m, k, n_in);
      } else {
        EXPECT(k - n_in < count || final, "%d / %d output %ld: sample %ld has not arrived (%ld + %ld)\n", L, M, m, k, n_in, count);
      }
    }
  }
  if (HL > 0)      // after ALL outputs: the last HL inputs
    for (long k = n1 - HL > n_in ? n1 - HL : n_in; k < n1; ++k) (*ring)[(size_t)rs_slot(k, HL)] = k;
  *n_in_ = n1;
  *n_out_ = n_out + due;
}

long check_cuts(int L, int M, int Z) {
  const long WL = Z == 0 ? 0 : rs_wl(Z, L, M), N = 5000;
  long reads = 0;
  for (int c = 0; c <= (int)(sizeof(PUSHES) / sizeof(PUSHES[0])); ++c) {
    const bool mixed = c == (int)(sizeof(PUSHES) / sizeof(PUSHES[0]));
    std::vector<long> ring((size_t)rs_history(WL, L) + 1, -1);
    long n_in = 0, n_out = 0;
    uint64_t seed = 0x9E3779B97F4A7C15ull + (uint64_t)(L * 1000 + M);
    while (n_in < N) {
      long m = mixed ? PUSHES[rnd(&seed) % 6] : PUSHES[c];
      if (m > N - n_in) m = N - n_in;
      walk_push(L, M, WL, m, false, &n_in, &n_out, &ring, &reads);
    }
    walk_push(L, M, WL, 0, true, &n_in, &n_out, &ring, &reads);
    EXPECT(n_in == N && n_out == rs_total(N, L, M), "%d / %d cut %d: %ld outputs of %ld inputs\n", L, M, c, n_out, n_in);
  }
  return reads;
}

}  // namespace

int main() {
  check_ratios();
  long counts = 0, reads = 0;
  for (const Ratio& r : RATIOS)
    for (int Z : {4, 64}) {
      counts += check_counts(r.L, r.M, Z);
      reads += check_cuts(r.L, r.M, Z);
    }
  for (int M = 1; M <= RS_MAX_DECIMATION; ++M) counts += check_counts(1, M, 64);      // (every decimation: the tiles at their widest)
  counts += check_counts(RS_MAX_L, RS_MAX_L * RS_MAX_DECIMATION - 1, 64) + check_counts(RS_MAX_L, 1, 64);
  counts += check_counts(1, 1, 0);
  reads += check_cuts(1, 1, 0);
  EXPECT(rs_ready(1L << 40, 160, 441, rs_wl(64, 160, 441)) == ((1L << 40) * 160 - 64 * 441) / 441 + 1, "64-bit positions\n");
  printf("13 rates, %ld counts, %ld tap reads\n", counts, reads);
  printf("resample_math_check: ok\n");
  return 0;
}
