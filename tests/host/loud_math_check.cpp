// Host check of csrc/loud_math.h, the index and gate rules of the running loudness estimate (csrc/live_loudness.hip):
//   1. the block table at 16 / 22.05 / 44.1 / 48 kHz: lo_j = j fs / 10, one block length, strictly increasing ends (200 000 blocks);
//   2. the kernel's walk -- runs that end where the next block completes, the ring of filtered samples written slot by slot --
//      over a 3-second index range cut into pushes of 1, 7, 1599, 1600, 1601, 3200, 6400, 9000 samples and into a mixed sequence
//      of those: the blocks that complete, their order, the ring slots their energy reads (each must hold exactly the sample the
//      block wants), the index at which the gain switches and the energy-ring slot written are those of the cut-free statement,
//      and the carried block counter equals loud_blocks_done after every push;
//   3. the two gates as the kernel evaluates them (256 strided partial sums and the tree, over a ring) against a direct two-pass
//      evaluation over the plain list of the last NB energies: the same blocks pass, the same count, sums and estimate to 1e-12
//      relative, the same decision to keep the gain.
// Exits non-zero at the first difference.  Built and run by tests/test_live_loudness_cpu.py, once more under the address and
// undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ubisoft-laforge-zeroeggs_amd/csrc/loud_math.h"

#define EXPECT(cond, ...)                                             \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "loud_math_check: %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                   \
      fprintf(stderr, "  [%s]\n", #cond);                             \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

namespace {

const int RATES[] = {16000, 22050, 44100, 48000};
const long PUSHES[] = {1, 7, 1599, 1600, 1601, 3200, 6400, 9000};

struct Event {      // one completed block as the walk saw it
  long j, first, hi, yslot_first, zslot;
  bool operator==(const Event& o) const { return j == o.j && first == o.first && hi == o.hi && yslot_first == o.yslot_first && zslot == o.zslot; }
};

uint64_t rnd(uint64_t* s) {
  *s ^= *s << 13; *s ^= *s >> 7; *s ^= *s << 17;
  return *s;
}

void check_table(int fs) {
  EXPECT(loud_rate_ok(fs, 200000), "fs %d\n", fs);
  const long len = loud_block_len(fs);
  EXPECT(len == (long)(0.4 * fs), "fs %d: block length %ld\n", fs, len);
  for (long j = 0; j < 200000; ++j) {
    EXPECT(loud_lo(j, fs) == j * fs / 10 && (j * (long)fs) % 10 == 0, "fs %d block %ld: lo %ld\n", fs, j, loud_lo(j, fs));
    EXPECT(loud_first(j, fs, len) == loud_lo(j, fs), "fs %d block %ld\n", fs, j);
  }
  EXPECT(!loud_rate_ok(5, 16), "a rate without blocks\n");
}

// the kernel's loop over one push of m samples on (n, j) and a ring of sample INDICES
void walk_push(int fs, int NB, long m, long* n_, long* j_, std::vector<long>* ring, std::vector<Event>* out) {
  const long len = loud_block_len(fs), n_end = *n_ + m;
  long n = *n_, j = *j_;
  while (n < n_end) {
    const long run_end = loud_run_end(j, n_end, fs);
    EXPECT(run_end > n && run_end <= n_end, "fs %d: run [%ld, %ld) of a push that ends at %ld\n", fs, n, run_end, n_end);
    for (long i = n; i < run_end; ++i) (*ring)[(size_t)loud_yslot(i, len)] = i;
    n = run_end;
    if (!loud_complete(j, n, fs)) break;
    EXPECT(n == loud_hi(j, fs), "fs %d block %ld: stopped at %ld\n", fs, j, n);
    const long first = loud_first(j, fs, len), hi = loud_hi(j, fs);
    long reads = 0;
    for (int t = 0; t < LOUD_THREADS; ++t)      // the slots loud_energy_partial reads, thread by thread
      for (long i = first + t; i < hi; i += LOUD_THREADS, ++reads)
        EXPECT((*ring)[(size_t)loud_yslot(i, len)] == i, "fs %d block %ld: slot %ld holds sample %ld, not %ld\n", fs, j, loud_yslot(i, len),
               (*ring)[(size_t)loud_yslot(i, len)], i);
    EXPECT(reads == hi - first && reads == len, "fs %d block %ld: %ld reads\n", fs, j, reads);
    out->push_back(Event{j, first, hi, loud_yslot(first, len), loud_zslot(j, NB)});
    ++j;
  }
  EXPECT(n == n_end, "fs %d: a push ended at %ld, not %ld\n", fs, n, n_end);
  EXPECT(j == loud_blocks_done(n, fs), "fs %d: %ld blocks counted after %ld samples, %ld by the table\n", fs, j, n, loud_blocks_done(n, fs));
  *n_ = n; *j_ = j;
}

long check_cuts(int fs) {
  const long N = 3L * fs;
  const int NB = 20;
  std::vector<Event> want;      // the cut-free statement: every block whose end lies inside the range, in order
  for (long j = 0; loud_hi(j, fs) <= N; ++j)
    want.push_back(Event{j, loud_lo(j, fs), loud_hi(j, fs), loud_lo(j, fs) % loud_block_len(fs), j % NB});
  EXPECT((long)want.size() == 27, "fs %d: %zu blocks in 3 s\n", fs, want.size());
  long walks = 0;
  for (int c = 0; c <= (int)(sizeof(PUSHES) / sizeof(PUSHES[0])); ++c) {
    const bool mixed = c == (int)(sizeof(PUSHES) / sizeof(PUSHES[0]));
    std::vector<long> ring((size_t)loud_block_len(fs), -1);
    std::vector<Event> got;
    long n = 0, j = 0;
    uint64_t seed = 0x9E3779B97F4A7C15ull + (uint64_t)fs;
    while (n < N) {
      long m = mixed ? PUSHES[rnd(&seed) % 8] : PUSHES[c];
      if (m > N - n) m = N - n;
      walk_push(fs, NB, m, &n, &j, &ring, &got);
    }
    EXPECT(got.size() == want.size(), "fs %d cut %d: %zu blocks, %zu wanted\n", fs, c, got.size(), want.size());
    for (size_t k = 0; k < want.size(); ++k)
      EXPECT(got[k] == want[k], "fs %d cut %d: block %zu is (%ld, %ld, %ld), wanted (%ld, %ld, %ld)\n", fs, c, k, got[k].j, got[k].first,
             got[k].hi, want[k].j, want[k].first, want[k].hi);
    ++walks;
  }
  return walks;
}

// the gates as the kernel runs them: per pass 256 partial sums, then the tree
void gate_pass(const std::vector<double>& zr, const std::vector<double>& lr, int NB, long j, int relative, double gamma_r, double* sum, double* cnt) {
  double s[LOUD_THREADS], c[LOUD_THREADS];
  for (int t = 0; t < LOUD_THREADS; ++t) loud_gate_partial(zr.data(), lr.data(), NB, j, relative, gamma_r, t, &s[t], &c[t]);
  for (int o = LOUD_THREADS / 2; o > 0; o >>= 1)
    for (int t = 0; t < LOUD_THREADS; ++t) {      // (ascending t: a step reads only entries >= o, which it does not write)
      loud_tree_step(s, t, o);
      loud_tree_step(c, t, o);
    }
  *sum = s[0]; *cnt = c[0];
}

bool close(double a, double b) { return a == b || fabs(a - b) <= 1e-12 * fabs(b); }

long check_gates() {
  const int NBS[] = {1, 7, 20, 300, 600};
  long steps = 0, fresh_n = 0, kept_n = 0, none_abs = 0;
  uint64_t seed = 12345;
  for (int NB : NBS)
    for (int warmup = 1; warmup <= 3; warmup += 2) {
      std::vector<double> zr((size_t)NB, 0.0), lr((size_t)NB, 0.0), all;
      for (long j = 0; j < 3L * NB + 5; ++j, ++steps) {
        // energies between silence and full scale: digital zero, far under the absolute gate, around the gates, loud
        const uint64_t r = rnd(&seed);
        const double u = (double)(rnd(&seed) >> 11) / 9007199254740992.0;
        const int kind = (j % (NB + 3) < 2 && NB > 1) ? 0 : (int)(r % 4);
        const double z = kind == 0 ? 0.0 : pow(10.0, kind == 1 ? -12.0 + 3.0 * u : (kind == 2 ? -7.5 + 3.0 * u : -3.0 + 2.5 * u));
        all.push_back(z);
        zr[(size_t)loud_zslot(j, NB)] = z;
        lr[(size_t)loud_zslot(j, NB)] = loud_level(z);
        double s1, c1, s2, c2, lufs = 0.0;
        gate_pass(zr, lr, NB, j, 0, 0.0, &s1, &c1);
        const double gamma = loud_gamma_r(s1, c1);
        gate_pass(zr, lr, NB, j, 1, gamma, &s2, &c2);
        const bool fresh = loud_estimate(s2, c2, warmup, &lufs);
        // direct: the plain list of the last NB energies
        const long first = j - NB + 1 > 0 ? j - NB + 1 : 0;
        EXPECT(first == loud_ring_first(j, NB), "NB %d block %ld\n", NB, j);
        double d1 = 0.0, n1 = 0.0, d2 = 0.0, n2 = 0.0;
        for (long b = first; b <= j; ++b)
          if (-0.691 + 10.0 * log10(all[(size_t)b]) >= -70.0) { d1 += all[(size_t)b]; n1 += 1.0; }
        const double dgamma = -0.691 + 10.0 * log10(d1 / n1) - 10.0;
        for (long b = first; b <= j; ++b) {
          const double l = -0.691 + 10.0 * log10(all[(size_t)b]);
          if (l > dgamma && l > -70.0) { d2 += all[(size_t)b]; n2 += 1.0; }
        }
        EXPECT(c1 == n1 && close(s1, d1), "NB %d block %ld: absolute gate %g of %g blocks, direct %g of %g\n", NB, j, s1, c1, d1, n1);
        EXPECT((n1 == 0.0) == (gamma != gamma) && (n1 == 0.0 || close(gamma, dgamma)), "NB %d block %ld: gamma %g, direct %g\n", NB, j, gamma, dgamma);
        EXPECT(c2 == n2 && close(s2, d2), "NB %d block %ld: relative gate %g of %g blocks, direct %g of %g\n", NB, j, s2, c2, d2, n2);
        EXPECT(fresh == (n2 >= warmup), "NB %d block %ld warmup %d\n", NB, j, warmup);
        if (fresh) {
          EXPECT(close(lufs, -0.691 + 10.0 * log10(d2 / n2)) && lufs > -70.0, "NB %d block %ld: %g LUFS\n", NB, j, lufs);
          const float g = loud_gain(lufs, -20.0, -30.0, 30.0);
          EXPECT(g >= 0.0316227f && g <= 31.62278f && close((double)g, (double)(float)pow(10.0, fmin(fmax(-20.0 - lufs, -30.0), 30.0) / 20.0)),
                 "NB %d block %ld: gain %g\n", NB, j, (double)g);
        }
        fresh_n += fresh; kept_n += !fresh; none_abs += n1 == 0.0;
      }
    }
  EXPECT(fresh_n > 100 && kept_n > 10 && none_abs > 3, "%ld fresh, %ld kept, %ld with nothing past the absolute gate\n", fresh_n, kept_n, none_abs);
  EXPECT(loud_gain(-80.0, -20.0, -30.0, 30.0) == (float)pow(10.0, 1.5) && loud_gain(20.0, -20.0, -30.0, 30.0) == (float)pow(10.0, -1.5), "clip\n");
  return steps;
}

}  // namespace

int main() {
  long walks = 0;
  for (int fs : RATES) {
    check_table(fs);
    walks += check_cuts(fs);
  }
  const long steps = check_gates();
  printf("4 rates, %ld walks, %ld gate steps\n", walks, steps);
  printf("loud_math_check: ok\n");
  return 0;
}
