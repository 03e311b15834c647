// Host check of csrc/mel_math.h, the integer rules of the audio front-end: mel_first_load (the closed form that decides whether a
// sliding window may be read) against the minimum over every tap (m, j) of the frame range enumerated through the shared index rule
// mel_src / mel_loaded, at both ends of the signal; and mel_frames_ready against the taps of the STFT frames an animation frame
// interpolates.  Exits non-zero at the first difference.  Built and run by tests/test_mel_math_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "../../ubisoft-laforge-zeroeggs_amd/csrc/mel_math.h"

#define EXPECT(cond, ...)                                            \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "mel_math_check: %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                  \
      fprintf(stderr, "  [%s]\n", #cond);                            \
      exit(1);                                                       \
    }                                                                \
  } while (0)

namespace {

const int SHAPES[][2] = {{800, 200}, {64, 16}, {30, 7}, {8, 16}};      // n_fft, hop (the last: hop > n_fft)
constexpr long OPEN = 1L << 50;                                        // length of a signal that continues

ZeggsMelDims dims(int n_fft, int hop, bool centred, bool pe) {
  ZeggsMelDims d{};
  d.n_fft = n_fft; d.hop = hop; d.n_mels = 80; d.fs = 16000; d.fps = 60.f; d.min_clip = 1e-5f;
  d.pre_emph = pe ? 0.97 : 0.0;
  d.flags = centred ? 0 : MEL_UNCENTERED;
  return d;
}

// every tap of the frames [m0, m1): the smallest index loaded (the sample before it too when pre-emphasis is on: mel.hip, mel_sample)
long first_load_by_enumeration(const ZeggsMelDims& d, long m0, long m1, long n, long n_avail) {
  long best = __LONG_MAX__;
  for (long m = m0; m < m1; ++m)
    for (long j = 0; j < d.n_fft; ++j) {
      const long src = mel_src(d, m, j, n);
      if (!mel_loaded(src, n, n_avail, 0)) continue;
      const long lo = (d.pre_emph != 0.0 && src > 0) ? src - 1 : src;
      if (lo < best) best = lo;
    }
  return best;
}

struct Seen { long ranges, nothing, right_only, right_reaches_left; };

void check_first_load(const ZeggsMelDims& d, long len, bool final, Seen* seen) {
  const long n = final ? len : OPEN;
  // finished signal: every range of its STFT frames; a signal that continues: the frames that start inside what is present, and two more
  const long M = final ? stft_frames(len, d.n_fft, d.hop, d.flags) : len / d.hop + 3;
  const long neff = n > d.n_fft ? n : d.n_fft;
  for (long m0 = 0; m0 < M; ++m0)
    for (long m1 = m0 + 1; m1 <= M; ++m1) {
      const long want = first_load_by_enumeration(d, m0, m1, n, len), got = mel_first_load(d, m0, m1, n, len);
      EXPECT(got == want, "n_fft %d hop %d flags %d pe %g len %ld final %d frames [%ld, %ld): first load %ld, enumeration gives %ld\n",
             d.n_fft, d.hop, d.flags, d.pre_emph, len, (int)final, m0, m1, got, want);
      ++seen->ranges;
      if (want == __LONG_MAX__) ++seen->nothing;
      const long a = mel_tap(d, m0, 0);
      if (a >= 0 && mel_tap(d, m1 - 1, d.n_fft - 1) >= neff) {      // no reflection on the left, one on the right
        ++seen->right_only;
        if (want < a) ++seen->right_reaches_left;
      }
    }
}

void check_frames_ready(const ZeggsMelDims& d) {
  long m0, m1;
  for (long n = 1; n <= 6L * d.n_fft + 5L * d.hop; ++n) {
    const long K = mel_frames_ready(d, n);
    for (long k = 0; k <= K; ++k) {
      mel_range_stft(d, 1L << 40, k, k + 1, &m0, &m1);
      bool inside = true;
      for (long m = m0; m < m1; ++m) inside = inside && mel_tap(d, m, d.n_fft - 1) < n;
      EXPECT(inside == (k < K), "n_fft %d hop %d flags %d: %ld samples, %ld frames ready, frame %ld needs STFT frames [%ld, %ld)\n", d.n_fft,
             d.hop, d.flags, n, K, k, m0, m1);
    }
  }
}

}  // namespace

int main() {
  Seen seen{};
  for (const auto& sh : SHAPES)
    for (int centred = 0; centred < 2; ++centred) {
      for (int pe = 0; pe < 2; ++pe) {
        const ZeggsMelDims d = dims(sh[0], sh[1], centred, pe);
        const long lens[] = {sh[0] - 3L, sh[0], 20L * sh[1], 20L * sh[1] + 3, 7L * sh[1] + sh[0] + 1};
        for (long len : lens)
          for (int final = 0; final < 2; ++final) check_first_load(d, len, final, &seen);
      }
      check_frames_ready(dims(sh[0], sh[1], centred, false));
    }
  // the grid reaches what it is there for: ranges that load nothing, ranges that reflect at the right end only, and among those some
  // whose reflection reaches further left than the first frame's own start
  EXPECT(seen.nothing > 0 && seen.right_only > 0 && seen.right_reaches_left > 0, "ranges %ld: nothing %ld, right only %ld, reaching left %ld\n",
         seen.ranges, seen.nothing, seen.right_only, seen.right_reaches_left);
  printf("ranges %ld (load nothing %ld, right reflection only %ld, of which reaching left of the first frame %ld)\n", seen.ranges,
         seen.nothing, seen.right_only, seen.right_reaches_left);
  printf("mel_math_check: ok\n");
  return 0;
}
