// The integer rules of the audio front-end (mel.hip) that host and device both need, stated once: how many STFT frames a signal
// has, which sample tap j of frame m reads and whether it is loaded, the window, and which STFT frames a range of animation frames
// interpolates.  Plain C++ behind a qualifier macro (no HIP include), so the same text runs in the kernels, in the host side of
// mel.hip and in tests/host/mel_math_check.cpp.  Reference: ZEGGS/audio/spectrograms.py:216-269, ZEGGS/data_pipeline.py:62-80.
#pragma once
#include <math.h>

#include "../../include/zeggs_hip.h"

#ifndef ZM_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZM_HD __host__ __device__ __forceinline__
#else
#define ZM_HD inline
#endif
#endif

// ZeggsMelDims.flags: bit 0 = audio_conf.centered is FALSE (no reflect padding: frame m starts at sample m hop, spectrograms.py:237-239),
// bit 1 = audio_conf.normalize_range is FALSE (the stored value is 20 log10 s, not mapped to [0, 1], spectrograms.py:123-129)
// bits 2-3 = audio_conf.resample_method (data_pipeline.py:65-79: scipy.interpolate.griddata for the mel table, interp1d for the energy):
// 0 "linear" (the shipped configurations), 4 "nearest", 8 "cubic"
#define MEL_UNCENTERED 1
#define MEL_RAW_RANGE 2
#define MEL_NEAREST 4
#define MEL_CUBIC 8

// spectrograms.py:233-246 (integer rule)
ZM_HD long stft_frames(long n, int n_fft, int hop, int flags) {
  long np = (n > n_fft ? n : n_fft) + ((flags & MEL_UNCENTERED) ? 0 : 2 * (long)(n_fft / 2));
  return (np % hop == 0) ? (np - n_fft) / hop : 1 + (np - n_fft) / hop;
}

// ---- the sample index rule.  Tap j of STFT frame m sits at index p of the signal before reflect padding ...
ZM_HD long mel_tap(const ZeggsMelDims& d, long m, long j) { return m * d.hop + j - ((d.flags & MEL_UNCENTERED) ? 0 : d.n_fft / 2); }
// ... which reads sample src of the n-sample signal, zero-extended to n_fft when shorter (spectrograms.py:233-234) and reflected at both ends ...
ZM_HD long mel_src(const ZeggsMelDims& d, long m, long j, long n) {
  const long neff = n > d.n_fft ? n : d.n_fft, p = mel_tap(d, m, j);
  return p < 0 ? -p : (p >= neff ? 2 * (neff - 1) - p : p);
}
// ... and is loaded from a buffer that holds samples base .. n_avail - 1 of it, zero otherwise
ZM_HD bool mel_loaded(long src, long n, long n_avail, long base) { return src >= base && src < n && src < n_avail; }

ZM_HD double mel_hann(int j, int n_fft) { return 0.5 - 0.5 * cos(2.0 * M_PI * (double)j / (double)(n_fft - 1)); }   // scipy hann(sym=True)

// ---- animation frame k sits at STFT time t_k = mel_rate k and interpolates STFT frames ceil(t_k) - 1, ceil(t_k)
ZM_HD double mel_rate(const ZeggsMelDims& d) { return ((double)d.fs / (double)d.hop) / (double)d.fps; }
// STFT frames [m0, m1) that the animation frames [k0, k1) interpolate; M = STFT frames of the signal
ZM_HD void mel_range_stft(const ZeggsMelDims& d, long M, long k0, long k1, long* m0_, long* m1_) {
  const double r = mel_rate(d);
  long m0 = (long)ceil(r * (double)k0) - 1, m1 = (long)ceil(r * (double)(k1 - 1)) + 1;
  if (m0 < 0) m0 = 0;
  if (m1 < 2) m1 = 2;
  if (m1 > M) m1 = M;
  if (m0 > m1 - 2) m0 = m1 - 2 > 0 ? m1 - 2 : 0;
  *m0_ = m0; *m1_ = m1;
}
// bounds of m1 - m0 above: for the range [k0, k1), and for any range of at most F animation frames
ZM_HD long mel_range_slots(const ZeggsMelDims& d, long k0, long k1) {
  return (long)ceil(mel_rate(d) * (double)(k1 - 1)) - (long)floor(mel_rate(d) * (double)k0) + 4;
}
ZM_HD long mel_batch_slots(const ZeggsMelDims& d, long F) { return (long)ceil(mel_rate(d) * (double)(F > 1 ? F : 1)) + 4; }
// animation frames 0 .. k-1 are computable from the first n_samples of a signal that continues: every tap of the STFT frames they
// interpolate lies below n_samples (frame m is complete when mel_tap(d, m, n_fft - 1) < n_samples)
ZM_HD long mel_frames_ready(const ZeggsMelDims& d, long n_samples) {
  const long room = n_samples - 1 - mel_tap(d, 0, d.n_fft - 1);      // frame m is complete when m hop <= room
  if (room < d.hop) return 0;                                        // frame 1 is not: nothing to interpolate yet
  const long mmax = room / d.hop;
  const double r = mel_rate(d);
  long k = (long)floor((double)mmax / r);                           // largest k with t_k <= mmax
  while (k >= 0 && ceil(r * (double)k) > (double)mmax) --k;
  return k + 1;
}

// smallest sample index that the STFT frames [m0, m1) load: n = signal length of the reflect rule, n_avail = samples present; the sample
// before it when pre-emphasis is on.  LONG_MAX: they load nothing.  Along the taps of a frame, src falls while p < 0, rises while
// 0 <= p < neff and falls again from p = neff on, and the loaded taps of such a run are those below min(n, n_avail): the smallest loaded
// index of a run is at one of its ends, so the six run ends are all a frame needs.
ZM_HD long mel_first_load(const ZeggsMelDims& d, long m0, long m1, long n, long n_avail) {
  const long NF = d.n_fft, neff = n > NF ? n : NF;
  long best = __LONG_MAX__;
  auto frame = [&](long m) {
    const long a = mel_tap(d, m, 0);
    const long ends[6] = {0, -a - 1, -a, neff - a - 1, neff - a, NF - 1};
    long lo = __LONG_MAX__;
    for (long j : ends) {
      if (j < 0 || j >= NF) continue;
      const long src = mel_src(d, m, j, n);
      if (mel_loaded(src, n, n_avail, 0) && src < lo) lo = src;
    }
    if (lo != __LONG_MAX__ && d.pre_emph != 0.0 && lo > 0) --lo;
    if (lo < best) best = lo;
  };
  long m = m0;
  for (; m < m1; ++m) {
    frame(m);
    if (mel_tap(d, m, 0) >= 0 && mel_tap(d, m, NF - 1) < neff) break;      // no reflection: every later frame without one starts further right ...
  }
  for (long q = m1 - 1; q > m && mel_tap(d, q, NF - 1) >= neff; --q) frame(q);      // ... and the frames that reflect at the right end are the last ones
  return best;
}
