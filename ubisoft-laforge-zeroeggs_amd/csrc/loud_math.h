// The index and gate rules of the running loudness estimate of live serving (live_loudness.hip), stated once: the bounds of the
// 400 ms gating blocks, which blocks complete inside a push, where a filtered sample and a block energy sit in their rings, and
// the two BS.1770 gates over the ring of block energies.  Plain C++ behind a qualifier macro (no HIP include), so the same text
// runs in the kernel, in the host side of live_loudness.hip and in tests/host/loud_math_check.cpp.
// Reference: pyloudnorm 0.1.0 meter.py as restated in oracle/loudness.py; the offline form is loudness.hip.
#pragma once
#include <math.h>

#ifndef ZL_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZL_HD __host__ __device__ __forceinline__
#else
#define ZL_HD inline
#endif
#endif

#define LOUD_THREADS 256          // partial sums of a block energy and of a gate (block_energy_k's order: strided sums, then the tree)
#define LOUD_ABS_GATE (-70.0)

// ---- block bounds: block j covers samples [loud_lo(j), loud_hi(j)) -- pyloudnorm's float64 products, truncated as int() does
// (audio.gating_blocks without its clamp to the signal's length).  j 0.25 is exact, so a fused j 0.25 + 1 rounds as the sum does.
ZL_HD long loud_lo(long j, int fs) { return (long)(0.4 * ((double)j * 0.25) * (double)fs); }
ZL_HD long loud_hi(long j, int fs) { return (long)(0.4 * ((double)j * 0.25 + 1.0) * (double)fs); }
// samples of a block = length of the ring of filtered samples: sample n sits in slot n % loud_block_len(fs)
ZL_HD long loud_block_len(int fs) { return loud_hi(0, fs) - loud_lo(0, fs); }
ZL_HD long loud_yslot(long n, long len) { return n % len; }
// first sample of block j that the ring still holds when sample loud_hi(j) - 1 has just arrived (loud_lo(j) wherever the block
// length is the constant it is for every rate checked by loud_rate_ok)
ZL_HD long loud_first(long j, int fs, long len) {
  const long lo = loud_lo(j, fs), hi = loud_hi(j, fs);
  return hi - lo > len ? hi - len : lo;
}
// block j completes with sample loud_hi(j) - 1: it is complete once n_end samples have arrived when ...
ZL_HD bool loud_complete(long j, long n_end, int fs) { return loud_hi(j, fs) <= n_end; }
// ... so a row that has completed `j` blocks and receives samples [n, n + m) next runs up to this index before it must stop to
// evaluate block j (== n + m: no block completes in what is left)
ZL_HD long loud_run_end(long j, long n_end, int fs) {
  const long hi = loud_hi(j, fs);
  return hi < n_end ? hi : n_end;
}
// the number of blocks complete after n samples, without a counter (what the carried counter must equal)
ZL_HD long loud_blocks_done(long n, int fs) {
  long j = (long)(((double)n / (double)fs - 0.4) * 10.0) - 2;
  if (j < 0) j = 0;
  while (j > 0 && !loud_complete(j - 1, n, fs)) --j;
  while (loud_complete(j, n, fs)) ++j;
  return j;
}
// the properties the kernel leans on, over the first `blocks` blocks: constant block length, strictly increasing ends
ZL_HD bool loud_rate_ok(int fs, long blocks) {
  if (fs < 10) return false;
  const long len = loud_block_len(fs);
  if (len < 1) return false;
  for (long j = 0; j < blocks; ++j)
    if (loud_hi(j, fs) - loud_lo(j, fs) != len || loud_hi(j + 1, fs) <= loud_hi(j, fs)) return false;
  return true;
}

// ---- the ring of block energies: block j in slot j % NB; after block j the estimate is over blocks loud_ring_first(j, NB) .. j
ZL_HD long loud_zslot(long j, int NB) { return j % NB; }
ZL_HD long loud_ring_first(long j, int NB) { return j - NB + 1 > 0 ? j - NB + 1 : 0; }
ZL_HD double loud_level(double z) { return -0.691 + 10.0 * log10(z); }

// thread t's share of a block energy: samples first + t, first + t + LOUD_THREADS, ... < hi from the ring, in that order
ZL_HD double loud_energy_partial(const double* yring, long len, long first, long hi, int t) {
  double acc = 0.0;
  for (long i = first + t; i < hi; i += LOUD_THREADS) {
    const double y = yring[loud_yslot(i, len)];
    acc = fma(y, y, acc);
  }
  return acc;
}
// one step of the tree over LOUD_THREADS partial sums (o = 128, 64, .. 1; a barrier between two steps): thread t's part
ZL_HD void loud_tree_step(double* sm, int t, int o) {
  if (t < o) sm[t] += sm[t + o];
}

// thread t's share of one gate pass over the ring after block j: blocks first + t, first + t + LOUD_THREADS, ... <= j, oldest
// first.  `lr` holds loud_level of `zr`, slot by slot.  relative == 0: the absolute gate (l >= -70); else l > gamma_r and l > -70
// (gamma_r NaN: nothing passes, as in pyloudnorm).  -> sum of the passing z and their count
ZL_HD void loud_gate_partial(const double* zr, const double* lr, int NB, long j, int relative, double gamma_r, int t, double* sum,
                             double* cnt) {
  double s = 0.0, c = 0.0;
  for (long b = loud_ring_first(j, NB) + t; b <= j; b += LOUD_THREADS) {
    const long k = loud_zslot(b, NB);
    const double l = lr[k];
    if (relative ? (l > gamma_r && l > LOUD_ABS_GATE) : (l >= LOUD_ABS_GATE)) { s += zr[k]; c += 1.0; }
  }
  *sum = s; *cnt = c;
}
ZL_HD double loud_gamma_r(double abs_sum, double abs_cnt) { return loud_level(abs_sum / abs_cnt) - 10.0; }      // 0 / 0 -> NaN
// the estimate from the second pass: true and *lufs when at least `warmup` blocks passed, else no new estimate
ZL_HD bool loud_estimate(double rel_sum, double rel_cnt, int warmup, double* lufs) {
  if (rel_cnt < (double)warmup) return false;
  *lufs = loud_level(rel_sum / rel_cnt);
  return true;
}
// the gain that brings an estimate to `target`, clipped in dB, as the float32 the samples are multiplied by
ZL_HD float loud_gain(double lufs, double target, double lo_db, double hi_db) {
  double db = target - lufs;
  db = db < lo_db ? lo_db : (db > hi_db ? hi_db : db);
  return (float)pow(10.0, db / 20.0);
}
