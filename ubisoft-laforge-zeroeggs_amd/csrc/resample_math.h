// The index rules of the band-limited rate converter of live serving (live_resample.hip), stated once: the reduced ratio of two
// rates, how many outputs a row owes after n inputs (while its signal goes on, and at its end), which input sample an output's
// first tap sits on and which row of the coefficient table it takes, and how many past inputs a row must carry from call to call.
// Plain C++ behind a qualifier macro (no HIP include), so the same text runs in the kernel, in the host side of
// live_resample.hip and in tests/host/resample_math_check.cpp.  The definition is DESIGN.md 3.7:
//   g = gcd(fi, fo), L = fo / g, M = fi / g; output m sits at input position p_m = m M / L; the filter h has the support
//   |t| < W, W = Z / min(1, L / M) input samples, so WL = W L = Z max(L, M) is an integer and everything below is integer
//   arithmetic on positions in units of 1 / L of an input sample:  P_m = m M,  tap k takes part when |P_m - k L| < WL.
// WL == 0 is the pass-through mode (L = M = 1, one tap of 1.0 on k = m: a format conversion only).
#pragma once

#ifndef ZR_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZR_HD __host__ __device__ __forceinline__
#else
#define ZR_HD inline
#endif
#endif

#define RS_MAX_L 640              // L <= 640 and M / L <= 24: 8 .. 384 kHz -> 16 kHz
#define RS_MAX_DECIMATION 24
#define RS_MAX_ZERO_CROSSINGS 64  // what the state of a row is sized for
#define RS_THREADS 1024           // threads of a workgroup = outputs of a tile, one each
#define RS_SPAN 12288             // float32 input samples a tile may touch (its staging area)

ZR_HD long rs_gcd(long a, long b) {
  while (b != 0) { const long t = a % b; a = b; b = t; }
  return a;
}
// the reduced ratio; false when a rate is not positive or the pair is outside what the converter supports
ZR_HD bool rs_ratio(long fi, long fo, int* L, int* M) {
  if (fi < 1 || fo < 1) return false;
  const long g = rs_gcd(fi, fo), l = fo / g, m = fi / g;
  if (l > RS_MAX_L || m > (long)RS_MAX_DECIMATION * l) return false;
  *L = (int)l; *M = (int)m;
  return true;
}
// W L for Z zero crossings
ZR_HD long rs_wl(int Z, int L, int M) { return (long)Z * (L > M ? L : M); }
// half width of a table row in input samples, ceil(W), and the row's length: tap j of output m sits on input k = q - H + j,
// q = floor(p_m); the taps with |p_m - k| >= W hold 0 and are never multiplied (rs_tap_range)
ZR_HD int rs_half(long WL, int L) { return (int)((WL + L - 1) / L); }
ZR_HD int rs_taps(long WL, int L) { return 2 * rs_half(WL, L) + 1; }
// past inputs a row carries: an output that is not ready after n inputs has p_m + W > n, so its first tap is > n - 2 W
ZR_HD int rs_history(long WL, int L) { return (int)((2 * WL + L - 1) / L); }
// sample k of a row sits in slot k % history of its ring (k >= 0)
ZR_HD int rs_slot(long k, int history) { return (int)(k % history); }

// outputs ready after n inputs while the signal goes on: p_m + W <= n
ZR_HD long rs_ready(long n, int L, int M, long WL) {
  if (WL == 0) return n;
  const long nl = n * (long)L;
  return nl < WL ? 0 : (nl - WL) / M + 1;
}
// outputs of a signal of n inputs in all: ceil(n L / M)
ZR_HD long rs_total(long n, int L, int M) { return (n * (long)L + M - 1) / M; }

// output m: q = floor(p_m) and the phase P_m - q L (the row of the table)
ZR_HD void rs_position(long m, int L, int M, long* q, int* phase) {
  const long P = m * (long)M;
  *q = P / L;
  *phase = (int)(P - *q * L);
}
// the taps of a table row of phase `phase` that lie inside the support, j0 <= j <= j1 (ascending j is ascending k)
ZR_HD void rs_tap_range(int phase, int L, long WL, int* j0, int* j1) {
  const int H = rs_half(WL, L);
  if (WL == 0) { *j0 = *j1 = 0; return; }
  // k L > P - WL  <=>  k - q >= -ceil((WL - phase) / L) + 1 ;  k L < P + WL  <=>  k - q <= ceil((phase + WL) / L) - 1
  *j0 = H - (int)((WL - phase + L - 1) / L) + 1;
  *j1 = H + (int)((phase + WL + L - 1) / L) - 1;
}
// outputs per tile: consecutive outputs m0 .. m0 + T - 1 touch at most (T - 1) M / L + 2 ceil(W) + 2 consecutive inputs
// (rs_first_tap(m0) .. rs_last_tap(m0 + T - 1): both grow with m), which must fit RS_SPAN.  >= 1 for every supported filter
ZR_HD int rs_tile_outputs(int L, int M, long WL) {
  const long room = ((long)RS_SPAN - 2 * rs_half(WL, L) - 2) * L / M;
  return (int)(room < RS_THREADS ? room : RS_THREADS);
}
// first input sample output m touches (may be negative: x is 0 there)
ZR_HD long rs_first_tap(long m, int L, int M, long WL) {
  long q; int ph, j0, j1;
  rs_position(m, L, M, &q, &ph);
  rs_tap_range(ph, L, WL, &j0, &j1);
  return q - rs_half(WL, L) + j0;
}
ZR_HD long rs_last_tap(long m, int L, int M, long WL) {
  long q; int ph, j0, j1;
  rs_position(m, L, M, &q, &ph);
  rs_tap_range(ph, L, WL, &j0, &j1);
  return q - rs_half(WL, L) + j1;
}
