// The counting and layout rules of the re-timing output head of live serving (live_retime.hip), stated once: which ratios
// frame_rate / fps = L / M it takes, how many output frames a stream has emitted after n input frames, where output frame m sits
// between the input frames, how a row's state is laid out, how many output frames a record can give, what the launch needs of
// the LDS, and the weights of the shortest-arc interpolation.  Plain C++ behind a qualifier macro (no HIP include), so the same
// text runs in the kernel, in the host side of live_retime.hip and in tests/host/retime_math_check.cpp.  The definition is
// DESIGN.md 3.7; the per-frame layouts are frames_math.h.
#pragma once
#include <math.h>

#include "frames_math.h"

#define RT_MAX_TERM 4096      // 1 <= L, M <= RT_MAX_TERM
#define RT_MAX_UP 8           // L / M <= RT_MAX_UP
#define RT_SMALL_SINE 1e-8    // below this sine of the arc the interpolation is linear

// ---- the ratio: 0, or the reason (1: L out of range, 2: M out of range, 3: not in lowest terms, 4: L / M above RT_MAX_UP)
ZF_HD long rt_gcd(long a, long b) {
  while (b != 0) { const long r = a % b; a = b; b = r; }
  return a;
}
ZF_HD int rt_ratio_refused(long L, long M) {
  if (L < 1 || L > RT_MAX_TERM) return 1;
  if (M < 1 || M > RT_MAX_TERM) return 2;
  if (rt_gcd(L, M) != 1) return 3;
  return L > (long)RT_MAX_UP * M ? 4 : 0;
}

// ---- counting.  Output frame m sits at input position m M / L = k + num / L; it is emitted in the call that delivers input
// frame k when num == 0 and frame k + 1 otherwise, so after n >= 1 input frames a stream has emitted ((n - 1) L) div M + 1 frames
ZF_HD long rt_n_out(long n, long L, long M) { return n < 1 ? 0 : ((n - 1) * L) / M + 1; }
ZF_HD void rt_position(long m, long L, long M, long* k, long* num) {
  const long p = m * M;
  *k = p / L;
  *num = p - *k * L;
}
// the last input frame output frame m needs
ZF_HD long rt_last_needed(long m, long L, long M) {
  long k, num;
  rt_position(m, L, M, &k, &num);
  return num == 0 ? k : k + 1;
}
// the most output frames a record of `count` input frames can give, whatever came before: ceil(count L / M) + 1
ZF_HD long rt_max_outputs(long count, long L, long M) { return count < 1 ? 0 : (count * L + M - 1) / M + 1; }

// ---- the state: the skeleton tables of the plain head (fr_tables_bytes), then per row the plain head's row -- placement, the two
// flags, the float32 quaternions last emitted -- and behind it the row's last input frame as the raw float32 it arrived in:
// rpos[3] | rrot[4] | lpos[J][3] | ltxy[J][6]
ZF_HD int rt_raw_floats(int J) { return 7 + 9 * J; }
ZF_HD int rt_raw_rpos() { return 0; }
ZF_HD int rt_raw_rrot() { return 3; }
ZF_HD int rt_raw_lpos(int j) { return 7 + 3 * j; }
ZF_HD int rt_raw_ltxy(int J, int j) { return 7 + 3 * J + 6 * j; }
ZF_HD long rt_row_raw_offset(int J) { return fr_row_bytes(J); }
ZF_HD long rt_row_bytes(int J) { return fr_row_bytes(J) + ((long)rt_raw_floats(J) * 4 + 7) / 8 * 8; }
ZF_HD long rt_state_bytes(int rows, int J) { return fr_tables_bytes(J) + (long)rows * rt_row_bytes(J); }
ZF_HD long rt_row_offset(int J, int row) { return fr_tables_bytes(J) + (long)row * rt_row_bytes(J); }

// ---- LDS: output frames are staged as the plain head stages its frames (fr_frame_lds_bytes), as many a pass as fit and never
// more than any ratio can give a record of max_frames input frames
ZF_HD int rt_pass_frames(int J, int max_frames) {
  const long most = rt_max_outputs(max_frames, RT_MAX_UP, 1);
  const long fit = FR_LDS_BYTES / fr_frame_lds_bytes(J);
  return (int)(fit < most ? fit : most);
}
ZF_HD long rt_lds_bytes(int J, int max_frames) { return rt_pass_frames(J, max_frames) * fr_frame_lds_bytes(J); }

// ---- the shortest arc between two unit quaternions whose dot product is d >= 0 (the far end negated first when it was not):
// the weights of the near and the far end at t in (0, 1); the weighted sum is normalised by the caller
ZF_HD void rt_slerp_weights(double d, double t, double* wa, double* wb) {
  const double r = 1.0 - d * d;
  const double s = sqrt(r > 0.0 ? r : 0.0);
  if (s < RT_SMALL_SINE) {
    *wa = 1.0 - t;
    *wb = t;
    return;
  }
  const double th = atan2(s, d);
  *wa = sin((1.0 - t) * th) / s;
  *wb = sin(t * th) / s;
}
