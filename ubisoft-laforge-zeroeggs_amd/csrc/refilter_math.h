// The counting and layout rules of the filter stage of the re-timing output head of live serving (live_refilter.hip), stated
// once: which ratios a filtered row takes, how many input frames the filter reaches to either side (`half`, H), how many output
// frames a filtered stream has emitted after n input frames, which input frame a tap sits on, where that frame lies -- in the
// call or in the row's ring -- how a row's state is laid out and what the launch needs of the LDS.  Plain C++ behind a qualifier
// macro (no HIP include), so the same text runs in the kernel, in the host side of live_refilter.hip and in
// tests/host/refilter_math_check.cpp.  The definition is DESIGN.md 3.7; the unfiltered rules are retime_math.h.
#pragma once
#include "retime_math.h"

#define RF_MAX_L 1024         // a filtered row: L <= RF_MAX_L (the table has L rows)
#define RF_MAX_DOWN 4         // ... and M <= RF_MAX_DOWN L
#define RF_MAX_Z 8            // zero crossings to either side, 1 .. RF_MAX_Z
#define RF_MAX_HALF 32        // so H <= RF_MAX_Z RF_MAX_DOWN
#define RF_SMALL_NORM 1e-8    // below this norm of the weighted quaternion sum the centre tap's quaternion is taken

// ---- the ratio of a filtered row: 0, or the reason (1 .. 4: rt_ratio_refused, 5: L above RF_MAX_L, 6: M above RF_MAX_DOWN L)
ZF_HD int rf_ratio_refused(long L, long M) {
  const int why = rt_ratio_refused(L, M);
  if (why != 0) return why;
  if (L > RF_MAX_L) return 5;
  return M > (long)RF_MAX_DOWN * L ? 6 : 0;
}
// H = ceil(W), W = Z max(L, M) / L input frames; the filter has 2 H + 1 taps
ZF_HD int rf_half(long L, long M, int Z) {
  const long WL = (long)Z * (L > M ? L : M);
  return (int)((WL + L - 1) / L);
}
ZF_HD int rf_taps(int H) { return 2 * H + 1; }
// is H the half width of some Z = 1 .. RF_MAX_Z at this ratio?
ZF_HD bool rf_half_fits(long L, long M, int H) {
  for (int Z = 1; Z <= RF_MAX_Z; ++Z)
    if (rf_half(L, M, Z) == H) return true;
  return false;
}

// ---- counting.  Output frame m sits at k + num / L (rt_position); tap j = 0 .. 2 H sits on input frame k - H + j; while the
// stream runs, m is emitted in the call that delivers input frame k + H: after n input frames nf(n) frames have left.  A record
// marked final emits everything up to rt_n_out(n), the far taps held on the last frame.
ZF_HD long rf_n_out(long n, long L, long M, int H) { return n <= H ? 0 : ((n - H) * L - 1) / M + 1; }
ZF_HD long rf_emitted(long n, long L, long M, int H, int final) { return final ? rt_n_out(n, L, M) : rf_n_out(n, L, M, H); }
// the input frame of tap j of an output whose position is k, of a stream whose last frame so far is `last` (>= 0): an index
// below 0 is frame 0, an index above `last` is `last` (the counting rule gives such an index only in a final record)
ZF_HD long rf_tap_frame(long k, int H, int j, long last) {
  const long i = k - H + j;
  return i < 0 ? 0 : (i > last ? last : i);
}

// ---- the state: the skeleton tables of the plain head (fr_tables_bytes), then per row the plain head's row and behind it a
// ring of the last D = 2 max_half input frames, each the raw float32 it arrived in (the rt_raw_* layout), frame i in slot i mod D
ZF_HD int rf_ring_frames(int max_half) { return 2 * max_half; }
ZF_HD int rf_slot(long i, int max_half) {
  const int D = rf_ring_frames(max_half);
  const long s = i % D;
  return (int)(s < 0 ? s + D : s);
}
ZF_HD long rf_row_ring_offset(int J) { return fr_row_bytes(J); }
ZF_HD long rf_ring_bytes(int J, int max_half) { return ((long)rf_ring_frames(max_half) * rt_raw_floats(J) * 4 + 7) / 8 * 8; }
ZF_HD long rf_row_bytes(int J, int max_half) { return fr_row_bytes(J) + rf_ring_bytes(J, max_half); }
ZF_HD long rf_state_bytes(int rows, int J, int max_half) { return fr_tables_bytes(J) + (long)rows * rf_row_bytes(J, max_half); }
ZF_HD long rf_row_offset(int J, int max_half, int row) { return fr_tables_bytes(J) + (long)row * rf_row_bytes(J, max_half); }
// where a tap finds input frame i (>= n_in - D by the coverage rule below) of a record that brings frames n_in .. n_in + count - 1:
// the index in the call, or -1 - slot for a frame of an earlier call.  Coverage: an output computed in a call with n_in earlier
// frames was not computable before, k + H >= n_in, so its earliest tap k - H >= n_in - 2 H >= n_in - D is still in the ring.
ZF_HD long rf_where(long i, long n_in, int max_half) { return i >= n_in ? i - n_in : -1 - (long)rf_slot(i, max_half); }
// the first frame of a call that is still in the ring after it (a call longer than the ring overwrites its own early frames)
ZF_HD long rf_first_kept(long count, int max_half) {
  const long D = rf_ring_frames(max_half);
  return count > D ? count - D : 0;
}

// ---- LDS: output frames are staged in passes as the unfiltered head stages them
ZF_HD int rf_pass_frames(int J, int max_frames) { return rt_pass_frames(J, max_frames); }
ZF_HD long rf_lds_bytes(int J, int max_frames) { return rt_lds_bytes(J, max_frames); }
