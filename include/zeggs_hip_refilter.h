/* C ABI of libzeggs_hip.so, seventh header: the filter stage of the re-timing output head of live serving
 * (zeggs_live_refilter_version() >= 1; zeggs_version(), zeggs_live_frames_version() and zeggs_live_retime_version() stay what
 * they are).
 *
 * The other six headers are closed sets (their tests pin their prototypes and structs); the entry points below have a header
 * of their own.  Same conventions as include/zeggs_hip_retime.h: the caller owns all memory, calls only enqueue on `stream`,
 * 0 on success / -1 with zeggs_last_error().  The Python mirror is zeggs/capi.py: RF_STRUCTS / RF_PROTOTYPES
 * (tests/test_live_refilter_cpu.py compares the two).
 *
 * zeggs_live_frames_refiltered is zeggs_live_frames_retimed with an optional band-limiting filter per row: the same three
 * outputs, one frame per OUTPUT frame, ONE launch for all rows whatever their ratios and whether they filter
 * (csrc/live_refilter.hip; the definition is DESIGN.md 3.7, the counting rules csrc/refilter_math.h).
 *
 * A record with half == 0 is a record of zeggs_live_frames_retimed: the same statement, the same emission rule, the same bits.
 *
 * A record with half = H > 0 is filtered.  frame_rate / fps = L / M as in the sixth header, and L <= 1024, M <= 4 L.  With
 * zero_crossings Z (1 .. 8), rolloff r and beta: s = min(1, L / M), c = r s, WL = Z max(L, M), W = WL / L, H = ceil(W),
 * taps = 2 H + 1, and the caller's table (float64, device memory, [L][taps]) holds
 *   table[phase][j] = h(phase / L + H - j) / sum_j h(...),  h(t) = c sinc(c t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta), |t| < W,
 * every phase row divided by its own sum (accumulated in ascending j): a pose held still stays that pose.
 * Output frame m sits at m M / L = k + num / L; its phase is num, tap j sits on input frame i = k - H + j; an index below 0 is
 * frame 0 and, in a final record, an index above the stream's last frame is the last frame.  While the stream runs, m is
 * emitted in the call that delivers input frame k + H: after n input frames
 *   nf(n) = 0 for n <= H, else ((n - H) L - 1) div M + 1
 * frames have left.  A record marked `final` emits everything up to n_out(n) = ((n - 1) L) div M + 1 with the far taps held,
 * also when it brings no new frame (count == 0): a closed filtered stream has as many frames as an unfiltered one, H input
 * frames later.
 * Per tap, in float64, ascending j, one accumulator of explicit fma(): the root is placed first; root position and lpos[j] are
 * sum w_j x_j; the root rotation and every joint's quaternion (of the two-axis encoding): each tap's quaternion is negated
 * when its dot product with the centre tap's (j = H, input frame k) is below 0, the weighted sum is divided by its norm n, and
 * the centre tap's quaternion is taken when n < 1e-8.  Everything behind that is the head's own: the root folded into joint 0,
 * Euler degrees, FK, the sign rule against the value emitted for the stream's previous OUTPUT frame, w >= 0 on output 0.
 * A row's state keeps its last 2 max_half input frames as the raw float32 they arrived in (frame i in slot i mod 2 max_half),
 * rewritten only when all passes of a call are through: a stream's output is a pure function of its input sequence, however
 * it is cut into calls, wherever the final record falls and whichever rows share a launch. */
#ifndef ZEGGS_HIP_REFILTER_H
#define ZEGGS_HIP_REFILTER_H
#include "zeggs_hip_retime.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one row's share of a call: the fields of ZeggsRetimeRow, where they sit there, then the filter: `table` (device memory,
 * NULL when half == 0), half = H (0: the row is not filtered) and final (the stream ends with this record; ignored when
 * half == 0).  outputs: emitted(n_in + count) - nf(n_in) for a filtered row, emitted = n_out in a final record and nf
 * otherwise; n_out(n_in + count) - n_out(n_in) for half == 0. */
typedef struct {
  const float* pose;
  const float* rpos;
  const float* rrot;
  float* local;
  float* world;
  double* bvh;
  long pose_ld, rpos_ld, rrot_ld;
  long n_in, outputs;
  int row, count, L, M;
  const double* table;
  int half, final;
} ZeggsRefilterRow;

int zeggs_live_refilter_version(void);
/* bytes of the state for rows whose half is at most max_half (1 .. 32): the skeleton tables, then per row what
 * zeggs_live_frames keeps for a row and a ring of 2 max_half input frames, raw float32, each
 * rpos[3] | rrot[4] | lpos[J][3] | ltxy[J][6].  0 with zeggs_last_error() for dims or a max_half that are refused. */
size_t zeggs_live_refilter_state_bytes(const ZeggsFramesDims*, int max_half);
/* the skeleton tables, as zeggs_live_frames_prepare (once per state; waits for its upload) */
int zeggs_live_refilter_prepare(const ZeggsFramesDims*, int max_half, const int* parents_host, const int* seq_host, void* state,
                                size_t state_bytes, void* stream);
/* row `row` opens: its next input frame is frame 0 of a stream; the placement as zeggs_live_frames_reset */
int zeggs_live_refilter_reset(const ZeggsFramesDims*, int max_half, void* state, size_t state_bytes, int row, const float* ref_pos,
                              const float* ref_rot, const double* start_pos, const double* start_rot, int rebase, void* stream);
/* ONE launch for all R records (grid = R, one workgroup per record).  rows_host: the records in HOST memory for the checks, all
 * ahead of the launch and naming the record they refuse: what zeggs_live_frames_retimed checks, and for a filtered record
 * L <= 1024 and M <= 4 L, a half that is ceil(Z max(L, M) / L) for some Z = 1 .. 8 and at most max_half, a non-NULL table on
 * an 8-byte boundary, final 0 or 1, and `outputs` equal to the rule above.  rows_dev: the same records in DEVICE memory; NULL
 * is allowed for R == 1.  A record with count == 0 is skipped unless it is a filtered final record; rows that are not in the
 * call keep their state. */
int zeggs_live_frames_refiltered(const ZeggsFramesDims*, int max_half, const ZeggsRefilterRow* rows_host, const ZeggsRefilterRow* rows_dev,
                                 int R, void* state, size_t state_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
