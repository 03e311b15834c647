/* C ABI of libzeggs_hip.so, sixth header: the output head of live serving at each stream's own frame rate
 * (zeggs_live_retime_version() >= 1; zeggs_version() and zeggs_live_frames_version() stay what they are).
 *
 * The other five headers are closed sets (their tests pin their prototypes and structs); the entry points below have a header
 * of their own.  Same conventions as include/zeggs_hip_frames.h: the caller owns all memory, calls only enqueue on `stream`,
 * 0 on success / -1 with zeggs_last_error().  The Python mirror is zeggs/capi.py: RT_STRUCTS / RT_PROTOTYPES
 * (tests/test_live_retime_cpu.py compares the two).
 *
 * zeggs_live_frames_retimed is zeggs_live_frames for streams whose consumer runs at another rate than the server: the same three
 * outputs (ZeggsFramesDims.what, the layouts of include/zeggs_hip_frames.h), one frame per OUTPUT frame, ONE launch for all
 * rows whatever their ratios (csrc/live_retime.hip; the definition is DESIGN.md 3.7, the counting rules csrc/retime_math.h).
 *
 * A stream's input frames are k = 0, 1, ... at the server's rate fps; it asks for frame_rate, frame_rate / fps = L / M in lowest
 * terms, 1 <= L, M <= 4096 and L / M <= 8.  Output frame m = 0, 1, ... sits at input position m M / L:
 *   k = (m M) div L, num = (m M) mod L, t = num / L (a double from the exact 64-bit integers).
 * It is emitted in the call that delivers input frame k when num == 0 and frame k + 1 otherwise: after n >= 1 input frames a
 * stream has emitted n_out(n) = ((n - 1) L) div M + 1 frames (n_out(0) = 0), and a call that takes the row from n0 to n1 emits
 * n_out(n1) - n_out(n0) frames, possibly none.  There is no tail.
 *   num == 0  the frame is zeggs_live_frames' frame of input k: no interpolation; positions and BVH rows the same bits.
 *   num != 0  interpolation of what the head stages in float64 ahead of FK -- the placed root (both ends placed first), the
 *             joints' local quaternions (of the two-axis encoding) and local positions -- positions a + t (b - a); rotations on
 *             the shortest arc: d = a.b, b and d negated when d < 0, s = sqrt(max(0, 1 - d^2)), theta = atan2(s, d), weights
 *             1 - t and t when s < 1e-8 and sin((1 - t) theta) / s, sin(t theta) / s otherwise, the weighted sum normalised.
 *             Everything behind that is the head's own on the interpolated locals: the root folded into joint 0, the Euler
 *             degrees, FK, the sign rule against the value emitted for the stream's previous OUTPUT frame, w >= 0 on output 0.
 * Going down in rate is point sampling (L = 1: every M-th frame): motion above half the output rate aliases.
 * The row's state keeps the last input frame as the raw float32 it arrived in, so a frame between the last input of one call and
 * the first of the next is computed by the same statement from the same bits: a stream's output is a pure function of its input
 * sequence, however it is cut into calls and whichever rows share a launch. */
#ifndef ZEGGS_HIP_RETIME_H
#define ZEGGS_HIP_RETIME_H
#include "zeggs_hip_frames.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one row's share of a call: `count` new INPUT frames as in ZeggsFramesRow, the row's ratio L / M, n_in: the input frames the
 * stream had delivered before this call, outputs: the output frames this call emits, n_out(n_in + count) - n_out(n_in); the
 * i-th of them is output frame n_out(n_in) + i of the stream and goes to local + i (7 + 7J), world + i 7J and bvh + i (3 + 3J). */
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
} ZeggsRetimeRow;

int zeggs_live_retime_version(void);
/* bytes of the state: the skeleton tables, then per row what zeggs_live_frames keeps for a row (placement, two flags, the
 * float32 quaternions last emitted) and the row's last input frame, raw float32: rpos[3] | rrot[4] | lpos[J][3] | ltxy[J][6].
 * ZeggsFramesDims.max_frames bounds the INPUT frames of a record.  0 with zeggs_last_error() for dims that are refused. */
size_t zeggs_live_retime_state_bytes(const ZeggsFramesDims*);
/* the skeleton tables, as zeggs_live_frames_prepare (once per state; waits for its upload) */
int zeggs_live_retime_prepare(const ZeggsFramesDims*, const int* parents_host, const int* seq_host, void* state, size_t state_bytes,
                              void* stream);
/* row `row` opens: its next input frame is frame 0 of a stream; the placement as zeggs_live_frames_reset */
int zeggs_live_retime_reset(const ZeggsFramesDims*, void* state, size_t state_bytes, int row, const float* ref_pos, const float* ref_rot,
                            const double* start_pos, const double* start_rot, int rebase, void* stream);
/* ONE launch for all R records (grid = R, one workgroup per record).  rows_host: the records in HOST memory for the checks, all
 * ahead of the launch and naming the record they refuse: the row and the sources as zeggs_live_frames, a ratio within the bounds
 * and in lowest terms, n_in >= 0, `outputs` equal to the rule above, and where outputs > 0 a non-NULL aligned destination for
 * every bit of d->what.  rows_dev: the same records in DEVICE memory; NULL is allowed for R == 1.  A record with count == 0 is
 * skipped; rows that are not in the call keep their state. */
int zeggs_live_frames_retimed(const ZeggsFramesDims*, const ZeggsRetimeRow* rows_host, const ZeggsRetimeRow* rows_dev, int R, void* state,
                              size_t state_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
