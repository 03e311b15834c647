// Live serving: the output head at each stream's own frame rate -- the frames of live_frames.hip, handed out at frame_rate =
// fps L / M instead of the model's fps (include/zeggs_hip_retime.h; the counting rules, the state layout and the interpolation
// weights are retime_math.h, the definition DESIGN.md 3.7).
//
// One workgroup of 256 threads per record, ONE launch per step whatever the rows' ratios; the server enqueues it INSTEAD of
// live_frames_k.  A record brings `count` input frames and emits the output frames m whose position m M / L = k + num / L became
// computable with them, n_out(n_in + count) - n_out(n_in) of them, possibly none.  They are walked in passes of rt_pass_frames
// output frames, and a pass is fr_pass() of frames_core.h, the plain head's passes 0 - 4 word for word; only the LOAD of passes 0
// and 1 is this file's:
//   num == 0  the staged frame is input frame k, loaded as live_frames_k loads it (no interpolation: the plain head's bits);
//   num != 0  both ends k and k + 1 are loaded that way -- the root placed, the joints' quaternions from their two-axis encoding
//             -- and the staged frame is a + t (b - a) for positions and the shortest arc for rotations, t = num / L.
// Input frame k of an output can be the row's LAST frame of an earlier call: the state keeps it as the raw float32 it arrived in
// (rpos, rrot, lpos, ltxy), written once all passes are through, so the frame between two calls is computed by the same statement
// from the same bits as inside one call.  The sign rule compares with the previous OUTPUT frame, kept as in the plain head.
// The LOAD itself is retime_core.h: live_refilter.hip runs the same statement for its rows without a filter.
#include "../../include/zeggs_hip_retime.h"
#include "common.h"
#include "anim_math.h"
#include "frames_math.h"
#include "retime_math.h"
#include "frames_core.h"
#include "retime_core.h"

namespace {

static_assert(FR_LOCAL == ZEGGS_FRAMES_LOCAL && FR_WORLD == ZEGGS_FRAMES_WORLD && FR_BVH == ZEGGS_FRAMES_BVH, "the header's bits");
static_assert(sizeof(ZeggsRetimeRow) == 104, "the record of the sixth header");

__global__ __launch_bounds__(FR_THREADS) void live_retime_k(ZeggsFramesDims d, const ZeggsRetimeRow* __restrict__ recs, ZeggsRetimeRow one,
                                                             char* state) {
  extern __shared__ double rt_lds[];
  const ZeggsRetimeRow rec = recs ? recs[blockIdx.x] : one;
  if (rec.count <= 0) return;
  const int J = d.J, order = order_code(d.order);
  const int FP = rt_pass_frames(J, d.max_frames);
  const int* parents = (const int*)state;
  const int* place = parents + 2 * J;
  char* row_state = state + rt_row_offset(J, rec.row);
  FrPlace* pl = (FrPlace*)row_state;
  float* prev = (float*)(pl + 1);
  float* raw = (float*)(row_state + rt_row_raw_offset(J));
  const bool rebase = pl->rebase != 0;
  const long m0 = rt_n_out(rec.n_in, rec.L, rec.M);
  const long outs = rt_n_out(rec.n_in + rec.count, rec.L, rec.M) - m0;
  double* lq = rt_lds;
  double* lp = rt_lds + (size_t)FP * (J + 1) * 4;
  for (long f0 = 0; f0 < outs; f0 += FP) {
    const int n = (int)(outs - f0 < FP ? outs - f0 : FP);
    fr_pass(RtLoad{rec, pl, raw, m0 + f0, J, rebase}, J, order, d.what, parents, place, prev, lq, lp, f0, n, m0 == 0 ? 0L : -1L, rec.local,
            rec.world, rec.bvh);
  }
  // the last input frame stays, raw (every pass ends behind a barrier: nothing reads the kept frame any more)
  const long last = rec.count - 1;
  const float* row = rec.pose + last * rec.pose_ld;
  for (int i = threadIdx.x; i < rt_raw_floats(J); i += FR_THREADS)
    raw[i] = i < 3 ? rec.rpos[last * rec.rpos_ld + i] : i < 7 ? rec.rrot[last * rec.rrot_ld + i - 3] : row[fr_pose_lpos(0) + i - 7];
  if (threadIdx.x == 0) pl->started = 1;
}

}  // namespace

#include "frames_host.h"      // the host contract the three forms of the head share

namespace {

int rt_dims_ok(const ZeggsFramesDims* d, const void* state, size_t state_bytes) {
  ZTRY(fh_shape_ok("retime", d));
  return lh_block_ok("retime", "state", state, state_bytes, (size_t)rt_state_bytes(d->rows, d->J), 8);
}

}  // namespace

extern "C" int zeggs_live_retime_version(void) { return 1; }

extern "C" size_t zeggs_live_retime_state_bytes(const ZeggsFramesDims* d) {
  if (rt_dims_ok(d, nullptr, (size_t)-1) != 0) return 0;
  return (size_t)rt_state_bytes(d->rows, d->J);
}

extern "C" int zeggs_live_retime_prepare(const ZeggsFramesDims* d, const int* parents, const int* seq, void* state, size_t state_bytes,
                                         void* stream) {
  ZTRY(rt_dims_ok(d, state, state_bytes));
  return fh_prepare("retime", d, parents, seq, state, stream);
}

extern "C" int zeggs_live_retime_reset(const ZeggsFramesDims* d, void* state, size_t state_bytes, int row, const float* ref_pos,
                                       const float* ref_rot, const double* start_pos, const double* start_rot, int rebase, void* stream) {
  ZTRY(rt_dims_ok(d, state, state_bytes));
  return fh_reset("retime", "live_retime_reset", d, state, rt_row_offset(d->J, row), row, ref_pos, ref_rot, start_pos, start_rot, rebase, stream);
}

extern "C" int zeggs_live_frames_retimed(const ZeggsFramesDims* d, const ZeggsRetimeRow* rows, const ZeggsRetimeRow* rows_dev, int R, void* state,
                                         size_t state_bytes, void* stream) {
  const char* who = "retime";
  ZTRY(rt_dims_ok(d, state, state_bytes));
  ZTRY(lh_count_ok(who, R, d->rows));
  if (R == 0) return 0;
  ZCHECK(rows != nullptr, "%s: NULL records", who);
  bool seen[ZEGGS_LIVE_MAX_ROWS] = {};
  bool work = false;
  const int J = d->J;
  for (int i = 0; i < R; ++i) {
    const ZeggsRetimeRow& w = rows[i];
    ZTRY(fh_row_ok(who, i, w, d, seen));
    ZTRY(fh_ratio_ok(who, i, w));
    const long want = rt_n_out(w.n_in + w.count, w.L, w.M) - rt_n_out(w.n_in, w.L, w.M);
    ZCHECK(w.outputs == want, "%s: record %d: %ld outputs disagree with n_out(%ld) - n_out(%ld) = %ld at %d / %d", who, i, w.outputs,
           w.n_in + w.count, w.n_in, want, w.L, w.M);
    if (w.count == 0) continue;
    ZTRY(lh_sources_ok(who, i, w, fr_pose_floats_read(J)));
    if (w.outputs > 0) ZTRY(fh_dests_ok(who, i, w, d->what));
    work = true;
  }
  if (!work) return 0;
  ZTRY(lh_dev_ok(who, "rows_dev", rows_dev, R, 8));
  hipLaunchKernelGGL(live_retime_k, dim3((unsigned)R), dim3(FR_THREADS), (size_t)rt_lds_bytes(J, d->max_frames), (hipStream_t)stream, *d, rows_dev,
                     rows[0], (char*)state);
  ZLAUNCH_CHECK("live_retime");
  return 0;
}
