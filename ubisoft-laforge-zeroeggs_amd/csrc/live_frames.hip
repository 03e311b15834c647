// Live serving: the output head -- the decoder's raw rows of every stream that advanced, turned into renderer-ready frames
// (include/zeggs_hip_frames.h; the layouts and the sign rule are frames_math.h, the definition DESIGN.md 3.7).
//
// One workgroup of 256 threads per record, ONE launch per step whatever the number of rows.  A record's frames are walked in
// PASSES of fr_pass_frames (all of them at the shipped sizes: 20 frames of 75 joints take 85 KB in float64, so 15 fit the 64 KB
// a workgroup may have and a first step goes in two passes).  A pass:
//   0. a thread per frame places the root (re-basing as pose_to_bvh_table_k) -> LDS, and LOCAL's root position;
//   1. a thread per (frame, joint): the joint's quaternion from its two-axis encoding (dq_from_xy, float64) and its position
//      -> LDS; LOCAL's lpos and the joint's three BVH channels (the root folded into joint 0) leave from here;
//   2. a thread per joint walks the pass's frames in order: the sign rule on lrot (and, one thread, root_rot) -> LOCAL;
//   3. a thread per frame walks the joints in index order: forward kinematics in place in LDS (a parent comes before its
//      children, so one sweep does it), the placed root folded into joint 0;
//   4. a thread per joint walks the frames in order again: gpos and the sign rule on grot -> WORLD.
// The passes are fr_pass() of frames_core.h, shared with the re-timing head (live_retime.hip); only the load of 0. and 1. is this file's.
// The sign rule compares with what was EMITTED for the stream's previous frame (float32): within a pass that is a register,
// across passes and calls the row's state, which the thread that owns the joint reads at the start of a pass and writes at its
// end.  The same statement computes a frame wherever it falls, so a stream's frames are the same bits however it is cut into
// calls, and rows share nothing but the launch.  Float64 throughout, as anim.hip; 20 frames cost two passes of five barriers.
#include "../../include/zeggs_hip_frames.h"
#include "common.h"
#include "anim_math.h"
#include "frames_math.h"
#include "frames_core.h"

namespace {

static_assert(FR_LOCAL == ZEGGS_FRAMES_LOCAL && FR_WORLD == ZEGGS_FRAMES_WORLD && FR_BVH == ZEGGS_FRAMES_BVH, "the header's bits");

// the LOAD of passes 0 and 1: a staged frame is a decoder frame of the record
struct FrLoadRows {
  ZeggsFramesRow rec;
  const FrPlace* pl;
  long f0;
  int J;
  bool rebase;
  __device__ __forceinline__ void root(int t, DQ& rr, D3& rp) const {
    const long f = f0 + t;
    fr_place_root(pl, rebase, rec.rpos + f * rec.rpos_ld, rec.rrot + f * rec.rrot_ld, rr, rp);
  }
  __device__ __forceinline__ void joint(int t, int j, DQ& q, D3& p) const {
    const float* row = rec.pose + (f0 + t) * rec.pose_ld;
    const float* x = row + fr_pose_ltxy(J, j);
    q = dq_from_xy(ldf3(x), ldf3(x + 3));
    p = ldf3(row + fr_pose_lpos(j));
  }
};

__global__ __launch_bounds__(FR_THREADS) void live_frames_k(ZeggsFramesDims d, const ZeggsFramesRow* __restrict__ recs, ZeggsFramesRow one,
                                                             char* state) {
  extern __shared__ double fr_lds[];
  const ZeggsFramesRow rec = recs ? recs[blockIdx.x] : one;
  if (rec.count <= 0) return;
  const int J = d.J, order = order_code(d.order);
  const int FP = fr_pass_frames(J, d.max_frames);
  const int* parents = (const int*)state;
  const int* place = parents + 2 * J;
  FrPlace* pl = (FrPlace*)(state + fr_row_offset(J, rec.row));
  float* prev = (float*)(pl + 1);
  const bool rebase = pl->rebase != 0, opened = pl->started == 0;      // (read by every thread before thread 0 sets `started` below)
  // LDS: per frame of the pass J + 1 quaternions and J + 1 positions, slot J = the placed root
  double* lq = fr_lds;
  double* lp = fr_lds + (size_t)FP * (J + 1) * 4;
  for (int f0 = 0; f0 < rec.count; f0 += FP) {
    const int n = rec.count - f0 < FP ? rec.count - f0 : FP;
    fr_pass(FrLoadRows{rec, pl, f0, J, rebase}, J, order, d.what, parents, place, prev, lq, lp, f0, n, opened ? 0L : -1L, rec.local, rec.world,
            rec.bvh);
  }
  if (threadIdx.x == 0) pl->started = 1;
}

}  // namespace

#include "frames_host.h"      // the host contract the three forms of the head share

namespace {

int fr_dims_ok(const ZeggsFramesDims* d, const void* state, size_t state_bytes) {
  ZTRY(fh_shape_ok("frames", d));
  return lh_block_ok("frames", "state", state, state_bytes, (size_t)fr_state_bytes(d->rows, d->J), 8);
}

}  // namespace

extern "C" int zeggs_live_frames_version(void) { return 1; }

extern "C" size_t zeggs_live_frames_state_bytes(const ZeggsFramesDims* d) {
  if (fr_dims_ok(d, nullptr, (size_t)-1) != 0) return 0;
  return (size_t)fr_state_bytes(d->rows, d->J);
}

extern "C" int zeggs_live_frames_prepare(const ZeggsFramesDims* d, const int* parents, const int* seq, void* state, size_t state_bytes,
                                         void* stream) {
  ZTRY(fr_dims_ok(d, state, state_bytes));
  return fh_prepare("frames", d, parents, seq, state, stream);
}

extern "C" int zeggs_live_frames_reset(const ZeggsFramesDims* d, void* state, size_t state_bytes, int row, const float* ref_pos,
                                       const float* ref_rot, const double* start_pos, const double* start_rot, int rebase, void* stream) {
  ZTRY(fr_dims_ok(d, state, state_bytes));
  return fh_reset("frames", "live_frames_reset", d, state, fr_row_offset(d->J, row), row, ref_pos, ref_rot, start_pos, start_rot, rebase, stream);
}

extern "C" int zeggs_live_frames(const ZeggsFramesDims* d, const ZeggsFramesRow* rows, const ZeggsFramesRow* rows_dev, int R, void* state,
                                 size_t state_bytes, void* stream) {
  const char* who = "frames";
  ZTRY(fr_dims_ok(d, state, state_bytes));
  ZTRY(lh_count_ok(who, R, d->rows));
  if (R == 0) return 0;
  ZCHECK(rows != nullptr, "%s: NULL records", who);
  bool seen[ZEGGS_LIVE_MAX_ROWS] = {};
  bool work = false;
  const int J = d->J;
  for (int i = 0; i < R; ++i) {
    const ZeggsFramesRow& w = rows[i];
    ZTRY(fh_row_ok(who, i, w, d, seen));
    if (w.count == 0) continue;
    ZTRY(lh_sources_ok(who, i, w, fr_pose_floats_read(J)));
    ZTRY(fh_dests_ok(who, i, w, d->what));
    work = true;
  }
  if (!work) return 0;
  ZTRY(lh_dev_ok(who, "rows_dev", rows_dev, R, 8));
  hipLaunchKernelGGL(live_frames_k, dim3((unsigned)R), dim3(FR_THREADS), (size_t)fr_lds_bytes(J, d->max_frames), (hipStream_t)stream, *d, rows_dev,
                     rows[0], (char*)state);
  ZLAUNCH_CHECK("live_frames");
  return 0;
}
