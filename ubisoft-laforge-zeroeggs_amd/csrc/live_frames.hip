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

__global__ void live_frames_reset_k(FrPlace place, char* row_state) { *(FrPlace*)row_state = place; }

int fr_dims_ok(const ZeggsFramesDims* d, const void* state, size_t state_bytes) {
  ZCHECK(d != nullptr, "frames: NULL dims");
  ZCHECK(d->rows >= 1 && d->rows <= ZEGGS_LIVE_MAX_ROWS, "frames: %d rows (1..%d)", d->rows, ZEGGS_LIVE_MAX_ROWS);
  const int why = fr_shape_refused(d->J, d->max_frames);
  ZCHECK(why != 1, "frames: %d joints (1..%d)", d->J, FR_MAX_JOINTS);
  ZCHECK(why != 2, "frames: max_frames %d (1..%d)", d->max_frames, FR_MAX_FRAMES);
  ZCHECK(why == 0, "frames: a frame of %d joints needs %ld bytes of LDS, the kernel may have %d", d->J, fr_frame_lds_bytes(d->J), FR_LDS_BYTES);
  ZCHECK(d->what >= 1 && d->what <= (FR_LOCAL | FR_WORLD | FR_BVH), "frames: what = %d (a mask of LOCAL 1 | WORLD 2 | BVH 4)", d->what);
  ZCHECK(order_code(d->order) == ORDER_ZYX || d->order == ORDER_XZY, "frames: channel order %d (\"zyx\" and \"xzy\" are supported)", d->order);
  if (state_bytes != (size_t)-1) {
    ZCHECK(state != nullptr, "frames: NULL state");
    ZCHECK(state_bytes >= (size_t)fr_state_bytes(d->rows, d->J), "frames: state too small (%zu < %zu)", state_bytes,
           (size_t)fr_state_bytes(d->rows, d->J));
    ZCHECK((uintptr_t)state % 8 == 0, "frames: misaligned state");
  }
  return 0;
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
  ZCHECK(parents != nullptr && seq != nullptr, "frames prepare: NULL parents / seq");
  const int J = d->J;
  int bad = fr_bad_parent(parents, J);
  ZCHECK(bad != 0, "frames prepare: parents[0] = %d (the root has parent -1)", parents[0]);
  ZCHECK(bad < 0, "frames prepare: parents[%d] = %d (a parent comes before its children: 0 .. %d)", bad, parents[bad], bad - 1);
  int tables[3 * FR_MAX_JOINTS];
  bad = fr_bad_seq(seq, J, tables + 2 * J);
  ZCHECK(bad < 0, "frames prepare: seq[%d] = %d: seq is no permutation of 0 .. %d", bad, seq[bad], J - 1);
  memcpy(tables, parents, sizeof(int) * J);
  memcpy(tables + J, seq, sizeof(int) * J);
  // once per server, never on the tick path: the copy is waited for, `tables` is gone when the call returns
  hipError_t e = hipMemcpyAsync(state, tables, sizeof(int) * 3 * J, hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  ZCHECK(e == hipSuccess, "frames prepare: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int zeggs_live_frames_reset(const ZeggsFramesDims* d, void* state, size_t state_bytes, int row, const float* ref_pos,
                                       const float* ref_rot, const double* start_pos, const double* start_rot, int rebase, void* stream) {
  ZTRY(fr_dims_ok(d, state, state_bytes));
  ZCHECK(row >= 0 && row < d->rows, "frames reset: row %d of %d", row, d->rows);
  FrPlace p = {};
  p.ref_rot[0] = p.start_rot[0] = 1.0;
  if (rebase) {
    ZCHECK(ref_pos != nullptr && ref_rot != nullptr && start_pos != nullptr && start_rot != nullptr,
           "frames reset: row %d: a placement needs ref_pos, ref_rot, start_pos and start_rot", row);
    for (int i = 0; i < 3; ++i) { p.ref_pos[i] = (double)ref_pos[i]; p.start_pos[i] = start_pos[i]; }
    for (int i = 0; i < 4; ++i) { p.ref_rot[i] = (double)ref_rot[i]; p.start_rot[i] = start_rot[i]; }
    p.rebase = 1;
  }
  hipLaunchKernelGGL(live_frames_reset_k, dim3(1), dim3(1), 0, (hipStream_t)stream, p, (char*)state + fr_row_offset(d->J, row));
  ZLAUNCH_CHECK("live_frames_reset");
  return 0;
}

extern "C" int zeggs_live_frames(const ZeggsFramesDims* d, const ZeggsFramesRow* rows, const ZeggsFramesRow* rows_dev, int R, void* state,
                                 size_t state_bytes, void* stream) {
  const char* who = "frames";
  ZTRY(fr_dims_ok(d, state, state_bytes));
  ZCHECK(R >= 0 && R <= d->rows, "%s: %d records for %d rows", who, R, d->rows);
  if (R == 0) return 0;
  ZCHECK(rows != nullptr, "%s: NULL records", who);
  bool seen[ZEGGS_LIVE_MAX_ROWS] = {};
  bool work = false;
  const int J = d->J;
  for (int i = 0; i < R; ++i) {
    const ZeggsFramesRow& w = rows[i];
    ZCHECK(w.row >= 0 && w.row < d->rows, "%s: record %d: row %d of %d", who, i, w.row, d->rows);
    ZCHECK(!seen[w.row], "%s: record %d: row %d twice in one call", who, i, w.row);
    seen[w.row] = true;
    ZCHECK(w.count >= 0, "%s: record %d: negative count %d", who, i, w.count);
    ZCHECK(w.count <= d->max_frames, "%s: record %d: %d frames, max_frames is %d", who, i, w.count, d->max_frames);
    if (w.count == 0) continue;
    ZCHECK(w.pose != nullptr && (uintptr_t)w.pose % 4 == 0 && w.rpos != nullptr && (uintptr_t)w.rpos % 4 == 0 && w.rrot != nullptr &&
               (uintptr_t)w.rrot % 4 == 0, "%s: record %d: NULL or misaligned source", who, i);
    ZCHECK(w.pose_ld >= fr_pose_floats_read(J) && w.rpos_ld >= 3 && w.rrot_ld >= 4,
           "%s: record %d: leading dimensions %ld, %ld, %ld (at least %d, 3, 4 floats)", who, i, w.pose_ld, w.rpos_ld, w.rrot_ld,
           fr_pose_floats_read(J));
    ZCHECK(!(d->what & FR_LOCAL) || (w.local != nullptr && (uintptr_t)w.local % 4 == 0), "%s: record %d: NULL or misaligned LOCAL destination",
           who, i);
    ZCHECK(!(d->what & FR_WORLD) || (w.world != nullptr && (uintptr_t)w.world % 4 == 0), "%s: record %d: NULL or misaligned WORLD destination",
           who, i);
    ZCHECK(!(d->what & FR_BVH) || (w.bvh != nullptr && (uintptr_t)w.bvh % 8 == 0), "%s: record %d: NULL or misaligned BVH destination", who, i);
    work = true;
  }
  if (!work) return 0;
  ZCHECK(rows_dev != nullptr || R == 1, "%s: %d records must also be in device memory (rows_dev)", who, R);
  ZCHECK(rows_dev == nullptr || (uintptr_t)rows_dev % 8 == 0, "%s: misaligned rows_dev", who);
  hipLaunchKernelGGL(live_frames_k, dim3((unsigned)R), dim3(FR_THREADS), (size_t)fr_lds_bytes(J, d->max_frames), (hipStream_t)stream, *d, rows_dev,
                     rows[0], (char*)state);
  ZLAUNCH_CHECK("live_frames");
  return 0;
}
