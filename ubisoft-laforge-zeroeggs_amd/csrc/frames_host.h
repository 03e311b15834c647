// The host contract of the output head of live serving, stated once for its three forms: the plain head (live_frames.hip), the
// head at each stream's own frame rate (live_retime.hip) and that head with its filter stage (live_refilter.hip).  What a dims
// record may hold, how the skeleton tables are written, what a reset stores and what makes a record acceptable are decided
// here; an entry point keeps what is its own -- the order of its checks, its `outputs` rule, its skip and `work` conditions and
// its launch.  Nothing here asks which form calls it: a form that needs more makes a call of its own between these.
// `who` is the form's word in every message ("frames", "retime", "refilter"), `i` the index of the record a message names.
// What the head shares with every other stage of live serving -- the head of the dims record, the state block, the row of a
// single-row call, a record's row once a call, the device copy of the records -- is live_host.h's, called from here.
// Host code, and the one kernel of a reset: include it behind a unit's own kernels (common.h, anim_math.h, frames_math.h and
// frames_core.h first), so that they stay the first of its code object.
#pragma once
#include "live_host.h"
#include "retime_math.h"

namespace {

// ---- the dims record.  The shape: what the three kernels take alike
int fh_shape_ok(const char* who, const ZeggsFramesDims* d) {
  ZTRY(lh_dims_ok(who, d));
  const int why = fr_shape_refused(d->J, d->max_frames);
  ZCHECK(why != 1, "%s: %d joints (1..%d)", who, d->J, FR_MAX_JOINTS);
  ZCHECK(why != 2, "%s: max_frames %d (1..%d)", who, d->max_frames, FR_MAX_FRAMES);
  ZCHECK(why == 0, "%s: a frame of %d joints needs %ld bytes of LDS, the kernel may have %d", who, d->J, fr_frame_lds_bytes(d->J), FR_LDS_BYTES);
  ZCHECK(d->what >= 1 && d->what <= (FR_LOCAL | FR_WORLD | FR_BVH), "%s: what = %d (a mask of LOCAL 1 | WORLD 2 | BVH 4)", who, d->what);
  ZCHECK(order_code(d->order) == ORDER_ZYX || d->order == ORDER_XZY, "%s: channel order %d (\"zyx\" and \"xzy\" are supported)", who, d->order);
  return 0;
}
// (the state block against the form's own size: lh_block_ok(who, "state", state, state_bytes, need, 8))

// ---- prepare, behind the form's dims check: the skeleton tables [parents | seq | place] to the front of the state
int fh_prepare(const char* who, const ZeggsFramesDims* d, const int* parents, const int* seq, void* state, void* stream) {
  ZCHECK(parents != nullptr && seq != nullptr, "%s prepare: NULL parents / seq", who);
  const int J = d->J;
  int bad = fr_bad_parent(parents, J);
  ZCHECK(bad != 0, "%s prepare: parents[0] = %d (the root has parent -1)", who, parents[0]);
  ZCHECK(bad < 0, "%s prepare: parents[%d] = %d (a parent comes before its children: 0 .. %d)", who, bad, parents[bad], bad - 1);
  int tables[3 * FR_MAX_JOINTS];
  bad = fr_bad_seq(seq, J, tables + 2 * J);
  ZCHECK(bad < 0, "%s prepare: seq[%d] = %d: seq is no permutation of 0 .. %d", who, bad, seq[bad], J - 1);
  memcpy(tables, parents, sizeof(int) * J);
  memcpy(tables + J, seq, sizeof(int) * J);
  // once per server, never on the tick path: the copy is waited for, `tables` is gone when the call returns
  hipError_t e = hipMemcpyAsync(state, tables, sizeof(int) * 3 * J, hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  ZCHECK(e == hipSuccess, "%s prepare: %s", who, hipGetErrorString(e));
  return 0;
}

// ---- reset, behind the form's dims check: the placement to the front of the row's state, which starts at state + row_offset
// (the form's own layout; an offset, so that no address is formed before `row` has passed).  `name`: the launch's
__global__ void live_head_reset_k(FrPlace place, char* row_state) { *(FrPlace*)row_state = place; }

int fh_reset(const char* who, const char* name, const ZeggsFramesDims* d, void* state, long row_offset, int row, const float* ref_pos,
             const float* ref_rot, const double* start_pos, const double* start_rot, int rebase, void* stream) {
  ZTRY(lh_row_ok(who, "reset", row, d->rows));
  FrPlace p = {};
  p.ref_rot[0] = p.start_rot[0] = 1.0;
  if (rebase) {
    ZCHECK(ref_pos != nullptr && ref_rot != nullptr && start_pos != nullptr && start_rot != nullptr,
           "%s reset: row %d: a placement needs ref_pos, ref_rot, start_pos and start_rot", who, row);
    for (int i = 0; i < 3; ++i) { p.ref_pos[i] = (double)ref_pos[i]; p.start_pos[i] = start_pos[i]; }
    for (int i = 0; i < 4; ++i) { p.ref_rot[i] = (double)ref_rot[i]; p.start_rot[i] = start_rot[i]; }
    p.rebase = 1;
  }
  hipLaunchKernelGGL(live_head_reset_k, dim3(1), dim3(1), 0, (hipStream_t)stream, p, (char*)state + row_offset);
  ZLAUNCH_CHECK(name);
  return 0;
}

// ---- a record (ZeggsFramesRow, ZeggsRetimeRow, ZeggsRefilterRow: the shared fields have the same names)
// its row, once a call (`seen`: one flag a row, the caller's), and its count of input frames
template <class Row>
int fh_row_ok(const char* who, int i, const Row& w, const ZeggsFramesDims* d, bool* seen) {
  ZTRY(lh_once_ok(who, i, w.row, d->rows, seen));
  ZCHECK(w.count >= 0, "%s: record %d: negative count %d", who, i, w.count);
  ZCHECK(w.count <= d->max_frames, "%s: record %d: %d frames, max_frames is %d", who, i, w.count, d->max_frames);
  return 0;
}
// the ratio and the input counter of a re-timing record
template <class Row>
int fh_ratio_ok(const char* who, int i, const Row& w) {
  const int why = rt_ratio_refused(w.L, w.M);
  ZCHECK(why != 1 && why != 2, "%s: record %d: ratio %d / %d (1 <= L, M <= %d)", who, i, w.L, w.M, RT_MAX_TERM);
  ZCHECK(why != 3, "%s: record %d: ratio %d / %d is not in lowest terms", who, i, w.L, w.M);
  ZCHECK(why == 0, "%s: record %d: ratio %d / %d is above %d", who, i, w.L, w.M, RT_MAX_UP);
  ZCHECK(w.n_in >= 0 && w.n_in <= (1L << 40), "%s: record %d: input counter %ld", who, i, w.n_in);
  return 0;
}
// (the sources of a record that brings frames: lh_sources_ok(who, i, w, fr_pose_floats_read(J)), which the plant stage calls
// with the whole pose row -- this header has a kernel, so a unit that is no head cannot include it)
// the destinations of a record that emits frames: those `what` asks for
template <class Row>
int fh_dests_ok(const char* who, int i, const Row& w, int what) {
  ZCHECK(!(what & FR_LOCAL) || (w.local != nullptr && (uintptr_t)w.local % 4 == 0), "%s: record %d: NULL or misaligned LOCAL destination", who, i);
  ZCHECK(!(what & FR_WORLD) || (w.world != nullptr && (uintptr_t)w.world % 4 == 0), "%s: record %d: NULL or misaligned WORLD destination", who, i);
  ZCHECK(!(what & FR_BVH) || (w.bvh != nullptr && (uintptr_t)w.bvh % 8 == 0), "%s: record %d: NULL or misaligned BVH destination", who, i);
  return 0;
}
// (the device copy of the records of a call that has work: lh_dev_ok(who, "rows_dev", rows_dev, R, 8))

}  // namespace
