// Live serving: feet that stay planted -- the contact lock and the leg IK between the decoder's raw rows and the output head
// (include/zeggs_hip_plant.h; the arithmetic is plant_math.h, the definition DESIGN.md 3.7).
//
// One workgroup of 256 threads per record, ONE launch per step whatever the number of rows.  A record's frames are walked in
// passes of PL_PASS_FRAMES; a pass of n frames and C chains:
//   1. a thread per (frame, chain): FK over the ancestors of the chain's foot from the RAW row, bottom up (the head's dq_from_xy,
//      the root folded into joint 0; every rotation brought to unit length first, so that FK is rigid) -> LDS: the unconstrained H, K, A, the world rotation of u's parent and the root's rotation;
//   2. a thread per chain walks the pass's frames in order through the state machine (pl_step): the frame's target -> LDS, its
//      contact flag -> the record's flags.  The chain's state lives in registers from the record's first frame to its last;
//   3. a thread per (frame, chain): the two-bone solve (pl_solve) and the ltxy of u, m, e -> the corrected row -- or, for a target
//      that is the unconstrained ankle, those 18 floats as they came;
//   4. all threads copy every other float of the rows (no address is written twice, so no order between 3. and 4. is needed).
// Float64 throughout; the staged values of a (frame, chain) are PL_SLOT doubles, 32 frames of 4 chains take 21 KB of LDS.
// Plain loads and stores.
#include "../../include/zeggs_hip_plant.h"
#include "common.h"
#include "anim_math.h"
#include "plant_math.h"

#include <math.h>

namespace {

static_assert(PL_MAX_CHAINS == ZEGGS_PLANT_MAX_CHAINS && sizeof(PlantChain) == ZEGGS_PLANT_CHAIN_BYTES, "plant_math.h and the eleventh header disagree");
static_assert(PL_PASS_FRAMES * PL_MAX_CHAINS * PL_SLOT * 8 <= 32768, "the LDS of a pass");

__device__ __forceinline__ PlantOpts pl_opts(const ZeggsPlantDims& d) {
  return PlantOpts{d.dt, d.v_on, d.v_off, d.h_on, d.h_off, d.ground, d.slack, d.stretch, d.release};
}
__device__ __forceinline__ PlV pv(D3 a) { return PlV{a.x, a.y, a.z}; }
__device__ __forceinline__ PlQ pq(DQ q) { return PlQ{q.w, q.x, q.y, q.z}; }
__device__ __forceinline__ D3 ldf3p(const float* p) { return D3{(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ DQ dq_unit(DQ q) {
  const double n = 1.0 / sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  return DQ{n * q.w, n * q.x, n * q.y, n * q.z};
}
// a joint's local rotation: the head's dq_from_xy, then of unit length (its 1e-10 leaves it a hair short), so that FK is rigid
__device__ __forceinline__ DQ joint_rot(const float* row, int J, int j) {
  const float* x = row + pl_pose_ltxy(J, j);
  return dq_unit(dq_from_xy(ldf3p(x), ldf3p(x + 3)));
}

__global__ void live_plant_reset_k(PlantChain* row) {
  const int i = threadIdx.x;
  if (blockIdx.x != 0 || i >= PL_MAX_CHAINS) return;
  PlantChain s = {};
  s.mode = PL_FREE;
  row[i] = s;
}

__global__ __launch_bounds__(PL_THREADS) void live_plant_k(ZeggsPlantDims d, const ZeggsPlantRow* __restrict__ recs, ZeggsPlantRow one, char* state) {
  __shared__ double lds[PL_PASS_FRAMES * PL_MAX_CHAINS * PL_SLOT];
  __shared__ int chain[3 * PL_MAX_CHAINS];
  const ZeggsPlantRow rec = recs ? recs[blockIdx.x] : one;
  if (rec.count <= 0) return;
  const int tid = threadIdx.x, J = d.J, C = d.chains, PO = pl_pose_floats(J);
  const int* parents = (const int*)state;
  if (tid < 3 * PL_MAX_CHAINS) {      // (a state that was never prepared must not send an access astray)
    const int j = parents[J + tid];
    chain[tid] = tid < 3 * C && (unsigned)j < (unsigned)J ? j : -1;
  }
  __syncthreads();
  const PlantOpts o = pl_opts(d);
  PlantChain* rows = (PlantChain*)(state + pl_row_offset(J, rec.row));
  PlantChain st = {};
  if (tid < C) st = rows[tid];
  for (int f0 = 0; f0 < rec.count; f0 += PL_PASS_FRAMES) {
    const int n = rec.count - f0 < PL_PASS_FRAMES ? rec.count - f0 : PL_PASS_FRAMES;
    // ---- 1. the unconstrained chain
    for (int i = tid; i < n * C; i += PL_THREADS) {
      const int t = i / C, c = i - t * C;
      const long f = f0 + t;
      const int u = chain[3 * c], m = chain[3 * c + 1], e = chain[3 * c + 2];
      double* s = lds + (size_t)i * PL_SLOT;
      if (u < 0 || m < 0 || e < 0) {
        for (int k = 0; k < PL_SLOT; ++k) s[k] = 0.0;
        continue;
      }
      const float* row = rec.pose + f * rec.pose_ld;
      const float* rp = rec.rpos + f * rec.rpos_ld;
      const float* rq = rec.rrot + f * rec.rrot_ld;
      const DQ rr = dq_unit(DQ{(double)rq[0], (double)rq[1], (double)rq[2], (double)rq[3]});      // (float32: unit to 1e-7 only)
      // the world transform of u's parent, composed bottom up; the root folded into joint 0
      DQ gq = DQ{1.0, 0.0, 0.0, 0.0};
      D3 gx = D3{0.0, 0.0, 0.0};
      int a = parents[u];
      for (int guard = 0; guard < J && (unsigned)a < (unsigned)J; ++guard) {
        const DQ q = joint_rot(row, J, a);
        gx = dq_mul_vec(q, gx) + ldf3p(row + pl_pose_lpos(a));
        gq = dq_mul(q, gq);
        a = parents[a];
      }
      gx = dq_mul_vec(rr, gx) + ldf3p(rp);
      gq = dq_mul(rr, gq);
      const DQ gu = dq_mul(gq, joint_rot(row, J, u));
      const D3 H = dq_mul_vec(gq, ldf3p(row + pl_pose_lpos(u))) + gx;
      const DQ gm = dq_mul(gu, joint_rot(row, J, m));
      const D3 K = dq_mul_vec(gu, ldf3p(row + pl_pose_lpos(m))) + H;
      const D3 A = dq_mul_vec(gm, ldf3p(row + pl_pose_lpos(e))) + K;
      st3(s, H); st3(s + 3, K); st3(s + 6, A);
      stq(s + 9, gq); stq(s + 13, rr);
    }
    __syncthreads();
    // ---- 2. the state machine, frame by frame
    if (tid < C) {
      for (int t = 0; t < n; ++t) {
        double* s = lds + (size_t)(t * C + tid) * PL_SLOT;
        const PlV A = pv(ld3(s + 6));
        PlV T;
        const int held = pl_step(o, st, pv(ld3(s)), pv(ld3(s + 3)), A, T);
        s[17] = T.x; s[18] = T.y; s[19] = T.z;
        s[20] = pl_same(T, A) || chain[3 * tid] < 0 ? 0.0 : 1.0;
        rec.contacts[(long)(f0 + t) * C + tid] = (unsigned char)held;
      }
    }
    __syncthreads();
    // ---- 3. the solve; the chain's 18 floats of ltxy
    for (int i = tid; i < n * C; i += PL_THREADS) {
      const int t = i / C, c = i - t * C;
      const long f = f0 + t;
      const int j3[3] = {chain[3 * c], chain[3 * c + 1], chain[3 * c + 2]};
      if (j3[0] < 0 || j3[1] < 0 || j3[2] < 0) continue;
      const double* s = lds + (size_t)i * PL_SLOT;
      const float* row = rec.pose + f * rec.pose_ld;
      float* out = rec.out + f * rec.out_ld;
      if (s[20] == 0.0) {
        for (int k = 0; k < 3; ++k)
          for (int x = 0; x < 6; ++x) out[pl_pose_ltxy(J, j3[k]) + x] = row[pl_pose_ltxy(J, j3[k]) + x];
        continue;
      }
      PlQ q3[3] = {pq(joint_rot(row, J, j3[0])), pq(joint_rot(row, J, j3[1])), pq(joint_rot(row, J, j3[2]))};
      pl_solve(o.stretch, pv(ld3(s)), pv(ld3(s + 3)), pv(ld3(s + 6)), PlV{s[17], s[18], s[19]}, pq(ldq(s + 9)), pq(ldq(s + 13)), q3[0], q3[1], q3[2]);
      for (int k = 0; k < 3; ++k) {
        double xy[6];
        pl_to_xy(q3[k], xy);
        for (int x = 0; x < 6; ++x) out[pl_pose_ltxy(J, j3[k]) + x] = (float)xy[x];
      }
    }
    // ---- 4. every other float of the rows
    const int lo = pl_pose_ltxy(J, 0), hi = pl_pose_ltxy(J, J);
    for (int i = tid; i < n * PO; i += PL_THREADS) {
      const int t = i / PO, x = i - t * PO;
      if (x >= lo && x < hi) {
        const int j = (x - lo) / 6;
        bool mine = false;
        for (int k = 0; k < 3 * PL_MAX_CHAINS; ++k) mine = mine || chain[k] == j;
        if (mine) continue;
      }
      rec.out[(long)(f0 + t) * rec.out_ld + x] = rec.pose[(long)(f0 + t) * rec.pose_ld + x];
    }
    __syncthreads();      // (the next pass rewrites the LDS)
  }
  if (tid < C) rows[tid] = st;
}

}  // namespace

#include "live_host.h"      // the host contract every stage of live serving keeps

namespace {

int pl_dims_ok(const ZeggsPlantDims* d, const void* state, size_t state_bytes) {
  ZTRY(lh_dims_ok("plant", d));      // (pl_dims_refused's 1, the rows, is refused here: with the same words)
  const int why = pl_dims_refused(d->rows, ZEGGS_LIVE_MAX_ROWS, d->J, d->max_frames, d->chains, d->release);
  ZCHECK(why != 2, "plant: %d joints (3..%d)", d->J, PL_MAX_JOINTS);
  ZCHECK(why != 3, "plant: max_frames %d (1..%d)", d->max_frames, PL_MAX_FRAMES);
  ZCHECK(why != 4, "plant: %d chains (1..%d)", d->chains, PL_MAX_CHAINS);
  ZCHECK(why == 0, "plant: release %d frames (0..%d)", d->release, PL_MAX_RELEASE);
  const PlantOpts o = {d->dt, d->v_on, d->v_off, d->h_on, d->h_off, d->ground, d->slack, d->stretch, d->release};
  const int bad = pl_opts_refused(o);
  ZCHECK(bad != 1, "plant: frame time %g (> 0)", d->dt);
  ZCHECK(bad != 2, "plant: speed thresholds on %g, off %g (0 <= on <= off)", d->v_on, d->v_off);
  ZCHECK(bad != 3, "plant: height thresholds on %g, off %g (on <= off)", d->h_on, d->h_off);
  ZCHECK(bad != 4, "plant: ground %g", d->ground);
  ZCHECK(bad != 5, "plant: slack %g (>= 0)", d->slack);
  ZCHECK(bad == 0, "plant: stretch %g (0 < stretch <= 1)", d->stretch);
  return lh_block_ok("plant", "state", state, state_bytes, (size_t)pl_state_bytes(d->rows, d->J), 8);
}

}  // namespace

extern "C" int zeggs_live_plant_version(void) { return 1; }

extern "C" size_t zeggs_live_plant_state_bytes(const ZeggsPlantDims* d) {
  if (pl_dims_ok(d, nullptr, (size_t)-1) != 0) return 0;
  return (size_t)pl_state_bytes(d->rows, d->J);
}

extern "C" int zeggs_live_plant_prepare(const ZeggsPlantDims* d, const int* parents, const int* chains, void* state, size_t state_bytes,
                                        void* stream) {
  ZTRY(pl_dims_ok(d, state, state_bytes));
  ZCHECK(parents != nullptr && chains != nullptr, "plant prepare: NULL parents / chains");
  const int J = d->J;
  ZCHECK(parents[0] == -1, "plant prepare: parents[0] = %d (the root has parent -1)", parents[0]);
  for (int j = 1; j < J; ++j)
    ZCHECK(parents[j] >= 0 && parents[j] < j, "plant prepare: parents[%d] = %d (a parent comes before its children: 0 .. %d)", j, parents[j], j - 1);
  int why = 0;
  const int bad = pl_bad_chain(parents, J, chains, d->chains, &why);
  if (bad >= 0) {
    const int* c = chains + 3 * bad;
    ZCHECK(why != 1, "plant prepare: chain %d (%d, %d, %d): a joint outside 0 .. %d", bad, c[0], c[1], c[2], J - 1);
    ZCHECK(why != 2, "plant prepare: chain %d (%d, %d, %d) is no chain: parents[%d] = %d, parents[%d] = %d", bad, c[0], c[1], c[2], c[1],
           parents[c[1]], c[2], parents[c[2]]);
    ZCHECK(false, "plant prepare: chain %d (%d, %d, %d) shares a joint with an earlier chain", bad, c[0], c[1], c[2]);
  }
  int tables[PL_MAX_JOINTS + 3 * PL_MAX_CHAINS];
  memcpy(tables, parents, sizeof(int) * J);
  for (int i = 0; i < 3 * PL_MAX_CHAINS; ++i) tables[J + i] = i < 3 * d->chains ? chains[i] : -1;
  // once per server, never on the tick path: the copy is waited for, `tables` is gone when the call returns
  hipError_t e = hipMemcpyAsync(state, tables, sizeof(int) * (J + 3 * PL_MAX_CHAINS), hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  ZCHECK(e == hipSuccess, "plant prepare: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int zeggs_live_plant_reset(const ZeggsPlantDims* d, void* state, size_t state_bytes, int row, void* stream) {
  ZTRY(pl_dims_ok(d, state, state_bytes));
  ZTRY(lh_row_ok("plant", "reset", row, d->rows));
  hipLaunchKernelGGL(live_plant_reset_k, dim3(1), dim3(64), 0, (hipStream_t)stream, (PlantChain*)((char*)state + pl_row_offset(d->J, row)));
  ZLAUNCH_CHECK("live_plant_reset");
  return 0;
}

extern "C" int zeggs_live_plant_spans(const ZeggsPlantDims* d, int row, ZeggsSnapSpan* spans, int max_spans) {
  if (zeggs_live_plant_state_bytes(d) == 0) return -1;
  const bool has = row >= 0 && row < d->rows;
  const size_t o = has ? (size_t)pl_row_offset(d->J, row) : 0, b = (size_t)pl_row_bytes();
  return lh_spans_out("plant spans", has ? 1 : -1, row, d->rows, max_spans, &o, &b, spans);
}

extern "C" int zeggs_live_plant(const ZeggsPlantDims* d, const ZeggsPlantRow* recs, const ZeggsPlantRow* recs_dev, int R, void* state,
                                size_t state_bytes, void* stream) {
  const char* who = "plant";
  ZTRY(pl_dims_ok(d, state, state_bytes));
  ZTRY(lh_count_ok(who, R, d->rows));
  if (R == 0) return 0;
  ZCHECK(recs != nullptr, "plant: NULL records");
  bool seen[ZEGGS_LIVE_MAX_ROWS] = {};
  bool work = false;
  const int PO = pl_pose_floats(d->J);
  for (int i = 0; i < R; ++i) {
    const ZeggsPlantRow& w = recs[i];
    ZTRY(lh_once_ok(who, i, w.row, d->rows, seen));
    ZCHECK(w.count >= 0, "plant: record %d: negative count %d", i, w.count);
    ZCHECK(w.count <= d->max_frames, "plant: record %d: %d frames, max_frames is %d", i, w.count, d->max_frames);
    if (w.count == 0) continue;
    ZTRY(lh_sources_ok(who, i, w, PO));
    ZCHECK(w.out != nullptr && (uintptr_t)w.out % 4 == 0, "plant: record %d: NULL or misaligned destination", i);
    ZCHECK(w.out != w.pose, "plant: record %d: the destination is the source (the stage writes a copy)", i);
    ZCHECK(w.out_ld >= PO, "plant: record %d: destination leading dimension %ld (at least %d floats)", i, w.out_ld, PO);
    ZCHECK(w.contacts != nullptr, "plant: record %d: NULL contact flags", i);
    work = true;
  }
  if (!work) return 0;
  ZTRY(lh_dev_ok(who, "recs_dev", recs_dev, R, 8));
  hipLaunchKernelGGL(live_plant_k, dim3((unsigned)R), dim3(PL_THREADS), 0, (hipStream_t)stream, *d, recs_dev, recs[0], (char*)state);
  ZLAUNCH_CHECK("live_plant");
  return 0;
}
