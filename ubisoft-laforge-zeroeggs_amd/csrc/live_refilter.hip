// Live serving: the filter stage of the re-timing output head -- the frames of live_retime.hip with a band-limiting filter in
// front of FK for the rows that ask for one (include/zeggs_hip_refilter.h; the counting rules, the ring and the state layout are
// refilter_math.h, the definition DESIGN.md 3.7).
//
// One workgroup of 256 threads per record, ONE launch per step whatever the rows' ratios and whether they filter; a server with
// the filter stage enqueues it INSTEAD of live_retime_k.  Output frames are walked in passes of rf_pass_frames frames, and a pass
// is fr_pass() of frames_core.h, the plain head's passes 0 - 4 word for word; only the LOAD of passes 0 and 1 differs:
//   half == 0  RtLoad of retime_core.h, live_retime_k's own statement with its emission rule (the same bits);
//   half  > 0  RfLoad below: the staged frame is the weighted combination of the 2 H + 1 input frames around its position,
//              weights table[num][0 .. 2 H] in float64 -- per tap the root is placed and the joints' quaternions come from their
//              two-axis encoding as live_frames_k loads them; positions are sum w_j x_j, quaternions are brought to the centre
//              tap's side, summed and normalised; ascending j, one accumulator of explicit fma().
// A tap's input frame is one of the call's or, when it came with an earlier call, one of the row's ring: the state keeps the last
// 2 max_half input frames as the raw float32 they arrived in, frame i in slot i mod 2 max_half, in global memory (L2), so a frame
// whose taps span two calls is computed by the same statement from the same bits as inside one call.  The ring is rewritten only
// when all passes are through (every pass ends behind a barrier).  The sign rule compares with the previous OUTPUT frame.
#include "../../include/zeggs_hip_refilter.h"
#include "common.h"
#include "anim_math.h"
#include "frames_math.h"
#include "retime_math.h"
#include "refilter_math.h"
#include "frames_core.h"
#include "retime_core.h"

namespace {

static_assert(FR_LOCAL == ZEGGS_FRAMES_LOCAL && FR_WORLD == ZEGGS_FRAMES_WORLD && FR_BVH == ZEGGS_FRAMES_BVH, "the header's bits");
static_assert(sizeof(ZeggsRefilterRow) == 120 && offsetof(ZeggsRefilterRow, table) == sizeof(ZeggsRetimeRow), "the record of the seventh header");
static_assert(offsetof(ZeggsRefilterRow, M) == offsetof(ZeggsRetimeRow, M) && offsetof(ZeggsRefilterRow, n_in) == offsetof(ZeggsRetimeRow, n_in),
              "the sixth header's fields where they sit there");

__device__ __forceinline__ ZeggsRetimeRow rf_plain(const ZeggsRefilterRow& w) {
  return ZeggsRetimeRow{w.pose, w.rpos, w.rrot, w.local, w.world, w.bvh, w.pose_ld, w.rpos_ld, w.rrot_ld, w.n_in, w.outputs, w.row, w.count, w.L, w.M};
}

struct RfAcc {      // one accumulator per component, explicit fma, in the order the taps come
  double a, b, c, d;
  __device__ __forceinline__ void add(double w, DQ q) { a = fma(w, q.w, a); b = fma(w, q.x, b); c = fma(w, q.y, c); d = fma(w, q.z, d); }
  __device__ __forceinline__ void add(double w, D3 p) { a = fma(w, p.x, a); b = fma(w, p.y, b); c = fma(w, p.z, c); }
  __device__ __forceinline__ DQ quat(DQ centre) const {
    const double n = sqrt(a * a + b * b + c * c + d * d);
    return n < RF_SMALL_NORM ? centre : DQ{a / n, b / n, c / n, d / n};
  }
};
__device__ __forceinline__ DQ rf_side(DQ q, DQ centre) {
  return q.w * centre.w + q.x * centre.x + q.y * centre.y + q.z * centre.z < 0.0 ? DQ{-q.w, -q.x, -q.y, -q.z} : q;
}

// the LOAD of passes 0 and 1 of a filtered row: staged frame t is output frame m0 + t of the stream
struct RfLoad {
  ZeggsRefilterRow rec;
  const FrPlace* pl;
  const float* ring;
  long m0, last;      // last: the stream's last input frame so far, n_in + count - 1 (>= 0 where a frame is staged)
  int J, max_half, RF;
  bool rebase;
  __device__ __forceinline__ const double* where(int t, long& k) const {
    long num;
    rt_position(m0 + t, rec.L, rec.M, &k, &num);
    return rec.table + num * rf_taps(rec.half);
  }
  // input frame i of the stream: rf_where says whether it is one of the call's or one of the ring's
  __device__ __forceinline__ void root_of(long i, DQ& rr, D3& rp) const {
    const long at = rf_where(i, rec.n_in, max_half);
    const float* slot = ring + (size_t)(at < 0 ? -1 - at : 0) * RF;
    fr_place_root(pl, rebase, at < 0 ? slot + rt_raw_rpos() : rec.rpos + at * rec.rpos_ld, at < 0 ? slot + rt_raw_rrot() : rec.rrot + at * rec.rrot_ld,
                  rr, rp);
  }
  __device__ __forceinline__ void joint_of(long i, int j, DQ& q, D3& p) const {
    const long at = rf_where(i, rec.n_in, max_half);
    const float* slot = ring + (size_t)(at < 0 ? -1 - at : 0) * RF;
    const float* row = rec.pose + (at < 0 ? 0 : at) * rec.pose_ld;
    const float* x = at < 0 ? slot + rt_raw_ltxy(J, j) : row + fr_pose_ltxy(J, j);
    q = dq_from_xy(ldf3(x), ldf3(x + 3));
    p = ldf3(at < 0 ? slot + rt_raw_lpos(j) : row + fr_pose_lpos(j));
  }
  __device__ __forceinline__ void root(int t, DQ& rr, D3& rp) const {
    long k;
    const double* w = where(t, k);
    const int H = rec.half;
    DQ centre, q;
    D3 p;
    root_of(rf_tap_frame(k, H, H, last), centre, p);
    RfAcc aq = {0.0, 0.0, 0.0, 0.0}, ap = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < rf_taps(H); ++j) {
      root_of(rf_tap_frame(k, H, j, last), q, p);
      aq.add(w[j], rf_side(q, centre));
      ap.add(w[j], p);
    }
    rr = aq.quat(centre);
    rp = D3{ap.a, ap.b, ap.c};
  }
  __device__ __forceinline__ void joint(int t, int jt, DQ& qo, D3& po) const {
    long k;
    const double* w = where(t, k);
    const int H = rec.half;
    DQ centre, q;
    D3 p;
    joint_of(rf_tap_frame(k, H, H, last), jt, centre, p);
    RfAcc aq = {0.0, 0.0, 0.0, 0.0}, ap = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < rf_taps(H); ++j) {
      joint_of(rf_tap_frame(k, H, j, last), jt, q, p);
      aq.add(w[j], rf_side(q, centre));
      ap.add(w[j], p);
    }
    qo = aq.quat(centre);
    po = D3{ap.a, ap.b, ap.c};
  }
};

__global__ __launch_bounds__(FR_THREADS) void live_refilter_k(ZeggsFramesDims d, int max_half, const ZeggsRefilterRow* __restrict__ recs,
                                                               ZeggsRefilterRow one, char* state) {
  extern __shared__ double rf_lds[];
  const ZeggsRefilterRow rec = recs ? recs[blockIdx.x] : one;
  const bool filtered = rec.half > 0;
  if (rec.count <= 0 && !(filtered && rec.final)) return;
  const int J = d.J, order = order_code(d.order);
  const int FP = rf_pass_frames(J, d.max_frames);
  const int RF = rt_raw_floats(J);
  const int* parents = (const int*)state;
  const int* place = parents + 2 * J;
  char* row_state = state + rf_row_offset(J, max_half, rec.row);
  FrPlace* pl = (FrPlace*)row_state;
  float* prev = (float*)(pl + 1);
  float* ring = (float*)(row_state + rf_row_ring_offset(J));
  const bool rebase = pl->rebase != 0;
  const long n1 = rec.n_in + rec.count;
  const long m0 = filtered ? rf_n_out(rec.n_in, rec.L, rec.M, rec.half) : rt_n_out(rec.n_in, rec.L, rec.M);
  const long outs = (filtered ? rf_emitted(n1, rec.L, rec.M, rec.half, rec.final) : rt_n_out(n1, rec.L, rec.M)) - m0;
  double* lq = rf_lds;
  double* lp = rf_lds + (size_t)FP * (J + 1) * 4;
  const long first = m0 == 0 ? 0L : -1L;
  if (filtered) {
    for (long f0 = 0; f0 < outs; f0 += FP) {
      const int n = (int)(outs - f0 < FP ? outs - f0 : FP);
      fr_pass(RfLoad{rec, pl, ring, m0 + f0, n1 - 1, J, max_half, RF, rebase}, J, order, d.what, parents, place, prev, lq, lp, f0, n, first, rec.local,
              rec.world, rec.bvh);
    }
  } else {
    // the unfiltered statement: its kept frame is the ring's slot of input frame n_in - 1
    const float* raw = ring + (size_t)rf_slot(rec.n_in - 1, max_half) * RF;
    for (long f0 = 0; f0 < outs; f0 += FP) {
      const int n = (int)(outs - f0 < FP ? outs - f0 : FP);
      fr_pass(RtLoad{rf_plain(rec), pl, raw, m0 + f0, J, rebase}, J, order, d.what, parents, place, prev, lq, lp, f0, n, first, rec.local, rec.world,
              rec.bvh);
    }
  }
  if (rec.count <= 0) return;
  // the call's frames enter the ring, raw (every pass ends behind a barrier: nothing reads the ring any more)
  for (long f = rf_first_kept(rec.count, max_half); f < rec.count; ++f) {
    float* slot = ring + (size_t)rf_slot(rec.n_in + f, max_half) * RF;
    const float* row = rec.pose + f * rec.pose_ld;
    for (int i = threadIdx.x; i < RF; i += FR_THREADS)
      slot[i] = i < 3 ? rec.rpos[f * rec.rpos_ld + i] : i < 7 ? rec.rrot[f * rec.rrot_ld + i - 3] : row[fr_pose_lpos(0) + i - 7];
  }
  if (threadIdx.x == 0) pl->started = 1;
}

}  // namespace

#include "frames_host.h"      // the host contract the three forms of the head share

namespace {

int rf_dims_ok(const ZeggsFramesDims* d, int max_half, const void* state, size_t state_bytes) {
  ZTRY(fh_shape_ok("refilter", d));
  ZCHECK(max_half >= 1 && max_half <= RF_MAX_HALF, "refilter: max_half %d (1..%d)", max_half, RF_MAX_HALF);
  return lh_block_ok("refilter", "state", state, state_bytes, (size_t)rf_state_bytes(d->rows, d->J, max_half), 8);
}

}  // namespace

extern "C" int zeggs_live_refilter_version(void) { return 1; }

extern "C" size_t zeggs_live_refilter_state_bytes(const ZeggsFramesDims* d, int max_half) {
  if (rf_dims_ok(d, max_half, nullptr, (size_t)-1) != 0) return 0;
  return (size_t)rf_state_bytes(d->rows, d->J, max_half);
}

extern "C" int zeggs_live_refilter_prepare(const ZeggsFramesDims* d, int max_half, const int* parents, const int* seq, void* state,
                                           size_t state_bytes, void* stream) {
  ZTRY(rf_dims_ok(d, max_half, state, state_bytes));
  return fh_prepare("refilter", d, parents, seq, state, stream);
}

extern "C" int zeggs_live_refilter_reset(const ZeggsFramesDims* d, int max_half, void* state, size_t state_bytes, int row, const float* ref_pos,
                                         const float* ref_rot, const double* start_pos, const double* start_rot, int rebase, void* stream) {
  ZTRY(rf_dims_ok(d, max_half, state, state_bytes));
  return fh_reset("refilter", "live_refilter_reset", d, state, rf_row_offset(d->J, max_half, row), row, ref_pos, ref_rot, start_pos, start_rot,
                  rebase, stream);
}

extern "C" int zeggs_live_frames_refiltered(const ZeggsFramesDims* d, int max_half, const ZeggsRefilterRow* rows, const ZeggsRefilterRow* rows_dev,
                                            int R, void* state, size_t state_bytes, void* stream) {
  const char* who = "refilter";
  ZTRY(rf_dims_ok(d, max_half, state, state_bytes));
  ZTRY(lh_count_ok(who, R, d->rows));
  if (R == 0) return 0;
  ZCHECK(rows != nullptr, "%s: NULL records", who);
  bool seen[ZEGGS_LIVE_MAX_ROWS] = {};
  bool work = false;
  const int J = d->J;
  for (int i = 0; i < R; ++i) {
    const ZeggsRefilterRow& w = rows[i];
    ZTRY(fh_row_ok(who, i, w, d, seen));
    ZTRY(fh_ratio_ok(who, i, w));
    ZCHECK(w.half >= 0, "%s: record %d: negative half %d", who, i, w.half);
    const bool filtered = w.half > 0;
    long want;
    if (filtered) {
      ZCHECK(rf_ratio_refused(w.L, w.M) == 0, "%s: record %d: a filtered row at ratio %d / %d (L <= %d and M <= %d L)", who, i, w.L, w.M, RF_MAX_L,
             RF_MAX_DOWN);
      ZCHECK(rf_half_fits(w.L, w.M, w.half), "%s: record %d: half %d is no ceil(Z max(L, M) / L) for Z = 1 .. %d at %d / %d", who, i, w.half,
             RF_MAX_Z, w.L, w.M);
      ZCHECK(w.half <= max_half, "%s: record %d: half %d, max_half is %d", who, i, w.half, max_half);
      ZCHECK(w.table != nullptr && (uintptr_t)w.table % 8 == 0, "%s: record %d: NULL or misaligned table", who, i);
      ZCHECK(w.final == 0 || w.final == 1, "%s: record %d: final = %d (0 or 1)", who, i, w.final);
      want = rf_emitted(w.n_in + w.count, w.L, w.M, w.half, w.final) - rf_n_out(w.n_in, w.L, w.M, w.half);
      ZCHECK(w.outputs == want, "%s: record %d: %ld outputs disagree with %s(%ld) - nf(%ld) = %ld at %d / %d, half %d", who, i, w.outputs,
             w.final ? "n_out" : "nf", w.n_in + w.count, w.n_in, want, w.L, w.M, w.half);
    } else {
      want = rt_n_out(w.n_in + w.count, w.L, w.M) - rt_n_out(w.n_in, w.L, w.M);
      ZCHECK(w.outputs == want, "%s: record %d: %ld outputs disagree with n_out(%ld) - n_out(%ld) = %ld at %d / %d", who, i, w.outputs,
             w.n_in + w.count, w.n_in, want, w.L, w.M);
    }
    if (w.count > 0) ZTRY(lh_sources_ok(who, i, w, fr_pose_floats_read(J)));
    if (w.count == 0 && !(filtered && w.final)) continue;
    if (w.outputs > 0) ZTRY(fh_dests_ok(who, i, w, d->what));
    if (w.count > 0 || w.outputs > 0) work = true;
  }
  if (!work) return 0;
  ZTRY(lh_dev_ok(who, "rows_dev", rows_dev, R, 8));
  hipLaunchKernelGGL(live_refilter_k, dim3((unsigned)R), dim3(FR_THREADS), (size_t)rf_lds_bytes(J, d->max_frames), (hipStream_t)stream, *d, max_half,
                     rows_dev, rows[0], (char*)state);
  ZLAUNCH_CHECK("live_refilter");
  return 0;
}
