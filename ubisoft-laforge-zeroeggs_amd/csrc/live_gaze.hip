// Live serving: a gaze target per row that can move while speech goes on (include/zeggs_hip_gaze.h; the arithmetic is
// gaze_math.h, the definition DESIGN.md 3.7).
//
// The state is one GazeRow of 64 bytes per row.  Three small kernels, each ONE launch whatever the number of rows, one workgroup
// per record -- at a few thousand values a call the launch is the cost, not the arithmetic:
//   live_gaze_set_k    one lane per record: the row's old schedule at frame k - 1 becomes the new start, a root-space target is
//                      resolved with the row's root state, read here on the device, and the new schedule is stored;
//   live_condition_k   the conditioning rows of one decoder call: lanes over the frames write the gaze rows (float64 from the
//                      float32 schedule, rounded once at the store), then lanes over frames x channels write the style rows
//                      lerp(sty_old, sty_new, w) -- what the host otherwise does with a weight upload and a torch.lerp;
//   live_gaze_reset_k  start = end = the first pose's gaze.
// Plain loads and stores, no LDS, nothing indexed in registers.
#include "../../include/zeggs_hip_gaze.h"
#include "common.h"
#include "gaze_math.h"

#include <math.h>

namespace {

constexpr int GAZE_THREADS = 256;

static_assert(GAZE_ROW_BYTES == ZEGGS_GAZE_ROW_BYTES && GAZE_WORLD == ZEGGS_GAZE_WORLD && GAZE_ROOT == ZEGGS_GAZE_ROOT &&
                  GAZE_LINE == ZEGGS_GAZE_LINE && GAZE_ARC == ZEGGS_GAZE_ARC && GAZE_LINEAR == ZEGGS_GAZE_LINEAR && GAZE_SMOOTH == ZEGGS_GAZE_SMOOTH,
              "gaze_math.h and the ninth header disagree");

__global__ void live_gaze_reset_k(GazeRow* g, const float* __restrict__ gaze0) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (int i = 0; i < 3; ++i) {
    g->start[i] = gaze0[i];
    g->end[i] = gaze0[i];
    g->pivot[i] = 0.f;
  }
  g->path = GAZE_LINE; g->ease = GAZE_LINEAR; g->pad = 0;
  g->k = 0; g->fade = 0;
}

__global__ __launch_bounds__(64) void live_gaze_set_k(const ZeggsGazeSet* __restrict__ recs, ZeggsGazeSet one, GazeRow* state,
                                                      const float* __restrict__ rpos, long rpos_ld, const float* __restrict__ rrot, long rrot_ld) {
  if (threadIdx.x != 0) return;
  const ZeggsGazeSet rec = recs ? recs[blockIdx.x] : one;
  float p[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f};
  if (rec.space == GAZE_ROOT) {
    const float* rp = rpos + (long)rec.row * rpos_ld;
    const float* rq = rrot + (long)rec.row * rrot_ld;
    p[0] = rp[0]; p[1] = rp[1]; p[2] = rp[2];
    q[0] = rq[0]; q[1] = rq[1]; q[2] = rq[2]; q[3] = rq[3];
  }
  GazeRow g = state[rec.row];
  gaze_apply(&g, rec.target, rec.pivot, rec.has_pivot, rec.space, rec.path, rec.ease, rec.k, rec.fade, p, q);
  state[rec.row] = g;
}

__global__ __launch_bounds__(GAZE_THREADS) void live_condition_k(const ZeggsGazeCond* __restrict__ recs, ZeggsGazeCond one,
                                                                  const GazeRow* __restrict__ state, const float* __restrict__ sty_old,
                                                                  const float* __restrict__ sty_new, float* __restrict__ gaze_out,
                                                                  float* __restrict__ style_out, long stride, int ST) {
  const ZeggsGazeCond rec = recs ? recs[blockIdx.x] : one;
  const int tid = threadIdx.x, n = rec.n;
  const GazeRow g = state[rec.row];
  float* go = gaze_out + (long)rec.out_row * stride * 3;
  for (int i = tid; i < n; i += GAZE_THREADS) {
    double p[3];
    gaze_eval(g, rec.k0 + i, p);
    go[3 * i + 0] = (float)p[0];
    go[3 * i + 1] = (float)p[1];
    go[3 * i + 2] = (float)p[2];
  }
  const float* a = sty_old + (long)rec.row * ST;
  const float* b = sty_new + (long)rec.row * ST;
  float* so = style_out + (long)rec.out_row * stride * ST;
  const int total = n * ST;
  for (int e = tid; e < total; e += GAZE_THREADS) {
    const int i = e / ST, c = e - i * ST;
    so[e] = gaze_style_lerp(a[c], b[c], gaze_style_weight(rec.k0 + i, rec.k_style, rec.fade_style));
  }
}

}  // namespace

#include "live_host.h"      // the host contract every stage of live serving keeps

namespace {

int gaze_dims_ok(const ZeggsGazeDims* d, const void* state, size_t state_bytes) {
  ZTRY(lh_dims_ok("live gaze", d));
  ZCHECK(d->ST >= 1 && d->ST <= (1 << 16), "live gaze: style rows of %d floats", d->ST);
  return lh_block_ok("live gaze", "state", state, state_bytes, (size_t)d->rows * GAZE_ROW_BYTES, 8);
}

bool finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

}  // namespace

extern "C" int zeggs_live_gaze_version(void) { return 1; }

extern "C" size_t zeggs_live_gaze_state_bytes(const ZeggsGazeDims* d) {
  if (gaze_dims_ok(d, nullptr, (size_t)-1) != 0) return 0;
  return (size_t)d->rows * GAZE_ROW_BYTES;
}

extern "C" int zeggs_live_gaze_reset(const ZeggsGazeDims* d, void* state, size_t state_bytes, int row, const float* gaze0, void* stream) {
  ZTRY(gaze_dims_ok(d, state, state_bytes));
  ZTRY(lh_row_ok("live gaze", "reset", row, d->rows));
  ZCHECK(gaze0 != nullptr && (uintptr_t)gaze0 % 4 == 0, "live gaze reset: NULL or misaligned gaze");
  hipLaunchKernelGGL(live_gaze_reset_k, dim3(1), dim3(64), 0, (hipStream_t)stream, (GazeRow*)state + row, gaze0);
  ZLAUNCH_CHECK("live_gaze_reset");
  return 0;
}

extern "C" int zeggs_live_gaze_set(const ZeggsGazeDims* d, const ZeggsGazeSet* recs, const ZeggsGazeSet* recs_dev, int R, const float* rpos,
                                   long rpos_ld, const float* rrot, long rrot_ld, void* state, size_t state_bytes, void* stream) {
  const char* who = "live gaze set";
  ZTRY(gaze_dims_ok(d, state, state_bytes));
  ZTRY(lh_count_ok(who, R, d->rows));
  if (R == 0) return 0;
  ZCHECK(recs != nullptr, "live gaze set: NULL records");
  bool seen[ZEGGS_LIVE_MAX_ROWS] = {};
  bool root = false;
  for (int i = 0; i < R; ++i) {
    const ZeggsGazeSet& w = recs[i];
    ZTRY(lh_once_ok(who, i, w.row, d->rows, seen));
    ZCHECK(w.k >= 1, "live gaze set: record %d: frame %ld (>= 1)", i, w.k);
    ZCHECK(w.fade >= 0, "live gaze set: record %d: negative fade %ld", i, w.fade);
    ZCHECK(w.space == ZEGGS_GAZE_WORLD || w.space == ZEGGS_GAZE_ROOT, "live gaze set: record %d: space %d", i, w.space);
    ZCHECK(w.path == ZEGGS_GAZE_LINE || w.path == ZEGGS_GAZE_ARC, "live gaze set: record %d: path %d", i, w.path);
    ZCHECK(w.ease == ZEGGS_GAZE_LINEAR || w.ease == ZEGGS_GAZE_SMOOTH, "live gaze set: record %d: ease %d", i, w.ease);
    ZCHECK(finite3(w.target), "live gaze set: record %d: the target is not finite", i);
    ZCHECK(!w.has_pivot || finite3(w.pivot), "live gaze set: record %d: the pivot is not finite", i);
    ZCHECK(w.has_pivot || w.space == ZEGGS_GAZE_ROOT || w.path != ZEGGS_GAZE_ARC, "live gaze set: record %d: an arc in world space needs a pivot", i);
    root = root || w.space == ZEGGS_GAZE_ROOT;
  }
  if (root) {
    ZCHECK(rpos != nullptr && rrot != nullptr && (uintptr_t)rpos % 4 == 0 && (uintptr_t)rrot % 4 == 0,
           "live gaze set: root space needs the rows' root state (NULL or misaligned rpos / rrot)");
    ZCHECK(rpos_ld >= 3 && rrot_ld >= 4, "live gaze set: root strides %ld / %ld (>= 3 / >= 4)", rpos_ld, rrot_ld);
  }
  ZTRY(lh_dev_ok(who, "recs_dev", recs_dev, R));
  hipLaunchKernelGGL(live_gaze_set_k, dim3((unsigned)R), dim3(64), 0, (hipStream_t)stream, recs_dev, recs[0], (GazeRow*)state, rpos, rpos_ld,
                     rrot, rrot_ld);
  ZLAUNCH_CHECK("live_gaze_set");
  return 0;
}

extern "C" int zeggs_live_condition(const ZeggsGazeDims* d, const ZeggsGazeCond* recs, const ZeggsGazeCond* recs_dev, int R, const void* state,
                                    size_t state_bytes, const float* sty_old, const float* sty_new, float* gaze_out, float* style_out,
                                    int out_rows, long stride, void* stream) {
  ZTRY(gaze_dims_ok(d, state, state_bytes));
  ZCHECK(out_rows >= 1 && out_rows <= ZEGGS_LIVE_MAX_ROWS, "live condition: %d output slices (1..%d)", out_rows, ZEGGS_LIVE_MAX_ROWS);
  ZCHECK(stride >= 1 && stride <= (1 << 20), "live condition: a stride of %ld frames", stride);
  ZCHECK(R >= 0 && R <= d->rows && R <= out_rows, "live condition: %d records for %d rows and %d output slices", R, d->rows, out_rows);
  if (R == 0) return 0;
  ZCHECK(recs != nullptr, "live condition: NULL records");
  bool seen[ZEGGS_LIVE_MAX_ROWS] = {}, taken[ZEGGS_LIVE_MAX_ROWS] = {};
  for (int i = 0; i < R; ++i) {
    const ZeggsGazeCond& w = recs[i];
    ZTRY(lh_once_ok("live condition", i, w.row, d->rows, seen));
    ZCHECK(w.out_row >= 0 && w.out_row < out_rows, "live condition: record %d: output slice %d of %d", i, w.out_row, out_rows);
    ZCHECK(!taken[w.out_row], "live condition: record %d: output slice %d twice in one call", i, w.out_row);
    taken[w.out_row] = true;
    ZCHECK(w.n >= 1 && w.n <= stride, "live condition: record %d: %d frames (1..%ld)", i, w.n, stride);
    ZCHECK(w.k0 >= 0, "live condition: record %d: negative frame %ld", i, w.k0);
    ZCHECK(w.fade_style >= 0, "live condition: record %d: negative style fade %ld", i, w.fade_style);
  }
  ZCHECK(sty_old != nullptr && sty_new != nullptr && gaze_out != nullptr && style_out != nullptr, "live condition: NULL tensor");
  ZCHECK(((uintptr_t)sty_old | (uintptr_t)sty_new | (uintptr_t)gaze_out | (uintptr_t)style_out) % 4 == 0, "live condition: misaligned tensor");
  ZTRY(lh_dev_ok("live condition", "recs_dev", recs_dev, R));
  hipLaunchKernelGGL(live_condition_k, dim3((unsigned)R), dim3(GAZE_THREADS), 0, (hipStream_t)stream, recs_dev, recs[0], (const GazeRow*)state,
                     sty_old, sty_new, gaze_out, style_out, stride, d->ST);
  ZLAUNCH_CHECK("live_condition");
  return 0;
}

extern "C" int zeggs_live_gaze_read(const ZeggsGazeDims* d, const void* state, size_t state_bytes, int row, long frame, double* out, void* stream) {
  ZTRY(gaze_dims_ok(d, state, state_bytes));
  ZTRY(lh_row_ok("live gaze", "read", row, d->rows));
  ZCHECK(out != nullptr, "live gaze read: NULL output");
  GazeRow g;
  hipError_t e = hipMemcpyAsync(&g, (const GazeRow*)state + row, sizeof(g), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  ZCHECK(e == hipSuccess, "live gaze read: %s", hipGetErrorString(e));
  double p[3];
  gaze_eval(g, frame, p);
  for (int i = 0; i < 3; ++i) {
    out[ZEGGS_GAZE_READ_TARGET + i] = (double)(float)p[i];
    out[ZEGGS_GAZE_READ_START + i] = (double)g.start[i];
    out[ZEGGS_GAZE_READ_END + i] = (double)g.end[i];
    out[ZEGGS_GAZE_READ_PIVOT + i] = (double)g.pivot[i];
  }
  out[ZEGGS_GAZE_READ_K] = (double)g.k;
  out[ZEGGS_GAZE_READ_FADE] = (double)g.fade;
  out[ZEGGS_GAZE_READ_PATH] = (double)g.path;
  out[ZEGGS_GAZE_READ_EASE] = (double)g.ease;
  return 0;
}

extern "C" int zeggs_live_gaze_spans(const ZeggsGazeDims* d, int row, ZeggsSnapSpan* spans, int max_spans) {
  if (zeggs_live_gaze_state_bytes(d) == 0) return -1;
  const size_t o = (size_t)row * GAZE_ROW_BYTES, b = GAZE_ROW_BYTES;
  return lh_spans_out("live gaze spans", row >= 0 && row < d->rows ? 1 : -1, row, d->rows, max_spans, &o, &b, spans);
}
