// Live serving: a band-limited rate converter per row, in front of the loudness stage and the window
// (include/zeggs_hip_resample.h; the index rules are resample_math.h, the definition DESIGN.md 3.7).
//
// One workgroup of 1024 threads per record, ONE launch per push whatever the number of rows.  A row's outputs are walked in
// TILES of up to 1024 (rs_tile_outputs: fewer where the inputs they touch would not fit the staging area): all threads stage
// the tile's input span in LDS as float32 -- an input sample older than this call comes from the row's ring (sample k in slot
// k % ceil(2 W)), a newer one from the call's source, converted on load; beyond the end of a signal (a final call) and before
// its start it is 0 -- then thread t computes output t of the tile: rs_output(), the taps inside the support in ascending
// input index, one float64 accumulator of explicit fma(), rounded to float32 once.  The staging decides only WHERE a sample is
// read from, so an output is the same bits wherever it falls in a tile, in a call and in whichever call.  The inner loop reads
// LDS and the coefficient row (the vector L1 holds the few rows a tile uses) at addresses that do not depend on the
// accumulator: what a thread waits for is the chain of dependent float64 fma().
// The hazard the loudness kernel does not have: this call's outputs read the ring this call must also rewrite.  The row has
// one workgroup, which finishes ALL its tiles (each ends at a barrier) and only then moves the last ceil(2 W) inputs into the
// ring -- no output reads a half-updated history.
#include "../../include/zeggs_hip_resample.h"
#include "common.h"
#include "resample_math.h"
#include "snapshot_math.h"

namespace {

static_assert(RS_THREADS == 1024 && RS_SPAN * sizeof(float) <= 48 * 1024, "one output per thread and tile; 48 KB of LDS");

__device__ __forceinline__ float rs_load(const void* src, int format, long i) {
  return format == ZEGGS_RS_S16 ? (float)((const short*)src)[i] * (1.0f / 32768.0f) : ((const float*)src)[i];
}

// output m of a row: xs[k - k_lo] is the row's input sample k as float32 (0 outside the signal)
__device__ __forceinline__ float rs_output(long m, int L, int M, long WL, const double* __restrict__ table, const float* xs, long k_lo) {
  long q;
  int ph, j0, j1;
  rs_position(m, L, M, &q, &ph);
  rs_tap_range(ph, L, WL, &j0, &j1);
  const int H = rs_half(WL, L);
  const double* c = table + (size_t)ph * (size_t)(2 * H + 1);
  const int off = (int)(q - H - k_lo);      // tap j reads input q - H + j, staged at xs[off + j] (>= 0 from j0 on)
  double acc = 0.0;
#pragma unroll 8
  for (int j = j0; j <= j1; ++j) acc = fma((double)xs[off + j], c[j], acc);
  return (float)acc;
}

// outputs m0 .. m0 + cnt - 1 (cnt <= rs_tile_outputs) -> dst[0 .. cnt): the span they touch into LDS, then one output per thread.
// Every thread of the workgroup calls it (two barriers); x_at(k) is the row's input sample k as float32
template <class X>
__device__ __forceinline__ void rs_tile(float* xs, long m0, int cnt, float* dst, int L, int M, long WL, const double* __restrict__ table, X x_at) {
  const long k_lo = rs_first_tap(m0, L, M, WL);
  long span = rs_last_tap(m0 + cnt - 1, L, M, WL) - k_lo + 1;
  if (span > RS_SPAN) span = RS_SPAN;      // (never: rs_tile_outputs, checked by tests/host/resample_math_check.cpp)
  for (int i = threadIdx.x; i < (int)span; i += RS_THREADS) xs[i] = x_at(k_lo + i);
  __syncthreads();
  if ((int)threadIdx.x < cnt) dst[threadIdx.x] = rs_output(m0 + threadIdx.x, L, M, WL, table, xs, k_lo);
  __syncthreads();                          // (the next tile rewrites xs)
}

__global__ __launch_bounds__(RS_THREADS) void live_resample_k(const ZeggsResampleRow* __restrict__ recs, ZeggsResampleRow one, float* state,
                                                               int history) {
  __shared__ float xs[RS_SPAN];
  const ZeggsResampleRow rec = recs ? recs[blockIdx.x] : one;
  if (rec.count <= 0 && rec.outputs <= 0) return;
  const int tid = threadIdx.x, L = rec.L, M = rec.M, fmt = rec.format;
  const long WL = rec.WL, n_in = rec.n_in, count = rec.count;
  const int HL = rs_history(WL, L);
  float* hist = state + (size_t)rec.row * (size_t)history;
  const void* src = rec.src;
  auto x_at = [=](long k) -> float {
    if (k < 0) return 0.f;
    if (k < n_in) return HL > 0 ? hist[rs_slot(k, HL)] : 0.f;
    const long i = k - n_in;
    return i < count ? rs_load(src, fmt, i) : 0.f;
  };
  const int tile = rs_tile_outputs(L, M, WL);
  for (long i = 0; i < rec.outputs; i += tile)
    rs_tile(xs, rec.n_out + i, (int)(rec.outputs - i < tile ? rec.outputs - i : tile), rec.dst + i, L, M, WL, rec.table, x_at);
  if (HL <= 0 || count <= 0) return;      // (uniform over the workgroup)
  __syncthreads();                         // every output of the row is done: now its history may move
  const long n1 = n_in + count;
  const long lo = n1 - HL > n_in ? n1 - HL : n_in;
  for (long k = lo + tid; k < n1; k += RS_THREADS) hist[rs_slot(k, HL)] = rs_load(src, fmt, k - n_in);
}

__global__ __launch_bounds__(RS_THREADS) void resample_whole_k(const double* __restrict__ table, int L, int M, long WL, const void* src, int fmt,
                                                                long n_in, float* __restrict__ dst, long n_out) {
  __shared__ float xs[RS_SPAN];
  const int tile = rs_tile_outputs(L, M, WL);
  const long m0 = (long)blockIdx.x * tile;      // one tile per workgroup
  rs_tile(xs, m0, (int)(n_out - m0 < tile ? n_out - m0 : tile), dst + m0, L, M, WL, table,
          [=](long k) -> float { return k < 0 || k >= n_in ? 0.f : rs_load(src, fmt, k); });
}

}  // namespace

#include "live_host.h"      // the host contract every stage of live serving keeps

namespace {

int rs_dims_ok(const ZeggsResampleDims* d, const void* state, size_t state_bytes) {
  ZTRY(lh_dims_ok("resample", d));
  ZCHECK(d->history >= 1 && d->history <= (1 << 20), "resample: a history of %d samples", d->history);
  return lh_block_ok("resample", "state", state, state_bytes, (size_t)d->rows * d->history * sizeof(float), 4);
}

// L, M, WL of a record or of the whole-signal call: a supported ratio and a support that belongs to it
int rs_filter_ok(const char* who, int L, int M, long WL) {
  ZCHECK(L >= 1 && L <= RS_MAX_L && M >= 1 && (long)M <= (long)RS_MAX_DECIMATION * L && rs_gcd(L, M) == 1,
         "%s: ratio L / M = %d / %d (coprime, L <= %d, M / L <= %d)", who, L, M, RS_MAX_L, RS_MAX_DECIMATION);
  const long big = L > M ? L : M;
  ZCHECK(WL >= 0 && WL % big == 0 && WL / big <= RS_MAX_ZERO_CROSSINGS, "%s: support WL = %ld is no multiple (1 .. %d) of max(L, M) = %ld", who,
         WL, RS_MAX_ZERO_CROSSINGS, big);
  ZCHECK(WL > 0 || (L == 1 && M == 1), "%s: pass-through (WL = 0) needs L = M = 1, not %d / %d", who, L, M);
  return 0;
}

int rs_push(const char* who, const ZeggsResampleDims* d, const ZeggsResampleRow* rows, const ZeggsResampleRow* rows_dev, int R, bool final,
            void* state, size_t state_bytes, void* stream) {
  ZTRY(rs_dims_ok(d, state, state_bytes));
  ZTRY(lh_count_ok(who, R, d->rows));
  if (R == 0) return 0;
  ZCHECK(rows != nullptr, "%s: NULL records", who);
  bool seen[ZEGGS_LIVE_MAX_ROWS] = {};
  bool work = false;
  char name[96];
  for (int i = 0; i < R; ++i) {
    const ZeggsResampleRow& w = rows[i];
    ZTRY(lh_once_ok(who, i, w.row, d->rows, seen));
    ZCHECK(w.count >= 0, "%s: record %d: negative count %ld", who, i, w.count);
    ZCHECK(w.format == ZEGGS_RS_F32 || w.format == ZEGGS_RS_S16, "%s: record %d: format %d", who, i, w.format);
    snprintf(name, sizeof(name), "%s: record %d", who, i);
    ZTRY(rs_filter_ok(name, w.L, w.M, w.WL));
    ZCHECK(rs_history(w.WL, w.L) <= d->history, "%s: record %d: a history of %d samples, the state holds %d", who, i,
           rs_history(w.WL, w.L), d->history);
    ZCHECK(w.n_in >= 0 && w.n_in <= (1L << 46) && w.count <= (1L << 40), "%s: record %d: input counter %ld, count %ld", who, i, w.n_in,
           w.count);
    ZCHECK(w.n_out == rs_ready(w.n_in, w.L, w.M, w.WL), "%s: record %d: %ld outputs before the call disagree with ready(%ld) = %ld",
           who, i, w.n_out, w.n_in, rs_ready(w.n_in, w.L, w.M, w.WL));
    const bool fin = final || w.final != 0;
    const long n1 = w.n_in + w.count, want = (fin ? rs_total(n1, w.L, w.M) : rs_ready(n1, w.L, w.M, w.WL)) - w.n_out;
    ZCHECK(w.outputs == want, "%s: record %d: %ld outputs disagree with %s(%ld) - %ld = %ld", who, i, w.outputs, fin ? "total" : "ready",
           n1, w.n_out, want);
    ZCHECK(w.table != nullptr && (uintptr_t)w.table % 8 == 0, "%s: record %d: NULL or misaligned table", who, i);
    const uintptr_t align = w.format == ZEGGS_RS_S16 ? 2 : 4;
    ZCHECK(w.count == 0 || (w.src != nullptr && (uintptr_t)w.src % align == 0), "%s: record %d: NULL or misaligned source", who, i);
    ZCHECK(w.outputs == 0 || (w.dst != nullptr && (uintptr_t)w.dst % 4 == 0), "%s: record %d: NULL or misaligned destination", who, i);
    work = work || w.count > 0 || w.outputs > 0;
  }
  if (!work) return 0;
  ZTRY(lh_dev_ok(who, "rows_dev", rows_dev, R));
  ZeggsResampleRow one = rows[0];
  if (final) one.final = 1;
  hipLaunchKernelGGL(live_resample_k, dim3((unsigned)R), dim3(RS_THREADS), 0, (hipStream_t)stream, rows_dev, one, (float*)state, d->history);
  ZLAUNCH_CHECK("live_resample");
  return 0;
}

}  // namespace

extern "C" int zeggs_live_resample_version(void) { return 1; }

extern "C" size_t zeggs_resample_state_bytes(const ZeggsResampleDims* d) {
  if (rs_dims_ok(d, nullptr, (size_t)-1) != 0) return 0;
  return (size_t)d->rows * rs_state_row_bytes(d->history);      // (a row's place is stated in snapshot_math.h)
}

extern "C" int zeggs_resample_reset(const ZeggsResampleDims* d, void* state, size_t state_bytes, int row, void* stream) {
  ZTRY(rs_dims_ok(d, state, state_bytes));
  ZTRY(lh_row_ok("resample", "reset", row, d->rows));
  const size_t rb = rs_state_row_bytes(d->history);
  hipError_t e = hipMemsetAsync((char*)state + (size_t)row * rb, 0, rb, (hipStream_t)stream);
  ZCHECK(e == hipSuccess, "resample reset: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int zeggs_resample_push(const ZeggsResampleDims* d, const ZeggsResampleRow* rows, const ZeggsResampleRow* rows_dev, int R, void* state,
                                   size_t state_bytes, void* stream) {
  return rs_push("resample push", d, rows, rows_dev, R, false, state, state_bytes, stream);
}

extern "C" int zeggs_resample_flush(const ZeggsResampleDims* d, const ZeggsResampleRow* row, void* state, size_t state_bytes, void* stream) {
  return rs_push("resample flush", d, row, nullptr, 1, true, state, state_bytes, stream);
}

extern "C" int zeggs_resample_whole(const double* table, int L, int M, long WL, const void* src, int format, long n_in, float* dst, long n_out,
                                    void* stream) {
  ZTRY(rs_filter_ok("resample whole", L, M, WL));
  ZCHECK(format == ZEGGS_RS_F32 || format == ZEGGS_RS_S16, "resample whole: format %d", format);
  ZCHECK(n_in >= 0 && n_in <= (1L << 40), "resample whole: %ld input samples", n_in);
  ZCHECK(n_out == rs_total(n_in, L, M), "resample whole: %ld outputs, %ld inputs at %d / %d give %ld", n_out, n_in, L, M, rs_total(n_in, L, M));
  if (n_out == 0) return 0;
  ZCHECK(table != nullptr && (uintptr_t)table % 8 == 0, "resample whole: NULL or misaligned table");
  ZCHECK(src != nullptr && (uintptr_t)src % (format == ZEGGS_RS_S16 ? 2 : 4) == 0, "resample whole: NULL or misaligned source");
  ZCHECK(dst != nullptr && (uintptr_t)dst % 4 == 0, "resample whole: NULL or misaligned destination");
  const long tile = rs_tile_outputs(L, M, WL), tiles = (n_out + tile - 1) / tile;
  ZCHECK(tiles < (1L << 31), "resample whole: %ld outputs are more than one launch takes", n_out);
  hipLaunchKernelGGL(resample_whole_k, dim3((unsigned)tiles), dim3(RS_THREADS), 0, (hipStream_t)stream, table,
                     L, M, WL, src, format, n_in, dst, n_out);
  ZLAUNCH_CHECK("resample_whole");
  return 0;
}
