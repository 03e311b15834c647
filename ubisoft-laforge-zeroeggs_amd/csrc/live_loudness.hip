// Live serving: a running BS.1770 gated loudness estimate per row and the gain it asks for, applied as the samples enter the row's
// device window (include/zeggs_hip_loudness.h; the offline form over a whole signal is loudness.hip).
//
// One workgroup of 256 threads per row, ONE launch per push whatever the number of rows.  A row's chunk is walked in RUNS that end
// where the next gating block completes (loud_math.h: loud_run_end), so a gain change lands exactly on sample index hi_j wherever
// that falls inside the chunk, and the ring of filtered samples holds exactly block j when its energy is taken:
//   per run   tiles of LOUD_TILE samples: all threads load the tile and write it to the window times the current gain; thread 0
//             runs the two K-weighting biquads over it from the carried states (the recurrence is strictly sequential: a
//             chunk-parallel scan would make the states depend on the cut; the two stages are software-pipelined one sample
//             apart, which changes no operation of either); all threads move the filtered tile into the row's ring;
//   per block its energy from the ring (256 strided partial sums, then the tree: the order of block_energy_k), its level, the
//             two gates over the ring of block energies (same shape of sum), and -- unless held -- the new gain.
// Every multiply-add of the filters and the energy is an explicit fma(), so no operation depends on what the compiler contracts
// in one place and not in another: the state after n samples is a function of the n samples alone, bitwise.
#include "../../include/zeggs_hip_loudness.h"
#include "common.h"
#include "loud_math.h"
#include "snapshot_math.h"

#include <atomic>

namespace {

constexpr int LOUD_TILE = 2048;

struct LoudHead {            // 128 bytes in front of a row's rings
  double s[4];               // filter states: stage 1 (s1, s2), stage 2
  long n, blocks;            // samples received / gating blocks completed
  double lufs;               // the last estimate (NaN: none yet)
  float gain;
  int hold, gated, kept;     // hold flag / blocks past the relative gate at the last block / the last block left the gain alone
  double pad[7];
};
static_assert(sizeof(LoudHead) == LOUD_HEAD_BYTES, "LoudHead");

// (the layout of a row is stated in snapshot_math.h, which also reports it as the spans of a snapshot)
__host__ __device__ inline size_t loud_row_bytes(const ZeggsLoudDims& d) { return loud_state_row_bytes(d.fs, d.ring_blocks); }

struct Biquad { double b0, b1, b2, a1, a2; };
// one sample of direct form II transposed (scipy.signal.lfilter): y = b0 x + s1; s1 = b1 x - a1 y + s2; s2 = b2 x - a2 y
__device__ __forceinline__ double biquad_step(const Biquad& q, double x, double& s1, double& s2) {
  const double y = fma(q.b0, x, s1);
  s1 = fma(-q.a1, y, fma(q.b1, x, s2));
  s2 = fma(-q.a2, y, q.b2 * x);
  return y;
}

__global__ __launch_bounds__(LOUD_THREADS) void live_loudness_k(ZeggsLoudDims d, const ZeggsLoudRow* __restrict__ recs, ZeggsLoudRow one,
                                                                 char* state, size_t row_bytes) {
  __shared__ float xs[LOUD_TILE];
  __shared__ double ys[LOUD_TILE];
  __shared__ double sm[2 * LOUD_THREADS];
  const ZeggsLoudRow rec = recs ? recs[blockIdx.x] : one;
  const long m = rec.count;
  if (m <= 0) return;
  const int tid = threadIdx.x, fs = d.fs, NB = d.ring_blocks;
  LoudHead* head = (LoudHead*)(state + (size_t)rec.row * row_bytes);
  const long len = loud_block_len(fs);
  double* yr = (double*)(head + 1);
  double* zr = yr + len;
  double* lr = zr + NB;
  const long n0 = head->n, n_end = n0 + m;
  long j = head->blocks;
  if (n0 < 0 || j < 0) return;      // a state that was never reset: nothing of it is used as an index
  float g = head->gain;
  double lufs = head->lufs;
  int gated = head->gated, kept = head->kept;
  const int hold = head->hold;
  const Biquad q1{d.coef[0], d.coef[1], d.coef[2], d.coef[3], d.coef[4]}, q2{d.coef[5], d.coef[6], d.coef[7], d.coef[8], d.coef[9]};
  double s1a = head->s[0], s2a = head->s[1], s1b = head->s[2], s2b = head->s[3];      // (thread 0's are the ones that count)
  const double inv_len = 1.0 / (0.4 * (double)fs);
  long n = n0;
  while (n < n_end) {
    long run_end = loud_run_end(j, n_end, fs);
    if (run_end < n) run_end = n;      // (only a block counter behind its sample count, i.e. a state that was never reset)
    for (long t0 = n; t0 < run_end; t0 += LOUD_TILE) {
      const int cnt = (int)(run_end - t0 < LOUD_TILE ? run_end - t0 : LOUD_TILE);
      const float* src = rec.src + (t0 - n0);
      float* dst = rec.dst + (t0 - n0);
      for (int i = tid; i < cnt; i += LOUD_THREADS) {
        const float x = src[i];
        xs[i] = x;
        dst[i] = x * g;
      }
      __syncthreads();
      if (tid == 0) {
        // stage 2 runs one sample behind stage 1: two independent dependency chains per iteration
        double u = (double)(float)biquad_step(q1, (double)xs[0], s1a, s2a);
#pragma unroll 4
        for (int i = 1; i < cnt; ++i) {
          const double u_next = (double)(float)biquad_step(q1, (double)xs[i], s1a, s2a);
          ys[i - 1] = (double)(float)biquad_step(q2, u, s1b, s2b);
          u = u_next;
        }
        ys[cnt - 1] = (double)(float)biquad_step(q2, u, s1b, s2b);
      }
      __syncthreads();
      for (int i = tid; i < cnt; i += LOUD_THREADS) yr[loud_yslot(t0 + i, len)] = ys[i];
      __syncthreads();      // (the ring is read below by other threads; xs / ys are rewritten by the next tile)
    }
    n = run_end;
    if (!loud_complete(j, n, fs)) break;      // the chunk ends inside block j
    // ---- block j is complete: energy, level, gates, gain
    sm[tid] = loud_energy_partial(yr, len, loud_first(j, fs, len), loud_hi(j, fs), tid);
    __syncthreads();
    for (int o = LOUD_THREADS / 2; o > 0; o >>= 1) {
      loud_tree_step(sm, tid, o);
      __syncthreads();
    }
    if (tid == 0) {
      const double z = sm[0] * inv_len;
      zr[loud_zslot(j, NB)] = z;
      lr[loud_zslot(j, NB)] = loud_level(z);
    }
    __syncthreads();
    double gamma_r = 0.0, tot = 0.0, num = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
      loud_gate_partial(zr, lr, NB, j, pass, gamma_r, tid, &sm[tid], &sm[LOUD_THREADS + tid]);
      __syncthreads();
      for (int o = LOUD_THREADS / 2; o > 0; o >>= 1) {
        loud_tree_step(sm, tid, o);
        loud_tree_step(sm + LOUD_THREADS, tid, o);
        __syncthreads();
      }
      tot = sm[0];
      num = sm[LOUD_THREADS];
      __syncthreads();
      if (pass == 0) gamma_r = loud_gamma_r(tot, num);
    }
    // (every thread holds the same sums: the decision needs no broadcast)
    gated = (int)num;
    double est;
    const bool fresh = loud_estimate(tot, num, d.warmup, &est);
    if (fresh) lufs = est;
    kept = !(fresh && !hold);
    if (!kept) g = loud_gain(lufs, d.target, d.gain_lo, d.gain_hi);
    ++j;
  }
  if (tid == 0) {
    head->s[0] = s1a; head->s[1] = s2a; head->s[2] = s1b; head->s[3] = s2b;
    head->n = n_end;
    head->blocks = j;
    head->lufs = lufs;
    head->gain = g;
    head->gated = gated;
    head->kept = kept;
  }
}

__global__ void loud_reset_k(char* row, size_t row_bytes, float gain0) {
  double* w = (double*)row;
  const size_t words = row_bytes / sizeof(double), head_words = sizeof(LoudHead) / sizeof(double);
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = head_words + gid; i < words; i += (size_t)gridDim.x * blockDim.x) w[i] = 0.0;      // the rings
  if (gid == 0) {            // the head, by ONE thread: zeroes first, then the two fields that are not zero
    LoudHead* h = (LoudHead*)row;
    for (size_t i = 0; i < head_words; ++i) w[i] = 0.0;
    h->lufs = __builtin_nan("");
    h->gain = gain0;
  }
}
__global__ void loud_hold_k(char* row, int on) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ((LoudHead*)row)->hold = on;
}

}  // namespace

#include "live_host.h"      // the host contract every stage of live serving keeps

namespace {

std::atomic<int> g_rate_ok{0};      // the last rate loud_rate_ok accepted (a push does not walk the block table again)

int loud_dims_ok(const ZeggsLoudDims* dp, const void* state, size_t state_bytes) {
  ZTRY(lh_dims_ok("live loudness", dp));
  const ZeggsLoudDims& d = *dp;
  ZCHECK(d.fs >= 1000 && d.fs <= 768000, "live loudness: sampling rate %d", d.fs);
  ZCHECK(d.ring_blocks >= 1 && d.ring_blocks <= (1 << 20), "live loudness: a ring of %d blocks", d.ring_blocks);
  ZCHECK(d.warmup >= 1, "live loudness: warmup %d (>= 1)", d.warmup);
  ZCHECK(d.gain_lo <= d.gain_hi, "live loudness: gain bounds %g > %g dB", d.gain_lo, d.gain_hi);      // (refuses NaN too)
  ZCHECK(d.target == d.target, "live loudness: target is NaN");
  if (g_rate_ok.load(std::memory_order_relaxed) != d.fs) {
    ZCHECK(loud_rate_ok(d.fs, 4096), "live loudness: the gating blocks of %d Hz do not have one length", d.fs);
    g_rate_ok.store(d.fs, std::memory_order_relaxed);
  }
  return lh_block_ok("live loudness", "state", state, state_bytes, (size_t)d.rows * loud_row_bytes(d), 8);
}

}  // namespace

extern "C" size_t zeggs_live_loudness_state_bytes(const ZeggsLoudDims* d) {
  if (loud_dims_ok(d, nullptr, (size_t)-1) != 0) return 0;
  return (size_t)d->rows * loud_row_bytes(*d);
}

extern "C" int zeggs_live_loudness_reset(const ZeggsLoudDims* d, void* state, size_t state_bytes, int row, float gain0, void* stream) {
  ZTRY(loud_dims_ok(d, state, state_bytes));
  ZTRY(lh_row_ok("live loudness", "reset", row, d->rows));
  ZCHECK(gain0 == gain0 && gain0 >= 0.f && gain0 < INFINITY, "live loudness reset: gain %g", (double)gain0);
  const size_t rb = loud_row_bytes(*d);
  hipLaunchKernelGGL(loud_reset_k, dim3(8), dim3(256), 0, (hipStream_t)stream, (char*)state + (size_t)row * rb, rb, gain0);
  ZLAUNCH_CHECK("live_loudness_reset");
  return 0;
}

extern "C" int zeggs_live_loudness_hold(const ZeggsLoudDims* d, void* state, size_t state_bytes, int row, int on, void* stream) {
  ZTRY(loud_dims_ok(d, state, state_bytes));
  ZTRY(lh_row_ok("live loudness", "hold", row, d->rows));
  hipLaunchKernelGGL(loud_hold_k, dim3(1), dim3(64), 0, (hipStream_t)stream, (char*)state + (size_t)row * loud_row_bytes(*d), on ? 1 : 0);
  ZLAUNCH_CHECK("live_loudness_hold");
  return 0;
}

extern "C" int zeggs_live_loudness_push(const ZeggsLoudDims* d, const ZeggsLoudRow* rows, const ZeggsLoudRow* rows_dev, int R, void* state,
                                        size_t state_bytes, void* stream) {
  const char* who = "live loudness push";
  ZTRY(loud_dims_ok(d, state, state_bytes));
  ZTRY(lh_count_ok(who, R, d->rows));
  if (R == 0) return 0;
  ZCHECK(rows != nullptr, "live loudness push: NULL records");
  bool seen[ZEGGS_LIVE_MAX_ROWS] = {};
  long total = 0;
  for (int i = 0; i < R; ++i) {
    const ZeggsLoudRow& w = rows[i];
    ZTRY(lh_once_ok(who, i, w.row, d->rows, seen));
    ZCHECK(w.count >= 0, "live loudness push: record %d: negative count %ld", i, w.count);
    if (w.count == 0) continue;
    ZCHECK(w.src != nullptr && w.dst != nullptr && (uintptr_t)w.src % 4 == 0 && (uintptr_t)w.dst % 4 == 0,
           "live loudness push: record %d: NULL or misaligned pointer", i);
    const uintptr_t s0 = (uintptr_t)w.src, s1 = (uintptr_t)(w.src + w.count), d0 = (uintptr_t)w.dst, d1 = (uintptr_t)(w.dst + w.count);
    ZCHECK(s1 <= d0 || d1 <= s0, "live loudness push: record %d: source and destination overlap", i);
    total += w.count;
  }
  if (total == 0) return 0;
  ZTRY(lh_dev_ok(who, "rows_dev", rows_dev, R));
  hipLaunchKernelGGL(live_loudness_k, dim3((unsigned)R), dim3(LOUD_THREADS), 0, (hipStream_t)stream, *d, rows_dev, rows[0], (char*)state,
                     loud_row_bytes(*d));
  ZLAUNCH_CHECK("live_loudness");
  return 0;
}

extern "C" int zeggs_live_loudness_read(const ZeggsLoudDims* d, const void* state, size_t state_bytes, int row, double* out, void* stream) {
  ZTRY(loud_dims_ok(d, state, state_bytes));
  ZTRY(lh_row_ok("live loudness", "read", row, d->rows));
  ZCHECK(out != nullptr, "live loudness read: NULL output");
  LoudHead h;
  hipError_t e = hipMemcpyAsync(&h, (const char*)state + (size_t)row * loud_row_bytes(*d), sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  ZCHECK(e == hipSuccess, "live loudness read: %s", hipGetErrorString(e));
  for (int i = 0; i < ZEGGS_LOUD_READ_WORDS; ++i) out[i] = 0.0;
  out[ZEGGS_LOUD_READ_LUFS] = h.lufs;
  out[ZEGGS_LOUD_READ_GAIN] = (double)h.gain;
  out[ZEGGS_LOUD_READ_BLOCKS] = (double)h.blocks;
  out[ZEGGS_LOUD_READ_GATED] = (double)h.gated;
  out[ZEGGS_LOUD_READ_HELD] = (double)h.kept;
  out[ZEGGS_LOUD_READ_SAMPLES] = (double)h.n;
  out[ZEGGS_LOUD_READ_HOLD] = (double)h.hold;
  return 0;
}
