// Dataset preparation (reference ZEGGS/data_pipeline.py:234-736, the stages around preprocess_audio / preprocess_animation):
//   * zeggs_spline_resample : the len_ratios time-stretch of a table [N, W] -> [M, W]: the not-a-knot cubic spline over the integer
//     grid evaluated at linspace(0, N-1, M) (griddata(method = "cubic") on 1-D points = interp1d(kind = "cubic")), float64 as scipy;
//   * zeggs_rot_stretch     : Euler degrees -> quaternions -> sign unrolling -> spline on the four components -> normalise -> Euler;
//   * zeggs_audio_prepare   : speaker silencing (union of sample intervals) and the [start, end) cut in one pass;
//   * zeggs_center_take     : the centring of a trimmed take (data_pipeline.py:449-459), in place;
//   * zeggs_masked_stats    : per-column mean / population std and the pooled std of a float32 table under a row mask, float64
//     accumulation, workgroup partials combined in a fixed order (two runs give the same bits).
// Plain HIP, HBM- or latency-bound; nothing here has a matrix product.
#include "../../include/zeggs_hip.h"
#include "common.h"
#include "anim_math.h"
#include "spline.h"

namespace {

// ------------------------------------------------------------------ spline evaluation (the solver: spline.h)
// evaluation at t_k = k (N-1) / (M-1)  (numpy.linspace: arange(M) * step, the last sample set to N-1 exactly)
__global__ void spline_eval_k(const double* __restrict__ y, const double* __restrict__ S, long N, int W, long M, double* __restrict__ out) {
  const long n = M * W;
  const double step = M > 1 ? (double)(N - 1) / (double)(M - 1) : 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long k = i / W;
    const int c = (int)(i % W);
    const double t = (k == M - 1 && M > 1) ? (double)(N - 1) : (double)k * step;
    long lo = (long)t;
    if (lo > N - 2) lo = N - 2;
    out[i] = spline_piece(y[lo * W + c], y[(lo + 1) * W + c], S[lo * W + c], S[(lo + 1) * W + c], t - (double)lo);
  }
}

inline dim3 grid_for(long n, int block) { long g = (n + block - 1) / block; return dim3((unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g))); }

// the time-stretch of a table: second derivatives into S, then the evaluation at the M new times
void spline_launch(const double* y, long N, int W, long M, double* out, double* S, hipStream_t s) {
  spline_second_derivatives(y, N, W, S, s);
  hipLaunchKernelGGL(spline_eval_k, grid_for(M * W, 256), dim3(256), 0, s, y, S, N, W, M, out);
}

// ------------------------------------------------------------------ rotation stretch
// signed (unrolled) quaternions as one table [N, 4 J]
__global__ void rot_sign_k(double* lrot, const double* sign, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const double s = sign[i];
    DQ q = ldq(lrot + i * 4);
    stq(lrot + i * 4, DQ{s * q.w, s * q.x, s * q.y, s * q.z});
  }
}
__global__ void rot_euler_k(const double* quat, double* euler, long n, int order) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    DQ q = ldq(quat + i * 4);
    const double nrm = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);      // quat.normalize, eps = 0
    q = DQ{q.w / nrm, q.x / nrm, q.y / nrm, q.z / nrm};
    dq_to_euler_deg(q, euler + i * 3, order);
  }
}
struct RotWs { double *lrot, *dprev, *sign, *S, *qout; };
RotWs carve_rot(long N, int J, long M, Arena& a) {
  RotWs w;
  w.lrot = (double*)a.raw((size_t)N * J * 4 * sizeof(double));
  w.dprev = (double*)a.raw((size_t)N * J * sizeof(double));
  w.sign = (double*)a.raw((size_t)N * J * sizeof(double));
  w.S = (double*)a.raw((size_t)N * J * 4 * sizeof(double));
  w.qout = (double*)a.raw((size_t)M * J * 4 * sizeof(double));
  return w;
}

// ------------------------------------------------------------------ audio: silence + cut
__global__ void audio_prepare_k(const float* __restrict__ wav, long n_wav, const long* __restrict__ iv, int n_iv, long start, long n_out,
                                float* __restrict__ out32, double* __restrict__ out64) {
  extern __shared__ long ivs[];
  for (int i = threadIdx.x; i < 2 * n_iv; i += blockDim.x) ivs[i] = iv[i];
  __syncthreads();
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (long)gridDim.x * blockDim.x) {
    const long p = start + i;
    bool keep = false;
    for (int j = 0; j < n_iv; ++j) keep = keep || (p >= ivs[2 * j] && p < ivs[2 * j + 1]);
    const float v = (keep && p < n_wav) ? wav[p] : 0.0f;      // (x * 0 of the reference: +-0, the same sample in a file and in a sum)
    if (out32) out32[i] = v;
    if (out64) out64[i] = (double)v;
  }
}

// ------------------------------------------------------------------ trimmed-take centring
// offsets of frame 0: position (x, 0, z) and the raw (w, 0, y, 0) of the root quaternion -- NOT normalised, as the reference
__global__ void center_offset_k(const double* pos, const double* euler, int order, double* off) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const DQ q = dq_from_euler_deg(euler, order);
    off[0] = pos[0]; off[1] = 0.0; off[2] = pos[2];
    off[3] = q.w; off[4] = 0.0; off[5] = -q.y; off[6] = 0.0;       // quat.inv of it
  }
}
__global__ void center_apply_k(double* pos, double* euler, long N, int J, int order, int round32, const double* off) {
  const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= N) return;
  const DQ inv = ldq(off + 3);
  double* p = pos + f * J * 3;
  double* e = euler + f * J * 3;
  D3 v = dq_mul_vec(inv, ld3(p) - ld3(off));
  double r[3];
  dq_to_euler_deg(dq_mul(inv, dq_from_euler_deg(e, order)), r, order);
  if (round32) {                                           // the take is stored as float32 (a take that was not stretched)
    v = D3{(double)(float)v.x, (double)(float)v.y, (double)(float)v.z};
    r[0] = (double)(float)r[0]; r[1] = (double)(float)r[1]; r[2] = (double)(float)r[2];
  }
  st3(p, v);
  e[0] = r[0]; e[1] = r[1]; e[2] = r[2];
}

// ------------------------------------------------------------------ masked statistics
// pass 0: column sums of the masked rows (and their count); pass 1: column sums of (x - mean)^2.  Workgroup (rows slab, column tile):
// 256 threads = TR row lanes x TCOL columns (TCOL = 64, or the next power of two >= D for narrow arrays, so that a 1-column array
// still uses every lane); the row lanes are added in lane order, the slabs in slab order: fixed, run after run.
constexpr int ST_ROWS = 2048, ST_T = 256;
__global__ __launch_bounds__(ST_T) void stats_partial_k(const float* __restrict__ x, const unsigned char* __restrict__ mask, long R, int D,
                                                        int tcol, int pass, const double* __restrict__ mean, double* __restrict__ part,
                                                        double* __restrict__ cnt) {
  __shared__ double red[ST_T], redn[ST_T];
  const int tr = ST_T / tcol, tx = threadIdx.x % tcol, ty = threadIdx.x / tcol;
  const int c = blockIdx.y * tcol + tx;
  const long r0 = (long)blockIdx.x * ST_ROWS, r1 = r0 + ST_ROWS < R ? r0 + ST_ROWS : R;
  double acc = 0.0, n = 0.0;
  if (c < D) {
    const double m = pass ? mean[c] : 0.0;
    for (long r = r0 + ty; r < r1; r += tr)
      if (mask[r]) {
        const double v = (double)x[r * D + c] - m;
        acc += pass ? v * v : v;
        n += 1.0;
      }
  }
  red[threadIdx.x] = acc; redn[threadIdx.x] = n;
  __syncthreads();
  if (ty == 0 && c < D) {
    double s = 0.0, sn = 0.0;
    for (int j = 0; j < tr; ++j) { s += red[j * tcol + tx]; sn += redn[j * tcol + tx]; }
    part[(long)blockIdx.x * D + c] = s;
    if (c == 0 && pass == 0) cnt[blockIdx.x] = sn;
  }
}
// pass 0: mean = sum / n.  pass 1: std = sqrt(ssq / n)
__global__ void stats_combine_k(const double* __restrict__ part, const double* __restrict__ cnt, int nblk, int D, int pass,
                                double* __restrict__ n_out, double* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= D) return;
  double n = 0.0, s = 0.0;
  if (pass == 0) { for (int b = 0; b < nblk; ++b) n += cnt[b]; if (c == 0) *n_out = n; } else n = *n_out;
  for (int b = 0; b < nblk; ++b) s += part[(long)b * D + c];
  out[c] = pass ? sqrt(s / n) : s / n;
}
// pooled std over all masked elements from the column statistics: sum (x - g)^2 = sum_c [ ssq_c + n (m_c - g)^2 ], one thread, column order
__global__ void stats_pooled_k(const double* __restrict__ mean, const double* __restrict__ std_, int D, double* __restrict__ pooled) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double g = 0.0;
  for (int c = 0; c < D; ++c) g += mean[c];
  g /= (double)D;
  double s = 0.0;
  for (int c = 0; c < D; ++c) s += std_[c] * std_[c] + (mean[c] - g) * (mean[c] - g);
  *pooled = sqrt(s / (double)D);
}
struct StatWs { double *part, *cnt, *n; };
StatWs carve_stats(long R, int D, Arena& a) {
  StatWs w;
  const long nblk = (R + ST_ROWS - 1) / ST_ROWS;
  w.part = (double*)a.raw((size_t)nblk * D * sizeof(double));
  w.cnt = (double*)a.raw((size_t)nblk * sizeof(double));
  w.n = (double*)a.raw(sizeof(double));
  return w;
}

}  // namespace

extern "C" int zeggs_spline_chunk(int* chunk, int* halo, int* narrow_width) {
  if (chunk) *chunk = SPL_C;
  if (halo) *halo = SPL_H;
  if (narrow_width) *narrow_width = SPL_NW;
  return 0;
}

extern "C" size_t zeggs_spline_resample_workspace_bytes(long N, int W) { return (size_t)N * W * sizeof(double) + 256; }

extern "C" int zeggs_spline_resample(const double* y, long N, int W, long M, double* out, void* ws, size_t ws_bytes, void* stream) {
  ZCHECK(N >= 4, "spline_resample: a cubic spline needs at least 4 rows, got %ld", N);
  ZCHECK(W >= 1 && M >= 1, "spline_resample: empty table (W = %d, M = %ld)", W, M);
  ZCHECK(N * (long)W < (1L << 40) && M * (long)W < (1L << 40), "spline_resample: table too large");
  Arena a(ws, ws_bytes);
  double* S = (double*)a.raw((size_t)N * W * sizeof(double));
  ZCHECK(a.ok() && ws != nullptr, "spline_resample: workspace too small (%zu < %zu)", ws_bytes, a.off);
  spline_launch(y, N, W, M, out, S, (hipStream_t)stream);
  ZLAUNCH_CHECK("spline_resample");
  return 0;
}

extern "C" size_t zeggs_rot_stretch_workspace_bytes(long N, int J, long M) {
  Arena a(nullptr, 0);
  carve_rot(N, J, M, a);
  return a.off + 256;
}

extern "C" int zeggs_rot_stretch(const double* euler_deg, long N, int J, long M, int order, double* out_deg, void* ws, size_t ws_bytes,
                                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  ZCHECK(N >= 4 && N < (1L << 31), "rot_stretch: need 4 .. 2^31 frames, got %ld", N);
  ZCHECK(J >= 1 && M >= 1, "rot_stretch: empty clip (J = %d, M = %ld)", J, M);
  const int oc = order_code(order);
  ZCHECK(oc == ORDER_ZYX || oc == ORDER_XZY, "rot_stretch: Cannot convert to this ordering (to_euler has \"zyx\" and \"xzy\")");
  Arena a(ws, ws_bytes);
  RotWs w = carve_rot(N, J, M, a);
  ZCHECK(a.ok() && ws != nullptr, "rot_stretch: workspace too small (%zu < %zu)", ws_bytes, a.off);
  const long NJ = N * J;
  hipLaunchKernelGGL(anim_quat_k, grid_for(NJ, 256), dim3(256), 0, s, euler_deg, w.lrot, w.dprev, (int)N, J, oc);
  hipLaunchKernelGGL(anim_unroll_k, dim3((J + 63) / 64), dim3(64), 0, s, w.dprev, w.sign, (int)N, J);
  hipLaunchKernelGGL(rot_sign_k, grid_for(NJ, 256), dim3(256), 0, s, w.lrot, w.sign, NJ);
  spline_launch(w.lrot, N, 4 * J, M, w.qout, w.S, s);
  hipLaunchKernelGGL(rot_euler_k, grid_for(M * J, 256), dim3(256), 0, s, w.qout, out_deg, M * J, oc);
  ZLAUNCH_CHECK("rot_stretch");
  return 0;
}

extern "C" int zeggs_audio_prepare(const float* wav, long n_wav, const long* intervals, int n_intervals, long start, long end,
                                   float* out_f32, double* out_f64, void* stream) {
  ZCHECK(n_wav >= 0 && start >= 0 && end >= start, "audio_prepare: bad range [%ld, %ld) of %ld samples", start, end, n_wav);
  ZCHECK(n_intervals >= 0 && n_intervals <= 4096, "audio_prepare: 0 .. 4096 intervals, got %d", n_intervals);
  const long n_out = (end < n_wav ? end : n_wav) - start;            // (a slice past the end is cut short, as numpy's)
  if (n_out <= 0) return 0;                                          // (an empty cut: nothing to write, an empty tensor has no address)
  ZCHECK(out_f32 != nullptr || out_f64 != nullptr, "audio_prepare: no output");
  hipLaunchKernelGGL(audio_prepare_k, grid_for(n_out, 256), dim3(256), (size_t)2 * n_intervals * sizeof(long), (hipStream_t)stream, wav,
                     n_wav, intervals, n_intervals, start, n_out, out_f32, out_f64);
  ZLAUNCH_CHECK("audio_prepare");
  return 0;
}

extern "C" int zeggs_center_take(double* positions, double* euler_deg, long N, int J, int order, int round_f32, void* ws, size_t ws_bytes,
                                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  ZCHECK(N >= 1 && J >= 1, "center_take: empty clip");
  const int oc = order_code(order);
  ZCHECK(oc == ORDER_ZYX || oc == ORDER_XZY, "center_take: Cannot convert to this ordering (to_euler has \"zyx\" and \"xzy\")");
  ZCHECK(ws != nullptr && ws_bytes >= 8 * sizeof(double), "center_take: workspace too small (%zu < 64)", ws_bytes);
  hipLaunchKernelGGL(center_offset_k, dim3(1), dim3(64), 0, s, positions, euler_deg, oc, (double*)ws);
  hipLaunchKernelGGL(center_apply_k, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, positions, euler_deg, N, J, oc, round_f32,
                     (const double*)ws);
  ZLAUNCH_CHECK("center_take");
  return 0;
}

extern "C" size_t zeggs_masked_stats_workspace_bytes(long R, int D) {
  Arena a(nullptr, 0);
  carve_stats(R, D, a);
  return a.off + 256;
}

extern "C" int zeggs_masked_stats(const float* x, const unsigned char* mask, long R, int D, double* mean, double* std_, double* pooled,
                                  void* ws, size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  ZCHECK(R >= 1 && D >= 1, "masked_stats: empty table");
  Arena a(ws, ws_bytes);
  StatWs w = carve_stats(R, D, a);
  ZCHECK(a.ok() && ws != nullptr, "masked_stats: workspace too small (%zu < %zu)", ws_bytes, a.off);
  const long nblk = (R + ST_ROWS - 1) / ST_ROWS;
  ZCHECK(nblk < (1L << 31), "masked_stats: too many rows");
  int tcol = 64;
  if (D < 64) { tcol = 1; while (tcol < D) tcol *= 2; }
  const dim3 grid((unsigned)nblk, (unsigned)((D + tcol - 1) / tcol));
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(stats_partial_k, grid, dim3(ST_T), 0, s, x, mask, R, D, tcol, pass, mean, w.part, w.cnt);
    hipLaunchKernelGGL(stats_combine_k, dim3((unsigned)((D + 63) / 64)), dim3(64), 0, s, w.part, w.cnt, (int)nblk, D, pass, w.n,
                       pass ? std_ : mean);
  }
  hipLaunchKernelGGL(stats_pooled_k, dim3(1), dim3(64), 0, s, mean, std_, D, pooled);
  ZLAUNCH_CHECK("masked_stats");
  return 0;
}
