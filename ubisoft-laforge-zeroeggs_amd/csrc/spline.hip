// Second derivatives of the not-a-knot cubic splines through the columns of a float64 table (spline.h has the equations).
// The interior system is strictly diagonally dominant: what a row feels of a row k places away decays like (2 - sqrt 3)^k = 0.268^k
// (1e-23 at k = 40), so the Thomas elimination is cut into chunks of SPL_C rows that start SPL_H rows early from an arbitrary state and
// look SPL_H rows past their end before substituting back: exact to the last bit of float64 (144 000 rows, 30 minutes of audio
// features, in ~0.1 ms instead of 45 ms as one sequential sweep).  The elimination coefficients c_0 = 1/4, c_j = 1 / (4 - c_{j-1})
// depend only on the distance j from where a sweep started and are the same double from j = 15 on (they converge like 0.0718^j): a
// compile-time table, no division in the sweeps.
#include "spline.h"

namespace {

constexpr int SPL_NC = 32;
struct SplCoef {
  double c[SPL_NC];
  constexpr SplCoef() : c{} {
    double p = 0.0;
    for (int j = 0; j < SPL_NC; ++j) { p = 1.0 / (4.0 - p); c[j] = p; }
  }
};
__constant__ const SplCoef spl_coef{};
__device__ __forceinline__ double spl_c(long j) { return spl_coef.c[j < SPL_NC ? j : SPL_NC - 1]; }

// Wide tables (the 225 position and 300 quaternion columns, the 81 audio features): thread = column, so that a row's loads are
// coalesced; one workgroup (one wave) per (chunk, tile of 64 columns).  The rows of the chunk are written to S as d' and turned into S
// by the back-substitution; the d' of the rows past the chunk's end wait in LDS.
constexpr int SPL_WT = 64;
__global__ __launch_bounds__(SPL_WT) void spline_solve_wide_k(const double* __restrict__ y, long N, int W, double* __restrict__ S) {
  __shared__ double halo[SPL_H][SPL_WT];
  const int c = blockIdx.y * SPL_WT + threadIdx.x;
  if (c >= W) return;                                   // (no barrier below: a lane owns its column from start to end)
  const long lo = 2, hi = N - 3;
  const long a = lo + (long)blockIdx.x * SPL_C;
  if (a > hi) return;
  const long b = (a + SPL_C - 1 < hi) ? a + SPL_C - 1 : hi;
  const long st = (a - SPL_H > lo) ? a - SPL_H : lo, en = (b + SPL_H < hi) ? b + SPL_H : hi;
  double ym = y[(st - 1) * W + c], y0 = y[st * W + c], d = 0.0;
  for (long i = st; i <= en; ++i) {
    const double yp = y[(i + 1) * W + c];
    double rhs = 6.0 * ((ym - y0) - (y0 - yp));
    if (i == lo) rhs -= (y[c] - y[W + c]) - (y[W + c] - y[2L * W + c]);                                  // S_1
    if (i == hi) rhs -= (y[(N - 3) * W + c] - y[(N - 2) * W + c]) - (y[(N - 2) * W + c] - y[(N - 1) * W + c]);   // S_{N-2}
    d = (rhs - d) * spl_c(i - st);
    if (i >= a && i <= b) S[i * W + c] = d;
    else if (i > b) halo[i - b - 1][threadIdx.x] = d;
    ym = y0; y0 = yp;
  }
  double x = 0.0;                                        // (en < hi: as if the row behind were zero -- forgotten before row b)
  for (long i = en; i >= a; --i) {
    const double dp = (i > b) ? halo[i - b - 1][threadIdx.x] : S[i * W + c];
    x = dp - spl_c(i - st) * x;
    if (i <= b) S[i * W + c] = x;
  }
}

// Narrow tables (the audio: W = 1, N in the millions): thread = (chunk, column), 64 / W chunks side by side in a wave.  A thread walks
// rows SPL_C * W doubles apart, so the workgroup's rows go through LDS: loaded and stored as one contiguous, coalesced range, and laid out
// chunk by chunk with one spare row per chunk -- lane (k, c) then sits at k (SPL_C + 1) W + c = lane (mod 32 doubles): no bank conflict
// among the 32 lanes that share an LDS cycle.  The sweeps work in place:
//   1. (reads only) every thread runs the SPL_H rows in front of its chunk and keeps y of the row behind it;
//   2. its own rows: y -> d';  the d' of the rows past its end are the NEXT threads' own rows (both started >= SPL_H rows earlier:
//      the same numbers), so nobody eliminates them twice; the last thread of the workgroup exists for that only;
//   3. (reads only) back-substitution over the SPL_H rows past the chunk; 4. own rows: d' -> S.
constexpr int SPL_NT = 64;                               // threads of a narrow workgroup
__device__ __forceinline__ int spl_idx(long tr, int W, int c) { return (int)((tr / SPL_C) * (SPL_C + 1) + (tr % SPL_C)) * W + c; }
__global__ __launch_bounds__(SPL_NT) void spline_solve_narrow_k(const double* __restrict__ y, long N, int W, double* __restrict__ S) {
  __shared__ double T[(SPL_NT + 2 * SPL_NW) * (SPL_C + 1)];   // (TC + 2) chunks of (SPL_C + 1) rows of W columns: TC W <= 64, W <= SPL_NW
  const int TC = SPL_NT / W, TCo = TC - 1;               // chunks walked / chunks written by this workgroup
  const long lo = 2, hi = N - 3;
  const long q0 = (long)blockIdx.x * TCo;                // first chunk
  const long R0 = lo + q0 * SPL_C - SPL_C;               // table row of tile row 0 (one chunk of rows in front: the first thread's run-up)
  const long nrows = (long)(TC + 1) * SPL_C + 2;         // ... up to two rows past the last chunk (S_{N-2} needs y_{N-1})
  for (long f = threadIdx.x; f < nrows * W; f += SPL_NT) {
    const long tr = f / W, r = R0 + tr;
    T[spl_idx(tr, W, (int)(f % W))] = (r >= 0 && r < N) ? y[R0 * W + f] : 0.0;
  }
  __syncthreads();
  const int k = threadIdx.x / W, c = threadIdx.x % W;
  const long a = lo + (q0 + k) * SPL_C;
  const bool on = k < TC && a <= hi;
  const long b = (a + SPL_C - 1 < hi) ? a + SPL_C - 1 : hi;
  const long st = (a - SPL_H > lo) ? a - SPL_H : lo, en = (b + SPL_H < hi) ? b + SPL_H : hi;
  auto t = [&](long r) -> double& { return T[spl_idx(r - R0, W, c)]; };
  double ym = 0.0, y0 = 0.0, ynext = 0.0, d = 0.0, s1 = 0.0, sl = 0.0;
  if (on) {                                              // 1.
    ym = t(st - 1); y0 = t(st);
    for (long i = st; i < a; ++i) {
      const double yp = t(i + 1);
      d = (6.0 * ((ym - y0) - (y0 - yp)) - d) * spl_c(i - st);      // (st > lo here: a run-up exists only behind the first chunk)
      ym = y0; y0 = yp;
    }
    ynext = t(b + 1);
    if (a == lo) s1 = (t(0) - t(1)) - (t(1) - t(2));
    if (b == hi) sl = (t(N - 3) - t(N - 2)) - (t(N - 2) - t(N - 1));
  }
  __syncthreads();
  if (on) {                                              // 2.
    for (long i = a; i <= b; ++i) {
      const double yp = (i < b) ? t(i + 1) : ynext;
      double rhs = 6.0 * ((ym - y0) - (y0 - yp));
      if (i == lo) rhs -= s1;
      if (i == hi) rhs -= sl;
      d = (rhs - d) * spl_c(i - st);
      t(i) = d;
      ym = y0; y0 = yp;
    }
  }
  __syncthreads();
  double x = 0.0;
  if (on && k < TCo)                                     // 3. (rows of the threads behind: their sweeps started >= SPL_H rows earlier)
    for (long i = en; i > b; --i) x = t(i) - spl_c(SPL_NC) * x;
  __syncthreads();
  if (on && k < TCo)                                     // 4.
    for (long i = b; i >= a; --i) { x = t(i) - spl_c(i - st) * x; t(i) = x; }
  __syncthreads();
  const long r_first = lo + q0 * SPL_C;                  // rows of the TCo chunks written here: contiguous in the table
  long r_last = r_first + (long)TCo * SPL_C - 1;
  if (r_last > hi) r_last = hi;
  for (long f = threadIdx.x; f < (r_last - r_first + 1) * W; f += SPL_NT)
    S[r_first * W + f] = T[spl_idx(SPL_C + f / W, W, (int)(f % W))];
}

// the two rows next to the ends and the ends themselves (not-a-knot)
__global__ void spline_ends_k(const double* __restrict__ y, long N, int W, double* __restrict__ S) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= W) return;
  const double s1 = (y[c] - y[W + c]) - (y[W + c] - y[2L * W + c]);
  const double sl = (y[(N - 3) * W + c] - y[(N - 2) * W + c]) - (y[(N - 2) * W + c] - y[(N - 1) * W + c]);
  const double s2 = N > 4 ? S[2L * W + c] : sl, sm3 = N > 4 ? S[(N - 3) * W + c] : s1;
  S[W + c] = s1;
  S[c] = 2.0 * s1 - s2;
  S[(N - 2) * W + c] = sl;
  S[(N - 1) * W + c] = 2.0 * sl - sm3;
}

}  // namespace

void spline_second_derivatives(const double* y, long N, int W, double* S, hipStream_t s) {
  const long hi = N - 3, nchunk = hi >= 2 ? (hi - 2) / SPL_C + 1 : 0;
  if (nchunk > 0) {
    if (W <= SPL_NW) {
      const long per = SPL_NT / W - 1;
      hipLaunchKernelGGL(spline_solve_narrow_k, dim3((unsigned)((nchunk + per - 1) / per)), dim3(SPL_NT), 0, s, y, N, W, S);
    } else {
      hipLaunchKernelGGL(spline_solve_wide_k, dim3((unsigned)nchunk, (unsigned)((W + SPL_WT - 1) / SPL_WT)), dim3(SPL_WT), 0, s, y, N, W, S);
    }
  }
  hipLaunchKernelGGL(spline_ends_k, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, s, y, N, W, S);
}
