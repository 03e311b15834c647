// The not-a-knot cubic spline over the integer grid 0 .. N-1, one per column of a float64 table: the single statement for the
// dataset preparation (prepare.hip: the len_ratios time-stretch) and the audio front-end (mel.hip: resample_method = "cubic").
// It is scipy's interp1d(kind = "cubic") = make_interp_spline(k = 3) = griddata(method = "cubic") on 1-D points, float64 as scipy.
// In terms of the second derivatives S_i:  S_{i-1} + 4 S_i + S_{i+1} = 6 (y_{i-1} - 2 y_i + y_{i+1}) =: r_i  (i = 1 .. N-2), and the
// not-a-knot conditions S_0 - 2 S_1 + S_2 = 0, S_{N-3} - 2 S_{N-2} + S_{N-1} = 0 turn the first and last equation into S_1 = r_1 / 6,
// S_{N-2} = r_{N-2} / 6.  What is left (i = 2 .. N-3) is a strictly diagonally dominant tridiagonal system (spline.hip solves it in
// chunks), and the ends follow as S_0 = 2 S_1 - S_2, S_{N-1} = 2 S_{N-2} - S_{N-3}.
#pragma once
#include <hip/hip_runtime.h>

// rows per chunk / rows a chunk's sweeps start early and look past its end / widest table of the narrow kernel (zeggs_spline_chunk)
constexpr int SPL_C = 64, SPL_H = 40, SPL_NW = 8;

// second derivatives of the splines through the columns of y [N, W] into S [N, W], enqueued on stream s (N >= 4)
void spline_second_derivatives(const double* y, long N, int W, double* S, hipStream_t s);

// the spline between two neighbouring grid points at the fraction u of the way from the lower to the upper one
__device__ __forceinline__ double spline_piece(double ylo, double yhi, double Slo, double Shi, double u) {
  const double v = 1.0 - u;
  return ylo * v + yhi * u + ((v * v * v - v) * Slo + (u * u * u - u) * Shi) / 6.0;
}
