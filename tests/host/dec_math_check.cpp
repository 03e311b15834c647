// csrc/quat_math.h + csrc/dec_math.h on the host: the fp32 step math of the decoder kernels against a float64 statement of the
// same formulas, written here from the reference (ZEGGS/anim/tquat.py: quat_mul, quat_mul_vec, quat_inv, quat_exp,
// quat_from_helical; ZEGGS/modules.py:696 gaze direction, :739-740 root update) and NOT from the headers.
//   (a) root_step, gaze_dir (and the float64 diagnostic root_step_fp64) against float64
//   (b) the one-piece adjoint root_bwd against the float64 analytic adjoint
//   (c) the float64 analytic adjoint against central differences of the float64 forward (differences taken in long double, so
//       that their own rounding stays below the comparison) -- this is what pins the derivation
//   (d) the split adjoint (root_prepare -> the 33 stored slots -> root_apply) against the one-piece adjoint, same inputs
//   (e) gru_cell_bwd against float64
// The half angle h = |vrt dt / 2| is drawn log-uniformly inside each branch of the exponential -- h < 1e-5, 1e-5 <= h < 1,
// h >= 1 -- a third of the cases each; the shares are printed and a branch below a tenth fails the run.
// Every error is max |got - want| / max |want| over the entries of the compared quantity, maximised over the cases of a branch;
// the adjoint carry is compared in two further ways, below.
// Bounds = 4 x the maximum measured with the shipped sample set (300 000 cases; x86-64, g++ 11 -O2 and clang++ 22 -O2 give the
// same figures); the factor covers another host's libm and compiler.  Measured, per branch (h < 1e-5 | 1e-5 <= h < 1 | h >= 1):
//   (a) root_step: root_pos              8.923e-08  6.378e-08  6.500e-08
//   (a) root_step: root_rot              5.768e-08  3.068e-07  9.951e-07
//   (a) gaze_dir                         4.186e-07  4.605e-07  5.175e-07
//   (a) root_step_fp64: root_pos         5.940e-08  5.941e-08  5.957e-08
//   (a) root_step_fp64: root_rot         5.768e-08  5.790e-08  5.720e-08
//   (b) half-rotation vector hu          4.154e-07  3.783e-07  3.830e-07
//   (b) root_bwd: carry / summands       4.133e-07  4.198e-07  5.156e-07
//   (b) root_bwd: carry, well cond.      6.812e-07  6.830e-07  9.595e-07
//   same vs the fp64 point (info only)   6.812e-07  6.831e-07  2.018e-06
//   (b) root_bwd: g6                     1.959e-07  2.112e-07  3.602e-07
//   (c) fp64 adjoint vs differences      1.347e-12  8.503e-11  8.390e-10
//   (d) split: carry / summands          3.276e-07  3.444e-07  4.716e-07
//   (d) split: carry, well cond.         5.481e-07  6.634e-07  7.172e-07
//   (d) split vs one piece: g6           2.517e-07  2.011e-07  2.420e-07
//   (e) gru_cell_bwd                     6.701e-07  7.068e-07  6.281e-07
// Every asserted figure is below 1e-6.  The adjoint carry (gradient wrt root_pos, root_rot of the frame before) needs care, because
// against the float64 adjoint at the float64 point and its own largest entry it reads 7.7e-7 | 1.6e-6 | 2.4e-5 over ALL cases.
// Two things make that up, and the program separates them:
//   * the carry is a sum -- dq1 + dqy + dq2, each of the rotation adjoints again a sum, the gaze term added to the incoming
//     gradient -- whose terms reach 27 x (h < 1) and 114 x (h >= 1) the result: for a unit q the exact map is
//     nq = q * exp(vrt dt / 2), of size |g|, while dqy and dq2 each grow with the angle |vrt dt| = 2 h, and the gaze term puts
//     2 |gaze - root_pos| |dgd| / sigma (up to 80 here) into the gradient of root_rot.  "carry / summands" holds EVERY case to the
//     size of those terms (a running sum of absolute values, carried through the exponential's and the rotation's adjoint in
//     float64): 4.1e-7 ... 5.2e-7 in all three branches, seven roundings.  "well cond." holds the cases whose terms are at most
//     WELL = 2 x the result to the result's own largest entry (61 % | 49 % | 6 % of the cases).
//   * the adjoint is evaluated at the fp32 code's own half-rotation vector hu (row "hu": 4e-7 from float64, the rounding of the
//     forward pass); the curvature of the exponential times the factor 2 h of the rotation adjoint turns that into an error that
//     grows like h^2.  It is not a property of the adjoint's arithmetic, so both rows compare with the float64 adjoint AT that hu;
//     the distance to the float64 point is printed for the well-conditioned cases (6.8e-7 | 6.8e-7 | 2.0e-6) and not asserted.
// Neither point needs the gaze term: at h >= 1 the sum dqy + dq2 and the h^2 growth are there without a next frame.  (c) pins
// the float64 derivation itself to 1e-9.  h >= 1, two radians per frame, does not occur in motion data.
// Usage: dec_math_check [cases, default 300000].  Prints "dec_math_check: ok" when every bound holds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../ubisoft-laforge-zeroeggs_amd/csrc/dec_math.h"

#define B3_(a, b, c) {4 * a, 4 * b, 4 * c}, {0, 0, 0}
#define B3(m) B3_(m)
#define M_POS 8.923e-08, 6.378e-08, 6.500e-08
#define M_ROT 5.768e-08, 3.068e-07, 9.951e-07
#define M_GAZE 4.186e-07, 4.605e-07, 5.175e-07
#define M_F64P 5.940e-08, 5.941e-08, 5.957e-08
#define M_F64R 5.768e-08, 5.790e-08, 5.720e-08
#define WELL 2.0      // summands at most 2 x the result: seven chained stages at 6e-8 each (4e-7 of the summands) stay below 1e-6 of the result
#define M_HU 4.154e-07, 3.783e-07, 3.830e-07
#define M_AC 4.133e-07, 4.198e-07, 5.156e-07
#define M_ACW 6.812e-07, 6.830e-07, 9.595e-07
#define M_AG 1.959e-07, 2.112e-07, 3.602e-07
#define M_FD 1.347e-12, 8.503e-11, 8.390e-10
#define M_SC 3.276e-07, 3.444e-07, 4.716e-07
#define M_SCW 5.481e-07, 6.634e-07, 7.172e-07
#define M_SG 2.517e-07, 2.011e-07, 2.420e-07
#define M_GRU 6.701e-07, 7.068e-07, 6.281e-07
static uint64_t g_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {      // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
static double unit() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }      // [0, 1)
static double sym(double a) { return a * (2.0 * unit() - 1.0); }
static double logu(double lo, double hi) { return exp(log(lo) + unit() * (log(hi) - log(lo))); }

// ------------------------------------------------------------------ the float64 statement (T = double, or long double under (c))
template <class T> static T t_sqrt(T x);
template <> double t_sqrt(double x) { return sqrt(x); }
template <> long double t_sqrt(long double x) { return sqrtl(x); }
template <class T> static T t_sin(T x);
template <> double t_sin(double x) { return sin(x); }
template <> long double t_sin(long double x) { return sinl(x); }
template <class T> static T t_cos(T x);
template <> double t_cos(double x) { return cos(x); }
template <> long double t_cos(long double x) { return cosl(x); }

template <class T> static void r_cross(const T* a, const T* b, T* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
template <class T> static void r_quat_mul(const T* x, const T* y, T* o) {      // tquat.py:6-15
  o[0] = y[0] * x[0] - y[1] * x[1] - y[2] * x[2] - y[3] * x[3];
  o[1] = y[0] * x[1] + y[1] * x[0] - y[2] * x[3] + y[3] * x[2];
  o[2] = y[0] * x[2] + y[1] * x[3] + y[2] * x[0] - y[3] * x[1];
  o[3] = y[0] * x[3] - y[1] * x[2] + y[2] * x[1] + y[3] * x[0];
}
template <class T> static void r_quat_mul_vec(const T* x, const T* y, T* o) {      // tquat.py:18-20
  T t[3], c[3];
  r_cross(x + 1, y, t);
  for (int i = 0; i < 3; ++i) t[i] *= 2;
  r_cross(x + 1, t, c);
  for (int i = 0; i < 3; ++i) o[i] = y[i] + x[0] * t[i] + c[i];
}
template <class T> static void r_quat_exp(const T* x, T* o) {      // tquat.py:94-98, eps = 1e-5; sinc(h / pi) = sin(h) / h
  const T h = t_sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  if (h < (T)1e-5) {
    const T n = t_sqrt(1 + h * h) + (T)1e-5;      // quat_normalize([1, x])
    o[0] = 1 / n;
    for (int i = 0; i < 3; ++i) o[1 + i] = x[i] / n;
  } else {
    const T s = t_sin(h) / h;
    o[0] = t_cos(h);
    for (int i = 0; i < 3; ++i) o[1 + i] = x[i] * s;
  }
}
// modules.py:739-740 and :696.  in = [q(4) | pos(3) | p(6)], gz: gaze target; out = [npos(3) | nq(4) | gd(3)]
template <class T> static void r_forward(T dt, const T* in, const T* gz, T* out) {
  const T *q = in, *pos = in + 4, *p = in + 7;
  T v[3], w[3], u[3], e[4], ql[4], d[3];
  for (int i = 0; i < 3; ++i) { v[i] = p[i] * dt; w[i] = p[3 + i] * dt; }
  r_quat_mul_vec(q, v, out);
  for (int i = 0; i < 3; ++i) out[i] += pos[i];
  r_quat_mul_vec(q, w, u);
  for (int i = 0; i < 3; ++i) u[i] /= 2;      // quat_from_helical
  r_quat_exp(u, e);
  r_quat_mul(e, q, out + 3);
  ql[0] = out[3]; ql[1] = -out[4]; ql[2] = -out[5]; ql[3] = -out[6];      // quat_inv
  for (int i = 0; i < 3; ++i) d[i] = gz[i] - out[i];
  r_quat_mul_vec(ql, d, out + 7);
}

// ------------------------------------------------------------------ the float64 analytic adjoint (derived here; pinned by (c))
// vector-Jacobian products of o = quat_mul_vec(x, y) given g: o = y + 2 w (a x y) + 2 a x (a x y), a = x[1:], w = x[0]
// sz (optional): per entry of dx the sum of the absolute values of its terms -- what an evaluation of dx rounds against
static void a_quat_mul_vec(const double* x, const double* y, const double* g, double* dx, double* dy, double* sz = nullptr) {
  const double* a = x + 1;
  double ay[3], ga[3], aga[3], yga[3];
  r_cross(a, y, ay);
  r_cross(g, a, ga);       // g x a
  r_cross(a, ga, aga);     // a x (g x a)
  r_cross(y, ga, yga);     // y x (g x a)
  dx[0] = 2 * (g[0] * ay[0] + g[1] * ay[1] + g[2] * ay[2]);
  // d/dy: g + 2 w (g x a) + 2 (g x a) x a   [(a x (a x y)) . g = y . ((g x a) x a)]
  for (int i = 0; i < 3; ++i) dy[i] = g[i] + 2 * x[0] * ga[i] - 2 * aga[i];
  // d/da: 2 w (y x g) + 2 [ (a x y) x g + y x (g x a) ]
  double ayg[3], yg[3];
  r_cross(ay, g, ayg);
  r_cross(y, g, yg);
  for (int i = 0; i < 3; ++i) dx[1 + i] = 2 * x[0] * yg[i] + 2 * (ayg[i] + yga[i]);
  if (sz) {
    sz[0] = 2 * (fabs(g[0] * ay[0]) + fabs(g[1] * ay[1]) + fabs(g[2] * ay[2]));
    for (int i = 0; i < 3; ++i) sz[1 + i] = 2 * fabs(x[0] * yg[i]) + 2 * (fabs(ayg[i]) + fabs(yga[i]));
  }
}
static void z_cross(const double* a, const double* b, double* o) {      // |a| x |b| with every product counted positive
  o[0] = fabs(a[1] * b[2]) + fabs(a[2] * b[1]); o[1] = fabs(a[2] * b[0]) + fabs(a[0] * b[2]); o[2] = fabs(a[0] * b[1]) + fabs(a[1] * b[0]);
}
// the same sizes when the upstream gradient g is itself a sum known by the size gs of its terms
static void z_quat_mul_vec(const double* x, const double* y, const double* gs, double* sz) {
  double ay[3], ga[3], yg[3], ayg[3], yga[3];
  z_cross(x + 1, y, ay); z_cross(gs, x + 1, ga); z_cross(y, gs, yg); z_cross(ay, gs, ayg); z_cross(y, ga, yga);
  sz[0] = 2 * (gs[0] * ay[0] + gs[1] * ay[1] + gs[2] * ay[2]);
  for (int i = 0; i < 3; ++i) sz[1 + i] = 2 * fabs(x[0]) * yg[i] + 2 * (ayg[i] + yga[i]);
}
static void a_quat_mul(const double* x, const double* y, const double* g, double* dx, double* dy) {
  // o = M(y) x = N(x) y with the sign pattern of tquat.py:12-15; dx = M(y)^T g, dy = N(x)^T g
  const double M[4][4] = {{y[0], -y[1], -y[2], -y[3]}, {y[1], y[0], y[3], -y[2]}, {y[2], -y[3], y[0], y[1]}, {y[3], y[2], -y[1], y[0]}};
  const double N[4][4] = {{x[0], -x[1], -x[2], -x[3]}, {x[1], x[0], -x[3], x[2]}, {x[2], x[3], x[0], -x[1]}, {x[3], -x[2], x[1], x[0]}};
  for (int j = 0; j < 4; ++j) {
    dx[j] = 0; dy[j] = 0;
    for (int i = 0; i < 4; ++i) { dx[j] += M[i][j] * g[i]; dy[j] += N[i][j] * g[i]; }
  }
}
// sz (optional): per entry the sum of the absolute values of the terms of dx
static void a_quat_exp(const double* x, const double* g, double* dx, double* sz = nullptr) {
  const double h = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const double gx = g[1] * x[0] + g[2] * x[1] + g[3] * x[2];
  if (h < 1e-5) {      // [1, x] / (n + eps), n = sqrt(1 + h^2): d(1 / (n + eps)) / dx = -x / (n (n + eps)^2)
    const double n = sqrt(1 + h * h), ne = n + 1e-5;
    for (int i = 0; i < 3; ++i) dx[i] = g[1 + i] / ne - (g[0] + gx) * x[i] / (n * ne * ne);
    if (sz) for (int i = 0; i < 3; ++i) sz[i] = fabs(g[1 + i] / ne) + (fabs(g[0]) + fabs(gx)) * fabs(x[i]) / (n * ne * ne);
  } else {             // [cos h, x sin h / h]: dh / dx = x / h
    const double s = sin(h) / h, ds = (cos(h) - s) / h;      // d(sin h / h) / dh
    for (int i = 0; i < 3; ++i) dx[i] = g[1 + i] * s + (-g[0] * sin(h) + gx * ds) * x[i] / h;
    if (sz) for (int i = 0; i < 3; ++i) sz[i] = fabs(g[1 + i] * s) + (fabs(g[0] * sin(h)) + fabs(gx * ds)) * fabs(x[i]) / h;
  }
}
// gradient of L = <gout, r_forward(in)> wrt in (13 values); gout = [g_npos(3) | g_nq(4) | g_gd(3)]
// returns the size of the carry's summands: max over its entries of |terms of dq1| + |dqy| + |terms of dq2| (+ the largest entry
// of the gaze term's two gradients), the number an fp32 evaluation of that sum rounds against
static double a_forward(double dt, const double* in, const double* gz, const double* gout, double* gin, const double* hu = nullptr) {
  const double *q = in, *p = in + 7;
  double out[10];
  r_forward(dt, in, gz, out);
  double gnp[3] = {gout[0], gout[1], gout[2]}, gnq[4] = {gout[3], gout[4], gout[5], gout[6]}, gaze_size = 0;
  {   // gd = qmv(inv(nq), gz - npos)
    double ql[4] = {out[3], -out[4], -out[5], -out[6]}, d[3] = {gz[0] - out[0], gz[1] - out[1], gz[2] - out[2]}, dql[4], dd[3];
    a_quat_mul_vec(ql, d, gout + 7, dql, dd);
    gnq[0] += dql[0];
    for (int i = 0; i < 3; ++i) { gnq[1 + i] -= dql[1 + i]; gnp[i] -= dd[i]; }
    for (int i = 0; i < 4; ++i) gaze_size = fmax(gaze_size, fabs(dql[i]));
    for (int i = 0; i < 3; ++i) gaze_size = fmax(gaze_size, fabs(dd[i]));
  }
  double v[3], w[3], u[3], e[4], dq1[4], dv[3], de[4], dq2[4], du[3], dq3[4], dw[3], s1[4], s3[4], su[3];
  for (int i = 0; i < 3; ++i) { v[i] = p[i] * dt; w[i] = p[3 + i] * dt; }
  a_quat_mul_vec(q, v, gnp, dq1, dv, s1);
  r_quat_mul_vec(q, w, u);
  for (int i = 0; i < 3; ++i) u[i] = hu ? hu[i] : u[i] / 2;      // hu: the adjoint AT a given half-rotation vector (see (b) in main)
  r_quat_exp(u, e);
  a_quat_mul(e, q, gnq, de, dq2);
  a_quat_exp(u, de, du, su);
  for (int i = 0; i < 3; ++i) { du[i] /= 2; su[i] /= 2; }
  a_quat_mul_vec(q, w, du, dq3, dw);
  z_quat_mul_vec(q, w, su, s3);
  for (int i = 0; i < 4; ++i) gin[i] = dq1[i] + dq2[i] + dq3[i];
  for (int i = 0; i < 3; ++i) { gin[4 + i] = gnp[i]; gin[7 + i] = dv[i] * dt; gin[10 + i] = dw[i] * dt; }
  double size = 0;
  for (int i = 0; i < 4; ++i) size = fmax(size, s1[i] + fabs(dq2[i]) + s3[i]);
  for (int i = 0; i < 3; ++i) size = fmax(size, fabs(gout[i]));
  return size + gaze_size;
}

// ------------------------------------------------------------------ bookkeeping
struct Max {      // one compared quantity: worst case and bound per branch of the exponential (0: h < 1e-5, 1: h < 1, 2: h >= 1)
  const char* name; double bound[3], worst[3];
  void add(const double* got, const double* want, int n, int br, double scale = 0) {      // scale 0: the largest entry of `want`
    double d = 0, s = 0;
    for (int i = 0; i < n; ++i) { d = fmax(d, fabs(got[i] - want[i])); s = fmax(s, fabs(want[i])); }
    if (scale > 0) s = scale;
    if (s > 0) worst[br] = fmax(worst[br], d / s);
  }
  bool report() const {
    bool ok = true;
    printf("  %-34s", name);
    for (int b = 0; b < 3; ++b) {
      if (bound[b] >= 1) printf("  %.3e                  ", worst[b]);      // information only
      else printf("  %.3e (bound %.3e)%s", worst[b], bound[b], worst[b] <= bound[b] ? "" : " FAILS");
      ok = ok && worst[b] <= bound[b];
    }
    printf("\n");
    return ok;
  }
};

int main(int argc, char** argv) {
  const long N = argc > 1 ? atol(argv[1]) : 300000;
  const float dt = 1.f / 60.f;
  // measured maxima per branch (h < 1e-5 | 1e-5 <= h < 1 | h >= 1); the bound is 4 x each
  Max m_pos{"(a) root_step: root_pos", B3(M_POS)}, m_rot{"(a) root_step: root_rot", B3(M_ROT)}, m_gaze{"(a) gaze_dir", B3(M_GAZE)},
      m_f64p{"(a) root_step_fp64: root_pos", B3(M_F64P)}, m_f64r{"(a) root_step_fp64: root_rot", B3(M_F64R)},
      m_hu{"(b) half-rotation vector hu", B3(M_HU)}, m_ac{"(b) root_bwd: carry / summands", B3(M_AC)}, m_acw{"(b) root_bwd: carry, well cond.", B3(M_ACW)}, m_ag{"(b) root_bwd: g6", B3(M_AG)}, m_fd{"(c) fp64 adjoint vs differences", B3(M_FD)},
      m_sc{"(d) split: carry / summands", B3(M_SC)}, m_scw{"(d) split: carry, well cond.", B3(M_SCW)}, m_sg{"(d) split vs one piece: g6", B3(M_SG)}, m_gru{"(e) gru_cell_bwd", B3(M_GRU)};
  Max i_exact{"    same vs the fp64 point (info)", {1, 1, 1}, {0, 0, 0}};
  long share[3] = {0, 0, 0}, well[3] = {0, 0, 0};
  double cond[3] = {0, 0, 0};
  for (long n = 0; n < N; ++n) {
    const int br = (int)(n % 3);
    // ---- inputs, rounded to fp32 (both sides see the same numbers)
    float qf[4], posf[3], pf[6], gzf[3], gstd[3];
    {
      double q[4], nq = 0, dir[3], nd = 0;
      for (int i = 0; i < 4; ++i) { q[i] = sym(1); nq += q[i] * q[i]; }
      const double nrm = 1.0 + sym(1e-3), sc = nrm / sqrt(nq);      // the root rotation is never re-normalised: norm 1 +- 1e-3
      for (int i = 0; i < 4; ++i) qf[i] = (float)(q[i] * sc);
      for (int i = 0; i < 3; ++i) { posf[i] = (float)sym(5); pf[i] = (float)sym(3); gzf[i] = posf[i] + (float)sym(5); gstd[i] = (float)(0.2 + 2 * unit()); }
      for (int i = 0; i < 3; ++i) { dir[i] = sym(1); nd += dir[i] * dir[i]; }
      const double h = br == 0 ? logu(1e-8, 5e-6) : br == 1 ? logu(2e-5, 0.99) : logu(1.01, 3.0);
      for (int i = 0; i < 3; ++i) pf[3 + i] = (float)(dir[i] / sqrt(nd) * h * 2 / (nrm * nrm) / dt);      // (|q|^2 scales the rotated vector, nearly)
    }
    const Q4 q = Q4{qf[0], qf[1], qf[2], qf[3]};
    const V3 pos = v3(posf[0], posf[1], posf[2]), gz = v3(gzf[0], gzf[1], gzf[2]);
    double in[13], gzd[3] = {gzf[0], gzf[1], gzf[2]}, out[10];
    for (int i = 0; i < 4; ++i) in[i] = qf[i];
    for (int i = 0; i < 3; ++i) in[4 + i] = posf[i];
    for (int i = 0; i < 6; ++i) in[7 + i] = pf[i];
    r_forward((double)dt, in, gzd, out);
    // ---- (a)
    V3 npos; Q4 nq;
    root_step(dt, q, pos, pf, npos, nq);
    {
      const V3 hu = 0.5f * quat_mul_vec(q, dt * v3(pf[3], pf[4], pf[5]));
      const float h = sqrtf(hu.x * hu.x + hu.y * hu.y + hu.z * hu.z);      // the branch the fp32 code takes
      ++share[h < 1e-5f ? 0 : h < 1.f ? 1 : 2];
    }
    const double gp[3] = {npos.x, npos.y, npos.z}, gq[4] = {nq.w, nq.x, nq.y, nq.z};
    m_pos.add(gp, out, 3, br);
    m_rot.add(gq, out + 3, 4, br);
    {
      // the gaze direction of the fp32 state against float64 FROM THAT STATE (the state's own error is measured above)
      double o2[3];
      const double ql[4] = {nq.w, -nq.x, -nq.y, -nq.z}, d[3] = {gzd[0] - npos.x, gzd[1] - npos.y, gzd[2] - npos.z};
      r_quat_mul_vec(ql, d, o2);
      const V3 gd = gaze_dir(nq, npos, gz);
      const double g3[3] = {gd.x, gd.y, gd.z};
      m_gaze.add(g3, o2, 3, br);
      V3 np64; Q4 nq64;
      root_step_fp64(dt, q, pos, pf, np64, nq64);
      const double a3[3] = {np64.x, np64.y, np64.z}, a4[4] = {nq64.w, nq64.x, nq64.y, nq64.z};
      // (its dt is the fp32 value widened, as here)
      m_f64p.add(a3, out, 3, br);
      m_f64r.add(a4, out + 3, 4, br);
    }
    // ---- upstream gradients.  The adjoint differentiates frame f = the OUTPUT of root_step: (q_t, p_t) below are the float64
    // forward's own outputs rounded to fp32, as the kernels read them back from the saved trajectory
    float grp[3], grr[4], dgd_in[3], g6in[6];
    for (int i = 0; i < 3; ++i) { grp[i] = (float)sym(1); dgd_in[i] = (float)sym(1); }
    for (int i = 0; i < 4; ++i) grr[i] = (float)sym(1);
    for (int i = 0; i < 6; ++i) g6in[i] = (float)sym(1);
    const bool has_next = (n / 3) % 4 != 0;
    double gout[10], gin[13];
    for (int i = 0; i < 3; ++i) { gout[i] = grp[i]; gout[7 + i] = has_next ? (double)dgd_in[i] / (double)gstd[i] : 0.0; }
    for (int i = 0; i < 4; ++i) gout[3 + i] = grr[i];
    const Q4 q_t = Q4{(float)out[3], (float)out[4], (float)out[5], (float)out[6]};
    const V3 p_t = v3((float)out[0], (float)out[1], (float)out[2]);
    a_forward((double)dt, in, gzd, gout, gin);
    double want_carry[7] = {gin[4], gin[5], gin[6], gin[0], gin[1], gin[2], gin[3]}, want_g6[6];
    for (int i = 0; i < 6; ++i) want_g6[i] = g6in[i] + gin[7 + i];
    // ---- (b)
    V3 g_rp = v3(grp[0], grp[1], grp[2]);
    Q4 g_rr = Q4{grr[0], grr[1], grr[2], grr[3]};
    float g6[6];
    for (int i = 0; i < 6; ++i) g6[i] = g6in[i];
    const V3 dgd = v3(dgd_in[0] / gstd[0], dgd_in[1] / gstd[1], dgd_in[2] / gstd[2]);
    root_bwd(dt, q_t, p_t, gz, dgd, has_next, q, v3(pf[0], pf[1], pf[2]), v3(pf[3], pf[4], pf[5]), g_rp, g_rr, g6);
    const double got_carry[7] = {g_rp.x, g_rp.y, g_rp.z, g_rr.w, g_rr.x, g_rr.y, g_rr.z};
    double got_g6[6];
    for (int i = 0; i < 6; ++i) got_g6[i] = g6[i];
    // The carry is a SUM (dq1 + dqy + dq2, gaze term included) whose parts can be far larger than the result, and it is evaluated
    // at the fp32 code's own half-rotation vector hu = quat_mul_vec(q, vrt dt) / 2, which carries the rounding of the forward pass
    // (row "hu"); the curvature of the exponential and the factor |vrt dt| = 2 h of qmv_bwd turn that into an error of the carry
    // that grows like h^2 -- nothing an fp32 adjoint can avoid, and nothing at the h of motion data.  So the adjoint ARITHMETIC is
    // held against the float64 adjoint AT that hu (everything else float64): every case against the size of the summands, and
    // against the carry's own largest entry the cases whose summands are at most WELL x the result (counted; worst ratio printed).
    // The distance to the float64 adjoint at the float64 point is printed for the well-conditioned cases, not asserted.
    const V3 huf = 0.5f * quat_mul_vec(q, dt * v3(pf[3], pf[4], pf[5]));
    const double hud[3] = {huf.x, huf.y, huf.z};
    {
      double w[3] = {in[10] * (double)dt, in[11] * (double)dt, in[12] * (double)dt}, u64[3];
      r_quat_mul_vec(in, w, u64);
      for (int i = 0; i < 3; ++i) u64[i] /= 2;
      m_hu.add(hud, u64, 3, br);
    }
    double gin_m[13];
    const double size = a_forward((double)dt, in, gzd, gout, gin_m, hud);
    const double at_hu[7] = {gin_m[4], gin_m[5], gin_m[6], gin_m[0], gin_m[1], gin_m[2], gin_m[3]};
    double wmax = 0;
    for (int i = 0; i < 7; ++i) wmax = fmax(wmax, fabs(at_hu[i]));
    const bool wellc = size <= WELL * wmax;
    well[br] += wellc;
    cond[br] = fmax(cond[br], size / wmax);
    m_ac.add(got_carry, at_hu, 7, br, size);
    if (wellc) {
      m_acw.add(got_carry, at_hu, 7, br);
      i_exact.add(got_carry, want_carry, 7, br);
    }
    m_ag.add(got_g6, want_g6, 6, br);
    // ---- (c) central differences of L = <gout, forward(in)> in long double, one input at a time
    if (n % 8 < 3) {      // (every branch; an eighth of the cost)
      long double inl[13], gzl[3] = {gzd[0], gzd[1], gzd[2]}, fd[13];
      const double nv = sqrt(in[10] * in[10] + in[11] * in[11] + in[12] * in[12]);
      for (int k = 0; k < 13; ++k) {
        // steps: small against the curvature, and inside the branch (h < 1e-5: the function is linear to 1e-11 there, and
        // h <= 5e-6 + 1e-6 stays below the threshold)
        const long double step = k < 4 ? 1e-6L : k < 7 ? 1e-5L : k < 10 ? 1e-5L : (long double)(1e-5 * nv + (br == 0 ? 1e-6 * 2 / dt : 0.0));
        long double lp = 0, lm = 0, o[10];
        for (int s = 0; s < 2; ++s) {
          for (int i = 0; i < 13; ++i) inl[i] = in[i];
          inl[k] += s ? -step : step;
          r_forward((long double)dt, inl, gzl, o);
          long double l = 0;
          for (int i = 0; i < 10; ++i) l += (long double)gout[i] * o[i];
          (s ? lm : lp) = l;
        }
        fd[k] = (lp - lm) / (2 * step);
      }
      double fdd[13];
      for (int k = 0; k < 13; ++k) fdd[k] = (double)fd[k];
      m_fd.add(gin, fdd, 13, br);
    }
    // ---- (d) the split form: same inputs through RootIn -> root_prepare -> 33 slots -> root_apply (next frame exists)
    if (has_next) {
      RootIn ri;
      const float items[33] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, q_t.w, q_t.x, q_t.y, q_t.z, p_t.x, p_t.y, p_t.z, gzf[0], gzf[1], gzf[2],
                               qf[0], qf[1], qf[2], qf[3], pf[0], pf[1], pf[2], pf[3], pf[4], pf[5],
                               g6in[0], g6in[1], g6in[2], g6in[3], g6in[4], g6in[5]};
      ri.gather([&](int item) { return items[item]; });
      RootPre pre;
      root_prepare(dt, ri, pre);
      float slots[33];
      root_pre_store(pre, [&](int slot, float v) { slots[slot] = v; });
      float cr[7] = {grp[0], grp[1], grp[2], grr[0], grr[1], grr[2], grr[3]}, s6[6];
      const float rstd[3] = {1.f / gstd[0], 1.f / gstd[1], 1.f / gstd[2]};
      for (int i = 0; i < 6; ++i) s6[i] = slots[27 + i];
      root_apply(dt, rstd, [&](int slot) { return slots[slot]; }, dgd_in, cr, s6);
      double sc[7], sg[6];
      for (int i = 0; i < 7; ++i) sc[i] = cr[i];
      for (int i = 0; i < 6; ++i) sg[i] = s6[i];
      m_sc.add(sc, got_carry, 7, br, size);
      if (wellc) m_scw.add(sc, got_carry, 7, br);
      m_sg.add(sg, got_g6, 6, br);
    }
    // ---- (e) GRU cell backward: h' = (1 - z) n + z h, n = tanh(an + r nh), r = sigmoid(ar), z = sigmoid(az)
    {
      struct { float x, y, z, w; } gt = {(float)(0.02 + 0.96 * unit()), (float)(0.02 + 0.96 * unit()), (float)sym(0.98), (float)sym(2)};
      const float g = (float)sym(1), hp = (float)sym(1);
      const GruGrad gg = gru_cell_bwd(g, gt, hp);
      const double r = gt.x, z = gt.y, nn = gt.z, nh = gt.w;
      const double dan = (double)g * (1 - z) * (1 - nn * nn);      // dh'/dn * tanh'
      const double want[5] = {dan * nh * r * (1 - r), (double)g * ((double)hp - nn) * z * (1 - z), dan, dan * r, (double)g * z};
      const double got[5] = {gg.dar, gg.daz, gg.dan, gg.dhn(), gg.dhc()};
      m_gru.add(got, want, 5, br);
    }
  }
  printf("dec_math_check: %ld cases; half-angle branches  h < 1e-5: %.3f   1e-5 <= h < 1: %.3f   h >= 1: %.3f\n", N,
         (double)share[0] / N, (double)share[1] / N, (double)share[2] / N);
  printf("max rel err per branch:               h < 1e-5                       1e-5 <= h < 1                  h >= 1\n");
  bool ok = true;
  for (int b = 0; b < 3; ++b)
    if (share[b] * 10 < N) { printf("  branch %d has less than a tenth of the cases\n", b); ok = false; }
  printf("carry: summands <= %g x result in     %.3f of the cases               %.3f                           %.3f\n", WELL,
         3.0 * well[0] / N, 3.0 * well[1] / N, 3.0 * well[2] / N);
  printf("carry: largest summands / result      %.3g                           %.3g                          %.3g\n", cond[0], cond[1], cond[2]);
  for (int b = 0; b < 3; ++b)
    if (well[b] * 50 < N / 3) { printf("  branch %d: fewer than a fiftieth of its cases are well conditioned\n", b); ok = false; }
  const Max* all[] = {&m_pos, &m_rot, &m_gaze, &m_f64p, &m_f64r, &m_hu, &m_ac, &m_acw, &i_exact, &m_ag, &m_fd, &m_sc, &m_scw, &m_sg, &m_gru};
  for (const Max* m : all) ok = m->report() && ok;
  printf(ok ? "dec_math_check: ok\n" : "dec_math_check: FAILED\n");
  return ok ? 0 : 1;
}
