// The gaze schedule of a live row (live_gaze.hip; include/zeggs_hip_gaze.h; the definition is DESIGN.md 3.7), stated once: the
// weight of a frame and its ease, the line and the arc with its fallback, the resolution of a root-space point with a row's
// root state, and what a `set` makes of a row's schedule.  Plain C++ behind a qualifier macro (no HIP include), so the same
// text runs in the kernels, in the host side of live_gaze.hip (zeggs_live_gaze_read) and in tests/host/gaze_math_check.cpp.
// Everything is float64 arithmetic over the float32 state; a value becomes float32 once, where it is stored.
#pragma once
#include <math.h>

#ifndef ZG_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZG_HD __host__ __device__ __forceinline__
#else
#define ZG_HD inline
#endif
#endif

#define GAZE_ROW_BYTES 64
#define GAZE_WORLD 0
#define GAZE_ROOT 1
#define GAZE_LINE 0
#define GAZE_ARC 1
#define GAZE_LINEAR 0
#define GAZE_SMOOTH 1
#define GAZE_EPS 1e-6             // below it a distance or the sine of the angle is no direction: the arc is the line

struct GazeRow {                  // a row's schedule: GAZE_ROW_BYTES bytes of the state block
  float start[3], end[3], pivot[3];
  int path, ease, pad;
  long k, fade;                   // P(w(f)): w = 0 up to frame k - 1, 1 from frame k + fade on
};
static_assert(sizeof(GazeRow) == GAZE_ROW_BYTES, "GazeRow");

// weight of the schedule's end at frame f: style_weight() of zeggs/live.py, the same float64 operations
ZG_HD double gaze_fade_weight(long f, long k, long fade) {
  const double w = (double)(f - k + 1) / ((double)fade + 1.0);
  return w < 0.0 ? 0.0 : w > 1.0 ? 1.0 : w;
}
ZG_HD double gaze_ease(double w, int ease) { return ease == GAZE_SMOOTH ? w * w * (3.0 - 2.0 * w) : w; }

// P(w) of a schedule -> out[3]
ZG_HD void gaze_point(const float* start, const float* end, const float* pivot, int path, double w, double* out) {
  const double p0[3] = {(double)start[0], (double)start[1], (double)start[2]};
  const double p1[3] = {(double)end[0], (double)end[1], (double)end[2]};
  if (path == GAZE_ARC) {
    const double c[3] = {(double)pivot[0], (double)pivot[1], (double)pivot[2]};
    const double a[3] = {p0[0] - c[0], p0[1] - c[1], p0[2] - c[2]}, b[3] = {p1[0] - c[0], p1[1] - c[1], p1[2] - c[2]};
    const double la = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), lb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    if (la >= GAZE_EPS && lb >= GAZE_EPS) {
      const double u[3] = {a[0] / la, a[1] / la, a[2] / la}, v[3] = {b[0] / lb, b[1] / lb, b[2] / lb};
      const double x[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
      const double s = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
      if (s >= GAZE_EPS) {
        const double theta = atan2(s, u[0] * v[0] + u[1] * v[1] + u[2] * v[2]);
        const double r = (1.0 - w) * la + w * lb, su = sin((1.0 - w) * theta), sv = sin(w * theta);
        out[0] = c[0] + r * (su * u[0] + sv * v[0]) / s;
        out[1] = c[1] + r * (su * u[1] + sv * v[1]) / s;
        out[2] = c[2] + r * (su * u[2] + sv * v[2]) / s;
        return;
      }
    }
  }
  out[0] = (1.0 - w) * p0[0] + w * p1[0];
  out[1] = (1.0 - w) * p0[1] + w * p1[1];
  out[2] = (1.0 - w) * p0[2] + w * p1[2];
}

// what frame f of row schedule g looks at -> out[3]
ZG_HD void gaze_eval(const GazeRow& g, long f, double* out) {
  gaze_point(g.start, g.end, g.pivot, g.path, gaze_ease(gaze_fade_weight(f, g.k, g.fade), g.ease), out);
}

// a point p of the character's root frame in the model's world: rpos + rrot (x) p, the quaternion (w first) as stored --
// quat_math.h's quat_mul_vec: t = 2 (q_v x p); p + w t + q_v x t
ZG_HD void gaze_resolve(const float* rpos, const float* rrot, const float* p, double* out) {
  const double qw = (double)rrot[0], qx = (double)rrot[1], qy = (double)rrot[2], qz = (double)rrot[3];
  const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
  const double tx = 2.0 * (qy * pz - qz * py), ty = 2.0 * (qz * px - qx * pz), tz = 2.0 * (qx * py - qy * px);
  out[0] = (double)rpos[0] + (px + qw * tx + (qy * tz - qz * ty));
  out[1] = (double)rpos[1] + (py + qw * ty + (qz * tx - qx * tz));
  out[2] = (double)rpos[2] + (pz + qw * tz + (qx * ty - qy * tx));
}

// a `set` on row schedule g: from frame k on, over `fade` frames, towards `target`.  The new start is the old schedule at frame
// k - 1; a root-space target / pivot is resolved with rpos[3] / rrot[4], and without a pivot of its own the pivot is rpos.
ZG_HD void gaze_apply(GazeRow* g, const float* target, const float* pivot, int has_pivot, int space, int path, int ease, long k,
                      long fade, const float* rpos, const float* rrot) {
  double p0[3], p1[3] = {(double)target[0], (double)target[1], (double)target[2]}, c[3] = {0.0, 0.0, 0.0};
  gaze_eval(*g, k - 1, p0);
  if (has_pivot) { c[0] = (double)pivot[0]; c[1] = (double)pivot[1]; c[2] = (double)pivot[2]; }
  if (space == GAZE_ROOT) {
    gaze_resolve(rpos, rrot, target, p1);
    if (has_pivot) gaze_resolve(rpos, rrot, pivot, c);
    else { c[0] = (double)rpos[0]; c[1] = (double)rpos[1]; c[2] = (double)rpos[2]; }
  }
  for (int i = 0; i < 3; ++i) {
    g->start[i] = (float)p0[i];
    g->end[i] = (float)p1[i];
    g->pivot[i] = (float)c[i];
  }
  g->path = path; g->ease = ease; g->pad = 0;
  g->k = k; g->fade = fade;
}

// weight of the NEW style at frame f, as float32: what the host's style_weight() rows were uploaded as
ZG_HD float gaze_style_weight(long f, long k_style, long fade_style) { return (float)gaze_fade_weight(f, k_style, fade_style); }
// torch.lerp's float32 formula
ZG_HD float gaze_style_lerp(float a, float b, float w) {
  const float d = b - a;
  return w < 0.5f ? a + w * d : b - d * (1.0f - w);
}
