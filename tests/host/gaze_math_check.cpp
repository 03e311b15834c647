// Stand-alone host program over csrc/gaze_math.h, the header the gaze kernels of live serving evaluate a schedule with
// (tests/test_live_gaze_cpu.py builds and runs it, once plain and once under the address and undefined-behaviour sanitizers, and
// compares every row of the table it prints with the float64 oracle tests/live_gaze_oracle.py).  It walks:
//   - weights for fade 0, 1 and 12 with frames before, inside and after the fade, both eases, on the line;
//   - the arc at 1, 90 and 179 degrees, at equal and at unequal distances, over a whole fade, both eases;
//   - each fallback of the arc: the same direction, the opposite direction, a target on the pivot, a start on the pivot;
//   - root-space resolution with stored quaternions that are not of unit length;
//   - a second set in the middle of a fade (in root space, with and without a pivot of its own), and the frames around it.
// Rows (every float is a float32 printed with 9 significant digits, which reads back exactly):
//   point <name> <start 3> <end 3> <pivot 3> <path> <ease> <k> <fade> <f> | <x y z>
//   resolve <name> <rpos 3> <rrot 4> <p 3> | <x y z>
//   apply <name> <old: start 3, end 3, pivot 3, path, ease, k, fade> <k> <fade> <space> <path> <ease> <has_pivot> <target 3> <pivot 3>
//         <rpos 3> <rrot 4> | <start 3> <end 3> <pivot 3>
// and the properties it checks itself: the line begins at the start and ends at the end exactly, the weight is 0 up to frame
// k - 1 and 1 from frame k + fade on, and the smooth ease keeps both ends.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../ubisoft-laforge-zeroeggs_amd/csrc/gaze_math.h"

static int failures = 0;
#define EXPECT(cond, ...)              \
  do {                                 \
    if (!(cond)) {                     \
      ++failures;                      \
      printf("FAILED: " __VA_ARGS__);  \
      printf("\n");                    \
    }                                  \
  } while (0)

static void print3(const float* v) { printf(" %.9g %.9g %.9g", (double)v[0], (double)v[1], (double)v[2]); }

static GazeRow schedule(const float* s, const float* e, const float* c, int path, int ease, long k, long fade) {
  GazeRow g;
  for (int i = 0; i < 3; ++i) { g.start[i] = s[i]; g.end[i] = e[i]; g.pivot[i] = c[i]; }
  g.path = path; g.ease = ease; g.pad = 0; g.k = k; g.fade = fade;
  return g;
}

static void point_row(const char* name, const GazeRow& g, long f) {
  double p[3];
  gaze_eval(g, f, p);
  const float out[3] = {(float)p[0], (float)p[1], (float)p[2]};
  printf("point %s", name);
  print3(g.start); print3(g.end); print3(g.pivot);
  printf(" %d %d %ld %ld %ld |", g.path, g.ease, g.k, g.fade, f);
  print3(out);
  printf("\n");
}

static void resolve_row(const char* name, const float* rpos, const float* rrot, const float* p) {
  double w[3];
  gaze_resolve(rpos, rrot, p, w);
  const float out[3] = {(float)w[0], (float)w[1], (float)w[2]};
  printf("resolve %s", name);
  print3(rpos);
  printf(" %.9g %.9g %.9g %.9g", (double)rrot[0], (double)rrot[1], (double)rrot[2], (double)rrot[3]);
  print3(p);
  printf(" |");
  print3(out);
  printf("\n");
}

static GazeRow apply_row(const char* name, GazeRow g, long k, long fade, int space, int path, int ease, int has_pivot, const float* target,
                         const float* pivot, const float* rpos, const float* rrot) {
  printf("apply %s", name);
  print3(g.start); print3(g.end); print3(g.pivot);
  printf(" %d %d %ld %ld", g.path, g.ease, g.k, g.fade);
  printf(" %ld %ld %d %d %d %d", k, fade, space, path, ease, has_pivot);
  print3(target); print3(pivot); print3(rpos);
  printf(" %.9g %.9g %.9g %.9g |", (double)rrot[0], (double)rrot[1], (double)rrot[2], (double)rrot[3]);
  gaze_apply(&g, target, pivot, has_pivot, space, path, ease, k, fade, rpos, rrot);
  print3(g.start); print3(g.end); print3(g.pivot);
  printf("\n");
  EXPECT(g.k == k && g.fade == fade && g.path == path && g.ease == ease, "apply %s: the schedule's own fields", name);
  return g;
}

// b = the direction of a turned by `deg` degrees about the axis (0.2, 1, -0.3) normalised (Rodrigues), at length `len`
static void turned(const float* a, double deg, double len, const float* pivot, float* out) {
  const double ax[3] = {0.2, 1.0, -0.3}, an = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  const double n[3] = {ax[0] / an, ax[1] / an, ax[2] / an};
  // the part of a perpendicular to the axis is what turns; start from a direction perpendicular to it
  double d[3] = {a[0], a[1], a[2]};
  const double along = d[0] * n[0] + d[1] * n[1] + d[2] * n[2];
  for (int i = 0; i < 3; ++i) d[i] -= along * n[i];
  const double dl = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  for (int i = 0; i < 3; ++i) d[i] /= dl;
  const double t = deg * 3.14159265358979323846 / 180.0, c = cos(t), s = sin(t);
  const double x[3] = {n[1] * d[2] - n[2] * d[1], n[2] * d[0] - n[0] * d[2], n[0] * d[1] - n[1] * d[0]};
  for (int i = 0; i < 3; ++i) out[i] = (float)((double)pivot[i] + len * (c * d[i] + s * x[i]));
}

int main() {
  const float S[3] = {1.25f, 1.6f, 3.0f}, E[3] = {-2.0f, 0.5f, 4.25f}, Z[3] = {0.f, 0.f, 0.f};
  char name[96];
  // ---- weights, eases, the line
  const long fades[3] = {0, 1, 12};
  for (int fi = 0; fi < 3; ++fi)
    for (int ease = 0; ease < 2; ++ease) {
      const long k = 7, fade = fades[fi];
      const GazeRow g = schedule(S, E, Z, GAZE_LINE, ease, k, fade);
      const long frames[8] = {0, k - 2, k - 1, k, k + fade / 2, k + fade - 1, k + fade, k + fade + 3};
      for (int j = 0; j < 8; ++j) {
        snprintf(name, sizeof name, "line_fade%ld_ease%d", fade, ease);
        point_row(name, g, frames[j]);
        const double w = gaze_ease(gaze_fade_weight(frames[j], k, fade), ease);
        EXPECT(w >= 0.0 && w <= 1.0, "weight %g outside [0, 1]", w);
        if (frames[j] <= k - 1) EXPECT(w == 0.0, "frame %ld before k: weight %g", frames[j], w);
        if (frames[j] >= k + fade) EXPECT(w == 1.0, "frame %ld after the fade: weight %g", frames[j], w);
        double p[3];
        gaze_eval(g, frames[j], p);
        if (w == 0.0) EXPECT((float)p[0] == S[0] && (float)p[1] == S[1] && (float)p[2] == S[2], "the line does not begin at its start");
        if (w == 1.0) EXPECT((float)p[0] == E[0] && (float)p[1] == E[1] && (float)p[2] == E[2], "the line does not end at its end");
      }
    }
  EXPECT(gaze_fade_weight(9, 7, 12) == 3.0 / 13.0, "the weight of frame 9 in a fade of 12 from 7");
  EXPECT(gaze_ease(0.5, GAZE_SMOOTH) == 0.5 && gaze_ease(0.25, GAZE_SMOOTH) == 0.15625, "the smooth ease");
  // ---- the arc
  const float C[3] = {0.1f, 1.5f, -0.2f};
  const double degs[3] = {1.0, 90.0, 179.0}, lens[2][2] = {{2.0, 2.0}, {1.5, 4.0}};
  for (int di = 0; di < 3; ++di)
    for (int li = 0; li < 2; ++li)
      for (int ease = 0; ease < 2; ++ease) {
        float a[3], b[3];
        const float dir[3] = {1.0f, 0.3f, 0.5f};
        turned(dir, 0.0, lens[li][0], C, a);
        turned(dir, degs[di], lens[li][1], C, b);
        const GazeRow g = schedule(a, b, C, GAZE_ARC, ease, 20, 12);
        snprintf(name, sizeof name, "arc_%gdeg_len%d_ease%d", degs[di], li, ease);
        for (long f = 18; f <= 34; ++f) point_row(name, g, f);
        // the distance from the pivot goes on a line
        double p[3];
        gaze_eval(g, 26, p);
        const double w = gaze_ease(gaze_fade_weight(26, 20, 12), ease);
        const double r = sqrt((p[0] - C[0]) * (p[0] - C[0]) + (p[1] - C[1]) * (p[1] - C[1]) + (p[2] - C[2]) * (p[2] - C[2]));
        EXPECT(fabs(r - ((1.0 - w) * lens[li][0] + w * lens[li][1])) < 1e-5, "%s: distance %g from the pivot", name, r);
      }
  // ---- the fallbacks
  {
    float a[3], same[3], opposite[3];
    const float dir[3] = {1.0f, 0.3f, 0.5f};
    turned(dir, 0.0, 2.0, C, a);
    for (int i = 0; i < 3; ++i) { same[i] = C[i] + 2.0f * (a[i] - C[i]); opposite[i] = C[i] - (a[i] - C[i]); }
    const GazeRow gs = schedule(a, same, C, GAZE_ARC, GAZE_LINEAR, 5, 12), go = schedule(a, opposite, C, GAZE_ARC, GAZE_SMOOTH, 5, 12);
    const GazeRow gt = schedule(a, C, C, GAZE_ARC, GAZE_LINEAR, 5, 12), gp = schedule(C, a, C, GAZE_ARC, GAZE_LINEAR, 5, 12);
    for (long f = 4; f <= 18; f += 2) {
      point_row("fallback_same_direction", gs, f);
      point_row("fallback_opposite_direction", go, f);
      point_row("fallback_target_on_pivot", gt, f);
      point_row("fallback_start_on_pivot", gp, f);
    }
  }
  // ---- root-space resolution, the quaternion as stored
  {
    const float rp[3] = {0.4f, 0.0f, -1.3f}, p[3] = {0.3f, 1.6f, 2.5f};
    const float q1[4] = {0.9f, 0.3f, -0.2f, 0.4f}, q2[4] = {1.0f, 0.f, 0.f, 0.f}, q3[4] = {0.70710677f, 0.f, 0.70710677f, 0.f},
                q4[4] = {-0.31f, 0.52f, 0.77f, -0.12f};
    resolve_row("not_unit_length", rp, q1, p);
    resolve_row("identity", rp, q2, p);
    resolve_row("quarter_turn_about_y", rp, q3, p);
    resolve_row("negative_w_not_unit", rp, q4, p);
    double w[3];
    gaze_resolve(rp, q2, p, w);
    EXPECT(w[0] == (double)rp[0] + (double)p[0] && w[1] == (double)rp[1] + (double)p[1], "the identity rotation moves the point");
  }
  // ---- sets: the first on a fresh row, the second in the middle of the first one's fade (root space, the root's own pivot),
  // a third with a pivot of its own, a fourth back in world space on the line
  {
    const float rp[3] = {0.4f, 0.0f, -1.3f}, rq[4] = {0.88f, 0.05f, -0.43f, 0.11f}, none[3] = {0.f, 0.f, 0.f};
    const float t1[3] = {-1.5f, 1.7f, 2.0f}, c1[3] = {0.0f, 1.5f, 0.0f}, t2[3] = {0.6f, 1.55f, 3.0f}, t3[3] = {-0.7f, 1.2f, 2.2f},
                c3[3] = {0.0f, 1.45f, 0.1f}, t4[3] = {2.0f, 1.0f, 1.0f};
    GazeRow g = schedule(S, S, Z, GAZE_LINE, GAZE_LINEAR, 0, 0);
    g = apply_row("first_world_arc", g, 10, 12, GAZE_WORLD, GAZE_ARC, GAZE_SMOOTH, 1, t1, c1, none, rq);
    for (long f = 9; f <= 16; ++f) point_row("after_first", g, f);
    g = apply_row("second_in_the_fade_root_arc", g, 16, 5, GAZE_ROOT, GAZE_ARC, GAZE_LINEAR, 0, t2, none, rp, rq);
    for (long f = 15; f <= 23; ++f) point_row("after_second", g, f);
    g = apply_row("third_in_the_fade_root_pivot", g, 19, 12, GAZE_ROOT, GAZE_ARC, GAZE_SMOOTH, 1, t3, c3, rp, rq);
    for (long f = 18; f <= 32; f += 2) point_row("after_third", g, f);
    g = apply_row("fourth_world_line_step", g, 25, 0, GAZE_WORLD, GAZE_LINE, GAZE_LINEAR, 0, t4, none, rp, rq);
    for (long f = 24; f <= 26; ++f) point_row("after_fourth", g, f);
    EXPECT(g.end[0] == t4[0] && g.end[1] == t4[1] && g.end[2] == t4[2], "a world-space target is stored as it is");
  }
  if (failures) {
    printf("gaze_math_check: %d FAILED\n", failures);
    return 1;
  }
  printf("gaze_math_check: ok\n");
  return 0;
}
