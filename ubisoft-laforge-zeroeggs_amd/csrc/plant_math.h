// The planting stage of live serving (live_plant.hip; include/zeggs_hip_plant.h; the definition is DESIGN.md 3.7), stated once:
// the layout of the state, the contact state machine of a leg chain with its hysteresis and its fade, the reach limit and the
// analytic two-bone solve.  Plain C++ behind a qualifier macro (no HIP include), so the same text runs in the kernel, in the host
// side of live_plant.hip and in tests/host/plant_math_check.cpp.  Everything is float64; a rotation becomes float32 once, where
// its two columns are stored.
//
// A chain is three joints (u, m, e): upper leg, lower leg, foot, parents[m] == u and parents[e] == m.  Per model frame the
// kernel runs FK over the ancestors of e from the RAW row (dq_from_xy of anim_math.h, the root folded into joint 0; the root's
// rotation and every local rotation brought to unit length first: the float32 root is unit to 1e-7 only) and hands
// this header the unconstrained world points H (joint u), K (joint m), A (joint e), the world rotation of u's parent and the
// local rotations of u, m, e.  Per frame and chain (pl_step):
//   1. s = |A - a_prev| / dt (0 on the stream's first frame), y = A.y - ground;
//   2. e_off = o0 g(k / N), N = release, g(x) = 1 - x^2 (3 - 2 x) below 1 and 0 from 1 on; 0 when N == 0;
//   3. at most one transition: HELD and (s > v_off or y > h_off or |A - L| > slack) -> FREE, o0 = L - A, k = 0, e_off again
//      (now o0: the target stays where it was); else FREE and s <= v_on and y <= h_on -> HELD, L = A + e_off;
//   4. T = L when HELD, else A + e_off and k = min(k + 1, N);
//   5. l1 = |K - H|, l2 = |A - K|: a T with |T - H| > stretch (l1 + l2) is pulled onto that sphere along T - H;
//   8. a_prev = A; the frame's contact flag is mode == HELD.
// A frame whose T equals A keeps its three joints as they are (6.); any other goes through pl_solve (7.):
//   the interior angles at H and K before (dot products of normalised differences, clamped to [-1, 1]) and those the cosine rule
//   gives for |T - H| clamped to [PL_EPS, stretch (l1 + l2)]; the bend axis normalise((A - H) x (K - H)) -- below PL_EPS the
//   root's forward axis crossed with A - H --, the swing axis normalise((A - H) x (T - H)) -- below PL_EPS: no swing --, each
//   expressed in the frame of the joint it turns:
//     u.lrot <- u.lrot R(bend, d_H) R(swing, angle(A - H, T - H)),  m.lrot <- m.lrot R(bend, d_K),  e.lrot <- inv(m.world') e.world
//   with angle(a, t) = atan2(|a x t|, a . t), which keeps its precision for a T that is almost on the line through H and A
//   (the swing axis in u's frame AFTER the bend, so that in the world the bend comes first and the swing carries the bent leg
//   onto T - H: the solved ankle is T).  Bone lengths, lpos and H are untouched, the foot keeps its world rotation.
#pragma once
#include <math.h>

#ifndef ZP_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZP_HD __host__ __device__ __forceinline__
#else
#define ZP_HD inline
#endif
#endif

#define PL_MAX_CHAINS 4
#define PL_FREE 0
#define PL_HELD 1
#define PL_EPS 1e-8               // below it a length or a cross product is no direction
#define PL_THREADS 256            // threads of a workgroup (one workgroup per record)
#define PL_PASS_FRAMES 32         // frames a workgroup stages at a time
#define PL_SLOT 21                // doubles staged per (frame, chain): H 3 | K 3 | A 3 | parent rotation 4 | root rotation 4 | T 3 | solve 1
#define PL_MAX_JOINTS 1024
#define PL_MAX_FRAMES 4096        // frames of one record
#define PL_MAX_RELEASE 4096

struct PlV { double x, y, z; };
struct PlQ { double w, x, y, z; };

struct PlantOpts {                // the numbers of ZeggsPlantDims the arithmetic reads
  double dt, v_on, v_off, h_on, h_off, ground, slack, stretch;
  int release;
};

struct PlantChain {               // the state of one chain of one row
  double L[3], o0[3], a_prev[3];  // the held point | the offset at release | the unconstrained ankle of the previous frame
  int mode, started, k, pad;      // PL_FREE / PL_HELD | the stream has had a frame | frames since release (<= release)
};
static_assert(sizeof(PlantChain) == 88, "PlantChain");

// ---- the state: [parents int[J] | chain table int[PL_MAX_CHAINS][3], padded to 8 bytes] then per row PL_MAX_CHAINS PlantChain
ZP_HD long pl_tables_bytes(int J) { return ((long)(J + 3 * PL_MAX_CHAINS) * 4 + 7) / 8 * 8; }
ZP_HD long pl_row_bytes() { return (long)PL_MAX_CHAINS * (long)sizeof(PlantChain); }
ZP_HD long pl_state_bytes(int rows, int J) { return pl_tables_bytes(J) + (long)rows * pl_row_bytes(); }
ZP_HD long pl_row_offset(int J, int row) { return pl_tables_bytes(J) + (long)row * pl_row_bytes(); }
// a pose row of the decoder: root_vel 3 | root_vrt 3 | lpos 3J | ltxy 6J | lvel 3J | lvrt 3J
ZP_HD int pl_pose_floats(int J) { return 6 + 15 * J; }
ZP_HD int pl_pose_lpos(int j) { return 6 + 3 * j; }
ZP_HD int pl_pose_ltxy(int J, int j) { return 6 + 3 * J + 6 * j; }

// what the entry points take: 0, or the reason
ZP_HD int pl_dims_refused(int rows, int max_rows, int J, int max_frames, int chains, int release) {
  if (rows < 1 || rows > max_rows) return 1;
  if (J < 3 || J > PL_MAX_JOINTS) return 2;
  if (max_frames < 1 || max_frames > PL_MAX_FRAMES) return 3;
  if (chains < 1 || chains > PL_MAX_CHAINS) return 4;
  if (release < 0 || release > PL_MAX_RELEASE) return 5;
  return 0;
}
ZP_HD int pl_opts_refused(const PlantOpts& o) {
  if (!(o.dt > 0.0) || !isfinite(o.dt)) return 1;
  if (!(o.v_on >= 0.0) || !(o.v_on <= o.v_off) || !isfinite(o.v_off)) return 2;
  if (!(o.h_on <= o.h_off) || !isfinite(o.h_on) || !isfinite(o.h_off)) return 3;
  if (!isfinite(o.ground)) return 4;
  if (!(o.slack >= 0.0) || !isfinite(o.slack)) return 5;
  if (!(o.stretch > 0.0) || !(o.stretch <= 1.0)) return 6;
  return 0;
}
// the chain table against the parents: -1, or the first chain that is refused (why: 1 an index out of range, 2 parents[m] != u
// or parents[e] != m, 3 a joint that another chain has)
ZP_HD int pl_bad_chain(const int* parents, int J, const int* chains, int C, int* why) {
  for (int c = 0; c < C; ++c) {
    const int u = chains[3 * c], m = chains[3 * c + 1], e = chains[3 * c + 2];
    *why = 1;
    if (u < 0 || u >= J || m < 0 || m >= J || e < 0 || e >= J) return c;
    *why = 2;
    if (parents[m] != u || parents[e] != m) return c;
    *why = 3;
    for (int i = 0; i < 3 * c; ++i)
      if (chains[i] == u || chains[i] == m || chains[i] == e) return c;
  }
  *why = 0;
  return -1;
}

// ---- vectors and quaternions (w first)
ZP_HD PlV pl_add(PlV a, PlV b) { return PlV{a.x + b.x, a.y + b.y, a.z + b.z}; }
ZP_HD PlV pl_sub(PlV a, PlV b) { return PlV{a.x - b.x, a.y - b.y, a.z - b.z}; }
ZP_HD PlV pl_scale(double s, PlV a) { return PlV{s * a.x, s * a.y, s * a.z}; }
ZP_HD double pl_dot(PlV a, PlV b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
ZP_HD double pl_len(PlV a) { return sqrt(pl_dot(a, a)); }
ZP_HD PlV pl_cross(PlV a, PlV b) { return PlV{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
ZP_HD PlQ pl_inv(PlQ q) { return PlQ{q.w, -q.x, -q.y, -q.z}; }
ZP_HD PlQ pl_mul(PlQ a, PlQ b) {
  return PlQ{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + b.w * a.x + (a.y * b.z - a.z * b.y),
             a.w * b.y + b.w * a.y + (a.z * b.x - a.x * b.z), a.w * b.z + b.w * a.z + (a.x * b.y - a.y * b.x)};
}
ZP_HD PlV pl_rot(PlQ q, PlV v) {
  const PlV qv = PlV{q.x, q.y, q.z};
  const PlV t = pl_scale(2.0, pl_cross(qv, v));
  return pl_add(pl_add(v, pl_scale(q.w, t)), pl_cross(qv, t));
}
ZP_HD PlQ pl_axis_angle(PlV axis, double angle) {      // `axis` of unit length
  const double h = 0.5 * angle, s = sin(h);
  return PlQ{cos(h), s * axis.x, s * axis.y, s * axis.z};
}
ZP_HD double pl_clamp(double x, double lo, double hi) { return x < lo ? lo : x > hi ? hi : x; }
// angle between two directions: the dot product of the normalised vectors, clamped to [-1, 1]
ZP_HD double pl_angle(PlV a, PlV b) { return acos(pl_clamp(pl_dot(pl_scale(1.0 / pl_len(a), a), pl_scale(1.0 / pl_len(b), b)), -1.0, 1.0)); }
// the two-axis encoding of a rotation: the first two columns of the matrix of q / |q|
ZP_HD void pl_to_xy(PlQ q, double* xy) {
  const double n = 1.0 / sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  const double w = n * q.w, x = n * q.x, y = n * q.y, z = n * q.z;
  xy[0] = 1.0 - 2.0 * (y * y + z * z); xy[1] = 2.0 * (x * y + w * z); xy[2] = 2.0 * (x * z - w * y);
  xy[3] = 2.0 * (x * y - w * z); xy[4] = 1.0 - 2.0 * (x * x + z * z); xy[5] = 2.0 * (y * z + w * x);
}

// ---- the fade of a released offset
ZP_HD double pl_fade(int k, int N) {
  if (N <= 0 || k >= N) return 0.0;
  const double x = (double)k / (double)N;
  return 1.0 - x * x * (3.0 - 2.0 * x);
}

// ---- steps 1 - 5 and 8 of a frame: the chain's state moves on, T is the frame's target -> the contact flag
ZP_HD int pl_step(const PlantOpts& o, PlantChain& s, PlV H, PlV K, PlV A, PlV& T) {
  const PlV prev = PlV{s.a_prev[0], s.a_prev[1], s.a_prev[2]};
  const double speed = s.started ? pl_len(pl_sub(A, prev)) / o.dt : 0.0;
  const double y = A.y - o.ground;
  PlV L = PlV{s.L[0], s.L[1], s.L[2]}, o0 = PlV{s.o0[0], s.o0[1], s.o0[2]};
  PlV off = pl_scale(pl_fade(s.k, o.release), o0);
  if (s.mode == PL_HELD) {
    if (speed > o.v_off || y > o.h_off || pl_len(pl_sub(A, L)) > o.slack) {
      s.mode = PL_FREE;
      o0 = pl_sub(L, A);
      s.k = 0;
      off = pl_scale(pl_fade(0, o.release), o0);
    }
  } else if (speed <= o.v_on && y <= o.h_on) {
    s.mode = PL_HELD;
    L = pl_add(A, off);
  }
  if (s.mode == PL_HELD) {
    T = L;
  } else {
    T = pl_add(A, off);
    s.k = s.k + 1 < o.release ? s.k + 1 : o.release;
  }
  const double reach = o.stretch * (pl_len(pl_sub(K, H)) + pl_len(pl_sub(A, K)));
  const PlV d = pl_sub(T, H);
  const double dist = pl_len(d);
  if (dist > reach) T = pl_add(H, pl_scale(reach / dist, d));
  s.L[0] = L.x; s.L[1] = L.y; s.L[2] = L.z;
  s.o0[0] = o0.x; s.o0[1] = o0.y; s.o0[2] = o0.z;
  s.a_prev[0] = A.x; s.a_prev[1] = A.y; s.a_prev[2] = A.z;
  s.started = 1;
  return s.mode == PL_HELD;
}
// step 6: a target that is the unconstrained ankle changes nothing
ZP_HD bool pl_same(PlV T, PlV A) { return T.x == A.x && T.y == A.y && T.z == A.z; }

// ---- step 7: the new local rotations of u, m, e.  gp: the world rotation of u's parent (the placed root for a u that is joint 0),
// root: the root's rotation (its forward axis is the bend axis of a straight leg), qu / qm / qe: the local rotations as they are
ZP_HD void pl_solve(double stretch, PlV H, PlV K, PlV A, PlV T, PlQ gp, PlQ root, PlQ& qu, PlQ& qm, PlQ& qe) {
  const PlQ gu = pl_mul(gp, qu), gm = pl_mul(gu, qm), ge = pl_mul(gm, qe);
  const PlV ab = pl_sub(K, H), ac = pl_sub(A, H), cb = pl_sub(K, A), at = pl_sub(T, H);
  const double l1 = pl_len(ab), l2 = pl_len(cb);
  const double lat = pl_clamp(pl_len(at), PL_EPS, stretch * (l1 + l2));
  const double h0 = pl_angle(ac, ab), k0 = pl_angle(pl_sub(H, K), pl_sub(A, K));
  const double h1 = acos(pl_clamp((l2 * l2 - l1 * l1 - lat * lat) / (-2.0 * l1 * lat), -1.0, 1.0));
  const double k1 = acos(pl_clamp((lat * lat - l1 * l1 - l2 * l2) / (-2.0 * l1 * l2), -1.0, 1.0));
  PlV bend = pl_cross(ac, ab);
  if (pl_len(bend) < PL_EPS) bend = pl_cross(pl_rot(root, PlV{0.0, 0.0, 1.0}), ac);
  const double nb = pl_len(bend);
  bend = nb > 0.0 ? pl_scale(1.0 / nb, bend) : PlV{1.0, 0.0, 0.0};
  const PlQ ru = pl_axis_angle(pl_rot(pl_inv(gu), bend), h1 - h0);
  const PlQ rm = pl_axis_angle(pl_rot(pl_inv(gm), bend), k1 - k0);
  PlQ nu = pl_mul(qu, ru);
  const PlV swing = pl_cross(ac, at);
  const double ns = pl_len(swing);
  if (ns >= PL_EPS) {
    const PlQ gub = pl_mul(gp, nu);      // u's world rotation after the bend: the swing axis in THAT frame
    nu = pl_mul(nu, pl_axis_angle(pl_rot(pl_inv(gub), pl_scale(1.0 / ns, swing)), atan2(ns, pl_dot(ac, at))));
  }
  const PlQ nm = pl_mul(qm, rm);
  const PlQ gm2 = pl_mul(pl_mul(gp, nu), nm);
  qu = nu;
  qm = nm;
  qe = pl_mul(pl_inv(gm2), ge);
}
