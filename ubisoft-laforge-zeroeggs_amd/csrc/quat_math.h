// 3-vectors and quaternions (w, x, y, z) of the animation math, forward and analytic backward: plain C++ behind a qualifier
// macro (no HIP include), so the same text runs in the kernels and in tests/host/dec_math_check.cpp on the host.
#pragma once

#ifndef ZQ_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZQ_HD __host__ __device__ __forceinline__
#else
#define ZQ_HD inline
#endif
#endif

struct V3 {
  float x, y, z;
};
ZQ_HD V3 v3(float x, float y, float z) { return V3{x, y, z}; }
ZQ_HD V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
ZQ_HD V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
ZQ_HD V3 operator*(float s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
ZQ_HD V3 cross(V3 a, V3 b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
ZQ_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
struct Q4 {
  float w, x, y, z;
};
// reference anim/tquat.py:18-20: t = 2 (q_v x v); v + w t + q_v x t
ZQ_HD V3 quat_mul_vec(Q4 q, V3 v) {
  V3 qv = v3(q.x, q.y, q.z);
  V3 t = 2.0f * cross(qv, v);
  return v + q.w * t + cross(qv, t);
}
ZQ_HD Q4 quat_inv(Q4 q) { return Q4{q.w, -q.x, -q.y, -q.z}; }
// reference anim/tquat.py:6-15
ZQ_HD Q4 quat_mul(Q4 x, Q4 y) {
  return Q4{y.w * x.w - y.x * x.x - y.y * x.y - y.z * x.z,
            y.w * x.x + y.x * x.w - y.y * x.z + y.z * x.y,
            y.w * x.y + y.x * x.z + y.y * x.w - y.z * x.x,
            y.w * x.z - y.x * x.y + y.y * x.x + y.z * x.w};
}

// backward of out = quat_mul_vec(q, v) given upstream g
ZQ_HD void qmv_bwd(Q4 q, V3 v, V3 g, Q4& dq, V3& dv) {
  V3 qv = v3(q.x, q.y, q.z);
  V3 t = 2.0f * cross(qv, v);
  float dw = dot(g, t);
  V3 dt = q.w * g + cross(g, qv);
  V3 dqv = cross(t, g) + 2.0f * cross(v, dt);
  dv = g + 2.0f * cross(dt, qv);
  dq = Q4{dw, dqv.x, dqv.y, dqv.z};
}
// backward of out = quat_mul(x, y)
ZQ_HD void qmul_bwd(Q4 x, Q4 y, Q4 g, Q4& dx, Q4& dy) {
  dx.w = g.w * y.w + g.x * y.x + g.y * y.y + g.z * y.z;
  dx.x = -g.w * y.x + g.x * y.w - g.y * y.z + g.z * y.y;
  dx.y = -g.w * y.y + g.x * y.z + g.y * y.w - g.z * y.x;
  dx.z = -g.w * y.z - g.x * y.y + g.y * y.x + g.z * y.w;
  dy.w = g.w * x.w + g.x * x.x + g.y * x.y + g.z * x.z;
  dy.x = -g.w * x.x + g.x * x.w + g.y * x.z - g.z * x.y;
  dy.y = -g.w * x.y - g.x * x.z + g.y * x.w + g.z * x.x;
  dy.z = -g.w * x.z + g.x * x.y - g.y * x.x + g.z * x.w;
}
