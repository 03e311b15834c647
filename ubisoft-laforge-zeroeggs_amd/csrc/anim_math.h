// float64 quaternion / Euler helpers and the two cross-frame kernels (raw local quaternions, sign unrolling) shared by the animation
// feature kernels (anim.hip) and the dataset preparation kernels (prepare.hip).  Everything sits in an unnamed namespace: each
// translation unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct D3 { double x, y, z; };
struct DQ { double w, x, y, z; };
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator*(double s, D3 a) { return D3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ D3 dcross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ DQ dq_inv(DQ q) { return DQ{q.w, -q.x, -q.y, -q.z}; }
__device__ __forceinline__ DQ dq_mul(DQ a, DQ b) {   // quat.py mul: (aw bw - av.bv, aw bv + bw av + av x bv)
  return DQ{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + b.w * a.x + (a.y * b.z - a.z * b.y),
            a.w * b.y + b.w * a.y + (a.z * b.x - a.x * b.z), a.w * b.z + b.w * a.z + (a.x * b.y - a.y * b.x)};
}
__device__ __forceinline__ D3 dq_mul_vec(DQ q, D3 v) {
  const D3 qv = D3{q.x, q.y, q.z};
  const D3 t = 2.0 * dcross(qv, v);
  return v + q.w * t + dcross(qv, t);
}
__device__ __forceinline__ DQ dq_abs(DQ q) { return q.w > 0.0 ? q : DQ{-q.w, -q.x, -q.y, -q.z}; }
// helical (scaled angle-axis) = 2 log(q), quat.py log: atan2(|v|, w) / |v| * v, identity when |v| < eps
__device__ __forceinline__ D3 dq_to_helical(DQ q) {
  const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
  const double s = n < 1e-5 ? 1.0 : atan2(n, q.w) / n;
  return D3{2.0 * s * q.x, 2.0 * s * q.y, 2.0 * s * q.z};
}
__device__ __forceinline__ DQ dq_axis(double angle, int axis) {
  const double h = 0.5 * angle, s = sin(h), c = cos(h);
  return DQ{c, axis == 0 ? s : 0.0, axis == 1 ? s : 0.0, axis == 2 ? s : 0.0};
}
// Channel order of the BVH rotation channels, packed: axis of channel i (0 x, 1 y, 2 z) in bits 2 i .. 2 i + 1; 0 = "zyx" (every
// ZeroEGGS rig).  from_euler takes any order (quat.py:154-163: q = q(e0, axis0) * (q(e1, axis1) * q(e2, axis2))), to_euler the two
// the reference implements (quat.py:111-127: "zyx", "xzy"; it raises for the others, and so does the host side here).
constexpr int ORDER_ZYX = 2 | (1 << 2) | (0 << 4), ORDER_XZY = 0 | (2 << 2) | (1 << 4);
__host__ __device__ inline int order_code(int order) { return order == 0 ? ORDER_ZYX : order; }
__device__ __forceinline__ DQ dq_from_euler_deg(const double* e, int order) {
  const double r = 0.017453292519943295;
  return dq_mul(dq_axis(e[0] * r, order & 3), dq_mul(dq_axis(e[1] * r, (order >> 2) & 3), dq_axis(e[2] * r, (order >> 4) & 3)));
}
__device__ __forceinline__ void dq_to_euler_deg(DQ q, double* e, int order) {
  const double d = 57.29577951308232;
  if (order == ORDER_XZY) {      // quat.py:120-125
    double sz = 2.0 * (q.x * q.y + q.z * q.w);
    sz = sz > 1.0 ? 1.0 : (sz < -1.0 ? -1.0 : sz);
    e[0] = d * atan2(2.0 * (q.x * q.w - q.y * q.z), -q.x * q.x + q.y * q.y - q.z * q.z + q.w * q.w);
    e[1] = d * atan2(2.0 * (q.y * q.w - q.x * q.z), q.x * q.x - q.y * q.y - q.z * q.z + q.w * q.w);
    e[2] = d * asin(sz);
    return;
  }
  double sy = 2.0 * (q.w * q.y - q.z * q.x);      // "zyx", quat.py:114-119
  sy = sy > 1.0 ? 1.0 : (sy < -1.0 ? -1.0 : sy);
  e[0] = d * atan2(2.0 * (q.w * q.z + q.x * q.y), 1.0 - 2.0 * (q.y * q.y + q.z * q.z));
  e[1] = d * asin(sy);
  e[2] = d * atan2(2.0 * (q.w * q.x + q.y * q.z), 1.0 - 2.0 * (q.x * q.x + q.y * q.y));
}
// rotation taking direction a to direction b, normalised (quat.py between + normalize)
__device__ __forceinline__ DQ dq_between_n(D3 a, D3 b) {
  const D3 c = dcross(a, b);
  DQ q = DQ{sqrt(ddot(a, a) * ddot(b, b)) + ddot(a, b), c.x, c.y, c.z};
  const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  return DQ{q.w / n, q.x / n, q.y / n, q.z / n};
}
// rotation matrix (columns = the orthonormalised x, y, z axes of a two-axis encoding) -> quaternion;
// branch choice as quat.py from_xform (trace / largest diagonal element)
__device__ __forceinline__ DQ dq_from_xy(D3 x, D3 yin) {
  const double eps = 1e-10;
  D3 z = dcross(x, yin);
  D3 y = dcross(z, x);
  x = (1.0 / (sqrt(ddot(x, x)) + eps)) * x;
  y = (1.0 / (sqrt(ddot(y, y)) + eps)) * y;
  z = (1.0 / (sqrt(ddot(z, z)) + eps)) * z;
  // m[r][c]: column 0 = x, 1 = y, 2 = z
  const double m00 = x.x, m10 = x.y, m20 = x.z, m01 = y.x, m11 = y.y, m21 = y.z, m02 = z.x, m12 = z.y, m22 = z.z;
  const double tr = m00 + m11 + m22;
  const double a = m21 - m12, b = m02 - m20, c = m10 - m01, p = m01 + m10, q = m02 + m20, r = m12 + m21;
  if (tr > 0.0) {
    const double s = 0.5 / sqrt(fmax(tr + 1.0, eps));
    return DQ{0.25 / s, s * a, s * b, s * c};
  }
  if (m00 > m11 && m00 > m22) {
    const double s = 2.0 * sqrt(fmax(1.0 + m00 - m11 - m22, eps));
    return DQ{a / s, 0.25 * s, p / s, q / s};
  }
  if (m11 > m22) {
    const double s = 2.0 * sqrt(fmax(1.0 + m11 - m00 - m22, eps));
    return DQ{b / s, p / s, 0.25 * s, r / s};
  }
  const double s = 2.0 * sqrt(fmax(1.0 + m22 - m00 - m11, eps));
  return DQ{c / s, q / s, r / s, 0.25 * s};
}

__device__ __forceinline__ D3 ld3(const double* p) { return D3{p[0], p[1], p[2]}; }
__device__ __forceinline__ DQ ldq(const double* p) { return DQ{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void st3(double* p, D3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
__device__ __forceinline__ void stq(double* p, DQ q) { p[0] = q.w; p[1] = q.x; p[2] = q.y; p[3] = q.z; }

// 1. euler channels -> raw local quaternions and the dot product with the previous frame's raw quaternion
__global__ void anim_quat_k(const double* euler, double* lrot, double* dprev, int N, int J, int order) {
  const long n = (long)N * J;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const DQ q = dq_from_euler_deg(euler + i * 3, order);
    stq(lrot + i * 4, q);
    double d = 1.0;
    if (i >= J) {
      const DQ p = dq_from_euler_deg(euler + (i - J) * 3, order);
      d = q.w * p.w + q.x * p.x + q.y * p.y + q.z * p.z;
    }
    dprev[i] = d;
  }
}
// 2. sign unrolling (quat.py unroll): frame i is negated when its dot product with the ALREADY unrolled frame i-1
//    is negative: s_i = (s_{i-1} d_i < 0) ? -1 : +1.  One thread per joint walks the frames (loads are independent of
//    the recurrence, 8 in flight).
__global__ void anim_unroll_k(const double* dprev, double* sign, int N, int J) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= J) return;
  double s = 1.0;
  sign[j] = 1.0;
  int i = 1;
  for (; i + 8 <= N; i += 8) {
    double d[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) d[u] = dprev[(long)(i + u) * J + j];
#pragma unroll
    for (int u = 0; u < 8; ++u) { s = (s * d[u] < 0.0) ? -1.0 : 1.0; sign[(long)(i + u) * J + j] = s; }
  }
  for (; i < N; ++i) { s = (s * dprev[(long)i * J + j] < 0.0) ? -1.0 : 1.0; sign[(long)i * J + j] = s; }
}

}  // namespace
