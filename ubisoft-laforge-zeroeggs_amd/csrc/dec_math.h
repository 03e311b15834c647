// The pointwise math of one decoder step, stated once for every decoder kernel: the root integration of a frame
// (devectorize_output, ZEGGS/modules.py:716-742) with the gaze direction of the next input (:693), its adjoint in one piece and
// split for the persistent BPTT sweep, and the GRU cell forward / backward.  Each kernel keeps its own loads, stores and
// normalisation constants and calls these for the arithmetic.  The root part and gru_cell_bwd are plain C++ behind ZQ_HD
// (quat_math.h) and run on the host in tests/host/dec_math_check.cpp; gru_cell_fwd needs the hardware gates of common.h.
#pragma once
#include <math.h>
#include "quat_math.h"
#if defined(__HIPCC__)
#include "common.h"
#endif

// ------------------------------------------------------------------ quat_exp
// sin(h) / h and cos(h) of a half rotation angle.  The root turns a fraction of a radian per frame, so h < 1 is the only case
// that occurs in practice: two even polynomials in h^2 (truncation error 2.5e-8 / 2e-9 at h = 1, below fp32 rounding) instead of
// sinf + cosf + a division (~200 instructions with their range reduction) in the epilogue of every output stage of the
// persistent rollouts.  h >= 1: the library functions.
// -DZEGGS_EXACT_SINCOS=1: always the library functions (A/B builds of tools/drift_ab.py).
#ifndef ZEGGS_EXACT_SINCOS
#define ZEGGS_EXACT_SINCOS 0
#endif
ZQ_HD void d_sinc_cos(float h, float& sinc, float& c) {
  if (!ZEGGS_EXACT_SINCOS && h < 1.f) {
    const float u = h * h;
    sinc = 1.f + u * (-1.f / 6.f + u * (1.f / 120.f + u * (-1.f / 5040.f + u * (1.f / 362880.f + u * (-1.f / 39916800.f)))));
    c = 1.f + u * (-0.5f + u * (1.f / 24.f + u * (-1.f / 720.f + u * (1.f / 40320.f + u * (-1.f / 3628800.f + u * (1.f / 479001600.f))))));
  } else {
    sinc = sinf(h) / h;
    c = cosf(h);
  }
}

// The root update  q' = quat_mul(quat_from_helical(u), q) = quat_mul(quat_exp(u / 2), q)  (ZEGGS/modules.py:739) as q + DELTA.
// Written as a product, the scalar part of exp(x) -- cos|x| = 1 - |x|^2 / 2 + ..., |x| ~ 1e-3 per frame -- is rounded to the
// fp32 grid around 1 (spacing 6e-8) BEFORE it multiplies q: an error of up to 3e-8 per frame that keeps its sign while the
// root turns at a steady rate, i.e. the norm of the (never re-normalised) root quaternion drifts linearly, 1e-3 over the
// 108 000 frames of a 30-minute decode, and every later root step is scaled by it -- the whole long-run drift of round 3
// (tools/drift_ab.py: with the root update in float64 the deviation from the reference's fp64 run falls from 5e-2 to 2e-4;
// exact gates / exact sin, cos / no algebraic folds change nothing).  The reference's own fp32 run has the same defect with
// other rounding luck (3e-3).  Here cos|x| - 1 = -|x|^2 (1/2 - |x|^2 / 24 + ...) is formed at full relative precision and the
// small correction DELTA = (cos|x| - 1) q + [ -e.qv, q.w e + e x qv ] is added to q with ONE (data-dependent, zero-mean)
// rounding.  Same function as quat_mul(quat_exp(x), q) in exact arithmetic, both branches of quat_exp (tquat.py:94-99).
ZQ_HD Q4 quat_exp_mul(V3 x, Q4 q) {
  const float u = x.x * x.x + x.y * x.y + x.z * x.z;
  const float h = sqrtf(u);
  float cm1, s;          // scalar part of exp(x) minus one; factor of the vector part
  if (h < 1e-5f) {       // quat_normalize([1, x], eps = 1e-5) = [1, x] / (sqrt(1 + |x|^2) + 1e-5)
    const float nm1 = 0.5f * u;                    // sqrt(1 + u) - 1 for u < 1e-10
    const float ne = 1.f + (nm1 + 1e-5f);
    s = 1.f / ne;
    cm1 = -(nm1 + 1e-5f) * s;
  } else if (!ZEGGS_EXACT_SINCOS && h < 1.f) {
    s = 1.f + u * (-1.f / 6.f + u * (1.f / 120.f + u * (-1.f / 5040.f + u * (1.f / 362880.f + u * (-1.f / 39916800.f)))));
    cm1 = u * (-0.5f + u * (1.f / 24.f + u * (-1.f / 720.f + u * (1.f / 40320.f + u * (-1.f / 3628800.f + u * (1.f / 479001600.f))))));
  } else {
    const float sh = sinf(0.5f * h);
    s = sinf(h) / h;
    cm1 = -2.f * sh * sh;
  }
  const V3 e = s * x, qv = v3(q.x, q.y, q.z);
  const V3 c = cross(e, qv);
  return Q4{q.w + (cm1 * q.w - dot(e, qv)), q.x + (cm1 * q.x + q.w * e.x + c.x), q.y + (cm1 * q.y + q.w * e.y + c.y),
            q.z + (cm1 * q.z + q.w * e.z + c.z)};
}

// quat_exp (reference anim/tquat.py:94-107: quat_from_helical(x) = quat_exp(x / 2)) and its backward for the SAME argument
// share the norm and its sine / cosine: the root adjoint evaluates both on one thread
struct QExpCtx { float h, sh, ch; };
ZQ_HD Q4 quat_exp_ctx(V3 x, QExpCtx& c) {
  c.h = sqrtf(x.x * x.x + x.y * x.y + x.z * x.z);
  if (c.h < 1e-5f) {
    c.sh = 0.f; c.ch = 1.f;
    float n = sqrtf(1.f + c.h * c.h) + 1e-5f;
    return Q4{1.f / n, x.x / n, x.y / n, x.z / n};
  }
  float s;
  d_sinc_cos(c.h, s, c.ch);
  c.sh = s * c.h;
  return Q4{c.ch, x.x * s, x.y * s, x.z * s};
}
ZQ_HD V3 qexp_bwd_ctx(V3 x, Q4 g, const QExpCtx& c) {
  V3 gv = v3(g.x, g.y, g.z);
  if (c.h < 1e-5f) {
    float n = sqrtf(1.f + c.h * c.h), ne = n + 1e-5f;
    float ug = g.w + dot(gv, x);
    float k = ug / (n * ne * ne);
    return (1.f / ne) * gv - k * x;
  }
  const float s = c.sh / c.h, ds = (c.h * c.ch - c.sh) / (c.h * c.h);
  const float cc = -g.w * s + dot(gv, x) * ds / c.h;
  return s * gv + cc * x;
}
// the same backward as three coefficients at a prepared point x (the caller keeps x): du = ea * g_v + (eb_ * g_w + ec * <g_v, x>) * x, the
// divisions by the norm done when the frame is prepared (root_prepare / root_apply)
ZQ_HD void qexp_bwd_coef(const QExpCtx& c, float& ea, float& eb_, float& ec) {
  if (c.h < 1e-5f) {
    const float n = sqrtf(1.f + c.h * c.h), ne = n + 1e-5f, k = 1.f / (n * ne * ne);
    ea = 1.f / ne; eb_ = -k; ec = -k;
  } else {
    const float s = c.sh / c.h, ds = (c.h * c.ch - c.sh) / (c.h * c.h);
    ea = s; eb_ = -s; ec = ds / c.h;
  }
}

// ------------------------------------------------------------------ root integration, forward
// frame t from the root state (q, pos) of frame t-1 and the de-normalised root velocities p = pose_t[0:6]
ZQ_HD void root_step(float dt, Q4 q, V3 pos, const float (&p)[6], V3& npos, Q4& nq) {
  npos = quat_mul_vec(q, dt * v3(p[0], p[1], p[2])) + pos;
  const V3 uu = quat_mul_vec(q, dt * v3(p[3], p[4], p[5]));
  nq = quat_exp_mul(0.5f * uu, q);
}
// gaze direction of vectorize_input: quat_inv_mul_vec(root_rot, gaze_pos - root_pos), NOT normalised (modules.py:693)
ZQ_HD V3 gaze_dir(Q4 q, V3 pos, V3 gaze) { return quat_mul_vec(quat_inv(q), gaze - pos); }

// DIAGNOSTIC (-DZEGGS_ROOT_FP64=1, tools/drift_ab.py; called by the generic path only): root_step evaluated in float64 from
// the same fp32 inputs, rounded once at the end -- separates "rounding inside the root integration" from everything else
ZQ_HD void root_step_fp64(float dt, Q4 q, V3 pos, const float (&p)[6], V3& npos, Q4& nq) {
  auto qmv = [](const double* q4, const double* v, double* o) {
    const double tx = 2.0 * (q4[2] * v[2] - q4[3] * v[1]), ty = 2.0 * (q4[3] * v[0] - q4[1] * v[2]),
                 tz = 2.0 * (q4[1] * v[1] - q4[2] * v[0]);
    o[0] = v[0] + q4[0] * tx + (q4[2] * tz - q4[3] * ty);
    o[1] = v[1] + q4[0] * ty + (q4[3] * tx - q4[1] * tz);
    o[2] = v[2] + q4[0] * tz + (q4[1] * ty - q4[2] * tx);
  };
  const double qd[4] = {q.w, q.x, q.y, q.z}, dtd = (double)dt;
  const double v[3] = {dtd * p[0], dtd * p[1], dtd * p[2]}, w3[3] = {dtd * p[3], dtd * p[4], dtd * p[5]};
  double o[3], u3[3];
  qmv(qd, v, o);
  npos = v3((float)(o[0] + pos.x), (float)(o[1] + pos.y), (float)(o[2] + pos.z));
  qmv(qd, w3, u3);
  const double hx = 0.5 * u3[0], hy = 0.5 * u3[1], hz = 0.5 * u3[2], h = sqrt(hx * hx + hy * hy + hz * hz);
  double e[4];
  if (h < 1e-5) { const double n = sqrt(1.0 + h * h) + 1e-5; e[0] = 1.0 / n; e[1] = hx / n; e[2] = hy / n; e[3] = hz / n; }
  else { const double sc = sin(h) / h; e[0] = cos(h); e[1] = hx * sc; e[2] = hy * sc; e[3] = hz * sc; }
  // quat_mul(e, q)
  nq = Q4{(float)(qd[0] * e[0] - qd[1] * e[1] - qd[2] * e[2] - qd[3] * e[3]),
          (float)(qd[0] * e[1] + qd[1] * e[0] - qd[2] * e[3] + qd[3] * e[2]),
          (float)(qd[0] * e[2] + qd[1] * e[3] + qd[2] * e[0] - qd[3] * e[1]),
          (float)(qd[0] * e[3] - qd[1] * e[2] + qd[2] * e[1] + qd[3] * e[0])};
}

// ------------------------------------------------------------------ root integration, adjoint in one piece
// adjoint of gd = gaze_dir(q, pos, gaze) given dgd: dq wrt q (the sign of quat_inv applied), dw wrt w = gaze - pos, i.e.
// the gradient wrt gaze is dw and wrt pos is -dw
ZQ_HD void gaze_dir_bwd(Q4 q, V3 w, V3 dgd, Q4& dq, V3& dw) {
  Q4 dqi;
  qmv_bwd(quat_inv(q), w, dgd, dqi, dw);
  dq = Q4{dqi.w, -dqi.x, -dqi.y, -dqi.z};
}
// adjoint of root_step given (g_rp, g_rr) = gradient wrt (npos, nq): g6 += gradient wrt p, dq = gradient wrt q; the gradient
// wrt pos is g_rp itself.      npos = qmv(q, vel dt) + pos;  nq = qmul(E, q), E = qexp(u / 2), u = qmv(q, vrt dt)
ZQ_HD void root_step_bwd(float dt, Q4 q, V3 vel, V3 vrt, V3 g_rp, Q4 g_rr, float (&g6)[6], Q4& dq) {
  Q4 dq1; V3 dv1;
  qmv_bwd(q, dt * vel, g_rp, dq1, dv1);
  const V3 u = quat_mul_vec(q, dt * vrt);
  QExpCtx ec;
  const Q4 E = quat_exp_ctx(0.5f * u, ec);
  Q4 dE, dqy;
  qmul_bwd(E, q, g_rr, dE, dqy);
  const V3 du = 0.5f * qexp_bwd_ctx(0.5f * u, dE, ec);
  Q4 dq2; V3 dv2;
  qmv_bwd(q, dt * vrt, du, dq2, dv2);
  g6[0] += dt * dv1.x; g6[1] += dt * dv1.y; g6[2] += dt * dv1.z;
  g6[3] += dt * dv2.x; g6[4] += dt * dv2.y; g6[5] += dt * dv2.z;
  dq = Q4{dq1.w + dqy.w + dq2.w, dq1.x + dqy.x + dq2.x, dq1.y + dqy.y + dq2.y, dq1.z + dqy.z + dq2.z};
}
// BPTT of frame f.  In: (g_rp, g_rr) = gradient wrt (root_pos_f, root_rot_f) from the later frames plus this frame's direct
// loss gradients; g6 = dpose[f][0:6] + dx_{f+1} / sigma_i.  has_next: x_{f+1} exists and its gaze direction (gradient dgd,
// de-normalised; gz = gaze target of frame f+1) was formed from (q_t, p_t) = root state of frame f.  (q_p; vel, vrt) = root
// rotation of frame f-1; pose[f][0:6].  Out: (g_rp, g_rr) wrt the root state of frame f-1, g6 = total gradient wrt pose[f][0:6].
ZQ_HD void root_bwd(float dt, Q4 q_t, V3 p_t, V3 gz, V3 dgd, bool has_next, Q4 q_p, V3 vel, V3 vrt, V3& g_rp, Q4& g_rr,
                    float (&g6)[6]) {
  if (has_next) {
    Q4 dq; V3 dw;
    gaze_dir_bwd(q_t, gz - p_t, dgd, dq, dw);
    g_rr.w += dq.w; g_rr.x += dq.x; g_rr.y += dq.y; g_rr.z += dq.z;
    g_rp = g_rp - dw;
  }
  Q4 dq;
  root_step_bwd(dt, q_p, vel, vrt, g_rp, g_rr, g6, dq);
  g_rr = dq;
}

// ------------------------------------------------------------------ root integration, adjoint split in two
// For the persistent BPTT kernel: everything that depends on forward data only (the rotations, quat_exp and its sine /
// cosine) is evaluated one phase ahead by the root thread and parked in its LDS column (33 values, in place of the raw
// inputs); what is left behind the hand-off is linear in the incoming gradients.
// the raw inputs of a frame's root adjoint: drpos_f, drrot_f, rrot_f, rpos_f, gaze_{f+1}, rrot_{f-1}, pose_f[0:6], dpose_f[0:6]
struct RootIn {
  float a[3], e[4], rq[4], rp[3], gz[3], pq[4], pt[6], dp[6];
  template <class F>
  ZQ_HD void gather(F get) {      // get(item) -> value
#pragma unroll
    for (int i = 0; i < 3; ++i) { a[i] = get(i); rp[i] = get(11 + i); gz[i] = get(14 + i); }
#pragma unroll
    for (int i = 0; i < 4; ++i) { e[i] = get(3 + i); rq[i] = get(7 + i); pq[i] = get(17 + i); }
#pragma unroll
    for (int i = 0; i < 6; ++i) { pt[i] = get(21 + i); dp[i] = get(27 + i); }
  }
};
struct RootPre { Q4 qti; V3 w; Q4 qp; V3 dvel, dvrt, hu; Q4 E; float ea, eb_, ec; float dp[6]; };
ZQ_HD void root_prepare(float dt, const RootIn& ri, RootPre& o) {
  o.qti = quat_inv(Q4{ri.rq[0], ri.rq[1], ri.rq[2], ri.rq[3]});
  o.w = v3(ri.gz[0], ri.gz[1], ri.gz[2]) - v3(ri.rp[0], ri.rp[1], ri.rp[2]);
  o.qp = Q4{ri.pq[0], ri.pq[1], ri.pq[2], ri.pq[3]};
  o.dvel = dt * v3(ri.pt[0], ri.pt[1], ri.pt[2]);
  o.dvrt = dt * v3(ri.pt[3], ri.pt[4], ri.pt[5]);
  o.hu = 0.5f * quat_mul_vec(o.qp, o.dvrt);
  QExpCtx ctx;
  o.E = quat_exp_ctx(o.hu, ctx);
  qexp_bwd_coef(ctx, o.ea, o.eb_, o.ec);
#pragma unroll
  for (int i = 0; i < 6; ++i) o.dp[i] = ri.dp[i];
}
template <class F>
ZQ_HD void root_pre_store(const RootPre& o, F put) {      // put(slot, value)
  put(0, o.qti.w); put(1, o.qti.x); put(2, o.qti.y); put(3, o.qti.z); put(4, o.w.x); put(5, o.w.y); put(6, o.w.z);
  put(7, o.qp.w); put(8, o.qp.x); put(9, o.qp.y); put(10, o.qp.z); put(11, o.dvel.x); put(12, o.dvel.y); put(13, o.dvel.z);
  put(14, o.dvrt.x); put(15, o.dvrt.y); put(16, o.dvrt.z); put(17, o.hu.x); put(18, o.hu.y); put(19, o.hu.z);
  put(20, o.E.w); put(21, o.E.x); put(22, o.E.y); put(23, o.E.z); put(24, o.ea); put(25, o.eb_); put(26, o.ec);
#pragma unroll
  for (int i = 0; i < 6; ++i) put(27 + i, o.dp[i]);
}
// the scheduler may not move code across these on the device (see root_apply); nothing to say on the host
#if defined(__HIP_DEVICE_COMPILE__)
#define ZQ_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)
#else
#define ZQ_SCHED_BARRIER() ((void)0)
#endif
// cr: adjoint of (root_pos_f, root_rot_f) INCLUDING this frame's direct loss gradients (drpos / drrot were added when the
// frame was prepared).  The prepared values are fetched (get(slot), see root_pre_store) right where they are used: the
// workgroup's registers are full of weights, and 33 values loaded up front get spilled to scratch around this code.
template <class F>
ZQ_HD void root_apply(float dt, const float* gaze_rstd /* 1 / in_std[PO..PO+2] */, F get, const float (&dgd_in)[3],
                      float (&cr)[7], float (&g6)[6]) {
  V3 g_rp = v3(cr[0], cr[1], cr[2]);
  Q4 g_rr = Q4{cr[3], cr[4], cr[5], cr[6]};
  {
    const V3 dgd = v3(dgd_in[0] * gaze_rstd[0], dgd_in[1] * gaze_rstd[1], dgd_in[2] * gaze_rstd[2]);
    Q4 dqi; V3 dv;
    qmv_bwd(Q4{get(0), get(1), get(2), get(3)}, v3(get(4), get(5), get(6)), dgd, dqi, dv);
    g_rr.w += dqi.w; g_rr.x -= dqi.x; g_rr.y -= dqi.y; g_rr.z -= dqi.z;
    g_rp = g_rp - dv;
  }
  ZQ_SCHED_BARRIER();
  const Q4 qp = Q4{get(7), get(8), get(9), get(10)};
  Q4 dq1; V3 dv1;
  qmv_bwd(qp, v3(get(11), get(12), get(13)), g_rp, dq1, dv1);
  g6[0] += dt * dv1.x; g6[1] += dt * dv1.y; g6[2] += dt * dv1.z;
  ZQ_SCHED_BARRIER();
  Q4 dE, dqy;
  qmul_bwd(Q4{get(20), get(21), get(22), get(23)}, qp, g_rr, dE, dqy);
  ZQ_SCHED_BARRIER();
  V3 du;
  {
    const V3 hu = v3(get(17), get(18), get(19)), gv = v3(dE.x, dE.y, dE.z);
    du = 0.5f * (get(24) * gv + (get(25) * dE.w + get(26) * dot(gv, hu)) * hu);
  }
  Q4 dq2; V3 dv2;
  qmv_bwd(qp, v3(get(14), get(15), get(16)), du, dq2, dv2);
  g6[3] += dt * dv2.x; g6[4] += dt * dv2.y; g6[5] += dt * dv2.z;
  cr[0] = g_rp.x; cr[1] = g_rp.y; cr[2] = g_rp.z;
  cr[3] = dq1.w + dqy.w + dq2.w; cr[4] = dq1.x + dqy.x + dq2.x;
  cr[5] = dq1.y + dqy.y + dq2.y; cr[6] = dq1.z + dqy.z + dq2.z;
}

// ------------------------------------------------------------------ GRU cell (nn.GRU, gate order r, z, n)
// ar, az, an: the summed pre-activations of the three gates WITHOUT the hidden side of n; nh = W_hn h + b_hn.  Every site
// sums its partial products and biases in its own order before the call.  gt = (r, z, nn, nh): what the backward reads.
#if defined(__HIPCC__)
__device__ __forceinline__ float gru_cell_fwd(float ar, float az, float an, float nh, float hprev, f4& gt) {
  const float r = d_sigmoid(ar);
  const float z = d_sigmoid(az);
  const float nn = d_tanh(an + r * nh);
  gt = f4{r, z, nn, nh};
  return (1.f - z) * nn + z * hprev;
}
#endif
// g = total gradient wrt h' -> gradients wrt the pre-activations: (dar, daz, dan) of the input side; the hidden side shares
// dar, daz and has dhn() = dan * r in its n rows; dhc() = g * z is the direct path to h_prev.  The two products are formed
// where a site uses them, as every site did before (the persistent BPTT kernel's instruction stream depends on it).
// GT: any (x, y, z, w) = (r, z, nn, nh).
struct GruGrad {
  float dar, daz, dan, g, r, z;
  ZQ_HD float dhn() const { return dan * r; }
  ZQ_HD float dhc() const { return g * z; }
};
template <class GT>
ZQ_HD GruGrad gru_cell_bwd(float g, const GT& gt, float hprev) {
  const float r = gt.x, z = gt.y, nn = gt.z, nh = gt.w;
  const float dn = g * (1.f - z);
  const float dz = g * (hprev - nn);
  const float dan = dn * (1.f - nn * nn);
  const float dar = dan * nh * r * (1.f - r);
  const float daz = dz * z * (1.f - z);
  return GruGrad{dar, daz, dan, g, r, z};
}
