// Autoregressive gesture decoder: cell-state encoder + T-1 sequential steps of
//   vectorize_input -> Linear+ELU -> 2-layer GRU (seq len 1) -> Linear -> devectorize_output
// (reference ZEGGS/modules.py:47-243, 677-742) and the matching BPTT.
//
// Data layout (all time-major so that one step's rows are contiguous and the
// weight-gradient GEMMs contract over the flattened (t, b) axis):
//   Gin [T][B][GL]   GL = round4(H + XD): per step [hid(H) | x(XD)], x = [pose(PI) | speech | style]
//   H0/H1 [T][B][H]  hidden states, slot 0 = CellStateEncoder output
//   R*,Z*,N*,NH*     [T][B][H] saved gates (NH = W_hn h + b_hn) for both layers
//   D*               [T][B][.] gate/pre-activation gradients produced by the backward sweep
#include "../../include/zeggs_hip.h"
#include "common.h"
#include "gemm.h"
#include "kernels.h"
#include "dec_math.h"
#include "dec_prologue.h"
#include "decoder_ws.h"

int g_decoder_fast = 1;      // option "decoder_fast": 0 = generic per-step GEMM path everywhere (A/B reference of the stage kernels)
int g_bwd_chunks = 1;        // option "bwd_chunks": BPTT sweep chunks whose weight-gradient GEMMs overlap the rest of the sweep (1: serial)
int g_tp_prologue = 1;       // option "tp_prologue", 0 / 1: the training rollout's prologue in five launches instead of ten
int g_wgrad_order = 0;       // option "wgrad_order", 0 / 1 / 2: see dec_recurrent_wgrads

// What tells a caller that a persistent kernel gave up AFTER its first (validated) use -- e.g. a co-tenant took CUs, so not
// every workgroup was resident and a bounded wait ran out: (1) the kernel ORs its bit into the caller-owned sticky status word
// (ZeggsDecCall.status) that zeggs_radam_step_guarded reads on the device -- the optimizer step of that iteration is then a
// no-op, nothing invalid reaches the weights -- and that the caller inspects whenever it likes; (2) it writes NaN into what its
// consumers read first (last output frame / the carries of the CellStateEncoder backward).  The library keeps no per-process
// watch state of its own.
// 1: the persistent kernel was validated on this process, 0: it failed once and is disabled, -1: not used yet
extern "C" int zeggs_persistent_state(int which /* 0 decode (B=1), 1 training forward, 2 BPTT sweep */) {
  return g_sweep_kernels[which == 0 ? SWEEP_DECODE : which == 1 ? SWEEP_ROLLOUT : SWEEP_BPTT].state;
}

namespace {

// ------------------------------------------------------------------ kernels
// init: frame-0 outputs, CellStateEncoder input (gaze of frame 0) and the pose part of x_1 (gaze of frame 1)
__global__ void dec_init_k(ZeggsDecDims d, ZeggsDecStats st, const float* pose0, const float* rp0, const float* rr0,
                           const float* gaze, const float* style, float* pose, float* rpos, float* rrot,
                           float* cse_in, float* gin1, int GL) {
  dec_init_body(blockIdx.x, d, st, pose0, rp0, rr0, gaze, style, pose, rpos, rrot, cse_in, gin1, GL);
}

// speech / style columns of x_t for one step (or all steps when nt > 1): Gin[t][b][H+PI ...]
__global__ void dec_fill_cond_k(ZeggsDecDims d, const float* speech, const float* style, float* gin, int GL, int t0,
                                int nt, long slot_stride, int ring) {
  dec_fill_cond_body(blockIdx.x, gridDim.x, d, speech, style, gin, GL, t0, nt, slot_stride, ring);
}

// GRU cell gate math (nn.GRU, gate order r,z,n)
__global__ void gru_gate_fwd_k(const float* gi, const float* gh, const float* hprev, float* hout, f4* GT, int B, int H) {
  long n = (long)B * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int u = (int)(i % H);
    long b = i / H;
    const float* gib = gi + b * 3 * H;
    const float* ghb = gh + b * 3 * H;
    f4 gt;
    hout[i] = gru_cell_fwd(gib[u] + ghb[u], gib[H + u] + ghb[H + u], gib[2 * H + u], ghb[2 * H + u], hprev[i], gt);
    if (GT) GT[i] = gt;
  }
}

// dh (total grad wrt h') -> di [B,3H] (grad wrt W_ih x + b_ih), dhh [B,3H] (grad wrt W_hh h + b_hh),
// dhc = dh * z (direct path to h_prev)
__global__ void gru_gate_bwd_k(const float* dh, const f4* GT, const float* hprev, float* di, float* dhh, float* dhc, int B,
                               int H) {
  long n = (long)B * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int u = (int)(i % H);
    long b = i / H;
    const GruGrad gg = gru_cell_bwd(dh[i], GT[i], hprev[i]);
    float* dib = di + b * 3 * H;
    float* dhb = dhh + b * 3 * H;
    dib[u] = gg.dar; dib[H + u] = gg.daz; dib[2 * H + u] = gg.dan;
    dhb[u] = gg.dar; dhb[H + u] = gg.daz; dhb[2 * H + u] = gg.dhn();
    dhc[i] = gg.dhc();
  }
}

// devectorize_output + next step's vectorize_input for one step t
__global__ void dec_devec_k(ZeggsDecDims d, ZeggsDecStats st, const float* y, int POL, const float* gaze, float* pose,
                            float* rpos, float* rrot, float* gin_next, int GL, int t) {
  const int b = blockIdx.x;
  const float* yb = y + (long)b * POL;
  float* pb = pose + ((long)b * d.T + t) * d.PO;
  for (int c = threadIdx.x; c < d.PO; c += blockDim.x) {
    float p = yb[c] * st.out_std[c] + st.out_mean[c];
    pb[c] = p;
    if (gin_next) gin_next[(long)b * GL + d.H + c] = (p - st.in_mean[c]) / st.in_std[c];
  }
  if (threadIdx.x == 0) {
    float p[6];
    for (int c = 0; c < 6; ++c) p[c] = yb[c] * st.out_std[c] + st.out_mean[c];
    const float* rq = rrot + ((long)b * d.T + t - 1) * 4;
    const float* rp = rpos + ((long)b * d.T + t - 1) * 3;
    Q4 q = Q4{rq[0], rq[1], rq[2], rq[3]};
    V3 pos = v3(rp[0], rp[1], rp[2]);
    V3 npos; Q4 nq;
#if defined(ZEGGS_ROOT_FP64) && ZEGGS_ROOT_FP64
    root_step_fp64(d.dt, q, pos, p, npos, nq);      // diagnostic build (tools/drift_ab.py), this path only
#else
    root_step(d.dt, q, pos, p, npos, nq);
#endif
    float* op = rpos + ((long)b * d.T + t) * 3; op[0] = npos.x; op[1] = npos.y; op[2] = npos.z;
    float* oq = rrot + ((long)b * d.T + t) * 4; oq[0] = nq.w; oq[1] = nq.x; oq[2] = nq.y; oq[3] = nq.z;
    if (gin_next) {
      const float* gz = gaze + ((long)b * d.T + t + 1) * 3;
      V3 gd = gaze_dir(nq, npos, v3(gz[0], gz[1], gz[2]));
      float gv[3] = {gd.x, gd.y, gd.z};
      for (int k = 0; k < 3; ++k)
        gin_next[(long)b * GL + d.H + d.PO + k] = (gv[k] - st.in_mean[d.PO + k]) / st.in_std[d.PO + k];
    }
  }
}

// backward of dec_devec_k for step t.
//   dxn   [B, XD]  grad wrt x_{t+1} (pose part used), null at the last step
//   carry [B, 8]   grad wrt (rpos_t[3], rrot_t[4]) coming from steps > t (updated to frame t-1's)
//   dy    [B, POL] output: grad wrt the raw network output of step t
__global__ void dec_devec_bwd_k(ZeggsDecDims d, ZeggsDecStats st, const float* dpose, const float* drpos,
                                const float* drrot, const float* dxn, int XD, const float* gaze, const float* pose,
                                const float* rpos, const float* rrot, float* carry, float* dy, int POL, int t) {
  const int b = blockIdx.x;
  const float* dpb = dpose + ((long)b * d.T + t) * d.PO;
  const float* dxb = dxn ? dxn + (long)b * XD : nullptr;
  float* dyb = dy + (long)b * POL;
  for (int c = 6 + threadIdx.x; c < d.PO; c += blockDim.x) {
    float g = dpb[c] + (dxb ? dxb[c] / st.in_std[c] : 0.f);
    dyb[c] = g * st.out_std[c];
  }
  if (threadIdx.x == 0) {
    float g6[6];
    for (int c = 0; c < 6; ++c) g6[c] = dpb[c] + (dxb ? dxb[c] / st.in_std[c] : 0.f);
    float* cr = carry + b * 8;
    const float* a = drpos + ((long)b * d.T + t) * 3;
    const float* e = drrot + ((long)b * d.T + t) * 4;
    V3 g_rp = v3(cr[0] + a[0], cr[1] + a[1], cr[2] + a[2]);
    Q4 g_rr = Q4{cr[3] + e[0], cr[4] + e[1], cr[5] + e[2], cr[6] + e[3]};
    const float* rq = rrot + ((long)b * d.T + t) * 4;
    const float* rp = rpos + ((long)b * d.T + t) * 3;
    V3 gz = v3(0.f, 0.f, 0.f), dgd = gz;
    if (dxb) {   // gaze direction of x_{t+1}
      const float* gp = gaze + ((long)b * d.T + t + 1) * 3;
      gz = v3(gp[0], gp[1], gp[2]);
      dgd = v3(dxb[d.PO] / st.in_std[d.PO], dxb[d.PO + 1] / st.in_std[d.PO + 1], dxb[d.PO + 2] / st.in_std[d.PO + 2]);
    }
    const float* pq = rrot + ((long)b * d.T + t - 1) * 4;
    const float* pt = pose + ((long)b * d.T + t) * d.PO;
    root_bwd(d.dt, Q4{rq[0], rq[1], rq[2], rq[3]}, v3(rp[0], rp[1], rp[2]), gz, dgd, dxb != nullptr,
             Q4{pq[0], pq[1], pq[2], pq[3]}, v3(pt[0], pt[1], pt[2]), v3(pt[3], pt[4], pt[5]), g_rp, g_rr, g6);
    cr[0] = g_rp.x; cr[1] = g_rp.y; cr[2] = g_rp.z;
    cr[3] = g_rr.w; cr[4] = g_rr.x; cr[5] = g_rr.y; cr[6] = g_rr.z;
    for (int c = 0; c < 6; ++c) dyb[c] = g6[c] * st.out_std[c];
  }
}

// d0[b][u] = dgin[b][u] * ELU'(hid[b][u]);  rows strided by GL
__global__ void elu_bwd_rows_k(float* d0, const float* dgin, const float* gin, int B, int H, int GL) {
  long n = (long)B * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int u = (int)(i % H);
    long b = i / H;
    d0[i] = dgin[b * GL + u] * d_elu_grad_from_out(gin[b * GL + u]);
  }
}

// copy rows: dst[b][0:w] = src[b][off : off+w]
__global__ void copy_cols_k(float* dst, long ldd, const float* src, long lds, int off, int w, int B) {
  long n = (long)B * w;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int c = (int)(i % w);
    long b = i / w;
    dst[b * ldd + c] = src[b * lds + off + c];
  }
}

// scatter time-major dX [T][B][XD] speech/style columns into batch-major outputs
__global__ void dec_scatter_cond_grad_k(ZeggsDecDims d, const float* DX, int XD, float* dspeech, float* dstyle) {
  const int XC = d.SP + (d.film ? 0 : d.ST);
  long n = (long)d.T * d.B * XC;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int c = (int)(i % XC);
    long r = i / XC;
    int b = (int)(r % d.B);
    int t = (int)(r / d.B);
    float v = t == 0 ? 0.f : DX[((long)t * d.B + b) * XD + d.PI + c];
    if (c < d.SP) dspeech[((long)b * d.T + t) * d.SP + c] = v;
    else dstyle[((long)b * d.T + t) * d.ST + (c - d.SP)] = v;
  }
}
// ---- FiLM (reference modules.py:213-225): out = a * (1 + gamma) + beta; all operands row-strided views
__global__ void film_fwd_k(float* out, long ldo, const float* a, const float* gam, const float* bet, long ldg, int B,
                           int H) {
  long n = (long)B * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int u = (int)(i % H);
    long b = i / H;
    out[b * ldo + u] = a[i] * (1.f + gam[b * ldg + u]) + bet[b * ldg + u];
  }
}
// g = grad wrt the modulated value -> dpre = g (1+gamma) ELU'(a) (a = ELU output), dgamma = g a, dbeta = g
__global__ void film_bwd_k(const float* g, long ldgr, const float* a, const float* gam, long ldg, float* dpre,
                           float* dgam, float* dbet, int B, int H) {
  long n = (long)B * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int u = (int)(i % H);
    long b = i / H;
    const float gv = g[b * ldgr + u], av = a[i];
    dpre[i] = gv * (1.f + gam[b * ldg + u]) * d_elu_grad_from_out(av);
    dgam[b * ldg + u] = gv * av;
    dbet[b * ldg + u] = gv;
  }
}
// batch-major style [B,T,ST] <-> time-major [T,B,ST]
__global__ void style_time_major_k(ZeggsDecDims d, const float* style, float* stm) {
  long n = (long)d.T * d.B * d.ST;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int c = (int)(i % d.ST);
    long r = i / d.ST;
    int b = (int)(r % d.B), t = (int)(r / d.B);
    stm[i] = style[((long)b * d.T + t) * d.ST + c];
  }
}
__global__ void style_grad_from_time_major_k(ZeggsDecDims d, const float* dstm, float* dstyle) {
  long n = (long)d.T * d.B * d.ST;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int c = (int)(i % d.ST);
    long r = i / d.ST;
    int b = (int)(r % d.B), t = (int)(r / d.B);
    dstyle[((long)b * d.T + t) * d.ST + c] = t == 0 ? 0.f : dstm[i];
  }
}
__global__ void add_style0_grad_k(ZeggsDecDims d, const float* dcse_in, float* dstyle) {
  long n = (long)d.B * d.ST;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int c = (int)(i % d.ST);
    long b = i / d.ST;
    dstyle[(b * d.T) * d.ST + c] += dcse_in[b * (d.PI + d.ST) + d.PI + c];
  }
}

// weight gradients of the recurrent part for the steps t_lo..t_hi: contraction over the flattened (t, b) rows
// compact != 0 (fast path): DH0 / DH1 hold only the n rows of the hidden-side gate gradients, [T][B][H]; their r, z rows
// are the r, z rows of DI0 / DI1.
// what: 1 = weight gradients (GEMMs) of layer2 and GRU layer 1, 4 = of GRU layer 0 and layer0 (the two halves of the decoder's
// slice of a flat gradient buffer in parameter order: the caller can all-reduce the first while the second is computed),
// 2 = the bias gradients (column sums); 7 = everything
int dec_recurrent_wgrads(const ZeggsDecDims& d, const DecWs& w, const ZeggsDecGrads* G, int t_lo, int t_hi, float beta,
                         int compact, hipStream_t s, int what = 7) {
  const int B = d.B, H = d.H, GL = w.GL, XD = w.XD, POL = w.POL;
  const long sG = (long)B * GL, sH = (long)B * H, s3 = 3 * sH, sY = (long)B * POL;
  const int M = (t_hi - t_lo + 1) * B;
  const long o = t_lo;
  if (d.film) {
    const long sg = (long)B * 2 * H, sS = (long)B * d.ST;
    if (what & 1) ZTRY(gemm_tn(w.DY + o * sY, POL, w.F2 + o * sH, H, G->l3_w, H, M, d.PO, H, beta, s));
    if (what & 2) ZTRY(k_colsum(G->l3_b, w.DY + o * sY, M, d.PO, POL, beta, s));
    if (what & 1) ZTRY(gemm_tn(w.D2 + o * sH, H, w.H1 + o * sH, H, G->l2_w, H, M, H, H, beta, s));
    if (what & 2) ZTRY(k_colsum(G->l2_b, w.D2 + o * sH, M, H, H, beta, s));
    if (what & 1) ZTRY(gemm_tn(w.DGAM + o * sg, 2 * H, w.STm + o * sS, d.ST, G->g_w, d.ST, M, 2 * H, d.ST, beta, s));
    if (what & 2) ZTRY(k_colsum(G->g_b, w.DGAM + o * sg, M, 2 * H, 2 * H, beta, s));
    if (what & 1) ZTRY(gemm_tn(w.DBET + o * sg, 2 * H, w.STm + o * sS, d.ST, G->be_w, d.ST, M, 2 * H, d.ST, beta, s));
    if (what & 2) ZTRY(k_colsum(G->be_b, w.DBET + o * sg, M, 2 * H, 2 * H, beta, s));
  } else {
    if ((what & 3) == 3) ZTRY(gemm_tn_bias(w.DY + o * sY, POL, w.H1 + o * sH, H, G->l2_w, H, M, d.PO, H, beta, G->l2_b, s));
    else {
    if (what & 1) ZTRY(gemm_tn(w.DY + o * sY, POL, w.H1 + o * sH, H, G->l2_w, H, M, d.PO, H, beta, s));
    if (what & 2) ZTRY(k_colsum(G->l2_b, w.DY + o * sY, M, d.PO, POL, beta, s));
    }
  }
  // a weight-gradient product and the bias column sums of the same dy: ONE launch where both are asked for in this call and the
  // direct kernel takes the product (gemm_tn_bias: round 5, the sums were a dozen launches of 4-18 workgroups between the products)
  auto tn = [&](int gbit, const float* dy, long lddy, const float* x, long ldx, float* dW, long lddw, int N, int K, float* db) -> int {
    if ((what & gbit) && (what & 2)) return gemm_tn_bias(dy, lddy, x, ldx, dW, lddw, M, N, K, beta, db, s);
    if (what & gbit) ZTRY(gemm_tn(dy, lddy, x, ldx, dW, lddw, M, N, K, beta, s));
    if (what & 2) ZTRY(k_colsum(db, dy, M, N, lddy, beta, s));
    return 0;
  };
  // option "wgrad_order" (A/B, round 6): where the biggest product (dW_ih0, 0.8 ms of the second queue's 3.3) stands among the
  // others -- 0: parameter order (shipped), 1: first of its group, in front of layer 1's too when both groups are in this call,
  // 2: last of all
  auto ih0 = [&]() -> int { return tn(4, w.DI0 + o * s3, 3 * H, w.Gin + o * sG, GL, G->w_ih0, H + XD, 3 * H, H + XD, G->b_ih0); };
  if (g_wgrad_order == 1) ZTRY(ih0());
  ZTRY(tn(1, w.DI1 + o * s3, 3 * H, w.H0 + o * sH, H, G->w_ih1, H, 3 * H, H, G->b_ih1));
  if (compact) {
    ZTRY(tn(1, w.DI1 + o * s3, 3 * H, w.H1 + (o - 1) * sH, H, G->w_hh1, H, 2 * H, H, G->b_hh1));
    ZTRY(tn(1, w.DH1 + o * sH, H, w.H1 + (o - 1) * sH, H, G->w_hh1 + 2L * H * H, H, H, H, G->b_hh1 + 2 * H));
  } else {
    ZTRY(tn(1, w.DH1 + o * s3, 3 * H, w.H1 + (o - 1) * sH, H, G->w_hh1, H, 3 * H, H, G->b_hh1));
  }
  if (g_wgrad_order == 0) ZTRY(ih0());
  if (compact) {
    ZTRY(tn(4, w.DI0 + o * s3, 3 * H, w.H0 + (o - 1) * sH, H, G->w_hh0, H, 2 * H, H, G->b_hh0));
    ZTRY(tn(4, w.DH0 + o * sH, H, w.H0 + (o - 1) * sH, H, G->w_hh0 + 2L * H * H, H, H, H, G->b_hh0 + 2 * H));
  } else {
    ZTRY(tn(4, w.DH0 + o * s3, 3 * H, w.H0 + (o - 1) * sH, H, G->w_hh0, H, 3 * H, H, G->b_hh0));
  }
  ZTRY(tn(4, w.D0 + o * sH, H, w.Gin + o * sG + H, GL, G->l0_w, XD, H, XD, G->l0_b));
  if (g_wgrad_order == 2) ZTRY(ih0());
  return 0;
}

// Side stream (lowest priority) + events for the overlapped weight-gradient GEMMs, one set per device.
struct SideStream { hipStream_t s; hipEvent_t done; };
int side_stream(SideStream** out) {
  static SideStream pool[16];
  static bool ready[16] = {};
  int dev = 0;
  ZCHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16, "decoder bwd: unsupported device index");
  if (!ready[dev]) {
    int lo = 0, hi = 0;
    ZCHECK(hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess, "hipDeviceGetStreamPriorityRange failed");
    ZCHECK(hipStreamCreateWithPriority(&pool[dev].s, hipStreamNonBlocking, lo) == hipSuccess, "side stream creation failed");
    ZCHECK(hipEventCreateWithFlags(&pool[dev].done, hipEventDisableTiming) == hipSuccess, "event creation failed");
    ready[dev] = true;
  }
  *out = &pool[dev];
  return 0;
}

// `to` continues behind what `from` holds now.  The event of such a hand-over: stream-ordered use only (record on one stream, wait
// on another, both enqueued before this returns), so one event per device and hand-over point (`which`: 0 / 1 the deferred weight
// gradients of the recurrent layers / the CellStateEncoder, 2 a chunk of the stage sweep) is enough; events carry no data and are
// created once
int stream_fork(hipStream_t from, hipStream_t to, int which) {
  static hipEvent_t pool[16][3];
  static bool ready[16][3] = {};
  int dev = 0;
  ZCHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16, "decoder bwd: unsupported device index");
  if (!ready[dev][which]) {
    ZCHECK(hipEventCreateWithFlags(&pool[dev][which], hipEventDisableTiming) == hipSuccess, "event creation failed");
    ready[dev][which] = true;
  }
  ZCHECK(hipEventRecord(pool[dev][which], from) == hipSuccess, "hipEventRecord failed");
  ZCHECK(hipStreamWaitEvent(to, pool[dev][which], 0) == hipSuccess, "hipStreamWaitEvent failed");
  return 0;
}

inline dim3 g1(long n) { long g = (n + 255) / 256; return dim3((unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g))); }

// ------------------------------------------------------------------ the head of a rollout, piece by piece
// frame 0 of the outputs, the CellStateEncoder's input and the pose part of x_1 (the caller checks the launch)
void dec_init(const DecCtx& c, const DecFwdIO& io, float* gin1) {
  hipLaunchKernelGGL(dec_init_k, dim3(c.d.B), dim3(256), 0, c.s, c.d, *c.st, io.pose0, io.rpos0, io.rrot0, io.gaze, io.style, io.pose,
                     io.rpos, io.rrot, c.w.cse_in, gin1, c.w.GL);
}
// speech / style columns of x_t, t = t0 .. t0 + nt - 1, in the canonical input rows (ring: the 2-slot ring of inference)
int dec_fill_cond(const DecCtx& c, const DecFwdIO& io, int t0, int nt, int ring) {
  const ZeggsDecDims& d = c.d;
  hipLaunchKernelGGL(dec_fill_cond_k, g1((long)nt * d.B * (d.SP + d.ST)), dim3(256), 0, c.s, d, io.speech, io.style, c.w.Gin, c.w.GL,
                     t0, nt, (long)d.B * c.w.GL, ring);
  ZLAUNCH_CHECK("dec_fill_cond");
  return 0;
}
int gemm_nt_item(const GemmNtItem& i, int M, hipStream_t s) {
  return gemm_nt(i.x, i.ldx, i.W, i.ldw, i.y, i.ldy, i.bias, M, i.N, i.K, i.act, 0.f, s);
}
// hid_1 = ELU(W0 x_1 + b0) in slot 1 of the canonical input rows
GemmNtItem dec_hid1_item(const DecCtx& c) {
  float* gin1 = c.w.Gin + (long)c.d.B * c.w.GL;
  return GemmNtItem{gin1 + c.d.H, c.w.GL, c.P->l0_w, c.w.XD, gin1, c.w.GL, c.P->l0_b, c.d.H, c.w.XD, ACT_ELU};
}
int dec_hid1(const DecCtx& c) { return gemm_nt_item(dec_hid1_item(c), c.d.B, c.s); }
// the CellStateEncoder's four products: two layers, then the halves of the last one, which are the initial states of the GRU layers
struct CseItems { GemmNtItem it[4]; };
CseItems dec_cse_items(const DecCtx& c, float* h0_dst, float* h1_dst) {
  const ZeggsDecParams* P = c.P; const DecWs& w = c.w;
  const int H = c.d.H, CI = c.d.PI + c.d.ST;
  return CseItems{{{w.cse_in, CI, P->c0_w, CI, w.cse_a, H, P->c0_b, H, CI, ACT_ELU},
                   {w.cse_a, H, P->c1_w, H, w.cse_b, H, P->c1_b, H, H, ACT_ELU},
                   {w.cse_b, H, P->c2_w, H, h0_dst, H, P->c2_b, H, H, ACT_NONE},
                   {w.cse_b, H, P->c2_w + (long)H * H, H, h1_dst, H, P->c2_b + H, H, H, ACT_NONE}}};
}
int dec_cse(const DecCtx& c, float* h0_dst, float* h1_dst) {
  const CseItems q = dec_cse_items(c, h0_dst, h1_dst);
  for (const GemmNtItem& i : q.it) ZTRY(gemm_nt_item(i, c.d.B, c.s));
  return 0;
}
// frame 0, then the recurrent state before step 1: given (resumed rollout) or the CellStateEncoder's
int dec_head(const DecCtx& c, const DecFwdIO& io, const float* h_in) {
  const long sH = (long)c.d.B * c.d.H;
  dec_init(c, io, c.w.Gin + (long)c.d.B * c.w.GL);
  ZLAUNCH_CHECK("dec_init");
  if (!h_in) return dec_cse(c, c.w.H0, c.w.H1);
  ZTRY(k_copy(c.w.H0, h_in, sH, c.s));
  return k_copy(c.w.H1, h_in + sH, sH, c.s);
}
// The same head in front of the persistent training rollout (train_persistent.hip), five launches instead of ten (round 6; option
// "tp_prologue", default on): [dec_init | dec_fill_cond | tp_cond] in one, [CellStateEncoder layer 0 | hid_1 | the step-1 pose
// product] in one, CellStateEncoder layer 1, the two halves of its last layer in one, and the rollout's own operand fragments
// (dec_tp_run) -- every one of them was launch latency on an idle chip
int dec_head_prologue(const DecCtx& c, const DecFwdIO& io, bool zeroed) {
  ZTRY(dec_tp_prologue(c, io, zeroed));
  const CseItems q = dec_cse_items(c, c.w.H0, c.w.H1);
  const GemmNtItem l1[3] = {q.it[0], dec_hid1_item(c), dec_tp_p1x_item(c)};
  ZTRY(gemm_nt_multi(l1, 3, c.d.B, c.s));
  ZTRY(gemm_nt_item(q.it[1], c.d.B, c.s));
  return gemm_nt_multi(q.it + 2, 2, c.d.B, c.s);
}
// training: the speech / style columns of every step (unless the prologue launch has filled them) and, with FiLM, the modulation
// vectors of every step in two GEMMs over the time-major style
int dec_train_inputs(const DecCtx& c, const DecFwdIO& io, bool cond_filled) {
  const ZeggsDecDims& d = c.d; const ZeggsDecParams* P = c.P; DecWs& w = c.w; hipStream_t s = c.s;
  if (!cond_filled) ZTRY(dec_fill_cond(c, io, 1, d.T - 1, 0));
  if (!d.film) return 0;
  ZCHECK(P->l3_w && P->l3_b && P->g_w && P->g_b && P->be_w && P->be_b, "decoder: film parameters missing");
  hipLaunchKernelGGL(style_time_major_k, g1((long)d.T * d.B * d.ST), dim3(256), 0, s, d, io.style, w.STm);
  ZLAUNCH_CHECK("style_time_major");
  ZTRY(gemm_nt(w.STm, d.ST, P->g_w, d.ST, w.GAM, 2 * d.H, P->g_b, d.T * d.B, 2 * d.H, d.ST, ACT_NONE, 0.f, s));
  return gemm_nt(w.STm, d.ST, P->be_w, d.ST, w.BET, 2 * d.H, P->be_b, d.T * d.B, 2 * d.H, d.ST, ACT_NONE, 0.f, s);
}

// ------------------------------------------------------------------ the paths of a rollout, in the order they are tried.  A persistent
// sweep that gave up on its first use leaves *done false (the kernel is then disabled for this process): the next path redoes the rollout.
// batch-1 inference: the weight-stationary persistent kernel (one launch for all frames, decode_persistent.hip)
int fwd_persistent_decode(const DecCtx& c, const DecFwdIO& io, unsigned* status, bool* done) {
  const ZeggsDecDims& d = c.d; DecWs& w = c.w;
  SweepKernel& k = g_sweep_kernels[SWEEP_DECODE];
  if (!(dec_persistent_supported(d, w) && k.may_run(c.s))) return 0;
  const long fin = (long)((d.T - 1) & 1) * d.B * d.H;
  ZTRY(dec_fill_cond(c, io, 1, 1, 1));
  ZTRY(dec_hid1(c));
  ZTRY(dec_fast_merge_prep(c));
  dec_timing_mark(0, c.s);
  ZTRY(dec_persistent_run(c, io, w.Gin + (long)d.B * w.GL, w.H0, w.H1, w.H0 + fin, w.H1 + fin, k.status_arg(status)));
  dec_timing_mark(1, c.s);
  return k.settle(c.s, dp_errword(w), done);
}
// training, batch <= 64: the forward rollout as one persistent launch (train_persistent.hip)
int fwd_persistent_rollout(const DecCtx& c, const DecFwdIO& io, bool prepared, bool prologue_done, unsigned* status, bool* done) {
  SweepKernel& k = g_sweep_kernels[SWEEP_ROLLOUT];
  if (!prologue_done) ZTRY(dec_hid1(c));
  if (!prepared) ZTRY(dec_tp_pack(c));
  dec_timing_mark(0, c.s);
  ZTRY(dec_tp_run(c, io, prepared, k.status_arg(status), prologue_done));
  dec_timing_mark(1, c.s);
  return k.settle(c.s, tp_errword(c.w), done);
}
// the stage kernels, three or four launches per step (decoder_fast.hip)
int fwd_stage_launches(const DecCtx& c, const DecFwdIO& io, int training) {
  if (!training && c.d.T > 1) ZTRY(dec_fill_cond(c, io, 1, 1, 1));
  ZTRY(dec_fast_pack_fwd(c));
  return dec_fast_fwd_steps(c, io, training);
}
// generic GEMMs and elementwise kernels, step by step
int fwd_generic_steps(const DecCtx& c, const DecFwdIO& io, int training) {
  const ZeggsDecDims& d = c.d; const ZeggsDecParams* P = c.P; const ZeggsDecStats* st = c.st; DecWs& w = c.w; hipStream_t s = c.s;
  const int B = d.B, T = d.T, H = d.H, GL = w.GL, XD = w.XD;
  const long sG = (long)B * GL, sH = (long)B * H;
  auto slot = [&](int t) { return training ? t : (t & 1); };
  for (int t = 1; t < T; ++t) {
    float* gin = w.Gin + slot(t) * sG;
    float* gin_next = (t + 1 < T) ? w.Gin + slot(t + 1) * sG : nullptr;
    const float *h0p = w.H0 + slot(t - 1) * sH, *h1p = w.H1 + slot(t - 1) * sH;
    float *h0 = w.H0 + slot(t) * sH, *h1 = w.H1 + slot(t) * sH;
    if (!training) ZTRY(dec_fill_cond(c, io, t, 1, 1));
    // hid = ELU(layer0(x))   [film: modulated by the style]
    const float *gam = nullptr, *bet = nullptr;
    if (d.film) {
      if (!training) {   // ring path: this step's modulation vectors from style[:, t]
        ZCHECK(P->l3_w && P->l3_b && P->g_w && P->g_b && P->be_w && P->be_b, "decoder: film parameters missing");
        ZTRY(gemm_nt(io.style + (long)t * d.ST, (long)T * d.ST, P->g_w, d.ST, w.GAM, 2 * H, P->g_b, B, 2 * H, d.ST, ACT_NONE,
                     0.f, s));
        ZTRY(gemm_nt(io.style + (long)t * d.ST, (long)T * d.ST, P->be_w, d.ST, w.BET, 2 * H, P->be_b, B, 2 * H, d.ST, ACT_NONE,
                     0.f, s));
      }
      gam = w.GAM + (training ? (long)t * B * 2 * H : 0);
      bet = w.BET + (training ? (long)t * B * 2 * H : 0);
      float* a0 = w.A0 + slot(t) * sH;
      ZTRY(gemm_nt(gin + H, GL, P->l0_w, XD, a0, H, P->l0_b, B, H, XD, ACT_ELU, 0.f, s));
      hipLaunchKernelGGL(film_fwd_k, g1(sH), dim3(256), 0, s, gin, (long)GL, a0, gam, bet, (long)2 * H, B, H);
    } else {
      ZTRY(gemm_nt(gin + H, GL, P->l0_w, XD, gin, GL, P->l0_b, B, H, XD, ACT_ELU, 0.f, s));
    }
    // GRU layer 0
    ZTRY(gemm_nt(gin, GL, P->w_ih0, H + XD, w.gi, 3 * H, P->b_ih0, B, 3 * H, H + XD, ACT_NONE, 0.f, s));
    ZTRY(gemm_nt(h0p, H, P->w_hh0, H, w.gh, 3 * H, P->b_hh0, B, 3 * H, H, ACT_NONE, 0.f, s));
    const long o = (long)t * sH;
    hipLaunchKernelGGL(gru_gate_fwd_k, g1(sH), dim3(256), 0, s, w.gi, w.gh, h0p, h0,
                       training ? (f4*)w.GT0 + o : (f4*)nullptr, B, H);
    // GRU layer 1
    ZTRY(gemm_nt(h0, H, P->w_ih1, H, w.gi, 3 * H, P->b_ih1, B, 3 * H, H, ACT_NONE, 0.f, s));
    ZTRY(gemm_nt(h1p, H, P->w_hh1, H, w.gh, 3 * H, P->b_hh1, B, 3 * H, H, ACT_NONE, 0.f, s));
    hipLaunchKernelGGL(gru_gate_fwd_k, g1(sH), dim3(256), 0, s, w.gi, w.gh, h1p, h1,
                       training ? (f4*)w.GT1 + o : (f4*)nullptr, B, H);
    // output projection + pose integration
    if (d.film) {
      float *a2 = w.A2 + slot(t) * sH, *f2 = w.F2 + slot(t) * sH;
      ZTRY(gemm_nt(h1, H, P->l2_w, H, a2, H, P->l2_b, B, H, H, ACT_ELU, 0.f, s));
      hipLaunchKernelGGL(film_fwd_k, g1(sH), dim3(256), 0, s, f2, (long)H, a2, gam + H, bet + H, (long)2 * H, B, H);
      ZTRY(gemm_nt(f2, H, P->l3_w, H, w.Y, w.POL, P->l3_b, B, d.PO, H, ACT_NONE, 0.f, s));
    } else {
      ZTRY(gemm_nt(h1, H, P->l2_w, H, w.Y, w.POL, P->l2_b, B, d.PO, H, ACT_NONE, 0.f, s));
    }
    hipLaunchKernelGGL(dec_devec_k, dim3(B), dim3(256), 0, s, d, *st, w.Y, w.POL, io.gaze, io.pose, io.rpos, io.rrot,
                       gin_next, GL, t);
    ZLAUNCH_CHECK("dec_step");
  }
  return 0;
}

// ------------------------------------------------------------------ the pieces of the backward
// the zero state a sweep starts from: the carries and (with_dx) the frame-0 slot of DX, unused but read by the scatter
int dec_bwd_zero_state(const DecCtx& c, bool with_dx) {
  const ZeggsDecDims& d = c.d;
  ZTRY(k_fill(c.w.dH0c, (long)d.B * d.H, 0.f, c.s));
  ZTRY(k_fill(c.w.dH1c, (long)d.B * d.H, 0.f, c.s));
  ZTRY(k_fill(c.w.carry, (long)2 * d.B * 8, 0.f, c.s));
  if (with_dx) ZTRY(k_fill(c.w.DX, (long)d.B * c.w.XD, 0.f, c.s));
  return 0;
}
// The stage launches (decoder_fast.hip).  The sweep is a chain of small dependent launches that leaves most of the chip idle; with
// option "bwd_chunks" > 1 the weight-gradient GEMMs of the steps already swept run beside it on a low-priority stream, chunk by
// chunk: *ss is then the side stream the caller joins.
int bwd_stage_sweep(const DecCtx& c, const DecBwdIO& io, const ZeggsDecGrads* G, float gb, SideStream** ss) {
  const int T = c.d.T;
  ZTRY(dec_fast_pack_bwd(c));
  const int nch = g_bwd_chunks < T - 1 ? g_bwd_chunks : T - 1;
  if (nch > 1) ZTRY(side_stream(ss));
  for (int k = 0; k < nch; ++k) {
    const int t_hi = T - 1 - (int)((long)(T - 1) * k / nch), t_lo = T - (int)((long)(T - 1) * (k + 1) / nch);
    ZTRY(dec_fast_bwd_steps(c, io, t_hi, t_lo));
    if (nch > 1) {
      ZTRY(stream_fork(c.s, (*ss)->s, 2));
      ZTRY(dec_recurrent_wgrads(c.d, c.w, G, t_lo, t_hi, k == 0 ? gb : 1.f, 1, (*ss)->s));
    }
  }
  if (nch > 1) ZCHECK(hipEventRecord((*ss)->done, (*ss)->s) == hipSuccess, "hipEventRecord failed");
  return 0;
}
// generic GEMMs and elementwise kernels, step by step
int bwd_generic_steps(const DecCtx& c, const DecBwdIO& io) {
  const ZeggsDecDims& d = c.d; const ZeggsDecParams* P = c.P; const ZeggsDecStats* st = c.st; DecWs& w = c.w; hipStream_t s = c.s;
  const int B = d.B, T = d.T, H = d.H, GL = w.GL, XD = w.XD, POL = w.POL;
  const long sG = (long)B * GL, sH = (long)B * H, s3 = 3 * sH;
  for (int t = T - 1; t >= 1; --t) {
    const float* gin = w.Gin + t * sG;
    const long o = (long)t * sH;
    float* dy = w.DY + (long)t * B * POL;
    const float* dxn = (t + 1 < T) ? w.DX + (long)(t + 1) * B * XD : nullptr;
    hipLaunchKernelGGL(dec_devec_bwd_k, dim3(B), dim3(256), 0, s, d, *st, io.dpose, io.drpos, io.drrot, dxn, XD, io.gaze,
                       io.pose, io.rpos, io.rrot, w.carry, dy, POL, t);
    ZLAUNCH_CHECK("dec_devec_bwd");
    // dH1 total = dy W2 + carried   [film: through layer3, the modulation and layer2]
    if (d.film) {
      const long og = (long)t * B * 2 * H;
      ZTRY(gemm_nn(dy, POL, P->l3_w, H, w.dF2, H, B, d.PO, H, 0.f, s));
      hipLaunchKernelGGL(film_bwd_k, g1(sH), dim3(256), 0, s, w.dF2, (long)H, w.A2 + o, w.GAM + og + H, (long)2 * H,
                         w.D2 + o, w.DGAM + og + H, w.DBET + og + H, B, H);
      ZTRY(gemm_nn(w.D2 + o, H, P->l2_w, H, w.dH1c, H, B, H, H, 1.f, s));
    } else {
      ZTRY(gemm_nn(dy, POL, P->l2_w, H, w.dH1c, H, B, d.PO, H, 1.f, s));
    }
    hipLaunchKernelGGL(gru_gate_bwd_k, g1(sH), dim3(256), 0, s, w.dH1c, (const f4*)w.GT1 + o,
                       w.H1 + o - sH, w.DI1 + t * s3, w.DH1 + t * s3, w.t0, B, H);
    // t0 = dH1 * z (direct path); dH1c <- t0 + DH1 W_hh1 ; dH0 total = dH0c + DI1 W_ih1
    ZTRY(k_copy(w.dH1c, w.t0, sH, s));
    ZTRY(gemm_nn(w.DH1 + t * s3, 3 * H, P->w_hh1, H, w.dH1c, H, B, 3 * H, H, 1.f, s));
    ZTRY(gemm_nn(w.DI1 + t * s3, 3 * H, P->w_ih1, H, w.dH0c, H, B, 3 * H, H, 1.f, s));
    hipLaunchKernelGGL(gru_gate_bwd_k, g1(sH), dim3(256), 0, s, w.dH0c, (const f4*)w.GT0 + o,
                       w.H0 + o - sH, w.DI0 + t * s3, w.DH0 + t * s3, w.t0, B, H);
    ZTRY(k_copy(w.dH0c, w.t0, sH, s));
    ZTRY(gemm_nn(w.DH0 + t * s3, 3 * H, P->w_hh0, H, w.dH0c, H, B, 3 * H, H, 1.f, s));
    // dGin = DI0 W_ih0 -> [dhid | dx]
    ZTRY(gemm_nn(w.DI0 + t * s3, 3 * H, P->w_ih0, H + XD, w.dGin, GL, B, 3 * H, H + XD, 0.f, s));
    if (d.film) {
      const long og = (long)t * B * 2 * H;
      hipLaunchKernelGGL(film_bwd_k, g1(sH), dim3(256), 0, s, w.dGin, (long)GL, w.A0 + o, w.GAM + og, (long)2 * H,
                         w.D0 + o, w.DGAM + og, w.DBET + og, B, H);
    } else {
      hipLaunchKernelGGL(elu_bwd_rows_k, g1(sH), dim3(256), 0, s, w.D0 + o, w.dGin, gin, B, H, GL);
    }
    // dx_t = dGin[:, H:] + D0 W0
    float* dx = w.DX + (long)t * B * XD;
    hipLaunchKernelGGL(copy_cols_k, g1((long)B * XD), dim3(256), 0, s, dx, (long)XD, w.dGin, (long)GL, H, XD, B);
    ZLAUNCH_CHECK("dec_bwd_step");
    ZTRY(gemm_nn(w.D0 + o, H, P->l0_w, XD, dx, XD, B, H, XD, 1.f, s));
  }
  return 0;
}
// CellStateEncoder backward: dH0c / dH1c are the grads wrt its two output halves.  The input-gradient chain (four batch-sized
// products, the ELU' factors in their epilogues) is what the caller's next kernels wait for (dstyle -> the style encoder's
// backward): it goes first; the weight / bias gradients need only its intermediates and, with deferred GEMMs (gs != null), join
// the recurrent layers' on the weight-gradient stream.
int dec_cse_bwd(const DecCtx& c, const ZeggsDecGrads* G, float gb, hipStream_t gs) {
  const ZeggsDecParams* P = c.P; DecWs& w = c.w; hipStream_t s = c.s;
  const int B = c.d.B, H = c.d.H, CI = c.d.PI + c.d.ST;
  // out = [H0_init | H1_init] = cse_b W2^T + b2
  float* db = w.t0;                       // [B,H] grad wrt cse_b
  float* da = w.t0 + (long)B * H;         // [B,H] grad wrt cse_a
  ZTRY(gemm_nn(w.dH0c, H, P->c2_w, H, db, H, B, H, H, 0.f, s));
  ZTRY(gemm_nn_actbwd(w.dH1c, H, P->c2_w + (long)H * H, H, db, H, B, H, H, 1.f, w.cse_b, H, ACT_ELU, s));
  ZTRY(gemm_nn_actbwd(db, H, P->c1_w, H, da, H, B, H, H, 0.f, w.cse_a, H, ACT_ELU, s));
  ZTRY(gemm_nn(da, H, P->c0_w, CI, w.t1, CI, B, H, CI, 0.f, s));   // t1 = d cse_in [B, PI+ST]
  if (gs) ZTRY(stream_fork(s, gs, 1));
  else gs = s;
  ZTRY(gemm_tn(w.dH0c, H, w.cse_b, H, G->c2_w, H, B, H, H, gb, gs));
  ZTRY(gemm_tn(w.dH1c, H, w.cse_b, H, G->c2_w + (long)H * H, H, B, H, H, gb, gs));
  ZTRY(k_colsum(G->c2_b, w.dH0c, B, H, H, gb, gs));
  ZTRY(k_colsum(G->c2_b + H, w.dH1c, B, H, H, gb, gs));
  ZTRY(gemm_tn(db, H, w.cse_a, H, G->c1_w, H, B, H, H, gb, gs));
  ZTRY(k_colsum(G->c1_b, db, B, H, H, gb, gs));
  ZTRY(gemm_tn(da, H, w.cse_in, CI, G->c0_w, CI, B, H, CI, gb, gs));
  return k_colsum(G->c0_b, da, B, H, H, gb, gs);
}
// the gradients of the conditioning inputs: DX's speech / style columns, the style through FiLM's predictors, the style of frame 0
int dec_cond_grads(const DecCtx& c, float* dspeech, float* dstyle) {
  const ZeggsDecDims& d = c.d; const ZeggsDecParams* P = c.P; DecWs& w = c.w; hipStream_t s = c.s;
  const int B = d.B, T = d.T, H = d.H;
  hipLaunchKernelGGL(dec_scatter_cond_grad_k, g1((long)T * B * (d.SP + d.ST)), dim3(256), 0, s, d, w.DX, w.XD, dspeech, dstyle);
  if (d.film) {   // the style reaches the steps through the two predictors only
    const long M1 = (long)(T - 1) * B, sg = (long)B * 2 * H, sS = (long)B * d.ST;
    ZTRY(gemm_nn(w.DGAM + sg, 2 * H, P->g_w, d.ST, w.dSTm + sS, d.ST, (int)M1, 2 * H, d.ST, 0.f, s));
    ZTRY(gemm_nn(w.DBET + sg, 2 * H, P->be_w, d.ST, w.dSTm + sS, d.ST, (int)M1, 2 * H, d.ST, 1.f, s));
    hipLaunchKernelGGL(style_grad_from_time_major_k, g1((long)T * B * d.ST), dim3(256), 0, s, d, w.dSTm, dstyle);
  }
  hipLaunchKernelGGL(add_style0_grad_k, g1((long)B * d.ST), dim3(256), 0, s, d, w.t1, dstyle);
  ZLAUNCH_CHECK("dec_bwd_tail");
  return 0;
}

}  // namespace

extern "C" size_t zeggs_decoder_workspace_bytes(const ZeggsDecDims* d, int training) {
  Arena a(nullptr, 0);
  carve_dec(*d, training, a);
  return a.off + 256;
}

// every forward entry point: validation, carve, head, the paths in the order they are tried, the state after the last frame
static int decoder_fwd_impl(const ZeggsDecDims* dp, const ZeggsDecParams* P, const ZeggsDecStats* st, const DecFwdIO& io,
                            int training, const float* h_in, float* h_out, void* ws, size_t ws_bytes, void* stream,
                            const ZeggsDecCall* call) {
  const ZeggsDecDims& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  const bool fwd_prepared = call && (call->prepared & 1);
  unsigned* status = call ? call->status : nullptr;
  ZCHECK(d.PI == d.PO + 3, "decoder: pose_input_size must be pose_output_size + 3 (gaze)");
  ZCHECK(d.B >= 1 && d.T >= 1, "decoder: empty batch or sequence");
  Arena a(ws, ws_bytes);
  DecWs w = carve_dec(d, training, a);
  ZCHECK(a.ok(), "decoder: workspace too small (%zu < %zu)", ws_bytes, a.off);
  const DecCtx c{d, P, st, w, s};
  const long sH = (long)d.B * d.H;
  if (!training) ZTRY(k_fill(w.Gin, 2L * d.B * w.GL, 0.f, s));   // ring slots: pad columns must be finite (GEMV decode path)
  const bool fast = g_decoder_fast && dec_fast_supported(d);
  // training, batch <= 64: will the rollout run as one persistent launch?  Then its head is the five-launch prologue
  const bool tp_path = fast && training && dec_tp_supported(d, w) && g_sweep_kernels[SWEEP_ROLLOUT].may_run(s);
  const bool tp_pro = tp_path && g_tp_prologue && !h_in && d.T > 1 && !d.film;
  ZTRY(tp_pro ? dec_head_prologue(c, io, fwd_prepared) : dec_head(c, io, h_in));
  if (training && d.T > 1) ZTRY(dec_train_inputs(c, io, tp_pro));
  bool done = false;
  if (fast && !training) ZTRY(fwd_persistent_decode(c, io, status, &done));
  if (!done && tp_path) ZTRY(fwd_persistent_rollout(c, io, fwd_prepared, tp_pro, status, &done));
  if (!done && fast) ZTRY(fwd_stage_launches(c, io, training));
  else if (!done) ZTRY(fwd_generic_steps(c, io, training));
  if (h_out) {      // the state after the last frame (inference: its ring slot)
    const long last = (training ? d.T - 1 : (d.T - 1) & 1) * sH;
    ZTRY(k_copy(h_out, w.H0 + last, sH, s));
    ZTRY(k_copy(h_out + sH, w.H1 + last, sH, s));
  }
  return 0;
}

extern "C" int zeggs_decoder_fwd(const ZeggsDecDims* dp, const ZeggsDecParams* P, const ZeggsDecStats* st,
                                 const float* pose0, const float* rpos0, const float* rrot0, const float* gaze,
                                 const float* speech, const float* style, float* pose, float* rpos, float* rrot,
                                 int training, void* ws, size_t ws_bytes, void* stream) {
  const DecFwdIO io{pose0, rpos0, rrot0, gaze, speech, style, pose, rpos, rrot};
  return decoder_fwd_impl(dp, P, st, io, training, nullptr, nullptr, ws, ws_bytes, stream, nullptr);
}
extern "C" int zeggs_decoder_fwd_ex(const ZeggsDecDims* dp, const ZeggsDecParams* P, const ZeggsDecStats* st,
                                    const float* pose0, const float* rpos0, const float* rrot0, const float* gaze,
                                    const float* speech, const float* style, float* pose, float* rpos, float* rrot,
                                    int training, void* ws, size_t ws_bytes, void* stream, const ZeggsDecCall* call) {
  const DecFwdIO io{pose0, rpos0, rrot0, gaze, speech, style, pose, rpos, rrot};
  return decoder_fwd_impl(dp, P, st, io, training, nullptr, nullptr, ws, ws_bytes, stream, call);
}

// Chunked (streaming) decode: frame 0 of the chunk is the last frame already produced (its pose / root state come in as
// pose0 / rpos0 / rrot0), h_in [2,B,H] is the GRU state after that frame (NULL: first chunk, CellStateEncoder), h_out
// receives the state after the chunk's last frame.  Inference only (2-slot rings).
extern "C" int zeggs_decoder_fwd_state(const ZeggsDecDims* dp, const ZeggsDecParams* P, const ZeggsDecStats* st,
                                       const float* pose0, const float* rpos0, const float* rrot0, const float* gaze,
                                       const float* speech, const float* style, float* pose, float* rpos, float* rrot,
                                       const float* h_in, float* h_out, void* ws, size_t ws_bytes, void* stream) {
  const DecFwdIO io{pose0, rpos0, rrot0, gaze, speech, style, pose, rpos, rrot};
  return decoder_fwd_impl(dp, P, st, io, 0, h_in, h_out, ws, ws_bytes, stream, nullptr);
}
// the same with per-call controls: ZeggsDecCall.status receives the give-up bit of the B = 1 persistent kernel, so that a caller
// that feeds the returned state into the NEXT chunk (zeggs/stream.py) can notice a rollout that did not complete and redo it
extern "C" int zeggs_decoder_fwd_state_ex(const ZeggsDecDims* dp, const ZeggsDecParams* P, const ZeggsDecStats* st,
                                          const float* pose0, const float* rpos0, const float* rrot0, const float* gaze,
                                          const float* speech, const float* style, float* pose, float* rpos, float* rrot,
                                          const float* h_in, float* h_out, void* ws, size_t ws_bytes, void* stream,
                                          const ZeggsDecCall* call) {
  const DecFwdIO io{pose0, rpos0, rrot0, gaze, speech, style, pose, rpos, rrot};
  return decoder_fwd_impl(dp, P, st, io, 0, h_in, h_out, ws, ws_bytes, stream, call);
}

// ---------------------------------------------------------------- batch decode: many clips per weight-stationary rollout
// N rows of inference advance together, chunk by chunk, on the training rollout's sweep (train_persistent.hip, inference form): the
// weights stay in the register files and a step costs about what ONE row costs the B = 1 kernel.  The rollout is chunked and
// resumable exactly like zeggs_decoder_fwd_state (frame 0 of a chunk = the last frame already produced, h_in / h_out [2,B,H]); a
// row starts a new clip at a chunk boundary by taking its h_in rows from zeggs_decoder_state_init.  Reached only through these
// entry points: what the existing ones dispatch to is unchanged.
static thread_local int t_batch_last_path = 0;
extern "C" int zeggs_decoder_batch_last_path(void) { return t_batch_last_path; }

extern "C" size_t zeggs_decoder_batch_workspace_bytes(const ZeggsDecDims* d) {
  Arena a(nullptr, 0);
  carve_dec_batch(*d, a);
  return a.off + 256;
}

// bit 0: the sweep takes these dimensions; bit 1 (with bit 0): its GRU packs are 4-row tiles
static int batch_sweep_mask(const ZeggsDecDims& d, const DecWs& w) {
  const SweepKernel& k = g_sweep_kernels[SWEEP_ROLLOUT];
  if (!(g_decoder_fast && dec_fast_supported(d) && k.enabled && k.state != 0 && dec_tb_supported(d, w))) return 0;
  return 1 | (dec_tb_t4(w) ? 2 : 0);
}

extern "C" int zeggs_decoder_batch_prepare(const ZeggsDecDims* dp, const ZeggsDecParams* P, const ZeggsDecStats* st, void* ws,
                                           size_t ws_bytes, void* stream) {
  const ZeggsDecDims& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  Arena a(ws, ws_bytes);
  DecWs w = carve_dec_batch(d, a);
  ZCHECK(a.ok(), "decoder batch prepare: workspace too small (%zu < %zu)", ws_bytes, a.off);
  const int mask = batch_sweep_mask(d, w);
  if (!mask) return 0;
  const DecCtx c{d, P, st, w, s};
  ZTRY(dec_tp_pack(c, (mask & 2) ? 1 : 0));
  return mask;
}

// the CellStateEncoder alone: GRU state [2,B,H] a clip starts from, given its first pose and the gaze target / style of frame 0
extern "C" int zeggs_decoder_state_init(const ZeggsDecDims* dp, const ZeggsDecParams* P, const ZeggsDecStats* st,
                                        const float* pose0, const float* rpos0, const float* rrot0, const float* gaze0,
                                        const float* style0, float* h_out, void* ws, size_t ws_bytes, void* stream) {
  ZeggsDecDims d = *dp;
  d.T = 1;                                        // gaze0 [B,3], style0 [B,ST]: one frame per row
  ZCHECK(d.PI == d.PO + 3, "decoder: pose_input_size must be pose_output_size + 3 (gaze)");
  ZCHECK(d.B >= 1, "decoder: empty batch");
  Arena a(ws, ws_bytes);
  DecWs w = carve_dec(d, 0, a);
  ZCHECK(a.ok(), "decoder state init: workspace too small (%zu < %zu)", ws_bytes, a.off);
  const DecCtx c{d, P, st, w, (hipStream_t)stream};
  // (frame-0 copies of the outputs land in step scratch: Y [B,POL], gi [B,3H])
  const DecFwdIO io{pose0, rpos0, rrot0, gaze0, nullptr, style0, w.Y, w.gi, w.gi + 4L * d.B};
  dec_init(c, io, w.Gin);
  ZLAUNCH_CHECK("dec_init");
  return dec_cse(c, h_out, h_out + (long)d.B * d.H);
}

// mode 0: the sweep (first use on a process validated by a device sync and the error word -- never inside a stream capture --,
// later give-ups OR ZEGGS_GAVE_UP_BATCH_FWD into call->status and the caller redoes the chunk with mode 1); dimensions the sweep
// does not take, a disabled sweep, a failed validation: the stage launches.  mode 1: the stage launches.
extern "C" int zeggs_decoder_fwd_batch(const ZeggsDecDims* dp, const ZeggsDecParams* P, const ZeggsDecStats* st,
                                       const float* pose0, const float* rpos0, const float* rrot0, const float* gaze,
                                       const float* speech, const float* style, float* pose, float* rpos, float* rrot,
                                       const float* h_in, float* h_out, void* ws, size_t ws_bytes, void* stream,
                                       const ZeggsDecCall* call, int mode) {
  const ZeggsDecDims& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  ZCHECK(d.PI == d.PO + 3, "decoder: pose_input_size must be pose_output_size + 3 (gaze)");
  ZCHECK(d.B >= 1 && d.T >= 2, "decoder batch: empty batch or chunk");
  ZCHECK(h_in && h_out, "decoder batch: h_in and h_out are required (zeggs_decoder_state_init gives the state a clip starts from)");
  Arena a(ws, ws_bytes);
  DecWs w = carve_dec_batch(d, a);
  ZCHECK(a.ok(), "decoder batch: workspace too small (%zu < %zu)", ws_bytes, a.off);
  const DecCtx c{d, P, st, w, s};
  const DecFwdIO io{pose0, rpos0, rrot0, gaze, speech, style, pose, rpos, rrot};
  SweepKernel& tpk = g_sweep_kernels[SWEEP_ROLLOUT];
  const int mask = mode == 0 && tpk.may_run(s) ? batch_sweep_mask(d, w) : 0;
  if (mask) {
    ZTRY(k_fill(w.Gin, 2L * d.B * w.GL, 0.f, s));
    dec_init(c, io, w.Gin + (long)d.B * w.GL);
    ZTRY(dec_fill_cond(c, io, 1, 1, 1));
    ZTRY(dec_hid1(c));
    if (!(call && (call->prepared & 1) && (call->prepared & 2) == (mask & 2))) ZTRY(dec_tp_pack(c, (mask & 2) ? 1 : 0));
    ZTRY(dec_tb_run(c, io, h_in, h_out, tpk.status_arg(call ? call->status : nullptr)));
    t_batch_last_path = 1;
    bool ok = false;
    ZTRY(tpk.settle(s, tp_errword(w), &ok));
    if (ok) return 0;
    // a bounded wait gave up: disabled for this process, the stage launches redo the chunk
  }
  t_batch_last_path = 2;
  return decoder_fwd_impl(dp, P, st, io, 0, h_in, h_out, ws, ws_bytes, stream, nullptr);
}

// error word of the chained (run-ahead) stage launches of the last rollout that used `ws`: 0 = every hand-off wait was
// satisfied; non-zero = a bounded spin gave up (the results of that rollout are invalid).  Synchronises the device.
extern "C" int zeggs_decoder_chain_errors(const ZeggsDecDims* dp, int training, void* ws, size_t ws_bytes, int* out) {
  Arena a(ws, ws_bytes);
  DecWs w = carve_dec(*dp, training, a);
  ZCHECK(a.ok() && w.chain, "chain_errors: workspace too small or no fast path for these dims");
  unsigned v = 0;
  ZCHECK(hipMemcpy(&v, w.chain + 4 * 8 * 32, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess, "chain_errors: copy failed");
  *out = (int)v;
  return 0;
}
// measurement builds (-DZEGGS_CHTIME): the phase stamps of the last 16 chained launches, 16 launches x {first, last
// workgroup} x 16 stamps (100 MHz wall clock)
extern "C" int zeggs_decoder_chain_stamps(const ZeggsDecDims* dp, int training, void* ws, size_t ws_bytes,
                                          unsigned long long* out /* [16][2][16] host */) {
  Arena a(ws, ws_bytes);
  DecWs w = carve_dec(*dp, training, a);
  ZCHECK(a.ok() && w.chain, "chain_stamps: workspace too small or no fast path for these dims");
  ZCHECK(hipMemcpy(out, w.chain + 4 * 8 * 32 + 32, 16 * 2 * 16 * 8, hipMemcpyDeviceToHost) == hipSuccess, "copy failed");
  return 0;
}

// Second half of the deferred weight gradients (option "defer_wgrads" = 2): the GEMMs of GRU layer 0 and layer0 (what = 4) on the
// caller's stream -- normally zeggs_side_stream again, behind the first half and the all-reduce the caller has started on it.
extern "C" int zeggs_decoder_wgrads(const ZeggsDecDims* dp, const ZeggsDecGrads* G, void* ws, size_t ws_bytes, int what,
                                    void* stream) {
  const ZeggsDecDims& d = *dp;
  Arena a(ws, ws_bytes);
  DecWs w = carve_dec(d, 1, a);
  ZCHECK(a.ok(), "decoder wgrads: workspace too small (was the forward run with training=1?)");
  ZCHECK(d.T > 1, "decoder wgrads: T must be > 1");
  const bool fast_path = g_decoder_fast && dec_fast_supported(d);
  // what & 8: the gradient outputs are zero on entry (ZeggsDecCall.grads_zeroed of the backward this call completes)
  return dec_recurrent_wgrads(d, w, G, 1, d.T - 1, (what & 8) ? 1.f : 0.f, fast_path ? 1 : 0, (hipStream_t)stream, what & 5);
}
// Everything the two persistent sweeps of a training step need that depends on the WEIGHTS only (the merged / folded
// matrices, the per-workgroup fragment packs of both kernels): the caller may run it on a second stream beside the encoders'
// forward and passes ZeggsDecCall.prepared to the zeggs_decoder_fwd_ex / _bwd_ex calls that follow on the same workspace.  Returns a bit mask
// (1: forward packs ready, 2: backward packs ready; 0: these dimensions take another path, nothing was done), < 0 on error.
extern "C" int zeggs_decoder_prepare(const ZeggsDecDims* dp, const ZeggsDecParams* P, const ZeggsDecStats* st, void* ws,
                                     size_t ws_bytes, void* stream) {
  const ZeggsDecDims& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  Arena a(ws, ws_bytes);
  DecWs w = carve_dec(d, 1, a);
  ZCHECK(a.ok(), "decoder prepare: workspace too small");
  const bool fast = g_decoder_fast && dec_fast_supported(d);
  // only once the kernels have been validated on this process (the first use takes the ordinary path)
  const SweepKernel &tpk = g_sweep_kernels[SWEEP_ROLLOUT], &bpk = g_sweep_kernels[SWEEP_BPTT];
  if (!(fast && d.T > 1 && tpk.enabled && tpk.state == 1 && dec_tp_supported(d, w))) return 0;
  const DecCtx c{d, P, st, w, s};
  ZTRY(dec_tp_pack(c));
  ZTRY(dec_tp_zero(d, w, s));
  int mask = 1;
  if (bpk.enabled && bpk.state == 1 && dec_bp_supported(d, w)) {
    ZTRY(dec_bp_pack(c));
    // ... and the zero state the backward starts from (carries, frame-0 slot of DX, arrival slots + error word)
    ZTRY(dec_bwd_zero_state(c, true));
    ZTRY(dec_bp_zero_slots(w, s));
    mask |= 2;
  }
  return mask;
}
// the library's low-priority second stream of the current device (also used by the chunked stage-launch sweep)
extern "C" int zeggs_side_stream(void** out) {
  SideStream* ss = nullptr;
  ZTRY(side_stream(&ss));
  *out = (void*)ss->s;
  return 0;
}

extern "C" int zeggs_decoder_bwd(const ZeggsDecDims* dp, const ZeggsDecParams* P, const ZeggsDecStats* st,
                                 const float* gaze, const float* pose, const float* rpos, const float* rrot,
                                 const float* dpose, const float* drpos, const float* drrot, const ZeggsDecGrads* G,
                                 float* dspeech, float* dstyle, void* ws, size_t ws_bytes, void* stream) {
  return zeggs_decoder_bwd_ex(dp, P, st, gaze, pose, rpos, rrot, dpose, drpos, drrot, G, dspeech, dstyle, ws, ws_bytes, stream,
                              nullptr);
}
extern "C" int zeggs_decoder_bwd_ex(const ZeggsDecDims* dp, const ZeggsDecParams* P, const ZeggsDecStats* st,
                                    const float* gaze, const float* pose, const float* rpos, const float* rrot,
                                    const float* dpose, const float* drpos, const float* drrot, const ZeggsDecGrads* G,
                                    float* dspeech, float* dstyle, void* ws, size_t ws_bytes, void* stream,
                                    const ZeggsDecCall* call) {
  const ZeggsDecDims& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  const bool bwd_prepared = call && (call->prepared & 2);
  const int defer_wgrads = call ? call->defer_wgrads : 0;
  unsigned* status = call ? call->status : nullptr;
  const float gb = (call && call->grads_zeroed) ? 1.f : 0.f;      // gradient outputs are zero on entry: accumulate, no fills
  ZCHECK(defer_wgrads == 0 || call->wgrad_stream != nullptr, "decoder bwd: defer_wgrads needs ZeggsDecCall.wgrad_stream");
  Arena a(ws, ws_bytes);
  DecWs w = carve_dec(d, 1, a);
  ZCHECK(a.ok(), "decoder bwd: workspace too small (was the forward run with training=1?)");
  const DecCtx c{d, P, st, w, s};
  const DecBwdIO io{gaze, pose, rpos, rrot, dpose, drpos, drrot};
  if (!bwd_prepared) ZTRY(dec_bwd_zero_state(c, true));      // (zeggs_decoder_prepare has done it)
  ZCHECK(d.T > 1, "decoder bwd: T must be > 1");
  const bool fast_path = g_decoder_fast && dec_fast_supported(d);
  // ---- the sweep t = T-1 .. 1 leaves DY, DI*, DH*, D0, DX and the final carries.  Batch <= 64: as one persistent launch
  // (train_bwd_persistent.hip); if it gave up on its first use, the stage kernels redo it from clean carries
  bool swept = false;
  SideStream* ss = nullptr;      // set where the sweep has started the weight gradients beside itself
  SweepKernel& bpk = g_sweep_kernels[SWEEP_BPTT];
  if (fast_path && dec_bp_supported(d, w) && bpk.may_run(s)) {
    ZTRY(dec_bp_run(c, io, bwd_prepared, bpk.status_arg(status)));
    ZTRY(bpk.settle(s, bp_errword(w), &swept));
    if (!swept) ZTRY(dec_bwd_zero_state(c, false));
  }
  if (!swept && fast_path) ZTRY(bwd_stage_sweep(c, io, G, gb, &ss));
  else if (!swept) ZTRY(bwd_generic_steps(c, io));
  // ---- weight gradients of the recurrent layers.  Option "defer_wgrads": the seven large GEMMs (K = B (T-1), they read only
  // what the sweep saved) start NOW on the library's second stream, beside the CellStateEncoder backward below and whatever the
  // caller enqueues on `s` after this call (the encoders' backward).  No join here: the caller makes every consumer of the
  // decoder gradients wait for zeggs_side_stream.
  const bool deferred = !ss && defer_wgrads && !stream_capturing(s);
  hipStream_t gs = deferred ? (hipStream_t)call->wgrad_stream : nullptr;
  // (value 2: only the first half of the parameter order here -- the caller all-reduces it while zeggs_decoder_wgrads
  //  computes the second half)
  // The bias sums (a dozen column sums over the same saves) go with them: since the split-K retune the GEMMs are the shorter
  // of the two queues.
  const int what = deferred ? (defer_wgrads == 2 ? 1 : 5) | 2 : 7;
  if (deferred) ZTRY(stream_fork(s, gs, 0));
  if (!ss) ZTRY(dec_recurrent_wgrads(d, w, G, 1, d.T - 1, gb, fast_path ? 1 : 0, deferred ? gs : s, what));
  ZTRY(dec_cse_bwd(c, G, gb, gs));
  ZTRY(dec_cond_grads(c, dspeech, dstyle));
  if (ss) ZCHECK(hipStreamWaitEvent(s, ss->done, 0) == hipSuccess, "hipStreamWaitEvent failed");   // join
  return 0;
}
