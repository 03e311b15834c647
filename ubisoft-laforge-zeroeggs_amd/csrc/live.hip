// Live serving: the speech encoder (ZEGGS/modules.py:249-272, eval mode) advanced incrementally for R independent rows in ONE launch.
//
// Conv k=1 -> ELU -> Conv k=KW (replicate padding) -> ELU -> Linear -> ELU.  Layer 0 is pointwise: the activation of a frame is
// computed once, when its feature row arrives, and kept in the row's ring ([D, H] floats, frame f in slot f % D); a step then costs
// KW H O MACs per produced frame and row instead of an encoder call over a KW-wide halo per stream (zeggs/stream.py).
//
// One workgroup of 512 threads per row.  The work is tiny (31 64 64 MACs per frame) and latency-bound, so the layout only makes sure
// that nothing is slow: the weights are read from L2 in a packed layout in which a lane's 16-byte load covers 4 input channels of
// its output channel and the 64 lanes of a wave read 1 KB contiguously (zeggs_speech_encoder_live_prepare, once per weight set);
// the KW - 1 + 8 activation rows a pass needs are staged in LDS and read as wave-uniform 16-byte broadcasts; per-row arguments
// travel by value in the kernel arguments (scalar loads, no device-side table to upload); no scratch memory.
#include "../../include/zeggs_hip_live.h"
#include "common.h"

namespace {

constexpr int LTHR = 512;

struct LiveRows { ZeggsLiveRow r[ZEGGS_LIVE_MAX_ROWS]; };

struct LivePacks {
  float* w0t;   // [F][H]
  float* w1p;   // [KW][H/4][O][4]: (tap, channel quad, output channel) -> 4 consecutive input channels
  float* w2t;   // [O/4][O][4]
};
LivePacks carve_live(const ZeggsLiveDims& d, Arena& a) {
  LivePacks p;
  p.w0t = a.f((size_t)d.F * d.H);
  p.w1p = a.f((size_t)d.KW * d.H * d.O);
  p.w2t = a.f((size_t)d.O * d.O);
  return p;
}

__global__ void live_pack_k(ZeggsLiveDims d, const float* w0, const float* w1, const float* w2, LivePacks p) {
  const int H = d.H, O = d.O, F = d.F, KW = d.KW;
  const long n0 = (long)F * H, n1 = (long)KW * H * O, n2 = (long)O * O;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n0 + n1 + n2; i += (long)gridDim.x * blockDim.x) {
    if (i < n0) {
      const int c = (int)(i / H), h = (int)(i % H);
      p.w0t[i] = w0[(long)h * F + c];
    } else if (i < n0 + n1) {
      const long q = i - n0;
      const int e = (int)(q & 3), o = (int)((q >> 2) % O), c4 = (int)((q >> 2) / O % (H / 4)), j = (int)((q >> 2) / O / (H / 4));
      p.w1p[q] = w1[((long)o * H + 4 * c4 + e) * KW + j];
    } else {
      const long q = i - n0 - n1;
      const int e = (int)(q & 3), o2 = (int)((q >> 2) % O), o4 = (int)((q >> 2) / O);
      p.w2t[q] = w2[(long)o2 * O + 4 * o4 + e];
    }
  }
}

__host__ __device__ inline size_t live_lds(const ZeggsLiveDims& d) {
  const int FRP = LTHR / d.O, FA = LTHR / d.H;
  return sizeof(float) * ((size_t)(FRP + d.KW - 1) * d.H + (((size_t)FA * d.F + 3) / 4 * 4) + (size_t)FRP * d.O);
}

__global__ __launch_bounds__(LTHR) void live_speech_k(ZeggsLiveDims d, LiveRows rows, const float* __restrict__ mean,
                                                      const float* __restrict__ stdv, const float* __restrict__ feats, float* ring,
                                                      float* __restrict__ out, LivePacks p, const float* __restrict__ b0,
                                                      const float* __restrict__ b1, const float* __restrict__ b2) {
  extern __shared__ __attribute__((aligned(16))) float lsm[];
  const int H = d.H, O = d.O, F = d.F, KW = d.KW, D = d.D, half = (KW - 1) / 2;
  const int FRP = LTHR / O, FA = LTHR / H, NA = FRP + KW - 1;
  float* act = lsm;                      // [NA][H] layer-0 activations of the frames a pass reads
  float* xs = act + (size_t)NA * H;      // [FA][F] normalised feature rows
  float* h1s = xs + ((size_t)FA * F + 3) / 4 * 4;      // [FRP][O] conv outputs (16-byte aligned)
  const int r = blockIdx.x, tid = threadIdx.x;
  const ZeggsLiveRow& rw = rows.r[r];
  const long n_ring = rw.n_ring, k0 = rw.k0;
  const int n_new = rw.n_new, n_out = rw.n_out;
  float* orow = out + (size_t)r * d.out_ld * O;
  for (int i = n_out * O + tid; i < d.out_ld * O; i += LTHR) orow[i] = 0.f;      // what the row does not produce: finite filler
  if (n_new == 0 && n_out == 0) return;
  float* rg = ring + (size_t)r * D * H;
  // ---- layer 0 of the new frames -> ring
  const float* fr = feats + ((size_t)r * d.feat_ld + rw.feat_off) * F;
  for (int i0 = 0; i0 < n_new; i0 += FA) {
    for (int i = tid; i < FA * F; i += LTHR) {
      const int fi = i / F, c = i - fi * F;
      xs[i] = (i0 + fi < n_new) ? (fr[(size_t)(i0 + fi) * F + c] - mean[c]) / stdv[c] : 0.f;
    }
    __syncthreads();
    {
      const int fi = tid / H, h = tid - fi * H;
      if (i0 + fi < n_new) {
        const float* x = xs + (size_t)fi * F;
        float acc = 0.f;
        for (int c = 0; c < F; ++c) acc = fmaf(x[c], p.w0t[(size_t)c * H + h], acc);
        rg[(size_t)((n_ring + i0 + fi) % D) * H + h] = d_elu(acc + b0[h]);
      }
    }
    __syncthreads();      // (also: the ring rows written above are read below by other threads of this workgroup)
  }
  if (n_out == 0) return;
  // ---- conv k=KW + ELU, Linear + ELU: FRP frames per pass
  const long top = rw.last >= 0 ? rw.last : n_ring + n_new - 1;      // replicate padding at the signal's end / newest frame in the ring
  const int fi = tid / O, o = tid - fi * O;
  const int H4 = H / 4, O4 = O / 4;
  for (int f0 = 0; f0 < n_out; f0 += FRP) {
    for (int i = tid; i < NA * H4; i += LTHR) {
      const int j = i / H4, c4 = i - j * H4;
      long q = k0 + f0 + j - half;
      q = q < 0 ? 0 : (q > top ? top : q);
      ((f4*)act)[i] = *(const f4*)(rg + (size_t)(q % D) * H + 4 * c4);
    }
    __syncthreads();
    {
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      const f4* wp = (const f4*)p.w1p + o;
      const f4* ap = (const f4*)act + (size_t)fi * H4;
      for (int j = 0; j < KW; ++j) {
#pragma unroll 8
        for (int c4 = 0; c4 < H4; ++c4) {
          const f4 a = ap[(size_t)j * H4 + c4];
          const f4 w = wp[((size_t)j * H4 + c4) * O];
          acc += a * w;
        }
      }
      h1s[tid] = d_elu((acc.x + acc.y) + (acc.z + acc.w) + b1[o]);
    }
    __syncthreads();
    {
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      const f4* wp = (const f4*)p.w2t + o;
      const f4* hp = (const f4*)(h1s + (size_t)fi * O);
#pragma unroll 8
      for (int o4 = 0; o4 < O4; ++o4) acc += hp[o4] * wp[(size_t)o4 * O];
      if (f0 + fi < n_out) orow[(size_t)(f0 + fi) * O + o] = d_elu((acc.x + acc.y) + (acc.z + acc.w) + b2[o]);
    }
    __syncthreads();
  }
}

int live_dims_ok(const ZeggsLiveDims& d) {
  ZCHECK(d.R >= 1 && d.R <= ZEGGS_LIVE_MAX_ROWS, "live speech encoder: %d rows (1..%d)", d.R, ZEGGS_LIVE_MAX_ROWS);
  ZCHECK(d.KW % 2 == 1 && d.KW >= 1, "live speech encoder: even kernel width %d", d.KW);
  ZCHECK(d.F >= 1 && d.H >= 4 && d.O >= 4 && d.H % 4 == 0 && d.O % 4 == 0 && LTHR % d.H == 0 && LTHR % d.O == 0,
         "live speech encoder: H = %d / O = %d must be multiples of 4 that divide %d", d.H, d.O, LTHR);
  ZCHECK(d.D >= d.KW && d.feat_ld >= 1 && d.out_ld >= 1, "live speech encoder: ring of %d frames under a kernel of %d", d.D, d.KW);
  ZCHECK(live_lds(d) <= 64 * 1024, "live speech encoder: %zu bytes of LDS", live_lds(d));
  return 0;
}

}  // namespace

extern "C" size_t zeggs_speech_encoder_live_workspace_bytes(const ZeggsLiveDims* d) {
  Arena a(nullptr, 0);
  carve_live(*d, a);
  return a.off + 256;
}

extern "C" int zeggs_speech_encoder_live_prepare(const ZeggsLiveDims* dp, const ZeggsSpeechParams* P, void* ws, size_t ws_bytes,
                                                 void* stream) {
  const ZeggsLiveDims& d = *dp;
  ZTRY(live_dims_ok(d));
  Arena a(ws, ws_bytes);
  LivePacks p = carve_live(d, a);
  ZCHECK(ws != nullptr && a.ok(), "live speech encoder: workspace too small (%zu < %zu)", ws_bytes, a.off);
  const long n = (long)d.F * d.H + (long)d.KW * d.H * d.O + (long)d.O * d.O;
  hipLaunchKernelGGL(live_pack_k, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, d, P->w0, P->w1, P->w2, p);
  ZLAUNCH_CHECK("live_pack");
  return 0;
}

extern "C" int zeggs_speech_encoder_live(const ZeggsLiveDims* dp, const ZeggsSpeechParams* P, const float* mean, const float* stdv,
                                         const ZeggsLiveRow* rows, const float* feats, float* ring, float* out, const void* ws,
                                         size_t ws_bytes, void* stream) {
  const ZeggsLiveDims& d = *dp;
  ZTRY(live_dims_ok(d));
  Arena a((void*)ws, ws_bytes);
  LivePacks p = carve_live(d, a);
  ZCHECK(ws != nullptr && a.ok(), "live speech encoder: workspace too small (%zu < %zu)", ws_bytes, a.off);
  const int half = (d.KW - 1) / 2;
  LiveRows lr;
  for (int r = 0; r < d.R; ++r) {
    const ZeggsLiveRow& w = rows[r];
    ZCHECK(w.n_new >= 0 && w.n_out >= 0 && w.n_ring >= 0 && w.feat_off >= 0, "live speech encoder: row %d: negative count", r);
    ZCHECK(w.n_new <= d.D && w.feat_off + w.n_new <= d.feat_ld, "live speech encoder: row %d: %d new frames at %d (ring %d, feats %d)", r,
           w.n_new, w.feat_off, d.D, d.feat_ld);
    ZCHECK(w.n_out <= d.out_ld, "live speech encoder: row %d: %d frames into %d output rows", r, w.n_out, d.out_ld);
    const long total = w.n_ring + w.n_new;       // frames [total - D, total) are in the ring after the new ones went in
    if (w.last >= 0) ZCHECK(total == w.last + 1, "live speech encoder: row %d ended at frame %ld but %ld frames arrived", r, w.last, total);
    if (w.n_out > 0) {
      ZCHECK(w.k0 >= 0 && total >= 1, "live speech encoder: row %d: nothing to read", r);
      long lo = w.k0 - half, hi = w.k0 + w.n_out - 1 + half;
      if (lo < 0) lo = 0;
      if (w.last >= 0) {
        ZCHECK(w.k0 + w.n_out - 1 <= w.last, "live speech encoder: row %d: frame %ld is past the last one (%ld)", r, w.k0 + w.n_out - 1, w.last);
        if (hi > w.last) hi = w.last;
        if (lo > w.last) lo = w.last;
      }
      ZCHECK(hi < total, "live speech encoder: row %d: frame %ld needs frame %ld, %ld are in the ring", r, w.k0 + w.n_out - 1, hi, total);
      ZCHECK(lo >= total - d.D, "live speech encoder: row %d: frame %ld has left the ring of %d (newest %ld)", r, lo, d.D, total - 1);
    }
    lr.r[r] = w;
  }
  for (int r = d.R; r < ZEGGS_LIVE_MAX_ROWS; ++r) lr.r[r] = ZeggsLiveRow{0, 0, -1, 0, 0, 0, 0};
  hipLaunchKernelGGL(live_speech_k, dim3((unsigned)d.R), dim3(LTHR), live_lds(d), (hipStream_t)stream, d, lr, mean, stdv, feats, ring, out,
                     p, P->b0, P->b1, P->b2);
  ZLAUNCH_CHECK("live_speech");
  return 0;
}

// ---------------------------------------------------------------- many small copies in one launch (include/zeggs_hip_live.h)
// What a tick's audio side moves between device buffers -- window compactions, the new samples behind them, pending feature rows --
// as ONE launch: blockIdx.y = segment, the workgroups of a segment stride over it.  Windows are appended at arbitrary sample
// offsets, so a segment's ends are only float-aligned: where source and destination share their offset within 16 bytes the body
// moves in 16-byte lanes between a scalar head and tail, otherwise float by float (coalesced either way).
namespace {
constexpr int SEG_THR = 256, SEG_MAX_X = 32;
__global__ __launch_bounds__(SEG_THR) void copy_segments_k(const ZeggsSeg* __restrict__ segs) {
  const ZeggsSeg sg = segs[blockIdx.y];
  const float* src = sg.src;
  float* dst = sg.dst;
  const long cnt = sg.count;
  if (cnt <= 0) return;
  const uintptr_t sa = (uintptr_t)src, da = (uintptr_t)dst;
  long head = cnt, nv = 0;
  if (((sa ^ da) & 15) == 0) {
    head = (long)(((16 - (da & 15)) & 15) >> 2);
    if (head > cnt) head = cnt;
    nv = (cnt - head) >> 2;
  }
  const long tail0 = head + 4 * nv, tid = (long)blockIdx.x * SEG_THR + threadIdx.x, stride = (long)gridDim.x * SEG_THR;
  const f4* sv = (const f4*)(src + head);
  f4* dv = (f4*)(dst + head);
  for (long i = tid; i < nv; i += stride) dv[i] = sv[i];
  for (long i = tid; i < head; i += stride) dst[i] = src[i];
  for (long i = tail0 + tid; i < cnt; i += stride) dst[i] = src[i];
}
}  // namespace

extern "C" int zeggs_copy_segments(const ZeggsSeg* segs, const ZeggsSeg* segs_dev, int n, void* stream) {
  ZCHECK(n >= 0 && n <= ZEGGS_MAX_SEGMENTS, "copy segments: %d segments (0..%d)", n, ZEGGS_MAX_SEGMENTS);
  if (n == 0) return 0;
  ZCHECK(segs != nullptr, "copy segments: NULL records");
  // destinations in address order: neighbours must not overlap, and no source may reach into any of them
  struct Span { uintptr_t lo, hi; int i; };
  Span dsts[ZEGGS_MAX_SEGMENTS];
  int nd = 0;
  long most = 0;
  for (int i = 0; i < n; ++i) {
    const ZeggsSeg& g = segs[i];
    ZCHECK(g.count >= 0, "copy segments: segment %d: negative count %ld", i, g.count);
    if (g.count == 0) continue;
    ZCHECK(g.src != nullptr && g.dst != nullptr && (uintptr_t)g.src % 4 == 0 && (uintptr_t)g.dst % 4 == 0,
           "copy segments: segment %d: NULL or misaligned pointer", i);
    dsts[nd++] = Span{(uintptr_t)g.dst, (uintptr_t)(g.dst + g.count), i};
    if (g.count > most) most = g.count;
  }
  if (nd == 0) return 0;
  for (int i = 1; i < nd; ++i) {      // insertion sort: the callers' lists are short and nearly ordered
    const Span x = dsts[i];
    int j = i - 1;
    for (; j >= 0 && dsts[j].lo > x.lo; --j) dsts[j + 1] = dsts[j];
    dsts[j + 1] = x;
  }
  for (int i = 1; i < nd; ++i)
    ZCHECK(dsts[i - 1].hi <= dsts[i].lo, "copy segments: the destinations of segments %d and %d overlap", dsts[i - 1].i, dsts[i].i);
  for (int i = 0; i < n; ++i) {
    const ZeggsSeg& g = segs[i];
    if (g.count == 0) continue;
    const uintptr_t lo = (uintptr_t)g.src, hi = (uintptr_t)(g.src + g.count);
    int a = 0, b = nd;                  // first destination that ends above lo
    while (a < b) { const int m = (a + b) / 2; if (dsts[m].hi > lo) b = m; else a = m + 1; }
    ZCHECK(a == nd || dsts[a].lo >= hi, "copy segments: the source of segment %d overlaps the destination of segment %d", i,
           a < nd ? dsts[a].i : -1);
  }
  ZCHECK(segs_dev != nullptr, "copy segments: the records must also be in device memory (segs_dev)");
  const long gx = (most + 4 * SEG_THR - 1) / (4 * SEG_THR);
  hipLaunchKernelGGL(copy_segments_k, dim3((unsigned)(gx > SEG_MAX_X ? SEG_MAX_X : gx), (unsigned)n), dim3(SEG_THR), 0, (hipStream_t)stream,
                     segs_dev);
  ZLAUNCH_CHECK("copy_segments");
  return 0;
}
