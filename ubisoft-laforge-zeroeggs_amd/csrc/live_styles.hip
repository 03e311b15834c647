// Live serving: a bank of named styles on the device, mixed per row (include/zeggs_hip_styles.h; the arithmetic is style_math.h,
// the definition DESIGN.md 3.7).
//
// The bank is [capacity][2][ST] float32: a slot's mean row and its deviation row.  Two small kernels, each ONE launch:
//   live_style_put_k   lanes over the columns: a slot from an encoder row (mean | log-variance) or from a plain vector;
//   live_style_mix_k   one workgroup per record, lanes over the columns: the row's new style is the weighted sum of up to
//                      STYLE_MAX_TERMS slots (float64 from the float32 operands, rounded once at the store), its old style is
//                      where the row's unfinished fade stands at frame k - 1 -- live_condition_k's statement.
// Plain loads and stores, no LDS, nothing indexed in registers: the loop over the terms is unrolled with the count as a guard,
// and the record's fields are wave-uniform.  A column is read and written by one lane only, so a call needs no ordering.
#include "../../include/zeggs_hip_styles.h"
#include "common.h"
#include "style_math.h"

#include <math.h>

namespace {

constexpr int STYLE_THREADS = 256;

static_assert(STYLE_MAX_TERMS == ZEGGS_STYLE_MAX_TERMS, "style_math.h and the tenth header disagree");
static_assert(sizeof(ZeggsStyleMix) == 112 && sizeof(((ZeggsStyleMix*)nullptr)->weight) == 4 * STYLE_MAX_TERMS &&
                  sizeof(((ZeggsStyleMix*)nullptr)->slot) == 4 * STYLE_MAX_TERMS,
              "ZeggsStyleMix");

__global__ __launch_bounds__(STYLE_THREADS) void live_style_put_k(float* __restrict__ slot, const float* __restrict__ enc, int ST, int E) {
  for (int c = blockIdx.x * STYLE_THREADS + threadIdx.x; c < ST; c += gridDim.x * STYLE_THREADS) {
    slot[c] = style_slot_mean(enc, c);
    slot[ST + c] = style_slot_dev(enc, ST, E, c);
  }
}

__global__ __launch_bounds__(STYLE_THREADS) void live_style_mix_k(const ZeggsStyleMix* __restrict__ recs, ZeggsStyleMix one,
                                                                   const float* __restrict__ bank, const float* __restrict__ eps,
                                                                   float* sty_old, float* sty_new, int ST) {
  const ZeggsStyleMix rec = recs ? recs[blockIdx.x] : one;
  const float* e = eps != nullptr && rec.eps_row >= 0 ? eps + (long)rec.eps_row * STYLE_MAX_TERMS * ST : nullptr;
  float* po = sty_old + (long)rec.row * ST;
  float* pn = sty_new + (long)rec.row * ST;
  for (int c = threadIdx.x; c < ST; c += STYLE_THREADS) {
    float o = po[c], n = pn[c];
    style_mix_column(rec.slot, rec.weight, rec.terms, bank, ST, c, e, rec.temperature, rec.k, rec.k_style, rec.fade_style, rec.reset, &o, &n);
    po[c] = o;
    pn[c] = n;
  }
}

}  // namespace

#include "live_host.h"      // the host contract every stage of live serving keeps

namespace {

int style_dims_ok(const ZeggsStyleBankDims* d, const void* bank, size_t bank_bytes) {
  ZTRY(lh_dims_ok("live styles", d));
  ZCHECK(d->ST >= 1 && d->ST <= (1 << 16), "live styles: style rows of %d floats", d->ST);
  ZCHECK(d->capacity >= 1 && d->capacity <= ZEGGS_STYLE_MAX_SLOTS, "live styles: a bank of %d slots (1..%d)", d->capacity, ZEGGS_STYLE_MAX_SLOTS);
  return lh_block_ok("live styles", "bank", bank, bank_bytes, (size_t)d->capacity * 2 * d->ST * sizeof(float), 4);
}

}  // namespace

extern "C" int zeggs_live_styles_version(void) { return 1; }

extern "C" size_t zeggs_live_style_bank_bytes(const ZeggsStyleBankDims* d) {
  if (style_dims_ok(d, nullptr, (size_t)-1) != 0) return 0;
  return (size_t)d->capacity * 2 * d->ST * sizeof(float);
}

extern "C" int zeggs_live_style_put(const ZeggsStyleBankDims* d, void* bank, size_t bank_bytes, int slot, const float* enc, int E, void* stream) {
  ZTRY(style_dims_ok(d, bank, bank_bytes));
  ZCHECK(slot >= 0 && slot < d->capacity, "live style put: slot %d of %d", slot, d->capacity);
  ZCHECK(E == d->ST || E == 2 * d->ST, "live style put: a row of %d floats (%d: a plain vector, %d: mean and log-variance)", E, d->ST, 2 * d->ST);
  ZCHECK(enc != nullptr && (uintptr_t)enc % 4 == 0, "live style put: NULL or misaligned row");
  const int blocks = (d->ST + STYLE_THREADS - 1) / STYLE_THREADS;
  hipLaunchKernelGGL(live_style_put_k, dim3((unsigned)(blocks < 64 ? blocks : 64)), dim3(STYLE_THREADS), 0, (hipStream_t)stream,
                     (float*)bank + (size_t)slot * 2 * d->ST, enc, d->ST, E);
  ZLAUNCH_CHECK("live_style_put");
  return 0;
}

extern "C" int zeggs_live_style_mix(const ZeggsStyleBankDims* d, const ZeggsStyleMix* recs, const ZeggsStyleMix* recs_dev, int R, const void* bank,
                                    size_t bank_bytes, const float* eps, int eps_rows, float* sty_old, float* sty_new, void* stream) {
  const char* who = "live style mix";
  ZTRY(style_dims_ok(d, bank, bank_bytes));
  ZTRY(lh_count_ok(who, R, d->rows));
  ZCHECK(eps_rows >= 0 && eps_rows <= (1 << 20), "live style mix: a noise tensor of %d slices", eps_rows);
  if (R == 0) return 0;
  ZCHECK(recs != nullptr, "live style mix: NULL records");
  bool seen[ZEGGS_LIVE_MAX_ROWS] = {};
  for (int i = 0; i < R; ++i) {
    const ZeggsStyleMix& w = recs[i];
    ZTRY(lh_once_ok(who, i, w.row, d->rows, seen));
    ZCHECK(w.terms >= 1 && w.terms <= ZEGGS_STYLE_MAX_TERMS, "live style mix: record %d: %d terms (1..%d)", i, w.terms, ZEGGS_STYLE_MAX_TERMS);
    for (int t = 0; t < w.terms; ++t) {
      ZCHECK(w.slot[t] >= 0 && w.slot[t] < d->capacity, "live style mix: record %d: term %d: slot %d of %d", i, t, w.slot[t], d->capacity);
      ZCHECK(isfinite(w.weight[t]), "live style mix: record %d: term %d: the weight is not finite", i, t);
    }
    ZCHECK(w.k >= 0, "live style mix: record %d: negative frame %ld", i, w.k);
    ZCHECK(w.k_style >= 0, "live style mix: record %d: negative style frame %ld", i, w.k_style);
    ZCHECK(w.fade_style >= 0, "live style mix: record %d: negative style fade %ld", i, w.fade_style);
    ZCHECK(isfinite(w.temperature) && w.temperature >= 0.f, "live style mix: record %d: temperature %g (finite, >= 0)", i, (double)w.temperature);
    ZCHECK(w.eps_row >= -1 && w.eps_row < (eps_rows > 0 ? eps_rows : 0), "live style mix: record %d: noise slice %d of %d", i, w.eps_row, eps_rows);
    ZCHECK(!(w.temperature > 0.f && w.eps_row >= 0) || eps != nullptr, "live style mix: record %d: noise asked for with a NULL noise tensor", i);
  }
  ZCHECK(sty_old != nullptr && sty_new != nullptr && sty_old != sty_new, "live style mix: NULL style tensor (or one tensor twice)");
  ZCHECK(((uintptr_t)sty_old | (uintptr_t)sty_new | (uintptr_t)eps) % 4 == 0, "live style mix: misaligned tensor");
  ZTRY(lh_dev_ok(who, "recs_dev", recs_dev, R));
  hipLaunchKernelGGL(live_style_mix_k, dim3((unsigned)R), dim3(STYLE_THREADS), 0, (hipStream_t)stream, recs_dev, recs[0], (const float*)bank, eps,
                     sty_old, sty_new, d->ST);
  ZLAUNCH_CHECK("live_style_mix");
  return 0;
}

extern "C" int zeggs_live_style_read(const ZeggsStyleBankDims* d, const void* bank, size_t bank_bytes, int slot, const float* sty_old,
                                     const float* sty_new, int row, float* out, void* stream) {
  ZCHECK(out != nullptr, "live style read: NULL output");
  hipError_t e;
  if (row < 0) {
    ZTRY(style_dims_ok(d, bank, bank_bytes));
    ZCHECK(row == -1 && slot >= 0 && slot < d->capacity, "live style read: slot %d of %d (row %d: -1 reads a slot)", slot, d->capacity, row);
    e = hipMemcpyAsync(out, (const float*)bank + (size_t)slot * 2 * d->ST, (size_t)2 * d->ST * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream);
  } else {
    ZTRY(style_dims_ok(d, nullptr, (size_t)-1));
    ZCHECK(slot == -1 && row < d->rows, "live style read: row %d of %d (slot %d: -1 reads a row)", row, d->rows, slot);
    ZCHECK(sty_old != nullptr && sty_new != nullptr, "live style read: NULL style tensor");
    e = hipMemcpyAsync(out, sty_old + (size_t)row * d->ST, (size_t)d->ST * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(out + d->ST, sty_new + (size_t)row * d->ST, (size_t)d->ST * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  ZCHECK(e == hipSuccess, "live style read: %s", hipGetErrorString(e));
  return 0;
}
