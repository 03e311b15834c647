/* C ABI of libzeggs_hip.so, tenth header: a bank of named styles on the device, mixed per live row
 * (zeggs_live_styles_version() >= 1; zeggs_version() >= 109 and the versions of the other headers stay what they are).
 *
 * The other nine headers are closed sets (their tests pin their prototypes and structs); the entry points below have a header
 * of their own.  Same conventions as include/zeggs_hip_gaze.h: the caller owns all memory, calls only enqueue on `stream`
 * (zeggs_live_style_read also waits for it), 0 on success / -1 with zeggs_last_error().  The Python mirror is zeggs/capi.py:
 * SB_STRUCTS / SB_PROTOTYPES (tests/test_live_styles_cpu.py compares the two).
 *
 * The BANK holds `capacity` slots of two float32 rows of ST floats each, [capacity][2][ST]: a slot's MEAN row and its DEVIATION
 * row.  zeggs_live_style_put writes a slot from a row in device memory: the style encoder's VAE output (E == 2 ST: mean[c] =
 * enc[c], dev[c] = expf(0.5f * enc[ST + c]), the float32 expression of the offline re-parameterisation) or a plain vector
 * (E == ST: dev = 0).  zeggs_live_style_mix writes the two style rows of a live row from the bank (csrc/style_math.h, the one
 * statement for host and device):
 *   new'[c] = (float) sum_i w_i (mean_i[c] + (dev_i[c] / temperature) eps_i[c])      i = 0 .. terms - 1, in record order,
 * accumulated in float64 from the float32 operands and rounded once at the store; without noise (temperature 0, eps_row -1) a
 * term is w_i mean_i[c].  The weights are not normalised and a slot may appear twice.
 *   old'[c] = lerp(old[c], new[c], w_style(k - 1; k_style, fade_style))
 * -- the statement zeggs_live_condition evaluates for frame k - 1, so an unfinished fade goes on from exactly the row the
 * decoder was last fed; with `reset`, old' = new'. */
#ifndef ZEGGS_HIP_STYLES_H
#define ZEGGS_HIP_STYLES_H
#include "zeggs_hip_gaze.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZEGGS_STYLE_MAX_TERMS 8
#define ZEGGS_STYLE_MAX_SLOTS 4096

typedef struct {
  int rows, ST, capacity;   /* rows of the style tensors (<= ZEGGS_LIVE_MAX_ROWS); floats of a style row (>= 1); slots (1 .. ZEGGS_STYLE_MAX_SLOTS) */
} ZeggsStyleBankDims;

/* one row's new style: terms i = 0 .. terms - 1 of (slot[i], weight[i]), from frame k on; k_style / fade_style are the row's OLD
 * fade (where it stands at frame k - 1 becomes the new old row); temperature 0: the means alone; eps_row: the slice
 * [ZEGGS_STYLE_MAX_TERMS][ST] of the noise tensor that holds this record's noise, term i in its row i (-1: none) */
typedef struct {
  long k, k_style, fade_style;
  float weight[8];
  int slot[8];
  float temperature;
  int row, terms, eps_row, reset;
} ZeggsStyleMix;

int zeggs_live_styles_version(void);
/* bytes of a bank of d->capacity slots: 2 ST floats each, one slot behind another (mean row, then deviation row) */
size_t zeggs_live_style_bank_bytes(const ZeggsStyleBankDims*);
/* ONE launch: slot `slot` <- enc[E] (float32, DEVICE memory), E == 2 ST (mean | log-variance) or E == ST (a plain vector) */
int zeggs_live_style_put(const ZeggsStyleBankDims*, void* bank, size_t bank_bytes, int slot, const float* enc, int E, void* stream);
/* ONE launch for all R records (grid = R, lanes over the ST columns).  recs_host: the records in HOST memory for the checks, all
 * ahead of the launch and naming the record they refuse: row in 0 .. d->rows - 1 and not twice in a call, terms in 1 ..
 * ZEGGS_STYLE_MAX_TERMS, every slot in 0 .. d->capacity - 1, finite weights, k >= 0, k_style >= 0, fade_style >= 0, a finite
 * temperature >= 0, eps_row in -1 .. eps_rows - 1, and noise asked for (temperature > 0 and eps_row >= 0) with eps == NULL.
 * recs_dev: the same records in DEVICE memory; NULL is allowed for R == 1 (the record then travels in the kernel arguments).
 * eps: [eps_rows][ZEGGS_STYLE_MAX_TERMS][ST] float32 in DEVICE memory or NULL.  sty_old / sty_new: [rows][ST], read and
 * written; rows no record names are not touched. */
int zeggs_live_style_mix(const ZeggsStyleBankDims*, const ZeggsStyleMix* recs_host, const ZeggsStyleMix* recs_dev, int R, const void* bank,
                         size_t bank_bytes, const float* eps, int eps_rows, float* sty_old, float* sty_new, void* stream);
/* out_host[2 ST] floats <- slot `slot`'s mean and deviation rows (slot >= 0, row == -1), or row `row`'s old and new style rows
 * (row >= 0, slot == -1), after everything enqueued on `stream` so far (waits for the stream): monitoring, not for the tick path */
int zeggs_live_style_read(const ZeggsStyleBankDims*, const void* bank, size_t bank_bytes, int slot, const float* sty_old, const float* sty_new,
                          int row, float* out_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif
