/* C ABI of libzeggs_hip.so, third header: running loudness normalisation of live serving (zeggs_version() >= 109).
 *
 * include/zeggs_hip.h and include/zeggs_hip_live.h are closed sets (tests/test_abi.py, tests/test_live_push_cpu.py pin their
 * prototypes and structs); the entry points below have a header of their own.  Same conventions as the other two: the caller
 * owns all memory, calls only enqueue on `stream` (zeggs_live_loudness_read also waits for it), 0 on success / -1 with
 * zeggs_last_error().  The Python mirror is zeggs/capi.py: LOUD_STRUCTS / LOUD_PROTOTYPES (tests/test_live_loudness_cpu.py
 * compares the two).
 *
 * Every row (stream) of a live server keeps a running ITU-R BS.1770 gated loudness estimate of the float32 samples it has
 * received since its last reset, and new samples enter the row's device window multiplied by the gain that brings the
 * estimate to `target` (csrc/live_loudness.hip; the definition is DESIGN.md 3.7, the index and gate rules csrc/loud_math.h):
 *   - y = HP(HS(x)): the two K-weighting biquads, direct form II transposed in float64, strictly sequential per row with
 *     the states carried from call to call, each stage's output rounded to float32 (the offline path's f32_stages = 1);
 *   - block j covers samples [trunc(0.4 (j 0.25) fs), trunc(0.4 (j 0.25 + 1) fs)); its energy is taken when its last sample
 *     has arrived, from a ring of the last block-length filtered samples, in the summation order of the offline kernel;
 *   - after block j the two gates run over the last `ring_blocks` block energies; when at least `warmup` blocks pass the
 *     relative gate the estimate L_j is new and the gain becomes (float) 10^(clip(target - L_j, gain_lo, gain_hi) / 20),
 *     valid from sample index hi_j on -- wherever that index falls inside a call; otherwise the gain stays.
 * Nothing depends on how a row's samples are cut into calls, nor on which other rows take part in a call: bitwise. */
#ifndef ZEGGS_HIP_LOUDNESS_H
#define ZEGGS_HIP_LOUDNESS_H
#include "zeggs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int fs, rows;             /* sampling rate; rows of the state (<= ZEGGS_LIVE_MAX_ROWS) */
  int ring_blocks, warmup;  /* blocks the estimate looks back over (10 per second); gated blocks an estimate needs (>= 1) */
  double target;            /* LUFS */
  double gain_lo, gain_hi;  /* bounds of the gain in dB, gain_lo <= gain_hi */
  double coef[10];          /* high shelf (b0 b1 b2 a1 a2), high pass: the K-weighting biquads for fs, a0 = 1 */
} ZeggsLoudDims;

/* one row's share of a push: count new samples at src (device, unscaled) go to dst (device: their place in the row's window)
 * as src[i] * gain, a float32 product, with the gain valid at each sample's index */
typedef struct { const float* src; float* dst; long count; int row; } ZeggsLoudRow;

/* what zeggs_live_loudness_read writes, as doubles */
#define ZEGGS_LOUD_READ_LUFS 0      /* the last estimate; NaN before the first one */
#define ZEGGS_LOUD_READ_GAIN 1      /* the gain new samples are multiplied by now */
#define ZEGGS_LOUD_READ_BLOCKS 2    /* gating blocks completed */
#define ZEGGS_LOUD_READ_GATED 3     /* blocks that passed the relative gate when the last block completed */
#define ZEGGS_LOUD_READ_HELD 4      /* 1: the last completed block left the gain as it was (no estimate, or the hold flag) */
#define ZEGGS_LOUD_READ_SAMPLES 5   /* samples received since the reset: the state is the only owner of this count */
#define ZEGGS_LOUD_READ_HOLD 6      /* the hold flag */
#define ZEGGS_LOUD_READ_WORDS 8

/* bytes of the state of d->rows rows: per row four filter states, the counters, the gain, the last estimate, the hold flag, a
 * ring of one block of filtered samples (0.4 fs doubles) and a ring of ring_blocks block energies with their levels */
size_t zeggs_live_loudness_state_bytes(const ZeggsLoudDims*);
/* row `row` starts from nothing: zero filter states and counters, empty rings, no estimate, hold off, gain = gain0 */
int zeggs_live_loudness_reset(const ZeggsLoudDims*, void* state, size_t state_bytes, int row, float gain0, void* stream);
/* on != 0: the row goes on filtering and metering but its gain stays what it is; 0: the next estimate moves it again */
int zeggs_live_loudness_hold(const ZeggsLoudDims*, void* state, size_t state_bytes, int row, int on, void* stream);
/* ONE launch for all R records (grid = R).  rows_host: the records in HOST memory for the checks, all ahead of the launch and
 * naming the record they refuse: row in 0 .. d->rows - 1 and not twice in a call, count >= 0, non-NULL 4-byte-aligned
 * pointers where count > 0.  rows_dev: the same records in DEVICE memory; NULL is allowed for R == 1 (the record then travels
 * in the kernel arguments).  dst must have room for count floats; src and dst must not overlap. */
int zeggs_live_loudness_push(const ZeggsLoudDims*, const ZeggsLoudRow* rows_host, const ZeggsLoudRow* rows_dev, int R, void* state,
                             size_t state_bytes, void* stream);
/* out_host[ZEGGS_LOUD_READ_WORDS] <- the row's figures after everything enqueued on `stream` so far (waits for the stream):
 * monitoring, not for the tick path */
int zeggs_live_loudness_read(const ZeggsLoudDims*, const void* state, size_t state_bytes, int row, double* out_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif
