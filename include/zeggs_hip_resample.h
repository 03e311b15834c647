/* C ABI of libzeggs_hip.so, fourth header: the band-limited rate converter of live serving
 * (zeggs_live_resample_version() >= 1; zeggs_version() stays what it is).
 *
 * include/zeggs_hip.h, include/zeggs_hip_live.h and include/zeggs_hip_loudness.h are closed sets (their tests pin their
 * prototypes and structs); the entry points below have a header of their own.  Same conventions as the other three: the caller
 * owns all memory, calls only enqueue on `stream`, 0 on success / -1 with zeggs_last_error().  The Python mirror is
 * zeggs/capi.py: RS_STRUCTS / RS_PROTOTYPES (tests/test_live_resample_cpu.py compares the two).
 *
 * Every row (stream) of a live server may deliver its audio at a rate fi of its own, as float32 or 16-bit PCM, and is converted
 * to the server's rate fo as it arrives (csrc/live_resample.hip; the definition is DESIGN.md 3.7, the index rules
 * csrc/resample_math.h):  g = gcd(fi, fo), L = fo / g, M = fi / g;  output m sits at input position p_m = m M / L and is
 *     y[m] = sum over the integers k with |p_m - k| < W of x[k] h(p_m - k),   x[k] = 0 for k < 0 (and past the end of the signal)
 * with a Kaiser-windowed sinc h of support W = Z / min(1, L / M) input samples.  The caller builds the coefficients in float64,
 * one table [L][taps] per (fi, fo, Z, rolloff, beta): row `phase` = (m M) mod L, tap j on input k = floor(p_m) - ceil(W) + j,
 * taps = 2 ceil(W) + 1 (zeggs.audio.resample_table).  The device accumulates an output in float64, ascending k, one
 * accumulator of explicit fma(), then rounds to float32: an output is the same bits wherever it falls in a call, however the
 * row's input is cut into calls and whichever rows share a call.  While the signal goes on output m is ready once
 * p_m + W <= n_in; at its end the total is ceil(n_in L / M) and the tail is computed against zeros.
 * 16-bit PCM is x = s / 32768 (exact).  WL = 0 is the pass-through mode: L = M = 1, a table of the one tap 1.0, y[m] = x[m]. */
#ifndef ZEGGS_HIP_RESAMPLE_H
#define ZEGGS_HIP_RESAMPLE_H
#include "zeggs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZEGGS_RS_F32 0            /* float32 samples */
#define ZEGGS_RS_S16 1            /* 16-bit signed PCM, x = s / 32768 */
#define ZEGGS_RS_MAX_HISTORY 3072 /* 2 W at 64 zero crossings and the largest supported decimation, 24 */

typedef struct {
  int rows;     /* rows of the state (<= ZEGGS_LIVE_MAX_ROWS) */
  int history;  /* float32 samples of past input a row can carry (>= ceil(2 W) of every table used on it) */
} ZeggsResampleDims;

/* one row's share of a push.  The counters are the caller's (the host plans with them as it plans frames): before the call
 * the row has received n_in input samples and produced n_out outputs, n_out == ready(n_in).  `count` new inputs at src (device,
 * `format`); `outputs` converted samples go to dst (device float32): outputs == ready(n_in + count) - n_out, or with `final`
 * != 0 (the signal ends with this call) ceil((n_in + count) L / M) - n_out.  After a final call the row must be reset. */
typedef struct {
  const void* src;
  float* dst;
  const double* table; /* device, [L][2 ceil(WL / L) + 1] */
  long count, n_in, n_out, outputs;
  long WL;             /* W L = Z max(L, M); 0: pass-through */
  int row, format, final, L, M;
} ZeggsResampleRow;

int zeggs_live_resample_version(void);
/* bytes of the state of d->rows rows: per row a ring of d->history float32 input samples (sample k in slot k % ceil(2 W)) */
size_t zeggs_resample_state_bytes(const ZeggsResampleDims*);
/* row `row` starts from nothing (an all-zero history); the counters of its next record are 0 */
int zeggs_resample_reset(const ZeggsResampleDims*, void* state, size_t state_bytes, int row, void* stream);
/* ONE launch for all R records (grid = R; a row's outputs are all computed before its history moves).  rows_host: the records
 * in HOST memory for the checks, all ahead of the launch and naming the record they refuse: row in 0 .. d->rows - 1 and not
 * twice in a call, count >= 0, a known format, a supported ratio whose history fits d->history, counters that agree with
 * ready(), non-NULL aligned pointers (src where count > 0, dst where outputs > 0, table always).  rows_dev: the same records in
 * DEVICE memory; NULL is allowed for R == 1 (the record then travels in the kernel arguments). */
int zeggs_resample_push(const ZeggsResampleDims*, const ZeggsResampleRow* rows_host, const ZeggsResampleRow* rows_dev, int R, void* state,
                        size_t state_bytes, void* stream);
/* the tail of ONE row at the end of its signal: zeggs_resample_push of the one record with `final` taken as set */
int zeggs_resample_flush(const ZeggsResampleDims*, const ZeggsResampleRow* row_host, void* state, size_t state_bytes, void* stream);
/* a whole signal in one piece, no state: n_in samples at src -> n_out == ceil(n_in L / M) outputs at dst, zeros before and
 * behind the signal.  The same device function as the streaming entry: bitwise its outputs. */
int zeggs_resample_whole(const double* table, int L, int M, long WL, const void* src, int format, long n_in, float* dst, long n_out,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
