/* C ABI of libzeggs_hip.so, second header: the batched audio side of live serving (zeggs_version() >= 107).
 *
 * include/zeggs_hip.h is a closed set (tests/test_abi.py pins its prototypes and structs, and allows no pointer fields in new
 * structs there); the entry points below take per-row RECORDS that hold device pointers, so they live here.  Same conventions
 * as the main header: the caller owns all memory, calls only enqueue on `stream`, 0 on success / -1 with zeggs_last_error().
 * The Python mirror is zeggs/capi.py: EXT_STRUCTS / EXT_PROTOTYPES (tests/test_live_push_cpu.py compares the two).
 */
#ifndef ZEGGS_HIP_LIVE_H
#define ZEGGS_HIP_LIVE_H
#include "zeggs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- batched mel front-end
 * zeggs_mel_features_window for up to ZEGGS_LIVE_MAX_ROWS independent rows in TWO launches whatever R is: one STFT launch whose
 * workgroups map to (row, block of 4 STFT frames of that row) through a prefix table of block counts -- a block never holds
 * frames of two rows --, one resample launch over all rows' output elements.  The per-frame arithmetic is the code of the
 * per-row FFT kernel: every row's output is bit-identical to what zeggs_mel_features_window writes for the same arguments.
 *
 *   tables     twiddles / window and the packed filterbank, built ONCE per (dims, filterbank) by zeggs_mel_batch_prepare into a
 *              caller-owned buffer of zeggs_mel_batch_tables_bytes(d) bytes (the per-row entry points rebuild them per call)
 *   rows_host  R records in HOST memory: every argument check reads these, all ahead of any launch, and names the row it refuses
 *              (per row the checks of zeggs_mel_features_window: k1 <= zeggs_mel_frames_ready unless final, no "cubic", the
 *              window does not start above the first sample the row's frames load)
 *   rows_dev   the same R records in DEVICE memory (what the kernels read); NULL: the library uploads rows_host into `ws` on
 *              `stream` itself
 *   ws         zeggs_mel_batch_workspace_bytes(d, R, F) bytes, F >= the largest k1 - k0 of the call
 * Where the FFT form does not apply (option "mel_fft" = 0, an n_fft / 2 that does not factor into 4 / 5 / 2, too much LDS) the
 * call runs the per-row path for each row inside the same call (the fall-back rule of zeggs_decoder_fwd_batch): same results,
 * two or three launches per row.  zeggs_mel_batch_last_ops(): what the calling thread's last zeggs_mel_features_batch enqueued
 * (launches, + 1 for the records' upload when rows_dev was NULL). */
typedef struct {            /* one stream's share of a batched front-end call */
  const float* wav;         /* device: the row's window, wav[i] = sample base + i */
  float* out;               /* device: [k1 - k0, n_mels + 1] */
  long base, n_samples;     /* as zeggs_mel_features_window */
  long k0, k1;              /* feature rows [k0, k1); k1 == k0: the row takes no part */
  int final;
} ZeggsMelRow;
size_t zeggs_mel_batch_tables_bytes(const ZeggsMelDims*);
int zeggs_mel_batch_prepare(const ZeggsMelDims*, const double* filterbank, void* tables, size_t bytes, void* stream);
size_t zeggs_mel_batch_workspace_bytes(const ZeggsMelDims*, int rows, long max_frames_per_row);
int zeggs_mel_features_batch(const ZeggsMelDims*, const ZeggsMelRow* rows_host, const ZeggsMelRow* rows_dev, int R,
                             const double* filterbank, const void* tables, void* ws, size_t ws_bytes, void* stream);
int zeggs_mel_batch_last_ops(void);

/* ---------------------------------------------------------------- many small copies in one launch
 * n <= ZEGGS_MAX_SEGMENTS segments of floats, dst[0 .. count) = src[0 .. count) each, device to device.  Any 4-byte-aligned
 * src / dst (16-byte lanes where both sides of a segment share their offset within 16 bytes); count == 0 is allowed.
 * segs_host: the records in HOST memory for the checks -- refused ahead of the launch: a negative count, a NULL or misaligned
 * pointer, a segment whose source overlaps its own or any other segment's destination, two destinations that overlap;
 * segs_dev: the same records in DEVICE memory (n x 24 bytes do not fit the kernel arguments). */
#define ZEGGS_MAX_SEGMENTS 256
typedef struct { const float* src; float* dst; long count; } ZeggsSeg;
int zeggs_copy_segments(const ZeggsSeg* segs_host, const ZeggsSeg* segs_dev, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
