/* C ABI of libzeggs_hip.so, twelfth header: the signed column gather behind left/right mirroring
 * (zeggs_mirror_version() >= 1; zeggs_version() >= 109 and the versions of the other headers stay what they are).
 *
 * The other eleven headers are closed sets (their tests pin their prototypes and structs); the entry points below have a header
 * of their own.  Same conventions: 0 on success / -1 with zeggs_last_error(), zeggs_mirror_rows only enqueues on `stream`, and
 * the library keeps no caller memory -- the one thing it owns is the plan it made.  The Python mirror is zeggs/capi.py:
 * MR_PROTOTYPES (tests/test_mirror_cpu.py compares the two).
 *
 *   out[r, c] = +-in[r, source(c)]       over a row-major table [rows, cols] of 4-byte or 8-byte elements
 *
 * The TABLE holds one int32 per OUTPUT column: the source column in the low 31 bits, the sign flip in bit 31.  The flip is an
 * exclusive-or on the element's top bit, not a multiplication: -0.0, infinities and NaN payloads keep every other bit, and a
 * table that is an involution applied twice gives back the input bit for bit.  A table must name every column exactly once.
 * Which columns pair up and which change sign for a given row layout is the caller's business (zeggs/anim.py: mirror_table). */
#ifndef ZEGGS_HIP_MIRROR_H
#define ZEGGS_HIP_MIRROR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZEGGS_MIRROR_MAX_COLS 3072

int zeggs_mirror_version(void);
/* host only: 0 when table[cols] (HOST memory) names every column 0 .. cols - 1 once and 1 <= cols <= ZEGGS_MIRROR_MAX_COLS,
 * else -1 and the first offending column in zeggs_last_error() */
int zeggs_mirror_table_check(const int32_t* table, int cols);
/* *plan <- a plan for table[cols] (HOST memory; checked as above before anything touches the device).  The plan keeps a copy
 * of the table on the current device; this call allocates, uploads and waits for the upload, zeggs_mirror_rows does none of
 * that.  A plan serves any number of calls, streams and element sizes. */
int zeggs_mirror_plan_create(const int32_t* table, int cols, void** plan);
/* frees a plan once no launch that reads it is pending (the caller's business); NULL is allowed */
int zeggs_mirror_plan_free(void* plan);
int zeggs_mirror_plan_cols(const void* plan);                    /* the plan's column count, -1 when it is no plan */
/* ONE launch: out[rows, cols] <- the signed gather of in[rows, cols] (DEVICE memory, both contiguous, aligned to elem_bytes,
 * elem_bytes 4 or 8).  in and out must not share a byte (-1, nothing is launched); rows == 0 is a no-op. */
int zeggs_mirror_rows(const void* plan, const void* in, void* out, long rows, int elem_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
