/* C ABI of libzeggs_hip.so, eighth header: snapshot and restore of a live row's state
 * (zeggs_live_snapshot_version() >= 1; zeggs_version() and the versions of the other headers stay what they are).
 *
 * The other seven headers are closed sets (their tests pin their prototypes and structs); the entry points below have a header
 * of their own.  Same conventions as include/zeggs_hip_refilter.h: the caller owns all memory, calls only enqueue on `stream`,
 * 0 on success / -1 with zeggs_last_error().  The Python mirror is zeggs/capi.py: SNAP_STRUCTS / SNAP_PROTOTYPES
 * (tests/test_live_snapshot_cpu.py compares the two).
 *
 * Two things are here.  The SPAN REPORTS say where a row's state lives inside each opaque state block of live serving: host
 * only, one function per state family, over the family's dims and the extra arguments its *_state_bytes function takes.  Given
 * a row, a function fills spans[0 .. count - 1] with {offset, bytes} into the state block and returns the count (at most
 * ZEGGS_SNAP_MAX_SPANS), or -1 with zeggs_last_error() when `max_spans` is too small, the row is out of range or the dims are
 * refused.  Together a row's spans are every byte of the block that belongs to that row and nothing else:
 *   - the number of spans, their sizes and their order depend on the dims other than `rows`, never on `row` or d->rows: a row
 *     taken from a 64-row block goes into row 1 of a 2-row block;
 *   - every offset and size is a multiple of 4; the spans of a row are disjoint and inside *_state_bytes; the spans of two
 *     rows are disjoint.
 * What a block holds that is derived and not state is in no span: the skeleton tables that zeggs_live_frames_prepare,
 * zeggs_live_retime_prepare and zeggs_live_refilter_prepare write in front of the rows (a destination has its own, from its own
 * prepare).  Loudness: 2 spans (the head: filter states, counters, estimate, gain and flags; the rings of filtered samples,
 * block energies and levels).  The converter: 1 (the ring of input samples).  The three heads: 1 each (placement, flags, the
 * quaternions last emitted, and behind them the raw input frame(s) the re-timing and the filtering head keep).  The arithmetic
 * is csrc/snapshot_math.h, shared with the kernels that own the layouts.
 *
 * PACK and UNPACK move many such pieces between their places on the device and one contiguous blob on the device, ONE launch
 * for any number of records (csrc/live_snapshot.hip: the grid runs over segment x chunk, the records are read from device
 * memory).  A record names the STATE side by address (`src`), the BLOB side by offset: zeggs_live_pack copies
 * src[0 .. bytes) to blob + dst_offset, zeggs_live_unpack copies blob + dst_offset .. back to src (the same records with the
 * direction reversed: `src` is written).  A record whose two sides share their offset within 16 bytes moves in 16-byte lanes,
 * any other dword by dword: lay the blob out so that the first is the rule.
 * Checks, all on the host ahead of the launch and naming the record they refuse: a NULL or misaligned (4 bytes) pointer, a
 * size that is no multiple of 4, dst_offset + bytes past blob_bytes, two records whose blob ranges overlap; also a NULL or
 * misaligned blob and more than ZEGGS_SNAP_MAX_SEGMENTS records.  A record of 0 bytes is skipped; n == 0 launches nothing.
 * The state sides are the caller's: unpack into two records that name overlapping state writes both. */
#ifndef ZEGGS_HIP_SNAPSHOT_H
#define ZEGGS_HIP_SNAPSHOT_H
#include "zeggs_hip_loudness.h"
#include "zeggs_hip_refilter.h"
#include "zeggs_hip_resample.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZEGGS_SNAP_MAX_SPANS 2
#define ZEGGS_SNAP_MAX_SEGMENTS 65535

/* a piece of a state block: byte offset from the block's start, byte count */
typedef struct {
  size_t offset, bytes;
} ZeggsSnapSpan;

/* one piece of a pack / unpack call: the state side (device memory), where it sits in the blob, its size */
typedef struct {
  const void* src;
  size_t dst_offset;
  size_t bytes;
} ZeggsSnapSeg;

int zeggs_live_snapshot_version(void);

/* the span reports (host only) */
int zeggs_live_loudness_spans(const ZeggsLoudDims*, int row, ZeggsSnapSpan* spans, int max_spans);
int zeggs_resample_spans(const ZeggsResampleDims*, int row, ZeggsSnapSpan* spans, int max_spans);
int zeggs_live_frames_spans(const ZeggsFramesDims*, int row, ZeggsSnapSpan* spans, int max_spans);
int zeggs_live_retime_spans(const ZeggsFramesDims*, int row, ZeggsSnapSpan* spans, int max_spans);
int zeggs_live_refilter_spans(const ZeggsFramesDims*, int max_half, int row, ZeggsSnapSpan* spans, int max_spans);

/* segs_host: the records in HOST memory for the checks; segs_dev: the same records in DEVICE memory, which the kernel reads */
int zeggs_live_pack(const ZeggsSnapSeg* segs_host, const ZeggsSnapSeg* segs_dev, int n, void* blob_dev, size_t blob_bytes, void* stream);
int zeggs_live_unpack(const ZeggsSnapSeg* segs_host, const ZeggsSnapSeg* segs_dev, int n, const void* blob_dev, size_t blob_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
