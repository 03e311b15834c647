// Where a live row's state lives inside each opaque state block of live serving, stated once: the spans -- byte offset and byte
// count -- that together are every byte of a block that belongs to one row and nothing else, per state family (running
// loudness, the rate converter, the output head in its plain, re-timing and filtering form), and the rules the snapshot launch
// (live_snapshot.hip) cuts its work by.  Plain C++ behind the qualifier macros of the families' own headers (no HIP include), so
// the same text runs in the kernels that own the layouts (live_loudness.hip and live_resample.hip size and address their rows
// through it; the three heads through frames_math.h / retime_math.h / refilter_math.h, which it only combines), in the host
// side of live_snapshot.hip and in tests/host/snapshot_check.cpp.  The definition is DESIGN.md 3.7.
//
// The rules every span list obeys (tests/host/snapshot_check.cpp walks them): the number of spans, their sizes and their order
// depend on the dims other than `rows`, never on the row; offsets and sizes are multiples of 4; the spans of a row are disjoint
// and inside the block; the spans of two rows are disjoint.  What a family keeps per block that is derived and not state -- the
// skeleton tables *_prepare writes in front of the heads' rows -- is in no span.
#pragma once
#include <stddef.h>

#include "loud_math.h"
#include "refilter_math.h"
#include "resample_math.h"

#define SNAP_MAX_SPANS 2          // the most spans any family reports for a row
#define SNAP_MAX_ROWS 64          // ZEGGS_LIVE_MAX_ROWS

// ---- running loudness: rows one behind another, each [head, LOUD_HEAD_BYTES: filter states, counters, estimate, gain, flags |
// ring of the last block's filtered samples double[loud_block_len(fs)] | block energies double[ring_blocks] | block levels
// double[ring_blocks]].  Two spans: the head, the three rings.
#define LOUD_HEAD_BYTES 128
ZL_HD size_t loud_rings_bytes(int fs, int ring_blocks) { return sizeof(double) * ((size_t)loud_block_len(fs) + 2 * (size_t)ring_blocks); }
ZL_HD size_t loud_state_row_bytes(int fs, int ring_blocks) { return LOUD_HEAD_BYTES + loud_rings_bytes(fs, ring_blocks); }
ZL_HD int snap_loud_spans(int fs, int ring_blocks, int rows, int row, size_t* offset, size_t* bytes, int cap) {
  if (row < 0 || row >= rows || cap < 2) return -1;
  const size_t base = (size_t)row * loud_state_row_bytes(fs, ring_blocks);
  offset[0] = base;
  bytes[0] = LOUD_HEAD_BYTES;
  offset[1] = base + LOUD_HEAD_BYTES;
  bytes[1] = loud_rings_bytes(fs, ring_blocks);
  return 2;
}

// ---- the rate converter: rows one behind another, each a ring of `history` float32 input samples.  One span.
ZR_HD size_t rs_state_row_bytes(int history) { return (size_t)history * sizeof(float); }
ZR_HD int snap_resample_spans(int history, int rows, int row, size_t* offset, size_t* bytes, int cap) {
  if (row < 0 || row >= rows || cap < 1) return -1;
  offset[0] = (size_t)row * rs_state_row_bytes(history);
  bytes[0] = rs_state_row_bytes(history);
  return 1;
}

// ---- the output heads: the skeleton tables (derived: *_prepare writes them from parents and seq; in no span), then the rows,
// each one piece -- the placement, the two flags and the quaternions last emitted; behind them the re-timing head's last raw
// input frame, or the filtering head's ring of 2 max_half raw input frames.  One span each.
ZF_HD int snap_frames_spans(int J, int rows, int row, size_t* offset, size_t* bytes, int cap) {
  if (row < 0 || row >= rows || cap < 1) return -1;
  offset[0] = (size_t)fr_row_offset(J, row);
  bytes[0] = (size_t)fr_row_bytes(J);
  return 1;
}
ZF_HD int snap_retime_spans(int J, int rows, int row, size_t* offset, size_t* bytes, int cap) {
  if (row < 0 || row >= rows || cap < 1) return -1;
  offset[0] = (size_t)rt_row_offset(J, row);
  bytes[0] = (size_t)rt_row_bytes(J);
  return 1;
}
ZF_HD int snap_refilter_spans(int J, int max_half, int rows, int row, size_t* offset, size_t* bytes, int cap) {
  if (row < 0 || row >= rows || cap < 1) return -1;
  offset[0] = (size_t)rf_row_offset(J, max_half, row);
  bytes[0] = (size_t)rf_row_bytes(J, max_half);
  return 1;
}

// ---- the launch of zeggs_live_pack / zeggs_live_unpack: blockIdx.y = segment, blockIdx.x = chunk of SNAP_CHUNK bytes of it, one
// 16-byte lane per thread and SNAP_LANES passes: 1 KiB per wave instruction, the widest a wave moves, and a chunk that is a
// whole number of them.  A segment whose two sides share their offset within 16 bytes moves in 16-byte lanes between a dword
// head and tail; any other moves dword by dword (coalesced either way).  All of it in 4-byte words.
#define SNAP_THREADS 256
#define SNAP_LANES 4
#define SNAP_CHUNK (SNAP_THREADS * SNAP_LANES * 16)
#define SNAP_MAX_SEGMENTS 65535   // gridDim.y
ZF_HD long snap_chunks(size_t bytes) { return (long)((bytes + SNAP_CHUNK - 1) / SNAP_CHUNK); }
// words of the dword head of a segment whose state side sits at address `a` (both sides congruent mod 16), of `words` words
ZF_HD long snap_head_words(size_t a, long words) {
  const long head = (long)(((16 - (a & 15)) & 15) >> 2);
  return head < words ? head : words;
}
