// The host contract every stage of live serving keeps, stated once: loudness, resampling, the gaze schedule, the style bank, the
// plant stage and the three forms of the output head (through frames_host.h).  A stage has a dims record whose first word of
// refusal is its row count, an opaque block of device memory ("state", "bank") that it is handed with its size, calls on ONE
// row (reset, hold, read), launches over records of which each names a row at most once a call and which travel in the kernel
// arguments when there is one and in device memory when there are more, and a report of where a row lives inside the block.
// What a stage's own fields may hold, the order of its checks, its skip / `work` conditions, its `R == 0` return and its launch
// stay in its unit.  Nothing here asks which stage calls it: `who` is the caller's word in every message.
// Host code only, no kernel: include it behind a unit's kernels (common.h first), so that they stay the first of its code object.
#pragma once
#include "../../include/zeggs_hip_snapshot.h"

namespace {

// ---- the head of a dims record: there is one, and it has 1 .. ZEGGS_LIVE_MAX_ROWS rows
template <class Dims>
int lh_dims_ok(const char* who, const Dims* d) {
  ZCHECK(d != nullptr, "%s: NULL dims", who);
  ZCHECK(d->rows >= 1 && d->rows <= ZEGGS_LIVE_MAX_ROWS, "%s: %d rows (1..%d)", who, d->rows, ZEGGS_LIVE_MAX_ROWS);
  return 0;
}
// ---- the block (`word`: "state", "bank") against `need`, the stage's own size for dims that passed, and the alignment its
// kernels read it at.  bytes == (size_t)-1: the size query of *_state_bytes, which has no block yet
int lh_block_ok(const char* who, const char* word, const void* block, size_t bytes, size_t need, unsigned align) {
  if (bytes == (size_t)-1) return 0;
  ZCHECK(block != nullptr, "%s: NULL %s", who, word);
  ZCHECK(bytes >= need, "%s: %s too small (%zu < %zu)", who, word, bytes, need);
  ZCHECK((uintptr_t)block % align == 0, "%s: misaligned %s", who, word);
  return 0;
}
// ---- the row of a single-row call (`verb`: "reset", "hold", "read")
int lh_row_ok(const char* who, const char* verb, int row, int rows) {
  ZCHECK(row >= 0 && row < rows, "%s %s: row %d of %d", who, verb, row, rows);
  return 0;
}
// ---- the records of a launch: at most one a row ...
int lh_count_ok(const char* who, int R, int rows) {
  ZCHECK(R >= 0 && R <= rows, "%s: %d records for %d rows", who, R, rows);
  return 0;
}
// ... record `i` names a row of the state, and no record before it did (`seen`: one flag a row, the caller's)
int lh_once_ok(const char* who, int i, int row, int rows, bool* seen) {
  ZCHECK(row >= 0 && row < rows, "%s: record %d: row %d of %d", who, i, row, rows);
  ZCHECK(!seen[row], "%s: record %d: row %d twice in one call", who, i, row);
  seen[row] = true;
  return 0;
}
// ... and the device copy of a call that has work: one record travels in the kernel arguments, more do not.  `word`: the
// parameter's name; `align`: what the kernel loads a record at, 0 where the stage never asked
int lh_dev_ok(const char* who, const char* word, const void* dev, int R, unsigned align = 0) {
  ZCHECK(dev != nullptr || R == 1, "%s: %d records must also be in device memory (%s)", who, R, word);
  ZCHECK(align == 0 || dev == nullptr || (uintptr_t)dev % align == 0, "%s: misaligned %s", who, word);
  return 0;
}

// ---- the sources of a record that brings pose frames (the head's records and the plant stage's: the fields have the same
// names), and their leading dimensions.  `pose_floats`: what the caller's kernel reads of a pose row
template <class Row>
int lh_sources_ok(const char* who, int i, const Row& w, int pose_floats) {
  ZCHECK(w.pose != nullptr && (uintptr_t)w.pose % 4 == 0 && w.rpos != nullptr && (uintptr_t)w.rpos % 4 == 0 && w.rrot != nullptr &&
             (uintptr_t)w.rrot % 4 == 0, "%s: record %d: NULL or misaligned source", who, i);
  ZCHECK(w.pose_ld >= pose_floats && w.rpos_ld >= 3 && w.rrot_ld >= 4,
         "%s: record %d: leading dimensions %ld, %ld, %ld (at least %d, 3, 4 floats)", who, i, w.pose_ld, w.rpos_ld, w.rrot_ld,
         pose_floats);
  return 0;
}

// ---- the span report: `count` pieces of a row's state inside the block, count < 0 for a row the dims do not have
int lh_spans_out(const char* who, int count, int row, int rows, int max_spans, const size_t* offset, const size_t* bytes, ZeggsSnapSpan* spans) {
  ZCHECK(count >= 0, "%s: row %d of %d", who, row, rows);
  ZCHECK(spans != nullptr && max_spans >= count, "%s: room for %d spans, the row has %d", who, spans ? max_spans : 0, count);
  for (int i = 0; i < count; ++i) spans[i] = ZeggsSnapSpan{offset[i], bytes[i]};
  return count;
}

}  // namespace
