// The signed column table of the mirror kernel (include/zeggs_hip_mirror.h) and its check: host code, shared by csrc/mirror.hip
// and the stand-alone program tests/host/mirror_table_check.cpp.  No HIP, no library state: the message goes into a caller's buffer.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

constexpr int MIRROR_MAX_COLS = 3072;     // ZEGGS_MIRROR_MAX_COLS: the table and a tile of four rows fit 64 KiB of LDS

// one entry: the source column in the low 31 bits, the sign flip in bit 31
inline int mirror_entry_source(int32_t e) { return (int)((uint32_t)e & 0x7fffffffu); }
inline bool mirror_entry_flips(int32_t e) { return ((uint32_t)e >> 31) != 0u; }
inline int32_t mirror_entry(int source, bool flip) { return (int32_t)((uint32_t)source | (flip ? 0x80000000u : 0u)); }

// 0: `table` names every column 0 .. cols - 1 exactly once; -1 with the first offence in `msg` (always terminated)
inline int mirror_table_check(const int32_t* table, int cols, char* msg, size_t msg_len) {
  if (table == nullptr) {
    snprintf(msg, msg_len, "NULL table");
    return -1;
  }
  if (cols < 1 || cols > MIRROR_MAX_COLS) {
    snprintf(msg, msg_len, "%d columns (1..%d)", cols, MIRROR_MAX_COLS);
    return -1;
  }
  std::vector<int> first((size_t)cols, -1);
  for (int c = 0; c < cols; ++c) {
    const int s = mirror_entry_source(table[c]);
    if (s >= cols) {
      snprintf(msg, msg_len, "column %d: source %d of %d columns", c, s, cols);
      return -1;
    }
    if (first[(size_t)s] >= 0) {
      snprintf(msg, msg_len, "column %d: source %d is also the source of column %d (not a bijection)", c, s, first[(size_t)s]);
      return -1;
    }
    first[(size_t)s] = c;
  }
  return 0;
}

// rows of a tile: as many as fit `tile_bytes`, a multiple of the elements of a 16-byte access (so that every tile of an aligned
// table starts on a 16-byte boundary), at least one such group
inline int mirror_tile_rows(int cols, int elem_bytes, size_t tile_bytes) {
  const int group = 16 / elem_bytes;
  long fit = (long)(tile_bytes / ((size_t)cols * (size_t)elem_bytes));
  fit = fit / group * group;
  return (int)(fit < group ? group : fit);
}

// do the byte ranges [a, a + n) and [b, b + n) share a byte
inline bool mirror_ranges_overlap(uintptr_t a, uintptr_t b, size_t n) { return n != 0 && a < b + n && b < a + n; }
