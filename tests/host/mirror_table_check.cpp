// Host check of csrc/mirror_table.h: the signed column table of the mirror kernel (include/zeggs_hip_mirror.h), its bijection
// check, the tile rule and the overlap rule.  Stand-alone: its own main, no HIP, built and run plain and under the address and
// undefined-behaviour sanitizers by tests/test_mirror_cpu.py.
//
//   * entries: source and flip survive the packing for sources 0 .. 2^31 - 1, a flipped column 0 is INT32_MIN;
//   * accepted tables: identity, all flipped, reversal, a seeded random signed involution, at 1, 2, 63, 64, 65, 225, 1137 and
//     MIRROR_MAX_COLS columns;
//   * refused, with the offending column in the message: a duplicate source (with and without a flip on one of the two), a source
//     == cols, a source of 2^31 - 1, 0 columns, MIRROR_MAX_COLS + 1 columns, a NULL table;
//   * the host model of the kernel -- out[c] = in[source(c)] with the top bit flipped -- applied twice with an involutive table
//     gives back the input's bits, -0.0, infinities and NaN payloads included;
//   * the tile rule: rows are a positive multiple of 16 / elem_bytes, the tile and the table fit 64 KiB of LDS at every column
//     count, and every LDS index row * cols + source of a checked table is inside the tile;
//   * the overlap rule: equal, nested, touching and disjoint ranges.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ubisoft-laforge-zeroeggs_amd/csrc/mirror_table.h"

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      ++failures;                                 \
      fprintf(stderr, "mirror_table_check: ");    \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, " [%s]\n", #cond);          \
      if (failures > 20) exit(1);                 \
    }                                             \
  } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rng() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

// a random signed involution: columns paired at random (some left alone), a pair shares its sign
static std::vector<int32_t> involution(int cols) {
  std::vector<int> order((size_t)cols);
  for (int i = 0; i < cols; ++i) order[(size_t)i] = i;
  for (int i = cols - 1; i > 0; --i) {
    const int j = (int)(rng() % (uint32_t)(i + 1));
    const int t = order[(size_t)i];
    order[(size_t)i] = order[(size_t)j];
    order[(size_t)j] = t;
  }
  std::vector<int32_t> table((size_t)cols);
  int i = 0;
  while (i < cols) {
    const bool flip = (rng() & 1u) != 0u;
    if (i + 1 < cols && rng() % 4u != 0u) {
      table[(size_t)order[(size_t)i]] = mirror_entry(order[(size_t)i + 1], flip);
      table[(size_t)order[(size_t)i + 1]] = mirror_entry(order[(size_t)i], flip);
      i += 2;
    } else {
      table[(size_t)order[(size_t)i]] = mirror_entry(order[(size_t)i], flip);
      i += 1;
    }
  }
  return table;
}

template <typename W>
static std::vector<W> apply(const std::vector<int32_t>& table, const std::vector<W>& in) {
  const W sign = (W)1 << (8 * sizeof(W) - 1);
  std::vector<W> out(in.size());
  for (size_t c = 0; c < in.size(); ++c) {
    const W x = in[(size_t)mirror_entry_source(table[c])];
    out[c] = mirror_entry_flips(table[c]) ? (W)(x ^ sign) : x;
  }
  return out;
}

static bool refused(const std::vector<int32_t>& table, const char* needle) {
  char msg[160] = "";
  const int rc = mirror_table_check(table.data(), (int)table.size(), msg, sizeof msg);
  return rc == -1 && strstr(msg, needle) != nullptr;
}

int main() {
  char msg[160];
  // entries
  CHECK(mirror_entry(0, true) == INT32_MIN && mirror_entry(0, false) == 0, "packing of column 0");
  for (int s : {0, 1, 1136, 3071, 0x7fffffff})
    for (bool f : {false, true}) {
      const int32_t e = mirror_entry(s, f);
      CHECK(mirror_entry_source(e) == s && mirror_entry_flips(e) == f, "entry %d %d", s, (int)f);
    }
  // accepted tables, and twice an involution is the identity on every bit pattern
  const uint32_t special32[] = {0x80000000u, 0x00000000u, 0x7f800000u, 0xff800000u, 0x7fc00001u, 0xffc12345u, 0x7f800001u, 0x00000001u};
  const uint64_t special64[] = {0x8000000000000000ull, 0ull, 0x7ff0000000000000ull, 0xfff0000000000000ull, 0x7ff8000000000001ull,
                                0xfff8123456789abcull, 0x7ff0000000000001ull, 1ull};
  for (int cols : {1, 2, 63, 64, 65, 225, 1137, MIRROR_MAX_COLS}) {
    std::vector<int32_t> ident((size_t)cols), neg((size_t)cols), rev((size_t)cols);
    for (int c = 0; c < cols; ++c) {
      ident[(size_t)c] = mirror_entry(c, false);
      neg[(size_t)c] = mirror_entry(c, true);
      rev[(size_t)c] = mirror_entry(cols - 1 - c, (c & 1) == ((cols - 1 - c) & 1) && (c & 1));
    }
    const std::vector<int32_t> inv = involution(cols);
    const std::vector<int32_t>* tables[] = {&ident, &neg, &rev, &inv};
    for (const std::vector<int32_t>* t : tables) {
      CHECK(mirror_table_check(t->data(), cols, msg, sizeof msg) == 0, "%d columns refused: %s", cols, msg);
      std::vector<uint32_t> a((size_t)cols);
      std::vector<uint64_t> b((size_t)cols);
      for (int c = 0; c < cols; ++c) {
        a[(size_t)c] = c % 3 == 0 ? special32[(size_t)(c / 3) % 8] : rng() * 2654435761u;
        b[(size_t)c] = c % 3 == 0 ? special64[(size_t)(c / 3) % 8] : ((uint64_t)rng() << 40) ^ ((uint64_t)rng() << 16) ^ rng();
      }
      CHECK(apply(*t, apply(*t, a)) == a, "%d columns: twice is not the identity (4-byte elements)", cols);
      CHECK(apply(*t, apply(*t, b)) == b, "%d columns: twice is not the identity (8-byte elements)", cols);
    }
    if (cols >= 8) {
      std::vector<uint32_t> a((size_t)cols, 0u);
      for (int c = 0; c < 8; ++c) a[(size_t)c] = special32[c];
      const std::vector<uint32_t> o = apply(neg, a);
      for (int c = 0; c < 8; ++c) CHECK(o[(size_t)c] == (special32[c] ^ 0x80000000u), "flip of %08x", special32[c]);
    }
    // the tile rule and the LDS indices
    for (int eb : {4, 8}) {
      const int tr = mirror_tile_rows(cols, eb, 32768);
      const int table_pad = (cols + 3) / 4 * 4;
      CHECK(tr >= 16 / eb && tr % (16 / eb) == 0, "%d columns of %d bytes: %d rows a tile", cols, eb, tr);
      CHECK((size_t)table_pad * 4 + (size_t)tr * (size_t)cols * (size_t)eb <= 65536, "%d columns of %d bytes: %d rows do not fit", cols, eb, tr);
      CHECK((size_t)tr * (size_t)cols * (size_t)eb <= 32768 || tr == 16 / eb, "%d columns of %d bytes: %d rows are more than the budget", cols, eb, tr);
      long worst = 0;
      for (int c = 0; c < cols; ++c) {
        const long idx = (long)(tr - 1) * cols + mirror_entry_source(inv[(size_t)c]);
        worst = idx > worst ? idx : worst;
      }
      CHECK(worst < (long)tr * cols, "%d columns: LDS index %ld outside a tile of %d rows", cols, worst, tr);
    }
  }
  // refused tables
  CHECK(refused({0, 0}, "column 1: source 0 is also the source of column 0"), "duplicate source");
  CHECK(refused({1, mirror_entry(1, true), 2}, "column 1: source 1 is also the source of column 0"), "duplicate source under a flip");
  CHECK(refused({0, 2}, "column 1: source 2 of 2 columns"), "source == cols");
  CHECK(refused({0, 0x7fffffff, 1}, "column 1: source 2147483647 of 3 columns"), "huge source");
  CHECK(refused({mirror_entry(3, true), 1, 2}, "column 0: source 3 of 3 columns"), "source == cols under a flip");
  CHECK(mirror_table_check(nullptr, 4, msg, sizeof msg) == -1 && strstr(msg, "NULL"), "NULL table");
  {
    std::vector<int32_t> big((size_t)MIRROR_MAX_COLS + 1, 0);
    CHECK(mirror_table_check(big.data(), 0, msg, sizeof msg) == -1 && strstr(msg, "0 columns"), "0 columns");
    CHECK(mirror_table_check(big.data(), -1, msg, sizeof msg) == -1, "-1 columns");
    CHECK(mirror_table_check(big.data(), MIRROR_MAX_COLS + 1, msg, sizeof msg) == -1 && strstr(msg, "3073 columns"), "too many columns");
    char tiny[8];
    CHECK(mirror_table_check(big.data(), MIRROR_MAX_COLS + 1, tiny, sizeof tiny) == -1 && strlen(tiny) == 7, "a short message buffer is terminated");
  }
  // the overlap rule
  CHECK(mirror_ranges_overlap(1000, 1000, 16), "equal ranges");
  CHECK(mirror_ranges_overlap(1000, 1008, 16) && mirror_ranges_overlap(1008, 1000, 16), "shifted ranges");
  CHECK(mirror_ranges_overlap(1000, 1015, 16) && mirror_ranges_overlap(1015, 1000, 16), "one shared byte");
  CHECK(!mirror_ranges_overlap(1000, 1016, 16) && !mirror_ranges_overlap(1016, 1000, 16), "touching ranges");
  CHECK(!mirror_ranges_overlap(1000, 1000, 0), "empty ranges");
  if (failures) return 1;
  printf("mirror_table_check: ok\n");
  return 0;
}
