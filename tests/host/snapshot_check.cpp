// Host check of csrc/snapshot_math.h, the header that says where a live row's state lives inside each opaque state block
// (include/zeggs_hip_snapshot.h: the span reports) and how the snapshot launch cuts its work.  Stand-alone: its own main, no HIP,
// built and run plain and under the address and undefined-behaviour sanitizers by tests/test_live_snapshot_cpu.py.
//
// Per family -- running loudness (sampling rates 16000 and 48000, rings of 1 and 2^20 blocks), the rate converter (histories 2 and
// 3072), the output head in its plain, re-timing and filtering form (1, 5 and 75 joints; max_half 0, 4 and 16) -- and rows = 1, 2
// and 64 it walks the rules of the eighth header:
//   * the number of spans, their sizes and their order are the same for every row and every `rows`; in particular the list of
//     row 0 at rows = 1 equals, in sizes and order, that of row 63 at rows = 64;
//   * every offset and size is a multiple of 4;
//   * the spans of a row are disjoint and inside the block; the spans of two rows are disjoint;
//   * all rows' spans together with what the family declares derived (the heads' skeleton tables) are exactly the block;
//   * a row out of range and a list that is too short give -1;
// and of the launch: the chunks of a size cover it, the dword head of any address is 0 .. 3 words and brings it to 16 bytes.
// With --table it prints the spans of row 63 at rows = 64 per case, which the test compares with the library's own reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../../ubisoft-laforge-zeroeggs_amd/csrc/snapshot_math.h"

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      ++failures;                                 \
      fprintf(stderr, "snapshot_check: ");        \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, " [%s]\n", #cond);          \
      if (failures > 20) exit(1);                 \
    }                                             \
  } while (0)

struct Span { size_t off, bytes; };
// spans(rows, row, offsets, sizes, cap) -> count; block(rows) -> bytes of the state block; derived: bytes in no span
using Spans = std::function<int(int, int, size_t*, size_t*, int)>;
using Block = std::function<size_t(int)>;

static std::vector<Span> list(const Spans& f, int rows, int row) {
  size_t o[SNAP_MAX_SPANS], b[SNAP_MAX_SPANS];
  const int n = f(rows, row, o, b, SNAP_MAX_SPANS);
  std::vector<Span> out;
  for (int i = 0; i < n; ++i) out.push_back(Span{o[i], b[i]});
  return out;
}

static void family(const char* name, const Spans& f, const Block& block, size_t derived, bool table) {
  const int ROWS[3] = {1, 2, 64};
  const std::vector<Span> first = list(f, 1, 0);
  CHECK(!first.empty() && (int)first.size() <= SNAP_MAX_SPANS, "%s: %zu spans", name, first.size());
  for (int rows : ROWS) {
    const size_t total = block(rows);
    std::vector<Span> all;
    size_t sum = 0;
    for (int row = 0; row < rows; ++row) {
      const std::vector<Span> s = list(f, rows, row);
      CHECK(s.size() == first.size(), "%s: rows %d row %d: %zu spans, row 0 of 1 has %zu", name, rows, row, s.size(), first.size());
      for (size_t i = 0; i < s.size() && i < first.size(); ++i) {
        CHECK(s[i].bytes == first[i].bytes, "%s: rows %d row %d span %zu: %zu bytes, row 0 of 1 has %zu", name, rows, row, i, s[i].bytes, first[i].bytes);
        CHECK(s[i].off % 4 == 0 && s[i].bytes % 4 == 0 && s[i].bytes > 0, "%s: rows %d row %d span %zu: offset %zu, %zu bytes", name, rows, row, i,
              s[i].off, s[i].bytes);
        CHECK(s[i].off + s[i].bytes <= total, "%s: rows %d row %d span %zu ends at %zu of %zu", name, rows, row, i, s[i].off + s[i].bytes, total);
        all.push_back(s[i]);
        sum += s[i].bytes;
      }
    }
    for (size_t a = 0; a < all.size(); ++a)           // disjoint: within a row and between rows alike
      for (size_t b = a + 1; b < all.size(); ++b)
        CHECK(all[a].off + all[a].bytes <= all[b].off || all[b].off + all[b].bytes <= all[a].off, "%s: rows %d: spans %zu and %zu overlap", name, rows, a, b);
    CHECK(sum + derived == total, "%s: rows %d: the spans hold %zu bytes and %zu are derived, the block has %zu", name, rows, sum, derived, total);
    size_t o[SNAP_MAX_SPANS], b[SNAP_MAX_SPANS];
    CHECK(f(rows, rows, o, b, SNAP_MAX_SPANS) == -1 && f(rows, -1, o, b, SNAP_MAX_SPANS) == -1, "%s: rows %d: a row out of range is taken", name, rows);
    CHECK(f(rows, 0, o, b, (int)first.size() - 1) == -1, "%s: rows %d: a list that is too short is taken", name, rows);
  }
  const std::vector<Span> last = list(f, 64, 63);
  CHECK(last.size() == first.size(), "%s: row 63 of 64 has %zu spans, row 0 of 1 %zu", name, last.size(), first.size());
  if (table) {
    printf("%s", name);
    for (const Span& s : last) printf(" %zu %zu", s.off, s.bytes);
    printf("\n");
  }
}

int main(int argc, char** argv) {
  const bool table = argc > 1 && strcmp(argv[1], "--table") == 0;
  char name[96];
  for (int fs : {16000, 48000})
    for (int nb : {1, 1 << 20}) {
      snprintf(name, sizeof name, "loudness %d %d", fs, nb);
      family(name, [=](int rows, int row, size_t* o, size_t* b, int cap) { return snap_loud_spans(fs, nb, rows, row, o, b, cap); },
             [=](int rows) { return (size_t)rows * loud_state_row_bytes(fs, nb); }, 0, table);
    }
  for (int history : {2, 3072}) {
    snprintf(name, sizeof name, "resample %d", history);
    family(name, [=](int rows, int row, size_t* o, size_t* b, int cap) { return snap_resample_spans(history, rows, row, o, b, cap); },
           [=](int rows) { return (size_t)rows * rs_state_row_bytes(history); }, 0, table);
  }
  for (int J : {1, 5, 75}) {
    snprintf(name, sizeof name, "frames %d", J);
    family(name, [=](int rows, int row, size_t* o, size_t* b, int cap) { return snap_frames_spans(J, rows, row, o, b, cap); },
           [=](int rows) { return (size_t)fr_state_bytes(rows, J); }, (size_t)fr_tables_bytes(J), table);
    snprintf(name, sizeof name, "retime %d", J);
    family(name, [=](int rows, int row, size_t* o, size_t* b, int cap) { return snap_retime_spans(J, rows, row, o, b, cap); },
           [=](int rows) { return (size_t)rt_state_bytes(rows, J); }, (size_t)fr_tables_bytes(J), table);
    for (int mh : {0, 4, 16}) {
      snprintf(name, sizeof name, "refilter %d %d", J, mh);
      family(name, [=](int rows, int row, size_t* o, size_t* b, int cap) { return snap_refilter_spans(J, mh, rows, row, o, b, cap); },
             [=](int rows) { return (size_t)rf_state_bytes(rows, J, mh); }, (size_t)fr_tables_bytes(J), table);
    }
  }
  // ---- the launch: chunks cover a size; the dword head brings an address to its 16-byte boundary or ends the segment
  for (size_t bytes : {(size_t)4, (size_t)12, (size_t)SNAP_CHUNK - 4, (size_t)SNAP_CHUNK, (size_t)SNAP_CHUNK + 4, (size_t)71680, (size_t)1 << 31}) {
    const long c = snap_chunks(bytes);
    CHECK((size_t)c * SNAP_CHUNK >= bytes && (size_t)(c - 1) * SNAP_CHUNK < bytes, "%zu bytes in %ld chunks", bytes, c);
    // the 16-byte lanes of a chunk are the chunk's share of the words: no chunk count below what the lanes need
    CHECK((size_t)c * SNAP_THREADS * SNAP_LANES >= bytes / 16, "%zu bytes: %ld chunks for %zu lanes", bytes, c, bytes / 16);
  }
  for (size_t a = 0x1000; a < 0x1020; a += 4)
    for (long words : {1L, 2L, 3L, 4L, 100L}) {
      const long h = snap_head_words(a, words);
      CHECK(h >= 0 && h <= 3 && h <= words, "address %zx, %ld words: head %ld", a, words, h);
      CHECK(h == words || (a + 4 * (size_t)h) % 16 == 0, "address %zx, %ld words: head %ld does not reach a 16-byte boundary", a, words, h);
    }
  if (failures) return 1;
  printf("snapshot_check: ok\n");
  return 0;
}
