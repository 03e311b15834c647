// Left/right mirroring of row tables: a signed column gather (include/zeggs_hip_mirror.h).
//
//   out[r, c] = in[r, source(c)] ^ (flip(c) ? top bit : 0)
//
// Bandwidth-bound, no arithmetic.  ONE kernel, one workgroup per TILE of whole rows (grid-stride over the tiles):
//   1. the tile -- `tile_rows` consecutive rows, one contiguous span of the table -- is copied into LDS with 16-byte loads where
//      the tables are 16-byte aligned (tile_rows is a multiple of the elements of such an access, so every tile of an aligned
//      table starts aligned whatever the row length is: 1137 floats are 4548 bytes), element by element otherwise;
//   2. every lane builds 16 bytes of consecutive OUTPUT elements from LDS -- the gather never leaves the row, so it never leaves
//      the tile -- and stores them with one access: the stores are as coalesced as the loads.
// The table sits in LDS in front of the tile (one read from device memory per workgroup).  Its check (csrc/mirror_table.h, host
// code shared with tests/host/mirror_table_check.cpp) is what bounds every LDS index: a source is < cols, so row * cols + source
// stays inside the rows of the tile that were loaded.
#include "../../include/zeggs_hip_mirror.h"
#include "common.h"
#include "mirror_table.h"

namespace {

constexpr int MIRROR_THREADS = 256;
constexpr size_t MIRROR_TILE_BYTES = 32768;      // per workgroup, + the table (<= 12 KiB): two or more workgroups a CU
constexpr uint64_t MIRROR_MAGIC = 0x5a4d4952524f5231ull;

static_assert(MIRROR_MAX_COLS == ZEGGS_MIRROR_MAX_COLS, "mirror_table.h and the twelfth header disagree");
static_assert((size_t)MIRROR_MAX_COLS * 4 + (size_t)MIRROR_MAX_COLS * 16 <= 65536, "the table and the smallest tile must fit 64 KiB of LDS");

struct MirrorPlan {
  uint64_t magic;
  int cols;
  int* table;      // device
};

template <typename W> struct Vec16;
template <> struct Vec16<uint32_t> { typedef uint32_t T __attribute__((ext_vector_type(4))); };
template <> struct Vec16<uint64_t> { typedef uint64_t T __attribute__((ext_vector_type(2))); };

template <typename W, bool VEC>
__global__ __launch_bounds__(MIRROR_THREADS) void mirror_rows_k(const W* __restrict__ in, W* __restrict__ out, const int* __restrict__ table,
                                                                long rows, int cols, int tile_rows, int table_pad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mirror_lds[];
  typedef typename Vec16<W>::T V;
  constexpr int G = 16 / (int)sizeof(W);
  constexpr W SIGN = (W)1 << (8 * sizeof(W) - 1);
  int* tab = (int*)mirror_lds;
  W* tile = (W*)(mirror_lds + (size_t)table_pad * sizeof(int));
  for (int c = threadIdx.x; c < cols; c += MIRROR_THREADS) tab[c] = table[c];
  const long tiles = (rows + tile_rows - 1) / tile_rows;
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long r0 = t * tile_rows;
    const int nr = (int)(rows - r0 < (long)tile_rows ? rows - r0 : (long)tile_rows);
    const int n = nr * cols;                      // elements of this tile
    const W* src = in + r0 * cols;
    W* dst = out + r0 * cols;
    const int nv = VEC ? n / G : 0;               // whole 16-byte groups; the rest (and everything, unaligned) goes by element
    if (VEC)
      for (int i = threadIdx.x; i < nv; i += MIRROR_THREADS) ((V*)tile)[i] = ((const V*)src)[i];
    for (int i = nv * G + threadIdx.x; i < n; i += MIRROR_THREADS) tile[i] = src[i];
    __syncthreads();                              // (the first pass: the table too)
    if (VEC)
      for (int i = threadIdx.x; i < nv; i += MIRROR_THREADS) {
        const int e = i * G;
        int base = e / cols * cols, c = e - base;
        V v;
#pragma unroll
        for (int k = 0; k < G; ++k) {
          const int s = tab[c];
          const W x = tile[base + (s & 0x7fffffff)];
          v[k] = s < 0 ? (W)(x ^ SIGN) : x;
          if (++c == cols) {
            c = 0;
            base += cols;
          }
        }
        ((V*)dst)[i] = v;
      }
    for (int i = nv * G + threadIdx.x; i < n; i += MIRROR_THREADS) {
      const int base = i / cols * cols;
      const int s = tab[i - base];
      const W x = tile[base + (s & 0x7fffffff)];
      dst[i] = s < 0 ? (W)(x ^ SIGN) : x;
    }
    __syncthreads();                              // the tile is overwritten by the next pass
  }
}

template <typename W>
void mirror_launch(const MirrorPlan* p, const void* in, void* out, long rows, hipStream_t stream) {
  const int tile_rows = mirror_tile_rows(p->cols, (int)sizeof(W), MIRROR_TILE_BYTES);
  const int table_pad = (p->cols + 3) / 4 * 4;
  const size_t lds = (size_t)table_pad * sizeof(int) + (size_t)tile_rows * p->cols * sizeof(W);
  const long tiles = (rows + tile_rows - 1) / tile_rows;
  const dim3 grid((unsigned)(tiles < 2048 ? tiles : 2048)), block(MIRROR_THREADS);
  if ((((uintptr_t)in | (uintptr_t)out) & 15) == 0)
    hipLaunchKernelGGL((mirror_rows_k<W, true>), grid, block, lds, stream, (const W*)in, (W*)out, p->table, rows, p->cols, tile_rows, table_pad);
  else
    hipLaunchKernelGGL((mirror_rows_k<W, false>), grid, block, lds, stream, (const W*)in, (W*)out, p->table, rows, p->cols, tile_rows, table_pad);
}

const MirrorPlan* mirror_plan(const void* plan) {
  const MirrorPlan* p = (const MirrorPlan*)plan;
  return p != nullptr && p->magic == MIRROR_MAGIC ? p : nullptr;
}

}  // namespace

extern "C" int zeggs_mirror_version(void) { return 1; }

extern "C" int zeggs_mirror_table_check(const int32_t* table, int cols) {
  char msg[160];
  ZCHECK(mirror_table_check(table, cols, msg, sizeof msg) == 0, "mirror table: %s", msg);
  return 0;
}

extern "C" int zeggs_mirror_plan_create(const int32_t* table, int cols, void** plan) {
  ZCHECK(plan != nullptr, "mirror plan: NULL result pointer");
  *plan = nullptr;
  ZTRY(zeggs_mirror_table_check(table, cols));
  int* dev = nullptr;
  hipError_t e = hipMalloc((void**)&dev, (size_t)cols * sizeof(int));
  ZCHECK(e == hipSuccess, "mirror plan: hipMalloc: %s", hipGetErrorString(e));
  e = hipMemcpy(dev, table, (size_t)cols * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    ZCHECK(false, "mirror plan: upload: %s", hipGetErrorString(e));
  }
  *plan = new MirrorPlan{MIRROR_MAGIC, cols, dev};
  return 0;
}

extern "C" int zeggs_mirror_plan_free(void* plan) {
  if (plan == nullptr) return 0;
  MirrorPlan* p = (MirrorPlan*)plan;
  ZCHECK(p->magic == MIRROR_MAGIC, "mirror plan: not a plan (or freed already)");
  p->magic = 0;
  const hipError_t e = hipFree(p->table);
  delete p;
  ZCHECK(e == hipSuccess, "mirror plan: hipFree: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int zeggs_mirror_plan_cols(const void* plan) {
  const MirrorPlan* p = mirror_plan(plan);
  ZCHECK(p != nullptr, "mirror plan: not a plan");
  return p->cols;
}

extern "C" int zeggs_mirror_rows(const void* plan, const void* in, void* out, long rows, int elem_bytes, void* stream) {
  const MirrorPlan* p = mirror_plan(plan);
  ZCHECK(p != nullptr, "mirror rows: not a plan");
  ZCHECK(elem_bytes == 4 || elem_bytes == 8, "mirror rows: elements of %d bytes (4 or 8)", elem_bytes);
  ZCHECK(rows >= 0 && rows <= (1l << 40) / p->cols, "mirror rows: %ld rows of %d columns", rows, p->cols);
  if (rows == 0) return 0;
  ZCHECK(in != nullptr && out != nullptr, "mirror rows: NULL table");
  ZCHECK((((uintptr_t)in | (uintptr_t)out) % (uintptr_t)elem_bytes) == 0, "mirror rows: a table is not aligned to its %d-byte elements", elem_bytes);
  const size_t bytes = (size_t)rows * (size_t)p->cols * (size_t)elem_bytes;
  ZCHECK(!mirror_ranges_overlap((uintptr_t)in, (uintptr_t)out, bytes), "mirror rows: in and out overlap (%zu bytes each): the gather is not done in place", bytes);
  if (elem_bytes == 4)
    mirror_launch<uint32_t>(p, in, out, rows, (hipStream_t)stream);
  else
    mirror_launch<uint64_t>(p, in, out, rows, (hipStream_t)stream);
  ZLAUNCH_CHECK("mirror_rows");
  return 0;
}
