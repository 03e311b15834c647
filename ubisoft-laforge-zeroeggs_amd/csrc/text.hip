// BVH motion text on the device: table [rows, cols] float64 -> "%f" + ' ' per number, '\n' per row, the bytes the host's
// snprintf loop (hostio.hip: zeggs_format_table_text) gives, so that what generate / prepare download IS the file content.  The
// digits come from text_math.h (integer arithmetic, checked against glibc on the host: tests/host/text_format_check.cpp).
//
//   measure   one wave per row: width of every number (sign + integer digits + 8), summed -> len[row]; out-of-domain -> status bit
//   scan      inclusive scan of len inside blocks of TEXT_SCAN rows (one row per thread) + one block over the block totals;
//             every offset is 64-bit (a 30-minute clip is 265 MB of text, and nothing keeps a table under 2^31 bytes)
//   emit      one workgroup per row, TEXT_SEG columns at a time: a lane recomputes its number's digits (cheaper than storing
//             them), a block scan of the widths places them, and every lane stores its characters straight to global memory
//             (the row is contiguous, so the bytes of neighbouring lanes meet in the same cache lines).  The other variant
//             (option text_emit = 1) assembles the segment in LDS at the destination's alignment mod 16 and writes aligned
//             16-byte stores with byte stores for the head and the tail; measured equal within the spread on a 4096 x 228 table
//             (emit 18.8 us against 17.6 us per-byte, profiles/bvh_text_device.json: the digit arithmetic and the launches
//             are what costs, 10 MB of text is 1.3 us of HBM time), so the simpler one is the default and this one is kept
//             for measurement.
#include <hip/hip_runtime.h>

#include "../../include/zeggs_hip.h"
#include "common.h"
#include "text_math.h"

int g_text_emit = 0;        // 0: per-byte global stores, 1: LDS assembly + aligned 16-byte stores (tools/bvh_text_bench.py)
int g_text_passes = 7;      // bit 0 measure, bit 1 scan, bit 2 emit: the bench times the passes one by one on a workspace that a
                            // full call has filled; anything but 7 is measurement only

namespace {
constexpr int TEXT_SCAN = 256;      // rows per scan block = threads of the scan kernels
constexpr int TEXT_SEG = 256;       // columns per emit step = threads of the emit kernel
constexpr int TEXT_LDS = 16 + TEXT_SEG * ZT_MAX_WIDTH + 16;      // alignment pad + a full segment + '\n', in 16-byte units below

__device__ inline long long wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// inclusive scan over the TEXT_SCAN threads of a block (sh: TEXT_SCAN / 64 entries); *total = the block's sum
__device__ inline long long block_scan(long long v, long long* sh, long long* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  __syncthreads();            // (sh may still be read from the call before)
  if (lane == 63) sh[w] = v;
  __syncthreads();
  long long before = 0, all = 0;
  for (int i = 0; i < TEXT_SCAN / 64; ++i) {
    if (i < w) before += sh[i];
    all += sh[i];
  }
  *total = all;
  return v + before;
}

__global__ __launch_bounds__(256) void text_measure_k(const double* __restrict__ table, long rows, int cols, long long* __restrict__ len,
                                                      unsigned* __restrict__ status) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);      // (wave-uniform: the shuffles below see whole waves)
  if (row >= rows) return;
  const unsigned long long* p = reinterpret_cast<const unsigned long long*>(table) + row * cols;
  long long w = 0;
  bool bad = false;
  for (int c = threadIdx.x & 63; c < cols; c += 64) {
    const ZtNum n = zt_decompose(p[c]);
    w += zt_width(n);
    bad |= !n.ok;
  }
  w = wave_sum(w);
  if (bad) atomicOr(status, 1u);
  if ((threadIdx.x & 63) == 0) len[row] = w + 1;
}

// len[r] -> inclusive sum inside its block of TEXT_SCAN rows (in place); sums[block] = the block's total
__global__ __launch_bounds__(TEXT_SCAN) void text_scan_rows_k(long long* __restrict__ len, long rows, long long* __restrict__ sums) {
  __shared__ long long sh[TEXT_SCAN / 64];
  const long r = (long)blockIdx.x * TEXT_SCAN + threadIdx.x;
  long long total;
  const long long v = block_scan(r < rows ? len[r] : 0, sh, &total);
  if (r < rows) len[r] = v;
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[0 .. n) -> exclusive scan in place, one block, TEXT_SCAN entries per step
__global__ __launch_bounds__(TEXT_SCAN) void text_scan_sums_k(long long* __restrict__ sums, long n) {
  __shared__ long long sh[TEXT_SCAN / 64];
  long long carry = 0;
  for (long i0 = 0; i0 < n; i0 += TEXT_SCAN) {
    const long i = i0 + threadIdx.x;
    const long long x = i < n ? sums[i] : 0;
    long long total;
    const long long v = block_scan(x, sh, &total);
    if (i < n) sums[i] = carry + v - x;
    carry += total;
  }
}

// row blockIdx.x: text[start, end) with end = sums[block] + len[row] (also written to row_end); a row that would pass `cap` is
// not written at all and sets status bit 1
template <bool BYTES>
__global__ __launch_bounds__(TEXT_SEG) void text_emit_k(const double* __restrict__ table, int cols, const long long* __restrict__ len,
                                                        const long long* __restrict__ sums, char* __restrict__ text, size_t cap,
                                                        long long* __restrict__ row_end, unsigned* __restrict__ status) {
  __shared__ uint4 lds4[BYTES ? 1 : TEXT_LDS / 16];
  __shared__ long long sh[TEXT_SCAN / 64];
  static_assert(TEXT_SEG == TEXT_SCAN, "block_scan spans the emit block");
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  const long long base = sums[row / TEXT_SCAN];
  const long long start = base + (row % TEXT_SCAN ? len[row - 1] : 0), end = base + len[row];
  if (tid == 0) row_end[row] = end;
  if ((unsigned long long)end > (unsigned long long)cap) {      // (block-uniform)
    if (tid == 0) atomicOr(status, 2u);
    return;
  }
  const unsigned long long* p = reinterpret_cast<const unsigned long long*>(table) + row * cols;
  char* dst = text + start;
  char* lds = reinterpret_cast<char*>(lds4);
  for (int c0 = 0; c0 < cols; c0 += TEXT_SEG) {
    const int c = c0 + tid;
    const bool have = c < cols, last = c == cols - 1;
    ZtNum n = zt_decompose(have ? p[c] : 0ULL);
    const int w = have ? zt_width(n) + (last ? 1 : 0) : 0;
    long long seg;
    const int off = (int)block_scan(w, sh, &seg) - w;
    if (BYTES) {
      if (have) {
        char* o = dst + off;
        const int k = zt_put(n, o);
        o[k] = ' ';
        if (last) o[k + 1] = '\n';
      }
    } else {
      const int pad = (int)(reinterpret_cast<uintptr_t>(dst) & 15);      // LDS and global memory agree mod 16
      if (have) {
        char* o = lds + pad + off;
        const int k = zt_put(n, o);
        o[k] = ' ';
        if (last) o[k + 1] = '\n';
      }
      __syncthreads();
      const int nbytes = (int)seg;
      const int head = min(nbytes, (16 - pad) & 15);
      const int nvec = (nbytes - head) >> 4;
      const int tail = nbytes - head - (nvec << 4);
      if (tid < head) dst[tid] = lds[pad + tid];
      uint4* d4 = reinterpret_cast<uint4*>(dst + head);
      const uint4* s4 = lds4 + ((pad + head) >> 4);
      for (int i = tid; i < nvec; i += TEXT_SEG) d4[i] = s4[i];
      if (tid < tail) dst[head + (nvec << 4) + tid] = lds[pad + head + (nvec << 4) + tid];
      __syncthreads();      // (the next segment overwrites the buffer)
    }
    dst += seg;
  }
}
}  // namespace

extern "C" size_t zeggs_table_text_workspace_bytes(long rows, int cols) {
  (void)cols;
  if (rows <= 0) return 0;
  return (size_t)(rows + cdiv(rows, TEXT_SCAN)) * sizeof(long long);
}

extern "C" int zeggs_table_text_device(const double* table, long rows, int cols, char* text, size_t cap, long long* row_end,
                                       unsigned* status, void* ws, size_t ws_bytes, void* stream) {
  ZCHECK(rows >= 0 && cols > 0, "table_text_device: bad shape %ld x %d", rows, cols);
  if (rows == 0) return 0;
  ZCHECK(table && text && row_end && status, "table_text_device: table / text / row_end / status missing");
  ZCHECK(ws && ws_bytes >= zeggs_table_text_workspace_bytes(rows, cols), "table_text_device: workspace too small");
  ZCHECK(rows <= 0x7FFFFFFFL, "table_text_device: more than 2^31 - 1 rows (one workgroup per row)");
  hipStream_t s = (hipStream_t)stream;
  long long* len = (long long*)ws;
  long long* sums = len + rows;
  const int nblk = cdiv(rows, TEXT_SCAN);
  if (g_text_passes & 1) {
    hipLaunchKernelGGL(text_measure_k, dim3(cdiv(rows, 4)), dim3(256), 0, s, table, rows, cols, len, status);
    ZLAUNCH_CHECK("table_text_device (measure)");
  }
  if (g_text_passes & 2) {
    hipLaunchKernelGGL(text_scan_rows_k, dim3(nblk), dim3(TEXT_SCAN), 0, s, len, rows, sums);
    hipLaunchKernelGGL(text_scan_sums_k, dim3(1), dim3(TEXT_SCAN), 0, s, sums, (long)nblk);
    ZLAUNCH_CHECK("table_text_device (scan)");
  }
  if (g_text_passes & 4) {
    if (g_text_emit != 1)
      hipLaunchKernelGGL(text_emit_k<true>, dim3((unsigned)rows), dim3(TEXT_SEG), 0, s, table, cols, len, sums, text, cap, row_end, status);
    else
      hipLaunchKernelGGL(text_emit_k<false>, dim3((unsigned)rows), dim3(TEXT_SEG), 0, s, table, cols, len, sums, text, cap, row_end, status);
    ZLAUNCH_CHECK("table_text_device (emit)");
  }
  return 0;
}
