// Live serving: snapshot and restore of a row's state (include/zeggs_hip_snapshot.h).
//
// The span reports are the host side of snapshot_math.h: where a row's state lives inside each opaque state block.
//
// zeggs_live_pack / zeggs_live_unpack gather many pieces of device memory into one blob, or scatter them back, in ONE launch
// whatever their number: a tick's failover snapshot of 64 rows is about a thousand pieces, from 12 bytes (a root position) to
// a few hundred KiB (a sample window that has grown), far past what zeggs_copy_segments takes.  blockIdx.y = record, blockIdx.x
// = chunk of SNAP_CHUNK bytes of it; the grid's x extent is that of the largest record and a workgroup past its record's end
// leaves at once -- for the sizes above that is a few thousand workgroups of which most are one load and a branch, against one
// launch per piece.  The records are read from device memory (one 24-byte load per workgroup, uniform).  A record whose state
// side and blob side share their offset within 16 bytes moves in 16-byte lanes, 1 KiB per wave instruction, between a dword
// head and tail that chunk 0 moves; any other record moves dword by dword, coalesced as well.  Plain loads and stores, no LDS,
// nothing indexed in registers.
#include "../../include/zeggs_hip_snapshot.h"
#include "common.h"
#include "snapshot_math.h"

#include <algorithm>
#include <vector>

namespace {

static_assert(SNAP_MAX_SPANS == ZEGGS_SNAP_MAX_SPANS && SNAP_MAX_SEGMENTS == ZEGGS_SNAP_MAX_SEGMENTS && SNAP_MAX_ROWS == ZEGGS_LIVE_MAX_ROWS,
              "snapshot_math.h and the eighth header disagree");

template <bool PACK>
__global__ __launch_bounds__(SNAP_THREADS) void live_snapshot_k(const ZeggsSnapSeg* __restrict__ segs, char* blob) {
  const ZeggsSnapSeg sg = segs[blockIdx.y];
  const long words = (long)(sg.bytes >> 2);
  const long chunk = blockIdx.x;
  if (chunk * (SNAP_CHUNK / 4) >= words) return;
  unsigned* state = (unsigned*)const_cast<void*>(sg.src);
  unsigned* piece = (unsigned*)(blob + sg.dst_offset);
  const unsigned* from = PACK ? state : piece;
  unsigned* to = PACK ? piece : state;
  const int tid = threadIdx.x;
  if ((((uintptr_t)state ^ (uintptr_t)piece) & 15) == 0) {
    const long head = snap_head_words((size_t)(uintptr_t)state, words);
    const long nv = (words - head) >> 2, tail0 = head + 4 * nv;
    const uint4* fv = (const uint4*)(from + head);
    uint4* tv = (uint4*)(to + head);
    const long v0 = chunk * (SNAP_THREADS * SNAP_LANES);
#pragma unroll
    for (int p = 0; p < SNAP_LANES; ++p) {
      const long i = v0 + p * SNAP_THREADS + tid;
      if (i < nv) tv[i] = fv[i];
    }
    if (chunk == 0) {          // at most 3 words in front and 3 behind
      if (tid < head) to[tid] = from[tid];
      if (tail0 + tid < words) to[tail0 + tid] = from[tail0 + tid];
    }
  } else {
    const long w0 = chunk * (SNAP_CHUNK / 4);
#pragma unroll 4
    for (int p = 0; p < SNAP_CHUNK / 4 / SNAP_THREADS; ++p) {
      const long i = w0 + p * SNAP_THREADS + tid;
      if (i < words) to[i] = from[i];
    }
  }
}

int snap_launch(const char* who, bool pack, const ZeggsSnapSeg* segs, const ZeggsSnapSeg* segs_dev, int n, const void* blob, size_t blob_bytes,
                void* stream) {
  ZCHECK(n >= 0 && n <= ZEGGS_SNAP_MAX_SEGMENTS, "%s: %d records (0..%d)", who, n, ZEGGS_SNAP_MAX_SEGMENTS);
  if (n == 0) return 0;
  ZCHECK(segs != nullptr, "%s: NULL records", who);
  std::vector<int> order;
  order.reserve((size_t)n);
  size_t most = 0;
  const uintptr_t b0 = (uintptr_t)blob, b1 = b0 + blob_bytes;
  for (int i = 0; i < n; ++i) {
    const ZeggsSnapSeg& g = segs[i];
    ZCHECK(g.bytes % 4 == 0, "%s: record %d: %zu bytes is no multiple of 4", who, i, g.bytes);
    ZCHECK(g.dst_offset % 4 == 0, "%s: record %d: blob offset %zu is no multiple of 4", who, i, g.dst_offset);
    ZCHECK(g.dst_offset <= blob_bytes && g.bytes <= blob_bytes - g.dst_offset, "%s: record %d: blob offset %zu + %zu bytes is past the blob's %zu", who,
           i, g.dst_offset, g.bytes, blob_bytes);
    if (g.bytes == 0) continue;
    ZCHECK(g.src != nullptr && (uintptr_t)g.src % 4 == 0, "%s: record %d: NULL or misaligned pointer", who, i);
    const uintptr_t s0 = (uintptr_t)g.src, s1 = s0 + g.bytes;
    ZCHECK(blob == nullptr || s1 <= b0 || b1 <= s0, "%s: record %d: its state side lies inside the blob", who, i);
    order.push_back(i);
    if (g.bytes > most) most = g.bytes;
  }
  if (order.empty()) return 0;
  std::sort(order.begin(), order.end(), [segs](int a, int b) {
    return segs[a].dst_offset != segs[b].dst_offset ? segs[a].dst_offset < segs[b].dst_offset : a < b;
  });
  for (size_t k = 1; k < order.size(); ++k) {
    const ZeggsSnapSeg &p = segs[order[k - 1]], &q = segs[order[k]];
    ZCHECK(p.dst_offset + p.bytes <= q.dst_offset, "%s: the blob ranges of records %d and %d overlap", who, std::min(order[k - 1], order[k]),
           std::max(order[k - 1], order[k]));
  }
  ZCHECK(blob != nullptr && (uintptr_t)blob % 4 == 0, "%s: NULL or misaligned blob", who);
  ZCHECK(segs_dev != nullptr, "%s: the records must also be in device memory (segs_dev)", who);
  const dim3 grid((unsigned)snap_chunks(most), (unsigned)n);
  if (pack)
    hipLaunchKernelGGL(live_snapshot_k<true>, grid, dim3(SNAP_THREADS), 0, (hipStream_t)stream, segs_dev, (char*)const_cast<void*>(blob));
  else
    hipLaunchKernelGGL(live_snapshot_k<false>, grid, dim3(SNAP_THREADS), 0, (hipStream_t)stream, segs_dev, (char*)const_cast<void*>(blob));
  ZLAUNCH_CHECK(who);
  return 0;
}

}  // namespace

#include "live_host.h"      // the span writer, with the rest of the stages' host contract

extern "C" int zeggs_live_snapshot_version(void) { return 1; }

// (each family's own *_state_bytes refuses what the family refuses of the dims, with its own message)
extern "C" int zeggs_live_loudness_spans(const ZeggsLoudDims* d, int row, ZeggsSnapSpan* spans, int max_spans) {
  if (zeggs_live_loudness_state_bytes(d) == 0) return -1;
  size_t o[SNAP_MAX_SPANS], b[SNAP_MAX_SPANS];
  return lh_spans_out("live loudness spans", snap_loud_spans(d->fs, d->ring_blocks, d->rows, row, o, b, SNAP_MAX_SPANS), row, d->rows, max_spans, o, b, spans);
}

extern "C" int zeggs_resample_spans(const ZeggsResampleDims* d, int row, ZeggsSnapSpan* spans, int max_spans) {
  if (zeggs_resample_state_bytes(d) == 0) return -1;
  size_t o[SNAP_MAX_SPANS], b[SNAP_MAX_SPANS];
  return lh_spans_out("resample spans", snap_resample_spans(d->history, d->rows, row, o, b, SNAP_MAX_SPANS), row, d->rows, max_spans, o, b, spans);
}

extern "C" int zeggs_live_frames_spans(const ZeggsFramesDims* d, int row, ZeggsSnapSpan* spans, int max_spans) {
  if (zeggs_live_frames_state_bytes(d) == 0) return -1;
  size_t o[SNAP_MAX_SPANS], b[SNAP_MAX_SPANS];
  return lh_spans_out("frames spans", snap_frames_spans(d->J, d->rows, row, o, b, SNAP_MAX_SPANS), row, d->rows, max_spans, o, b, spans);
}

extern "C" int zeggs_live_retime_spans(const ZeggsFramesDims* d, int row, ZeggsSnapSpan* spans, int max_spans) {
  if (zeggs_live_retime_state_bytes(d) == 0) return -1;
  size_t o[SNAP_MAX_SPANS], b[SNAP_MAX_SPANS];
  return lh_spans_out("retime spans", snap_retime_spans(d->J, d->rows, row, o, b, SNAP_MAX_SPANS), row, d->rows, max_spans, o, b, spans);
}

extern "C" int zeggs_live_refilter_spans(const ZeggsFramesDims* d, int max_half, int row, ZeggsSnapSpan* spans, int max_spans) {
  if (zeggs_live_refilter_state_bytes(d, max_half) == 0) return -1;
  size_t o[SNAP_MAX_SPANS], b[SNAP_MAX_SPANS];
  return lh_spans_out("refilter spans", snap_refilter_spans(d->J, max_half, d->rows, row, o, b, SNAP_MAX_SPANS), row, d->rows, max_spans, o, b, spans);
}

extern "C" int zeggs_live_pack(const ZeggsSnapSeg* segs_host, const ZeggsSnapSeg* segs_dev, int n, void* blob_dev, size_t blob_bytes, void* stream) {
  return snap_launch("live pack", true, segs_host, segs_dev, n, blob_dev, blob_bytes, stream);
}

extern "C" int zeggs_live_unpack(const ZeggsSnapSeg* segs_host, const ZeggsSnapSeg* segs_dev, int n, const void* blob_dev, size_t blob_bytes,
                                 void* stream) {
  return snap_launch("live unpack", false, segs_host, segs_dev, n, blob_dev, blob_bytes, stream);
}
