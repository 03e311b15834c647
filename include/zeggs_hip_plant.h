/* C ABI of libzeggs_hip.so, eleventh header: feet that stay planted -- contact lock and leg IK for live rows
 * (zeggs_live_plant_version() >= 1; zeggs_version() >= 109 and the versions of the other headers stay what they are).
 *
 * The other ten headers are closed sets (their tests pin their prototypes and structs); the entry points below have a header
 * of their own.  Same conventions as include/zeggs_hip_frames.h: the caller owns all memory, calls only enqueue on `stream`
 * (zeggs_live_plant_prepare also waits for it), 0 on success / -1 with zeggs_last_error().  The Python mirror is zeggs/capi.py:
 * PL_STRUCTS / PL_PROTOTYPES (tests/test_live_plant_cpu.py compares the two).
 *
 * The planting stage stands between the decoder's raw rows and the output head: it reads a pose row [root_vel 3 | root_vrt 3 |
 * lpos 3J | ltxy 6J | lvel 3J | lvrt 3J] with its root position [3] and root rotation [4] (w first) and writes a corrected copy
 * of the row, which the head then reads in place of the decoder's (ZeggsFramesRow.pose is only a pointer).  A CHAIN is three
 * joints (u, m, e) -- upper leg, lower leg, foot; parents[m] == u, parents[e] == m; at most ZEGGS_PLANT_MAX_CHAINS, no joint in
 * two of them.  Per model frame and chain, in float64 (csrc/plant_math.h, the one statement for host and device):
 *   - FK over the ancestors of e from the RAW row (the head's dq_from_xy, the root folded into joint 0, no re-basing; the root's
 *     rotation and every local rotation brought to unit length first) gives the unconstrained world points H (u), K (m), A (e);
 *   - s = |A - a_prev| / dt (0 on a stream's first frame), y = A.y - ground; e_off = o0 g(k / release), g(x) = 1 - x^2 (3 - 2 x)
 *     below 1 and 0 from 1 on (0 with release == 0);
 *   - at most one transition: HELD and (s > v_off or y > h_off or |A - L| > slack) -> FREE with o0 = L - A, k = 0 and e_off
 *     taken again; else FREE and s <= v_on and y <= h_on -> HELD with L = A + e_off;
 *   - the target T = L when HELD, else A + e_off and k = min(k + 1, release); a T farther from H than stretch (|K - H| + |A - K|)
 *     is pulled onto that sphere along T - H;
 *   - a T that equals A leaves the chain's joints as they are; any other goes through the analytic two-bone solve, which turns u
 *     (bend, then swing) and m (bend) so that the ankle is T and gives e the local rotation that keeps its world rotation.  The
 *     two columns of the three new local rotations go back as ltxy, rounded to float32 once; every other float of the row
 *     leaves as the same bits;
 *   - a_prev = A; the frame's contact flag is 1 when the chain is HELD.
 * A row's frames are so a pure function of its frame sequence: the same bits however the sequence is cut into calls and
 * whichever rows share a call. */
#ifndef ZEGGS_HIP_PLANT_H
#define ZEGGS_HIP_PLANT_H
#include "zeggs_hip_snapshot.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZEGGS_PLANT_MAX_CHAINS 4
#define ZEGGS_PLANT_CHAIN_BYTES 88 /* the state of one chain of one row */

typedef struct {
  int rows;         /* rows of the state (<= ZEGGS_LIVE_MAX_ROWS) */
  int J;            /* joints (>= 3) */
  int max_frames;   /* frames of one record at most */
  int chains;       /* chains (1 .. ZEGGS_PLANT_MAX_CHAINS) */
  int release;      /* frames the correction takes to fade out after a release (>= 0) */
  int pad;
  double dt;        /* the frame time the speed is taken over (> 0) */
  double v_on, v_off; /* contact begins at a speed <= v_on and ends above v_off (0 <= v_on <= v_off) */
  double h_on, h_off; /* ... and at a height above `ground` <= h_on, ends above h_off (h_on <= h_off) */
  double ground;    /* the height of the ground plane */
  double slack;     /* a held ankle whose unconstrained position is farther than this from the held point is released (>= 0) */
  double stretch;   /* the share of |K - H| + |A - K| the ankle may be from H (0 < stretch <= 1) */
} ZeggsPlantDims;

/* one row's share of a call: `count` new frames, frame f of them at pose + f pose_ld, rpos + f rpos_ld, rrot + f rrot_ld (device
 * float32; leading dimensions in floats).  Frame f's corrected row (6 + 15J floats) goes to out + f out_ld, its contact flags
 * (one byte a chain, 0 or 1) to contacts + f chains.  `out` is memory of its own: not the source rows. */
typedef struct {
  const float* pose;
  const float* rpos;
  const float* rrot;
  float* out;
  unsigned char* contacts;
  long pose_ld, rpos_ld, rrot_ld, out_ld;
  int row, count;
} ZeggsPlantRow;

int zeggs_live_plant_version(void);
/* bytes of the state: the skeleton's parents and the chain table, then per row ZEGGS_PLANT_MAX_CHAINS chain states of
 * ZEGGS_PLANT_CHAIN_BYTES.  0 with zeggs_last_error() for dims the entry points refuse. */
size_t zeggs_live_plant_state_bytes(const ZeggsPlantDims*);
/* writes the tables into the state: parents_host[J] (parents[0] == -1, 0 <= parents[j] < j: refused otherwise, the joint named)
 * and chains_host[d->chains][3], the joints (u, m, e) of every chain (refused, the chain named: an index out of range, parents[m]
 * != u or parents[e] != m, a joint that an earlier chain has).  Once per state, never on the tick path: the one entry that
 * waits for `stream` (its upload).  The rows' own state is not touched. */
int zeggs_live_plant_prepare(const ZeggsPlantDims*, const int* parents_host, const int* chains_host, void* state, size_t state_bytes,
                             void* stream);
/* row `row` opens: every chain FREE with no offset, its next frame the first of a stream */
int zeggs_live_plant_reset(const ZeggsPlantDims*, void* state, size_t state_bytes, int row, void* stream);
/* the span report of the family (include/zeggs_hip_snapshot.h): one span, the row's chain states */
int zeggs_live_plant_spans(const ZeggsPlantDims*, int row, ZeggsSnapSpan* spans, int max_spans);
/* ONE launch for all R records (grid = R, one workgroup per record).  recs_host: the records in HOST memory for the checks, all
 * ahead of the launch and naming the record they refuse: row in 0 .. d->rows - 1 and not twice in a call, 0 <= count <=
 * d->max_frames, and where count > 0 non-NULL 4-byte aligned sources with leading dimensions that hold what is read (6 + 15J, 3,
 * 4 floats), a non-NULL 4-byte aligned `out` that is not `pose` with out_ld >= 6 + 15J, and non-NULL `contacts`.  recs_dev: the
 * same records in DEVICE memory; NULL is allowed for R == 1 (the record then travels in the kernel arguments).  Rows that are
 * not in the call keep their state. */
int zeggs_live_plant(const ZeggsPlantDims*, const ZeggsPlantRow* recs_host, const ZeggsPlantRow* recs_dev, int R, void* state,
                     size_t state_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
