/* C ABI of libzeggs_hip.so, fifth header: the output head of live serving
 * (zeggs_live_frames_version() >= 1; zeggs_version() stays what it is).
 *
 * The other four headers are closed sets (their tests pin their prototypes and structs); the entry points below have a header
 * of their own.  Same conventions as include/zeggs_hip_resample.h: the caller owns all memory, calls only enqueue on `stream`,
 * 0 on success / -1 with zeggs_last_error().  The Python mirror is zeggs/capi.py: FR_STRUCTS / FR_PROTOTYPES
 * (tests/test_live_frames_cpu.py compares the two).
 *
 * A live server hands out the decoder's raw rows: per frame a pose [root_vel 3 | root_vrt 3 | lpos 3J | ltxy 6J | lvel 3J |
 * lvrt 3J], a root position [3] and a root rotation [4] (w first).  zeggs_live_frames turns the new frames of every row
 * (stream) that advanced into what a renderer or a BVH recorder takes, ONE launch for all of them (csrc/live_frames.hip; the
 * definition is DESIGN.md 3.7, the layouts csrc/frames_math.h).  Per frame, in float64:
 *   root    with `rebase`: pos = start_rot ref_rot^-1 (x - ref_pos) + start_pos, rot = start_rot ref_rot^-1 q, as
 *           zeggs_pose_to_bvh_table re-bases; ref is the stream's frame 0, given when the row opens.  Without: as it is.
 *   LOCAL   float32 [7 + 7J]: root_pos[3] | root_rot[4] | lrot[J][4] | lpos[J][3]; lrot[j] the quaternion of the two-axis
 *           encoding ltxy[j]; the root is NOT folded into joint 0.
 *   WORLD   float32 [7J]: gpos[J][3] | grot[J][4], forward kinematics over `parents` with the placed root folded into joint 0.
 *   BVH     float64 [3 + 3J]: the motion-block row of zeggs_pose_to_bvh_table: root position, then the Euler degrees (channel
 *           order `order`) of joint seq[0], seq[1], ...
 * Every emitted root_rot, lrot[j] and grot[j] is negated when its dot product with the value emitted for the previous frame of
 * that stream is below 0; the previous values are kept in the row's state as the emitted float32 values, and the very first
 * frame of a stream is emitted with w >= 0.  The frames of a stream are so a pure function of its frame sequence: the same
 * bits however the sequence is cut into calls and whichever rows share a call. */
#ifndef ZEGGS_HIP_FRAMES_H
#define ZEGGS_HIP_FRAMES_H
#include "zeggs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZEGGS_FRAMES_LOCAL 1
#define ZEGGS_FRAMES_WORLD 2
#define ZEGGS_FRAMES_BVH 4

typedef struct {
  int rows;        /* rows of the state (<= ZEGGS_LIVE_MAX_ROWS) */
  int J;           /* joints */
  int max_frames;  /* frames of one record at most */
  int what;        /* ZEGGS_FRAMES_LOCAL | _WORLD | _BVH */
  int order;       /* channel order of the BVH rotations, packed as ZeggsBvhDims.order; "zyx" (0) and "xzy" only */
} ZeggsFramesDims;

/* one row's share of a call: `count` new frames, frame f of them at pose + f pose_ld, rpos + f rpos_ld, rrot + f rrot_ld
 * (device float32; leading dimensions in floats).  Frame f goes to local + f (7 + 7J), world + f 7J (device float32) and
 * bvh + f (3 + 3J) (device float64); a destination whose bit is off in `what` is not looked at and may be NULL. */
typedef struct {
  const float* pose;
  const float* rpos;
  const float* rrot;
  float* local;
  float* world;
  double* bvh;
  long pose_ld, rpos_ld, rrot_ld;
  int row, count;
} ZeggsFramesRow;

int zeggs_live_frames_version(void);
/* bytes of the state: the skeleton tables, then per row the placement (ref / start, float64), two flags and the float32
 * quaternions emitted for the row's last frame (4 + 8J floats).  0 with zeggs_last_error() for dims the entry points refuse. */
size_t zeggs_live_frames_state_bytes(const ZeggsFramesDims*);
/* writes the skeleton tables into the state: parents_host[J] (parents[0] == -1, 0 <= parents[j] < j: refused otherwise, the
 * joint named) and seq_host[J], the joint order of the BVH file (a permutation: refused otherwise).  Once per state, never on
 * the tick path: the one entry that waits for `stream` (its upload).  The rows' own state is not touched. */
int zeggs_live_frames_prepare(const ZeggsFramesDims*, const int* parents_host, const int* seq_host, void* state, size_t state_bytes,
                              void* stream);
/* row `row` opens: its next frame is the first of a stream.  ref_pos[3] / ref_rot[4]: the stream's frame 0 (host, float32 as
 * the frames are); start_pos[3] / start_rot[4]: where the character stands (host, float64); rebase == 0: the root is taken as it
 * is and the four may be NULL. */
int zeggs_live_frames_reset(const ZeggsFramesDims*, void* state, size_t state_bytes, int row, const float* ref_pos, const float* ref_rot,
                            const double* start_pos, const double* start_rot, int rebase, void* stream);
/* ONE launch for all R records (grid = R, one workgroup per record).  rows_host: the records in HOST memory for the checks, all
 * ahead of the launch and naming the record they refuse: row in 0 .. d->rows - 1 and not twice in a call, 0 <= count <=
 * d->max_frames, and where count > 0 non-NULL 4-byte aligned sources with leading dimensions that hold what is read
 * (6 + 9J, 3, 4 floats) and a non-NULL aligned destination (4 bytes, bvh 8) for every bit of d->what.  A J or max_frames whose
 * LDS need exceeds what the kernel may have is refused with the dims.  rows_dev: the same records in DEVICE memory; NULL is
 * allowed for R == 1 (the record then travels in the kernel arguments).  Rows that are not in the call keep their state. */
int zeggs_live_frames(const ZeggsFramesDims*, const ZeggsFramesRow* rows_host, const ZeggsFramesRow* rows_dev, int R, void* state,
                      size_t state_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
