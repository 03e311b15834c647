/* C ABI of libzeggs_hip.so, ninth header: a gaze target per live row that can move while speech goes on
 * (zeggs_live_gaze_version() >= 1; zeggs_version() >= 109 and the versions of the other headers stay what they are).
 *
 * The other eight headers are closed sets (their tests pin their prototypes and structs); the entry points below have a header
 * of their own.  Same conventions as include/zeggs_hip_loudness.h: the caller owns all memory, calls only enqueue on `stream`
 * (zeggs_live_gaze_read also waits for it), 0 on success / -1 with zeggs_last_error().  The Python mirror is zeggs/capi.py:
 * GZ_STRUCTS / GZ_PROTOTYPES (tests/test_live_gaze_cpu.py compares the two).
 *
 * Every row (stream) of a gaze server keeps a SCHEDULE on the device, ZEGGS_GAZE_ROW_BYTES bytes: start, end and pivot as
 * float32 triples in the model's world (the space of the root position), the frame k it holds from, the frames `fade` it takes,
 * a path and an ease.  Frame f looks at P(w(f)) (csrc/gaze_math.h, the one statement for host and device):
 *   - w(f) = clip((f - k + 1) / (fade + 1), 0, 1); with ZEGGS_GAZE_SMOOTH the weight becomes w^2 (3 - 2 w);
 *   - ZEGGS_GAZE_LINE: P(w) = (1 - w) start + w end;
 *   - ZEGGS_GAZE_ARC: with a = start - pivot, b = end - pivot, u = a / |a|, v = b / |b|, s = |u x v|, theta = atan2(s, u.v):
 *     P(w) = pivot + ((1 - w) |a| + w |b|) (sin((1 - w) theta) u + sin(w theta) v) / s; the line when |a| or |b| < 1e-6 or
 *     s < 1e-6;
 * in float64 from the float32 state, rounded to float32 once at the store.  zeggs_live_gaze_set replaces a row's schedule: the
 * new start is the old schedule at frame k - 1 (an unfinished fade goes on from where it stands), and a target or pivot given
 * in the character's root frame (ZEGGS_GAZE_ROOT) becomes rpos + rrot (x) p with the row's root state as the caller's tensors
 * hold it at the call (the quaternion as stored, rotated as csrc/quat_math.h rotates a vector) -- once: from then on the
 * schedule is a world-space schedule.  zeggs_live_condition writes, for the frames of one decoder call, the gaze rows AND the
 * style rows lerp(sty_old, sty_new, w_style(f)) of every participating row, in ONE launch. */
#ifndef ZEGGS_HIP_GAZE_H
#define ZEGGS_HIP_GAZE_H
#include "zeggs_hip_snapshot.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZEGGS_GAZE_ROW_BYTES 64
#define ZEGGS_GAZE_WORLD 0
#define ZEGGS_GAZE_ROOT 1
#define ZEGGS_GAZE_LINE 0
#define ZEGGS_GAZE_ARC 1
#define ZEGGS_GAZE_LINEAR 0
#define ZEGGS_GAZE_SMOOTH 1

typedef struct {
  int rows, ST;             /* rows of the state (<= ZEGGS_LIVE_MAX_ROWS); floats of a style row (>= 1) */
} ZeggsGazeDims;

/* one row's new schedule: from frame k on (>= 1), over `fade` frames (>= 0) towards `target`; `pivot` counts where has_pivot
 * != 0 (an arc in world space needs one; in root space the default is the root position used for the conversion) */
typedef struct {
  float target[3], pivot[3];
  long k, fade;
  int row, space, path, ease, has_pivot;
} ZeggsGazeSet;

/* one row's share of a decoder call: frames k0 .. k0 + n - 1 go to slice `out_row` of the two output tensors; the style rows
 * carry the weight of the style fade (k_style, fade_style) */
typedef struct {
  long k0, k_style, fade_style;
  int row, out_row, n;
} ZeggsGazeCond;

/* what zeggs_live_gaze_read writes, as doubles */
#define ZEGGS_GAZE_READ_TARGET 0    /* [3]: what frame `frame` looks at */
#define ZEGGS_GAZE_READ_K 3
#define ZEGGS_GAZE_READ_FADE 4
#define ZEGGS_GAZE_READ_START 5     /* [3] */
#define ZEGGS_GAZE_READ_END 8       /* [3] */
#define ZEGGS_GAZE_READ_PIVOT 11    /* [3] */
#define ZEGGS_GAZE_READ_PATH 14
#define ZEGGS_GAZE_READ_EASE 15
#define ZEGGS_GAZE_READ_WORDS 16

int zeggs_live_gaze_version(void);
/* bytes of the state of d->rows rows: ZEGGS_GAZE_ROW_BYTES each, one behind another */
size_t zeggs_live_gaze_state_bytes(const ZeggsGazeDims*);
/* row `row` looks at gaze0[3] (DEVICE memory) from now on: start = end = gaze0, fade 0, the line */
int zeggs_live_gaze_reset(const ZeggsGazeDims*, void* state, size_t state_bytes, int row, const float* gaze0, void* stream);
/* ONE launch for all R records (grid = R).  recs_host: the records in HOST memory for the checks, all ahead of the launch and
 * naming the record they refuse: row in 0 .. d->rows - 1 and not twice in a call, k >= 1, fade >= 0, finite target (and pivot
 * where it counts), a known space, path and ease, an arc in world space without a pivot.  recs_dev: the same records in DEVICE
 * memory; NULL is allowed for R == 1 (the record then travels in the kernel arguments).  rpos / rrot: the rows' root position
 * [rows][3] and rotation [rows][4] (w first) after frame k - 1, DEVICE memory, row strides in floats. */
int zeggs_live_gaze_set(const ZeggsGazeDims*, const ZeggsGazeSet* recs_host, const ZeggsGazeSet* recs_dev, int R, const float* rpos,
                        long rpos_ld, const float* rrot, long rrot_ld, void* state, size_t state_bytes, void* stream);
/* ONE launch per decoder call (grid = R).  Per record: gaze_out[out_row][i][0..3) <- the row's schedule at frame k0 + i and
 * style_out[out_row][i][0..ST) <- lerp(sty_old[row], sty_new[row], w(k0 + i; k_style, fade_style)), i = 0 .. n - 1.  The
 * output tensors hold out_rows slices of `stride` frames each (float32, DEVICE memory); slices no record names are not
 * touched.  sty_old / sty_new: [rows][ST].  recs_host / recs_dev as above; refused ahead of the launch, naming the record: a
 * row or an out_row out of range or twice, n outside 1 .. stride, negative k0 or fade_style. */
int zeggs_live_condition(const ZeggsGazeDims*, const ZeggsGazeCond* recs_host, const ZeggsGazeCond* recs_dev, int R, const void* state,
                         size_t state_bytes, const float* sty_old, const float* sty_new, float* gaze_out, float* style_out, int out_rows,
                         long stride, void* stream);
/* out_host[ZEGGS_GAZE_READ_WORDS] <- the row's schedule after everything enqueued on `stream` so far (waits for the stream) and
 * what frame `frame` looks at: monitoring, not for the tick path */
int zeggs_live_gaze_read(const ZeggsGazeDims*, const void* state, size_t state_bytes, int row, long frame, double* out_host, void* stream);
/* the span report of the family (include/zeggs_hip_snapshot.h): one span, the row's schedule */
int zeggs_live_gaze_spans(const ZeggsGazeDims*, int row, ZeggsSnapSpan* spans, int max_spans);

#ifdef __cplusplus
}
#endif
#endif
