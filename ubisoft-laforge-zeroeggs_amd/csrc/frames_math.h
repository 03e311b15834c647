// The layout and index rules of the output head of live serving (live_frames.hip), stated once: how many floats a frame takes
// in each of the three outputs and where its fields sit, how a row's state is laid out, how many frames the kernel stages per
// pass and what that costs in LDS, which skeleton tables it takes, and the sign rule that keeps a stream's quaternions
// continuous from frame to frame and from call to call.  Plain C++ behind a qualifier macro (no HIP include), so the same text
// runs in the kernel, in the host side of live_frames.hip and in tests/host/frames_math_check.cpp.  The definition is DESIGN.md 3.7.
#pragma once

#ifndef ZF_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZF_HD __host__ __device__ __forceinline__
#else
#define ZF_HD inline
#endif
#endif

#define FR_LOCAL 1            // ZEGGS_FRAMES_LOCAL / _WORLD / _BVH
#define FR_WORLD 2
#define FR_BVH 4
#define FR_THREADS 256        // threads of a workgroup (one workgroup per record)
#define FR_LDS_BYTES 65536    // LDS a workgroup may have
#define FR_MAX_JOINTS 1024
#define FR_MAX_FRAMES 4096    // frames of one record

// ---- the three outputs, per frame
// LOCAL (float32): root_pos[3] | root_rot[4] | lrot[J][4] | lpos[J][3]
ZF_HD int fr_local_floats(int J) { return 7 + 7 * J; }
ZF_HD int fr_local_root_pos() { return 0; }
ZF_HD int fr_local_root_rot() { return 3; }
ZF_HD int fr_local_lrot(int j) { return 7 + 4 * j; }
ZF_HD int fr_local_lpos(int J, int j) { return 7 + 4 * J + 3 * j; }
// WORLD (float32): gpos[J][3] | grot[J][4]
ZF_HD int fr_world_floats(int J) { return 7 * J; }
ZF_HD int fr_world_gpos(int j) { return 3 * j; }
ZF_HD int fr_world_grot(int J, int j) { return 3 * J + 4 * j; }
// BVH (float64): root position[3] | Euler degrees of joint seq[0], seq[1], ... [J][3]
ZF_HD int fr_bvh_doubles(int J) { return 3 + 3 * J; }
ZF_HD int fr_bvh_euler(int k) { return 3 + 3 * k; }
// a pose row of the decoder: root_vel 3 | root_vrt 3 | lpos 3J | ltxy 6J | lvel 3J | lvrt 3J -- what the kernel reads of it
ZF_HD int fr_pose_lpos(int j) { return 6 + 3 * j; }
ZF_HD int fr_pose_ltxy(int J, int j) { return 6 + 3 * J + 6 * j; }
ZF_HD int fr_pose_floats_read(int J) { return 6 + 9 * J; }

// ---- the state: [parents int[J] | seq int[J] | place int[J] (place[seq[k]] = k), padded to 8 bytes] then per row
//   double ref_pos[3], ref_rot[4], start_pos[3], start_rot[4] | int rebase, started | float prev root_rot[4], lrot[J][4], grot[J][4]
ZF_HD long fr_tables_bytes(int J) { return ((long)3 * J * 4 + 7) / 8 * 8; }
ZF_HD int fr_row_prev_floats(int J) { return 4 + 8 * J; }
ZF_HD long fr_row_bytes(int J) { return 14 * 8 + 2 * 4 + ((long)fr_row_prev_floats(J) * 4 + 7) / 8 * 8; }
ZF_HD long fr_state_bytes(int rows, int J) { return fr_tables_bytes(J) + (long)rows * fr_row_bytes(J); }
ZF_HD long fr_row_offset(int J, int row) { return fr_tables_bytes(J) + (long)row * fr_row_bytes(J); }
ZF_HD int fr_prev_root() { return 0; }
ZF_HD int fr_prev_lrot(int j) { return 4 + 4 * j; }
ZF_HD int fr_prev_grot(int J, int j) { return 4 + 4 * J + 4 * j; }

// ---- LDS: a pass stages per frame the placed root and every joint as a quaternion and a position in float64 (local, then
// overwritten by the global ones): 7 doubles for each of J + 1 slots.  Frames of a pass: as many as fit, at most max_frames.
ZF_HD long fr_frame_lds_bytes(int J) { return (long)(J + 1) * 7 * 8; }
ZF_HD int fr_pass_frames(int J, int max_frames) {
  const long fit = FR_LDS_BYTES / fr_frame_lds_bytes(J);
  return (int)(fit < max_frames ? fit : max_frames);
}
ZF_HD long fr_lds_bytes(int J, int max_frames) { return fr_pass_frames(J, max_frames) * fr_frame_lds_bytes(J); }
// what the entry points take: 0, or the reason (1: J, 2: max_frames, 3: not one frame of J joints fits the LDS)
ZF_HD int fr_shape_refused(int J, int max_frames) {
  if (J < 1 || J > FR_MAX_JOINTS) return 1;
  if (max_frames < 1 || max_frames > FR_MAX_FRAMES) return 2;
  return fr_pass_frames(J, max_frames) < 1 ? 3 : 0;
}

// ---- the skeleton tables: -1, or the first joint that is refused
// parents: parents[0] == -1, 0 <= parents[j] < j (a parent comes before its children: FK walks the joints in index order)
ZF_HD int fr_bad_parent(const int* parents, int J) {
  if (parents[0] != -1) return 0;
  for (int j = 1; j < J; ++j)
    if (parents[j] < 0 || parents[j] >= j) return j;
  return -1;
}
// seq: a permutation of 0 .. J - 1 (the joint order of the BVH file); place[seq[k]] = k is written when it is one
ZF_HD int fr_bad_seq(const int* seq, int J, int* place) {
  for (int j = 0; j < J; ++j) place[j] = -1;
  for (int k = 0; k < J; ++k) {
    if (seq[k] < 0 || seq[k] >= J || place[seq[k]] != -1) return k;
    place[seq[k]] = k;
  }
  return -1;
}

// ---- the sign rule (quat.unroll carried across calls): q is negated when its dot product with the value EMITTED for the stream's
// previous frame (float32, from the row's state or from this call) is below 0; the first frame of a stream is emitted with w >= 0
ZF_HD bool fr_flip(bool started, double w, double x, double y, double z, const float* prev) {
  if (!started) return w < 0.0;
  return w * (double)prev[0] + x * (double)prev[1] + y * (double)prev[2] + z * (double)prev[3] < 0.0;
}
// emits q (or -q) as float32 into out[4] and into prev[4]
ZF_HD void fr_emit(bool started, double w, double x, double y, double z, float* prev, float* out) {
  const double s = fr_flip(started, w, x, y, z, prev) ? -1.0 : 1.0;
  prev[0] = (float)(s * w); prev[1] = (float)(s * x); prev[2] = (float)(s * y); prev[3] = (float)(s * z);
  out[0] = prev[0]; out[1] = prev[1]; out[2] = prev[2]; out[3] = prev[3];
}
