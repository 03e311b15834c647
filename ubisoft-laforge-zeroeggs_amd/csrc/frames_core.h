// The per-frame arithmetic of the output head of live serving, stated once for its two kernels: live_frames_k (live_frames.hip),
// whose frames are the decoder's, and live_retime_k (live_retime.hip), whose frames sit between them.  fr_pass() is passes 0 - 4 of
// one pass of n staged frames (the head of live_frames.hip says what each does); the two kernels differ only in the LOAD of
// passes 0 and 1 -- where the placed root and a joint's local quaternion and position of a staged frame come from:
//   load.root(t, rr, rp)      the placed root of staged frame t
//   load.joint(t, j, q, p)    joint j's local quaternion and position of staged frame t
// Device code: include common.h, anim_math.h and frames_math.h first.
#pragma once

struct FrPlace {      // what a row's state starts with
  double ref_pos[3], ref_rot[4], start_pos[3], start_rot[4];
  int rebase, started;
};
static_assert(sizeof(FrPlace) == 14 * 8 + 2 * 4, "fr_row_bytes");

__device__ __forceinline__ D3 ldf3(const float* p) { return D3{(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ void stf3(float* p, D3 v) { p[0] = (float)v.x; p[1] = (float)v.y; p[2] = (float)v.z; }

// the root of a decoder frame as it is handed out: re-based on the stream's frame 0 (as pose_to_bvh_table_k) with a placement
__device__ __forceinline__ void fr_place_root(const FrPlace* pl, bool rebase, const float* rpos, const float* rrot, DQ& rr, D3& rp) {
  rr = DQ{(double)rrot[0], (double)rrot[1], (double)rrot[2], (double)rrot[3]};
  rp = ldf3(rpos);
  if (rebase) {
    const DQ r0 = dq_inv(ldq(pl->ref_rot)), sr = ldq(pl->start_rot);
    rp = dq_mul_vec(sr, dq_mul_vec(r0, rp - ld3(pl->ref_pos))) + ld3(pl->start_pos);
    rr = dq_mul(sr, dq_mul(r0, rr));
  }
}

// One pass: staged frames t = 0 .. n - 1 are frames f0 + t of the record, whose frame f goes to local + f LL, world + f WL and
// bvh + f BL.  `first`: the index in the record of the stream's very first frame (emitted with w >= 0), -1 when it is not here.
// lq / lp: the LDS of the pass, per frame J + 1 quaternions and J + 1 positions, slot J = the placed root.  prev: the row's
// float32 quaternions last emitted, read by the thread that owns the joint at the start of the pass and written at its end.
template <class Load>
__device__ __forceinline__ void fr_pass(const Load& load, int J, int order, int what, const int* parents, const int* place, float* prev,
                                        double* lq, double* lp, long f0, int n, long first, float* local_out, float* world_out,
                                        double* bvh_out) {
  const int tid = threadIdx.x;
  const bool local = (what & FR_LOCAL) != 0, world = (what & FR_WORLD) != 0, bvh = (what & FR_BVH) != 0;
  const int LL = fr_local_floats(J), WL = fr_world_floats(J), BL = fr_bvh_doubles(J);
  // ---- 0. the placed root
  for (int t = tid; t < n; t += FR_THREADS) {
    const long f = f0 + t;
    DQ rr;
    D3 rp;
    load.root(t, rr, rp);
    stq(lq + ((size_t)t * (J + 1) + J) * 4, rr);
    st3(lp + ((size_t)t * (J + 1) + J) * 3, rp);
    if (local) stf3(local_out + f * LL + fr_local_root_pos(), rp);
  }
  __syncthreads();
  // ---- 1. local quaternions and positions; LOCAL's lpos; the BVH row
  for (int i = tid; i < n * J; i += FR_THREADS) {
    const int t = i / J, j = i - t * J;
    const long f = f0 + t;
    DQ q;
    D3 p;
    load.joint(t, j, q, p);
    const size_t s = (size_t)t * (J + 1) + j;
    stq(lq + s * 4, q);
    st3(lp + s * 3, p);
    if (local) stf3(local_out + f * LL + fr_local_lpos(J, j), p);      // (a decoder frame's float32 comes back as it was)
    if (bvh) {
      double* b = bvh_out + f * BL;
      DQ e = q;
      if (j == 0) {      // the placed root folded into joint 0
        const DQ rr = ldq(lq + ((size_t)t * (J + 1) + J) * 4);
        st3(b, dq_mul_vec(rr, p) + ld3(lp + ((size_t)t * (J + 1) + J) * 3));
        e = dq_mul(rr, q);
      }
      const int k = place[j];      // (a state that was never prepared must not send a store astray)
      if ((unsigned)k < (unsigned)J) dq_to_euler_deg(e, b + fr_bvh_euler(k), order);
    }
  }
  __syncthreads();
  // ---- 2. LOCAL's quaternions, frame by frame: thread j owns joint j, j == J is the root's rotation
  if (local) {
    for (int j = tid; j <= J; j += FR_THREADS) {
      float* sp = prev + (j == J ? fr_prev_root() : fr_prev_lrot(j));
      float pv[4] = {sp[0], sp[1], sp[2], sp[3]};
      for (int t = 0; t < n; ++t) {
        const DQ q = ldq(lq + ((size_t)t * (J + 1) + j) * 4);
        fr_emit(f0 + t != first, q.w, q.x, q.y, q.z, pv, local_out + (long)(f0 + t) * LL + (j == J ? fr_local_root_rot() : fr_local_lrot(j)));
      }
      sp[0] = pv[0]; sp[1] = pv[1]; sp[2] = pv[2]; sp[3] = pv[3];
    }
  }
  if (world) {
    __syncthreads();      // (3. overwrites what 2. reads)
    // ---- 3. forward kinematics in place, joints in index order
    for (int t = tid; t < n; t += FR_THREADS) {
      double* q = lq + (size_t)t * (J + 1) * 4;
      double* p = lp + (size_t)t * (J + 1) * 3;
      const DQ rr = ldq(q + J * 4);
      st3(p, dq_mul_vec(rr, ld3(p)) + ld3(p + J * 3));
      stq(q, dq_mul(rr, ldq(q)));
      for (int j = 1; j < J; ++j) {
        const int a = (unsigned)parents[j] < (unsigned)j ? parents[j] : 0;
        const DQ pq = ldq(q + a * 4);
        st3(p + j * 3, dq_mul_vec(pq, ld3(p + j * 3)) + ld3(p + a * 3));
        stq(q + j * 4, dq_mul(pq, ldq(q + j * 4)));
      }
    }
    __syncthreads();
    // ---- 4. WORLD, frame by frame
    for (int j = tid; j < J; j += FR_THREADS) {
      float* sp = prev + fr_prev_grot(J, j);
      float pv[4] = {sp[0], sp[1], sp[2], sp[3]};
      for (int t = 0; t < n; ++t) {
        const size_t s = (size_t)t * (J + 1) + j;
        float* o = world_out + (long)(f0 + t) * WL;
        stf3(o + fr_world_gpos(j), ld3(lp + s * 3));
        const DQ q = ldq(lq + s * 4);
        fr_emit(f0 + t != first, q.w, q.x, q.y, q.z, pv, o + fr_world_grot(J, j));
      }
      sp[0] = pv[0]; sp[1] = pv[1]; sp[2] = pv[2]; sp[3] = pv[3];
    }
  }
  __syncthreads();      // (the next pass rewrites the LDS)
}
