// The LOAD of the re-timing output head of live serving, stated once for its two kernels: live_retime_k (live_retime.hip) and the
// rows of live_refilter_k (live_refilter.hip) that run without the filter.  Staged frame t of a pass is output frame m0 + t of the
// stream, at input position k + num / L (retime_math.h):
//   num == 0  the staged frame is input frame k, loaded as live_frames_k loads it (no interpolation: the plain head's bits);
//   num != 0  both ends k and k + 1 are loaded that way -- the root placed, the joints' quaternions from their two-axis encoding
//             -- and the staged frame is a + t (b - a) for positions and the shortest arc for rotations, t = num / L.
// Device code: include common.h, anim_math.h, frames_math.h, retime_math.h and frames_core.h first.
#pragma once

__device__ __forceinline__ DQ rt_slerp(DQ a, DQ b, double t) {
  double d = a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z;
  if (d < 0.0) {
    b = DQ{-b.w, -b.x, -b.y, -b.z};
    d = -d;
  }
  double wa, wb;
  rt_slerp_weights(d, t, &wa, &wb);
  const DQ q = DQ{wa * a.w + wb * b.w, wa * a.x + wb * b.x, wa * a.y + wb * b.y, wa * a.z + wb * b.z};
  const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  return DQ{q.w / n, q.x / n, q.y / n, q.z / n};
}

// the LOAD of passes 0 and 1: staged frame t is output frame m0 + t of the stream
struct RtLoad {
  ZeggsRetimeRow rec;
  const FrPlace* pl;
  const float* raw;      // the row's last input frame of an earlier call (input frame n_in - 1)
  long m0;
  int J;
  bool rebase;
  // input frame i of the call, i = -1: the kept one (an index the counting rule cannot give is brought back into the call)
  __device__ __forceinline__ long clamp(long i, long lo) const { return i < lo ? lo : (i > rec.count - 1 ? rec.count - 1 : i); }
  __device__ __forceinline__ void where(int t, long& i, long& num) const {
    long k;
    rt_position(m0 + t, rec.L, rec.M, &k, &num);
    i = clamp(k - rec.n_in, rec.n_in > 0 ? -1 : 0);
  }
  __device__ __forceinline__ void root_of(long i, DQ& rr, D3& rp) const {
    const float* p = i < 0 ? raw + rt_raw_rpos() : rec.rpos + i * rec.rpos_ld;
    const float* r = i < 0 ? raw + rt_raw_rrot() : rec.rrot + i * rec.rrot_ld;
    fr_place_root(pl, rebase, p, r, rr, rp);
  }
  __device__ __forceinline__ void joint_of(long i, int j, DQ& q, D3& p) const {
    const float* row = rec.pose + (i < 0 ? 0 : i) * rec.pose_ld;
    const float* x = i < 0 ? raw + rt_raw_ltxy(J, j) : row + fr_pose_ltxy(J, j);
    q = dq_from_xy(ldf3(x), ldf3(x + 3));
    p = ldf3(i < 0 ? raw + rt_raw_lpos(j) : row + fr_pose_lpos(j));
  }
  __device__ __forceinline__ void root(int t, DQ& rr, D3& rp) const {
    long i, num;
    where(t, i, num);
    root_of(i, rr, rp);
    if (num != 0) {
      DQ rb;
      D3 pb;
      root_of(clamp(i + 1, 0), rb, pb);
      const double u = (double)num / (double)rec.L;
      rp = rp + u * (pb - rp);
      rr = rt_slerp(rr, rb, u);
    }
  }
  __device__ __forceinline__ void joint(int t, int j, DQ& q, D3& p) const {
    long i, num;
    where(t, i, num);
    joint_of(i, j, q, p);
    if (num != 0) {
      DQ qb;
      D3 pb;
      joint_of(clamp(i + 1, 0), j, qb, pb);
      const double u = (double)num / (double)rec.L;
      p = p + u * (pb - p);
      q = rt_slerp(q, qb, u);
    }
  }
};
