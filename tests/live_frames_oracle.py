"""Float64 oracle of the output head of live serving (include/zeggs_hip_frames.h), composed from oracle/anim.py,
and the inputs the tests of the head share.  TEST INFRASTRUCTURE ONLY: tests/test_live_frames_cpu.py checks it against itself,
tests/test_gpu_live_frames.py compares the kernel and the server with it.

frames(): the WHOLE frame sequence of a stream (root positions and rotations, local positions and two-axis rotations, float32 as
the decoder hands them out), the skeleton, the joint order of the BVH rows and the placement -> the three outputs in float64.
"""
import numpy as np

from oracle import anim as oanim

SKEW = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
TURN_AXES = (np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]), SKEW)
TURN_STEP = 0.25


def unroll(q):
    """quat.unroll carried from the stream's first frame, which is emitted with w >= 0: q [T, ..., 4]"""
    q = np.array(q, np.float64)
    shape = q.shape
    q = q.reshape(shape[0], -1, 4)
    q[0] = np.where(q[0, :, :1] < 0.0, -q[0], q[0])
    return oanim.q_unroll(q).reshape(shape)


def placed_root(rpos, rrot, placement=None):
    """the root trajectory as handed out: re-based on frame 0 with a placement (start_position, start_rotation), as it is without"""
    rpos, rrot = np.asarray(rpos, np.float64), np.asarray(rrot, np.float64)
    if placement is None:
        return rpos, rrot
    inv0 = oanim.q_inv(rrot[0:1])
    sr = np.asarray(placement[1], np.float64)[None]
    return (oanim.q_mul_vec(sr, oanim.q_mul_vec(inv0, rpos - rpos[0:1])) + np.asarray(placement[0], np.float64)[None],
            oanim.q_mul(sr, oanim.q_mul(inv0, rrot)))


def frames(rpos, rrot, lpos, ltxy, parents, seq, placement=None, order="zyx"):
    """-> dict(root_pos [T,3], root_rot [T,4], lrot [T,J,4], lpos [T,J,3], gpos [T,J,3], grot [T,J,4], bvh [T,3+3J], and for the
    tests' own conditions: raw = dict of the quaternions before the sign rule, mid_sin [T,J]: the sine of the middle Euler angle)"""
    T, J = np.asarray(lpos).shape[:2]
    lpos = np.asarray(lpos, np.float64)
    lrot = oanim.q_from_xform(oanim.xform_from_xy(np.asarray(ltxy, np.float64).reshape(T, J, 2, 3)))
    rp, rr = placed_root(rpos, rrot, placement)
    flrot, flpos = lrot.copy(), lpos.copy()                      # the placed root folded into joint 0
    flrot[:, 0] = oanim.q_mul(rr, lrot[:, 0])
    flpos[:, 0] = oanim.q_mul_vec(rr, lpos[:, 0]) + rp
    grot, gpos = oanim.q_fk(flrot, flpos, list(parents))
    pos, eul = oanim.bvh_channels(rpos, rrot, lpos, np.asarray(ltxy).reshape(T, J, 2, 3), *(placement or (None, None)), order=order)
    assert np.array_equal(pos[:, 0], flpos[:, 0])               # (bvh_channels places and folds the root the same way)
    w, x, y, z = (flrot[..., i] for i in range(4))
    mid = 2.0 * (w * y - z * x) if order == "zyx" else 2.0 * (x * y + z * w)
    return dict(root_pos=rp, root_rot=unroll(rr), lrot=unroll(lrot), lpos=lpos, gpos=gpos, grot=unroll(grot),
                bvh=np.concatenate([pos[:, 0], eul[:, list(seq)].reshape(T, 3 * J)], axis=1),
                raw=dict(root_rot=rr, lrot=lrot, grot=grot), mid_sin=mid)


def sign_margins(o):
    """-> (min |dot| between neighbouring frames, min |w| of frame 0) over the three quaternion outputs: where the sign rule decides"""
    dots, w0 = [1.0], []
    for q in o["raw"].values():
        q = q.reshape(q.shape[0], -1, 4)
        w0.append(np.abs(q[0, :, 0]).min())
        if q.shape[0] > 1:
            dots.append(np.abs(np.sum(q[1:] * q[:-1], axis=-1)).min())
    return float(min(dots)), float(min(w0))


# ----------------------------------------------------------------------------- inputs
def q_axis(angle, axis):
    return oanim.q_from_angle_axis(np.asarray(angle, np.float64), np.asarray(axis, np.float64))


def xy_of(q):
    """two-axis encoding of q [..., 4] as float32 [..., 2, 3] with a second axis that is neither a unit vector nor orthogonal to
    the first: (1.7 x, 0.6 y + 0.2 x)"""
    x = oanim.q_mul_vec(q, np.array([1.0, 0.0, 0.0]))
    y = oanim.q_mul_vec(q, np.array([0.0, 1.0, 0.0]))
    return np.stack([1.7 * x, 0.6 * y + 0.2 * x], axis=-2).astype(np.float32)


def full_turn(T, axis, start=0.0):
    """rotations about `axis` by start + 0.25 n rad, n = 0 .. T - 1 -> [T, 4] (w = cos of half the angle: not sign continuous past pi)"""
    return q_axis(start + TURN_STEP * np.arange(T), np.broadcast_to(axis, (T, 3)))


def smooth(T, n, rng, spread=0.6, step=0.3):
    """n sequences of T rotations: a start within `spread` rad of the identity, then increments about a fixed axis of its own by
    at most `step` rad a frame (most joints slower: step u^3) -> [T, n, 4]"""
    ax = rng.standard_normal((2, n, 3))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    q0 = q_axis(spread * rng.random(n), ax[0])
    speed = step * rng.uniform(-1.0, 1.0, n) ** 3
    return np.stack([oanim.q_mul(q0, q_axis(speed * t, ax[1])) for t in range(T)])


def inputs(J, T, seed, turns=True):
    """the decoder-shaped frames of a stream of T frames and J joints: smooth random rotations everywhere, the full turns about x,
    y, z and the skew axis on the LAST min(J, 4) joints (placed so that the raw quaternion's sign flips -- the turn completes --
    in the middle of the sequence) -> dict(rpos [T,3], rrot [T,4], lpos [T,J,3], ltxy [T,J,2,3]) float32"""
    rng = np.random.default_rng(seed)
    q = smooth(T, J, rng)
    if turns:
        for i, axis in enumerate(TURN_AXES[:min(J, 4)]):
            q[:, J - 1 - i] = full_turn(T, axis, 2.0 * np.pi - TURN_STEP * (T // 2) + 0.124)
    rr = smooth(T, 1, rng, spread=0.5, step=0.05)[:, 0]
    rpos = np.cumsum(rng.standard_normal((T, 3)) * 0.5, axis=0) + rng.standard_normal(3) * 20.0
    lpos = rng.standard_normal((J, 3)) * 8.0 + rng.standard_normal((T, J, 3)) * 0.05
    return dict(rpos=rpos.astype(np.float32), rrot=rr.astype(np.float32), lpos=lpos.astype(np.float32), ltxy=xy_of(q))


# the cases of the kernel test: skeletons ("rig": zeggs.synth.PARENTS, 75 joints, is added by the test), frames per record, and
# per case the first seed for which the oracle ALONE leaves no frame out by the Euler rule (|sin| of the middle angle <= 0.999) and
# decides every sign with |dot| > 0.5 and |w| of frame 0 > 0.02, with and without the placement and in both channel orders
SKELETONS = {"one": [-1], "two": [-1, 0], "chain": [-1, 0, 1, 2, 3], "star": [-1, 0, 0, 0], "tree": [-1, 0, 0, 1, 2]}
TREE_SEQ = [0, 1, 3, 2, 4]          # depth first: the file order of "tree" differs from its index order
COUNTS = (1, 5, 20)
PLACE = (np.array([3.0, -1.5, 40.0]), q_axis(2.1, SKEW))
SEEDS = {("star", 20): 2, ("rig", 20): 2}


def seed_for(name, T):
    return SEEDS.get((name, T), 1)


def raw_flips(q):
    """sign changes of the dot product between neighbouring frames of q [T, 4] -> (count, min |dot|)"""
    d = np.sum(q[1:] * q[:-1], axis=-1)
    return int((d < 0.0).sum()), float(np.abs(d).min())
