"""Float64 oracle of the re-timing output head of live serving (include/zeggs_hip_retime.h), composed from
tests/live_frames_oracle.py and oracle/anim.py, and the counting rules restated in plain Python integers.  TEST INFRASTRUCTURE
ONLY: tests/test_live_retime_cpu.py checks it against itself, the frames oracle and the analytic cases,
tests/test_gpu_live_retime.py compares the kernel and the server with it.

frames(): the WHOLE input sequence of a stream at the server's rate and the ratio L / M -> the three outputs of every output frame
the stream has emitted after its last input frame, in float64.  Output frames that fall on an input frame are the frames oracle's
frames of that input, taken as they are; the others are the head's own steps (root folded into joint 0, Euler degrees, FK) on
locals interpolated between the two neighbours as the frames oracle stages them (placed root, local quaternions, local positions).
"""
from fractions import Fraction

import numpy as np

import live_frames_oracle as fo
from oracle import anim as oanim

MAX_TERM, MAX_UP = 4096, 8
# the ratios of the GPU tests: L / M of frame_rate / 60
RATIOS = ((1, 1), (1, 2), (2, 1), (3, 2), (2, 5), (5, 12), (500, 1001), (8, 1), (1, 7))
RATES = {24: (2, 5), 25: (5, 12), 30: (1, 2), 50: (5, 6), 72: (6, 5), 90: (3, 2), 120: (2, 1), 480: (8, 1),
         Fraction(24000, 1001): (400, 1001), Fraction(30000, 1001): (500, 1001), Fraction(60000, 1001): (1000, 1001),
         Fraction(120000, 1001): (2000, 1001)}


# ----------------------------------------------------------------------------- counting
def ratio(frame_rate, fps=60):
    """frame_rate / fps in lowest terms -> (L, M); ValueError outside 1 <= L, M <= 4096, L / M <= 8 or for a rate <= 0"""
    r = Fraction(frame_rate) / Fraction(fps)
    if r <= 0:
        raise ValueError("not a positive rate")
    if r.numerator > MAX_TERM or r.denominator > MAX_TERM or r > MAX_UP:
        raise ValueError(f"{r.numerator} / {r.denominator}")
    return r.numerator, r.denominator


def n_out(n, L, M):
    return 0 if n < 1 else ((n - 1) * L) // M + 1


def position(m, L, M):
    """output frame m sits at k + num / L"""
    return divmod(m * M, L)


def last_needed(m, L, M):
    k, num = position(m, L, M)
    return k if num == 0 else k + 1


# ----------------------------------------------------------------------------- interpolation of the staged locals
def slerp(a, b, t):
    """the shortest arc between unit quaternions a, b [..., 4] at t [..., 1] in (0, 1), as the definition states it"""
    a, b = np.asarray(a, np.float64), np.array(b, np.float64)
    d = np.sum(a * b, axis=-1, keepdims=True)
    b = np.where(d < 0.0, -b, b)
    d = np.abs(d)
    s = np.sqrt(np.maximum(0.0, 1.0 - d * d))
    th = np.arctan2(s, d)
    small = s < 1e-8
    ss = np.where(small, 1.0, s)
    wa = np.where(small, 1.0 - t, np.sin((1.0 - t) * th) / ss)
    wb = np.where(small, t, np.sin(t * th) / ss)
    q = wa * a + wb * b
    return q / np.sqrt(np.sum(q * q, axis=-1, keepdims=True))


def retime_locals(rp, rr, lrot, lpos, L, M):
    """the staged float64 locals of T input frames (placed root position [T,3] and rotation [T,4], local quaternions [T,J,4] and
    positions [T,J,3]) -> the same of the n_out(T) output frames, and `on` [n_out] bool: the frame falls on an input frame (it is
    that frame, untouched) and `k` [n_out]: its input frame (the earlier neighbour of a frame between two)"""
    T = len(rp)
    N = n_out(T, L, M)
    pos = [position(m, L, M) for m in range(N)]
    k = np.array([p[0] for p in pos], np.int64).reshape(N)
    num = np.array([p[1] for p in pos], np.int64).reshape(N)
    on = num == 0
    k1 = np.where(on, k, k + 1)
    assert N == 0 or k1.max() <= T - 1
    t = num.astype(np.float64) / float(L)
    out = []
    for x in (rp, lpos):
        x = np.asarray(x, np.float64)
        tt = t.reshape((N,) + (1,) * (x.ndim - 1))
        y = x[k] + tt * (x[k1] - x[k])
        y[on] = x[k[on]]
        out.append(y)
    for x in (rr, lrot):
        x = np.asarray(x, np.float64)
        tt = t.reshape((N,) + (1,) * (x.ndim - 1))
        y = slerp(x[k], x[k1], np.where(tt == 0.0, 0.5, tt))
        y[on] = x[k[on]]
        out.append(y)
    return out[0], out[2], out[3], out[1], on, k


def head(rp, rr, lrot, lpos, parents, seq, order="zyx"):
    """the head's own steps behind the staging, on float64 locals: the placed root folded into joint 0, FK over `parents`, the Euler
    degrees in `seq` order -> dict(gpos, bvh, mid_sin, raw grot)"""
    T, J = lpos.shape[:2]
    flrot, flpos = lrot.copy(), lpos.copy()
    flrot[:, 0] = oanim.q_mul(rr, lrot[:, 0])
    flpos[:, 0] = oanim.q_mul_vec(rr, lpos[:, 0]) + rp
    grot, gpos = oanim.q_fk(flrot, flpos, list(parents))
    eul = np.degrees(oanim.q_to_euler(flrot, order=order))
    w, x, y, z = (flrot[..., i] for i in range(4))
    mid = 2.0 * (w * y - z * x) if order == "zyx" else 2.0 * (x * y + z * w)
    return dict(gpos=gpos, grot=grot, bvh=np.concatenate([flpos[:, 0], eul[:, list(seq)].reshape(T, 3 * J)], axis=1), mid_sin=mid)


def frames(rpos, rrot, lpos, ltxy, parents, seq, L, M, placement=None, order="zyx"):
    """-> the dict of live_frames_oracle.frames for the n_out(T) output frames, plus on [n_out] (the frame is an input frame) and
    k [n_out] (which one)"""
    full = fo.frames(rpos, rrot, lpos, ltxy, parents, seq, placement, order)
    rp, rr, lrot, lp, on, k = retime_locals(full["root_pos"], full["raw"]["root_rot"], full["raw"]["lrot"], full["lpos"], L, M)
    h = head(rp, rr, lrot, lp, parents, seq, order)
    for key in ("gpos", "bvh", "mid_sin"):              # a frame on an input frame is the frames oracle's, as it is
        h[key][on] = full[key][k[on]]
    h["grot"][on] = full["raw"]["grot"][k[on]]
    N = len(on)
    un = fo.unroll if N else (lambda q: np.array(q, np.float64))
    return dict(root_pos=rp, root_rot=un(rr), lrot=un(lrot), lpos=lp, gpos=h["gpos"], grot=un(h["grot"]), bvh=h["bvh"],
                raw=dict(root_rot=rr, lrot=lrot, grot=h["grot"]), mid_sin=h["mid_sin"], on=on, k=k)


def left_out(o, gimbal=0.999):
    """share of the output frames the Euler rule leaves out of the BVH comparison"""
    return 0.0 if len(o["on"]) == 0 else 1.0 - float((np.abs(o["mid_sin"]) <= gimbal).all(axis=1).mean())
