"""Float64 oracle of the filter stage of the re-timing output head of live serving (include/zeggs_hip_refilter.h),
composed from tests/live_retime_oracle.py and tests/live_frames_oracle.py, and the counting rules restated in plain Python
integers.  TEST INFRASTRUCTURE ONLY: tests/test_live_refilter_cpu.py checks it against itself, the frames oracle and the analytic
cases, tests/test_gpu_live_refilter.py compares the kernel and the server with it.

frames(): the WHOLE input sequence of a CLOSED stream at the server's rate, the ratio L / M and the filter's table -> the three
outputs of its n_out(T) output frames in float64: the locals as the frames oracle stages them (placed root, local quaternions,
local positions), every output frame their weighted combination over the 2 H + 1 input frames around its position (an index below
0 is frame 0, an index above the last frame the last), then the head's own steps (live_retime_oracle.head) and the sign rule over
the OUTPUT sequence.  Stream: the same frame by frame as a running stream emits them, for the cut tests.
"""
import functools

import numpy as np

import live_frames_oracle as fo
import live_retime_oracle as ro

MAX_L, MAX_DOWN, MAX_Z = 1024, 4, 8
DEFAULTS = dict(zero_crossings=4, rolloff=0.75, beta=5.0)
# the ratios of the tests: L / M of frame_rate / 60; 1 / 1 is the jitter filter
RATIOS = ((2, 5), (1, 2), (500, 1001), (3, 2), (2, 1), (1, 1))
SMALL_NORM = 1e-8


# ----------------------------------------------------------------------------- table and counting
def half(L, M, Z=4):
    return -(-Z * max(L, M) // L)


@functools.lru_cache(maxsize=None)
def table(L, M, zero_crossings=4, rolloff=0.75, beta=5.0):
    """the definition, written out on its own (not through zeggs.audio): -> (table [L, 2 H + 1], H); computed once per ratio and
    shared (read only)"""
    Z = zero_crossings
    WL = Z * max(L, M)
    H = half(L, M, Z)
    W = WL / float(L)
    c = rolloff * min(1.0, L / float(M))
    tab = np.zeros((L, 2 * H + 1))
    for phase in range(L):
        for j in range(2 * H + 1):
            num = phase + (H - j) * L                     # t L, exact
            if abs(num) < WL:
                t = num / float(L)
                tab[phase, j] = c * np.sinc(c * t) * np.i0(beta * np.sqrt(1.0 - (t / W) ** 2)) / np.i0(beta)
        s = 0.0
        for j in range(2 * H + 1):                        # the row's own sum, ascending j
            s = s + tab[phase, j]
        tab[phase] = tab[phase] / s
    return tab, H


def nf(n, L, M, H):
    """output frames a filtered stream has emitted after n input frames while it runs"""
    return 0 if n <= H else ((n - H) * L - 1) // M + 1


def emitted(n, L, M, H, final):
    return ro.n_out(n, L, M) if final or H == 0 else nf(n, L, M, H)


def response(tab, H, f, fps=60.0):
    """|sum_j w_j e^(i w (j - H - phase / L))| of every phase row at f Hz of a stream at fps -> [L]: tap j sits j - H - phase / L
    input frames from the output it serves"""
    L = tab.shape[0]
    off = np.arange(2 * H + 1)[None, :] - H - np.arange(L)[:, None] / float(L)
    return np.abs(np.sum(tab * np.exp(2j * np.pi * f / fps * off), axis=1))


# ----------------------------------------------------------------------------- the filter over the staged locals
def _combine(x, idx, w, quat):
    """x [T, ..., 3 | 4], idx [taps] input frames, w [taps] -> the weighted combination; quaternions are brought to the side of
    the centre tap's (idx[H]) first, the sum is normalised, and the centre tap's is taken where the norm is below 1e-8"""
    taps = len(idx)
    centre = x[idx[taps // 2]]
    acc = np.zeros_like(centre)
    for j in range(taps):                                 # ascending j, one accumulator
        v = x[idx[j]]
        if quat:
            v = np.where(np.sum(v * centre, axis=-1, keepdims=True) < 0.0, -v, v)
        acc = acc + w[j] * v
    if not quat:
        return acc
    n = np.sqrt(np.sum(acc * acc, axis=-1, keepdims=True))
    return np.where(n < SMALL_NORM, centre, acc / np.where(n < SMALL_NORM, 1.0, n))


def filter_locals(rp, rr, lrot, lpos, L, M, tab, H, m0=0, m1=None, last=None):
    """the staged float64 locals of the input frames so far (placed root position [T,3] and rotation [T,4], local quaternions
    [T,J,4] and positions [T,J,3]) -> the same of output frames m0 .. m1 - 1 (default: all n_out(T) of a closed stream), taps
    held on frame 0 and on frame `last` (default T - 1), and k [m1 - m0]: the input frame under each"""
    T = len(rp)
    last = T - 1 if last is None else last
    m1 = ro.n_out(T, L, M) if m1 is None else m1
    out, ks = ([], [], [], []), []
    for m in range(m0, m1):
        k, num = ro.position(m, L, M)
        idx = np.clip(k - H + np.arange(2 * H + 1), 0, last)
        assert 0 <= k <= last
        for o, x, quat in zip(out, (rp, rr, lrot, lpos), (False, True, True, False)):
            o.append(_combine(np.asarray(x, np.float64), idx, tab[num], quat))
        ks.append(k)
    shapes = [np.asarray(x).shape[1:] for x in (rp, rr, lrot, lpos)]
    return tuple(np.array(o, np.float64).reshape((len(ks),) + s) for o, s in zip(out, shapes)) + (np.array(ks, np.int64),)


def frames(rpos, rrot, lpos, ltxy, parents, seq, L, M, tab, H, placement=None, order="zyx"):
    """-> the dict of live_frames_oracle.frames for the n_out(T) output frames of the closed stream, plus k [n_out]"""
    full = fo.frames(rpos, rrot, lpos, ltxy, parents, seq, placement, order)
    rp, rr, lrot, lp, k = filter_locals(full["root_pos"], full["raw"]["root_rot"], full["raw"]["lrot"], full["lpos"], L, M, tab, H)
    return finish(rp, rr, lrot, lp, k, parents, seq, order)


def finish(rp, rr, lrot, lp, k, parents, seq, order="zyx"):
    """the head's own steps and the sign rule behind filtered locals"""
    h = ro.head(rp, rr, lrot, lp, parents, seq, order)
    un = fo.unroll if len(k) else (lambda q: np.array(q, np.float64))
    return dict(root_pos=rp, root_rot=un(rr), lrot=un(lrot), lpos=lp, gpos=h["gpos"], grot=un(h["grot"]), bvh=h["bvh"],
                raw=dict(root_rot=rr, lrot=lrot, grot=h["grot"]), mid_sin=h["mid_sin"], k=k, on=np.zeros(len(k), bool))


def left_out(o, gimbal=0.999):
    """share of the output frames the Euler rule leaves out of the BVH comparison"""
    return 0.0 if len(o["k"]) == 0 else 1.0 - float((np.abs(o["mid_sin"]) <= gimbal).all(axis=1).mean())


def stream_locals(rp, rr, lrot, lpos, L, M, tab, H, cuts, final=True):
    """the filtered locals as a RUNNING stream emits them: the input in calls of cuts[i] frames, each call computing the frames
    nf(n0) .. nf(n1) - 1 from the frames delivered so far only; with `final` one more record without a frame emits the tail
    -> (the four locals concatenated, the number of frames each call emitted)"""
    parts, counts, n = [], [], 0
    for c in list(cuts) + ([0] if final else []):
        last_call = final and len(counts) == len(cuts)
        n1 = n + c
        m0, m1 = nf(n, L, M, H), emitted(n1, L, M, H, last_call)
        parts.append(filter_locals(rp[:n1], rr[:n1], lrot[:n1], lpos[:n1], L, M, tab, H, m0, m1, n1 - 1)[:4])
        counts.append(m1 - m0)
        n = n1
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4)), counts


# ----------------------------------------------------------------------------- the tone
TONE_AXIS = np.array([2.0, -1.0, 2.0]) / 3.0
TONE_AMP = 1e-3


def tone_inputs(T, f, J=1, joint=0, fps=60.0, amp=TONE_AMP):
    """T frames of a J-joint skeleton at rest but for joint `joint`, which turns by amp sin(2 pi f k / fps) rad about TONE_AXIS ->
    the frames oracle's inputs (float32, two-axis encoding) and the angles [T]"""
    ang = amp * np.sin(2.0 * np.pi * f * np.arange(T) / fps)
    q = np.zeros((T, J, 4))
    q[..., 0] = 1.0
    q[:, joint] = fo.q_axis(ang, np.broadcast_to(TONE_AXIS, (T, 3)))
    rr = np.zeros((T, 4), np.float32)
    rr[:, 0] = 1.0
    return dict(rpos=np.zeros((T, 3), np.float32), rrot=rr, lpos=np.zeros((T, J, 3), np.float32), ltxy=fo.xy_of(q)), ang


def tone_angle(lrot):
    """the signed angle about TONE_AXIS of quaternions [N, 4] (either sign)"""
    q = np.asarray(lrot, np.float64)
    q = np.where(q[:, :1] < 0.0, -q, q)
    return 2.0 * np.arctan2(q[:, 1:] @ TONE_AXIS, q[:, 0])


def interior(N, T, L, M, H):
    """the output frames all of whose taps lie inside the stream (no held frame): a mask [N]"""
    k = np.array([ro.position(m, L, M)[0] for m in range(N)])
    return (k - H >= 0) & (k + H <= T - 1)
