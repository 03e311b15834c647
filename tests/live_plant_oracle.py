"""Float64 oracle of the planting stage of live serving (include/zeggs_hip_plant.h; csrc/plant_math.h) and the
inputs its tests share.  TEST INFRASTRUCTURE ONLY: tests/test_live_plant_cpu.py checks it against itself and against the
header on the host, tests/test_gpu_live_plant.py compares the kernel, anim.plant_feet and the server with it.

The definition, once more, per model frame and chain (u, m, e) -- everything float64, positions and speeds in model units:
  FK over the ancestors of e from the RAW row (q_from_xform(xform_from_xy(ltxy)), the root folded into joint 0, no re-basing;
  the root's rotation and every local rotation brought to unit length first) gives the unconstrained world points H (u), K (m),
  A (e) and the world rotations.
  1. s = |A - a_prev| / dt (0 on the stream's first frame), y = A.y - ground.
  2. e_off = o0 g(k / N), N = release, g(x) = 1 - x^2 (3 - 2 x) for x < 1, else 0; 0 when N == 0.
  3. At most one transition: HELD and (s > v_off or y > h_off or |A - L| > slack) -> FREE, o0 = L - A, k = 0, e_off again;
     else FREE and s <= v_on and y <= h_on -> HELD, L = A + e_off.
  4. T = L when HELD, else A + e_off and k = min(k + 1, N).
  5. l1 = |K - H|, l2 = |A - K|; a T with |T - H| > stretch (l1 + l2) is pulled onto that sphere along T - H.
  6. A T that equals A: the chain's joints stay as they are.
  7. Else the two-bone solve: interior angles at H and K before (dot products of normalised differences, clamped) and after (cosine
     rule for |T - H| clamped to [EPS, stretch (l1 + l2)]); bend axis normalise((A - H) x (K - H)) (below EPS: the root's forward
     axis crossed with A - H); swing axis normalise((A - H) x (T - H)) (below EPS: no swing) by atan2(|(A - H) x (T - H)|, (A - H) . (T - H));
     u.lrot <- u.lrot R(bend, d_H) R(swing, angle), m.lrot <- m.lrot R(bend, d_K), every axis in the frame of the joint it turns
     (the swing in u's frame after the bend); e.lrot <- inv(m.world') e.world.  The two columns of the new rotations go back
     as ltxy, rounded to float32 once; every other float of the row leaves as the same bits.
  8. a_prev = A; the contact flag is mode == HELD.
"""
import numpy as np

from oracle import anim as oanim

EPS = 1e-8
FREE, HELD = 0, 1


# ----------------------------------------------------------------------------- small float64 helpers
def _q(x):
    return np.asarray(x, np.float64)


def qmul(a, b):
    return oanim.q_mul(_q(a), _q(b))


def qrot(q, v):
    return oanim.q_mul_vec(_q(q), _q(v))


def qinv(q):
    return oanim.q_inv(_q(q))


def axis_angle(axis, angle):
    h = 0.5 * angle
    return np.concatenate([[np.cos(h)], np.sin(h) * _q(axis)])


def norm(v):
    return float(np.sqrt(np.dot(v, v)))


def angle_dot(a, b):
    return float(np.arccos(np.clip(np.dot(a / norm(a), b / norm(b)), -1.0, 1.0)))


def to_xy(q):
    """the first two columns of the matrix of q / |q| -> [6]"""
    w, x, y, z = _q(q) / norm(q)
    return np.array([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + w * z), 2.0 * (x * z - w * y),
                     2.0 * (x * y - w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z + w * x)])


def fade(k, N):
    if N <= 0 or k >= N:
        return 0.0
    x = k / N
    return 1.0 - x * x * (3.0 - 2.0 * x)


def split(pose, J):
    """a pose row [.., 6 + 15J] -> (lpos [.., J, 3], ltxy [.., J, 2, 3]) views"""
    pose = np.asarray(pose)
    return pose[..., 6:6 + 3 * J].reshape(*pose.shape[:-1], J, 3), pose[..., 6 + 3 * J:6 + 9 * J].reshape(*pose.shape[:-1], J, 2, 3)


def local_rotations(ltxy):
    """the head's dq_from_xy over [.., J, 2, 3] float32, brought to unit length -> [.., J, 4] float64"""
    q = oanim.q_from_xform(oanim.xform_from_xy(np.asarray(ltxy, np.float64)))
    return q / np.sqrt(np.sum(q * q, axis=-1, keepdims=True))


# ----------------------------------------------------------------------------- the unconstrained chain
def chain_fk(lrot, lpos, rpos, rrot, parents, chain):
    """FK over the ancestors of the chain's foot, composed bottom up as the kernel composes it -> dict(H, K, A, gp: the world
    rotation of u's parent (the root's for a u that is joint 0), gu, gm, ge, root)"""
    u, m, e = chain
    gq, gx = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)
    a = parents[u]
    while a >= 0:
        gx = qrot(lrot[a], gx) + lpos[a]
        gq = qmul(lrot[a], gq)
        a = parents[a]
    rr = _q(rrot) / norm(_q(rrot))
    gx = qrot(rr, gx) + _q(rpos)
    gq = qmul(rr, gq)
    gu = qmul(gq, lrot[u])
    H = qrot(gq, lpos[u]) + gx
    gm = qmul(gu, lrot[m])
    K = qrot(gu, lpos[m]) + H
    A = qrot(gm, lpos[e]) + K
    return dict(H=H, K=K, A=A, gp=gq, gu=gu, gm=gm, ge=qmul(gm, lrot[e]), root=rr)


# ----------------------------------------------------------------------------- the state machine
def new_state():
    return dict(mode=FREE, L=np.zeros(3), o0=np.zeros(3), k=0, a_prev=np.zeros(3), started=False)


def step(opt, s, H, K, A, margins=None):
    """steps 1 - 5 and 8 on state s (changed in place) -> (T, held).  `margins`: a list that takes (what, lhs, rhs) of every
    comparison the frame decides"""
    note = (lambda *a: margins.append(a)) if margins is not None else (lambda *a: None)
    v_on, v_off = opt["speed"]
    h_on, h_off = opt["height"]
    N = opt["release"]
    sp = norm(A - s["a_prev"]) / opt["dt"] if s["started"] else 0.0
    y = A[1] - opt["ground"]
    off = fade(s["k"], N) * s["o0"]
    if s["mode"] == HELD:
        dist = norm(A - s["L"])
        note("v_off", sp, v_off), note("h_off", y, h_off), note("slack", dist, opt["slack"])
        if sp > v_off or y > h_off or dist > opt["slack"]:
            s["mode"], s["o0"], s["k"] = FREE, s["L"] - A, 0
            off = fade(0, N) * s["o0"]
    else:
        note("v_on", sp, v_on), note("h_on", y, h_on)
        if sp <= v_on and y <= h_on:
            s["mode"], s["L"] = HELD, A + off
    if s["mode"] == HELD:
        T = s["L"].copy()
    else:
        T = A + off
        s["k"] = min(s["k"] + 1, N)
    reach = opt["stretch"] * (norm(K - H) + norm(A - K))
    d = T - H
    note("reach", norm(d), reach)
    if norm(d) > reach:
        T = H + (reach / norm(d)) * d
    s["a_prev"], s["started"] = A.copy(), True
    return T, s["mode"] == HELD


# ----------------------------------------------------------------------------- the two-bone solve
def solve(stretch, H, K, A, T, gp, root, qu, qm, qe, margins=None):
    """step 7 -> the new local rotations (qu', qm', qe')"""
    note = (lambda *a: margins.append(a)) if margins is not None else (lambda *a: None)
    gu = qmul(gp, qu)
    gm = qmul(gu, qm)
    ge = qmul(gm, qe)
    ab, ac, at = K - H, A - H, T - H
    l1, l2 = norm(ab), norm(K - A)
    lat = float(np.clip(norm(at), EPS, stretch * (l1 + l2)))
    h0, k0 = angle_dot(ac, ab), angle_dot(H - K, A - K)
    h1 = float(np.arccos(np.clip((l2 * l2 - l1 * l1 - lat * lat) / (-2.0 * l1 * lat), -1.0, 1.0)))
    k1 = float(np.arccos(np.clip((lat * lat - l1 * l1 - l2 * l2) / (-2.0 * l1 * l2), -1.0, 1.0)))
    bend = np.cross(ac, ab)
    note("bend", norm(bend), EPS)
    if norm(bend) < EPS:
        bend = np.cross(qrot(root, [0.0, 0.0, 1.0]), ac)
    bend = bend / norm(bend) if norm(bend) > 0.0 else np.array([1.0, 0.0, 0.0])
    ru = axis_angle(qrot(qinv(gu), bend), h1 - h0)
    rm = axis_angle(qrot(qinv(gm), bend), k1 - k0)
    nu = qmul(qu, ru)
    swing = np.cross(ac, at)
    ns = norm(swing)
    note("swing", ns, EPS)
    if ns >= EPS:
        gub = qmul(gp, nu)
        nu = qmul(nu, axis_angle(qrot(qinv(gub), swing / ns), float(np.arctan2(ns, np.dot(ac, at)))))
    nm = qmul(qm, rm)
    gm2 = qmul(qmul(gp, nu), nm)
    return nu, nm, qmul(qinv(gm2), ge)


# ----------------------------------------------------------------------------- a whole sequence
def options(**over):
    """explicit options of the tests (NOT the package's defaults): speeds in units a second, lengths in units"""
    o = dict(speed=(15.0, 40.0), height=(12.0, 16.0), ground=0.5, slack=8.0, release=6, stretch=0.999, dt=1.0 / 60.0)
    o.update(over)
    return o


def plant(pose, rpos, rrot, parents, chains, opt, states=None, detail=False):
    """the stage over the frames pose [T, 6 + 15J] float32 of one stream -> (planted pose [T, 6 + 15J] float32, contacts [T, C] uint8).
    `states`: the chains' states (new_state() each), carried on from call to call.  detail=True -> also a dict: per frame and chain
    the unconstrained chain (H, K, A), the target T, solved: whether the solve ran, the new local rotations in float64 (lrot:
    [T, C, 3, 4], of u, m, e) with the rotations they replace (lrot0), gp, root, |o0| and k after the frame, and `margins`: every comparison as (frame, chain, what, lhs, rhs)."""
    pose = np.ascontiguousarray(pose, np.float32)
    T, J, C = pose.shape[0], len(parents), len(chains)
    assert pose.shape[1] == 6 + 15 * J
    states = [new_state() for _ in chains] if states is None else states
    lpos, ltxy = split(pose, J)
    lrot, lpos = local_rotations(ltxy), lpos.astype(np.float64)
    out, contacts = pose.copy(), np.zeros((T, C), np.uint8)
    out_xy = split(out, J)[1]
    det = dict(H=np.zeros((T, C, 3)), K=np.zeros((T, C, 3)), A=np.zeros((T, C, 3)), T=np.zeros((T, C, 3)), solved=np.zeros((T, C), bool),
               lrot=np.zeros((T, C, 3, 4)), lrot0=np.zeros((T, C, 3, 4)), gp=np.zeros((T, C, 4)), root=np.zeros((T, C, 4)), o0=np.zeros((T, C)),
               k=np.zeros((T, C), int), margins=[])
    for f in range(T):
        for c, chain in enumerate(chains):
            fk = chain_fk(lrot[f], lpos[f], rpos[f], rrot[f], parents, chain)
            H, K, A = fk["H"], fk["K"], fk["A"]
            m = []
            Tg, held = step(opt, states[c], H, K, A, m)
            contacts[f, c] = held
            q3 = [lrot[f, j] for j in chain]
            same = bool(np.all(Tg == A))
            if not same:
                q3n = solve(opt["stretch"], H, K, A, Tg, fk["gp"], fk["root"], *q3, margins=m)
                for j, q in zip(chain, q3n):
                    out_xy[f, j] = to_xy(q).reshape(2, 3).astype(np.float32)
            else:
                q3n = q3
            det["H"][f, c], det["K"][f, c], det["A"][f, c], det["T"][f, c], det["solved"][f, c] = H, K, A, Tg, not same
            det["lrot"][f, c], det["lrot0"][f, c], det["gp"][f, c], det["root"][f, c] = np.stack(q3n), np.stack(q3), fk["gp"], fk["root"]
            det["o0"][f, c], det["k"][f, c] = norm(states[c]["o0"]), states[c]["k"]
            det["margins"] += [(f, c) + x for x in m]
    return (out, contacts, det) if detail else (out, contacts)


def min_margin(margins):
    """the smallest relative margin |lhs - rhs| / max(|lhs|, |rhs|) over the comparisons of a run, and which one"""
    worst = (np.inf, None)
    for rec in margins:
        lhs, rhs = rec[-2], rec[-1]
        scale = max(abs(lhs), abs(rhs))
        r = abs(lhs - rhs) / scale if scale > 0.0 else np.inf
        if r < worst[0]:
            worst = (r, rec)
    return worst


# ----------------------------------------------------------------------------- inputs: a scripted walk
# the 9-joint skeleton: pelvis, then two chains of upper leg, lower leg, foot and toe
WALK_PARENTS = [-1, 0, 1, 2, 3, 0, 5, 6, 7]
WALK_NAMES = ["Hips", "RightUpLeg", "RightLeg", "RightFoot", "RightToeBase", "LeftUpLeg", "LeftLeg", "LeftFoot", "LeftToeBase"]
WALK_CHAINS = [(1, 2, 3), (5, 6, 7)]
RIG_CHAINS = [("RightUpLeg", "RightLeg", "RightFoot"), ("LeftUpLeg", "LeftLeg", "LeftFoot")]
T_WALK = 40
L1, L2 = 41.0, 39.0
STAND, FLY = 9.0, 25.0            # ankle heights above y = 0 of a standing and of a swinging foot


def _script(T, seed):
    """the ankle's world track of both feet and the pelvis track.  The pelvis walks on at 2 units a frame.  Each foot alternately
    stands (a slow drift under v_on) and swings.  The right foot's first stance turns into a drag at a speed between v_on and
    v_off, behind the hip: the held point leaves the leg's reach (frames 17, 18), then the slack releases it (frame 19) and it
    swings.  The left foot slips for one frame in its first stance (a release) and stands again in the next (a re-entry in the
    unfinished fade)."""
    rng = np.random.default_rng(seed)
    pelvis_y = 68.0 + 0.2 * rng.random()
    pelvis = np.stack([np.array([0.4 * np.sin(0.21 * f + seed), pelvis_y + 0.5 * np.sin(0.33 * f), 2.0 * f]) for f in range(T)])
    side = (-9.0, 9.0)
    # per foot: where it starts behind (-) the pelvis, then (first frame, kind, step in z a frame) spans
    plans = ((-25.0, ((0, "stand", 0.08), (7, "stand", 0.6), (20, "swing", 12.0), (28, "stand", 0.07))),
             (-40.0, ((0, "swing", 10.5), (8, "stand", 0.09), (15, "stand", -1.1), (16, "stand", 0.09), (26, "swing", 6.2), (34, "stand", 0.06))))
    tracks = []
    for c, (z, plan) in enumerate(plans):
        tr = np.zeros((T, 3))
        for f in range(T):
            start, kind, dz = [p for p in plan if p[0] <= f][-1]
            ends = [p[0] for p in plan if p[0] > f]
            z += dz if f else 0.0
            y = STAND
            if kind == "swing":
                span = (ends[0] if ends else T) - start
                y = STAND + 6.0 + (FLY - STAND) * np.sin(np.pi * (f - start + 0.5) / span) ** 0.5
            tr[f] = (side[c] + 0.05 * np.sin(0.4 * f + c), y + 0.02 * np.sin(0.9 * f + c), z)
        tracks.append(tr)
    return pelvis, tracks


def _rest(J, parents, chains, rng):
    """rest offsets: the legs hang down with L1, L2; everything else a few units from its parent"""
    lpos = rng.standard_normal((J, 3)) * 4.0
    for c, (u, m, e) in enumerate(chains):
        lpos[u] = (-9.0 if c == 0 else 9.0, -4.0, 0.5)
        lpos[m] = (0.3, -L1, 0.2)
        lpos[e] = (-0.2, -L2, 0.4)
    return lpos


def walk(parents, chains, seed, T=T_WALK, names=None):
    """the decoder-shaped rows of a stream of T frames on `parents` whose chains `chains` (indices) walk the script -> dict(pose
    [T, 6 + 15J] float32, rpos [T, 3], rrot [T, 4] float32).  The legs are posed by solve() from a bent rest pose; every other
    joint turns smoothly at random; the remaining floats of a row are noise."""
    rng = np.random.default_rng(seed)
    J = len(parents)
    pelvis, tracks = _script(T, seed)
    lpos0 = _rest(J, parents, chains, rng)
    ax = rng.standard_normal((J, 3))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    sp, ph = 0.05 * rng.uniform(-1, 1, J), 0.3 * rng.uniform(-1, 1, J)
    pose = (rng.standard_normal((T, 6 + 15 * J)) * 0.3).astype(np.float32)
    rpos, rrot = np.zeros((T, 3), np.float32), np.zeros((T, 4), np.float32)
    lpos_v, ltxy_v = split(pose, J)
    for f in range(T):
        lrot = np.stack([axis_angle(ax[j], ph[j] + sp[j] * f) for j in range(J)])
        lrot[0] = axis_angle([0.0, 1.0, 0.0], 0.06 * np.sin(0.17 * f))
        lpos = lpos0 + 0.01 * rng.standard_normal((J, 3))
        lpos[0] = (0.0, 0.0, 0.0)
        rr = axis_angle([0.0, 1.0, 0.0], 0.1 * np.sin(0.05 * f + seed))
        # the root sits under the pelvis; joint 0 carries the height
        rp = np.array([pelvis[f, 0], 0.0, pelvis[f, 2]])
        lpos[0] = qrot(qinv(rr), pelvis[f] - rp)
        for c, (u, m, e) in enumerate(chains):          # a bent leg first, then the solve puts its ankle on the script
            a = parents[u]
            lrot[u], lrot[m] = axis_angle([1.0, 0.0, 0.0], -0.5), axis_angle([1.0, 0.0, 0.0], 0.9)
            while a > 0:                                # legs hang from the pelvis through unturned joints (the rig: directly)
                lrot[a] = np.array([1.0, 0.0, 0.0, 0.0])
                a = parents[a]
            fk = chain_fk(lrot, lpos, rp, rr, parents, (u, m, e))
            lrot[u], lrot[m], lrot[e] = solve(1.0, fk["H"], fk["K"], fk["A"], tracks[c][f], fk["gp"], fk["root"], lrot[u], lrot[m], lrot[e])
        lpos_v[f] = lpos.astype(np.float32)
        for j in range(J):                              # a two-axis encoding that is neither normalised nor orthogonal
            x, y = qrot(lrot[j], [1.0, 0.0, 0.0]), qrot(lrot[j], [0.0, 1.0, 0.0])
            ltxy_v[f, j] = np.stack([1.3 * x, 0.7 * y + 0.15 * x]).astype(np.float32)
        rpos[f], rrot[f] = rp.astype(np.float32), rr.astype(np.float32)
    return dict(pose=pose, rpos=rpos, rrot=rrot)


def chain_indices(chains, names):
    return [tuple(names.index(j) if isinstance(j, str) else int(j) for j in c) for c in chains]


def skeletons():
    """{name: (parents, names, chains as the options give them, chains as indices)}: the 9-joint walker, chains by index, and
    the 75-joint rig, chains by name"""
    from zeggs import synth
    return {"walker": (WALK_PARENTS, WALK_NAMES, WALK_CHAINS, WALK_CHAINS),
            "rig": (list(synth.PARENTS), list(synth.BONE_NAMES), RIG_CHAINS, chain_indices(RIG_CHAINS, synth.BONE_NAMES))}


_CACHE = {}


def case(name, seed):
    """the shared input and its oracle run for skeleton `name`: dict(parents, names, chains, idx, opt, pose, rpos, rrot, out,
    contacts, det) -- computed once, never changed (the arrays are read-only)"""
    key = (name, seed)
    if key not in _CACHE:
        parents, names, chains, idx = skeletons()[name]
        w = walk(parents, idx, seed)
        opt = options()
        out, contacts, det = plant(w["pose"], w["rpos"], w["rrot"], parents, idx, opt, detail=True)
        for a in (*w.values(), out, contacts):
            a.setflags(write=False)
        _CACHE[key] = dict(parents=parents, names=names, chains=chains, idx=idx, opt=opt, out=out, contacts=contacts, det=det, **w)
    return _CACHE[key]


def knee_angles(det):
    """interior knee angles of the unconstrained chains in degrees [T, C]"""
    a, b = det["H"] - det["K"], det["A"] - det["K"]
    cosv = np.sum(a * b, -1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
    return np.degrees(np.arccos(np.clip(cosv, -1.0, 1.0)))


def plant_kwargs(opt, chains):
    """the oracle's options as anim.plant_feet / LiveServer(plant=) take them"""
    return dict(chains=chains, speed=opt["speed"], height=opt["height"], ground=opt["ground"], slack=opt["slack"], release=opt["release"],
                stretch=opt["stretch"])
