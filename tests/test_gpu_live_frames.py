"""LiveServer's output head (include/zeggs_hip_frames.h): zeggs_live_frames against the float64 oracle
(tests/live_frames_oracle.py) and against zeggs_pose_to_bvh_table, its independence of the cuts and of the other rows bit for bit,
and the server's "frames" from step() to close()."""
import functools

import numpy as np
import pytest
import torch

import live_frames_oracle as fo
import test_gpu_live_push as lp
from zeggs import anim, audio, capi, live, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23            # float32 outputs: half a unit of float32 rounding (2^-24 s) plus float64 noise far below it
BVH_TOL = 1e-9              # BVH rows: degrees and position units
GIMBAL = 0.999              # ... on frames where the oracle's |sin| of the middle angle is at most this
MARGIN = 1e-3               # signs are compared where the oracle decides them by more than this
SKELETONS = dict(fo.SKELETONS, rig=list(synth.PARENTS))
QUATS, POSITIONS = ("root_rot", "lrot", "grot"), ("root_pos", "lpos", "gpos")
GUARD = 7.25


def _seq(name):
    return fo.TREE_SEQ if name == "tree" else ops.frames_seq(SKELETONS[name])


def _pose_rows(x, seed=0):
    """the oracle's inputs as the decoder's rows: pose [T, 6 + 15J] (what the head does not read is noise), rpos, rrot -- on the device"""
    T, J = x["lpos"].shape[:2]
    pose = np.random.default_rng(seed).standard_normal((T, 6 + 15 * J)).astype(np.float32)
    pose[:, 6:6 + 3 * J] = x["lpos"].reshape(T, 3 * J)
    pose[:, 6 + 3 * J:6 + 9 * J] = x["ltxy"].reshape(T, 6 * J)
    return tuple(torch.as_tensor(np.ascontiguousarray(a), device=DEV) for a in (pose, x["rpos"], x["rrot"]))


class _Out:
    """destinations of one record with a guard behind each: LOCAL, WORLD (float32) and BVH (float64)"""

    def __init__(self, lf, count):
        self.count, self.lf = count, lf
        self.local = torch.full((count * lf.local_floats + 8,), GUARD, device=DEV)
        self.world = torch.full((count * lf.world_floats + 8,), GUARD, device=DEV)
        self.bvh = torch.full((count * lf.bvh_doubles + 8,), GUARD, device=DEV, dtype=torch.float64)

    def guards_ok(self):
        n = self.count
        return bool((self.local[n * self.lf.local_floats:] == GUARD).all() and (self.world[n * self.lf.world_floats:] == GUARD).all()
                    and (self.bvh[n * self.lf.bvh_doubles:] == GUARD).all())

    def host(self):
        buf = np.concatenate([self.bvh[:self.count * self.lf.bvh_doubles].cpu().numpy().view(np.uint8),
                              self.local[:self.count * self.lf.local_floats].cpu().numpy().view(np.uint8),
                              self.world[:self.count * self.lf.world_floats].cpu().numpy().view(np.uint8)])
        return live.frames_unpack(buf, [self.count], self.lf.J, 7)[0]


def _record(q, row, src, a, c, out):
    pose, rpos, rrot = src
    q.pose, q.rpos, q.rrot = pose[a:].data_ptr(), rpos[a:].data_ptr(), rrot[a:].data_ptr()
    q.pose_ld, q.rpos_ld, q.rrot_ld = pose.stride(0), rpos.stride(0), rrot.stride(0)
    q.local, q.world, q.bvh, q.row, q.count = out.local.data_ptr(), out.world.data_ptr(), out.bvh.data_ptr(), row, c


def _run_cuts(lf, row, src, cuts):
    """frames [0, sum(cuts)) of `src` through row `row` in calls of cuts[i] frames each (one record, in the kernel arguments)
    -> the outputs concatenated; every guard is looked at"""
    parts, a = [], 0
    rec = (capi.FramesRow * 1)()
    for c in cuts:
        out = _Out(lf, c)
        _record(rec[0], row, src, a, c, out)
        ops.live_frames(lf, rec, 1)
        assert out.guards_ok(), (a, c)
        parts.append(out.host())
        a += c
    return live.frames_cat(parts)


def _row_state(lf, row):
    torch.cuda.synchronize()
    per = (lf.state.numel() - (3 * lf.J * 4 + 7) // 8 * 8) // lf.d.rows
    off = lf.state.numel() - (lf.d.rows - row) * per
    return lf.state[off:off + per].cpu().numpy().copy()


def _reset(lf, row, src, place):
    if place is None:
        ops.live_frames_reset(lf, row)
    else:
        ops.live_frames_reset(lf, row, src[1][0].cpu().numpy(), src[2][0].cpu().numpy(), *place)


def _compare(got, want, what=""):
    """the bounds of the issue: float32 outputs within 2^-23 s of the oracle (s = 1 for quaternions, max(1, max |coordinate|) of
    the frame's positions), BVH rows within 1e-9 on the frames the Euler rule keeps; signs where the oracle decides them by more
    than 1e-3 (elsewhere, and behind such a frame on the same track, a quaternion is compared up to its sign).
    -> (fraction of frames the Euler rule leaves out, fraction of quaternion tracks compared with their sign)"""
    T = want["lpos"].shape[0]
    signed = total = 0
    for key in QUATS:
        g, w, raw = (a.reshape(T, -1, 4) for a in (got[key].astype(np.float64), want[key], want["raw"][key]))
        margin = np.abs(raw[:, :, 0]) if T == 1 else np.concatenate([np.abs(raw[:1, :, 0]), np.abs(np.sum(raw[1:] * raw[:-1], axis=-1))])
        sure = np.logical_and.accumulate(margin > MARGIN, axis=0)              # [T, tracks]: decided so far on this track
        s = np.where(np.sum(g * w, axis=-1, keepdims=True) < 0.0, -1.0, 1.0)
        assert (s[..., 0][sure] == 1.0).all(), f"{what}{key}: a sign differs where the oracle decides it"
        err = np.abs(g - s * w).max()
        assert err <= EPS, f"{what}{key}: {err:.3e} > 2^-23"
        signed, total = signed + int(sure[-1].sum()), total + sure.shape[1]
    groups = {"root_pos": ("root_pos", "lpos"), "lpos": ("root_pos", "lpos"), "gpos": ("gpos",)}
    for key in POSITIONS:
        s = np.maximum(1.0, np.max([np.abs(want[k].reshape(T, -1)).max(axis=1) for k in groups[key]], axis=0))
        err = np.abs(got[key].astype(np.float64) - want[key]).reshape(T, -1).max(axis=1)
        assert (err <= EPS * s).all(), f"{what}{key}: {float((err / s).max()):.3e} s > 2^-23 s"
    keep = (np.abs(want["mid_sin"]) <= GIMBAL).all(axis=1)
    if keep.any():
        err = np.abs(got["bvh"][keep] - want["bvh"][keep]).max()
        assert err <= BVH_TOL, f"{what}bvh: {err:.3e} > 1e-9"
    assert np.isfinite(got["bvh"]).all()
    return 1.0 - keep.mean(), signed / total


# ----------------------------------------------------------------------------- 1. the kernel against the oracle
@functools.lru_cache(maxsize=None)
def _case(name, T):
    return fo.inputs(len(SKELETONS[name]), T, fo.seed_for(name, T))


LEFT_OUT = []


@pytest.mark.parametrize("T", fo.COUNTS)
@pytest.mark.parametrize("name", list(SKELETONS))
def test_kernel_equals_the_oracle(name, T):
    """one record of T frames per skeleton (one joint, two, a chain, a star, a tree whose file order differs from its index order,
    the 75-joint rig: 20 frames of it go in two passes), smooth random rotations with a scaled, skewed second axis and the four full
    turns, with and without a placement, channel orders zyx and xzy: LOCAL, WORLD and BVH within the bounds of _compare, every sign
    compared (the oracle decides each by more than 1e-3), no frame left out by the Euler rule; the BVH rows also within 1e-9 of
    zeggs_pose_to_bvh_table with the same reference; LOCAL's lpos is the input bit for bit; guards behind every destination"""
    parents, seq, x = SKELETONS[name], _seq(name), _case(name, T)
    J = len(parents)
    src = _pose_rows(x, T)
    for order in ("zyx", "xzy"):
        lf = ops.LiveFrames(2, parents, 20, ("local", "world", "bvh"), order, seq, DEV)
        for row, place in ((1, None), (0, fo.PLACE)):
            want = fo.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], parents, seq, place, order)
            dot, w0 = fo.sign_margins(want)
            assert dot > MARGIN and w0 > MARGIN
            _reset(lf, row, src, place)
            got = _run_cuts(lf, row, src, [T])
            left_out, signed = _compare(got, want, f"{name} T={T} {order} placed={place is not None}: ")
            LEFT_OUT.append(left_out)
            assert signed == 1.0 and left_out == 0.0
            assert np.array_equal(got["lpos"], x["lpos"])
            # the offline kernel, same reference frame
            d = capi.BvhDims(T, J, int(place is not None))
            d.order = anim._to_euler_order(order)
            if place is not None:
                d.start_pos[:], d.start_rot[:] = list(place[0]), list(place[1])
            table = torch.empty(T, 3 + 3 * J, dtype=torch.float64, device=DEV)
            lpos, ltxy = (torch.as_tensor(x[k], device=DEV).contiguous() for k in ("lpos", "ltxy"))
            capi.api().zeggs_pose_to_bvh_table(d, src[1], src[2], lpos, ltxy, src[1][:1].contiguous(), src[2][:1].contiguous(),
                                               torch.as_tensor(np.asarray(seq, np.int32), device=DEV), table, ops._stream())
            err = float(np.abs(table.cpu().numpy() - got["bvh"]).max())
            assert err <= BVH_TOL, (name, T, order, err)
    assert np.mean(LEFT_OUT) <= 0.01


def test_outputs_that_are_off_are_not_written():
    """what = BVH alone and LOCAL | WORLD: the destinations whose bit is off may be NULL, the others are what the full head writes"""
    parents, seq, x = SKELETONS["tree"], fo.TREE_SEQ, _case("tree", 5)
    src = _pose_rows(x)
    full = ops.LiveFrames(1, parents, 20, ("local", "world", "bvh"), "zyx", seq, DEV)
    _reset(full, 0, src, fo.PLACE)
    want = _run_cuts(full, 0, src, [5])
    for what in (("bvh",), ("local", "world")):
        lf = ops.LiveFrames(1, parents, 20, what, "zyx", seq, DEV)
        _reset(lf, 0, src, fo.PLACE)
        out, rec = _Out(lf, 5), (capi.FramesRow * 1)()
        _record(rec[0], 0, src, 0, 5, out)
        for k in ("local", "world", "bvh"):
            if k not in what:
                setattr(rec[0], k, None)
        ops.live_frames(lf, rec, 1)
        got = out.host()
        for k in ("local", "world", "bvh"):
            for key in ops.FRAMES_KEYS[k]:
                if k in what:
                    assert got[key].tobytes() == want[key].tobytes(), (what, key)
                else:
                    assert (got[key] == GUARD).all(), (what, key)


# ----------------------------------------------------------------------------- 2. cuts and neighbours, bit for bit
@pytest.mark.parametrize("name", ["rig", "tree"])
def test_cuts_do_not_change_a_bit(name):
    """one 20-frame record (two passes on the rig), twenty 1-frame calls and 5 + 1 + 14: all outputs and the row's state identical"""
    parents, seq, x = SKELETONS[name], _seq(name), _case(name, 20)
    src = _pose_rows(x)
    lf = ops.LiveFrames(3, parents, 20, ("local", "world", "bvh"), "zyx", seq, DEV)
    runs = []
    for row, cuts in ((0, [20]), (1, [1] * 20), (2, [5, 1, 14])):
        _reset(lf, row, src, fo.PLACE)
        runs.append((_run_cuts(lf, row, src, cuts), _row_state(lf, row)))
    for got, state in runs[1:]:
        for key in runs[0][0]:
            assert got[key].tobytes() == runs[0][0][key].tobytes(), key
        assert state.tobytes() == runs[0][1].tobytes()
    assert runs[0][1][120:].view(np.float32).any() and runs[0][1][112:120].view(np.int32).tolist() == [1, 1]      # rebase, started


def test_64_records_in_one_launch_equal_each_row_alone():
    """64 rows of the tree, two calls: counts mixed over 0, 1 and 5 (rows with 0 in both calls stay untouched), the records on the
    device, against the same rows one by one on a second state: outputs and states identical, rows that are absent from a call
    keep their state, guards behind every destination"""
    parents, seq = SKELETONS["tree"], fo.TREE_SEQ
    x = fo.inputs(5, 10, 5)
    src = _pose_rows(x)
    both = [ops.LiveFrames(64, parents, 20, ("local", "world", "bvh"), "zyx", seq, DEV) for _ in range(2)]
    for lf in both:
        for r in range(64):
            _reset(lf, r, src, fo.PLACE if r % 2 else None)
    together, alone = both
    rng = np.random.default_rng(11)
    done = [0] * 64
    for call in range(2):
        counts = [int(rng.choice([0, 1, 5])) for _ in range(64)]
        counts[7] = counts[8] = 0
        absent = [r for r in range(64) if r % 9 == 4]                       # not in the call at all
        rows = [r for r in range(64) if r not in absent]
        before = {r: _row_state(together, r) for r in absent + [7, 8]}
        recs, outs = (capi.FramesRow * len(rows))(), []
        for q, r in zip(recs, rows):
            outs.append(_Out(together, counts[r]))
            _record(q, r, src, done[r], counts[r], outs[-1])
        dev = lp._to_device(recs)
        ops.live_frames(together, recs, len(rows), dev.data_ptr())
        for r, out in zip(rows, outs):
            assert out.guards_ok(), r
            if counts[r]:
                want = _run_cuts(alone, r, tuple(t[done[r]:] for t in src), [counts[r]])
                got = out.host()
                for key in want:
                    assert got[key].tobytes() == want[key].tobytes(), (call, r, key)
                assert _row_state(together, r).tobytes() == _row_state(alone, r).tobytes(), (call, r)
            done[r] += counts[r]
        for r, state in before.items():
            assert _row_state(together, r).tobytes() == state.tobytes(), (call, r)
    assert max(done) >= 6 and done[7] == 0


# ----------------------------------------------------------------------------- 3. the server
FRAMES = dict(parents=synth.PARENTS, names=synth.BONE_NAMES)
NSAMP = 16000                    # 1 s: 60 frames


def _serve(srv, streams, chunk, many):
    """streams: {sid: wav}; the audio in chunks of `chunk` samples through push() or push_many(), a step() after every round, then
    drain() and close() -> {sid: [parts]} (each part: pose, rpos, rrot tensors and "frames")"""
    parts = {sid: [] for sid in streams}
    n = max(w.size for w in streams.values())
    for a in range(0, n, chunk):
        if many:
            srv.push_many({sid: w[a:a + chunk] for sid, w in streams.items()})
        else:
            for sid, w in streams.items():
                srv.push(sid, w[a:a + chunk])
        for sid, o in srv.step().items():
            parts[sid].append(o)
    for sid, o in srv.drain().items():
        parts[sid].append(o)
    for sid in streams:
        parts[sid].append(srv.close(sid))
    return parts


def _whole(parts):
    parts = [p for p in parts if p]
    out = {k: torch.cat([p[k] for p in parts]).cpu().numpy() for k in lp.KEYS}
    out["frames"] = live.frames_cat([p["frames"] for p in parts])
    return out


def _oracle_of(w, place, order="zyx"):
    J = len(synth.PARENTS)
    T = w["pose"].shape[0]
    return fo.frames(w["rpos"], w["rrot"], w["pose"][:, 6:6 + 3 * J].reshape(T, J, 3), w["pose"][:, 6 + 3 * J:6 + 9 * J].reshape(T, J, 2, 3),
                     synth.PARENTS, ops.frames_seq(synth.PARENTS), place, order)


@pytest.mark.parametrize("rows", [1, 2, 8])
def test_server_frames_equal_the_oracle_of_the_streams_own_rows(rows):
    """rows = 1 (the B = 1 decoder path), 2 and 8 streams at tick 4, every second one placed: each stream's "frames" from step() to
    close() equal the oracle applied to that stream's own concatenated pose, rpos and rrot; frame 0, the first pose, is there once;
    launches_per_step is the 9 (10 at one row) of a server without the head plus two, which a second server in the same process
    still reports, without a "frames" key"""
    srv, plain = lp._server(rows, 4, frames=FRAMES), lp._server(rows, 4)
    places = [fo.PLACE if r % 2 else None for r in range(rows)]
    sids = [srv.open(lp._first(3 + r % 2), lp._style(70 + r), **({} if p is None else dict(start_position=p[0], start_rotation=p[1])))
            for r, p in enumerate(places)]
    wavs = {sid: lp._wav(NSAMP - 1600 * (r % 3), 60 + r) for r, sid in enumerate(sids)}
    parts = _serve(srv, wavs, 1600, rows > 1)
    assert srv.stats["launches_per_step"] == (12 if rows == 1 else 11) and srv.stats["frame_bytes"] > 0
    psids = [plain.open(lp._first(3), lp._style(70)) for _ in range(rows)]
    pparts = _serve(plain, {sid: lp._wav(NSAMP, 60) for sid in psids}, 1600, rows > 1)
    assert plain.stats["launches_per_step"] == (10 if rows == 1 else 9) and "frame_bytes" not in plain.stats
    assert all("frames" not in p for v in pparts.values() for p in v) and plain._fr is None and plain._fr_stage is None
    for r, sid in enumerate(sids):
        w = _whole(parts[sid])
        T = audio.n_anim_frames(wavs[sid].size)
        assert w["pose"].shape[0] == T and all(v.shape[0] == T for v in w["frames"].values())
        first = lp._first(3 + r % 2)
        assert np.array_equal(w["rpos"][0], first[0][0].to(torch.float32).cpu().numpy())
        assert sum("frames" in p for p in parts[sid]) == len([p for p in parts[sid] if p]) >= 3
        want = _oracle_of(w, places[r])
        left_out, signed = _compare(w["frames"], want, f"rows={rows} stream {r}: ")
        print(f"rows={rows} stream {r}: {T} frames, {left_out:.1%} left out by the Euler rule, {signed:.1%} of the tracks compared with their sign")
        assert left_out < 0.5 and signed > 0.9


def test_server_frames_are_a_function_of_the_frame_sequence():
    """the same stream (audio, style, first pose, placement) on three servers of 8 rows: pushed alone with push() in chunks of 1600,
    with push_many() in chunks of 2500 among three other open streams, and the same with other streams half as long.  Each variant's frames are, bit for bit, what the kernel gives for that variant's own pose rows in ONE other cut (records
    of 20 frames on a fresh state), so they depend on the frame sequence alone; and wherever two variants decoded the same bits,
    their frames are the same bits"""
    wav = lp._wav(NSAMP, 81)
    got = []
    for variant in range(3):
        srv = lp._server(8, 4, frames=FRAMES)
        others = [srv.open(lp._first(4), lp._style(90 + i)) for i in range(3 if variant else 0)]
        sid = srv.open(lp._first(3), lp._style(80), start_position=fo.PLACE[0], start_rotation=fo.PLACE[1])
        streams = {o: lp._wav(NSAMP // (2 if variant == 2 else 1), 82 + i) for i, o in enumerate(others)}
        streams[sid] = wav
        got.append(_whole(_serve(srv, streams, 2500 if variant else 1600, bool(variant))[sid]))
    lf = ops.LiveFrames(1, synth.PARENTS, 20, ("local", "world", "bvh"), "zyx", None, DEV)
    for i, w in enumerate(got):
        src = tuple(torch.as_tensor(w[k], device=DEV) for k in lp.KEYS)
        T = w["pose"].shape[0]
        _reset(lf, 0, src, fo.PLACE)
        again = _run_cuts(lf, 0, src, [20] * (T // 20) + ([T % 20] if T % 20 else []))
        for key, v in again.items():
            assert w["frames"][key].tobytes() == v.tobytes(), (i, key)
    same = 0
    for w in got[1:]:
        if all(np.array_equal(w[k], got[0][k]) for k in lp.KEYS):
            same += 1
            for key, v in got[0]["frames"].items():
                assert w["frames"][key].tobytes() == v.tobytes(), key
    print(f"{same} of 2 variants decoded the bits of the first")


def test_two_placements_differ_by_the_rigid_transform():
    """two streams on the same audio, style and first pose, one handed out as it is and one placed.  The decoder gives two rows
    with the same input rows that agree within its bound, not bit for bit (measured: tests/test_gpu_live.py's bound is what the
    existing tests ask of it), so the transform is checked where it is exact: the placed stream's world positions and root are the
    rigid transform start_rot ref_rot^-1 (x - ref_pos) + start_pos of what the head gives for THAT stream's own rows without a
    placement (the kernel on a fresh state); the two streams' rows agree within the decoder's bound.  Bound: each side
    carries at most 2^-24 s of float32 rounding (s = the larger max |coordinate| of the two frames, at least 1) and the transform
    of the first side's error has its size: 2^-23 s; as much again for the rotation's own path: 2^-22 s"""
    srv = lp._server(2, 4, frames=dict(FRAMES, what=("local", "world")))
    a = srv.open(lp._first(3), lp._style(75))
    b = srv.open(lp._first(3), lp._style(75), start_position=fo.PLACE[0], start_rotation=fo.PLACE[1])
    wav = lp._wav(NSAMP, 77)
    parts = _serve(srv, {a: wav, b: wav}, 1600, True)
    bound = lp._bound(srv)
    wa, wb = _whole(parts[a]), _whole(parts[b])
    assert all(np.abs(wa[k] - wb[k]).max() <= bound for k in lp.KEYS)
    assert "bvh" not in wa["frames"] and set(wa["frames"]) == {"root_pos", "root_rot", "lrot", "lpos", "gpos", "grot"}
    lf = ops.LiveFrames(1, synth.PARENTS, 20, ("local", "world"), "zyx", None, DEV)
    src = tuple(torch.as_tensor(wb[k], device=DEV) for k in lp.KEYS)
    T = wb["pose"].shape[0]
    _reset(lf, 0, src, None)
    rec, free = (capi.FramesRow * 1)(), []
    for f0 in range(0, T, 20):
        out = _Out(lf, min(20, T - f0))
        _record(rec[0], 0, src, f0, out.count, out)
        rec[0].bvh = None
        ops.live_frames(lf, rec, 1)
        free.append({k: v for k, v in out.host().items() if k != "bvh"})
    free = live.frames_cat(free)
    r0 = fo.oanim.q_inv(wb["rrot"][0:1].astype(np.float64))
    sr = fo.PLACE[1][None]
    for key in ("gpos", "root_pos"):
        pa, pb = free[key].astype(np.float64), wb["frames"][key].astype(np.float64)
        want = fo.oanim.q_mul_vec(sr, fo.oanim.q_mul_vec(r0, pa - wb["rpos"][0].astype(np.float64))) + fo.PLACE[0]
        s = np.maximum(1.0, np.maximum(np.abs(pa).reshape(T, -1).max(axis=1), np.abs(pb).reshape(T, -1).max(axis=1)))
        err = np.abs(want - pb).reshape(T, -1).max(axis=1)
        print(f"{key}: max |placed - transform(unplaced)| / s = {float((err / s).max()):.3e}")
        assert (err <= 2.0 ** -22 * s).all(), (key, float((err / s).max()))
    assert np.array_equal(free["lrot"], wb["frames"]["lrot"]) and np.array_equal(free["lpos"], wb["frames"]["lpos"])
    qa = fo.oanim.q_mul(sr[None], fo.oanim.q_mul(r0[None], free["grot"].astype(np.float64)))
    qb = wb["frames"]["grot"].astype(np.float64)
    assert np.abs(np.abs(np.sum(qa * qb, axis=-1)) - 1.0).max() <= 2.0 ** -20      # the same rotation (either sign); four float32 quaternions' norms


@pytest.mark.parametrize("order", ["zyx", "xzy"])
def test_text_is_format_rows_and_reads_back_as_a_bvh_file(order, tmp_path):
    """text=True: each stream's bytes equal anim.format_rows of its returned rows, step by step; bvh_header(sid, n) plus the
    concatenated text is a file whose numbers are the returned rows within 5e-7, the last printed digit, and anim.bvh_load reads
    it back to exactly those numbers as float32"""
    srv = lp._server(2, 4, frames=dict(FRAMES, what=("bvh",), order=order, text=True))
    sids = [srv.open(lp._first(3), lp._style(95)), srv.open(lp._first(4), lp._style(96), start_position=fo.PLACE[0], start_rotation=fo.PLACE[1])]
    T = audio.n_anim_frames(NSAMP // 2)
    heads = {sid: srv.bvh_header(sid, T) for sid in sids}
    parts = _serve(srv, {sid: lp._wav(NSAMP // 2, 97 + i) for i, sid in enumerate(sids)}, 1600, True)
    assert srv.stats["launches_per_step"] == 11 + 3
    seq = ops.frames_seq(synth.PARENTS)
    for sid in sids:
        for p in parts[sid]:
            if p:
                assert set(p["frames"]) == {"bvh", "text"} and isinstance(p["frames"]["text"], bytes)
                assert p["frames"]["text"] == anim.format_rows(np.ascontiguousarray(p["frames"]["bvh"]))
        w = _whole(parts[sid])
        assert w["frames"]["bvh"].shape == (T, 3 + 3 * len(seq)) and f"Frames: {T}\n" in heads[sid]
        path = tmp_path / f"{sid}.bvh"
        path.write_bytes(heads[sid].encode() + w["frames"]["text"])
        back = anim.bvh_load(str(path))
        rows = np.concatenate([back["positions"][:, 0], back["rotations"][:, seq].reshape(T, -1)], axis=1)
        # the printed numbers are the returned rows within 5e-7, the last printed digit; bvh_load holds them as float32, which adds
        # half a float32 unit of the value (2^-24 |v|: 8e-6 at 131 degrees) on top
        printed = np.array(w["frames"]["text"].split(), np.float64).reshape(T, -1)
        assert np.abs(printed - w["frames"]["bvh"]).max() <= 5e-7
        assert back["order"] == order and back["rotations"].dtype == np.float32
        assert (np.abs(rows - w["frames"]["bvh"]) <= 5e-7 + 2.0 ** -24 * np.abs(w["frames"]["bvh"])).all()
        assert np.array_equal(rows, printed.astype(np.float32))
        # frame 0 stands on its offsets: the first row's root position is joint 0's OFFSET
        assert (np.abs(back["offsets"][0] - w["frames"]["bvh"][0, :3]) <= 5e-7 + 2.0 ** -24 * np.abs(w["frames"]["bvh"][0, :3])).all()
        assert back["names"] == list(synth.BONE_NAMES) and list(back["parents"]) == list(synth.PARENTS)
