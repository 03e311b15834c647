"""LiveServer's re-timing output head (include/zeggs_hip_retime.h): zeggs_live_frames_retimed against the float64 oracle
(tests/live_retime_oracle.py) and against the plain head (zeggs_live_frames), its independence of the cuts and of the other rows
bit for bit, and the server's "frames" at each stream's own rate from step() to close().  The bounds are the plain head's
(tests/test_gpu_live_frames.py: _compare)."""
import functools

import numpy as np
import pytest
import torch

import live_frames_oracle as fo
import live_retime_oracle as ro
import test_gpu_live_frames as plain
import test_gpu_live_push as lp
from test_live_retime_cpu import GPU_CASES
from zeggs import anim, audio, capi, live, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SKELETONS = plain.SKELETONS
T_IN = 20
ALL = ("local", "world", "bvh")
KEYS = ("root_pos", "root_rot", "lrot", "lpos", "gpos", "grot", "bvh")


@functools.lru_cache(maxsize=None)
def _case(name):
    return fo.inputs(len(SKELETONS[name]), T_IN, GPU_CASES[name])


@functools.lru_cache(maxsize=None)
def _oracle(name, ratio, placed, order):
    """computed once per case and shared (read only)"""
    x = _case(name)
    return ro.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], SKELETONS[name], plain._seq(name), *ratio, fo.PLACE if placed else None, order)


def _reset(lr, row, src, place):
    if place is None:
        ops.live_retime_reset(lr, row)
    else:
        ops.live_retime_reset(lr, row, src[1][0].cpu().numpy(), src[2][0].cpu().numpy(), *place)


def _record(q, row, src, a, c, out, ratio, n_in):
    plain._record(q, row, src, a, c, out)
    q.L, q.M, q.n_in = ratio[0], ratio[1], n_in
    q.outputs = ro.n_out(n_in + c, *ratio) - ro.n_out(n_in, *ratio)
    return q.outputs


def _run_cuts(lr, row, src, cuts, ratio, n_in=0, off=()):
    """input frames [0, sum(cuts)) of `src` through row `row` in calls of cuts[i] frames each (one record, in the kernel arguments)
    -> the outputs concatenated; every guard is looked at; destinations named in `off` are NULL"""
    parts, a = [], 0
    rec = (capi.RetimeRow * 1)()
    for c in cuts:
        n = ro.n_out(n_in + a + c, *ratio) - ro.n_out(n_in + a, *ratio)
        out = plain._Out(lr, n)
        assert _record(rec[0], row, src, a, c, out, ratio, n_in + a) == n
        for k in off:
            setattr(rec[0], k, None)
        ops.live_frames_retimed(lr, rec, 1)
        assert out.guards_ok(), (a, c)
        parts.append(out.host())
        a += c
    return live.frames_cat(parts)


def _row_state(lr, row):
    torch.cuda.synchronize()
    per = (lr.state.numel() - (3 * lr.J * 4 + 7) // 8 * 8) // lr.d.rows
    off = lr.state.numel() - (lr.d.rows - row) * per
    return lr.state[off:off + per].cpu().numpy().copy()


def _same_bits(a, b, what, keys=KEYS):
    for key in keys:
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (what, key)


# ----------------------------------------------------------------------------- 1. the kernel against the oracle
@pytest.mark.parametrize("ratio", ro.RATIOS, ids=lambda r: f"{r[0]}over{r[1]}")
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_kernel_equals_the_oracle(name, ratio):
    """one record of 20 input frames per skeleton (one joint, the tree whose file order differs from its index order, the 75-joint
    rig: two output passes from 2 / 1 on) and ratio, with and without a placement, channel orders zyx and xzy: LOCAL, WORLD and BVH
    of every output frame within the plain head's bounds (float32 outputs within 2^-23 s, BVH rows within 1e-9 where the oracle's
    |sin| of the middle angle is at most 0.999), signs where the oracle decides them; at most 5 % of a case's output frames are
    left out by the Euler rule; LOCAL's lpos of a frame that falls on an input frame is the input bit for bit; guards behind
    every destination"""
    parents, seq, x = SKELETONS[name], plain._seq(name), _case(name)
    src = plain._pose_rows(x, T_IN)
    N = ro.n_out(T_IN, *ratio)
    for order in ("zyx", "xzy"):
        lr = ops.LiveRetime(2, parents, T_IN, ALL, order, seq, DEV)
        for row, place in ((1, None), (0, fo.PLACE)):
            want = _oracle(name, ratio, place is not None, order)
            _reset(lr, row, src, place)
            got = _run_cuts(lr, row, src, [T_IN], ratio)
            assert got["bvh"].shape[0] == N == len(want["on"])
            what = f"{name} {ratio[0]}/{ratio[1]} {order} placed={place is not None}: "
            left_out, signed = plain._compare(got, want, what)
            print(f"{what}{N} frames, {left_out:.1%} left out by the Euler rule, {signed:.1%} of the tracks compared with their sign")
            assert left_out <= 0.05 and left_out == ro.left_out(want)
            assert np.array_equal(got["lpos"][want["on"]], x["lpos"][want["k"][want["on"]]])


@pytest.mark.parametrize("what", [("local",), ("world",), ("bvh",)])
def test_each_output_alone_is_what_the_full_head_writes(what):
    """each `what` bit alone at 3 / 2 on the placed tree: the destinations whose bit is off are NULL and stay untouched, the other
    is what the head with all three writes, bit for bit"""
    parents, seq, x = SKELETONS["tree"], fo.TREE_SEQ, _case("tree")
    src = plain._pose_rows(x)
    full = ops.LiveRetime(1, parents, T_IN, ALL, "zyx", seq, DEV)
    _reset(full, 0, src, fo.PLACE)
    want = _run_cuts(full, 0, src, [T_IN], (3, 2))
    lr = ops.LiveRetime(1, parents, T_IN, what, "zyx", seq, DEV)
    _reset(lr, 0, src, fo.PLACE)
    got = _run_cuts(lr, 0, src, [7, 13], (3, 2), off=[k for k in ALL if k not in what])
    for k in ALL:
        for key in ops.FRAMES_KEYS[k]:
            if k in what:
                assert got[key].tobytes() == want[key].tobytes(), (what, key)
            else:
                assert (got[key] == plain.GUARD).all(), (what, key)


# ----------------------------------------------------------------------------- 2. against the plain head
@pytest.mark.parametrize("name", ["tree", "rig"])
def test_one_to_one_is_the_plain_head_bit_for_bit(name):
    """L = M = 1 in cuts of 5 + 1 + 14 against zeggs_live_frames in one record, both channel orders, with a placement: every
    output and the carried state the two share (placement, flags, the quaternions last emitted) are the same bits"""
    parents, seq, x = SKELETONS[name], plain._seq(name), _case(name)
    src = plain._pose_rows(x)
    for order in ("zyx", "xzy"):
        lr = ops.LiveRetime(2, parents, T_IN, ALL, order, seq, DEV)
        lf = ops.LiveFrames(2, parents, T_IN, ALL, order, seq, DEV)
        _reset(lr, 1, src, fo.PLACE)
        plain._reset(lf, 1, src, fo.PLACE)
        got = _run_cuts(lr, 1, src, [5, 1, 14], (1, 1))
        want = plain._run_cuts(lf, 1, src, [T_IN])
        _same_bits(got, want, (name, order))
        shared = plain._row_state(lf, 1)
        assert _row_state(lr, 1)[:shared.size].tobytes() == shared.tobytes() and shared[112:120].view(np.int32).tolist() == [1, 1]


@pytest.mark.parametrize("ratio", [(1, 2), (2, 1)], ids=["1over2", "2over1"])
@pytest.mark.parametrize("name", ["tree", "rig"])
def test_frames_on_an_input_frame_are_the_plain_heads(name, ratio):
    """30 and 120 from 60: the output frames that fall on an input frame carry the plain head's positions and BVH rows of that
    frame bit for bit, and its quaternions up to their sign (the sign follows the stream's own previous OUTPUT frame)"""
    parents, seq, x = SKELETONS[name], plain._seq(name), _case(name)
    src = plain._pose_rows(x)
    lr = ops.LiveRetime(1, parents, T_IN, ALL, "zyx", seq, DEV)
    lf = ops.LiveFrames(1, parents, T_IN, ALL, "zyx", seq, DEV)
    _reset(lr, 0, src, fo.PLACE)
    plain._reset(lf, 0, src, fo.PLACE)
    got = _run_cuts(lr, 0, src, [T_IN], ratio)
    want = plain._run_cuts(lf, 0, src, [T_IN])
    N = ro.n_out(T_IN, *ratio)
    pos = [ro.position(m, *ratio) for m in range(N)]
    on = np.array([num == 0 for _, num in pos])
    k = np.array([kk for kk, _ in pos])[on]
    assert on.sum() == (10 if ratio == (1, 2) else 20) and N == (10 if ratio == (1, 2) else 39)
    for key in ("root_pos", "lpos", "gpos", "bvh"):
        assert got[key][on].tobytes() == want[key][k].tobytes(), key
    for key in ("root_rot", "lrot", "grot"):
        g, w = got[key][on], want[key][k]
        assert (np.all(g == w, axis=-1) | np.all(g == -w, axis=-1)).all(), key


# ----------------------------------------------------------------------------- 3. cuts and neighbours, bit for bit
@pytest.mark.parametrize("name", ["tree", "rig"])
def test_cuts_do_not_change_a_bit(name):
    """at every ratio of the list: one 20-frame record, twenty 1-frame calls and 5 + 1 + 14 give identical outputs and identical
    state (the raw last frame included) -- a frame between the last input of one call and the first of the next is the same bits"""
    parents, seq, x = SKELETONS[name], plain._seq(name), _case(name)
    src = plain._pose_rows(x)
    lr = ops.LiveRetime(3, parents, T_IN, ALL, "zyx", seq, DEV)
    for ratio in ro.RATIOS:
        runs = []
        for row, cuts in ((0, [20]), (1, [1] * 20), (2, [5, 1, 14])):
            _reset(lr, row, src, fo.PLACE)
            runs.append((_run_cuts(lr, row, src, cuts, ratio), _row_state(lr, row)))
        assert runs[0][0]["bvh"].shape[0] == ro.n_out(T_IN, *ratio)
        for got, state in runs[1:]:
            _same_bits(got, runs[0][0], (name, ratio))
            assert state.tobytes() == runs[0][1].tobytes(), ratio
        raw = runs[0][1][120 + (4 + 8 * len(parents)) * 4:].view(np.float32)[:7 + 9 * len(parents)]
        J = len(parents)
        want = np.concatenate([x["rpos"][-1], x["rrot"][-1], x["lpos"][-1].reshape(-1), x["ltxy"][-1].reshape(-1)])
        assert raw.tobytes() == want.tobytes() and raw.size == 7 + 9 * J, ratio


def test_64_records_in_one_launch_equal_each_row_alone():
    """64 rows of the tree, three calls: input counts mixed over 0, 1 and 5 and ratios mixed over the list, the records on the
    device, against the same rows one by one on a second state: outputs and states identical (records that emit nothing
    included: their raw frame moves on), rows that are absent from a call keep their state, guards behind every destination"""
    parents, seq = SKELETONS["tree"], fo.TREE_SEQ
    x = fo.inputs(5, 15, 5)
    src = plain._pose_rows(x)
    both = [ops.LiveRetime(64, parents, T_IN, ALL, "zyx", seq, DEV) for _ in range(2)]
    for lr in both:
        for r in range(64):
            _reset(lr, r, src, fo.PLACE if r % 2 else None)
    together, alone = both
    rng = np.random.default_rng(11)
    ratios = [ro.RATIOS[r % len(ro.RATIOS)] for r in range(64)]
    done, emitted, silent = [0] * 64, 0, 0
    for call in range(3):
        counts = [int(rng.choice([0, 1, 5])) for _ in range(64)]
        counts[7] = counts[8] = 0
        absent = [r for r in range(64) if r % 9 == 4]                       # not in the call at all
        rows = [r for r in range(64) if r not in absent]
        before = {r: _row_state(together, r) for r in absent + [7, 8]}
        recs, outs = (capi.RetimeRow * len(rows))(), []
        for q, r in zip(recs, rows):
            n = ro.n_out(done[r] + counts[r], *ratios[r]) - ro.n_out(done[r], *ratios[r])
            outs.append(plain._Out(together, n))
            _record(q, r, src, done[r], counts[r], outs[-1], ratios[r], done[r])
        dev = lp._to_device(recs)
        ops.live_frames_retimed(together, recs, len(rows), dev.data_ptr())
        for r, out in zip(rows, outs):
            assert out.guards_ok(), r
            if counts[r]:
                want = _run_cuts(alone, r, tuple(t[done[r]:] for t in src), [counts[r]], ratios[r], n_in=done[r])
                _same_bits(out.host(), want, (call, r))
                assert _row_state(together, r).tobytes() == _row_state(alone, r).tobytes(), (call, r)
                emitted, silent = emitted + out.count, silent + (out.count == 0)
            done[r] += counts[r]
        for r, state in before.items():
            assert _row_state(together, r).tobytes() == state.tobytes(), (call, r)
    assert max(done) >= 10 and done[7] == 0 and emitted > 100 and silent >= 3


# ----------------------------------------------------------------------------- 4. the server
FRAMES = dict(plain.FRAMES, text=True)
NSAMP = 16000                    # 1 s: 60 frames


def _whole(parts):
    parts = [p for p in parts if p]
    out = {k: torch.cat([p[k] for p in parts]).cpu().numpy() for k in lp.KEYS}
    out["frames"] = live.frames_cat([p["frames"] for p in parts])
    return out


def test_server_hands_out_each_stream_at_its_own_rate(tmp_path):
    """four streams on one server with max_rate 120: 30 frames a second (placed), 90, native (no frame_rate) and 24, text=True.
    Per stream: the frame counts follow the rule through step(), drain() and close() -- a part holds n_out(n1) - n_out(n0) frames
    for the input frames it brings, close() adds none beyond n_out of all of them, frame0 is contiguous; the frames equal, bit for
    bit, the kernel run on the stream's own returned pose / rpos / rrot rows in ANOTHER cut (records of 20 on a fresh state);
    bvh_header(sid, n) plus the concatenated text is a file anim.bvh_load reads: n frames, the stream's own frame time, rows that
    are the returned "bvh"; launches_per_step is that of a plain-head server of the same shape"""
    srv = lp._server(4, 4, frames=FRAMES, retime=dict(max_rate=120))
    ref = lp._server(4, 4, frames=FRAMES)
    rates = [30, 90, None, 24]
    ratios = [(1, 2), (3, 2), (1, 1), (2, 5)]
    places = [fo.PLACE, None, None, None]
    sids = [srv.open(lp._first(3 + r % 2), lp._style(70 + r), frame_rate=rate,
                     **({} if p is None else dict(start_position=p[0], start_rotation=p[1])))
            for r, (rate, p) in enumerate(zip(rates, places))]
    wavs = {sid: lp._wav(NSAMP - 1600 * (r % 3), 60 + r) for r, sid in enumerate(sids)}
    parts = plain._serve(srv, wavs, 1600, True)
    rsids = [ref.open(lp._first(3), lp._style(70)) for _ in range(4)]
    plain._serve(ref, {sid: lp._wav(NSAMP, 60) for sid in rsids}, 1600, True)
    assert srv.stats["launches_per_step"] == ref.stats["launches_per_step"] == 11 + 3
    assert isinstance(srv._fr, ops.LiveRetime) and type(ref._fr) is ops.LiveFrames
    seq = ops.frames_seq(synth.PARENTS)
    lr = ops.LiveRetime(1, synth.PARENTS, 20, ALL, "zyx", None, DEV)
    for r, sid in enumerate(sids):
        ratio = ratios[r]
        n_in = m = 0
        for p in (p for p in parts[sid] if p):
            f = p["frames"]
            n_in += p["pose"].shape[0]
            assert f["frame0"] == m and f["bvh"].shape[0] == ro.n_out(n_in, *ratio) - m, (r, n_in)
            assert all(f[k].shape[0] == f["bvh"].shape[0] for k in KEYS) and isinstance(f["text"], bytes)
            assert f["text"] == (anim.format_rows(np.ascontiguousarray(f["bvh"])) if f["bvh"].shape[0] else b"")
            m += f["bvh"].shape[0]
        T = audio.n_anim_frames(wavs[sid].size)
        N = ro.n_out(T, *ratio)
        assert n_in == T and m == N
        w = _whole(parts[sid])
        assert w["pose"].shape[0] == T and w["frames"]["frame0"] == 0
        # the kernel on the stream's own rows, another cut
        src = tuple(torch.as_tensor(w[k], device=DEV) for k in lp.KEYS)
        _reset(lr, 0, src, places[r])
        again = _run_cuts(lr, 0, src, [20] * (T // 20) + ([T % 20] if T % 20 else []), ratio)
        _same_bits(w["frames"], again, r)
    # the file (bvh_header is asked while a stream is open): a second, short run of two streams on the same server
    a = srv.open(lp._first(3), lp._style(95), frame_rate=(30000, 1001))
    b = srv.open(lp._first(4), lp._style(96), frame_rate=90, start_position=fo.PLACE[0], start_rotation=fo.PLACE[1])
    T = audio.n_anim_frames(NSAMP // 2)
    want_n = {a: ro.n_out(T, 500, 1001), b: ro.n_out(T, 3, 2)}
    heads = {sid: srv.bvh_header(sid, want_n[sid]) for sid in (a, b)}
    parts = plain._serve(srv, {sid: lp._wav(NSAMP // 2, 97 + i) for i, sid in enumerate((a, b))}, 1600, True)
    for sid, dt in ((a, synth.DT * 1001 / 500), (b, synth.DT * 2 / 3)):
        w = _whole(parts[sid])
        N = want_n[sid]
        assert w["frames"]["bvh"].shape == (N, 3 + 3 * len(seq)) and f"Frames: {N}\n" in heads[sid]
        assert "Frame Time: %f\n" % dt in heads[sid]
        path = tmp_path / f"{sid}.bvh"
        path.write_bytes(heads[sid].encode() + w["frames"]["text"])
        back = anim.bvh_load(str(path))
        assert back["rotations"].shape[0] == N and abs(back["frametime"] - dt) <= 5e-7
        rows = np.concatenate([back["positions"][:, 0], back["rotations"][:, seq].reshape(N, -1)], axis=1)
        printed = np.array(w["frames"]["text"].split(), np.float64).reshape(N, -1)
        assert np.abs(printed - w["frames"]["bvh"]).max() <= 5e-7          # the last printed digit, as the plain head's test
        assert np.array_equal(rows, printed.astype(np.float32))
        assert back["names"] == list(synth.BONE_NAMES) and list(back["parents"]) == list(synth.PARENTS)


def test_a_server_without_retime_is_the_server_it_was():
    """LiveServer(frames=..., retime=None) against a server built without the argument, same streams: the plain head's state and
    records, no "frame0", launches_per_step 11; each server's frames are, bit for bit, zeggs_live_frames on its own rows, and
    where the two decoded the same bits their frames are the same bits"""
    got = []
    for kw in (dict(retime=None), {}):
        srv = lp._server(2, 4, frames=plain.FRAMES, **kw)
        assert type(srv._fr) is ops.LiveFrames and srv.retime_conf is None and isinstance(srv._fr_stage.recs[0], ops.FramesRow)
        sids = [srv.open(lp._first(3), lp._style(75)), srv.open(lp._first(4), lp._style(76), start_position=fo.PLACE[0], start_rotation=fo.PLACE[1])]
        assert all(srv._rows[srv._sids[s]].rt is None for s in sids)
        with pytest.raises(ValueError, match="re-timing is off"):
            srv.open(lp._first(3), lp._style(77), frame_rate=30)
        parts = plain._serve(srv, {sid: lp._wav(NSAMP // 2, 60 + i) for i, sid in enumerate(sids)}, 1600, True)
        assert srv.stats["launches_per_step"] == 11
        assert all("frame0" not in p["frames"] for v in parts.values() for p in v if p)
        got.append([plain._whole(parts[sid]) for sid in sids])
    lf = ops.LiveFrames(1, synth.PARENTS, 20, ALL, "zyx", None, DEV)
    for ws in got:
        for w, place in zip(ws, (None, fo.PLACE)):
            src = tuple(torch.as_tensor(w[k], device=DEV) for k in lp.KEYS)
            T = w["pose"].shape[0]
            plain._reset(lf, 0, src, place)
            again = plain._run_cuts(lf, 0, src, [20] * (T // 20) + ([T % 20] if T % 20 else []))
            _same_bits(w["frames"], again, "own rows")
    for wa, wb in zip(*got):
        if all(np.array_equal(wa[k], wb[k]) for k in lp.KEYS):
            _same_bits(wa["frames"], wb["frames"], "two servers")
