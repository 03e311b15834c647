"""The filter stage of LiveServer's re-timing output head (include/zeggs_hip_refilter.h): zeggs_live_frames_refiltered against the
float64 oracle (tests/live_refilter_oracle.py), its independence of the cuts, of where the final record falls and of the other rows
bit for bit, its unfiltered rows against zeggs_live_frames_retimed bit for bit, a tone above half the output rate through the
kernel, and the server's filtered "frames" from step() to close().  The bounds are the plain head's
(tests/test_gpu_live_frames.py: _compare)."""
import functools

import numpy as np
import pytest
import torch

import live_frames_oracle as fo
import live_refilter_oracle as rf
import live_retime_oracle as ro
import test_gpu_live_frames as plain
import test_gpu_live_push as lp
import test_gpu_live_retime as unfiltered
from test_live_refilter_cpu import GPU_CASES, LEFT_OUT_CAP, T_IN
from zeggs import anim, audio, capi, live, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SKELETONS = plain.SKELETONS
ALL = ("local", "world", "bvh")
KEYS = unfiltered.KEYS
MAX_HALF = 16
_same_bits = unfiltered._same_bits


@functools.lru_cache(maxsize=None)
def _case(name):
    return fo.inputs(len(SKELETONS[name]), T_IN, GPU_CASES[name])


@functools.lru_cache(maxsize=None)
def _oracle(name, ratio, placed, order):
    """computed once per case and shared (read only)"""
    x = _case(name)
    return rf.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], SKELETONS[name], plain._seq(name), *ratio, *rf.table(*ratio),
                     fo.PLACE if placed else None, order)


def _head(rows, parents, seq, order="zyx", max_frames=T_IN, max_half=MAX_HALF, options=None):
    return ops.LiveRefilter(rows, parents, max_frames, max_half, options, ALL, order, seq, DEV)


def _reset(lr, row, src, place):
    if place is None:
        ops.live_refilter_reset(lr, row)
    else:
        ops.live_refilter_reset(lr, row, src[1][0].cpu().numpy(), src[2][0].cpu().numpy(), *place)


def _half_of(lr, ratio, filtered):
    """-> (H, the table's device address) of a row at `ratio`; (0, None) without the filter"""
    if not filtered:
        return 0, None
    t = lr.table(*ratio)
    return t["half"], t["table"].data_ptr()


def _record(q, row, src, a, c, out, ratio, n_in, half, table, final):
    plain._record(q, row, src, a, c, out)
    q.L, q.M, q.n_in, q.half, q.table, q.final = ratio[0], ratio[1], n_in, half, table, int(final)
    q.outputs = rf.emitted(n_in + c, *ratio, half, final) - rf.emitted(n_in, *ratio, half, False)
    return q.outputs


def _run_cuts(lr, row, src, cuts, ratio, filtered=True, final=True, n_in=0):
    """input frames [0, sum(cuts)) of `src` through row `row` in calls of cuts[i] frames each (one record, in the kernel
    arguments), the LAST of them marked final when `final` (a cut of 0 frames there is the record that only closes the stream)
    -> the outputs concatenated; every guard is looked at"""
    half, table = _half_of(lr, ratio, filtered)
    parts, a = [], 0
    rec = (capi.RefilterRow * 1)()
    for i, c in enumerate(cuts):
        last = final and i == len(cuts) - 1
        n = rf.emitted(n_in + a + c, *ratio, half, last) - rf.emitted(n_in + a, *ratio, half, False)
        out = plain._Out(lr, n)
        assert _record(rec[0], row, src, min(a, src[0].shape[0] - 1), c, out, ratio, n_in + a, half, table, last) == n
        ops.live_frames_refiltered(lr, rec, 1)
        assert out.guards_ok(), (a, c)
        parts.append(out.host())
        a += c
    return live.frames_cat(parts)


def _row_state(lr, row):
    torch.cuda.synchronize()
    per = (lr.state.numel() - (3 * lr.J * 4 + 7) // 8 * 8) // lr.d.rows
    off = lr.state.numel() - (lr.d.rows - row) * per
    return lr.state[off:off + per].cpu().numpy().copy()


# ----------------------------------------------------------------------------- 1. the kernel against the oracle
@pytest.mark.parametrize("ratio", rf.RATIOS, ids=lambda r: f"{r[0]}over{r[1]}")
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_kernel_equals_the_oracle(name, ratio):
    """one final record of 48 input frames per skeleton (one joint, the tree whose file order differs from its index order, the
    75-joint rig: several output passes) and ratio (24, 30, 29.97, 90, 120 from 60 and the jitter filter at 1 / 1), with and
    without a placement, channel orders zyx and xzy: LOCAL, WORLD and BVH of all n_out(48) output frames within the plain head's
    bounds (float32 outputs within 2^-23 s, BVH rows within 1e-9 where the oracle's |sin| of the middle angle is at most 0.999),
    signs where the oracle decides them; at most 10 % of a case's output frames are left out by the Euler rule, and no more than
    the oracle alone leaves out; guards behind every destination"""
    parents, seq, x = SKELETONS[name], plain._seq(name), _case(name)
    src = plain._pose_rows(x, T_IN)
    N = ro.n_out(T_IN, *ratio)
    for order in ("zyx", "xzy"):
        lr = _head(2, parents, seq, order)
        for row, place in ((1, None), (0, fo.PLACE)):
            want = _oracle(name, ratio, place is not None, order)
            _reset(lr, row, src, place)
            got = _run_cuts(lr, row, src, [T_IN], ratio)
            assert got["bvh"].shape[0] == N == len(want["k"])
            what = f"{name} {ratio[0]}/{ratio[1]} {order} placed={place is not None}: "
            left_out, signed = plain._compare(got, want, what)
            print(f"{what}{N} frames, {left_out:.1%} left out by the Euler rule, {signed:.1%} of the tracks compared with their sign")
            assert left_out <= LEFT_OUT_CAP and left_out == rf.left_out(want)


# ----------------------------------------------------------------------------- 2. cuts, bit for bit
@pytest.mark.parametrize("name", ["tree", "rig"])
def test_cuts_do_not_change_a_bit(name):
    """at every ratio: one final record of 48 frames, forty-eight records of 1 frame and a final record WITHOUT a frame, and
    5 + 1 + 14 + 28 with final on the last give identical outputs and identical state (the ring included); the total is
    n_out(48); the record without a frame emits the tail, n_out(48) - nf(48) frames"""
    parents, seq, x = SKELETONS[name], plain._seq(name), _case(name)
    src = plain._pose_rows(x)
    lr = _head(3, parents, seq)
    for ratio in rf.RATIOS:
        H = lr.table(*ratio)["half"]
        runs = []
        for row, cuts in ((0, [48]), (1, [1] * 48 + [0]), (2, [5, 1, 14, 28])):
            _reset(lr, row, src, fo.PLACE)
            runs.append((_run_cuts(lr, row, src, cuts, ratio), _row_state(lr, row)))
        assert runs[0][0]["bvh"].shape[0] == ro.n_out(T_IN, *ratio) > rf.nf(T_IN, *ratio, H)
        for got, state in runs[1:]:
            _same_bits(got, runs[0][0], (name, ratio))
            assert state.tobytes() == runs[0][1].tobytes(), ratio
        # the ring: the last 2 max_half input frames, raw, frame i in slot i mod 2 max_half
        J = len(parents)
        ring = runs[0][1][120 + (4 + 8 * J) * 4:].view(np.float32).reshape(2 * MAX_HALF, 7 + 9 * J)
        for i in range(T_IN - 2 * MAX_HALF, T_IN):
            want = np.concatenate([x["rpos"][i], x["rrot"][i], x["lpos"][i].reshape(-1), x["ltxy"][i].reshape(-1)])
            assert ring[i % (2 * MAX_HALF)].tobytes() == want.tobytes(), (ratio, i)


def test_a_final_record_without_a_frame_emits_the_tail():
    """24 from 60 on the tree: 48 frames in running records of 20 + 28 emit nf(48) = 16 frames, then a record with count = 0
    marked final emits the other 3; a stream that never got a frame closes with nothing"""
    parents, seq, x = SKELETONS["tree"], fo.TREE_SEQ, _case("tree")
    src = plain._pose_rows(x)
    lr = _head(2, parents, seq)
    _reset(lr, 0, src, None)
    _reset(lr, 1, src, None)
    whole = _run_cuts(lr, 0, src, [T_IN], (2, 5))
    running = _run_cuts(lr, 1, src, [20, 28], (2, 5), final=False)
    assert running["bvh"].shape[0] == rf.nf(T_IN, 2, 5, 10) == 16
    tail = _run_cuts(lr, 1, src, [0], (2, 5), n_in=T_IN)
    assert tail["bvh"].shape[0] == 3
    _same_bits(live.frames_cat([running, tail]), whole, "tail")
    _reset(lr, 1, src, None)
    assert _run_cuts(lr, 1, src, [0], (2, 5))["bvh"].shape[0] == 0


# ----------------------------------------------------------------------------- 3. rows, bit for bit
def test_64_records_in_one_launch_equal_each_row_alone():
    """64 rows of the tree, four calls: input counts mixed over 0, 1 and 5, ratios mixed over the list, filtered and half = 0
    rows mixed, the last call final for the filtered rows, the records on the device, against the same rows one by one on a
    second state: outputs and states identical (records that emit nothing included: their frames enter the ring), rows that are
    absent from a call keep their state, guards behind every destination"""
    parents, seq = SKELETONS["tree"], fo.TREE_SEQ
    x = fo.inputs(5, 20, 5)
    src = plain._pose_rows(x)
    both = [_head(64, parents, seq, max_frames=20) for _ in range(2)]
    for lr in both:
        for r in range(64):
            _reset(lr, r, src, fo.PLACE if r % 2 else None)
    together, alone = both
    rng = np.random.default_rng(11)
    ratios = [rf.RATIOS[r % len(rf.RATIOS)] for r in range(64)]
    filtered = [r % 4 != 3 for r in range(64)]
    halves = [_half_of(together, ratios[r], filtered[r]) for r in range(64)]
    done, emitted, silent, tails = [0] * 64, 0, 0, 0
    for call in range(4):
        final = call == 3
        counts = [int(rng.choice([0, 1, 5])) for _ in range(64)]
        counts[7] = counts[8] = 0
        absent = [r for r in range(64) if r % 9 == 4]                       # not in the call at all
        rows = [r for r in range(64) if r not in absent]
        before = {r: _row_state(together, r) for r in absent + [7, 8]}     # (8 is filtered: the final record of a stream without a frame emits nothing)
        recs, outs = (capi.RefilterRow * len(rows))(), []
        for q, r in zip(recs, rows):
            n = rf.emitted(done[r] + counts[r], *ratios[r], halves[r][0], final) - rf.emitted(done[r], *ratios[r], halves[r][0], False)
            outs.append(plain._Out(together, n))
            assert _record(q, r, src, done[r], counts[r], outs[-1], ratios[r], done[r], *halves[r], final) == n
        dev = lp._to_device(recs)
        ops.live_frames_refiltered(together, recs, len(rows), dev.data_ptr())
        for r, out in zip(rows, outs):
            assert out.guards_ok(), r
            if counts[r] or out.count:
                want = _run_cuts(alone, r, tuple(t[done[r]:] for t in src), [counts[r]], ratios[r], filtered[r], final, n_in=done[r])
                _same_bits(out.host(), want, (call, r))
                assert _row_state(together, r).tobytes() == _row_state(alone, r).tobytes(), (call, r)
                emitted, silent = emitted + out.count, silent + (out.count == 0)
                tails += final and counts[r] == 0
            done[r] += counts[r]
        for r, state in before.items():
            assert _row_state(together, r).tobytes() == state.tobytes(), (call, r)
    assert max(done) >= 10 and done[7] == 0 and emitted > 100 and silent >= 10 and tails >= 3


def test_unfiltered_rows_are_the_retiming_heads_bit_for_bit():
    """half = 0 records at the nine ratios of the unfiltered head's tests, in cuts of 5 + 1 + 14 + 28, against
    zeggs_live_frames_retimed in one record of 48: every output is the same bits, and so is the state the two share (placement,
    flags, the quaternions last emitted); `final` is ignored"""
    parents, seq, x = SKELETONS["rig"], plain._seq("rig"), _case("rig")
    src = plain._pose_rows(x)
    lr = _head(2, parents, seq)
    lt = ops.LiveRetime(2, parents, T_IN, ALL, "zyx", seq, DEV)
    for ratio in ro.RATIOS:
        _reset(lr, 1, src, fo.PLACE)
        unfiltered._reset(lt, 1, src, fo.PLACE)
        got = _run_cuts(lr, 1, src, [5, 1, 14, 28], ratio, filtered=False, final=True)
        want = unfiltered._run_cuts(lt, 1, src, [T_IN], ratio)
        _same_bits(got, want, ratio)
        shared = 120 + (4 + 8 * len(parents)) * 4
        assert _row_state(lr, 1)[:shared].tobytes() == unfiltered._row_state(lt, 1)[:shared].tobytes(), ratio


# ----------------------------------------------------------------------------- 4. the tone
def test_a_20_hz_tone_does_not_reach_24_frames_a_second():
    """tests/test_live_refilter_cpu.py::test_tones_at_24_frames_a_second through the kernel: joint 3 of the tree turns by
    1e-3 sin(2 pi 20 k / 60) rad, 96 frames in records of 48; over the frames whose taps lie inside the stream the row without the
    filter shows the 4 Hz alias at >= 0.9 of the input amplitude, the filtered row at <= 0.01 of it; a 3 Hz tone keeps >= 0.99"""
    parents, seq = SKELETONS["tree"], fo.TREE_SEQ
    lr = _head(2, parents, seq)
    T, H = 96, 10
    keep = rf.interior(ro.n_out(T, 2, 5), T, 2, 5, H)
    got = {}
    for f in (20, 3):
        x, ang = rf.tone_inputs(T, f, J=5, joint=3)
        src = plain._pose_rows(x)
        for row, filtered in ((0, True), (1, False)):
            _reset(lr, row, src, None)
            o = _run_cuts(lr, row, src, [48, 48], (2, 5), filtered)
            assert o["lrot"].shape[0] == ro.n_out(T, 2, 5)
            got[f, filtered] = np.abs(rf.tone_angle(o["lrot"][:, 3])[keep]).max() / np.abs(ang).max()
            rest = np.delete(o["lrot"], 3, axis=1)
            assert np.abs(rest - np.array([1.0, 0.0, 0.0, 0.0], np.float32)).max() <= 2.0 ** -23          # the other joints stay at rest
    print({k: float(v) for k, v in got.items()})
    assert got[20, False] >= 0.9 and got[20, True] <= 0.01 and 0.99 <= got[3, True] <= 1.01


# ----------------------------------------------------------------------------- 5. the server
FRAMES = dict(plain.FRAMES, text=True)
NSAMP = 16000                    # 1 s: 60 frames


def test_server_hands_out_filtered_frames():
    """three streams on a server of 3 rows, tick 4, retime=dict(max_rate=120, filter=True, min_rate=24): 24 frames a second
    (placed; filtered by default), 120 (filtered by default) and the server's own rate with filtered=True (the jitter filter),
    text=True; and the same three on a server without `filter`.  Per stream: a part holds nf(n1) - nf(n0) frames for the input
    frames it brings, close() adds the tail, "frame0" is contiguous and the stream ends with n_out of all its frames -- the
    count of the unfiltered server; the frames equal, bit for bit, the kernel run on the stream's own returned pose / rpos / rrot
    rows in ANOTHER cut (records of 20 on a fresh state, final on the last); "text" is format_rows of "bvh"; frame_delay is H;
    launches_per_step is the unfiltered server's"""
    conf = dict(max_rate=120, filter=True, min_rate=24)
    srv = lp._server(3, 4, frames=FRAMES, retime=conf)
    ref = lp._server(3, 4, frames=FRAMES, retime=dict(max_rate=120))
    assert isinstance(srv._fr, ops.LiveRefilter) and srv._fr.max_half == 10 and type(ref._fr) is ops.LiveRetime
    rates, ratios, halves = [24, 120, None], [(2, 5), (2, 1), (1, 1)], [10, 4, 4]
    places = [fo.PLACE, None, None]
    parts = {}
    for server, flt in ((srv, [None, None, True]), (ref, [None, None, None])):
        sids = [server.open(lp._first(3 + r % 2), lp._style(70 + r), frame_rate=rate, filtered=f,
                            **({} if p is None else dict(start_position=p[0], start_rotation=p[1])))
                for r, (rate, p, f) in enumerate(zip(rates, places, flt))]
        if server is srv:
            assert [server.frame_delay(s) for s in sids] == [(H, H / 60.0) for H in halves]
        else:
            assert [server.frame_delay(s) for s in sids] == [(0, 0.0)] * 3
        wavs = {sid: lp._wav(NSAMP - 1600 * (r % 3), 60 + r) for r, sid in enumerate(sids)}
        parts[server] = (sids, plain._serve(server, wavs, 1600, True), wavs)
    assert srv.stats["launches_per_step"] == ref.stats["launches_per_step"] == 11 + 3
    lr = ops.LiveRefilter(1, synth.PARENTS, 20, 10, None, ALL, "zyx", None, DEV)
    sids, got, wavs = parts[srv]
    for r, sid in enumerate(sids):
        ratio, H = ratios[r], halves[r]
        n_in = m = 0
        live_parts = [p for p in got[sid] if p]
        for i, p in enumerate(live_parts):
            f = p["frames"]
            n_in += p["pose"].shape[0]
            want = rf.emitted(n_in, *ratio, H, i == len(live_parts) - 1)
            assert f["frame0"] == m and f["bvh"].shape[0] == want - m, (r, n_in)
            assert all(f[k].shape[0] == f["bvh"].shape[0] for k in KEYS) and isinstance(f["text"], bytes)
            assert f["text"] == (anim.format_rows(np.ascontiguousarray(f["bvh"])) if f["bvh"].shape[0] else b"")
            m += f["bvh"].shape[0]
        T = audio.n_anim_frames(wavs[sid].size)
        assert n_in == T and m == ro.n_out(T, *ratio)
        w = unfiltered._whole(got[sid])
        assert w["pose"].shape[0] == T and w["frames"]["frame0"] == 0
        # the unfiltered server hands out as many frames
        rs, rgot, _ = parts[ref]
        assert unfiltered._whole(rgot[rs[r]])["frames"]["bvh"].shape[0] == m
        # the kernel on the stream's own rows, another cut
        src = tuple(torch.as_tensor(w[k], device=DEV) for k in lp.KEYS)
        _reset(lr, 0, src, places[r])
        again = _run_cuts(lr, 0, src, [20] * (T // 20) + ([T % 20] if T % 20 else []), ratio)
        _same_bits(w["frames"], again, r)


def test_a_server_without_filter_returns_what_it_returned():
    """LiveServer(frames=..., retime=dict(max_rate=120)) with and without filter=None / False, same streams at 30 and 90: the
    unfiltered head's state and records, and where the servers decoded the same bits their frames are the same bits; each
    server's frames are zeggs_live_frames_retimed on its own rows; open(filtered=True) is refused naming both rates, and
    open(filtered=False) on a server WITH the filter is the unfiltered head's frames bit for bit"""
    got = []
    for kw in (dict(max_rate=120), dict(max_rate=120, filter=None), dict(max_rate=120, filter=True)):
        srv = lp._server(2, 4, frames=plain.FRAMES, retime=kw)
        with_filter = bool(kw.get("filter"))
        assert (type(srv._fr) is ops.LiveRefilter) == with_filter and (type(srv._fr) is ops.LiveRetime) != with_filter
        assert isinstance(srv._fr_stage.recs[0], ops.RefilterRow if with_filter else ops.RetimeRow) and ("filter" in srv.retime_conf) == with_filter
        if not with_filter:
            with pytest.raises(ValueError, match="filtered=True at frame_rate 30 .* 60.0 frames per second: the filter stage is off"):
                srv.open(lp._first(3), lp._style(77), frame_rate=30, filtered=True)
        sids = [srv.open(lp._first(3), lp._style(75), frame_rate=30, filtered=False if with_filter else None),
                srv.open(lp._first(4), lp._style(76), frame_rate=90, filtered=False if with_filter else None, start_position=fo.PLACE[0],
                         start_rotation=fo.PLACE[1])]
        assert all(srv.frame_delay(s) == (0, 0.0) for s in sids)
        parts = plain._serve(srv, {sid: lp._wav(NSAMP // 2, 60 + i) for i, sid in enumerate(sids)}, 1600, True)
        assert srv.stats["launches_per_step"] == 11
        got.append([unfiltered._whole(parts[sid]) for sid in sids])
    lt = ops.LiveRetime(1, synth.PARENTS, 20, ALL, "zyx", None, DEV)
    for ws in got:
        for w, place, ratio in zip(ws, (None, fo.PLACE), ((1, 2), (3, 2))):
            src = tuple(torch.as_tensor(w[k], device=DEV) for k in lp.KEYS)
            T = w["pose"].shape[0]
            unfiltered._reset(lt, 0, src, place)
            again = unfiltered._run_cuts(lt, 0, src, [20] * (T // 20) + ([T % 20] if T % 20 else []), ratio)
            _same_bits(w["frames"], again, "own rows")
    for other in got[1:]:
        for wa, wb in zip(got[0], other):
            if all(np.array_equal(wa[k], wb[k]) for k in lp.KEYS):
                _same_bits(wa["frames"], wb["frames"], "two servers")
