"""Live serving at other encoder widths, at 64 rows and on tiny streams: the incremental speech encoder (csrc/live.hip:
live_speech_k) against oracle.nets.speech_encoder in float64 directly, and zeggs.live.LiveServer against the offline rollout at
its row limit, across batch-tile edges, on streams shorter than one flush and at another tick.

Why: F, H, O, KW and the ring depth are free in the C ABI (live_dims_ok), but tests/test_gpu_live.py runs the kernel at (81, 64,
64, 31) with three rows only, against the float32 offline encoder; the server had run at 1, 2, 3 and 5 rows, tick 3 and 4, and no
stream shorter than 71 frames.

1. The kernel.  helpers.LIVE_KERNEL_CASES names (F, H, O, KW, rows), helpers.live_schedule the seeded bursts of each (what they
   contain is asserted on the host by tests/test_live_encoder_oracle_cpu.py, which also shows that the float32 restatement of the
   scheme keeps a quarter of the bound and that six plausible mistakes each miss it by >= 10x).  One launch per burst; every frame
   of every row against the float64 whole-row oracle by helpers.relerr, bound helpers.SPEECH_OUT_BOUND = 1e-5 (the offline
   encoder's).  Each launch also asserts: the output block beyond n_out is zero, the ring of a row that received no frames is
   bit-unchanged, the NaN guard rows around `ring` and `out` are untouched.
   Refusals: every check of live_dims_ok (at zeggs_speech_encoder_live_prepare and at the launch entry) and of the per-row loop of
   zeggs_speech_encoder_live, matched on its message, with `ring` and `out` bit-identical afterwards.  The accepted side of each
   limit is in the cases (R = 64, the 64 144-byte LDS carve, n_new = D, feat_off + n_new = feat_ld, n_out = out_ld, a tap at the
   newest frame, a tap at the oldest frame of the ring) or in test_limits_accepted (R = 1, D = KW).

2. The server.  The yardstick of tests/test_gpu_live.py (helpers.live_offline / live_bound: 1e-4 where the weight-stationary
   sweep ran, 5e-5 on the stage launches, and which ran is asserted).

Measured on an MI355X (the whole file: 3 s, its longest test 0.6 s; the server figures are the larger of two runs -- run to run they
move by up to a factor of two with the order of the decoder's float atomics):
  kernel case (F, H, O, KW)      rows  launches  D    worst relerr vs float64   bound
  (81, 64, 64, 31)               64    21        53   6.0e-7                    1e-5
  (81, 128, 32, 31)              3     14        47   5.8e-7                    1e-5
  (81, 32, 128, 31)              3     18        53   3.5e-7                    1e-5
  (20, 512, 64, 3)               3     14        11   4.0e-7                    1e-5
  (20, 16, 512, 5)               3     21        11   2.8e-7                    1e-5
  (3, 4, 4, 1)                   3     11        129  1.1e-7                    1e-5
  (81, 256, 16, 29)              3     14        61   1.4e-6                    1e-5
  (81, 64, 64, 31), D = KW       1     1         31   4.6e-7                    1e-5
  (the float32 restatement on the host: 1e-7 .. 6e-7, tests/test_live_encoder_oracle_cpu.py)
  server case                                          worst |live - offline|   decoder path   bound
  rows = 64, tick = 4, 72 streams, 28 ticks, 40 steps  1.9e-6                   sweep          1e-4
  rows = 17, last row alone for 6 steps                9.5e-7                   sweep          1e-4
  rows = 33, last row alone for 6 steps                1.9e-6                   sweep          1e-4
  short streams of 5, 16, 20, 21 frames (close alone)  4.8e-7                   B = 1 entry    5e-5
  short streams of 24, 35 frames (steps, then close)   3.6e-7                   sweep          1e-4
  the long stream beside them                          5.4e-7                   sweep          1e-4
  rows = 3, tick = 9                                   5.1e-7                   sweep          5e-5
  close(): 5, 16 and 20 frames leave in one flush call, 21 in two; 24 and 35 had stepped in drain() (kd = 5 / 17) and leave in one.

Found: no fault in csrc/live.hip, zeggs/live.py or zeggs/ops.py -- every case passed on its first run on the device, tick = 9
included (no component refuses it).  One fact about the inputs: a signal whose last animation frame lies outside the hull of its
STFT frames -- 5200 samples are 20 frames but 26 STFT frames, t_19 = 25.33 > 25 -- has NaN mel rows at its end (griddata's fill
value in the reference, csrc/mel.hip mel_resample_elem), so both the offline rollout and the server return NaN frames for it; the
short streams here are 20 samples longer than the least that rounds to their frame count, which keeps the last frame inside.
"""
import numpy as np
import pytest
import torch

import helpers as H
from zeggs import audio, ops

pytestmark = pytest.mark.gpu
DEV = H.LIVE_DEV
CASES = H.LIVE_KERNEL_CASES
NAN = float("nan")


# ----------------------------------------------------------------------------- 1. the kernel against float64
def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(R, n, w):
    """[R, n, w] zeros between two guard rows of NaN -> (whole, inner view)"""
    big = torch.full((R + 2, n, w), NAN, device=DEV)
    big[1:-1] = 0.0
    return big, big[1:-1]


def _guards_intact(big):
    """both guard rows still hold the bits they were filled with"""
    want = _bits(torch.full_like(big[0], NAN))
    return torch.equal(_bits(big[0]), want) and torch.equal(_bits(big[-1]), want)


def _live_speech(case, data, R=None, D=None, feat_ld=None, out_ld=None):
    s = data["sched"]
    net = data["net"]
    for m in (net.layer0, net.layer1, net.layer2):
        m.to(DEV)
    return ops.LiveSpeech(net, data["mean"].to(DEV), data["std"].to(DEV), R or case["R"], D or s["D"], feat_ld or s["feat_ld"],
                          out_ld or s["out_ld"])


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_incremental_encoder_vs_float64(case):
    data = H.live_case_data(case)
    s, R, O = data["sched"], case["R"], case["O"]
    enc = _live_speech(case, data)
    ring_big, ring = _guarded(R, s["D"], case["H"])
    out_big, out = _guarded(R, s["out_ld"], O)
    col = torch.arange(s["out_ld"], device=DEV)[None, :]
    got = [[] for _ in range(R)]
    for c, recs in enumerate(s["calls"]):
        blk = H.live_feat_block(data, c).to(DEV)
        out.fill_(NAN)
        prev = ring.clone()
        ops.speech_encoder_live(enc, [ops.LiveRow(*rec, 0) for rec in recs], blk, ring, out)
        n_out = torch.tensor([rec[4] for rec in recs], device=DEV)[:, None]
        rest = (col >= n_out)[:, :, None].expand_as(out)
        assert bool((out[rest] == 0).all()), f"call {c}: the block beyond n_out is not zero"
        assert bool(torch.isfinite(out[~rest]).all()), f"call {c}"
        still = [r for r, rec in enumerate(recs) if rec[3] == 0]
        assert torch.equal(_bits(ring[still]), _bits(prev[still])), f"call {c}: the ring of a row without new frames changed"
        assert _guards_intact(ring_big) and _guards_intact(out_big), f"call {c}: a guard row was written"
        for r, rec in enumerate(recs):
            if rec[4]:
                got[r].append(out[r, :rec[4]].clone())
    errs = []
    for r, n in enumerate(s["lens"]):
        o = torch.cat(got[r])
        assert tuple(o.shape) == tuple(data["ref"][r].shape) == (n, O)
        errs.append(H.relerr(o, data["ref"][r]))
    worst = max(range(R), key=lambda r: errs[r])
    print(f"{case['id']}: worst relerr vs float64 {errs[worst]:.2e} (row {worst}, {s['lens'][worst]} frames; {len(s['calls'])} launches, "
          f"D = {s['D']})")
    assert errs[worst] <= H.SPEECH_OUT_BOUND, (worst, errs[worst])


BASE = dict(id="refusals", F=81, H=64, O=64, KW=31, R=3, bs=23, long=150)
BASE_D, BASE_FEAT_LD, BASE_OUT_LD = 53, 60, 38


def _filled(*shape, seed):
    return torch.randn(*shape, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))


def _refused(enc, d, recs, message):
    """a launch with dimensions d and records recs is refused with `message`; ring and out keep their bits"""
    feats, ring, out = _filled(d.R, d.feat_ld, d.F, seed=1), _filled(d.R, d.D, d.H, seed=2), _filled(d.R, d.out_ld, d.O, seed=3)
    ring0, out0 = ring.clone(), out.clone()
    old = enc.d
    enc.d = d
    try:
        with pytest.raises(RuntimeError, match=message):
            ops.speech_encoder_live(enc, [ops.LiveRow(*rec, 0) for rec in recs], feats, ring, out)
    finally:
        enc.d = old
    torch.cuda.synchronize()
    assert torch.equal(_bits(ring), _bits(ring0)) and torch.equal(_bits(out), _bits(out0)), message


# (R, F, H, O, KW, D): one refusal per check of live_dims_ok
DIMS_REFUSED = [((0, 81, 64, 64, 31, 53), "0 rows"), ((65, 81, 64, 64, 31, 53), "65 rows"),
                ((3, 81, 64, 64, 30, 53), "even kernel width 30"), ((3, 81, 12, 64, 31, 53), "H = 12 / O = 64 must be multiples of 4"),
                ((3, 81, 64, 12, 31, 53), "H = 64 / O = 12 must be multiples of 4"), ((3, 81, 64, 64, 31, 30), "ring of 30 frames under a kernel of 31"),
                ((3,) + H.LIVE_LDS_REFUSED + (53,), "66192 bytes of LDS")]


@pytest.mark.parametrize("dims,message", DIMS_REFUSED, ids=[m for _, m in DIMS_REFUSED])
def test_dimensions_refused(dims, message):
    """at the launch entry (a LiveSpeech of good dimensions, the refused ones in the call) and at prepare"""
    R, F, Hd, O, KW, D = dims
    data = H.live_case_data(CASES[0])
    enc = _live_speech(BASE, data, R=3, D=BASE_D, feat_ld=BASE_FEAT_LD, out_ld=BASE_OUT_LD)
    idle = (0, 0, -1, 0, 0, 0)
    if R >= 1:
        _refused(enc, ops.LiveDims(R, F, Hd, O, KW, D, BASE_FEAT_LD, BASE_OUT_LD), [(0, 0, -1, 5, 0, 0)] + [idle] * (R - 1), message)
    net = H.live_case_nets(dict(F=F, H=Hd, O=O, KW=KW))
    for m in (net.layer0, net.layer1, net.layer2):
        m.to(DEV)
    with pytest.raises(RuntimeError, match=message):
        ops.LiveSpeech(net, torch.zeros(F, device=DEV), torch.ones(F, device=DEV), R, D, BASE_FEAT_LD, BASE_OUT_LD)


D_ = BASE_D
ROWS_REFUSED = [((0, 0, -1, -1, 0, 0), "row 1: negative count"), ((0, 0, -1, 0, -1, 0), "row 1: negative count"),
                ((-1, 0, -1, 0, 0, 0), "row 1: negative count"), ((0, 0, -1, 0, 0, -1), "row 1: negative count"),
                ((0, 0, -1, D_ + 1, 0, 0), f"row 1: {D_ + 1} new frames at 0"),                       # n_new = D + 1 (feat_ld = 60 admits it)
                ((0, 0, -1, 10, 0, BASE_FEAT_LD - 9), f"row 1: 10 new frames at {BASE_FEAT_LD - 9}"),  # feat_off + n_new = feat_ld + 1
                ((100, 60, -1, 0, BASE_OUT_LD + 1, 0), f"row 1: {BASE_OUT_LD + 1} frames into {BASE_OUT_LD} output rows"),
                ((0, 0, 5, 5, 0, 0), "row 1 ended at frame 5 but 5 frames arrived"),
                ((0, 3, 5, 6, 4, 0), "row 1: frame 6 is past the last one"),
                ((0, 0, -1, 0, 1, 0), "row 1: nothing to read"), ((5, -1, -1, 0, 1, 0), "row 1: nothing to read"),
                ((0, 0, -1, 10, 1, 0), "row 1: frame 0 needs frame 15, 10 are in the ring"),
                ((100, 40, -1, 5, 1, 0), "row 1: frame 25 has left the ring of 53")]


@pytest.mark.parametrize("rec,message", ROWS_REFUSED, ids=[f"{i}-{m.split(': ')[-1][:24]}" for i, (_, m) in enumerate(ROWS_REFUSED)])
def test_rows_refused(rec, message):
    """the bad record is row 1's; rows 0 and 2 carry good work that must not have run"""
    data = H.live_case_data(CASES[0])
    enc = _live_speech(BASE, data, R=3, D=BASE_D, feat_ld=BASE_FEAT_LD, out_ld=BASE_OUT_LD)
    good = (0, 0, 19, 20, 20, 1)
    _refused(enc, enc.d, [good, rec, good], message.replace("(", r"\(").replace(")", r"\)"))


def test_limits_accepted():
    """R = 1 with D = KW, the least of both: a row of KW frames arrives and ends in one launch, against float64"""
    case = CASES[0]
    data = H.live_case_data(case)
    KW = case["KW"]
    r = max(range(case["R"]), key=lambda i: data["sched"]["lens"][i])
    enc = _live_speech(case, data, R=1, D=KW, feat_ld=KW, out_ld=KW)
    ring, out = torch.zeros(1, KW, case["H"], device=DEV), torch.full((1, KW, case["O"]), NAN, device=DEV)
    ops.speech_encoder_live(enc, [ops.LiveRow(0, 0, KW - 1, KW, KW, 0, 0)], data["feats"][r][None, :KW].to(DEV).contiguous(), ring, out)
    from oracle import nets as onets
    w = {k: v.detach().cpu().double() for k, v in H.live_case_weights(data["net"]).items()}
    x = (data["feats"][r][:KW].double() - data["mean"].double()) / data["std"].double()
    with torch.no_grad():
        ref = onets.speech_encoder(w, x[None])[0]
    e = H.relerr(out[0], ref)
    print(f"R = 1, D = KW = {KW}: {e:.2e}")
    assert e <= H.SPEECH_OUT_BOUND, e


# ----------------------------------------------------------------------------- 2. LiveServer at its limits
def _stream(i):
    """stream i of this file: (samples, wav seed, first-pose seed, style seed); 0.9 .. 1.6 s, all lengths different"""
    return (14400 + ((i * 29) % 72) * 155 + i, 100 + i, 3 + i, 300 + i)


def _open(srv, i):
    v = _stream(i)
    return srv.open(H.live_first(v[2]), H.live_style(v[3]))


def _check_all(srv, parts, ids, bound, label):
    worst = 0.0
    for i in ids:
        v = _stream(i)
        got = H.live_cat(parts[i])
        assert got["pose"].shape[0] == audio.n_anim_frames(v[0])
        e = max(H.live_err(got, H.live_offline_cached(*v)).values())
        worst = max(worst, e)
        assert e <= bound, (label, i, e, bound)
    print(f"{label}: worst |live - offline| over {len(ids)} streams {worst:.2e} (bound {bound:.0e}, path {ops.batch_last_path()})")


def _round(srv, live, pos, parts, only=None):
    """one tick: 1600 samples to every open stream that has some left (only: to these streams alone), the others that ran out are
    closed; then drain() -> the ids closed"""
    chunks, closed = {}, []
    for i, sid in list(live.items()):
        if only is not None and i not in only:
            continue
        w = H.live_wav(*_stream(i)[:2])
        if pos[i] < len(w):
            chunks[sid] = w[pos[i]:pos[i] + 1600]
            pos[i] += 1600
        else:
            parts[i].append(srv.close(sid))
            closed.append(i)
            del live[i]
    if chunks:
        srv.push_many(chunks)
    by_sid = {sid: i for i, sid in live.items()}
    out = srv.drain()
    for sid, o in out.items():
        parts[by_sid[sid]].append(o)
    return closed, {by_sid[sid] for sid in out}


def test_sixty_four_rows_and_reuse():
    """64 streams opened before the first push, one push_many of 1600 samples per stream and tick with drain() after each, each
    closed as it runs out; eight further streams open on rows that came free: all 72 equal their own offline rollouts"""
    srv = H.live_server(64, 4)
    live = {i: _open(srv, i) for i in range(64)}
    assert sorted(srv._sids[s] for s in live.values()) == list(range(64))
    with pytest.raises(RuntimeError, match="all 64 rows"):
        _open(srv, 64)
    pos, parts, waiting, freed, reused = {i: 0 for i in range(72)}, {i: [] for i in range(72)}, list(range(64, 72)), [], []
    rounds, full_steps = 0, 0
    while live:
        rows_before = {i: srv._sids[s] for i, s in live.items()}
        closed, stepped = _round(srv, live, pos, parts)
        full_steps += len(stepped) == 64
        freed += [rows_before[i] for i in closed]
        while waiting and len(live) < 64:
            i = waiting.pop(0)
            live[i] = _open(srv, i)
            reused.append(srv._sids[live[i]])
        rounds += 1
        assert rounds < 80
    assert not waiting and len(reused) == 8 and set(reused) <= set(freed)
    assert full_steps >= 3                                  # steps in which all 64 rows committed
    bound = H.live_bound(srv)
    _check_all(srv, parts, range(72), bound, f"rows=64 tick=4, {rounds} ticks, {srv.stats['steps']} steps")


@pytest.mark.parametrize("rows", [17, 33])
def test_last_row_alone_across_a_tile_edge(rows):
    """all rows live for the first steps; then only the last row (the first of a new 16-row batch tile) receives audio for at
    least three steps while the others stay open on filler; then they receive the rest"""
    ids = sorted(range(rows), key=lambda i: _stream(i)[0])          # the longest stream last
    srv = H.live_server(rows, 4)
    live = {i: _open(srv, i) for i in ids}
    assert srv._sids[live[ids[-1]]] == rows - 1
    pos, parts = {i: 0 for i in ids}, {i: [] for i in ids}
    together = 0
    for _ in range(6):
        _, stepped = _round(srv, live, pos, parts)
        together += len(stepped) == rows
    assert together >= 2
    steps0, alone = srv.stats["steps"], 0
    for _ in range(4):
        _, stepped = _round(srv, live, pos, parts, only={ids[-1]})
        assert stepped <= {ids[-1]}
        alone += len(stepped)
    n_alone = srv.stats["steps"] - steps0
    assert n_alone >= 3 and alone and len(live) == rows
    bound = H.live_bound(srv)
    rounds = 0
    while live:
        _round(srv, live, pos, parts)
        rounds += 1
        assert rounds < 40
    _check_all(srv, parts, ids, bound, f"rows={rows} tick=4, last row alone for {n_alone} steps")


def _samples_for(frames):
    """a signal of `frames` animation frames whose last frame lies inside the hull of its STFT frames: (frames - 1) * 4 / 3 <= n // 200.
    (Where it does not -- 5200 samples: 20 frames, 26 STFT frames -- the reference's griddata gives NaN mel rows, and so do the
    offline and the live path here, alike.)"""
    n = int(np.ceil((frames - 0.5) * 16000 / 60)) + 20          # 20 samples above the least that round to `frames`
    assert audio.n_anim_frames(n) == frames and (frames - 1) * 4 / 3 <= n // 200
    return n


SHORT = (5, 16, 20, 21, 24, 35)
FLUSH_CALLS = {5: 1, 16: 1, 20: 1, 21: 2}      # close() with no step before it: rem = frames - 1 <= tick + 15 = 19 is one call


def test_short_streams():
    """streams of 5 .. 35 frames, each pushed in one piece, drained and closed, beside an unrelated long stream in the other row;
    which path close() took is asserted: rem <= tick + 15 frames leave in one encoder + decoder call, more take `tick` first"""
    srv = H.live_server(2, 4)
    lw = H.live_wav(40123, 1)
    long_sid = srv.open(H.live_first(3), H.live_style(1))
    empty = srv.open(H.live_first(4), H.live_style(2))
    assert srv.close(empty) == {}
    calls = []
    inner = srv._encode
    srv._encode = lambda jobs, out_ld: (calls.append(out_ld), inner(jobs, out_ld))[1]
    lparts, lpos, worst = [], 0, 0.0
    for k, frames in enumerate(SHORT):
        srv.push(long_sid, lw[lpos:lpos + 6000])
        lpos += 6000
        lparts.append(srv.drain().get(long_sid))
        n = _samples_for(frames)
        wav, first, style = H.live_wav(n, 50 + k), H.live_first(5 + k), H.live_style(60 + k)
        sid = srv.open(first, style)
        srv.push(sid, wav)
        out = srv.drain()
        lparts.append(out.get(long_sid))
        kd = srv._rows[srv._sids[sid]].kd
        rem, expect = frames - kd, 0
        while rem > 0:
            expect, rem = expect + 1, rem - (rem if rem <= 19 else 4)
        bound = H.live_bound(srv) if out.get(sid) else 5e-5        # (no step: every frame leaves through close(), the B = 1 entry point)
        del calls[:]
        tail = srv.close(sid)
        assert len(calls) == expect, (frames, kd, len(calls), expect)
        if frames in FLUSH_CALLS:
            assert kd == 1 and sid not in out and len(calls) == FLUSH_CALLS[frames], (frames, kd, len(calls))
        e = max(H.live_err(H.live_cat([out.get(sid), tail]), H.live_offline(wav, first, style)).values())
        print(f"{frames} frames: kd = {kd} at close, {len(calls)} flush calls, |live - offline| = {e:.2e}")
        worst = max(worst, e)
        assert e <= bound, (frames, e, bound)
    srv.push(long_sid, lw[lpos:])
    lparts.append(srv.drain().get(long_sid))
    bound = H.live_bound(srv)
    lparts.append(srv.close(long_sid))
    e = max(H.live_err(H.live_cat(lparts), H.live_offline_cached(40123, 1, 3, 1)).values())
    print(f"short streams: worst {worst:.2e}; the long stream beside them {e:.2e} (bound {bound:.0e})")
    assert e <= bound, e


def test_tick_nine():
    """tick = 9 (ring of 40 frames, 25-frame flush, chunks of 10 frames), rows = 3, any chunking, against offline"""
    nsamp, seed = 40123, 1
    wav, ref = H.live_wav(nsamp, seed), H.live_offline_cached(nsamp, seed, 3, seed)
    srv = H.live_server(3, 9)
    assert srv.D == 40 and srv.tail == 24 and srv.T == 10
    sid = srv.open(H.live_first(3), H.live_style(seed))
    rng = np.random.default_rng(99)
    parts, pos = [], 0
    while pos < nsamp:
        n = int(rng.choice([37, 160, 1600, 5000, 16000]))
        srv.push(sid, wav[pos:pos + n])
        pos += n
        parts.append(srv.drain().get(sid))
    parts.append(srv.close(sid))
    got = H.live_cat(parts)
    assert got["pose"].shape[0] == audio.n_anim_frames(nsamp) == ref[0].shape[0]
    assert srv.stats["steps"] >= 3 and srv.stats["uploaded_samples"] == nsamp
    e = H.live_err(got, ref)
    print(f"rows=3 tick=9: {e} (path {ops.batch_last_path()})")
    assert max(e.values()) <= 5e-5, e
