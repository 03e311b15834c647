"""LiveServer(loudness=...): running BS.1770 loudness normalisation per row on the device (include/zeggs_hip_loudness.h,
csrc/live_loudness.hip).  Yardsticks: the float64 oracle of tests/live_loudness_oracle.py for the estimate and the gain (the
margin that makes the comparison decidable is asserted in tests/test_live_loudness_cpu.py), a plain server fed pre-scaled
samples for the features (bitwise), the offline device path for the final estimate, and the server against itself for
everything that must not depend on how a stream is cut into pushes, on push() versus push_many(), or on the other rows."""
import functools
import math
import struct

import numpy as np
import pytest
import torch

import live_loudness_oracle as oracle_ll
from test_gpu_live_push import DEV, KEYS, _bits, _bound, _cat, _first, _server, _style
from zeggs import audio, live, ops

pytestmark = pytest.mark.gpu
FS, HOP, BLK = 16000, 1600, 6400
CAP = 16384                      # windows compact during every test below


@functools.lru_cache(maxsize=None)
def _signals():
    return oracle_ll.signals(FS)


@functools.lru_cache(maxsize=None)
def _trace(name, horizon, n=None, gain0=1.0, hold=()):
    x = _signals()[name]
    return oracle_ll.running_loudness(x if n is None else x[:n], FS, horizon=horizon, gain0=gain0, hold_blocks=hold)


def _loud_server(rows, tick=4, horizon=60.0, **kw):
    return _server(rows, tick, window_capacity=CAP, loudness=dict(horizon=horizon), **kw)


def _f32_bits(v):
    return struct.pack("<f", v)


def _check_state(got, want, where):
    """a row's loudness() against the oracle's state_after: counts equal, the estimate within 2e-5 dB where there is one and NaN
    where there is none, held where the oracle holds, the gain within rtol 3e-6"""
    assert (got["blocks"], got["gated"], got["held"]) == (want["blocks"], want["gated"], want["held"]), (where, got, want)
    if math.isnan(want["lufs"]):
        assert math.isnan(got["lufs"]), (where, got, want)
    else:
        assert abs(got["lufs"] - want["lufs"]) <= 2e-5, (where, got, want)
    assert abs(got["gain"] - want["gain"]) <= 3e-6 * want["gain"], (where, got, want)


class _Feats:
    """every feature row a server computes for a row, collected push by push (a drain() between two pushes only moves the ring
    counter: the rows stay where they are until the next push compacts the block)"""

    def __init__(self, srv, rows):
        self.srv, self.seen, self.parts = srv, {r: 0 for r in rows}, {r: [] for r in rows}

    def grab(self):
        for r in self.seen:
            w = self.srv._rows[r]
            if w is not None and w.n_feat > self.seen[r]:
                self.parts[r].append(self.srv.feats[r, self.seen[r] - w.fbase:w.n_feat - w.fbase].clone())
                self.seen[r] = w.n_feat

    def restart(self, r):
        self.seen[r], self.parts[r] = 0, []

    def all(self, r):
        return torch.cat(self.parts[r]) if self.parts[r] else torch.zeros(0, 81, device=DEV)


def _window(srv, r):
    w = srv._rows[r]
    return w.base, srv.window[r][:w.n - w.base].clone()


# ----------------------------------------------------------------------------- 1. the trace against the oracle
@pytest.mark.parametrize("horizon", [60.0, 2.0])
@pytest.mark.parametrize("name", ["speech", "gap", "quiet", "step"])
def test_running_loudness_trace_vs_oracle(name, horizon):
    """one row, pushed hop by hop, loudness() read after every push: blocks and gated equal to the oracle's, lufs within 2e-5
    (NaN / held exactly where the oracle has no estimate), gain within rtol 3e-6"""
    x, tr = _signals()[name], _trace(name, horizon)
    srv = _loud_server(1, horizon=horizon)
    sid = srv.open(_first(3), _style(70))
    _check_state(srv.loudness(sid), oracle_ll.state_after(tr, 0), (name, horizon, 0))
    worst, n = 0.0, 0
    while n < x.size:
        m = BLK if n == 0 else HOP
        srv.push(sid, x[n:n + m])
        n += m
        got, want = srv.loudness(sid), oracle_ll.state_after(tr, n)
        _check_state(got, want, (name, horizon, n))
        if not math.isnan(want["lufs"]):
            worst = max(worst, abs(got["lufs"] - want["lufs"]))
        srv.drain()
    print(f"{name} horizon {horizon}: {want['blocks']} blocks, max |lufs - oracle| = {worst:.2e} dB, final gain {got['gain']:.6f}")
    assert want["blocks"] == (x.size - BLK) // HOP + 1 and srv.stats["window_capacity"] == [CAP] and srv._rows[0].base > 0


# ----------------------------------------------------------------------------- 2. the features are those of pre-scaled samples
@pytest.mark.parametrize("name,horizon", [("speech", 60.0), ("gap", 2.0), ("quiet", 2.0), ("step", 2.0), ("step", 60.0)])
def test_features_are_those_of_prescaled_samples(name, horizon):
    """pushes of 1000 samples, so every gain switch falls INSIDE a push: a plain server (loudness=None) fed x * g -- g the float32
    gains the device reported, each from the oracle's hi_j on -- has bitwise the same features, feature count and window"""
    x, tr = _signals()[name], _trace(name, horizon)
    srv = _loud_server(1, horizon=horizon)
    sid = srv.open(_first(3), _style(71))
    fa = _Feats(srv, [0])
    gains = np.ones(x.size, np.float32)
    done = 0
    for n in range(0, x.size, 1000):
        srv.push(sid, x[n:n + 1000])
        fa.grab()
        got = srv.loudness(sid)
        assert got["blocks"] - done in (0, 1)
        if got["blocks"] > done:
            done = got["blocks"]
            gains[tr["blocks"][done - 1]["hi"]:] = np.float32(got["gain"])
        srv.drain()
    assert done == len(tr["blocks"]) and len(set(gains.tolist())) >= (3 if name != "speech" else 2)
    assert any(b["hi"] % 1000 for b in tr["blocks"])
    plain = _server(1, 4, window_capacity=CAP)
    pid = plain.open(_first(3), _style(71))
    fb = _Feats(plain, [0])
    xg = x * gains
    assert xg.dtype == np.float32
    for n in range(0, x.size, 1000):
        plain.push(pid, xg[n:n + 1000])
        fb.grab()
        plain.drain()
    torch.cuda.synchronize()
    assert srv._rows[0].n_feat == plain._rows[0].n_feat > 100 and fa.all(0).shape == fb.all(0).shape
    assert torch.equal(_bits(fa.all(0)), _bits(fb.all(0)))
    (ba, wa), (bb, wb) = _window(srv, 0), _window(plain, 0)
    assert ba == bb > 0 and torch.equal(_bits(wa), _bits(wb))


# ----------------------------------------------------------------------------- 3. nothing depends on the cut
def test_cut_invariance_push_and_push_many():
    """`gap` into four rows in pushes of 160, 1600, 1601 and 5000 samples (the last of what is left); row 1 through push(), the
    others through push_many(), row 2 sitting out every third tick: features and final state (lufs, gain: bits) are equal
    across the rows; push_many enqueues at most six operations unless a buffer grew"""
    x = _signals()["gap"]
    sizes = [160, 1600, 1601, 5000]
    srv = _loud_server(4, horizon=2.0)
    sids = [srv.open(_first(3), _style(72)) for _ in range(4)]
    fe = _Feats(srv, range(4))
    pos, tick, most = [0] * 4, 0, 0
    while min(pos) < x.size:
        many = {}
        for r in (0, 2, 3):
            if pos[r] < x.size and not (r == 2 and tick % 3 == 2):
                many[sids[r]] = x[pos[r]:pos[r] + sizes[r]]
                pos[r] += many[sids[r]].size
        before = (list(srv.stats["window_capacity"]), srv.FC, srv._stage.n_samples)
        srv.push_many(many)
        grew = before != (list(srv.stats["window_capacity"]), srv.FC, srv._stage.n_samples)
        if many:
            assert 1 <= srv.stats["ops_last_push_many"] <= 6 or grew, (tick, srv.stats["ops_last_push_many"])
            most = max(most, 0 if grew else srv.stats["ops_last_push_many"])
        if pos[1] < x.size:
            srv.push(sids[1], x[pos[1]:pos[1] + sizes[1]])
            pos[1] = min(pos[1] + sizes[1], x.size)
        fe.grab()
        srv.drain()
        tick += 1
    torch.cuda.synchronize()
    assert pos == [x.size] * 4 and most == 6
    state = [srv.loudness(s) for s in sids]
    want = oracle_ll.state_after(_trace("gap", 2.0), x.size)
    _check_state(state[0], want, "gap, 160-sample pushes")
    f0 = fe.all(0)
    assert f0.shape[0] == srv._rows[0].n_feat > 400
    for r in (1, 2, 3):
        assert state[r]["blocks"] == state[0]["blocks"] == 81 and state[r]["gated"] == state[0]["gated"] and state[r]["held"] == state[0]["held"]
        assert struct.pack("<d", state[r]["lufs"]) == struct.pack("<d", state[0]["lufs"]), r
        assert _f32_bits(state[r]["gain"]) == _f32_bits(state[0]["gain"]), r
        assert srv._rows[r].n_feat == srv._rows[0].n_feat and torch.equal(_bits(fe.all(r)), _bits(f0)), r


# ----------------------------------------------------------------------------- 4. the offline path's estimate
@pytest.mark.parametrize("name", ["speech", "step"])
def test_final_estimate_is_the_offline_one(name):
    """the whole clip in ONE push (31 / 51 blocks complete inside it, the window grows): with a horizon that covers the clip the
    final estimate is within 2e-5 dB of audio.normalize_loudness_device of the same samples"""
    x = _signals()[name]
    srv = _loud_server(1, horizon=60.0)
    sid = srv.open(_first(3), _style(73))
    srv.push(sid, x)
    got = srv.loudness(sid)
    _, want = audio.normalize_loudness_device(x, FS)
    print(f"{name}: running {got['lufs']:.9f} LUFS, offline {want:.9f}, |diff| {abs(got['lufs'] - want):.2e}")
    assert got["blocks"] == (x.size - BLK) // HOP + 1
    assert abs(got["lufs"] - want) <= 2e-5
    _check_state(got, oracle_ll.state_after(_trace(name, 60.0), x.size), name)


# ----------------------------------------------------------------------------- 5. a fixed gain
def test_fixed_gain_and_release():
    """open(gain=g0) + hold(): the features are bitwise those of a plain server fed ops.scale_copy(x, g0) while the row goes on
    metering; after hold(sid, False) the trace continues as the oracle's with the held span metered"""
    x, g0, n_hold = _signals()["step"], 2.5, BLK + 24 * HOP
    held_blocks = tuple(range(25))
    tr = _trace("step", 2.0, None, g0, held_blocks)
    assert [b["hi"] <= n_hold for b in tr["blocks"]].count(True) == 25
    srv = _loud_server(1, horizon=2.0)
    sid = srv.open(_first(3), _style(74), gain=g0)
    srv.hold(sid)
    fa = _Feats(srv, [0])
    n = 0
    while n < x.size:
        if n == n_hold:
            torch.cuda.synchronize()
            n_feat_held, feats_held = srv._rows[0].n_feat, fa.all(0)
            srv.hold(sid, False)
        m = BLK if n == 0 else HOP
        srv.push(sid, x[n:n + m])
        n += m
        fa.grab()
        got = srv.loudness(sid)
        _check_state(got, oracle_ll.state_after(tr, n), ("step", n))
        if n <= n_hold:
            assert got["gain"] == g0 and (got["held"] or got["blocks"] == 0)
        srv.drain()
    assert got["gain"] != g0 and not got["held"]
    assert {float(b["g"]) for b in tr["blocks"][:25]} == {g0} and tr["blocks"][24]["fresh"]
    plain = _server(1, 4, window_capacity=CAP)
    pid = plain.open(_first(3), _style(74))
    fb = _Feats(plain, [0])
    xs = ops.scale_copy(torch.as_tensor(x[:n_hold], device=DEV), alpha=g0).cpu().numpy()
    n = 0
    while n < n_hold:                           # (the same pushes: one block first, then hops)
        m = BLK if n == 0 else HOP
        plain.push(pid, xs[n:n + m])
        n += m
        fb.grab()
        plain.drain()
    torch.cuda.synchronize()
    assert plain._rows[0].n_feat == n_feat_held > 100 and torch.equal(_bits(fb.all(0)), _bits(feats_held))
    with pytest.raises(ValueError, match="gain needs running loudness"):
        plain.open(_first(3), _style(74), gain=2.0)
    with pytest.raises(RuntimeError, match="running loudness is off"):
        plain.loudness(pid)


# ----------------------------------------------------------------------------- 6. a reused row, and its neighbour
def _stream_rows(srv, plan, fe):
    """plan: {row: (sid, samples)}; hop by hop through push_many until the longest is used up -> {row: [loudness() per push]}"""
    out = {r: [] for r in plan}
    n = 0
    while any(n < x.size for _, x in plan.values()):
        m = BLK if n == 0 else HOP
        srv.push_many({sid: x[n:n + m] for sid, x in plan.values() if n < x.size})
        fe.grab()
        for r, (sid, x) in plan.items():
            if n < x.size:
                out[r].append(srv.loudness(sid))
        srv.drain()
        n += m
    return out


def _same_trace(a, b):
    return len(a) == len(b) and all(
        (p["blocks"], p["gated"], p["held"]) == (q["blocks"], q["gated"], q["held"]) and _f32_bits(p["gain"]) == _f32_bits(q["gain"])
        and struct.pack("<d", p["lufs"]) == struct.pack("<d", q["lufs"]) for p, q in zip(a, b))


def test_row_reuse_and_isolation():
    """row 1 is closed mid-signal and opened again with another signal while row 0 keeps streaming: the reopened row's trace and
    features are bitwise a fresh server's, the neighbour's bitwise those of a server where it streams alone"""
    sig = _signals()
    n1 = BLK + 30 * HOP
    gap_a, gap_b = sig["gap"][:n1], sig["gap"][n1:n1 + BLK + 30 * HOP]
    srv = _loud_server(2, horizon=2.0)
    fe = _Feats(srv, [0, 1])
    s0, s1 = srv.open(_first(3), _style(75)), srv.open(_first(4), _style(76))
    t_first = _stream_rows(srv, {0: (s0, gap_a), 1: (s1, sig["step"][:n1])}, fe)
    assert t_first[1][-1]["blocks"] == 31 and t_first[1][-1]["gain"] != 1.0
    srv.close(s1)
    s1 = srv.open(_first(5), _style(77))
    assert srv._sids[s1] == 1
    fe.restart(1)
    fresh = srv.loudness(s1)
    assert (fresh["blocks"], fresh["gated"], fresh["held"], fresh["gain"]) == (0, 0, False, 1.0) and math.isnan(fresh["lufs"])
    t_second = _stream_rows(srv, {0: (s0, gap_b), 1: (s1, sig["speech"])}, fe)
    # the reopened row against a fresh server
    ref = _loud_server(2, horizon=2.0)
    fr = _Feats(ref, [0])
    t_ref = _stream_rows(ref, {0: (ref.open(_first(5), _style(77)), sig["speech"])}, fr)
    # the neighbour against a server where it streams alone (its second part starts on a hop boundary: same pushes)
    alone = _loud_server(2, horizon=2.0)
    fl = _Feats(alone, [0])
    sa = alone.open(_first(3), _style(75))
    t_alone = _stream_rows(alone, {0: (sa, gap_a)}, fl)[0]
    n = 0
    while n < gap_b.size:                       # (as _stream_rows pushed it: one block first, then hops)
        m = BLK if n == 0 else HOP
        alone.push_many({sa: gap_b[n:n + m]})
        fl.grab()
        t_alone.append(alone.loudness(sa))
        alone.drain()
        n += m
    torch.cuda.synchronize()
    assert _same_trace(t_second[1], t_ref[0]) and len(t_ref[0]) == 31
    assert fe.all(1).shape[0] > 150 and torch.equal(_bits(fe.all(1)), _bits(fr.all(0)))
    assert _same_trace(t_first[0] + t_second[0], t_alone) and t_alone[-1]["blocks"] > 60
    assert fe.all(0).shape[0] > 350 and torch.equal(_bits(fe.all(0)), _bits(fl.all(0)))


# ----------------------------------------------------------------------------- 7. end to end
def test_frames_are_those_of_prescaled_samples():
    """3 rows, tick 4, push_many + drain() and close(): the frames of the loudness server fed x are those of a plain server fed
    x * (the oracle's per-sample gain), within the decoder path's bound"""
    names, n = ("speech", "step", "gap"), BLK + 24 * HOP
    xs = [_signals()[k][:n] for k in names]
    scaled = [x * oracle_ll.running_loudness(x, FS, horizon=2.0)["gain"] for x in xs]
    assert all(float(np.abs(s - x).max()) > 1e-3 for s, x in zip(scaled, xs))
    out = {}
    for kind, wavs in (("loud", xs), ("plain", scaled)):
        srv = _loud_server(3, horizon=2.0) if kind == "loud" else _server(3, 4, window_capacity=CAP)
        sids = [srv.open(_first(3 + r), _style(80 + r)) for r in range(3)]
        parts = [[] for _ in range(3)]
        for p in range(0, n, HOP):
            srv.push_many({sid: w[p:p + HOP] for sid, w in zip(sids, wavs)})
            for sid, o in srv.drain().items():
                parts[sids.index(sid)].append(o)
        bound = _bound(srv)
        for r in range(3):
            parts[r].append(srv.close(sids[r]))
        out[kind] = [_cat(p) for p in parts]
    for r in range(3):
        assert out["loud"][r]["pose"].shape[0] == audio.n_anim_frames(n)
        for key in KEYS:
            got, want = out["loud"][r][key], out["plain"][r][key]
            assert got.shape == want.shape and torch.isfinite(got).all()
            e = float((got - want).abs().max())
            print(f"row {r} ({names[r]}) {key}: max |loudness server - plain server on pre-scaled samples| = {e:.3e}")
            assert e <= bound, (r, key, e)


# ----------------------------------------------------------------------------- 8. the off path is what it was
def _record_ops(monkeypatch):
    log = []

    def wrap(owner, name, tag):
        fn = getattr(owner, name)

        def inner(*a, **k):
            log.append(tag)
            return fn(*a, **k)
        monkeypatch.setattr(owner, name, inner)
    wrap(ops, "copy_segments", "copy")
    wrap(ops, "mel_features_batch", "mel")
    wrap(ops, "live_loudness_push", "loudness")
    wrap(ops, "live_loudness_reset", "reset")
    wrap(live._Staging, "upload", "upload")
    return log


@pytest.mark.parametrize("loud", [False, True])
def test_push_many_operations_with_loudness_off_and_on(monkeypatch, loud):
    """2 rows, 6000 samples per call into windows of 8192 (from the second call on every window compacts; feature blocks compact on
    the way).  loudness=None: the operations are what they were -- the upload, the copy launch, a second one when a feature block
    compacts, the front-end -- at most five, no loudness launch, no loudness state, the staging block laid out as before.  With
    loudness: the loudness launch behind the copy launch (which now holds only compactions and is left out when there are
    none), at most six"""
    log = _record_ops(monkeypatch)
    srv = _server(2, 4, window_capacity=8192, **(dict(loudness="running") if loud else {}))
    sids = [srv.open(_first(3), _style(60)) for _ in range(2)]
    assert log == (["reset"] * 4 if loud else [])          # (two at construction, one per open)
    x = np.tile(_signals()["speech"], 2)
    seen = set()
    for i in range(11):
        del log[:]
        srv.push_many({sid: x[6000 * i + 13 * r:6000 * (i + 1) + 13 * r] for r, sid in enumerate(sids)})
        n_ops = srv.stats["ops_last_push_many"]
        seen.add(tuple(log))
        if loud:
            assert n_ops <= 6 and log[0] == "upload" and log.count("loudness") == 1 and log.count("copy") <= 2
            assert log.index("loudness") == (2 if i > 0 else 1) and log[-1] == "mel"      # (the first call compacts nothing)
        else:
            assert n_ops <= 5 and log[:2] == ["upload", "copy"] and log[-1] == "mel" and "loudness" not in log
            assert log in (["upload", "copy", "mel"], ["upload", "copy", "copy", "mel"])
        assert n_ops == len(log) + 1                      # (the front-end is two launches)
        srv.drain()
    if loud:
        assert ("upload", "copy", "loudness", "copy", "mel") in seen and ("upload", "loudness", "mel") in seen
        assert srv._stage.o_smp - srv._stage.o_loud == 64
    else:
        assert seen == {("upload", "copy", "mel"), ("upload", "copy", "copy", "mel")}
        assert srv._loud is None and srv._chunk is None and srv.loudness_conf is None
        assert srv._stage.loud_rows == 0 and srv._stage.o_smp == srv._stage.o_loud == srv._stage.o_mel + 128
