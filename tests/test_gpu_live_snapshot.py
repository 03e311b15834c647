"""LiveServer.snapshot() / snapshot_many() / restore() (include/zeggs_hip_snapshot.h): zeggs_live_pack and zeggs_live_unpack as
the identity, restore-then-snapshot as the identity on blobs, a stream that goes on after a hand-over as if nothing had happened,
a fork, the refusals, and a server that never snapshots.

Across servers and calls the audio side and the output head are bit for bit; the decoder's products are combined with float
atomics.  So everything deterministic is held to equality and the decoder to the existing live bound (helpers.live_bound)."""
import functools

import numpy as np
import pytest
import torch

import helpers
import live_frames_oracle as fo
import test_gpu_live_dims as dims
import test_gpu_live_frames as plain
import test_gpu_live_push as lp
import test_gpu_live_refilter as filt
import test_gpu_live_retime as unfiltered
from zeggs import anim, audio, capi, live, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = dict(plain.FRAMES, text=True)
NSAMP = plain.NSAMP              # 1 s: 60 frames
RETIME = dict(max_rate=120, filter=True, min_rate=24)
ALL = ("local", "world", "bvh")
_same_bits = unfiltered._same_bits


def _full(rows, **kw):
    """every stage on: running loudness, the converter (from the first stream that asks for it), frames with all three outputs and
    text, the filtering re-timing head"""
    return lp._server(rows, 4, loudness="running", frames=FRAMES, retime=RETIME, **kw)


# the three streams of tests 2 and 4: 24 frames a second with a placement, 120 from 48 kHz s16, the server's own rate
STREAMS = (dict(frame_rate=24, start_position=fo.PLACE[0], start_rotation=fo.PLACE[1]), dict(frame_rate=120, rate=48000, pcm="s16"), dict())
RATIOS, FILTERED, PLACES = ((2, 5), (2, 1), (1, 1)), (True, True, False), (fo.PLACE, None, None)


@functools.lru_cache(maxsize=None)
def _audio(r, nsamp):
    """stream r's signal as it is delivered: float32 at 16 kHz, or int16 at 48 kHz for the converting stream"""
    if r == 1:
        return synth.synth_wav(3 * nsamp, seed=60 + r).astype(np.int16)
    return lp._wav(nsamp, 60 + r)


def _open_all(srv):
    return [srv.open(lp._first(3 + r % 2), lp._style(70 + r), **kw) for r, kw in enumerate(STREAMS)]


def _chunk(r, w, i, n=1600):
    k = 3 * n if r == 1 else n
    return w[i * k:(i + 1) * k]


def _payload_equal(a, b):
    """two blobs: every byte but the origin sid"""
    return a.shape == b.shape and a[:16].tobytes() == b[:16].tobytes() and a[24:].tobytes() == b[24:].tobytes()


def _loud_bits(srv, sid):
    got = ops.live_loudness_read(srv._loud, srv._row(sid)[0])
    return np.array([float(got[k]) for k in sorted(got)], np.float64).tobytes(), got


class _Count:
    """what snapshot_many() and restore() enqueue, counted where they enqueue it"""

    def __init__(self, monkeypatch):
        self.n = dict(upload=0, download=0, pack=0, unpack=0)
        for cls, name, key in ((live._SnapStaging, "upload", "upload"), (live._SnapStaging, "download", "download"), (ops, "live_pack", "pack"),
                               (ops, "live_unpack", "unpack")):
            monkeypatch.setattr(cls, name, self._wrap(getattr(cls, name), key))

    def _wrap(self, fn, key):
        def counted(*a, **kw):
            self.n[key] += 1
            return fn(*a, **kw)
        return counted

    def take(self):
        got, self.n = self.n, dict.fromkeys(self.n, 0)
        return got


# ----------------------------------------------------------------------------- 1. pack and unpack are the identity
def _pieces(rng, n, lo, hi):
    """n pieces: (bytes, misalignment of the state side, of the blob side) -- both sides misaligned differently, the same way,
    one side only, neither, in turn"""
    mis = [(4, 8), (12, 12), (0, 4), (8, 0), (0, 0)]
    return [(4 * int(rng.integers(lo // 4, hi // 4 + 1)), *mis[i % len(mis)]) for i in range(n)]


def _lay(pieces):
    """places on either side, 64 bytes of guard between two pieces -> (state offsets, blob offsets, state bytes, blob bytes)"""
    so, bo, s, b = [], [], 64, 64
    for nb, ms, mb in pieces:
        s, b = (s + 15) // 16 * 16 + ms, (b + 15) // 16 * 16 + mb
        so.append(s)
        bo.append(b)
        s, b = s + nb + 64, b + nb + 64
    return so, bo, s, b


def _round_trip(pieces, seed):
    rng = np.random.default_rng(seed)
    so, bo, s_bytes, b_bytes = _lay(pieces)
    src = torch.as_tensor(rng.integers(0, 256, s_bytes, dtype=np.uint8)).to(DEV)
    # the blob and the zeroed copy of the sources sit between two guard rows of NaN (test_gpu_live_dims._guarded); inside, every
    # byte that is no piece holds 0xA5
    words = (max(s_bytes, b_bytes) + 3) // 4
    big_b, blob = dims._guarded(1, 1, words)
    big_s, back = dims._guarded(1, 1, words)
    blob, back = blob.view(-1).view(torch.uint8), back.view(-1).view(torch.uint8)
    blob[:], back[:] = 0xA5, 0xA5
    for o, (nb, _, _) in zip(so, pieces):
        back[o:o + nb] = 0
    segs = (capi.SnapSeg * len(pieces))()
    for q, (nb, _, _), s, b in zip(segs, pieces, so, bo):
        q.src, q.dst_offset, q.bytes = src.data_ptr() + s, b, nb
    dev = lp._to_device(segs)
    ops.live_pack(segs, len(pieces), dev.data_ptr(), blob.data_ptr(), b_bytes)
    for q, s in zip(segs, so):
        q.src = back.data_ptr() + s
    dev2 = lp._to_device(segs)
    ops.live_unpack(segs, len(pieces), dev2.data_ptr(), blob.data_ptr(), b_bytes)
    torch.cuda.synchronize()
    assert dims._guards_intact(big_b) and dims._guards_intact(big_s)
    src_h, blob_h, back_h = src.cpu().numpy(), blob.cpu().numpy(), back.cpu().numpy()
    in_blob, in_back = np.zeros(blob_h.size, bool), np.zeros(back_h.size, bool)
    for i, ((nb, _, _), s, b) in enumerate(zip(pieces, so, bo)):
        assert blob_h[b:b + nb].tobytes() == src_h[s:s + nb].tobytes(), ("pack", i, nb)
        assert back_h[s:s + nb].tobytes() == src_h[s:s + nb].tobytes(), ("unpack", i, nb)
        in_blob[b:b + nb], in_back[s:s + nb] = True, True
    assert (blob_h[~in_blob] == 0xA5).all() and (back_h[~in_back] == 0xA5).all()      # the guard words around every destination


def test_pack_and_unpack_are_the_identity():
    """40 pieces of 4 bytes to 70 KiB (the smallest, the chunk size and its neighbours among them), the two sides misaligned
    within 16 bytes differently, in the same way, on one side and on neither: packed into a blob and unpacked into a zeroed
    copy of the sources, equal bytes; the 64 guard bytes around every destination on both sides and the guard rows around
    the buffers are intact.  Then 1 024 pieces in one call."""
    rng = np.random.default_rng(1)
    pieces = _pieces(rng, 30, 4, 70 * 1024)
    for i, nb in enumerate((4, 8, 12, 16, 20, 16384 - 4, 16384, 16384 + 4, 32768 + 12, 70 * 1024)):
        pieces.append((nb, *pieces[i][1:]))
        pieces.append((nb, 4, 4))
    assert len(pieces) == 50
    _round_trip(pieces, 2)
    _round_trip(_pieces(rng, 1024, 4, 2048), 3)


# ----------------------------------------------------------------------------- 2. restore, then snapshot: the same blob
def _busy(srv):
    """row 0 of the destination is another stream's"""
    sid = srv.open(lp._first(4), lp._style(99))
    srv.push(sid, lp._wav(NSAMP, 77)[:3200])
    return sid


def test_restore_then_snapshot_gives_the_same_blob(monkeypatch):
    """a 3-row server with every stage on and the three streams above, snapshot at five points -- right after open(), after a push
    no step has consumed, in the middle of a set_style fade, while the filtered streams' last H frames are held back, after
    hold() -- each restored into row 1 of a 2-row server whose row 0 is busy, and snapshot there: the same payload and the same
    header but the sid.  After hold(), loudness() of the copy is the source's, bit for bit, and the hold is still on.
    snapshot_many() of the three: one upload, one pack launch, one download; each restore(): one upload, one unpack launch."""
    count = _Count(monkeypatch)
    A, B = _full(3), _full(2)
    busy = _busy(B)
    sids = _open_all(A)
    wavs = [_audio(r, NSAMP) for r in range(3)]
    rounds = iter(range(100))

    def push(step=True):
        i = next(rounds)
        A.push_many({sid: _chunk(r, wavs[r], i) for r, sid in enumerate(sids)})
        return A.step() if step else {}

    def check(point, held=None):
        count.take()
        blobs = A.snapshot_many()
        assert count.take() == dict(upload=1, download=1, pack=1, unpack=0) and A.stats["ops_last_snapshot"] == 3, point
        assert list(blobs) == sids and all(b.dtype == np.uint8 and b.ndim == 1 for b in blobs.values())
        one = A.snapshot(sids[1])
        assert one.tobytes() == blobs[sids[1]].tobytes(), point          # alone or among others: the same blob
        for r, sid in enumerate(sids):
            info = live.snapshot_info(blobs[sid])
            assert info["sid"] == sid and info["row"]["n"] == A._rows[r].n and info["row"]["rs"] == int(r == 1)
            count.take()
            new = B.restore(blobs[sid])
            assert count.take() == dict(upload=1, download=0, pack=0, unpack=1) and B.stats["ops_last_restore"] == 2, (point, r)
            assert B._sids[new] == 1 and new != busy
            again = B.snapshot(new)
            assert live.snapshot_info(again)["sid"] == new
            assert _payload_equal(again, blobs[sid]), (point, r)
            if held == sid:
                (a_bits, a), (b_bits, b) = _loud_bits(A, sid), _loud_bits(B, new)
                assert a_bits == b_bits and a["hold"] and b["hold"], (a, b)
            B.close(new)
        return blobs

    first = check("open")
    assert all(live.snapshot_info(b)["row"]["n"] == 0 for b in first.values())
    push(step=False)
    assert all(w.kd == 1 and not w.sent0 for w in A._rows) and A._rows[0].n_feat > 0 and A._rows[1].rs["n_in"] == 4800
    check("push without step")
    for _ in range(3):
        push()
    k = A.set_style(sids[0], lp._style(91), fade=12)
    push()
    assert k < A._rows[0].kd < k + 12
    mid = check("in a fade")
    assert live.snapshot_info(mid[sids[0]])["row"]["fade"] == 12
    push()
    rts = [w.rt for w in A._rows]
    assert all(live.LiveServer._emitted(t, t["n_in"], True) > t["n_out"] for t in rts[:2]) and rts[0]["half"] == 10      # frames are held back
    check("frames held back")
    A.hold(sids[1])
    push()
    check("after hold", held=sids[1])
    A.close(sids[2])
    with pytest.raises(KeyError, match="no open stream"):
        A.snapshot(sids[2])
    with pytest.raises(KeyError, match="no open stream"):
        A.snapshot_many([sids[0], sids[2]])


# ----------------------------------------------------------------------------- 3. a window that has moved
def _live_window(srv, r):
    w = srv._rows[r]
    return w.base, srv.window[r][:w.n - w.base].clone()


def test_a_window_that_has_moved():
    """a stream 1.5 s long in a window of 4096 samples (its base has moved, compactions have happened) restored into a server whose
    window for that row has 1024 (it grows first) and is still at the start; the same further audio to both: after every push
    the pending feature rows, the live window samples and loudness() are equal bit for bit, and the counters but `base`"""
    A = lp._server(2, 4, window_capacity=4096, loudness="running")
    B = lp._server(2, 4, window_capacity=1024, loudness="running")
    wav = lp._wav(40000, 21)
    sid = A.open(lp._first(3), lp._style(31))
    for i in range(15):
        A.push_many({sid: wav[1600 * i:1600 * (i + 1)]})
        A.drain()
    A.push(sid, wav[24000:24700])                       # (a push no step has consumed: pending rows and a window off its start)
    w = A._rows[0]
    base0 = w.base
    assert base0 > 4096 and w.n - base0 > 1024 and w.n_feat > w.n_ring and A.stats["window_capacity"][0] == 4096
    new = B.restore(A.snapshot(sid))
    assert B.stats["window_capacity"][0] == w.n - w.base and B.stats["ops_last_restore"] == 3          # (the growth: one more)
    for i, cut in enumerate((24700, 26300, 27900, 30000, 33000)):
        if i:
            for srv, s in ((A, sid), (B, new)):
                if i % 2:
                    srv.push(s, wav[prev:cut])
                else:
                    srv.push_many({s: wav[prev:cut]})
        prev = cut
        a, b = A._rows[0], B._rows[0]
        assert (a.n, a.n_feat, a.fbase, a.n_ring, a.kd) == (b.n, b.n_feat, b.fbase, b.n_ring, b.kd), i
        assert a.n_feat > a.n_ring and torch.equal(lp._pending(A, 0), lp._pending(B, 0)), i
        (ba, wa), (bb, wb) = _live_window(A, 0), _live_window(B, 0)
        lo = max(ba, bb)
        assert a.n - lo > 1000 and torch.equal(lp._bits(wa[lo - ba:]), lp._bits(wb[lo - bb:])), i
        assert _loud_bits(A, sid)[0] == _loud_bits(B, new)[0], i
        if i in (1, 3):
            oa, ob = A.drain(), B.drain()
            assert sid in oa and new in ob and oa[sid]["pose"].shape == ob[new]["pose"].shape
    assert A._rows[0].base > base0


# ----------------------------------------------------------------------------- 4. the stream goes on
class _Tap:
    """every sample that enters the windows of a server's rows, as it lies there (converted, times the running gain): collected
    after every push and, through _features, inside close(), where a converting row's tail arrives"""

    def __init__(self, srv):
        self.srv, self.seen, self.parts = srv, {}, {}
        inner = srv._features

        def features(r, row, k1, final):
            self.grab()
            return inner(r, row, k1, final)
        srv._features = features

    def grab(self):
        for r, w in enumerate(self.srv._rows):
            if w is not None and w.n > self.seen.get(w.sid, 0):
                a = self.seen.get(w.sid, 0)
                assert a >= w.base
                self.parts.setdefault(w.sid, []).append(self.srv.window[r][a - w.base:w.n - w.base].cpu().numpy().copy())
                self.seen[w.sid] = w.n

    def wav(self, sid):
        return np.concatenate(self.parts[sid])


def _rounds(srv, sids, wavs, lo, hi, parts, tap=None):
    for i in range(lo, hi):
        srv.push_many({sid: _chunk(r, wavs[r], i) for r, sid in enumerate(sids) if _chunk(r, wavs[r], i).size})
        if tap:
            tap.grab()
        for sid, o in srv.step().items():
            parts[sids.index(sid)].append(o)


def _finish(srv, sids, parts):
    """drain, what the test reads just before close(), close -> per stream (loudness bits, window of the row)"""
    for sid, o in srv.drain().items():
        parts[sids.index(sid)].append(o)
    last = [(_loud_bits(srv, sid)[0], _live_window(srv, srv._sids[sid])) for sid in sids]
    for r, sid in enumerate(sids):
        parts[r].append(srv.close(sid))
    return last


def _own_rows_rule(w, r, what):
    """the frames of a stream, text included, are the head's kernel run in another cut (records of 20, a fresh state) on the pose
    rows the stream returned"""
    lr = ops.LiveRefilter(1, synth.PARENTS, 20, 10, None, ALL, "zyx", None, DEV)
    src = tuple(torch.as_tensor(w[k], device=DEV) for k in lp.KEYS)
    T = w["pose"].shape[0]
    filt._reset(lr, 0, src, PLACES[r])
    again = filt._run_cuts(lr, 0, src, [20] * (T // 20) + ([T % 20] if T % 20 else []), RATIOS[r], FILTERED[r])
    _same_bits(w["frames"], again, what)
    assert w["frames"]["text"] == anim.format_rows(np.ascontiguousarray(w["frames"]["bvh"])), what


def test_the_stream_goes_on_as_if_nothing_had_happened():
    """the three streams on server A for the first five of their ten chunks, snapshot, restored on server B and served to the end
    there; the same audio without interruption on server C.
    * pose, root position and rotation of A's parts followed by B's are within helpers.live_bound of the offline rollout, as C's
      are (the rollout is helpers.live_offline over the samples that entered C's windows -- converted and times the running gain
      by the stages as they stood before this feature; the copy's audio side is held to C's by equality below);
    * "frame0" is contiguous across the hand-over and the frame count at the end is C's;
    * the frames of A's and B's parts together obey the own-rows rule, text included;
    * loudness estimate and gain just before close() equal C's bit for bit, and so do the converting stream's window samples."""
    A, B, C = _full(3), _full(3), _full(3)
    wavs = [_audio(r, NSAMP - 1600 * (r % 3)) for r in range(3)]
    a_sids, c_sids = _open_all(A), _open_all(C)
    tap = _Tap(C)
    got, ref = [[] for _ in range(3)], [[] for _ in range(3)]
    _rounds(A, a_sids, wavs, 0, 5, got)
    blobs = A.snapshot_many()
    b_sids = [B.restore(blobs[sid]) for sid in reversed(a_sids)][::-1]          # (other rows than on A)
    assert [B._sids[s] for s in b_sids] == [2, 1, 0]
    _rounds(B, b_sids, wavs, 5, 10, got)
    _rounds(C, c_sids, wavs, 0, 10, ref, tap)
    bound = helpers.live_bound(B)
    last_b, last_c = _finish(B, b_sids, got), _finish(C, c_sids, ref)
    for r in range(3):
        wg, wc = unfiltered._whole(got[r]), unfiltered._whole(ref[r])
        eff = tap.wav(c_sids[r])
        T = audio.n_anim_frames(eff.size)
        assert T == wc["pose"].shape[0] == wg["pose"].shape[0] == audio.n_anim_frames(NSAMP - 1600 * (r % 3))
        offline = helpers.live_offline(eff, lp._first(3 + r % 2), lp._style(70 + r))
        for name, parts in (("uninterrupted", ref[r]), ("handed over", got[r])):
            e = helpers.live_err(lp._cat(parts), offline)
            print(f"stream {r} {name}: max |live - offline| = {e}")
            assert max(e.values()) <= bound, (r, name, e)
        m = 0
        for p in (p for p in got[r] if p):
            assert p["frames"]["frame0"] == m, r
            m += p["frames"]["bvh"].shape[0]
        assert m == wc["frames"]["bvh"].shape[0] == filt.ro.n_out(T, *RATIOS[r])
        _own_rows_rule(wg, r, ("handed over", r))
        assert last_b[r][0] == last_c[r][0], r
        (bb, xb), (bc, xc) = last_b[r][1], last_c[r][1]
        lo = max(bb, bc)
        assert xb.numel() + bb == xc.numel() + bc and torch.equal(lp._bits(xb[lo - bb:]), lp._bits(xc[lo - bc:])), r
    assert last_b[1][1][1].numel() > 1000


# ----------------------------------------------------------------------------- 5. fork
def test_fork_in_the_middle_of_a_style_fade():
    """one stream at 24 frames a second, placed, snapshot four frames into a 12-frame style fade and restored on the same server:
    the same audio to both, step(), close().  Both stay within the bound of the offline rollout with the fade's style rows; the
    frames of each obey the own-rows rule; where the two rows decoded the same bits their frames are the same bits"""
    srv = lp._server(3, 4, frames=FRAMES, retime=RETIME)
    wav = lp._wav(NSAMP + 3200, 64)
    sid = srv.open(lp._first(3), lp._style(70), **STREAMS[0])
    parts = {sid: []}
    for i in range(4):
        srv.push_many({sid: wav[1600 * i:1600 * (i + 1)]})
        parts[sid] += list(srv.step().values())
    k = srv.set_style(sid, lp._style(92), fade=12)
    srv.push_many({sid: wav[6400:8000]})
    parts[sid] += list(srv.step().values())
    assert k < srv._rows[0].kd < k + 12
    twin = srv.restore(srv.snapshot(sid))
    assert twin != sid and srv._sids[twin] == 1 and srv._rows[1].k_style == k and srv._rows[1].fade == 12
    parts[twin] = list(parts[sid])
    for i in range(5, (NSAMP + 3200) // 1600):
        srv.push_many({s: wav[1600 * i:1600 * (i + 1)] for s in (sid, twin)})
        for s, o in srv.step().items():
            parts[s].append(o)
    for s, o in srv.drain().items():
        parts[s].append(o)
    bound = helpers.live_bound(srv)
    for s in (sid, twin):
        parts[s].append(srv.close(s))
    T = audio.n_anim_frames(wav.size)
    wgt = torch.tensor([[live.style_weight(f, k, 12)] for f in range(T)], device=DEV)
    offline = helpers.live_offline(wav, lp._first(3), torch.lerp(lp._style(70), lp._style(92), wgt))
    whole = {}
    for s in (sid, twin):
        e = helpers.live_err(lp._cat(parts[s]), offline)
        print(f"{'source' if s == sid else 'fork'}: max |live - offline| = {e}")
        assert max(e.values()) <= bound, (s, e)
        whole[s] = unfiltered._whole(parts[s])
        _own_rows_rule(whole[s], 0, s)
    if all(np.array_equal(whole[sid][key], whole[twin][key]) for key in lp.KEYS):
        _same_bits(whole[sid]["frames"], whole[twin]["frames"], "fork")
        assert whole[sid]["frames"]["text"] == whole[twin]["frames"]["text"]


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_destination_as_it_was(monkeypatch):
    """a blob from a server with tick 5, a truncated blob and a blob from a server without loudness, offered to a tick-4 server with
    loudness: each raises ValueError naming the field or the section; nothing is enqueued; afterwards the destination's free
    rows, _next_sid and a snapshot of its one running stream are what they were.  A full server raises open()'s RuntimeError."""
    count = _Count(monkeypatch)
    dst = lp._server(2, 4, loudness="running")
    mine = dst.open(lp._first(3), lp._style(40))
    dst.push(mine, lp._wav(NSAMP, 41)[:4000])
    dst.step()
    before = (dst.snapshot(mine), [w is None for w in dst._rows], dst._next_sid, dict(dst._sids))
    blobs = {}
    for name, srv in (("tick", lp._server(2, 5, loudness="running")), ("loudness", lp._server(2, 4)), ("good", lp._server(2, 4, loudness="running"))):
        sid = srv.open(lp._first(4), lp._style(42))
        srv.push(sid, lp._wav(NSAMP, 43)[:4000])
        blobs[name] = srv.snapshot(sid)
    count.take()
    with pytest.raises(ValueError, match="a server with tick = 5.0, this one has tick = 4.0"):
        dst.restore(blobs["tick"])
    with pytest.raises(ValueError, match="a server with loudness = 0.0, this one has loudness = 1.0"):
        dst.restore(blobs["loudness"])
    with pytest.raises(ValueError, match="section '\\w+' ends at byte \\d+, the blob has \\d+: truncated"):
        dst.restore(blobs["good"][:live.snapshot_info(blobs["good"])["sections"]["ring"][0] + 64])
    longer = blobs["good"].copy()
    o_tab = live._SNAP_HEAD + 8 * len(live.SNAP_FINGERPRINT)
    with pytest.raises(ValueError, match="section"):
        longer[o_tab + 24 * live.SNAP_SECTIONS.index("pose") + 16:][:8] = np.frombuffer(np.array([4096], "<u8").tobytes(), np.uint8)
        dst.restore(longer)
    other = blobs["good"].copy()
    other[8:12] = np.frombuffer(np.array([live.SNAP_FORMAT + 1], "<u4").tobytes(), np.uint8)
    with pytest.raises(ValueError, match="format version 2"):
        dst.restore(other)
    other = blobs["good"].copy()
    other[12:16] = np.frombuffer(np.array([7], "<u4").tobytes(), np.uint8)
    with pytest.raises(ValueError, match="snapshot version 7, this library is version 1"):
        dst.restore(other)
    assert count.take() == dict(upload=0, download=0, pack=0, unpack=0)
    after = (dst.snapshot(mine), [w is None for w in dst._rows], dst._next_sid, dict(dst._sids))
    assert after[0].tobytes() == before[0].tobytes() and after[1:] == before[1:]
    new = dst.restore(blobs["good"])
    assert dst._sids[new] == 1 and new == before[2]
    count.take()
    with pytest.raises(RuntimeError, match="all 2 rows are in use"):
        dst.restore(blobs["good"])
    assert count.take() == dict(upload=0, download=0, pack=0, unpack=0)


# ----------------------------------------------------------------------------- 7. an unused feature costs nothing
def test_an_unused_feature_costs_nothing():
    """two servers with every stage on, the same three streams: one snapshots all rows after every step, the other never.  The one
    that never does holds no staging block and no snapshot counters, and both report the launches_per_step (11 + 3: the head, its
    download and the text) and at most the 7 operations per push_many that the existing tests pin for this configuration"""
    servers = {"never": _full(3), "snapshots": _full(3)}
    wavs = [_audio(r, NSAMP) for r in range(3)]
    for name, srv in servers.items():
        sids = _open_all(srv)
        ops_seen = set()
        for i in range(6):
            srv.push_many({sid: _chunk(r, wavs[r], i) for r, sid in enumerate(sids)})
            ops_seen.add(srv.stats["ops_last_push_many"])
            srv.step()
            if name == "snapshots":
                assert len(srv.snapshot_many()) == 3
        assert srv.stats["launches_per_step"] == 11 + 3 and max(ops_seen) <= 7, (name, ops_seen)
        servers[name] = ops_seen
        if name == "never":
            assert getattr(srv, "_snap", None) is None and not {"ops_last_snapshot", "ops_last_restore", "snapshot_bytes"} & set(srv.stats)
        else:
            assert srv.stats["ops_last_snapshot"] == 3 and srv._snap is not None
    assert servers["never"] == servers["snapshots"]
