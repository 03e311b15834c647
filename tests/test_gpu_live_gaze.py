"""Live serving, the moving gaze (LiveServer(gaze=...), set_gaze / set_gaze_many / gaze; include/zeggs_hip_gaze.h).  The yardstick
is the existing offline path -- audio.preprocess_audio -> speech encoder -> ops.decoder_core over the whole clip, as
helpers.live_offline runs it -- with a per-frame gaze tensor built by the float64 oracle tests/live_gaze_oracle.py from the k
each call returned; never the new code against itself.

Bounds: gaze rows 2^-23 max(1, |oracle|) per component (one float32 rounding of a float64 evaluation, which a last-bit
difference of two libms can flip); style rows 1e-6 against torch.lerp (two float32 roundings at an ulp of 4.8e-7 for |x| < 4);
frames helpers.live_bound(srv) against the offline rollout; 2e-5 between two runs of the same frames (run to run only the
split-K atomics of the prologue products differ, tests/test_gpu_live.py)."""
import numpy as np
import pytest
import torch

import helpers
import live_gaze_oracle as oracle_gz
from zeggs import audio, live, ops, synth

pytestmark = pytest.mark.gpu
DEV = helpers.LIVE_DEV
KEYS = helpers.LIVE_KEYS
NSAMP = 32000
_first, _wav, _style, _server, _cat = helpers.live_first, helpers.live_wav, helpers.live_style, helpers.live_server, helpers.live_cat


# ----------------------------------------------------------------------------- helpers
def _gaze0(first):
    return first[14][0].detach().cpu().numpy().astype(np.float32).reshape(3)


def _root0(first):
    return first[0][0].detach().cpu().numpy().astype(np.float32).reshape(3)


def _turned(first, deg=60.0):
    """the first gaze turned `deg` degrees about the vertical through the first root position -> (target, pivot), float64"""
    g, p = _gaze0(first).astype(np.float64), _root0(first).astype(np.float64)
    t, d = np.deg2rad(deg), g - p
    return p + np.array([np.cos(t) * d[0] + np.sin(t) * d[2], d[1], -np.sin(t) * d[0] + np.cos(t) * d[2]]), p


_OFFLINE = {}


def _offline(wav, first, style, track, key=None):
    """helpers.live_offline with a per-frame gaze tensor (track [n_frames, 3], float32 values; None: the first pose's gaze)"""
    if key is not None and key in _OFFLINE:
        return _OFFLINE[key]
    se, de = helpers.live_nets()
    st = helpers.live_stats()
    n_frames = audio.n_anim_frames(len(wav))
    feats = torch.as_tensor(audio.preprocess_audio(wav, 60, n_frames, helpers.LIVE_CONF, ["mel_spec", "energy"]), device=DEV)
    with torch.no_grad():
        sp = se(((feats[None] - st["audio_input_mean"]) / st["audio_input_std"]).contiguous())
        f32 = lambda a: a[0:1].to(torch.float32).contiguous()  # noqa: E731
        rp, rr, rv, rw, lp, _, lt, lv, lw = first[:9]
        pose0 = torch.cat([f32(x).reshape(1, -1) for x in (rv, rw, lp, lt, lv, lw)], dim=1)
        if track is None:
            gaze = f32(first[14]).repeat(n_frames, 1)[None].contiguous()
        else:
            assert track.shape == (n_frames, 3)
            gaze = torch.as_tensor(np.asarray(track, np.float64).astype(np.float32), device=DEV)[None].contiguous()
        ref = ops.decoder_core(de, pose0, f32(rp), f32(rr), gaze, sp, style.repeat(n_frames, 1)[None].contiguous(), st["anim_input_mean"],
                               st["anim_input_std"], st["anim_output_mean"], st["anim_output_std"], synth.DT)
    out = tuple(r[0] for r in ref)
    if key is not None:
        _OFFLINE[key] = out
    return out


class _Tap:
    """records the gaze rows every decoder call of the given servers is handed, per stream and frame (indices 1 .. of a chunk:
    the frames the call decodes; index 0 is the frame it starts from, which no step reads)"""

    def __init__(self, monkeypatch, *servers):
        self.servers, self.rows = list(servers), {}
        chunk, batch = ops.decoder_chunk, ops.decoder_batch_chunk

        def tapped_chunk(decoder, pose, rpos, rrot, gaze, *a, **kw):
            for s in self.servers:
                off = pose.data_ptr() - s.pose.data_ptr()
                if 0 <= off < 4 * s.pose.numel():
                    self._note(s, off // (4 * s.pose.shape[1]), gaze[0])
            return chunk(decoder, pose, rpos, rrot, gaze, *a, **kw)

        def tapped_batch(bd, pose, rpos, rrot, gaze, *a, **kw):
            for s in self.servers:
                if s.bd is bd:
                    for r in range(s.rows):
                        self._note(s, r, gaze[r])
            return batch(bd, pose, rpos, rrot, gaze, *a, **kw)
        monkeypatch.setattr(ops, "decoder_chunk", tapped_chunk)
        monkeypatch.setattr(ops, "decoder_batch_chunk", tapped_batch)

    def _note(self, s, r, g):
        row = s._rows[r]
        if row is None:
            return
        g = g.detach().cpu().numpy()
        mine = self.rows.setdefault((id(s), row.sid), {})
        for i in range(1, g.shape[0]):           # (a row that rides along on filler is overwritten when its frames are decoded)
            mine[row.kd - 1 + i] = g[i].copy()

    def track(self, s, sid, n_frames, gaze0):
        mine = self.rows[(id(s), sid)]
        assert set(range(1, n_frames)) <= set(mine)
        return np.stack([gaze0] + [mine[f] for f in range(1, n_frames)])


def _bound(srv):
    """helpers.live_bound where the rows rode the batched decoder call (it asserts which path ran); a one-row server decodes on the
    B = 1 entry point, whose bound is the smaller of live_bound's two"""
    return 5e-5 if srv.rows == 1 else helpers.live_bound(srv)


def _drive(srv, specs, chunks, many=False, before_close=None, after_open=None):
    """open one stream per spec -- dict(wav, first, style, sets=[dict(k= | at=, **set_gaze arguments)]) -- push every wav in
    `chunks` (push, or one push_many for all), step() until nothing is eligible after every push, then close.  A set with `at`
    is made in front of push number `at`; one with `k` in front of the step at which the stream's first undecoded frame is k
    (asserted to be met exactly).  -> per stream dict(sid, frames, sets: what the oracle needs of each call -- the returned k,
    the arguments, the served root of frame k - 1)"""
    runs = []
    for sp in specs:
        sid = srv.open(sp["first"], sp["style"])
        runs.append(dict(sid=sid, parts=[], sets=[], todo=[dict(s) for s in sp.get("sets", [])], wav=sp["wav"], pos=0))
    if after_open is not None:
        after_open()

    def due(i_push=None):
        for run in runs:
            while run["todo"]:
                s, kd = run["todo"][0], srv._rows[srv._sids[run["sid"]]].kd
                if ("at" in s and s["at"] != i_push) or ("k" in s and kd < s["k"]):
                    break
                run["todo"].pop(0)
                assert "at" in s or kd == s["k"], (kd, s)
                args = {k: v for k, v in s.items() if k not in ("at", "k")}
                k = srv.set_gaze(run["sid"], **args)
                assert k == kd
                got = _cat(run["parts"]) if any(run["parts"]) else None
                run["sets"].append(dict(args, k=k, rpos=None if got is None else got["rpos"][k - 1].cpu().numpy(),
                                        rrot=None if got is None else got["rrot"][k - 1].cpu().numpy()))

    for i, n in enumerate(chunks):
        due(i)
        if many:
            srv.push_many({run["sid"]: run["wav"][run["pos"]:run["pos"] + n] for run in runs})
        else:
            for run in runs:
                srv.push(run["sid"], run["wav"][run["pos"]:run["pos"] + n])
        for run in runs:
            run["pos"] += n
        while True:
            due()
            out = srv.step()
            if not out:
                break
            for run in runs:
                run["parts"].append(out.get(run["sid"]))
    assert all(run["pos"] >= len(run["wav"]) for run in runs)
    if before_close is not None:
        before_close()
    for run in runs:
        run["parts"].append(srv.close(run["sid"]))
        assert not [s for s in run["todo"] if "k" in s], run["todo"]
        run["frames"] = _cat(run["parts"])
    return runs


def _oracle_track(n_frames, first, sets):
    return oracle_gz.track(n_frames, _gaze0(first), [dict(s) for s in sets])


def _same_rows(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes()


def _within(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want.astype(np.float32).astype(np.float64)) / oracle_gz.bound(want)
    return float(err.max())


def _upload(recs):
    return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(DEV)


# ----------------------------------------------------------------------------- 1. the condition launch alone
@pytest.mark.parametrize("rows", [3, 1])
def test_the_condition_launch_alone(rows):
    """the state of 3 rows (row 1 takes no part) or of 1 row, set through the library; consecutive decoder calls of n = 4, 5 and
    tick + LOOKAHEAD + 1 = 20 frames each: a fade of 12 from k = 1 on an arc (it spans several calls), and on the 3-row state a
    step (fade 0) at k = 6 beside it.  Gaze rows against the oracle at 2^-23 max(1, |oracle|), style rows against torch.lerp with
    style_weight's weights at 1e-6, the slice of the row that does not take part bit for bit what it was"""
    ST, gen = 64, torch.Generator(DEV).manual_seed(5)
    lg = ops.LiveGaze(rows, ST, DEV)
    sty_old, sty_new = (torch.randn(rows, ST, device=DEV, generator=gen) * 0.5 for _ in range(2))
    assert float(torch.maximum(sty_old.abs().max(), sty_new.abs().max())) < 4.0
    g0 = np.array([[0.3, 1.6, 2.5], [9.0, 9.0, 9.0], [-1.0, 1.4, 2.0]], np.float32)[:rows]
    for r in range(rows):
        ops.live_gaze_reset(lg, r, torch.as_tensor(g0[r], device=DEV))
    rpos, rrot = torch.zeros(rows, 3, device=DEV), torch.zeros(rows, 4, device=DEV)
    sets = {0: dict(k=1, target=[-2.0, 1.2, 1.0], fade=12, path="arc", pivot=[0.0, 1.5, 0.0], ease="smooth")}
    style_fades = {0: (3, 12), 2: (0, 0)}                                      # (k_style, fade) of the rows' style fades
    if rows == 3:
        sets[2] = dict(k=6, target=[1.5, 1.0, 3.0], fade=0)
    recs = (ops.GazeSet * len(sets))()
    for q, (r, s) in zip(recs, sets.items()):
        q.target[:], q.pivot[:] = s["target"], s.get("pivot", [0.0] * 3)
        q.k, q.fade, q.row, q.has_pivot = s["k"], s["fade"], r, int("pivot" in s)
        q.space, q.path, q.ease = 0, ops.GAZE_PATHS[s.get("path", "line")], ops.GAZE_EASES[s.get("ease", "linear")]
    keep = _upload(recs)
    ops.live_gaze_set(lg, recs, len(sets), rpos, rrot, keep.data_ptr() if len(sets) > 1 else None)
    want = {r: oracle_gz.apply(oracle_gz.reset(g0[r]), **s) for r, s in sets.items()}
    for r, s in want.items():
        got = ops.live_gaze_read(lg, r, 0)
        assert (got["k"], got["fade"], got["path"], got["ease"]) == (s["k"], s["fade"], s["path"], s["ease"])
        assert _within(got["end"], s["end"]) == 0.0 and _within(got["start"], s["start"]) <= 1.0
    worst_g = worst_s = 0.0
    for n in (4, 5, 20):
        k0 = 0
        for _ in range(3):
            gaze = torch.rand(rows, 20, 3, device=DEV, generator=gen) + 40.0
            style = torch.rand(rows, 20, ST, device=DEV, generator=gen) + 40.0
            was_g, was_s = gaze.clone(), style.clone()
            cond = (ops.GazeCond * len(sets))()
            for q, r in zip(cond, sets):
                q.row, q.out_row, q.k0, q.n, q.k_style, q.fade_style = r, r, k0, n, *style_fades[r]
            keep = _upload(cond)
            ops.live_condition(lg, cond, len(sets), sty_old, sty_new, gaze, style, keep.data_ptr() if len(sets) > 1 else None)
            for r in range(rows):
                if r not in sets:
                    assert torch.equal(gaze[r].view(torch.int32), was_g[r].view(torch.int32)), "the idle row's gaze slice was touched"
                    assert torch.equal(style[r].view(torch.int32), was_s[r].view(torch.int32)), "the idle row's style slice was touched"
                    continue
                ref = np.stack([oracle_gz.point(want[r], k0 + i) for i in range(n)])
                worst_g = max(worst_g, _within(gaze[r, :n].cpu().numpy(), ref))
                wgt = torch.tensor([[live.style_weight(k0 + i, *style_fades[r])] for i in range(n)], dtype=torch.float32, device=DEV)
                lerp = torch.lerp(sty_old[r][None], sty_new[r][None], wgt)
                worst_s = max(worst_s, float((style[r, :n] - lerp).abs().max()))
                assert torch.equal(gaze[r, n:].view(torch.int32), was_g[r, n:].view(torch.int32)), "frames past n were touched"
                assert torch.equal(style[r, n:].view(torch.int32), was_s[r, n:].view(torch.int32)), "frames past n were touched"
            k0 += n - 1
    print(f"rows={rows}: gaze rows worst {worst_g:.3f} of the bound, style rows worst |diff| {worst_s:.2e}")
    assert worst_g <= 1.0 and worst_s <= 1e-6


# ----------------------------------------------------------------------------- 2. a moving gaze equals the offline rollout
_PLAIN_RUNS = {}


def _plain_run(rows, tick):
    """the stream of test 2 through a server of the same shape on which set_gaze is never called"""
    if (rows, tick) not in _PLAIN_RUNS:
        srv = _server(rows, tick, gaze=True)
        run = _drive(srv, [dict(wav=_wav(NSAMP, 2), first=_first(3), style=_style(31))], [1600] * 20)[0]
        _PLAIN_RUNS[(rows, tick)] = run["frames"]
    return _PLAIN_RUNS[(rows, tick)]


@pytest.mark.parametrize("mode", [("line", 0, None), ("line", 12, None), ("arc", 12, "smooth")], ids=["line-step", "line-fade12", "arc-fade12-smooth"])
@pytest.mark.parametrize("rows,tick", [(1, 4), (3, 3), (3, 4)])
def test_a_moving_gaze_equals_the_offline_rollout(rows, tick, mode):
    """set_gaze in front of push 9 of 20: the target is the first gaze turned 60 degrees about the first root position.  All frames
    within live_bound of ops.decoder_core with the oracle's per-frame gaze track; frames before k within 2e-5 of a run without the
    call; and the change took effect -- the two offline rollouts differ by more than 10 x the bound after k + fade (checked on
    the reference alone first), and so do the served frames"""
    path, fade, ease = mode
    wav, first, style = _wav(NSAMP, 2), _first(3), _style(31)
    target, pivot = _turned(first)
    call = dict(at=9, target=target, fade=fade, path=path, ease=ease, pivot=pivot if path == "arc" else None)
    srv = _server(rows, tick, gaze=dict(ease="linear"))
    run = _drive(srv, [dict(wav=wav, first=first, style=style, sets=[call])], [1600] * 20)[0]
    bound = _bound(srv)
    (s,), n_frames = run["sets"], audio.n_anim_frames(NSAMP)
    k = s["k"]
    assert 20 < k < n_frames - 20 - fade
    track = _oracle_track(n_frames, first, [dict(k=k, target=target, fade=fade, path=path, ease=ease or "linear", pivot=call["pivot"])])
    assert np.array_equal(track[:k], np.tile(_gaze0(first).astype(np.float64), (k, 1))) and np.allclose(track[k + fade:], target, atol=1e-6)
    ref = _offline(wav, first, style, track)
    e = helpers.live_err(run["frames"], ref)
    print(f"rows={rows} tick={tick} {mode} k={k}: {e} (bound {bound})")
    assert max(e.values()) <= bound, e
    still = _offline(wav, first, style, None, key="still")
    moved = float((ref[0][k + fade:] - still[0][k + fade:]).abs().max())
    print(f"offline with the track against offline without, frames {k + fade}..: {moved:.3e}")
    assert moved > 10 * bound, "the reference itself does not see the gaze move: the test shows nothing"
    plain = _plain_run(rows, tick)
    for key in KEYS:
        assert float((run["frames"][key][:k] - plain[key][:k]).abs().max()) <= 2e-5, key
    assert float((run["frames"]["pose"][k + fade:] - plain["pose"][k + fade:]).abs().max()) > 10 * bound


# ----------------------------------------------------------------------------- 3. root space
def test_a_target_in_the_root_frame_is_resolved_with_the_served_root():
    """set_gaze(space="root", path="arc") in the middle of a stream: gaze(sid)["end"] is the oracle's resolution of the target with
    the SERVED root of frame k - 1 (the stored quaternion as it is), the pivot that root position, and the frames equal the
    offline rollout with the resulting track"""
    wav, first, style = _wav(NSAMP, 2), _first(3), _style(31)
    local = [0.8, 1.6, 2.0]
    seen = {}
    srv = _server(3, 4, gaze=True)

    def look():
        seen.update(srv.gaze(0))
    run = _drive(srv, [dict(wav=wav, first=first, style=style, sets=[dict(at=8, target=local, fade=12, space="root", path="arc")])], [1600] * 20,
                 before_close=look)[0]
    bound = _bound(srv)
    (s,), n_frames = run["sets"], audio.n_anim_frames(NSAMP)
    k = s["k"]
    assert 20 < k < n_frames - 40 and s["rpos"] is not None
    want = oracle_gz.apply(oracle_gz.reset(_gaze0(first)), k, local, fade=12, space="root", path="arc", rpos=s["rpos"], rrot=s["rrot"])
    assert abs(np.linalg.norm(s["rrot"].astype(np.float64)) - 1.0) < 1e-3
    print(f"k={k}: end {seen['end']} against {want['end']}: {_within(seen['end'], oracle_gz.resolve(s['rpos'], s['rrot'], local)):.3f} of the bound")
    assert _within(seen["end"], oracle_gz.resolve(s["rpos"], s["rrot"], local)) <= 1.0
    assert (seen["k"], seen["fade"], seen["path"], seen["ease"]) == (k, 12, "arc", "linear")
    assert _within(seen["target"], want["end"]) <= 1.0                         # the fade is over when the stream closes
    track = _oracle_track(n_frames, first, [dict(k=k, target=local, fade=12, space="root", path="arc", rpos=s["rpos"], rrot=s["rrot"])])
    e = helpers.live_err(run["frames"], _offline(wav, first, style, track))
    print(f"root space: {e} (bound {bound})")
    assert max(e.values()) <= bound, e


# ----------------------------------------------------------------------------- 4. independence of the cuts and of the other rows
def _poison(srv, r):
    nan = float("nan")
    for t in (srv.window[r], srv.feats[r], srv.ring[r], srv.h[:, r], srv.pose[r], srv.rpos[r], srv.rrot[r], srv.gaze[r], srv.sty_old[r],
              srv.sty_new[r], srv._gz_style[r], srv._gz.state.view(torch.float32).view(srv.rows, -1)[r]):
        t.fill_(nan)


def test_the_schedule_does_not_depend_on_the_cuts_or_on_the_other_rows(monkeypatch):
    """one stream with two sets (the second in the middle of the first one's fade, on an arc about the first root position),
    placed at the same k, three ways on 3-row servers: in chunks of 1600 with an idle row poisoned with NaN, in chunks of 700 and
    2500, and through push_many beside two other streams with gaze schedules of their own.  The gaze rows handed to the decoder
    are the same bits in all three, the frames agree within the bound with each other and with the offline rollout"""
    wav, first, style = _wav(NSAMP, 2), _first(3), _style(31)
    target, pivot = _turned(first)
    other, _ = _turned(first, -45.0)
    sets = [dict(k=21, target=other, fade=12), dict(k=29, target=target, fade=12, path="arc", pivot=pivot, ease="smooth")]
    me = dict(wav=wav, first=first, style=style, sets=sets)
    n_frames = audio.n_anim_frames(NSAMP)
    got = {}
    for name, chunks, many in (("1600", [1600] * 20, False), ("700/2500", [700, 2500] * 10, False), ("push_many", [1600] * 20, True)):
        srv = _server(3, 4, gaze=True)
        tap = _Tap(monkeypatch, srv)
        specs = [me]
        if many:
            specs = [dict(wav=_wav(NSAMP, 7), first=_first(4), style=_style(33), sets=[dict(k=9, target=[0.0, 1.0, 3.0], fade=30)]), me,
                     dict(wav=_wav(NSAMP, 8), first=_first(5), style=_style(34), sets=[dict(at=3, target=[1.0, 1.5, 2.0], fade=5, space="root")])]
        runs = _drive(srv, specs, chunks, many=many, after_open=None if many else lambda: _poison(srv, 2))
        run = runs[1] if many else runs[0]
        assert [s["k"] for s in run["sets"]] == [21, 29]
        got[name] = (run["frames"], tap.track(srv, run["sid"], n_frames, _gaze0(first)), _bound(srv))
        if not many:
            assert all(torch.isnan(t).all() for t in (srv.h[:, 2], srv.pose[2], srv.gaze[2], srv._gz_style[2]))      # the idle row was never written
    base_frames, base_track, bound = got["1600"]
    track = _oracle_track(n_frames, first, [dict(s) for s in sets])
    print(f"handed gaze rows against the oracle: {_within(base_track, track):.3f} of the bound")
    assert _within(base_track, track) <= 1.0
    e = helpers.live_err(base_frames, _offline(wav, first, style, track))
    print(f"1600: {e} (bound {bound})")
    assert max(e.values()) <= bound, e
    for name in ("700/2500", "push_many"):
        frames, handed, _ = got[name]
        assert _same_rows(handed, base_track), f"{name}: the gaze rows are not the bits of the run in chunks of 1600"
        e = helpers.live_err(frames, tuple(base_frames[k] for k in KEYS))
        print(f"{name} against 1600: {e}")
        assert max(e.values()) <= bound, (name, e)


# ----------------------------------------------------------------------------- 5. set_gaze_many
def test_set_gaze_many_is_three_set_gaze_calls():
    """three streams, one set_gaze_many on one server and three set_gaze calls on its twin: the same k, the same state bit for
    bit through gaze(); one upload and one launch for the three, one launch for a single set_gaze.  Then a set in the middle of
    the unfinished fade: it starts where the fade stood"""
    reqs = [dict(target=[-1.0, 1.2, 2.0], fade=12), dict(target=[0.5, 1.7, 3.0], fade=0, path="arc", pivot=[0.0, 1.5, 0.1], ease="smooth"),
            [2.0, 1.0, 1.0]]
    servers = {name: _server(3, 4, gaze=dict(ease="smooth")) for name in ("many", "single")}
    state, sids = {}, {}
    for name, srv in servers.items():
        sids[name] = [srv.open(_first(3 + r), _style(31 + r)) for r in range(3)]
        srv.push_many({sid: _wav(NSAMP, 2 + r)[:8000] for r, sid in enumerate(sids[name])})
        srv.step()
        assert "ops_last_set_gaze" in srv.stats and srv.stats["ops_last_set_gaze"] == 0
        if name == "many":
            ks = srv.set_gaze_many(dict(zip(sids[name], reqs)))
            assert srv.stats["ops_last_set_gaze"] == 2
        else:
            ks = {}
            for sid, q in zip(sids[name], reqs):
                ks[sid] = srv.set_gaze(sid, **(q if isinstance(q, dict) else dict(target=q)))
                assert srv.stats["ops_last_set_gaze"] == 1
        assert list(ks.values()) == [srv._rows[r].kd for r in range(3)] == [5, 5, 5]
        state[name] = [srv.gaze(sid) for sid in sids[name]]
    for a, b, q in zip(state["many"], state["single"], reqs):
        assert set(a) == {"target", "k", "fade", "start", "end", "path", "ease"}
        for key in a:
            same = _same_rows(a[key], b[key]) if isinstance(a[key], np.ndarray) else a[key] == b[key]
            assert same, (key, a[key], b[key])
        want = q["target"] if isinstance(q, dict) else q
        assert a["end"].tolist() == np.float32(want).tolist() and a["ease"] == (q.get("ease") or "smooth" if isinstance(q, dict) else "smooth")
    assert servers["many"].set_gaze_many({}) == {} and servers["many"].stats["ops_last_set_gaze"] == 0
    with pytest.raises(KeyError, match="no open stream 99"):
        servers["many"].set_gaze_many({sids["many"][0]: [0, 0, 1], 99: [0, 0, 1]})
    with pytest.raises(ValueError, match="fade -2"):
        servers["many"].set_gaze_many({sids["many"][0]: [0, 0, 1], sids["many"][1]: dict(target=[0, 0, 1], fade=-2)})
    assert [servers["many"].gaze(sid)["k"] for sid in sids["many"]] == [5, 5, 5]          # a refused call changed nothing
    # ---- in the middle of stream 0's fade of 12
    srv, sid = servers["many"], sids["many"][0]
    srv.push_many({s: _wav(NSAMP, 2 + r)[8000:11200] for r, s in enumerate(sids["many"])})
    srv.step()
    old = dict(state["many"][0], pivot=np.zeros(3, np.float32))
    k2 = srv.set_gaze(sid, [0.0, 2.0, 2.5], fade=3, ease="linear")
    assert old["k"] < k2 - 1 < old["k"] + 12
    now = srv.gaze(sid)
    stood = oracle_gz.point(old, k2 - 1)
    print(f"k2={k2}: the new fade starts at {now['start']}, the old one stood at {stood}")
    assert _within(now["start"], stood) <= 1.0 and (now["k"], now["fade"], now["ease"]) == (k2, 3, "linear")
    assert not np.allclose(now["start"], old["start"], atol=1e-3) and not np.allclose(now["start"], old["end"], atol=1e-3)
    assert _within(now["target"], oracle_gz.point(oracle_gz.apply(old, k2, [0.0, 2.0, 2.5], fade=3), k2)) <= 1.0


# ----------------------------------------------------------------------------- 6. snapshot
def _payload(blob):
    b = np.array(blob)
    b[16:24] = 0          # the sid
    return b.tobytes()


def test_fork_in_the_middle_of_a_gaze_fade(monkeypatch):
    """a stream four frames into a gaze fade of 12 on an arc, snapshot and restored on the same server and on a second gaze
    server; the same audio to all three.  restore followed by snapshot gives the same blob; the three halves hand the decoder the
    same gaze rows bit for bit and their frames stay within the bound of the offline rollout with the oracle's track; a server
    without the stage refuses the blob naming section 'gaze' and is left as it was"""
    wav, first, style = _wav(NSAMP, 2), _first(3), _style(31)
    target, pivot = _turned(first)
    A, B, P = _server(3, 4, gaze=True), _server(2, 4, gaze=True), _server(2, 4)
    tap = _Tap(monkeypatch, A, B)
    sid = A.open(first, style)
    parts = []
    for i in range(6):
        A.push(sid, wav[1600 * i:1600 * (i + 1)])
        parts.append(A.step().get(sid))
    k = A.set_gaze(sid, target, fade=12, path="arc", pivot=pivot)
    A.push(sid, wav[9600:11200])
    parts.append(A.step().get(sid))
    assert k < A._rows[0].kd < k + 12
    blob, kd_snap = A.snapshot(sid), A._rows[0].kd
    info = live.snapshot_info(blob)
    assert info["format"] == 1 and info["version"] == 1 and len(info["fingerprint"]) == 43 and len(info["sections"]) == 15
    assert info["sections"]["gaze"][1] == live._a16(12 * A.T) + 64
    twin, far = A.restore(blob), B.restore(blob)
    assert _payload(A.snapshot(twin)) == _payload(blob) and _payload(B.snapshot(far)) == _payload(blob)
    for key in ("k", "fade", "path", "ease"):
        assert A.gaze(twin)[key] == B.gaze(far)[key] == A.gaze(sid)[key]
    for key in ("start", "end", "target"):
        assert _same_rows(A.gaze(twin)[key], A.gaze(sid)[key]) and _same_rows(B.gaze(far)[key], A.gaze(sid)[key])
    # ---- a server without the stage
    before = ([w is None for w in P._rows], P._next_sid, dict(P._sids))
    with pytest.raises(ValueError, match=r"section 'gaze' has \d+ bytes, this server's row takes \d+"):
        P.restore(blob)
    assert ([w is None for w in P._rows], P._next_sid, dict(P._sids)) == before
    ps = P.open(first, style)
    with pytest.raises(ValueError, match="section 'gaze'"):
        A.restore(P.snapshot(ps))                      # ... and the reverse
    P.close(ps)
    # ---- the three go on
    halves = {(A, sid): list(parts), (A, twin): list(parts), (B, far): list(parts)}
    for i in range(7, 20):
        for (srv, s), got in halves.items():
            srv.push(s, wav[1600 * i:1600 * (i + 1)])
        for srv in (A, B):
            while True:
                out = srv.step()
                if not out:
                    break
                for (s2, s), got in halves.items():
                    if s2 is srv:
                        got.append(out.get(s))
    n_frames = audio.n_anim_frames(NSAMP)
    track = _oracle_track(n_frames, first, [dict(k=k, target=target, fade=12, path="arc", pivot=pivot)])
    ref = _offline(wav, first, style, track)
    handed = {}
    for (srv, s), got in halves.items():
        got.append(srv.close(s))
        bound = _bound(srv)
        e = helpers.live_err(_cat(got), ref)
        print(f"{'A' if srv is A else 'B'} stream {s}: {e} (bound {bound})")
        assert max(e.values()) <= bound, e
        handed[(srv, s)] = tap.rows[(id(srv), s)]      # (a fork's frames before the snapshot were decoded by the source)
    src = handed[(A, sid)]
    for key, mine in handed.items():
        if key == (A, sid):
            continue
        frames = sorted(f for f in mine if f < n_frames)
        assert frames and frames[-1] == n_frames - 1 and frames[0] == kd_snap
        assert all(mine[f].tobytes() == src[f].tobytes() for f in frames), "a fork's gaze rows are not the source's bits"
    assert _within(np.stack([src[f] for f in range(1, n_frames)]), track[1:]) <= 1.0


# ----------------------------------------------------------------------------- 7. the stage off costs nothing
@pytest.mark.parametrize("rows", [1, 3])
def test_the_stage_costs_nothing_where_it_is_not_used(rows):
    """the same streams through a server with gaze=True on which set_gaze is never called and through one built without: the
    frames agree within 2e-5, the gaze server's launches_per_step is at most the plain server's, and the plain server holds no
    gaze state and no counter of the stage"""
    specs = [dict(wav=_wav(NSAMP, 2 + r), first=_first(3 + r), style=_style(31 + r)) for r in range(rows)]
    out, launches = {}, {}
    for name, kw in (("gaze", dict(gaze=True)), ("plain", {})):
        srv = _server(rows, 4, **kw)
        runs = _drive(srv, specs, [1600] * 20, many=rows > 1)
        out[name], launches[name] = [run["frames"] for run in runs], srv.stats["launches_per_step"]
        if name == "plain":
            assert srv._gz is None and srv._gz_style is None and srv._gz_set is None and srv._gz_cond is None and srv.gaze_conf is None
            assert "ops_last_set_gaze" not in srv.stats
            for call in (lambda: srv.set_gaze(0, [0, 0, 1]), lambda: srv.set_gaze_many({}), lambda: srv.gaze(0)):
                with pytest.raises(ValueError, match=r"LiveServer\(gaze=True\)"):
                    call()
    print(f"rows={rows}: launches per step {launches}")
    assert launches["gaze"] <= launches["plain"]
    for a, b in zip(out["gaze"], out["plain"]):
        for key in KEYS:
            assert float((a[key] - b[key]).abs().max()) <= 2e-5, key
