"""Live serving, named styles (LiveServer(styles=...), add_style / set_style / set_style_many / style; include/zeggs_hip_styles.h).
The yardsticks are the numpy float64 oracle tests/live_styles_oracle.py (written from the definition), torch.lerp for the collapse
of an unfinished fade, the offline style encoder call style_net(example, t, eps) for a bank entry, and a twin server that is
handed the same vectors as tensors through the calls that were there before; never the new code against itself.

Bounds: a mixed row 1/2 ulp32(want) + 2^-48 sum |w v| (one rounding at the store, at most 8 float64 roundings with room to
spare); a slot's deviation 2 float32 ulp of exp(logvar / 2) in float64 (expf's own error and the rounding of the float64 value); a
one-term mix against the offline z: 2^-21 (|mu| + |eps dev / t|) (three float32 roundings and a division there, one rounding
here); frames: the bound of the existing gaze tests."""
import numpy as np
import pytest
import torch

import helpers
import live_styles_oracle as oracle_sb
from zeggs import anim, audio, live, ops, synth
from zeggs.generate import _example_features

pytestmark = pytest.mark.gpu
DEV = helpers.LIVE_DEV
KEYS = helpers.LIVE_KEYS
NSAMP = 16000
ST = 64
_first, _wav, _style, _server, _cat = helpers.live_first, helpers.live_wav, helpers.live_style, helpers.live_server, helpers.live_cat
FADES = ((12, 4), (8, 9), (4, 7), (3, 0))          # (k_style, fade) of the OLD fade at k = 10: weight 0, 2 / 10, 6 / 8 and 1 at frame 9


# ----------------------------------------------------------------------------- helpers
def _bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes()


def _upload(recs):
    return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(DEV)


def _bound(srv):
    """the live bound of the gaze tests: helpers.live_bound where the rows rode the batched decoder call, the B = 1 bound otherwise"""
    return 5e-5 if srv.rows == 1 else helpers.live_bound(srv)


def _style_net():
    return helpers._live_cached("style_net", lambda: helpers.build_nets()[2].to(DEV).eval())


def _push_all(srv, wavs, lo, hi):
    srv.push_many({sid: w[lo:hi] for sid, w in wavs.items()})


# ----------------------------------------------------------------------------- 1. the mix launch alone
@pytest.mark.parametrize("capacity", [1, 5])
@pytest.mark.parametrize("st", [1, 63, 64, 65, 257])
def test_the_mix_launch_alone(st, capacity):
    """a state of 64 rows; calls of R = 1 (the record in the arguments), 3 and 64 records (uploaded) of 1, 2 and 8 terms, with and
    without noise, the old fade at weight 0, between (below and above 1/2) and 1, some with `reset`; the bank's last slot is used.
    sty_new' against the oracle within the derived bound, sty_old' bit for bit torch.lerp of the same float32 inputs (or sty_new'
    under reset); rows no record names (poisoned with NaN), every bank slot and the whole noise tensor bit for bit what they were"""
    rows, gen, rng = 64, torch.Generator(DEV).manual_seed(100 * st + capacity), np.random.default_rng(st + capacity)
    ls = ops.LiveStyles(rows, st, capacity, DEV)
    ls.bank.copy_(torch.randn(capacity, 2, st, device=DEV, generator=gen))
    ls.bank[:, 1].abs_()
    bank_was, bank = _bits(ls.bank), ls.bank.cpu().numpy()
    worst = 0.0
    for R in (1, 3, 64):
        named = sorted(rng.permutation(rows)[:R].tolist(), key=lambda r: (r * 7) % 11)       # (not in row order)
        sty_old, sty_new = (torch.randn(rows, st, device=DEV, generator=gen) * 0.5 for _ in range(2))
        ls.eps.copy_(torch.randn(rows, ops.STYLE_MAX_TERMS, st, device=DEV, generator=gen))
        jobs = []
        for i, r in enumerate(named):
            n = (1, 2, 8)[(i + R) % 3]
            slots = [capacity - 1 if j == 0 and i % 2 == 0 else int(rng.integers(capacity)) for j in range(n)]
            wts = [float(np.float32(w)) for w in rng.standard_normal(n)]
            jobs.append(dict(row=r, slots=slots, wts=wts, t=(0.0, 0.7, 1.0, 2.5)[(i + R) % 4], noise=i % 3 != 2, fade=FADES[i % 4],
                             reset=i % 5 == 4))
        idle = [r for r in range(rows) if r not in named]
        for r in idle:
            sty_old[r].fill_(float("nan"))
            sty_new[r].fill_(float("nan"))
        for job in jobs:                                  # the noise rows a record does not name are poison too
            if not (job["noise"] and job["t"] > 0):
                ls.eps[job["row"]].fill_(float("nan"))
            else:
                ls.eps[job["row"], len(job["slots"]):].fill_(float("nan"))
        for r in idle:
            ls.eps[r].fill_(float("nan"))
        old_was, new_was, eps_was, eps = sty_old.clone(), sty_new.clone(), _bits(ls.eps), ls.eps.cpu().numpy()
        recs = (ops.StyleMix * R)()
        for q, job in zip(recs, jobs):
            n = len(job["slots"])
            q.slot[:], q.weight[:] = job["slots"] + [0] * (8 - n), job["wts"] + [0.0] * (8 - n)
            q.k, (q.k_style, q.fade_style), q.row, q.terms, q.reset = 10, job["fade"], job["row"], n, int(job["reset"])
            q.temperature, q.eps_row = job["t"], job["row"] if job["noise"] else -1
        keep = _upload(recs)
        ops.live_style_mix(ls, recs, R, sty_old, sty_new, keep.data_ptr() if R > 1 else None)
        got_old, got_new = sty_old.cpu().numpy(), sty_new.cpu().numpy()
        for job in jobs:
            r = job["row"]
            want, mag = oracle_sb.mix(bank, list(zip(job["slots"], job["wts"])), job["t"], eps[r] if job["noise"] else None)
            err, bound = np.abs(got_new[r].astype(np.float64) - want), oracle_sb.bound(want, mag)
            worst = max(worst, float((err / bound).max()))
            assert np.isfinite(got_new[r]).all() and (err <= bound).all(), (R, job, float((err / bound).max()))
            if job["reset"]:
                assert _same(got_old[r], got_new[r]), (R, job)
            else:
                w = live.style_weight(10 - 1, *job["fade"])
                lerp = torch.lerp(old_was[r], new_was[r], w)
                assert torch.equal(_bits(sty_old[r]), _bits(lerp)), (R, job, w, float((sty_old[r] - lerp).abs().max()))
                if w in (0.0, 1.0):
                    assert torch.equal(_bits(sty_old[r]), _bits(old_was[r] if w == 0.0 else new_was[r]))
        for r in idle:
            assert torch.equal(_bits(sty_old[r]), _bits(old_was[r])) and torch.equal(_bits(sty_new[r]), _bits(new_was[r])), f"idle row {r} was touched"
        assert torch.equal(_bits(ls.bank), bank_was), "the bank was written by a mix"
        assert torch.equal(_bits(ls.eps), eps_was), "the noise tensor was written by a mix"
    print(f"ST={st} capacity={capacity}: a mixed value is at worst {worst:.3f} of the bound")
    assert worst <= 1.0


# ----------------------------------------------------------------------------- 2. put
@pytest.mark.parametrize("st", [1, 64, 257])
def test_put_writes_one_slot(st):
    """a VAE row into the last slot: the mean is the row's first half bit for bit, the deviation within 2 float32 ulp of
    exp(logvar / 2) in float64; a plain vector into slot 1: the mean is the vector, the deviation 0; every other slot (NaN) is
    bit for bit what it was"""
    gen = torch.Generator(DEV).manual_seed(st)
    ls = ops.LiveStyles(2, st, 4, DEV)
    ls.bank.fill_(float("nan"))
    enc = torch.randn(2 * st, device=DEV, generator=gen) * torch.cat([torch.ones(st, device=DEV), 3.0 * torch.ones(st, device=DEV)])
    vec = torch.randn(st, device=DEV, generator=gen)
    ops.live_style_put(ls, 3, enc)
    ops.live_style_put(ls, 1, vec)
    mean, dev = ops.live_style_read(ls, slot=3)
    assert _same(mean, enc[:st].cpu().numpy())
    want = np.exp(0.5 * enc[st:].cpu().numpy().astype(np.float64))
    err = np.abs(dev.astype(np.float64) - want) / oracle_sb.ulp32(want)
    print(f"ST={st}: the deviation is at worst {err.max():.3f} ulp from exp(logvar / 2)")
    assert (err <= 2.0).all()
    mean, dev = ops.live_style_read(ls, slot=1)
    assert _same(mean, vec.cpu().numpy()) and _same(dev, np.zeros(st, np.float32))
    assert torch.isnan(ls.bank[0]).all() and torch.isnan(ls.bank[2]).all()
    assert torch.equal(_bits(ls.bank[3, 0]), _bits(enc[:st])) and torch.equal(_bits(ls.bank[1, 0]), _bits(vec))


# ----------------------------------------------------------------------------- 3. one exemplar, offline against live
@pytest.mark.parametrize("trim", [None, (20, 97)], ids=["whole", "trimmed"])
def test_an_example_equals_the_offline_style_encoder(trim):
    """a synthetic clip of 128 frames, whole and trimmed to 77, through add_style() and through the calls the offline front end
    makes (anim.preprocess_animation, the exemplar feature rows, the normalisation, style_net(ex[None], t, eps)) -- with the
    encoder's products in a fixed summation order (ops.fixed_order_gemms, as add_style() runs them and as evaluate() does:
    split over workgroups they add up by atomics and the last place differs from run to run): the slot's mean is the offline
    mu bit for bit; a one-term mix at weight 1 with temperature t and the same eps (set_style(..., temperature=t,
    seed=s) draws ops.randn((1, ST), seed=s)) is within 2^-21 (|mu| + |eps dev / t|) of the offline z; with temperature None the
    row is mu"""
    net, t, seed = _style_net(), 0.8, 4321
    srv = _server(2, 4, styles=dict(net=net, capacity=3))
    clip = synth.make_bvh_clip(128, seed=9)
    slot = srv.add_style("example", clip, trim=trim)
    assert slot == 0 and srv.styles() == dict(example=0) and clip["rotations"].shape[0] == 128      # the caller's clip is not cut
    ref = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in clip.items()}
    if trim is not None:
        ref["rotations"], ref["positions"] = ref["rotations"][trim[0]:trim[1]], ref["positions"][trim[0]:trim[1]]
    st = helpers.live_stats()
    with torch.no_grad():
        ex = (_example_features(anim.preprocess_animation(ref, DEV)) - st["anim_input_mean"]) / st["anim_input_std"]
        assert ex.shape == (128 if trim is None else 77, synth.POSE_IN)
        eps = ops.randn((1, ST), DEV, seed=seed)
        with ops.fixed_order_gemms():
            z, mu, logvar = net(ex[None].contiguous(), t, eps)
    mean, dev = ops.live_style_read(srv._sb, slot=slot)
    assert _same(mean, mu[0].cpu().numpy()), float(np.abs(mean - mu[0].cpu().numpy()).max())
    want_dev = np.exp(0.5 * logvar[0].cpu().numpy().astype(np.float64))
    assert (np.abs(dev.astype(np.float64) - want_dev) <= 2.0 * oracle_sb.ulp32(want_dev)).all()
    sid = srv.open(_first(3), "example")
    got = srv.style(sid)
    assert _same(got["new"], mean) and _same(got["old"], mean) and _same(got["current"], mean) and (got["k"], got["fade"]) == (0, 0)
    assert srv.set_style(sid, "example", temperature=t, seed=seed) == 1 and srv.stats["ops_last_set_style"] == 2
    got = srv.style(sid)
    assert _same(srv._sb.eps[0, 0].cpu().numpy(), eps[0].cpu().numpy())
    term = eps[0].cpu().numpy().astype(np.float64) * dev.astype(np.float64) / float(np.float32(t))
    bound = 2.0 ** -21 * (np.abs(mean.astype(np.float64)) + np.abs(term))
    err = np.abs(got["new"].astype(np.float64) - z[0].cpu().numpy().astype(np.float64))
    print(f"{'whole' if trim is None else 'trimmed'}: the sampled row is at worst {(err / bound).max():.3f} of the bound from the offline z")
    assert (err <= bound).all() and float(np.abs(got["new"] - mean).max()) > 1e-3
    assert _same(got["old"], mean)                                   # the fade before it had ended: the old row is where it stood
    # the same name from a vector overwrites the slot; the row keeps what it was given
    assert srv.add_style("example", torch.arange(ST, dtype=torch.float32)) == 0
    assert _same(srv.style(sid)["new"], got["new"])
    assert _same(ops.live_style_read(srv._sb, slot=0)[1], np.zeros(ST, np.float32))


def test_exemplar_rows_take_the_same_route():
    """un-normalised exemplar rows [L, F] give the slot the clip they were made of gives, bit for bit; trimmed rows are the rows
    cut by hand; a tensor and an array are the same source"""
    net = _style_net()
    srv = _server(1, 4, styles=dict(net=net, capacity=4, terms=2))
    clip = synth.make_bvh_clip(64, seed=5)
    with torch.no_grad():
        rows = _example_features(anim.preprocess_animation({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in clip.items()}, DEV))
    a, b = srv.add_style("clip", clip), srv.add_style("rows", rows)
    assert (a, b) == (0, 1)
    for x, y in zip(ops.live_style_read(srv._sb, slot=a), ops.live_style_read(srv._sb, slot=b)):
        assert _same(x, y)
    b, c = srv.add_style("rows", rows, trim=(3, 60)), srv.add_style("rows again", rows[3:60].cpu().numpy())
    assert (b, c) == (1, 2)
    for x, y in zip(ops.live_style_read(srv._sb, slot=b), ops.live_style_read(srv._sb, slot=c)):
        assert _same(x, y)
    assert not _same(ops.live_style_read(srv._sb, slot=a)[0], ops.live_style_read(srv._sb, slot=b)[0])
    with pytest.raises(ValueError, match=r"exemplar rows are \[L, 1134\]"):
        srv.add_style("bad", rows[:, :100])
    sid = srv.open(_first(3), "clip")
    with pytest.raises(ValueError, match="3 terms"):
        srv.set_style_many({sid: {"clip": 1, "rows": 1, "rows again": 1}})


# ----------------------------------------------------------------------------- 4. many equals singles, rows are independent
def _bank_server(rows, tick=4, n=5, **kw):
    """a server whose bank holds s0 .. s{n-1}: the even ones from encoder rows (mean | log-variance), the odd ones from vectors"""
    srv = _server(rows, tick, styles=dict(capacity=n, terms=8), **kw)
    for i in range(n):
        vec = _style(50 + i).reshape(-1)
        assert srv.add_style(f"s{i}", vec if i % 2 else torch.cat([vec, _style(70 + i).reshape(-1)])) == i
    assert srv.styles() == {f"s{i}": i for i in range(n)}
    return srv


def _row_state(srv, sid):
    r, row = srv._row(sid)
    return srv.sty_old[r].cpu().numpy(), srv.sty_new[r].cpu().numpy(), row.k_style, row.fade


def test_set_style_many_is_the_same_calls_one_by_one():
    """three streams, one set_style_many on one server and three set_style calls on its twin, in the middle of an earlier fade:
    the same k, sty_old, sty_new, k_style and fade bit for bit; two operations for the three when nobody samples (three when one
    does), one for a single call.  Then all 64 rows of a server in one call against each row alone on its twin"""
    reqs = [dict(style={"s0": 0.3, "s3": 0.7}, fade=12), dict(style=[("s4", 1.0), ("s4", -0.5), ("s1", 0.25)], fade=0, temperature=0.9, seed=11),
            "s2"]
    servers = {name: _bank_server(3) for name in ("many", "single")}
    state = {}
    for name, srv in servers.items():
        sids = [srv.open(_first(3 + r), f"s{r}") for r in range(3)]
        _push_all(srv, {sid: _wav(NSAMP, 2 + r) for r, sid in enumerate(sids)}, 0, 8000)
        srv.step()
        assert srv.stats["ops_last_set_style"] == 0
        for sid in sids:                                  # an earlier fade of 12 from frame 5 on, still under way below
            assert srv.set_style(sid, {"s1": 0.5, "s2": 0.5}, fade=12) == 5 and srv.stats["ops_last_set_style"] == 1
        _push_all(srv, {sid: _wav(NSAMP, 2 + r) for r, sid in enumerate(sids)}, 8000, 9600)
        srv.step()
        if name == "many":
            ks = srv.set_style_many(dict(zip(sids, reqs)))
            assert srv.stats["ops_last_set_style"] == 3                    # the upload, the launch, one noise launch
            assert srv.set_style_many({}) == {} and srv.stats["ops_last_set_style"] == 0
        else:
            ks = {}
            for sid, q in zip(sids, reqs):
                ks[sid] = srv.set_style(sid, **q) if isinstance(q, dict) else srv.set_style(sid, q)
                assert srv.stats["ops_last_set_style"] == (2 if isinstance(q, dict) and q.get("temperature") else 1)
        assert list(ks.values()) == [srv._rows[r].kd for r in range(3)] and 5 < ks[sids[0]] - 1 < 5 + 12
        state[name] = [_row_state(srv, sid) for sid in sids]
    for a, b, q in zip(state["many"], state["single"], reqs):
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and a[2:] == b[2:] == (ks[sids[0]], q["fade"] if isinstance(q, dict) else 0)
        assert not _same(a[0], a[1])
    srv = servers["many"]
    with pytest.raises(KeyError, match="no open stream 99"):
        srv.set_style_many({sids[0]: "s0", 99: "s1"})
    with pytest.raises(ValueError, match="no style 'nope'"):
        srv.set_style_many({sids[0]: "s0", sids[1]: "nope"})
    assert all(_same(x[1], _row_state(srv, sid)[1]) for x, sid in zip(state["many"], sids))          # a refused call changed nothing
    # ---- two-term mixes for everybody: two operations whatever the number of rows
    srv.set_style_many({sid: {"s0": 0.5, "s1": 0.5} for sid in sids})
    assert srv.stats["ops_last_set_style"] == 2
    # ---- 64 rows in one call against each row alone
    big, lone = _bank_server(64), _bank_server(64)
    rng = np.random.default_rng(8)
    first = _first(3)
    req = {}
    for srv in (big, lone):
        sids = [srv.open(first, "s0") for _ in range(64)]
    for sid in sids:
        names = [f"s{int(j)}" for j in rng.integers(0, 5, size=int(rng.integers(1, 9)))]
        req[sid] = dict(style=[(n, float(w)) for n, w in zip(names, rng.standard_normal(len(names)))], fade=int(rng.integers(0, 20)))
        if sid % 4 == 1:
            req[sid].update(temperature=1.1, seed=1000 + sid)
    big.set_style_many(req)
    assert big.stats["ops_last_set_style"] == 2 + 16
    for sid, q in req.items():
        lone.set_style(sid, **q)
    for sid in sids:
        a, b = _row_state(big, sid), _row_state(lone, sid)
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and a[2:] == b[2:], sid


# ----------------------------------------------------------------------------- 5. continuity
def test_a_named_style_in_the_middle_of_a_fade_starts_where_the_fade_stood():
    """a gaze server (its condition launch writes the style rows the decoder is handed): a fade of 12 between two bank entries,
    two steps into it a named set_style -- the style row the server emitted for frame k - 1 is sty_old after the call, bit for
    bit, and lies strictly between the two entries"""
    srv = _bank_server(3, gaze=True)
    sid = srv.open(_first(3), "s1")
    wav = _wav(NSAMP, 2)
    srv.push(sid, wav[:8000])
    srv.step()
    k1 = srv.set_style(sid, "s3", fade=12)
    srv.push(sid, wav[8000:9600])
    srv.step()
    r, row = srv._row(sid)
    assert k1 < row.kd - 1 < k1 + 12
    emitted = srv._gz_style[r, srv.T - 1].clone()             # the last frame of the last decoder call: frame kd - 1
    before = srv.style(sid)
    k2 = srv.set_style(sid, {"s0": 0.5, "s4": 0.5}, fade=3)
    assert k2 == row.kd
    after = srv.style(sid)
    assert torch.equal(_bits(srv.sty_old[r]), _bits(emitted)), float((srv.sty_old[r] - emitted).abs().max())
    assert _same(after["old"], emitted.cpu().numpy()) and (after["k"], after["fade"]) == (k2, 3)
    lo, hi = np.minimum(before["old"], before["new"]), np.maximum(before["old"], before["new"])
    moved = np.abs(before["new"] - before["old"]) > 1e-3
    assert ((after["old"] > lo) & (after["old"] < hi))[moved].all()
    # style(sid)["current"]: the row of frame kd, which the next step emits at index 1 of its call
    srv.push(sid, wav[9600:11200])
    cur = srv.style(sid)["current"]
    srv.step()
    got = srv._gz_style[r, 1].cpu().numpy()
    assert (np.abs(got.astype(np.float64) - cur) <= oracle_sb.ulp32(got)).all() and not _same(got, after["old"])


# ----------------------------------------------------------------------------- 6. the server, end to end
class _StyleTap:
    """records the style rows every batched decoder call of the given servers is handed, per stream and frame"""

    def __init__(self, monkeypatch, *servers):
        self.servers, self.rows = list(servers), {}
        chunk, batch = ops.decoder_chunk, ops.decoder_batch_chunk

        def tapped_chunk(decoder, pose, rpos, rrot, gaze, speech, style, *a, **kw):
            for s in self.servers:
                off = pose.data_ptr() - s.pose.data_ptr()
                if 0 <= off < 4 * s.pose.numel():
                    self._note(s, off // (4 * s.pose.shape[1]), style[0])
            return chunk(decoder, pose, rpos, rrot, gaze, speech, style, *a, **kw)

        def tapped_batch(bd, pose, rpos, rrot, gaze, speech, style, *a, **kw):
            for s in self.servers:
                if s.bd is bd:
                    for r in range(s.rows):
                        self._note(s, r, style[r])
            return batch(bd, pose, rpos, rrot, gaze, speech, style, *a, **kw)
        monkeypatch.setattr(ops, "decoder_chunk", tapped_chunk)
        monkeypatch.setattr(ops, "decoder_batch_chunk", tapped_batch)

    def _note(self, s, r, rows):
        row = s._rows[r]
        if row is None:
            return
        rows = rows.detach().cpu().numpy()
        mine = self.rows.setdefault((id(s), row.sid), {})
        for i in range(1, rows.shape[0]):
            mine[row.kd - 1 + i] = rows[i].copy()

    def of(self, s, sid):
        return self.rows[(id(s), sid)]


@pytest.mark.parametrize("gaze", [False, True], ids=["plain", "gaze"])
@pytest.mark.parametrize("rows", [1, 3])
def test_a_bank_server_equals_its_twin_with_tensors(monkeypatch, rows, gaze):
    """`rows` streams opened by name and re-styled with a two-term mix and a fade of 12 in the middle of the audio, on a bank
    server; its twin without a bank is given the vectors style(sid) read back, as tensors, at the same frames.  The style rows the
    decoder is handed are the same bits, the frames agree within the live bound, launches_per_step is the twin's"""
    kw = dict(gaze=True) if gaze else {}
    bank, twin = _bank_server(rows, **kw), _server(rows, 4, **kw)
    tap = _StyleTap(monkeypatch, bank, twin)
    wavs = [_wav(NSAMP, 2 + r) for r in range(rows)]
    mixes = [{"s0": 0.3, "s3": 0.7}, {"s4": 1.25, "s1": -0.25}, [("s2", 0.5), ("s0", 0.5)]][:rows]
    n_frames = audio.n_anim_frames(NSAMP)
    frames, vectors, launches = {}, {}, {}
    for name, srv in (("bank", bank), ("twin", twin)):
        if name == "bank":
            sids = [srv.open(_first(3 + r), f"s{r}") for r in range(rows)]
            vectors["open"] = [srv.style(sid)["new"] for sid in sids]
        else:
            sids = [srv.open(_first(3 + r), torch.as_tensor(v)[None]) for r, v in enumerate(vectors["open"])]
        parts = {sid: [] for sid in sids}
        for i in range(NSAMP // 1600):
            if i == 5:
                if name == "bank":
                    ks = srv.set_style_many({sid: dict(style=m, fade=12) for sid, m in zip(sids, mixes)})
                    vectors["set"], vectors["k"] = [srv.style(sid)["new"] for sid in sids], ks
                else:
                    ks = {sid: srv.set_style(sid, torch.as_tensor(v), fade=12) for sid, v in zip(sids, vectors["set"])}
                    assert ks == vectors["k"]
            if rows == 1:
                srv.push(sids[0], wavs[0][1600 * i:1600 * (i + 1)])
            else:
                _push_all(srv, dict(zip(sids, wavs)), 1600 * i, 1600 * (i + 1))
            while True:
                out = srv.step()
                if not out:
                    break
                for sid in sids:
                    parts[sid].append(out.get(sid))
            if i == 7:
                launches[name] = srv.stats["launches_per_step"]
        bound = _bound(srv)
        for sid in sids:
            parts[sid].append(srv.close(sid))
        frames[name] = [_cat(parts[sid]) for sid in sids]
        vectors[name + " sids"] = sids
    print(f"rows={rows} gaze={gaze}: launches per step {launches}")
    assert launches["bank"] == launches["twin"]
    for r in range(rows):
        a, b = ({f: v for f, v in tap.of(s, vectors[name + " sids"][r]).items() if f < n_frames} for s, name in ((bank, "bank"), (twin, "twin")))
        assert set(a) == set(b) == set(range(1, n_frames))
        k = vectors["k"][vectors["bank sids"][r]]
        assert all(a[f].tobytes() == b[f].tobytes() for f in a), f"row {r}: the style rows are not the twin's bits"
        assert _same(a[k - 1], vectors["open"][r]) and _same(a[k + 12], vectors["set"][r]) and not _same(a[k + 3], a[k + 4])
        e = helpers.live_err(frames["bank"][r], tuple(frames["twin"][r][key] for key in KEYS))
        print(f"  row {r}: {e} (bound {bound})")
        assert max(e.values()) <= bound, e


# ----------------------------------------------------------------------------- 7. snapshots
def _payload(blob):
    b = np.array(blob)
    b[16:24] = 0          # the sid
    return b.tobytes()


def test_a_snapshot_moves_between_a_bank_server_and_a_plain_one(monkeypatch):
    """a stream four frames into a fade between two bank entries, snapshot on the bank server and restored on a plain server of
    the same configuration -- and a stream of the plain server, in a fade between two tensors, restored on the bank server.  The
    blobs have the sections and the sizes they had before there was a bank, restore followed by snapshot gives the same bytes,
    and source and copy hand the decoder the same style rows bit for bit in every later step"""
    A, P = _bank_server(2), _server(2, 4)
    tap = _StyleTap(monkeypatch, A, P)
    wav, first = _wav(NSAMP, 2), _first(3)
    a = A.open(first, "s0")
    p = P.open(first, _style(31))
    for i in range(5):
        A.push(a, wav[1600 * i:1600 * (i + 1)])
        P.push(p, wav[1600 * i:1600 * (i + 1)])
        A.step(), P.step()
    ka, kp = A.set_style(a, {"s1": 0.5, "s3": 0.5}, fade=12), P.set_style(p, _style(32), fade=12)
    A.push(a, wav[8000:9600]), P.push(p, wav[8000:9600])
    A.step(), P.step()
    assert ka < A._rows[0].kd < ka + 12 and kp == ka
    blob_a, blob_p = A.snapshot(a), P.snapshot(p)
    for blob in (blob_a, blob_p):
        info = live.snapshot_info(blob)
        assert info["format"] == 1 and info["version"] == 1 and len(info["fingerprint"]) == 43 and len(info["sections"]) == 15
        assert info["sections"]["sty_old"][1] == info["sections"]["sty_new"][1] == 4 * ST
    assert len(blob_a) == len(blob_p)                          # the same stream position: the bank adds nothing to a blob
    a_on_p, p_on_a = P.restore(blob_a), A.restore(blob_p)
    assert _payload(P.snapshot(a_on_p)) == _payload(blob_a) and _payload(A.snapshot(p_on_a)) == _payload(blob_p)
    assert A.style(p_on_a)["k"] == kp and _same(A.style(p_on_a)["new"], _style(32).reshape(-1).cpu().numpy())
    kd_snap = A._rows[0].kd
    for i in range(6, NSAMP // 1600):
        for srv, sids in ((A, (a, p_on_a)), (P, (p, a_on_p))):
            for sid in sids:
                srv.push(sid, wav[1600 * i:1600 * (i + 1)])
            while srv.step():
                pass
    for src, copy in (((A, a), (P, a_on_p)), ((P, p), (A, p_on_a))):
        x, y = tap.of(*src), tap.of(*copy)
        later = sorted(f for f in y if f >= kd_snap)
        assert later and later[0] == kd_snap and len(later) >= 12 and set(later) <= set(x)
        assert all(x[f].tobytes() == y[f].tobytes() for f in later), "the copy's style rows are not the source's bits"
        assert not _same(x[later[0]], x[later[3]])             # (the fade was still moving)
    # a named set_style on the stream that came from the plain server: the bank serves a restored row like any other
    assert A.set_style(p_on_a, "s2") == A._row(p_on_a)[1].kd


# ----------------------------------------------------------------------------- 8. the stage off costs nothing
@pytest.mark.parametrize("rows", [1, 3])
def test_the_bank_costs_nothing_where_it_is_not_used(rows):
    """the same streams through a server with styles=True on which no name is ever used and through one built without: the same
    launches per step, frames within 2e-5; the plain server holds no bank, no noise tensor, no staging block and no counter of
    the stage, and every call of the stage names the option; what the bank server holds beside is the bank, the rows' noise and
    the records' staging block"""
    out, launches = {}, {}
    for name, kw in (("bank", dict(styles=True)), ("plain", {})):
        srv = _server(rows, 4, **kw)
        sids = [srv.open(_first(3 + r), _style(31 + r)) for r in range(rows)]
        parts = {sid: [] for sid in sids}
        for i in range(NSAMP // 1600):
            _push_all(srv, {sid: _wav(NSAMP, 2 + r) for r, sid in enumerate(sids)}, 1600 * i, 1600 * (i + 1))
            if i == 5:
                for r, sid in enumerate(sids):
                    srv.set_style(sid, _style(41 + r), fade=6)           # a tensor: the path that was always there
            while True:
                o = srv.step()
                if not o:
                    break
                for sid in sids:
                    parts[sid].append(o.get(sid))
        launches[name] = srv.stats["launches_per_step"]
        out[name] = [_cat(parts[sid] + [srv.close(sid)]) for sid in sids]
        if name == "plain":
            assert srv._sb is None and srv._sb_set is None and srv.styles_conf is None and srv._style_names == {}
            assert "ops_last_set_style" not in srv.stats
            for call in (lambda: srv.set_style(0, "calm"), lambda: srv.set_style_many({}), lambda: srv.style(0), lambda: srv.styles(),
                         lambda: srv.add_style("calm", np.zeros(ST, np.float32)), lambda: srv.remove_style("calm"),
                         lambda: srv.open(_first(3), "calm")):
                with pytest.raises(ValueError, match=r"LiveServer\(styles=True\)"):
                    call()
        else:
            assert srv.stats["ops_last_set_style"] == 0 and srv.styles() == {}
            assert srv._sb.bank.shape == (64, 2, ST) and srv._sb.eps.shape == (rows, 8, ST) and srv._sb_set.dev.numel() == rows * 112
    print(f"rows={rows}: launches per step {launches}")
    assert launches["bank"] == launches["plain"]
    for a, b in zip(out["bank"], out["plain"]):
        for key in KEYS:
            assert float((a[key] - b[key]).abs().max()) <= 2e-5, key
