"""LiveServer.push_many and what it stands on (include/zeggs_hip_live.h): zeggs_mel_features_batch, zeggs_copy_segments.
Yardsticks are the existing per-row paths -- zeggs_mel_features_window for the features (bitwise), LiveServer.push() for the
server (bitwise features and counters; frames within the bound of tests/test_gpu_live.py for the decoder path that ran)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers
from zeggs import anim, audio, capi, live, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("pose", "rpos", "rrot")
CONF = dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True, normalize_mel_bins=True,
            normalize_range=True, min_clipping=1e-5, sampling_rate=16000, mel_fmin=20, mel_fmax=7600,
            n_mel_channels=80, filter_length=800, hop_length=200, resample_method="linear", normalize_loudness=False)


@pytest.fixture
def restore_options():
    yield
    for k, v in (("mel_fft", 1), ("mel_mfma", 1)):
        ops.set_option(k, v)


@functools.lru_cache(maxsize=None)
def _nets():
    se, de, _ = helpers.build_nets()
    return se.to(DEV).eval(), de.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _stats():
    return {k: torch.as_tensor(np.asarray(v), dtype=torch.float32, device=DEV) for k, v in synth.make_stats().items()}


@functools.lru_cache(maxsize=None)
def _first(seed):
    return anim.preprocess_animation(synth.make_bvh_clip(8, seed=seed), DEV)


@functools.lru_cache(maxsize=None)
def _wav(nsamp, seed):
    return synth.synth_wav(nsamp, seed=seed).astype(np.float32) / 32768.0


def _style(seed):
    return torch.randn(1, 64, device=DEV, generator=torch.Generator(DEV).manual_seed(seed)) * 0.5


def _server(rows, tick, **kw):
    se, de = _nets()
    return live.LiveServer(se, de, _stats(), CONF, synth.DT, rows=rows, tick=tick, **kw)


def _cat(parts):
    parts = [p for p in parts if p]
    return {k: torch.cat([p[k] for p in parts], dim=0) for k in KEYS}


def _bound(srv):
    """tests/test_gpu_live.py::_bound: 1e-4 where the rows rode the sweep, 5e-5 otherwise -- which of the two ran is asserted"""
    path = ops.batch_last_path()
    assert path == ("persistent" if srv.bd.sweep else "stage"), (path, srv.bd.sweep)
    return 1e-4 if path == "persistent" else 5e-5


def _mel_dims(pe=False, flags=None):
    g = CONF
    fb, min_clip = audio.mel_tables(g["filter_length"], 16000, 80, g["mel_fmin"], g["mel_fmax"], g["min_clipping"], True, True, DEV)
    d = audio.MelDims(800, 200, 80, 16000, 60.0, float(min_clip), 0.97 if pe else 0.0,
                      audio.mel_flags(True, True, "linear") if flags is None else flags)
    return d, fb


def _to_device(records):
    return torch.frombuffer(bytearray(records), dtype=torch.uint8).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- 1. the batched front-end == the per-row one
def _batch_cases():
    """(samples, signal seed, k0, k1 or None = as far as the signal allows, final) -- see the test's docstring"""
    return [(40123, 1, 0, None, 0), (20000, 2, 40, None, 1), (30000, 3, 17, None, 0), (12000, 4, 30, 31, 0), (6000, 5, 3, 6, 0),
            (9000, 6, 11, 11, 0)]


def _batch_rows(d, guard=1):
    """the six rows on the device: windows that start exactly at zeggs_mel_window_first_sample(k0), outputs pre-filled with 7.0
    with `guard` rows behind them -> (records, windows, outputs, [(base, n, final, k0, k1)])"""
    recs, wins, outs, args = (capi.MelRow * 6)(), [], [], []
    for i, (n, seed, k0, k1, final) in enumerate(_batch_cases()):
        if k1 is None:
            k1 = audio.n_anim_frames(n) if final else ops.mel_frames_ready(d, n)
        base = ops.mel_window_first_sample(d, k0)
        wins.append(torch.as_tensor(_wav(n, seed), device=DEV)[base:].clone())
        outs.append(torch.full((k1 - k0 + guard, 81), 7.0, device=DEV))
        q = recs[i]
        q.wav, q.out, q.base, q.n_samples, q.k0, q.k1, q.final = wins[i].data_ptr(), outs[i].data_ptr(), base, n, k0, k1, final
        args.append((base, n, final, k0, k1))
    return recs, wins, outs, args


@pytest.mark.parametrize("form,pe", [("fft", False), ("fft", True), ("fallback", False), ("fallback", True)])
def test_mel_batch_equals_mel_window_row_by_row(form, pe, restore_options):
    """six rows in ONE zeggs_mel_features_batch: k0 = 0 (left reflection), final = 1 up to n_anim_frames (right reflection), a window
    that starts exactly at zeggs_mel_window_first_sample(17), one feature frame, five STFT frames (a partial last block of 4),
    k1 == k0 (takes no part) -- every row bit-identical to zeggs_mel_features_window with the same arguments, the guard row behind
    each output and the idle row's output untouched; with the records uploaded by the caller and by the library; on the FFT form
    (2 launches) and with mel_fft = 0 (the per-row path inside the call)"""
    ops.set_option("mel_fft", 1 if form == "fft" else 0)
    d, fb = _mel_dims(pe)
    recs, wins, outs, args = _batch_rows(d)
    assert args[4][4] - args[4][3] == 3 and args[3][4] - args[3][3] == 1 and args[0][0] == 0 and args[2][0] > 0
    refs = []
    for (base, n, final, k0, k1), win in zip(args, wins):
        if k1 == k0:
            refs.append(None)
            continue
        ref = torch.empty(k1 - k0, 81, device=DEV)
        ops.mel_features_window(d, win, base, n, final, fb, k0, k1, ref, ops.mel_range_workspace(d, k1 - k0 + 2, DEV))
        refs.append(ref)
    mb = ops.MelBatch(d, fb, 6, max(a[4] - a[3] for a in args), DEV)
    for uploaded in (False, True):
        for o in outs:
            o.fill_(7.0)
        dev = _to_device(recs) if uploaded else None
        n_ops = ops.mel_features_batch(mb, recs, 6, dev.data_ptr() if uploaded else None)
        torch.cuda.synchronize()
        # the per-row path: table + STFT + resample on the matrix-core form, STFT + resample on the direct one (pre-emphasis)
        assert n_ops == ((2 if uploaded else 3) if form == "fft" else (2 if pe else 3) * 5), n_ops
        for i, (ref, out) in enumerate(zip(refs, outs)):
            assert float(out[-1].min()) == float(out[-1].max()) == 7.0, (i, "guard row")
            if ref is None:
                assert float(out.min()) == float(out.max()) == 7.0
            else:
                assert torch.equal(_bits(out[:-1]), _bits(ref)), (form, pe, uploaded, i)


# ----------------------------------------------------------------------------- 2. refusals, ahead of any launch
def test_mel_batch_refuses_before_it_launches():
    d, fb = _mel_dims()
    recs, wins, outs, args = _batch_rows(d)
    mb = ops.MelBatch(d, fb, 6, max(a[4] - a[3] for a in args), DEV)
    api, stream = capi.api(), ops._stream()

    def call(d_, recs_, n, ws_bytes=None):
        api.zeggs_mel_features_batch(d_, recs_, None, n, fb, mb.tables, mb.ws, mb.ws.numel() if ws_bytes is None else ws_bytes, stream)

    def untouched():
        torch.cuda.synchronize()
        assert all(float(o.min()) == float(o.max()) == 7.0 for o in outs)

    def changed(i, **kw):
        out = (capi.MelRow * 6)()
        C.memmove(out, recs, C.sizeof(recs))
        for k, v in kw.items():
            setattr(out[i], k, v)
        return out

    short = wins[2][1:].clone()                          # the window of row 2 one sample too short
    with pytest.raises(RuntimeError, match=r"row 2: .*window starts"):
        call(d, changed(2, wav=short.data_ptr(), base=args[2][0] + 1), 6)
    untouched()
    with pytest.raises(RuntimeError, match=r"row 3: .*not received yet"):
        call(d, changed(3, k1=ops.mel_frames_ready(d, args[3][1]) + 1), 6)
    untouched()
    cubic, _ = _mel_dims(flags=audio.mel_flags(True, True, "linear") | 8)
    with pytest.raises(RuntimeError, match=r"row 0: .*cubic"):
        call(cubic, recs, 6)
    untouched()
    many = (capi.MelRow * 65)()
    for i in range(65):
        C.memmove(C.byref(many[i]), C.byref(recs[i % 5]), C.sizeof(capi.MelRow))
    with pytest.raises(RuntimeError, match=r"65 rows"):
        call(d, many, 65)
    untouched()
    need = api.zeggs_mel_batch_workspace_bytes(d, 6, max(a[4] - a[3] for a in args))
    assert need == mb.ws.numel()
    with pytest.raises(RuntimeError, match=r"workspace too small"):
        call(d, recs, 6, need - 1)
    untouched()
    call(d, recs, 6)                                     # ... and the same records are taken as they are
    torch.cuda.synchronize()
    assert float(outs[0][:-1].max()) != 7.0 and float(outs[5].min()) == 7.0


# ----------------------------------------------------------------------------- 3. zeggs_copy_segments
@pytest.mark.parametrize("shift", [0, 1, 2])
def test_copy_segments(shift):
    """seventeen segments in one launch: counts 0, 1, 63, 64, 65 and 1 025 floats at source / destination offsets of 0, 1 and 3
    floats from a 16-byte boundary (equal offsets take the 16-byte lanes with a scalar head and tail, unequal ones go float by
    float); the destination buffer is bitwise what it was everywhere else"""
    counts, offs, pitch = (0, 1, 63, 64, 65, 1025), (0, 1, 3), 2048
    src = torch.randn(17 * pitch, device=DEV, generator=torch.Generator(DEV).manual_seed(5 + shift))
    dst = torch.full((17 * pitch,), -5.0, device=DEV)
    want = dst.clone()
    segs = (capi.Seg * 17)()
    pairs = set()
    for i in range(17):
        cnt, so, do = counts[i % 6], offs[(i + shift) % 3], offs[(i // 3) % 3]
        pairs.add((so, do))
        segs[i].src, segs[i].dst, segs[i].count = src.data_ptr() + 4 * (i * pitch + so), dst.data_ptr() + 4 * (i * pitch + do), cnt
        want[i * pitch + do:i * pitch + do + cnt] = src[i * pitch + so:i * pitch + so + cnt]
    assert len(pairs) >= 8 and src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    dev = _to_device(segs)
    ops.copy_segments(segs, 17, dev.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst), _bits(want))


# ----------------------------------------------------------------------------- 4. push_many == push
def _schedule(nsamp, seed):
    """chunk sizes per call for three rows: an empty chunk and one larger than the 4096-sample window in the first calls, then
    sizes that make the windows compact at different calls, until every signal is used up"""
    rng = np.random.default_rng(seed)
    calls = [[700, 5000, 0], [0, 123, 4100], [3000, 37, 2500]]
    pos = [sum(c[r] for c in calls) for r in range(3)]
    while min(pos) < nsamp:
        c = [int(rng.choice([0, 37, 160, 900, 1600, 2500, 3000])) for _ in range(3)]
        c = [min(x, nsamp - p) for x, p in zip(c, pos)]
        if not any(c):
            continue
        calls.append(c)
        pos = [p + x for p, x in zip(pos, c)]
    return calls


def _counters(srv):
    return [(w.n, w.base, w.n_feat, w.fbase, w.n_ring, w.kd) for w in srv._rows]


def _pending(srv, r):
    w = srv._rows[r]
    return _bits(srv.feats[r, w.n_ring - w.fbase:w.n_feat - w.fbase])


@pytest.mark.parametrize("tick", [3, 4])
def test_push_many_equals_push(tick):
    """three servers of 3 rows, windows of 4096 samples, the same three 2.5 s signals in the same irregular chunks (an empty one, one
    larger than the window, sizes that compact the windows; the pending-feature blocks compact on the way): push() per stream,
    push_many(), and the two taking turns on the same streams.  After every call the pending feature rows and the six host
    counters per row are bitwise equal; drained frames and close() tails agree within the decoder path's bound"""
    nsamp = 40000
    wavs = [_wav(nsamp, 20 + r) for r in range(3)]
    calls = _schedule(nsamp, tick)
    servers = {k: _server(3, tick, window_capacity=4096) for k in ("push", "many", "mixed")}
    sids = {k: [s.open(_first(3 + r), _style(30 + r)) for r in range(3)] for k, s in servers.items()}
    parts = {k: [[] for _ in range(3)] for k in servers}
    pos, fbases = [0, 0, 0], set()
    for ci, c in enumerate(calls):
        chunks = [wavs[r][pos[r]:pos[r] + c[r]] for r in range(3)]
        pos = [p + x for p, x in zip(pos, c)]
        for k, srv in servers.items():
            if k == "many" or (k == "mixed" and ci % 2 == 0):
                caps = list(srv.stats["window_capacity"])
                srv.push_many({sids[k][r]: chunks[r] for r in range(3)})
                grew = caps != srv.stats["window_capacity"]      # (a chunk that did not fit beside what must stay: the one exception)
                assert srv.stats["ops_last_push_many"] <= 5 or grew, (ci, k)
            else:
                for r in range(3):
                    srv.push(sids[k][r], chunks[r])
        ref = servers["push"]
        for k in ("many", "mixed"):
            assert _counters(servers[k]) == _counters(ref), (ci, k)
            for r in range(3):
                assert torch.equal(_pending(servers[k], r), _pending(ref, r)), (ci, k, r)
        fbases |= {(r, w.fbase) for r, w in enumerate(ref._rows)}
        for k, srv in servers.items():
            for sid, o in srv.drain().items():
                parts[k][sids[k].index(sid)].append(o)
        assert _counters(servers["many"]) == _counters(ref) == _counters(servers["mixed"])
    assert pos == [nsamp] * 3 and all(len({f for r, f in fbases if r == q}) >= 2 for q in range(3))      # every feature block compacted
    assert all(s.FC == max(4 * (tick + 16), 64) for s in servers.values())      # (no feature block grew)
    assert max(ref.stats["window_capacity"]) > 4096 and servers["many"].stats["window_capacity"] == ref.stats["window_capacity"]
    assert servers["many"].stats["uploaded_samples"] == ref.stats["uploaded_samples"] == 3 * nsamp
    bound = _bound(ref)
    for k, srv in servers.items():
        for r in range(3):
            parts[k][r].append(srv.close(sids[k][r]))
    for r in range(3):
        want = _cat(parts["push"][r])
        assert want["pose"].shape[0] == audio.n_anim_frames(nsamp)
        for k in ("many", "mixed"):
            got = _cat(parts[k][r])
            for key in KEYS:
                assert got[key].shape == want[key].shape and torch.isfinite(got[key]).all()
                e = float((got[key] - want[key]).abs().max())
                print(f"tick={tick} {k} row {r} {key}: max |push_many - push| = {e:.3e}")
                assert e <= bound, (k, r, key, e)


# ----------------------------------------------------------------------------- 5. rows do not see each other
def test_push_many_rows_do_not_see_each_other():
    """one row's audio is NaN: the other rows' features are bitwise what they are when that row gets silence"""
    wavs = [_wav(8000, 40 + r) for r in range(3)]
    feats = {}
    for poison in (False, True):
        srv = _server(3, 4, window_capacity=4096)
        sids = [srv.open(_first(3), _style(50 + r)) for r in range(3)]
        for i in range(5):                                   # (the third call compacts the windows)
            chunks = {sids[r]: wavs[r][1600 * i:1600 * (i + 1)] for r in range(3)}
            chunks[sids[1]] = np.full(1600, np.nan if poison else 0.0, np.float32)
            srv.push_many(chunks)
        torch.cuda.synchronize()
        assert all(w.n_feat > 20 and w.base > 0 for w in srv._rows)
        feats[poison] = [srv.feats[r, :srv._rows[r].n_feat].clone() for r in range(3)]
    for r in (0, 2):
        assert torch.isfinite(feats[True][r]).all() and torch.equal(_bits(feats[True][r]), _bits(feats[False][r])), r
    assert torch.isnan(feats[True][1]).any() and torch.isfinite(feats[False][1]).all()


# ----------------------------------------------------------------------------- 6. the operation count does not depend on the rows
@pytest.mark.parametrize("rows", [2, 64])
def test_push_many_operation_count_does_not_depend_on_the_rows(rows):
    """every row pushed in every call, 6000 samples into windows of 8192 (from the second call on every window compacts), steps in
    between: no call enqueues more than five operations, and the call in which every row compacts its window AND its feature
    block enqueues exactly five -- at 2 rows and at 64"""
    srv = _server(rows, 4, window_capacity=8192)
    sids = [srv.open(_first(3), _style(60)) for _ in range(rows)]
    wav = _wav(66100, 7)
    both = 0
    for i in range(11):
        before = _counters(srv)
        srv.push_many({sid: wav[6000 * i + 13 * (r % 5):6000 * (i + 1) + 13 * (r % 5)] for r, sid in enumerate(sids)})
        n_ops = srv.stats["ops_last_push_many"]
        assert 1 <= n_ops <= 5, (i, n_ops)
        after = _counters(srv)
        win = all(a[1] > b[1] for a, b in zip(after, before))
        fts = all(a[3] != b[3] for a, b in zip(after, before))
        if win and fts:
            both += 1
            assert n_ops == 5
        srv.drain()
    assert both >= 1 and srv.stats["window_capacity"] == [8192] * rows and srv.FC == 80
    assert srv.stats["uploaded_samples"] == rows * 66000
    torch.cuda.synchronize()
    assert all(torch.isfinite(srv.feats[r, :srv._rows[r].n_feat - srv._rows[r].fbase]).all() for r in range(rows))
