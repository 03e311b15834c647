"""Live serving (zeggs/live.py): sliding-window mel front-end, incremental speech encoder, LiveServer.  Yardsticks are the
existing paths -- zeggs_mel_features_range, zeggs_speech_encoder_fwd, the offline computation of
test_streaming_matches_offline_generation (audio.preprocess_audio -> speech encoder -> ops.decoder_core) and the reference's own
generate_gesture() fixture -- never the new code against itself.

Bounds: 5e-5 for re-associated fp32 on this chain (test_streaming_matches_offline_generation); 1e-4 where the rows rode the
weight-stationary sweep (test_gpu_batch_decode.test_single_chunk_vs_oracle)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import helpers
from zeggs import anim, audio, ops, synth

pytestmark = pytest.mark.gpu
DEV = helpers.LIVE_DEV
SPIN = 1 << 21
KEYS = helpers.LIVE_KEYS
CONF = helpers.LIVE_CONF


@pytest.fixture
def restore_options():
    yield
    for k, v in (("persistent_spin", SPIN), ("train_persistent", 1), ("bwd_persistent", 1), ("persistent", 1), ("mel_fft", 1),
                 ("mel_mfma", 1)):
        ops.set_option(k, v)


# the offline rollout, its bound and the seeded inputs live in tests/helpers.py (shared with tests/test_gpu_live_dims.py)
_nets, _stats, _first, _wav, _style = helpers.live_nets, helpers.live_stats, helpers.live_first, helpers.live_wav, helpers.live_style
_offline, _offline_cached, _server, _cat = helpers.live_offline, helpers.live_offline_cached, helpers.live_server, helpers.live_cat


def _feed(srv, sid, wav, chunks):
    """push `wav` in the given chunk sizes with drain() after each push, then close -> the stream's frames"""
    parts, pos = [], 0
    for n in chunks:
        srv.push(sid, wav[pos:pos + n])
        pos += n
        parts.append(srv.drain().get(sid))
    assert pos >= len(wav)
    parts.append(srv.close(sid))
    return _cat(parts)


_err, _bound = helpers.live_err, helpers.live_bound


# ----------------------------------------------------------------------------- 1. mel window == mel range
def _mel_range(d, fb, w, n, final, k0, k1):
    L = ops.lib()
    ws = ops.mel_range_workspace(d, k1 - k0 + 2, DEV)
    out = torch.empty(k1 - k0, d.n_mels + 1, device=DEV)
    rc = L.zeggs_mel_features_range(C.byref(d), C.c_void_p(w.data_ptr()), C.c_long(n), int(final), C.c_void_p(fb.data_ptr()),
                                    C.c_long(k0), C.c_long(k1), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                    C.c_size_t(ws.numel()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.zeggs_last_error().decode()
    return out


@pytest.mark.parametrize("form,pe", [("fft", False), ("fft", True), ("mfma", False), ("direct", False), ("direct", True)])
def test_mel_window_equals_mel_range(form, pe, restore_options):
    """rows [k0, k1) from a window that starts exactly at zeggs_mel_window_first_sample(k0) are bit-identical to
    zeggs_mel_features_range on the whole signal, on each kernel form (FFT, matrix-core DFT -- which does not take
    pre-emphasis --, direct DFT), signal continuing and ended; a window one sample shorter is refused"""
    ops.set_option("mel_fft", 1 if form == "fft" else 0)
    ops.set_option("mel_mfma", 1 if form == "mfma" else 0)
    g = CONF
    fb, min_clip = audio.mel_tables(g["filter_length"], 16000, 80, g["mel_fmin"], g["mel_fmax"], g["min_clipping"], True, True, DEV)
    d = audio.MelDims(800, 200, 80, 16000, 60.0, float(min_clip), 0.97 if pe else 0.0, audio.mel_flags(True, True, "linear"))
    n = 40123
    w = torch.as_tensor(_wav(n, 1), device=DEV)
    n_total, ready = audio.n_anim_frames(n), ops.mel_frames_ready(d, n)
    assert ready > 100 and n_total > ready
    for final, k1 in ((0, ready), (1, n_total)):
        for k0 in (0, 1, 17, 100):
            ref = _mel_range(d, fb, w, n, final, k0, k1)
            base = ops.mel_window_first_sample(d, k0)
            win = w[base:].clone()
            out = torch.full((k1 - k0, 81), 7.0, device=DEV)
            ops.mel_features_window(d, win, base, n, final, fb, k0, k1, out, ops.mel_range_workspace(d, k1 - k0 + 2, DEV))
            assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), (form, pe, final, k0)
            if base > 0:
                with pytest.raises(RuntimeError, match="window starts"):
                    ops.mel_features_window(d, win[1:].clone(), base + 1, n, final, fb, k0, k1, out,
                                            ops.mel_range_workspace(d, k1 - k0 + 2, DEV))


# ----------------------------------------------------------------------------- 2. incremental encoder == zeggs_speech_encoder_fwd
def test_incremental_encoder_equals_the_offline_encoder():
    """3 rows of 31 / 47 / 150 frames fed in bursts of 1, 4 and 23 frames through ONE launch per burst, rings of the minimum depth
    (KW + 23 - 1 = 53 frames: the longest row wraps it twice), the short row ends early and is skipped from then on (its ring is
    not touched): every frame -- the first 15 and last 15 with their replicate padding included -- within 5e-5 of
    zeggs_speech_encoder_fwd on the whole row"""
    se, _ = _nets()
    st = _stats()
    lens, bursts, D = (31, 47, 150), (1, 4, 23), 31 + 23 - 1
    rng = np.random.default_rng(3)
    mean, std = st["audio_input_mean"], st["audio_input_std"]
    feats = torch.zeros(3, 150, 81, device=DEV)
    for r, n in enumerate(lens):      # un-normalised rows with the statistics' spread
        feats[r, :n] = torch.as_tensor(rng.standard_normal((n, 81)).astype(np.float32), device=DEV) * std + mean
    with torch.no_grad():
        ref = [se(((feats[r:r + 1, :n] - mean) / std).contiguous())[0] for r, n in enumerate(lens)]
    enc = ops.LiveSpeech(se, mean, std, 3, D, 150, 23 + 15)
    ring = torch.zeros(3, D, 64, device=DEV)
    got = [[] for _ in lens]
    n_ring, done = [0, 0, 0], [0, 0, 0]      # frames in the ring / frames produced
    frozen, call = None, 0
    while any(done[r] < lens[r] for r in range(3)):
        rows = []
        for r, n in enumerate(lens):
            b = min(bursts[(call + r) % 3], n - n_ring[r])
            total = n_ring[r] + b
            final = total == n
            k1 = n if final else max(total - 15, done[r])
            if done[r] == n:
                rows.append(ops.LiveRow(0, 0, -1, 0, 0, 0, 0))
                continue
            rows.append(ops.LiveRow(n_ring[r], done[r], n - 1 if final else -1, b, k1 - done[r], n_ring[r], 0))
        out = torch.full((3, 38, 64), float("nan"), device=DEV)
        ops.speech_encoder_live(enc, rows, feats, ring, out)
        for r, row in enumerate(rows):
            got[r].append(out[r, :row.n_out].clone())
            assert row.n_out == 38 or float(out[r, row.n_out:].abs().max()) == 0.0      # the rest of a row's block: finite filler
            n_ring[r] += row.n_new
            done[r] += row.n_out
        if done[0] == lens[0]:
            if frozen is None:
                frozen = ring[0].clone()
            assert torch.equal(ring[0], frozen)
        call += 1
    assert frozen is not None and call > 10
    for r, n in enumerate(lens):
        o = torch.cat(got[r])
        assert o.shape == ref[r].shape == (n, 64)
        e = float((o - ref[r]).abs().max())
        print(f"row {r} ({n} frames): max |incremental - offline| = {e:.3e}")
        assert e <= 5e-5, (r, e)
    # a frame whose look-ahead is not in the ring is refused, not read
    with pytest.raises(RuntimeError, match="needs frame"):
        ops.speech_encoder_live(enc, [ops.LiveRow(0, 0, -1, 10, 1, 0, 0)] + [ops.LiveRow(0, 0, -1, 0, 0, 0, 0)] * 2, feats,
                                torch.zeros(3, D, 64, device=DEV), torch.zeros(3, 38, 64, device=DEV))
    with pytest.raises(RuntimeError, match="left the ring"):
        ops.speech_encoder_live(enc, [ops.LiveRow(100, 40, -1, 5, 1, 100, 0)] + [ops.LiveRow(0, 0, -1, 0, 0, 0, 0)] * 2, feats,
                                torch.zeros(3, D, 64, device=DEV), torch.zeros(3, 38, 64, device=DEV))


# ----------------------------------------------------------------------------- 3. one row, any chunking == offline
@pytest.mark.parametrize("rows,tick", [(1, 3), (1, 4), (3, 3), (3, 4)])
def test_one_stream_any_chunking_equals_offline(rows, tick):
    nsamp, seed = 40123, 1
    wav, ref = _wav(nsamp, seed), _offline_cached(nsamp, seed, 3, seed)
    srv = _server(rows, tick)
    sid = srv.open(_first(3), _style(seed))
    rng = np.random.default_rng(seed + 10 * rows + tick)
    chunks, tot = [], 0
    while tot < nsamp:
        chunks.append(int(rng.choice([37, 160, 1600, 5000, 16000])))
        tot += chunks[-1]
    got = _feed(srv, sid, wav, chunks)
    assert got["pose"].shape[0] == audio.n_anim_frames(nsamp) == ref[0].shape[0]
    assert srv.stats["steps"] >= 3 and srv.stats["uploaded_samples"] == nsamp
    e = _err(got, ref)
    print(f"rows={rows} tick={tick}: {e}")
    assert max(e.values()) <= 5e-5, e


# ----------------------------------------------------------------------------- 4. rows do not see each other
STREAMS = {"A": (19000, 11, 3, 21), "B": (30000, 12, 4, 22), "C": (26500, 13, 5, 23), "D": (22000, 14, 6, 24)}   # samples, wav / pose / style seed


def _poison(srv, r):
    nan = float("nan")
    for t in (srv.window[r], srv.feats[r], srv.ring[r], srv.h[:, r], srv.pose[r], srv.rpos[r], srv.rrot[r], srv.gaze[r],
              srv.sty_old[r], srv.sty_new[r]):
        t.fill_(nan)


def test_rows_do_not_see_each_other():
    """rows = 5; A, B, C (different audio, styles, first poses) are opened at different steps, A ends first and its row is taken
    by D; an idle row holds NaN in every buffer the server owns for it.  Each stream equals its own offline rollout, and D on
    the reused row equals D on a fresh server."""
    srv = _server(5, 4)
    wavs = {k: _wav(v[0], v[1]) for k, v in STREAMS.items()}
    start = {"A": 0, "B": 3, "C": 7}
    sids, pos, parts, row_of = {}, {}, {k: [] for k in STREAMS}, {}
    rnd = 0
    while len(parts["D"]) == 0 or "D" in sids:
        for k in list(STREAMS):
            if k not in sids and k not in pos and (start.get(k) == rnd or (k == "D" and "A" in pos and "A" not in sids)):
                sids[k] = srv.open(_first(STREAMS[k][2]), _style(STREAMS[k][3]))
                pos[k], row_of[k] = 0, srv._sids[sids[k]]
                if k == "A":
                    _poison(srv, 4)
        for k in list(sids):
            w = wavs[k]
            if pos[k] < len(w):
                srv.push(sids[k], w[pos[k]:pos[k] + 1600])
                pos[k] += 1600
            else:
                parts[k].append(srv.close(sids.pop(k)))
        for sid, o in srv.drain().items():
            parts[[k for k in sids if sids[k] == sid][0]].append(o)
        rnd += 1
        assert rnd < 200
    assert not sids and row_of["D"] == row_of["A"] == 0 and len({row_of[k] for k in "ABC"}) == 3
    assert all(torch.isnan(t).all() for t in (srv.h[:, 4], srv.pose[4], srv.ring[4]))      # the idle row was never committed
    bound = _bound(srv)
    for k, v in STREAMS.items():
        e = _err(_cat(parts[k]), _offline_cached(*v))
        print(f"stream {k}: {e}")
        assert max(e.values()) <= bound, (k, e)
    fresh = _server(5, 4)
    w = wavs["D"]
    got = _feed(fresh, fresh.open(_first(STREAMS["D"][2]), _style(STREAMS["D"][3])), w, [1600] * (len(w) // 1600 + 1))
    e = _err(_cat(parts["D"]), tuple(got[k] for k in KEYS))
    print(f"D reused row vs fresh server: {e}")
    assert max(e.values()) <= bound, e


# ----------------------------------------------------------------------------- 5. against the reference
def test_live_server_vs_the_reference_generate_gesture(golden_dir):
    """the 2 s clip of generate.npz (the reference's own generate_gesture() run) through a 2-row server beside an unrelated
    stream: rotations, positions and root within 1e-4, integer frame count exact"""
    gd = np.load(golden_dir / "generate.npz")
    wav = gd["wav"].astype(np.float32) / 32768.0
    clip = dict(rotations=gd["ex_rotations"], positions=gd["ex_positions"], offsets=gd["ex_offsets"], parents=gd["ex_parents"],
                names=synth.BONE_NAMES, order="zyx", frametime=synth.DT)
    first = anim.preprocess_animation(clip, DEV)
    style = torch.as_tensor(gd["encoding"][:, 0], device=DEV)
    srv = _server(2, 4)
    other = srv.open(_first(4), _style(9))
    sid = srv.open(first, style)
    ow = _wav(30000, 8)
    parts, pos = [], 0
    for i, n in enumerate((700, 5000, 123, 9000, 16000, 1177)):
        srv.push(other, ow[4000 * i:4000 * (i + 1)])
        srv.push(sid, wav[pos:pos + n])
        pos += n
        parts.append(srv.drain().get(sid))
    assert pos == len(wav)
    parts.append(srv.close(sid))
    got = {k: v.cpu().numpy() for k, v in _cat(parts).items()}
    pose, rpos, rrot = got["pose"], got["rpos"], got["rrot"]
    T, J = gd["dec_ltxy"].shape[0], synth.NJ
    assert pose.shape[0] == T
    assert np.abs(pose[:, 6 + 3 * J:6 + 9 * J].reshape(T, J, 2, 3) - gd["dec_ltxy"]).max() <= 1e-4
    assert np.abs(pose[:, 6:6 + 3 * J].reshape(T, J, 3) - gd["dec_lpos"]).max() <= 1e-4
    assert np.abs(rpos - gd["dec_root_pos"]).max() <= 1e-4 and np.abs(rrot - gd["dec_root_rot"]).max() <= 1e-4


# ----------------------------------------------------------------------------- 6. style change
@pytest.mark.parametrize("fade", [0, 12])
def test_style_change_while_speech_goes_on(fade):
    """set_style at an arbitrary moment: the frames equal ops.decoder_core with the per-frame style tensor built from the returned
    k (old before k, `fade` frames on the line between, new from k + fade on); frames before k are those of a run without the
    change (2e-5: run to run only the split-K atomics of the prologue products differ, test_slot_refill_and_padding_never_leaks)"""
    nsamp, seed = 32000, 2
    wav = _wav(nsamp, seed)
    old, new = _style(31), _style(32)
    chunks = [1600] * 20

    def run(change_at):
        srv = _server(2, 4)
        sid = srv.open(_first(3), old)
        parts, k = [], None
        for i in range(20):
            if i == change_at:
                k = srv.set_style(sid, new, fade=fade)
            srv.push(sid, wav[1600 * i:1600 * (i + 1)])
            parts.append(srv.drain().get(sid))
        parts.append(srv.close(sid))
        return srv, _cat(parts), k

    srv, got, k = run(9)
    n_frames = audio.n_anim_frames(nsamp)
    assert 20 < k < n_frames - 20
    f = torch.arange(n_frames, device=DEV, dtype=torch.float32)
    wgt = ((f - k + 1) / (fade + 1)).clamp(0, 1)[:, None]
    ref = _offline(wav, _first(3), old + wgt * (new - old))
    bound = _bound(srv)
    e = _err(got, ref)
    print(f"fade={fade} k={k}: {e}")
    assert max(e.values()) <= bound, e
    _, plain, _ = run(-1)
    for key in KEYS:
        assert float((got[key][:k] - plain[key][:k]).abs().max()) <= 2e-5, key
    assert float((got["pose"][k + fade:] - plain["pose"][k + fade:]).abs().max()) > 1e-3      # ... and the change took effect


# ----------------------------------------------------------------------------- 7. bounded state
def test_state_stays_bounded_over_twenty_seconds():
    """20 s of audio in 1/15 s pushes through rows = 2 with drain() after each: window capacity and ring bytes after 20 s are
    those after 2 s, only the pushed samples were uploaded, and the last step enqueues what the first one did"""
    fs, push = 16000, 16000 // 15
    wav = np.tile(_wav(4 * fs, 6), 5)
    srv = _server(2, 4)
    sid = srv.open(_first(3), _style(5))
    marks, first_launches, frames, pos = {}, None, 0, 0
    while pos < len(wav):
        srv.push(sid, wav[pos:pos + push])
        pos += push
        out = srv.drain().get(sid)
        if out:
            frames += out["pose"].shape[0]
            if first_launches is None:
                first_launches = srv.stats["launches_per_step"]
        if pos >= 2 * fs and "2s" not in marks:
            marks["2s"] = (list(srv.stats["window_capacity"]), srv.stats["ring_bytes"], srv.ring.numel() * 4, srv.feats.numel(),
                           [w.numel() for w in srv.window])
    marks["20s"] = (list(srv.stats["window_capacity"]), srv.stats["ring_bytes"], srv.ring.numel() * 4, srv.feats.numel(),
                    [w.numel() for w in srv.window])
    assert marks["20s"] == marks["2s"]
    assert srv.stats["uploaded_samples"] == len(wav)
    assert first_launches is not None and srv.stats["launches_per_step"] == first_launches
    assert srv._rows[0].base > 18 * fs                      # the window slid: it holds the recent samples only
    tail = srv.close(sid)
    assert frames + tail["pose"].shape[0] == audio.n_anim_frames(len(wav))
    assert torch.isfinite(tail["pose"]).all()


# ----------------------------------------------------------------------------- 8. give-up
def test_giveup_redoes_the_step(restore_options):
    """the method of test_streaming_giveup_redoes_the_chunk, applied to ONE step of a 2-row server: the sweep's bounded wait is
    exhausted for that step (option "persistent_spin" = 0, the existing hook, used once), the step is redone on the stage
    launches before anything is committed, counted, and the frames still equal the offline rollout"""
    nsamp, seed = 32000, 5
    wav, ref = _wav(nsamp, seed), _offline_cached(nsamp, seed, 3, seed)

    def run(fail_step):
        srv = _server(2, 4)
        sid = srv.open(_first(3), _style(seed))
        parts, steps = [], 0
        for i in range(20):
            srv.push(sid, wav[1600 * i:1600 * (i + 1)])
            while True:
                if steps == fail_step:
                    assert ops.lib().zeggs_persistent_state(1) == 1
                    ops.set_option("persistent_spin", 0)
                out = srv.step()
                ops.set_option("persistent_spin", SPIN)
                if not out:
                    break
                steps += 1
                parts.append(out[sid])
        parts.append(srv.close(sid))
        return srv, _cat(parts)

    ops.set_option("train_persistent", 1)
    srv, good = run(-1)
    if ops.lib().zeggs_persistent_state(1) != 1:
        pytest.skip("the batch decode sweep is not available on this device")
    assert srv.redone_steps == 0
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        srv, got = run(6)
    assert any("gave up" in str(w.message) for w in rec) and srv.redone_steps == 1
    e = _err(got, ref)
    print(f"redone step: {e}")
    assert max(e.values()) <= 1e-4, e
    assert max(_err(got, tuple(good[k] for k in KEYS)).values()) <= 5e-5
