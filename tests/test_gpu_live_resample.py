"""LiveServer rows at a rate and sample format of their own: the rate converter on the device (include/zeggs_hip_resample.h,
csrc/live_resample.hip).  Yardsticks: the float64 oracle of tests/live_resample_oracle.py for the converted samples (every
device float32 is the float32 nearest to the oracle's value or one of its two neighbours: the float64 accumulation error,
taps x 2^-53, is far below 2^-24, so only a value on a rounding boundary can differ), audio.resample_device and the kernel
against itself for everything that must not depend on the cuts (bitwise), and an all-native server fed the converted signals
for the plumbing (bitwise windows, features, loudness and frames)."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest
import torch

import live_resample_oracle as oracle_rs
from test_gpu_live_loudness import _Feats, _window
from test_gpu_live_push import DEV, KEYS, _bits, _cat, _first, _server, _style
from zeggs import audio, capi, live, ops, synth

pytestmark = pytest.mark.gpu
FS = 16000
RATES = (48000, 44100, 8000, 22050)          # 3:1, 441:160, 1:2, 441:320


def _signal(n, seed, fmt):
    """n samples: float32 noise in (-1, 1), or int16 PCM over the whole range (both ends included)"""
    rng = np.random.default_rng(seed)
    if fmt == "s16":
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        x[:2] = (-32768, 32767)
        return x
    return (rng.standard_normal(n) * 0.3).clip(-0.999, 0.999).astype(np.float32)


def _f64(x):
    return oracle_rs.pcm16(x) if x.dtype == np.int16 else x.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _want(fi, n, seed, fmt, Z):
    return oracle_rs.whole(_f64(_signal(n, seed, fmt)), fi, FS, Z=Z)


class _Kernel:
    """zeggs_resample_push driven directly: row r converts rates[r] -> 16 kHz; push({row: chunk}) is ONE launch for all its
    records (the records also in device memory), -> {row: the outputs that call wrote}"""

    def __init__(self, rates, fmt, Z):
        self.rs = ops.LiveResample(FS, len(rates), dict(zero_crossings=Z), DEV)
        self.tab = [self.rs.table(fi) for fi in rates]
        self.fmt, self.n_in, self.n_out = ops.RS_FORMATS[fmt], [0] * len(rates), [0] * len(rates)
        for r in range(len(rates)):
            ops.live_resample_reset(self.rs, r)
        self.launches = 0

    def push(self, chunks, final=False, flush=False):
        recs, keep, out = (ops.ResampleRow * len(chunks))(), [], {}
        for q, (r, c) in zip(recs, chunks.items()):
            t, n1 = self.tab[r], self.n_in[r] + len(c)
            due = audio.resample_total(n1, t["L"], t["M"]) if final or flush else audio.resample_ready(n1, t["L"], t["M"], t["WL"])
            src = torch.as_tensor(np.ascontiguousarray(c)).to(DEV) if len(c) else torch.zeros(1, device=DEV)
            out[r] = torch.full((due - self.n_out[r] + 1,), 7.0, device=DEV)      # (one guard element behind the outputs)
            keep.append(src)
            q.src, q.dst, q.table = src.data_ptr(), out[r].data_ptr(), t["table"].data_ptr()
            q.count, q.n_in, q.n_out, q.outputs, q.WL = len(c), self.n_in[r], self.n_out[r], due - self.n_out[r], t["WL"]
            q.row, q.format, q.final, q.L, q.M = r, self.fmt, int(final), t["L"], t["M"]
            self.n_in[r], self.n_out[r] = n1, due
        dev = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(DEV)
        if flush:                                    # zeggs_resample_flush: the one record is final whatever its flag says
            assert len(chunks) == 1 and not final
            capi.api().zeggs_resample_flush(self.rs.d, recs, self.rs.state, self.rs.state.numel(), ops._stream())
        else:
            ops.live_resample_push(self.rs, recs, len(chunks), dev.data_ptr())
        self.launches += 1
        torch.cuda.synchronize()
        for r, o in out.items():
            assert float(o[-1]) == 7.0, "the kernel wrote behind its outputs"
        return {r: o[:-1].cpu().numpy() for r, o in out.items()}


def _run_cut(rates, xs, fmt, Z, seed):
    """every row's signal in its own random cuts of 1..96 samples, call i carrying the i-th cut of every row that has one left,
    then the tails -> the outputs per row, and how many calls had three or more records"""
    k = _Kernel(rates, fmt, Z)
    cuts = [oracle_rs.cuts(len(x), seed * 10 + r) for r, x in enumerate(xs)]
    pos, parts, shared = [0] * len(xs), [[] for _ in xs], 0
    for i in range(max(len(c) for c in cuts)):
        call = {r: xs[r][pos[r]:pos[r] + cuts[r][i]] for r in range(len(xs)) if i < len(cuts[r])}
        shared += len(call) >= 3
        for r, o in k.push(call).items():
            parts[r].append(o)
            pos[r] += cuts[r][i]
    assert pos == [len(x) for x in xs]
    for r, o in k.push({r: xs[r][:0] for r in range(len(xs))}, final=True).items():
        assert 0 < o.size
        parts[r].append(o)
    return [np.concatenate(p) for p in parts], shared


# ----------------------------------------------------------------------------- 1. the kernel against the oracle
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_kernel_against_the_oracle_and_its_own_cuts(fmt):
    """Z = 4, the four ratios as four rows of one call (so three and more rows at different ratios share every early launch),
    700 input samples each, cuts of 1..96 samples drawn per row from a fixed seed: every output within one float32 of the
    oracle; bit for bit the same across two cuttings and equal to audio.resample_device of the whole signal"""
    n, Z = 700, 4
    xs = [_signal(n, 11 + r, fmt) for r in range(len(RATES))]
    a, shared = _run_cut(RATES, xs, fmt, Z, seed=1)
    b, _ = _run_cut(RATES, xs, fmt, Z, seed=2)
    assert shared >= 8
    for r, fi in enumerate(RATES):
        want = _want(fi, n, 11 + r, fmt, Z)
        whole = audio.resample_device(xs[r], fi, FS, zero_crossings=Z).cpu().numpy()
        assert a[r].dtype == np.float32 and a[r].size == want.size == -(-n * FS // fi)
        ok = oracle_rs.within_one_float32(a[r], want)
        exact = float((a[r] == want.astype(np.float32)).mean())
        print(f"{fmt} {fi} Hz: {a[r].size} outputs, {exact:.4f} equal to the nearest float32, max |dev - oracle| = "
              f"{float(np.abs(a[r] - want).max()):.2e}")
        assert ok.all(), (fi, np.flatnonzero(~ok)[:5])
        assert a[r].tobytes() == b[r].tobytes(), f"{fi} Hz: the outputs depend on the cuts"
        assert a[r].tobytes() == whole.tobytes(), f"{fi} Hz: the streaming outputs are not those of the whole-signal call"


# ----------------------------------------------------------------------------- 2. the defaults
def test_defaults_at_48k():
    """Z = 64, rolloff 0.95, beta 10: 0.2 s of 16-bit PCM at 48 kHz in cuts of 1..96 samples, same criterion"""
    n = 9600
    x = _signal(n, 5, "s16")
    (got,), _ = _run_cut((48000,), [x], "s16", 64, seed=3)
    want = _want(48000, n, 5, "s16", 64)
    ok = oracle_rs.within_one_float32(got, want)
    print(f"48000 Hz defaults: {got.size} outputs, max |dev - oracle| = {float(np.abs(got - want).max()):.2e}, "
          f"{float((got == want.astype(np.float32)).mean()):.4f} equal to the nearest float32")
    assert got.size == want.size == 3200 and ok.all(), np.flatnonzero(~ok)[:5]
    assert got.tobytes() == audio.resample_device(x, 48000, FS).cpu().numpy().tobytes()


# ----------------------------------------------------------------------------- 3. pass-through
def test_s16_at_the_servers_rate_is_a_format_conversion():
    """a s16 row at 16 kHz: one tap of 1.0, ready at once, output bitwise s / 32768 -- every int16 value"""
    x = np.arange(-32768, 32768, dtype=np.int16)
    np.random.default_rng(0).shuffle(x)
    k = _Kernel((FS,), "s16", 64)
    assert k.tab[0]["WL"] == 0 and tuple(k.tab[0]["table"].shape) == (1, 1)
    parts, pos = [], 0
    for m in oracle_rs.cuts(x.size, 4, 1, 5000):
        o = k.push({0: x[pos:pos + m]})[0]
        assert o.size == m
        parts.append(o)
        pos += m
    assert k.push({0: x[:0]}, final=True)[0].size == 0
    want = (x.astype(np.float64) / 32768.0).astype(np.float32)
    assert np.concatenate(parts).tobytes() == want.tobytes()
    assert audio.resample_device(x, FS, FS).cpu().numpy().tobytes() == want.tobytes()


# ----------------------------------------------------------------------------- 4. the history hazard
@pytest.mark.parametrize("fi", [48000, 44100, 8000])
def test_one_sample_at_a_time_equals_one_push(fi):
    """a row pushed ONE sample at a time for 3 ceil(2 W) samples -- every call reads the history the call must also replace --
    equals the single push of the same samples, and the tails agree"""
    Z = 4
    L, M = oracle_rs.ratio(fi, FS)
    hist = audio.resample_history(L, Z * max(L, M))
    x = _signal(3 * hist, 21, "f32")
    one, many = _Kernel((fi,), "f32", Z), _Kernel((fi,), "f32", Z)
    want = np.concatenate([one.push({0: x})[0], one.push({0: x[:0]}, flush=True)[0]])      # (its tail through zeggs_resample_flush)
    parts = [many.push({0: x[i:i + 1]})[0] for i in range(x.size)]
    parts.append(many.push({0: x[:0]}, final=True)[0])
    got = np.concatenate(parts)
    assert many.launches == x.size + 1 and got.size == want.size == -(-x.size * FS // fi)
    assert got.tobytes() == want.tobytes()
    assert oracle_rs.within_one_float32(got, _want_of(x, fi, Z)).all()


def _want_of(x, fi, Z):
    return oracle_rs.whole(_f64(x), fi, FS, Z=Z)


# ----------------------------------------------------------------------------- 5. the plumbing
def _pcm(n, seed):
    return np.asarray(synth.synth_wav(n, seed=seed)).astype(np.int16)


def _state(srv, sids, loud):
    torch.cuda.synchronize()
    return [srv.loudness(s) if loud else None for s in sids]


@pytest.mark.parametrize("loud", [False, True], ids=["plain", "loudness"])
def test_converting_rows_against_an_all_native_server(loud):
    """server A: rows opened at 48 kHz s16, 44.1 kHz f32 and native, about one second each, fed in random cuts through
    push_many; server B: all native, fed audio.resample_device of the same signals, each call the samples A's converter owed
    in that call (audio.resample_ready: host arithmetic), the tails before close.  Windows, features, loudness read-back and
    every frame of step() and close() are bitwise equal; a call with a converting row costs at most 6 operations (7 with
    loudness) unless a buffer grew, a native-only call on A at most 5 (6).  Both servers decode inside ops.fixed_order_gemms():
    as serving runs them the decoder's latency-bound products combine split-K partial sums with fp32 atomics, so the last bits
    of a frame change from run to run of ONE server on the same audio (DESIGN "Reproducible scores"; tests/test_gpu_live.py
    allows 2e-5 for it) -- in fixed order equal inputs give equal bits, and that is what is compared"""
    with ops.fixed_order_gemms():
        _converting_rows_against_an_all_native_server(loud)


def _converting_rows_against_an_all_native_server(loud):
    kw = dict(loudness=dict(horizon=2.0)) if loud else {}
    specs = [(48000, "s16"), (44100, "f32"), (None, "f32")]
    raw = [_pcm(48000, 31), (_pcm(44100, 32).astype(np.float32) / 32768.0), (_pcm(16000, 33).astype(np.float32) / 32768.0)]
    conv = [audio.resample_device(raw[0], 48000, FS).cpu().numpy(), audio.resample_device(raw[1], 44100, FS).cpu().numpy(), raw[2]]
    assert [c.size for c in conv] == [16000, 16000, 16000]
    A, B = _server(3, 4, window_capacity=8192, **kw), _server(3, 4, window_capacity=8192, **kw)
    sa = [A.open(_first(3), _style(80 + r), rate=fi, pcm=pcm) for r, (fi, pcm) in enumerate(specs)]
    sb = [B.open(_first(3), _style(80 + r)) for r in range(3)]
    assert A._rs is not None and B._rs is None and A._rows[2].rs is None
    tabs = [A._rows[r].rs for r in range(2)]
    fa, fb = _Feats(A, range(3)), _Feats(B, range(3))
    outs = {"A": [[] for _ in range(3)], "B": [[] for _ in range(3)]}
    cuts = [oracle_rs.cuts(len(raw[r]), 40 + r, 200, (6000, 5500, 2000)[r]) for r in range(3)]
    calls = []
    for i in range(max(len(c) for c in cuts)):
        call = {r: cuts[r][i] for r in range(3) if i < len(cuts[r])}
        if i == 3:
            calls.append({2: call.pop(2)})           # one tick in which only the native row speaks
        calls.append(call)
    pos, sent, most, most_native = [0] * 3, [0] * 3, 0, 0
    for i, call in enumerate(calls):
        native_only = set(call) == {2}
        ca, cb = {}, {}
        for r, m in call.items():
            ca[sa[r]] = raw[r][pos[r]:pos[r] + m]
            pos[r] += m
            due = pos[r] if r == 2 else audio.resample_ready(pos[r], tabs[r]["L"], tabs[r]["M"], tabs[r]["WL"])
            if due > sent[r]:
                cb[sb[r]] = conv[r][sent[r]:due]
            sent[r] = due
        grew_from = (list(A.stats["window_capacity"]), A.FC, A._stage.n_samples, A._stage.nbytes)
        A.push_many(ca)
        grew = grew_from != (list(A.stats["window_capacity"]), A.FC, A._stage.n_samples, A._stage.nbytes)
        n_ops = A.stats["ops_last_push_many"]
        if native_only:
            assert 1 <= n_ops <= 5 + loud, n_ops
            most_native = n_ops
        elif not grew:
            assert 1 <= n_ops <= 6 + loud, (i, n_ops)
            most = max(most, n_ops)
        B.push_many(cb)
        fa.grab()
        fb.grab()
        for name, srv, sids in (("A", A, sa), ("B", B, sb)):
            for sid, o in srv.drain().items():
                outs[name][sids.index(sid)].append(o)
    assert pos == [len(x) for x in raw] and most_native >= 2 and most >= 5
    # what the converters still owe arrives at close: B gets it as one more push
    for r in range(3):
        assert A._rows[r].n == B._rows[r].n == sent[r] and (r == 2 or 16000 - 64 <= sent[r] < 16000)
        (ba, wa), (bb, wb) = _window(A, r), _window(B, r)
        assert ba == bb and torch.equal(_bits(wa), _bits(wb)), r
    la, lb = _state(A, sa, loud), _state(B, sb, loud)
    for r in range(3):
        if sent[r] < conv[r].size:
            B.push_many({sb[r]: conv[r][sent[r]:]})      # (the features of the tails show in close()'s frames)
        outs["A"][r].append(A.close(sa[r]))
        outs["B"][r].append(B.close(sb[r]))
    torch.cuda.synchronize()
    for r in range(3):
        assert fa.all(r).shape == fb.all(r).shape and fa.all(r).shape[0] > 40
        assert torch.equal(_bits(fa.all(r)), _bits(fb.all(r))), f"row {r}: features"
        if loud:
            assert la[r]["blocks"] == lb[r]["blocks"] >= 5 and la[r]["gated"] == lb[r]["gated"] and la[r]["held"] == lb[r]["held"]
            assert struct.pack("<dd", la[r]["lufs"], la[r]["gain"]) == struct.pack("<dd", lb[r]["lufs"], lb[r]["gain"]), r
        a, b = _cat(outs["A"][r]), _cat(outs["B"][r])
        assert a["pose"].shape[0] == audio.n_anim_frames(16000) == b["pose"].shape[0]
        for key in KEYS:
            print(f"row {r} {key}: max |A - B| = {float((a[key] - b[key]).abs().max()):.3e}")
            assert torch.isfinite(a[key]).all() and torch.equal(_bits(a[key]), _bits(b[key])), (r, key)
    assert A.stats["resampled_rows"] >= 20 and B.stats["resampled_rows"] == 0
    assert A.stats["uploaded_samples"] == 16000 and B.stats["uploaded_samples"] == 48000
    assert A.stats["uploaded_bytes"] > 2 * 48000 + 4 * 44100 and B.stats["uploaded_bytes"] >= 4 * 48000


# ----------------------------------------------------------------------------- 6. isolation, push(), refusals
def test_a_converting_row_leaves_its_neighbours_alone():
    """rows 1 and 2 native, row 0 at 48 kHz s16: the native rows' frames are bitwise what they are while row 0 stays silent;
    row 0 through push() equals row 0 through push_many() (frames inside ops.fixed_order_gemms(), as in the test above);
    what open() and push() refuse"""
    with ops.fixed_order_gemms():
        runs = _isolation_runs()
    assert runs["with"][0]["pose"].shape[0] == audio.n_anim_frames(8000)
    for r in (1, 2):
        for key in KEYS:
            print(f"row {r} {key}: max |with - without| = {float((runs['with'][r][key] - runs['without'][r][key]).abs().max()):.3e}")
            assert torch.equal(_bits(runs["with"][r][key]), _bits(runs["without"][r][key])), (r, key)
    for key in KEYS:
        assert torch.equal(_bits(runs["with"][0][key]), _bits(runs["push"][0][key])), key
    srv = _server(2, 4)
    for bad in (400000, 16001, 44100.5):
        with pytest.raises(ValueError, match="16000"):
            srv.open(_first(3), _style(1), rate=bad)
    with pytest.raises(ValueError, match="pcm"):
        srv.open(_first(3), _style(1), pcm="u8")
    assert srv._rows == [None, None] and srv._rs is None
    s16, f32 = srv.open(_first(3), _style(1), pcm="s16"), srv.open(_first(3), _style(2))
    with pytest.raises(TypeError, match="int16 samples"):
        srv.push(s16, np.zeros(100, np.float32))
    with pytest.raises(TypeError, match="float samples"):
        srv.push_many({f32: np.zeros(100, np.int16)})
    assert srv._rows[0].n == srv._rows[1].n == 0 and srv._rows[0].rs["n_in"] == 0
    srv.push(s16, np.full(100, 16384, np.int16))
    torch.cuda.synchronize()
    assert srv._rows[0].n == 100 and bool((srv.window[0][:100] == 0.5).all())
    assert C.sizeof(ops.ResampleRow) == 88 and live.resample_row(48000, "s16", FS) == (48000, 1)


def _isolation_runs():
    x = [_pcm(24000, 51), _pcm(8000, 52).astype(np.float32) / 32768.0, _pcm(8000, 53).astype(np.float32) / 32768.0]
    runs = {}
    for kind in ("with", "without", "push"):
        srv = _server(3, 4, window_capacity=8192)
        sids = [srv.open(_first(3), _style(90 + r), **(dict(rate=48000, pcm="s16") if r == 0 else {})) for r in range(3)]
        parts = [[] for _ in range(3)]
        for i in range(8):
            call = {sids[r]: x[r][1000 * i:1000 * (i + 1)] for r in (1, 2)}
            if kind == "with":
                call[sids[0]] = x[0][3000 * i:3000 * (i + 1)]
            elif kind == "push":
                srv.push(sids[0], x[0][3000 * i:3000 * i + 1700])
                srv.push(sids[0], x[0][3000 * i + 1700:3000 * (i + 1)])
            srv.push_many(call)
            for sid, o in srv.drain().items():
                parts[sids.index(sid)].append(o)
        for r in range(3):
            parts[r].append(srv.close(sids[r]))
        runs[kind] = [_cat(p) if any(p) else None for p in parts]
    return runs
