"""Host-only parts of LiveServer's rate converter: the coefficient table against the float64 oracle
(tests/live_resample_oracle.py) and against its design figures, ready / total against brute force, the oracle's independence of
the cuts and its accuracy on tones, the shared index header on the host (tests/host/resample_math_check.cpp, plain and under
sanitizers), include/zeggs_hip_resample.h against zeggs/capi.py, and every refusal that comes before a launch.  No GPU needed --
the library loads on the CPU for host-only calls."""
import ctypes
import re
import shutil
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import live_resample_oracle as oracle_rs
import test_live_loudness_cpu as third
from zeggs import audio, capi, live, ops

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "zeggs_hip_resample.h"
FS = 16000
RATIOS = [(48000, 16000), (44100, 16000), (8000, 16000), (22050, 16000), (32000, 16000), (24000, 16000)]   # 3:1 441:160 1:2 441:320 2:1 3:2
CONF = dict(third.CONF, normalize_loudness=False)


# ----------------------------------------------------------------------------- 1. the table
@pytest.mark.parametrize("fi,fo,Z", [(fi, fo, Z) for fi, fo in RATIOS + [(16000, 48000)] for Z in (4, 64)] + [(11025, 16000, 4)])
def test_table_is_the_oracles_filter(fi, fo, Z):
    """audio.resample_table against h() of the oracle at t = phase / L + H - j, to 1e-15 relative.  Relative to the filter's
    peak c = h(0): sinc has zero crossings inside the support, next to which the value of two independent evaluations has no
    relative accuracy of its own, and an error of a coefficient enters an output in proportion to the peak.  The layout: L rows
    of 2 ceil(W) + 1 taps, zero exactly where |t| >= W, and (L, M, WL) the reduced ratio and Z max(L, M)."""
    tab, (L, M, WL) = audio.resample_table(fi, fo, zero_crossings=Z)
    assert (L, M) == oracle_rs.ratio(fi, fo) and WL == Z * max(L, M)
    W = oracle_rs.width(L, M, Z)
    H = -(-WL // L)
    assert H == -(-W.numerator // W.denominator) and tab.shape == (L, 2 * H + 1) and tab.dtype == np.float64
    t = np.arange(L)[:, None] / L + (H - np.arange(2 * H + 1))[None, :]
    want = oracle_rs.h(t, L, M, Z)
    peak = float(np.abs(want).max())
    err = float(np.abs(tab - want).max()) / peak
    print(f"{fi} -> {fo} Z {Z}: {L} x {tab.shape[1]} taps, max |table - h| / peak = {err:.2e}")
    assert abs(peak - 0.95 * min(1.0, L / M)) < 1e-15
    assert err <= 1e-15
    assert (tab[np.abs(t) >= float(W)] == 0.0).all() and (tab[np.abs(t) < float(W) - 1e-9] != 0.0).mean() > 0.99


def _response(fi, fo):
    """|G(f)| / L of the default table's prototype filter g[n] = h(n / L) on a fine grid -> (f in units of the lower Nyquist
    frequency, magnitude)"""
    tab, (L, M, WL) = audio.resample_table(fi, fo)
    H = (tab.shape[1] - 1) // 2
    proto = np.zeros(2 * H * L + L)
    for ph in range(L):
        proto[(H - np.arange(2 * H + 1)) * L + ph + H * L] = tab[ph]
    n = 1 << 22
    mag = np.abs(np.fft.rfft(proto, n)) / L
    f = np.arange(mag.size) / n * 2 * max(L, M)      # cycles per prototype sample -> units of the lower Nyquist frequency
    return f, mag, tab


@pytest.mark.parametrize("fi", [48000, 44100, 8000])
def test_default_table_meets_its_design_figures(fi):
    """Z = 64, rolloff 0.95, beta 10 -> 16 kHz: pass-band ripple <= 0.001 dB up to 0.9 of the lower Nyquist frequency
    (0.0002 dB by design), <= -95 dB from it upward (-99.5 dB by design), about -6 dB at 0.95; every phase sums to 1 within 1e-5"""
    f, mag, tab = _response(fi, FS)
    db = 20 * np.log10(np.maximum(mag, 1e-300))
    ripple, stop = float(np.abs(db[f <= 0.9]).max()), float(db[f >= 1.0].max())
    at95 = float(db[np.argmin(np.abs(f - 0.95))])
    dc = float(np.abs(tab.sum(axis=1) - 1.0).max())
    print(f"{fi} Hz: ripple {ripple:.5f} dB, {at95:.2f} dB at 0.95, stop band {stop:.1f} dB, {tab.shape[1]} taps, |DC - 1| {dc:.1e}")
    assert ripple <= 0.001 and stop <= -95.0 and -6.5 <= at95 <= -5.7
    assert dc <= 1e-5
    if fi == 48000:
        assert tab.shape == (1, 385)


# ----------------------------------------------------------------------------- 2. ready / total
@pytest.mark.parametrize("fi,fo", RATIOS)
@pytest.mark.parametrize("Z", [4, 64])
def test_ready_and_total_against_brute_force(fi, fo, Z):
    """audio.resample_ready / resample_total for n = 0 .. 2000 against exact rational arithmetic over the rule p_m + W <= n
    (resp. p_m < n); a ready output's last tap is below n, and the first output that is not ready reaches n or beyond"""
    L, M = oracle_rs.ratio(fi, fo)
    WL = Z * max(L, M)
    for n in list(range(0, 2001, 7)) + list(range(0, 130)) + [1999, 2000]:
        r = audio.resample_ready(n, L, M, WL)
        assert r == oracle_rs.ready_brute(n, L, M, Z), (n, r)
        assert audio.resample_total(n, L, M) == oracle_rs.total_brute(n, L, M), n
        if r:
            assert oracle_rs.support(r - 1, L, M, Z)[1] < n
        assert oracle_rs.support(r, L, M, Z)[1] >= n
    prev = -1
    for n in range(0, 2001):                                    # every n: against the brute-force count walked forward
        r = audio.resample_ready(n, L, M, WL)
        assert r >= max(prev, 0) and (r == 0 or oracle_rs.support(r - 1, L, M, Z)[1] < n <= oracle_rs.support(r, L, M, Z)[1])
        assert r > 0 or oracle_rs.support(0, L, M, Z)[1] >= n
        assert audio.resample_total(n, L, M) == -(-n * L // M) >= r
        prev = r
    assert audio.resample_ready(123, 1, 1, 0) == 123 and audio.resample_total(123, 1, 1) == 123
    assert audio.resample_history(L, WL) == -(-2 * WL // L)


# ----------------------------------------------------------------------------- 3. the oracle itself
@pytest.mark.parametrize("fi,fo", [(48000, 16000), (44100, 16000), (8000, 16000), (22050, 16000)])
def test_oracle_does_not_depend_on_the_cuts(fi, fo):
    """the outputs computed from the prefix alone at ready(n), for random cuts of 1..96 samples, and the tail at close equal
    those of the whole signal bit for bit"""
    x = np.random.default_rng(fi).standard_normal(700)
    want = oracle_rs.whole(x, fi, fo, Z=4)
    for seed in (1, 2):
        st, parts, pos = oracle_rs.Stream(fi, fo, Z=4), [], 0
        for m in oracle_rs.cuts(x.size, seed):
            parts.append(st.push(x[pos:pos + m]))
            pos += m
        mid = sum(p.size for p in parts)
        parts.append(st.close())
        got = np.concatenate(parts)
        assert 0 < mid < got.size == want.size == -(-x.size * fo // fi)
        assert got.tobytes() == want.tobytes()


def test_oracle_on_tones():
    """with the defaults, 48 kHz -> 16 kHz: a 1 kHz sine comes out as the 16 kHz sine within 1e-6 in the interior (3.0e-7 by
    design), an 11 kHz tone (beyond the new Nyquist frequency) leaks at most 1e-5 (1.6e-6 by design)"""
    n = 4800
    k = np.arange(n)
    m = np.arange(200, n // 3 - 200)                 # interior: the support (64 output samples) is inside the signal
    L, M = 1, 3
    for f0, bound in ((1000.0, 1e-6), (11000.0, 1e-5)):
        x = np.sin(2 * np.pi * f0 * k / 48000.0)
        y = np.array([oracle_rs.output(int(i), x, L, M) for i in m])
        want = np.sin(2 * np.pi * f0 * m / 16000.0) if f0 < 8000 else np.zeros(m.size)
        err = float(np.abs(y - want).max())
        print(f"{f0:.0f} Hz: max |oracle - ideal| = {err:.2e}")
        assert err <= bound


# ----------------------------------------------------------------------------- 4. csrc/resample_math.h on the host
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_resample_index_rules_on_the_host(tmp_path, flags):
    """tests/host/resample_math_check.cpp: a stand-alone program over the header the kernel uses (its head says what it walks);
    once plain, once under the address and undefined-behaviour sanitizers (host code with its own main, run directly)"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "resample_math_check"
    b = subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "resample_math_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "resample_math_check: ok"


# ----------------------------------------------------------------------------- 5. the fourth header against capi.RS_*
# (the parser of tests/test_live_loudness_cpu.py, pointed at the fourth header)
@pytest.fixture
def fourth(monkeypatch):
    monkeypatch.setattr(third, "HEADER", HEADER)
    return third


def test_resample_prototypes_are_the_fourth_header(fourth):
    """capi.RS_PROTOTYPES against include/zeggs_hip_resample.h: the same names; per function the return kind, the parameter count,
    every parameter's kind and every device pointer's element type; the library exports them all, zeggs_version() is still 109
    and zeggs_live_resample_version() is 1; the tables of the other three headers are the size they were"""
    header = fourth._header_prototypes()
    assert set(header) == set(capi.RS_PROTOTYPES) and len(header) == 6
    assert (len(capi.PROTOTYPES), len(capi.STRUCTS), len(capi.EXT_PROTOTYPES), len(capi.EXT_STRUCTS)) == (122, 21, 6, 2)
    assert (len(capi.LOUD_PROTOTYPES), len(capi.LOUD_STRUCTS)) == (5, 2)
    others = set(capi.PROTOTYPES) | set(capi.EXT_PROTOTYPES) | set(capi.LOUD_PROTOTYPES)
    assert not set(capi.RS_PROTOTYPES) & others
    assert not set(capi.RS_STRUCTS) & (set(capi.STRUCTS) | set(capi.EXT_STRUCTS) | set(capi.LOUD_STRUCTS))
    assert {b for _, _, ps in header.values() for b, depth in ps if depth == 0} <= set(fourth._SCALARS)       # no struct by value
    for name, (rbase, rdepth, params) in header.items():
        ret, kinds = capi.signature(name)
        want = {("int", 0): ("status", "mask", "int"), ("long", 0): ("long",), ("size_t", 0): ("size_t",), ("char", 1): ("str",)}
        assert ret in want[(rbase, rdepth)], (name, ret)
        assert len(kinds) == len(params), name
        for i, (kind, (base, depth)) in enumerate(zip(kinds, params)):
            where = (name, i, kind, base, depth)
            assert kind in capi.KINDS, where
            if depth == 0:
                assert kind == fourth._SCALARS[base], where
            elif kind == "stream":
                assert (base, depth) == ("void", 1), where
            elif kind == "host*":
                assert depth >= 1, where
            elif base.startswith("Zeggs"):
                assert kind == base + "*" and depth == 1 and base in capi.RS_STRUCTS, where
            else:
                assert depth == 1 and kind == fourth._ELEMENTS[base], where
    text = HEADER.read_text()
    assert '#include "zeggs_hip.h"' in text and "zeggs_live_resample_version() >= 1" in text
    L, api = ops.lib(), capi.api()
    assert L.zeggs_version() == 109 and L.zeggs_live_resample_version() == 1 and api.zeggs_live_resample_version() == 1
    for n in header:
        assert hasattr(L, n), f"libzeggs_hip.so does not export {n}"
        assert getattr(api, n).argtypes is not None and getattr(L, n).argtypes is None
    build = (ROOT / "ubisoft-laforge-zeroeggs_amd" / "csrc" / "build.sh").read_text()
    assert " live_resample\"" in build and "../../include/zeggs_hip_resample.h" in build


def test_resample_struct_mirrors_are_the_fourth_header(fourth):
    structs = fourth._header_structs()
    assert set(structs) == set(capi.RS_STRUCTS) == {"ZeggsResampleDims", "ZeggsResampleRow"}
    for name, fields in structs.items():
        mirror = capi.RS_STRUCTS[name]._fields_
        assert [f for f, _ in mirror] == [f for f, _, _, _ in fields], name
        for (f, ctype), (_, base, depth, n) in zip(mirror, fields):
            want = ctypes.c_void_p if depth else fourth._CTYPES[base]
            assert ctype is want and n is None, (name, f)
    assert ctypes.sizeof(capi.ResampleRow) == 88 and ctypes.sizeof(capi.ResampleDims) == 8
    defs = dict(re.findall(r"#define (ZEGGS_RS_\w+) (\d+)", fourth._header_text()))
    assert (int(defs["ZEGGS_RS_F32"]), int(defs["ZEGGS_RS_S16"])) == (ops.RS_F32, ops.RS_S16) == (0, 1)
    assert int(defs["ZEGGS_RS_MAX_HISTORY"]) == 2 * audio.RESAMPLE_MAX_ZERO_CROSSINGS * audio.RESAMPLE_MAX_DECIMATION == 3072


# ----------------------------------------------------------------------------- 6. refusals
def _dims(rows=4, history=3072):
    return capi.ResampleDims(rows, history)


GOOD = dict(src=0x10000, dst=0x20000, table=0x30000, count=96, n_in=0, n_out=0, outputs=None, WL=12, row=0, format=0, final=0, L=1, M=3)


def _recs(*rows):
    """records from GOOD (48 kHz -> 16 kHz, Z = 4) with overrides; outputs None: what ready() / total() ask for"""
    arr = (capi.ResampleRow * len(rows))()
    for q, over in zip(arr, rows):
        f = dict(GOOD, **over)
        if f["outputs"] is None:
            n1 = f["n_in"] + max(f["count"], 0)
            due = audio.resample_total(n1, f["L"], f["M"]) if f["final"] else audio.resample_ready(n1, f["L"], f["M"], f["WL"])
            f["outputs"] = due - f["n_out"]
        for k, v in f.items():
            setattr(q, k, v)
    return arr


def test_resample_state_size():
    """per row `history` float32 samples; the server sizes it for 64 zero crossings at the largest decimation"""
    api = capi.api()
    assert api.zeggs_resample_state_bytes(_dims(4, 3072)) == 4 * 3072 * 4
    assert api.zeggs_resample_state_bytes(_dims(64, 384)) == 64 * 384 * 4
    for bad in (_dims(0), _dims(65), _dims(4, 0), _dims(4, -1)):
        assert api.zeggs_resample_state_bytes(bad) == 0
    assert audio.resample_history(1, 64 * 24) == 3072


@pytest.mark.parametrize("what,rows,dev,match", [
    ("a row out of range", [dict(row=4)], None, "record 0: row 4 of 4"),
    ("a negative row", [dict(), dict(row=-1)], 0x7000, "record 1: row -1 of 4"),
    ("a row twice", [dict(row=2), dict(row=1), dict(row=2)], 0x7000, "record 2: row 2 twice"),
    ("a negative count", [dict(count=-1, outputs=0)], None, "record 0: negative count -1"),
    ("an unknown format", [dict(format=2)], None, "record 0: format 2"),
    ("a NULL source", [dict(src=0)], None, "record 0: NULL or misaligned source"),
    ("a NULL destination", [dict(), dict(row=1, dst=0)], 0x7000, "record 1: NULL or misaligned destination"),
    ("a NULL table", [dict(table=0)], None, "record 0: NULL or misaligned table"),
    ("a misaligned float source", [dict(src=0x10002)], None, "record 0: NULL or misaligned source"),
    ("a misaligned PCM source", [dict(src=0x10001, format=1)], None, "record 0: NULL or misaligned source"),
    ("a misaligned destination", [dict(dst=0x20002)], None, "record 0: NULL or misaligned destination"),
    ("a misaligned table", [dict(table=0x30004)], None, "record 0: NULL or misaligned table"),
    ("outputs that disagree with ready", [dict(outputs=30)], None, "record 0: 30 outputs disagree with ready\\(96\\) - 0 = 29"),
    ("outputs that disagree with total", [dict(final=1, outputs=29)], None, "record 0: 29 outputs disagree with total\\(96\\) - 0 = 32"),
    ("counters that disagree", [dict(n_in=96, n_out=28)], None, "record 0: 28 outputs before the call disagree with ready\\(96\\) = 29"),
    ("a ratio outside the supported ones", [dict(L=1, M=25, WL=100)], None, "record 0: ratio L / M = 1 / 25"),
    ("a ratio that is not reduced", [dict(L=2, M=6, WL=24)], None, "record 0: ratio L / M = 2 / 6"),
    ("a support that is no multiple", [dict(WL=13)], None, "record 0: support WL = 13"),
    ("pass-through at a ratio", [dict(WL=0)], None, "record 0: pass-through"),
    ("more zero crossings than the kernel stages", [dict(WL=3 * 65)], None, "record 0: support WL = 195"),
    ("two records without a device copy", [dict(), dict(row=1)], None, "must also be in device memory"),
    ("more records than rows", [dict(row=i % 4) for i in range(5)], 0x7000, "5 records for 4 rows"),
])
def test_resample_push_refuses_on_the_host(what, rows, dev, match):
    """every refusal comes before the launch (the addresses are never followed, there is no device here), with the record named"""
    d, arr = _dims(), _recs(*rows)
    nbytes = capi.api().zeggs_resample_state_bytes(d)
    dev_p = ctypes.cast(ctypes.c_void_p(dev), ctypes.POINTER(capi.ResampleRow)) if dev else None
    with pytest.raises(RuntimeError, match="zeggs_resample_push: resample push: .*" + match):
        capi.api().zeggs_resample_push(d, arr, dev_p, len(rows), ctypes.c_void_p(0x900000), nbytes, None)
    assert ops.lib().zeggs_resample_push(ctypes.byref(d), arr, ctypes.c_void_p(dev or 0), len(rows), ctypes.c_void_p(0x900000),
                                         ctypes.c_size_t(nbytes), None) == -1


def test_resample_entry_points_check_state_row_and_whole():
    api, d = capi.api(), _dims()
    nbytes = api.zeggs_resample_state_bytes(d)
    state = ctypes.c_void_p(0x900000)
    with pytest.raises(RuntimeError, match="state too small"):
        api.zeggs_resample_push(d, _recs({}), None, 1, state, nbytes - 1, None)
    with pytest.raises(RuntimeError, match="NULL state"):
        api.zeggs_resample_reset(d, None, nbytes, 0, None)
    with pytest.raises(RuntimeError, match="record 0: a history of 384 samples, the state holds 100"):
        api.zeggs_resample_push(_dims(4, 100), _recs(dict(WL=192, count=0, src=0, dst=0)), None, 1, state, nbytes, None)
    with pytest.raises(RuntimeError, match="reset: row 4 of 4"):
        api.zeggs_resample_reset(d, state, nbytes, 4, None)
    with pytest.raises(RuntimeError, match="64 rows|rows \\(1..64\\)"):
        api.zeggs_resample_reset(_dims(65), state, nbytes, 0, None)
    # the flush takes the one record as final whatever its flag says
    with pytest.raises(RuntimeError, match="zeggs_resample_flush: resample flush: record 0: 0 outputs disagree with total\\(96\\) - 29 = 3"):
        api.zeggs_resample_flush(d, _recs(dict(n_in=96, n_out=29, count=0, outputs=0)), state, nbytes, None)
    # nothing to do: no launch, no error
    assert api.zeggs_resample_push(d, None, None, 0, state, nbytes, None) == 0
    assert api.zeggs_resample_push(d, _recs(dict(count=0, src=0, dst=0), dict(count=0, row=3, src=0, dst=0)), None, 2, state, nbytes, None) == 0
    # the whole-signal call
    p = ctypes.c_void_p
    whole = ops.lib().zeggs_resample_whole
    args = lambda **k: [p(k.get("table", 0x30000)), k.get("L", 1), k.get("M", 3), ctypes.c_long(k.get("WL", 12)), p(k.get("src", 0x10000)),  # noqa: E731
                        k.get("fmt", 0), ctypes.c_long(k.get("n_in", 96)), p(k.get("dst", 0x20000)), ctypes.c_long(k.get("n_out", 32)), None]
    for bad, match in ((dict(n_out=29), "29 outputs, 96 inputs at 1 / 3 give 32"), (dict(src=0), "NULL or misaligned source"),
                       (dict(dst=0x20001), "NULL or misaligned destination"), (dict(table=0), "NULL or misaligned table"),
                       (dict(fmt=7), "format 7"), (dict(M=30, WL=120), "ratio L / M = 1 / 30"), (dict(n_in=-1, n_out=0), "-1 input samples")):
        assert whole(*args(**bad)) == -1
        assert re.search(match, ops.lib().zeggs_last_error().decode()), (bad, ops.lib().zeggs_last_error().decode())
    assert whole(*args(n_in=0, n_out=0, src=0, dst=0)) == 0


@pytest.mark.parametrize("bad,match", [
    (dict(zero_crossings=0), "zero_crossings"), (dict(zero_crossings=65), "zero_crossings"), (dict(zero_crossings=7.5), "zero_crossings"),
    (dict(rolloff=0.0), "rolloff"), (dict(rolloff=1.01), "rolloff"), (dict(rolloff=float("nan")), "rolloff"), (dict(beta=-1.0), "beta"),
    (dict(beta=float("inf")), "beta"), (dict(zero_crossing=8), "keys"), ("kaiser", "a dict with keys"), (dict(beta="x"), "options"),
])
def test_resample_options_are_checked_at_construction(bad, match):
    """before any weight is looked at"""
    with pytest.raises(ValueError, match=match):
        live.LiveServer(None, None, {}, CONF, 1 / 60.0, resample=bad)


def test_resample_options_defaults():
    assert audio.resample_options(None) == dict(zero_crossings=64, rolloff=0.95, beta=10.0) == audio.RESAMPLE_DEFAULTS
    assert audio.resample_options(dict(zero_crossings=8, beta=6)) == dict(zero_crossings=8, rolloff=0.95, beta=6.0)


def test_rates_and_formats_are_checked_at_open():
    """open() decides before it touches a row: today's row for rate None / the server's own with f32; every supported rate; a
    ValueError naming both rates for the others; an unknown format"""
    assert live.resample_row(None, "f32", FS) is None and live.resample_row(16000, "f32", FS) is None
    assert live.resample_row(None, "s16", FS) == (16000, ops.RS_S16) and live.resample_row(16000.0, "s16", FS) == (16000, ops.RS_S16)
    for fi in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000, 384000):
        assert live.resample_row(fi, "f32", FS) == (fi, ops.RS_F32) and live.resample_row(fi, "s16", FS) == (fi, ops.RS_S16)
    stub = types.SimpleNamespace(fs=FS, _loud=None)
    for bad in (400000, 16001, 44101, 0, -48000, 44100.5, "48k"):
        for call in (lambda: live.resample_row(bad, "s16", FS), lambda: live.LiveServer.open(stub, None, None, rate=bad)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(bad) in str(e.value) and "16000" in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="pcm 's24'"):
        live.LiveServer.open(stub, None, None, rate=48000, pcm="s24")
    with pytest.raises(ValueError, match="400000 Hz -> 16000 Hz is the ratio 1 / 25"):
        audio.resample_table(400000, 16000)


def test_a_chunk_must_match_the_rows_format():
    s16, f32 = dict(fmt=ops.RS_S16), dict(fmt=ops.RS_F32)
    pcm = np.arange(-4, 4, dtype=np.int16)
    assert live._samples(pcm, s16).dtype == np.int16 and live._samples(pcm.reshape(2, 4), s16).shape == (8,)
    for rs in (None, f32):
        got = live._samples(np.linspace(-1, 1, 5), rs)
        assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
        assert live._samples([0.0, 0.5], rs).dtype == np.float32
        with pytest.raises(TypeError, match="float samples"):
            live._samples(pcm, rs)
    for bad in (pcm.astype(np.float32), pcm.astype(np.int32), [1, 2, 3]):
        with pytest.raises(TypeError, match="int16 samples"):
            live._samples(bad, s16)


def test_offline_readers_still_refuse_a_foreign_rate(tmp_path):
    """the capability lives where the audio arrives: data_pipeline.read_wav keeps raising at a rate that is not the conf's"""
    import wave
    from zeggs import data_pipeline
    path = tmp_path / "x.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(48000)
        w.writeframes(np.zeros(480, np.int16).tobytes())
    with pytest.raises(ValueError, match="expected a 16000 Hz wav \\(got 48000 Hz\\)"):
        data_pipeline.read_wav(str(path), 16000)


# ----------------------------------------------------------------------------- 7. the staging block of a server that converts nothing
@pytest.mark.parametrize("loud_rows", [0, 4])
def test_staging_offsets_without_converting_rows_are_unchanged(monkeypatch, loud_rows):
    """_Staging(rows, n_samples, dev, loud_rows): [copy records | second launch | mel records | loudness records | samples], every
    area on a 64-byte boundary, and nothing behind the samples; with converting rows the records and the raw input follow the
    samples the CALL stages, and the four offsets stay where they are"""
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    a64 = lambda x: (x + 63) // 64 * 64  # noqa: E731
    rows, n = 4, 1000
    st = live._Staging(rows, n, "cpu", loud_rows)
    o_back = a64(3 * rows * ctypes.sizeof(ops.Seg))
    o_mel = o_back + a64(rows * ctypes.sizeof(ops.Seg))
    o_loud = o_mel + a64(rows * ctypes.sizeof(ops.MelRow))
    o_smp = o_loud + a64(loud_rows * ctypes.sizeof(ops.LoudRow))
    assert (st.o_back, st.o_mel, st.o_loud, st.o_smp) == (o_back, o_mel, o_loud, o_smp)
    assert st.nbytes == o_smp + 4 * n and st.tail_bytes == 0 and st.view[0]["smp"].size == n
    big = live._Staging(rows, n, "cpu", loud_rows, 4096)
    assert (big.o_back, big.o_mel, big.o_loud, big.o_smp) == (o_back, o_mel, o_loud, o_smp) and big.nbytes == st.nbytes + 4096
    o_rs, o_raw, end = big.tail(100, 2, 640)
    assert o_rs == a64(o_smp + 400) and o_raw == o_rs + a64(2 * ctypes.sizeof(ops.ResampleRow)) and end == o_raw + 640 <= big.nbytes
