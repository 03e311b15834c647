"""Host-only parts of LiveServer's running loudness normalisation: the float64 oracle (tests/live_loudness_oracle.py) against the
whole-signal meter it must end at, the margin that keeps the device comparison of tests/test_gpu_live_loudness.py honest, the
shared index / gate header on the host (tests/host/loud_math_check.cpp, plain and under sanitizers), include/zeggs_hip_loudness.h
against zeggs/capi.py, and every refusal that comes before a launch.  No GPU needed -- the library loads on the CPU for
host-only calls."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import live_loudness_oracle as oracle_ll
from oracle.loudness import Meter
from zeggs import audio, capi, live, ops

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "zeggs_hip_loudness.h"
FS = 16000
HORIZONS = (60.0, 2.0)
CONF = dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True, normalize_mel_bins=True,
            normalize_range=True, min_clipping=1e-5, sampling_rate=FS, mel_fmin=20, mel_fmax=7600, n_mel_channels=80,
            filter_length=800, hop_length=200, resample_method="linear", normalize_loudness=True)


# ----------------------------------------------------------------------------- 1, 2. the oracle
@pytest.mark.parametrize("name", ["speech", "gap", "quiet", "step"])
def test_oracle_ends_at_the_whole_signal_meter(name):
    """with a horizon that covers the clip the last running estimate is pyloudnorm's integrated loudness of the same float32
    samples (oracle/loudness.py: Meter), within the project's float32 bound 2e-5 (the lengths are whole hops: same blocks)"""
    x = oracle_ll.signals(FS)[name]
    assert x.dtype == np.float32 and (x.size - 6400) % 1600 == 0
    tr = oracle_ll.running_loudness(x, FS, horizon=60.0)
    want = Meter(FS).integrated_loudness(x)
    got = tr["blocks"][-1]["lufs"]
    print(f"{name}: running {got:.9f} LUFS, meter {want:.9f}, |diff| {abs(got - want):.2e}")
    assert len(tr["blocks"]) == (x.size - 6400) // 1600 + 1 and tr["blocks"][-1]["fresh"]
    assert abs(got - want) <= 2e-5


def test_no_block_of_the_test_signals_sits_on_a_gate():
    """every block in the ring stays >= 1e-3 dB away from both gates at every step, for every signal and horizon the GPU tests
    use: fifty times the 2e-5 dB a device level may deviate, so device and oracle must gate the same blocks.  Also what the
    signals are for: `step` reaches the +30 dB clamp, `quiet` at 2 s ends with every block gated out, `gap` at 2 s holds 8 steps"""
    sig = oracle_ll.signals(FS)
    tr = {(k, h): oracle_ll.running_loudness(x, FS, horizon=h) for k, x in sig.items() for h in HORIZONS}
    for key, t in tr.items():
        d = oracle_ll.min_gate_distance(t)
        print(key, f"closest block to a gate: {d:.4f} dB")
        assert d >= 1e-3, key
    assert max(float(b["g"]) for b in tr[("step", 60.0)]["blocks"]) == float(np.float32(10.0 ** 1.5))
    last = tr[("quiet", 2.0)]["blocks"][-1]
    assert last["gated"] == 0 and last["held"] and not last["fresh"]
    assert sum(b["held"] for b in tr[("gap", 2.0)]["blocks"]) == 8 and not any(b["held"] for b in tr[("gap", 60.0)]["blocks"])
    # the gain of a sample is that of the last block that ended at or before it
    t = tr[("step", 2.0)]
    for b, nxt in zip(t["blocks"], t["blocks"][1:]):
        assert (t["gain"][b["hi"]:nxt["hi"]] == b["g"]).all()
    assert (t["gain"][:t["blocks"][0]["hi"]] == 1.0).all()


# ----------------------------------------------------------------------------- 3. csrc/loud_math.h on the host
def _cxx():
    return shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_loudness_index_and_gate_rules_on_the_host(tmp_path, flags):
    """tests/host/loud_math_check.cpp: a stand-alone program over the header the kernel uses (its docstring says what it walks);
    once plain, once under the address and undefined-behaviour sanitizers (host code with its own main, run directly)"""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "loud_math_check"
    b = subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "loud_math_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "loud_math_check: ok"


# ----------------------------------------------------------------------------- 4. the third header against capi.LOUD_*
# (the rules tests/test_live_push_cpu.py applies to the second header)
_SCALARS = {"int": "int", "long": "long", "size_t": "size_t", "uint64_t": "uint64", "float": "float", "double": "double"}
_ELEMENTS = {"float": "f32*", "double": "f64*", "int": "i32*", "unsigned": "i32*", "int64_t": "i64*", "long": "i64*",
             "long long": "i64*", "uint8_t": "u8*", "unsigned char": "u8*", "char": "u8*", "void": "any*"}
_C_WORDS = {"int", "long", "unsigned", "char", "float", "double", "void", "size_t", "uint64_t", "int64_t", "uint8_t"}
_CTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
           "double": ctypes.c_double}


def _header_text():
    return re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)


def _declarator(text):
    """'const float* x' -> (base type, pointer depth, name or None, array length or None)"""
    m = re.search(r"\[(\d+)\]\s*$", text)
    text = text[:m.start()] if m else text
    depth = text.count("*")
    words = text.replace("*", " ").replace("const", " ").split()
    name = words.pop() if len(words) > 1 and words[-1] not in _C_WORDS and not words[-1].startswith("Zeggs") else None
    return " ".join(words), depth, name, int(m.group(1)) if m else None


def _header_prototypes():
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \*]*?)\b(zeggs_\w+)\s*\(([^()]*)\)\s*;", _header_text()):
        rbase, rdepth, _, _ = _declarator(ret + " f")
        plist = [] if params.strip() in ("", "void") else [_declarator(p)[:2] for p in params.split(",")]
        assert name not in out
        out[name] = (rbase, rdepth, plist)
    return out


def _header_structs():
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(Zeggs\w+)\s*;", _header_text(), flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = [p.strip() for p in decl.split(",")]
            base, depth, fname, n = _declarator(first)
            fields.append((fname, base, depth, n))
            for p in more:
                m = re.fullmatch(r"(\**)\s*(\w+)(?:\[(\d+)\])?", p)
                fields.append((m.group(2), base, len(m.group(1)), int(m.group(3)) if m.group(3) else None))
        out[name] = fields
    return out


def test_loudness_prototypes_are_the_third_header():
    """capi.LOUD_PROTOTYPES against include/zeggs_hip_loudness.h: the same names; per function the return kind, the parameter
    count, every parameter's kind and every device pointer's element type; the library exports them all and is version 109;
    the four tables of the other two headers are the size they were"""
    header = _header_prototypes()
    assert set(header) == set(capi.LOUD_PROTOTYPES) and len(header) == 5
    assert (len(capi.PROTOTYPES), len(capi.STRUCTS), len(capi.EXT_PROTOTYPES), len(capi.EXT_STRUCTS)) == (122, 21, 6, 2)
    assert not set(capi.LOUD_PROTOTYPES) & (set(capi.PROTOTYPES) | set(capi.EXT_PROTOTYPES))
    assert not set(capi.LOUD_STRUCTS) & (set(capi.STRUCTS) | set(capi.EXT_STRUCTS))
    assert {b for _, _, ps in header.values() for b, depth in ps if depth == 0} <= set(_SCALARS)       # no struct by value
    structs = {**capi.STRUCTS, **capi.EXT_STRUCTS, **capi.LOUD_STRUCTS}
    for name, (rbase, rdepth, params) in header.items():
        ret, kinds = capi.signature(name)
        want = {("int", 0): ("status", "mask", "int"), ("long", 0): ("long",), ("size_t", 0): ("size_t",), ("char", 1): ("str",)}
        assert ret in want[(rbase, rdepth)], (name, ret)
        assert len(kinds) == len(params), name
        for i, (kind, (base, depth)) in enumerate(zip(kinds, params)):
            where = (name, i, kind, base, depth)
            assert kind in capi.KINDS, where
            if depth == 0:
                assert kind == _SCALARS[base], where
            elif kind == "stream":
                assert (base, depth) == ("void", 1), where
            elif kind == "host*":
                assert depth >= 1, where
            elif base.startswith("Zeggs"):
                assert kind == base + "*" and depth == 1 and base in structs, where
            else:
                assert depth == 1 and kind == _ELEMENTS[base], where
    text = HEADER.read_text()
    assert '#include "zeggs_hip.h"' in text and "zeggs_version() >= 109" in text
    L, api = ops.lib(), capi.api()
    assert L.zeggs_version() == 109
    for n in header:
        assert hasattr(L, n), f"libzeggs_hip.so does not export {n}"
        assert getattr(api, n).argtypes is not None and getattr(L, n).argtypes is None


def test_loudness_struct_mirrors_are_the_third_header():
    structs = _header_structs()
    assert set(structs) == set(capi.LOUD_STRUCTS) == {"ZeggsLoudDims", "ZeggsLoudRow"}
    for name, fields in structs.items():
        mirror = capi.LOUD_STRUCTS[name]._fields_
        assert [f for f, _ in mirror] == [f for f, _, _, _ in fields], name
        for (f, ctype), (_, base, depth, n) in zip(mirror, fields):
            want = ctypes.c_void_p if depth else _CTYPES[base]
            assert ctype is (want * n if n else want) or (n and ctype._type_ is want and ctype._length_ == n), (name, f)
    assert ctypes.sizeof(capi.LoudRow) == 32 and ctypes.sizeof(capi.LoudDims) == 120
    assert int(re.search(r"#define ZEGGS_LOUD_READ_WORDS (\d+)", _header_text()).group(1)) == 8


# ----------------------------------------------------------------------------- 5. refusals
def test_loudness_none_still_refuses_the_shipped_conf():
    """loudness=None keeps today's behaviour: a conf with normalize_loudness true raises the same ValueError (before any weight is
    looked at); a gain at open() needs the feature"""
    with pytest.raises(ValueError, match="loudness normalisation needs the whole signal: apply audio.normalize_loudness\\(\\) first"):
        live.LiveServer(None, None, {}, CONF, 1 / 60.0)
    with pytest.raises(ValueError, match="loudness normalisation needs the whole signal"):
        live.LiveServer(None, None, {}, CONF, 1 / 60.0, loudness=None)


@pytest.mark.parametrize("bad,match", [
    (dict(horizon=0.0), "horizon"), (dict(horizon=-1.0), "horizon"), (dict(horizon=0.25), "multiple of 0.1"),
    (dict(horizon=float("nan")), "horizon"), (dict(warmup=0), "warmup"), (dict(warmup=1.5), "warmup"),
    (dict(gain_db=(3.0, -3.0)), "gain_db"), (dict(gain_db=(0.0,)), "loudness options"), (dict(horizont=2.0), "keys"),
    ("on", "None, 'running' or a dict"), (dict(target=float("inf")), "target"),
])
def test_loudness_options_are_checked_at_construction(bad, match):
    with pytest.raises(ValueError, match=match):
        live.LiveServer(None, None, {}, CONF, 1 / 60.0, loudness=bad)


def test_loudness_options_defaults():
    assert live.loudness_options(None) is None
    assert live.loudness_options("running") == dict(target=-20.0, horizon=60.0, warmup=1, gain_db=(-30.0, 30.0), ring_blocks=600)
    got = live.loudness_options(dict(horizon=2.0, warmup=3, gain_db=[-6, 12], target=-23))
    assert got == dict(target=-23.0, horizon=2.0, warmup=3, gain_db=(-6.0, 12.0), ring_blocks=20)
    assert live.loudness_options(dict(horizon=0.3))["ring_blocks"] == 3


def _dims(rows=4, nb=20, warmup=1, fs=FS, gain=(-30.0, 30.0)):
    coef = [c for b, a in audio._kweighting(fs) for c in (b[0], b[1], b[2], a[1], a[2])]
    return capi.LoudDims(fs, rows, nb, warmup, -20.0, gain[0], gain[1], (ctypes.c_double * 10)(*coef))


def _recs(*rows):
    arr = (capi.LoudRow * len(rows))()
    for q, (src, dst, count, row) in zip(arr, rows):
        q.src, q.dst, q.count, q.row = src, dst, count, row
    return arr


def test_loudness_state_size():
    """per row: a 128-byte head, one gating block of filtered samples, ring_blocks energies and their levels, as doubles"""
    api = capi.api()
    assert api.zeggs_live_loudness_state_bytes(_dims(4, 20)) == 4 * (128 + 8 * (6400 + 2 * 20))
    assert api.zeggs_live_loudness_state_bytes(_dims(1, 600, fs=48000)) == 128 + 8 * (19200 + 1200)
    for bad in (_dims(0), _dims(65), _dims(nb=0), _dims(warmup=0), _dims(gain=(1.0, 0.0)), _dims(fs=500)):
        assert api.zeggs_live_loudness_state_bytes(bad) == 0


@pytest.mark.parametrize("what,rows,dev,match", [
    ("a row out of range", [(0x10000, 0x20000, 8, 4)], None, "record 0: row 4 of 4"),
    ("a negative row", [(0x10000, 0x20000, 8, 0), (0x30000, 0x40000, 8, -1)], 0x7000, "record 1: row -1 of 4"),
    ("a row twice", [(0x10000, 0x20000, 8, 2), (0x30000, 0x40000, 8, 1), (0x50000, 0x60000, 8, 2)], 0x7000, "record 2: row 2 twice"),
    ("a negative count", [(0x10000, 0x20000, -1, 0)], None, "record 0: negative count -1"),
    ("a NULL source", [(0, 0x20000, 8, 0)], None, "record 0: NULL or misaligned"),
    ("a NULL destination", [(0x10000, 0x20000, 8, 0), (0x30000, 0, 8, 1)], 0x7000, "record 1: NULL or misaligned"),
    ("a misaligned pointer", [(0x10002, 0x20000, 8, 0)], None, "record 0: NULL or misaligned"),
    ("source over destination", [(0x10000, 0x10000 + 4 * 7, 8, 0)], None, "record 0: source and destination overlap"),
    ("two records without a device copy", [(0x10000, 0x20000, 8, 0), (0x30000, 0x40000, 8, 1)], None, "must also be in device memory"),
    ("more records than rows", [(0x10000 * (i + 1), 0x100000 * (i + 1), 8, i % 4) for i in range(5)], 0x7000, "5 records for 4 rows"),
])
def test_loudness_push_refuses_on_the_host(what, rows, dev, match):
    """every refusal comes before the launch (the addresses are never followed, there is no device here), with the record named"""
    d, arr = _dims(), _recs(*rows)
    nbytes = capi.api().zeggs_live_loudness_state_bytes(d)
    dev_p = ctypes.cast(ctypes.c_void_p(dev), ctypes.POINTER(capi.LoudRow)) if dev else None
    with pytest.raises(RuntimeError, match="zeggs_live_loudness_push: live loudness push: .*" + match):
        capi.api().zeggs_live_loudness_push(d, arr, dev_p, len(rows), ctypes.c_void_p(0x900000), nbytes, None)
    assert ops.lib().zeggs_live_loudness_push(ctypes.byref(d), arr, ctypes.c_void_p(dev or 0), len(rows), ctypes.c_void_p(0x900000),
                                              ctypes.c_size_t(nbytes), None) == -1


def test_loudness_entry_points_check_state_and_row():
    api, d = capi.api(), _dims()
    nbytes = api.zeggs_live_loudness_state_bytes(d)
    state = ctypes.c_void_p(0x900000)
    with pytest.raises(RuntimeError, match="state too small"):
        api.zeggs_live_loudness_push(d, _recs((0x10000, 0x20000, 8, 0)), None, 1, state, nbytes - 1, None)
    with pytest.raises(RuntimeError, match="NULL state"):
        api.zeggs_live_loudness_reset(d, None, nbytes, 0, 1.0, None)
    with pytest.raises(RuntimeError, match="reset: row 4 of 4"):
        api.zeggs_live_loudness_reset(d, state, nbytes, 4, 1.0, None)
    with pytest.raises(RuntimeError, match="reset: gain"):
        api.zeggs_live_loudness_reset(d, state, nbytes, 0, float("nan"), None)
    with pytest.raises(RuntimeError, match="hold: row -1 of 4"):
        api.zeggs_live_loudness_hold(d, state, nbytes, -1, 1, None)
    with pytest.raises(RuntimeError, match="read: row 9 of 4"):
        api.zeggs_live_loudness_read(d, state, nbytes, 9, ctypes.addressof((ctypes.c_double * 8)()), None)
    with pytest.raises(RuntimeError, match="warmup 0"):
        api.zeggs_live_loudness_hold(_dims(warmup=0), state, nbytes, 0, 1, None)
    # nothing to do: no launch, no error
    assert api.zeggs_live_loudness_push(d, None, None, 0, state, nbytes, None) == 0
    assert api.zeggs_live_loudness_push(d, _recs((0, 0, 0, 1), (0, 0, 0, 3)), None, 2, state, nbytes, None) == 0
