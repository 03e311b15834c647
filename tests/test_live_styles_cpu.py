"""Host-only parts of LiveServer's named styles: the shared mix header on the host (tests/host/style_math_check.cpp, plain and under
sanitizers) against the float64 oracle (tests/live_styles_oracle.py), include/zeggs_hip_styles.h against zeggs/capi.py, every
refusal that comes before a launch, and the Python side's parsing.  No GPU needed -- the library loads on the CPU for host-only
calls."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import live_styles_oracle as oracle_sb
from zeggs import capi, live, ops

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "zeggs_hip_styles.h"
CONF = dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True, normalize_mel_bins=True,
            normalize_range=True, min_clipping=1e-5, sampling_rate=16000, mel_fmin=20, mel_fmax=7600, n_mel_channels=80,
            filter_length=800, hop_length=200, resample_method="linear", normalize_loudness=False)
ST = 5


# ----------------------------------------------------------------------------- 1. csrc/style_math.h on the host, against the oracle
def _cxx():
    return shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")


def _same(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_mix_arithmetic_on_the_host_equals_the_oracle(tmp_path, flags):
    """tests/host/style_math_check.cpp: a stand-alone program over the header the kernels use (its head says what it walks and
    what it checks itself); once plain, once under the address and undefined-behaviour sanitizers (host code with its own main,
    run directly).  Every row of its table is recomputed here by the numpy oracle from the row's own inputs: the new row within
    1/2 ulp32 + 2^-48 sum |w v|, the old row bit for bit (the uncontracted float32 lerp: the host build has no fused multiply-add
    unless asked for one -- either form passes), a slot's mean bit for bit and its deviation within 2 ulp; the names say that
    every case was walked."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "style_math_check"
    b = subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "style_math_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "style_math_check: ok"
    bank, eps, names, worst = np.zeros((4, 2, ST), np.float32), np.zeros((8, ST), np.float32), set(), 0.0
    for line in lines[:-1]:
        kind, name, *rest = line.split()
        if kind == "bank":
            bank[int(name)] = np.array(rest, np.float64).astype(np.float32).reshape(2, ST)
        elif kind == "eps":
            eps[int(name)] = np.array(rest, np.float64).astype(np.float32)
    assert np.abs(bank).max() > 0 and np.abs(eps).max() > 0
    for line in lines[:-1]:
        kind, name, *rest = line.split()
        if kind in ("bank", "eps"):
            continue
        bar = rest.index("|")
        v, got = rest[:bar], np.array(rest[bar + 1:], np.float64).astype(np.float32)
        names.add(name)
        if kind == "put":
            E = int(v[0])
            enc = np.array(v[1:], np.float64).astype(np.float32)
            assert enc.size == E and got.size == 2 * ST, line
            mean, dev = oracle_sb.slot_of(enc, ST)
            assert _same(got[:ST], mean.astype(np.float32)), line
            assert (np.abs(got[ST:].astype(np.float64) - dev) <= 2 * oracle_sb.ulp32(dev) * (dev > 0)).all(), line
            continue
        assert kind == "mix", line
        terms, t = int(v[0]), float(v[1])
        k, k_style, fade, reset, noise = (int(x) for x in v[2:7])
        slots = [int(x) for x in v[7:7 + terms]]
        wts = [float(x) for x in v[7 + terms:7 + 2 * terms]]
        old, new = (np.array(v[7 + 2 * terms + i * ST:7 + 2 * terms + (i + 1) * ST], np.float64).astype(np.float32) for i in (0, 1))
        assert len(v) == 7 + 2 * terms + 2 * ST and got.size == 2 * ST, line
        want, mag = oracle_sb.mix(bank, list(zip(slots, wts)), t, eps if noise else None)
        err, bound = np.abs(got[ST:].astype(np.float64) - want), oracle_sb.bound(want, mag)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (line, err, bound)
        if reset:
            assert _same(got[:ST], got[ST:]), line
        else:
            w = np.float32(oracle_sb.weight(k - 1, k_style, fade))
            assert _same(got[:ST], oracle_sb.collapse(old, new, k, k_style, fade)) or _same(got[:ST], oracle_sb.lerp32_fused(old, new, w)), line
    print(f"{len(lines) - 1} rows, worst error of a mixed value {worst:.3f} of the bound")
    want = {"one_term_mean", "two_terms_mean", "eight_terms_mean", "eight_terms_noise", "one_term_noise", "two_terms_noise_cold",
            "temperature0_with_noise_block", "slot_twice", "weights_cancel", "weights_cancel_noise", "weights_zero", "reset_mean", "reset_noise",
            "frame_zero", "vae_row", "plain_vector"}
    assert want <= names, want - names


def test_oracle_properties():
    """what the oracle must do by the text alone: the weight is style_weight; one term of weight 1 without noise is the slot's
    mean; weights that cancel leave exactly 0; the temperature divides the deviation; the order of the terms is the order given;
    the float32 lerp is torch.lerp on both branches"""
    for f, k, fade in ((3, 7, 0), (6, 7, 0), (7, 7, 0), (9, 7, 12), (19, 7, 12), (40, 7, 12), (-1, 0, 0)):
        assert oracle_sb.weight(f, k, fade) == live.style_weight(f, k, fade)
    rng = np.random.default_rng(3)
    bank = rng.standard_normal((3, 2, 7)).astype(np.float32)
    bank[:, 1] = np.abs(bank[:, 1])
    eps = rng.standard_normal((8, 7)).astype(np.float32)
    got, mag = oracle_sb.mix(bank, [(2, 1.0)])
    assert np.array_equal(got, bank[2, 0].astype(np.float64)) and np.array_equal(mag, np.abs(got))
    assert np.array_equal(oracle_sb.mix(bank, [(1, 0.75), (1, -0.75)], 1.0, eps)[0] * 0, np.zeros(7))
    assert np.array_equal(oracle_sb.mix(bank, [(1, 0.75), (1, -0.75)])[0], np.zeros(7))
    a, _ = oracle_sb.mix(bank, [(0, 1.0)], 2.0, eps)
    assert np.allclose(a, bank[0, 0].astype(np.float64) + bank[0, 1].astype(np.float64) * eps[0] / 2.0, rtol=1e-15, atol=0)
    assert np.array_equal(oracle_sb.mix(bank, [(0, 1.0)], 0.0, eps)[0], bank[0, 0].astype(np.float64))
    x, y = rng.standard_normal(64).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    for w in (0.0, 0.2, 0.49999, 0.5, 0.75, 1.0):               # (torch on the host contracts the multiply-add where the CPU has one)
        got = torch.lerp(torch.as_tensor(x), torch.as_tensor(y), float(np.float32(w))).numpy()
        assert ((got == oracle_sb.lerp32(x, y, w)) | (got == oracle_sb.lerp32_fused(x, y, w))).all(), w
    assert _same(oracle_sb.lerp32(x, y, 0.0), x) and _same(oracle_sb.lerp32(x, y, 1.0), y)
    assert float(oracle_sb.ulp32(1.0)) == 2.0 ** -23 and float(oracle_sb.ulp32(0.0)) == 2.0 ** -149


# ----------------------------------------------------------------------------- 2. the tenth header against capi.SB_*
# (the rules tests/test_live_gaze_cpu.py applies to the ninth header)
_SCALARS = {"int": "int", "long": "long", "size_t": "size_t", "uint64_t": "uint64", "float": "float", "double": "double"}
_ELEMENTS = {"float": "f32*", "double": "f64*", "int": "i32*", "unsigned": "i32*", "int64_t": "i64*", "long": "i64*",
             "long long": "i64*", "uint8_t": "u8*", "unsigned char": "u8*", "char": "u8*", "void": "any*"}
_C_WORDS = {"int", "long", "unsigned", "char", "float", "double", "void", "size_t", "uint64_t", "int64_t", "uint8_t"}
_CTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
           "double": ctypes.c_double}
_OTHERS = ("", "EXT_", "LOUD_", "RS_", "FR_", "RT_", "RF_", "SNAP_", "GZ_")


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


def test_style_prototypes_are_the_tenth_header():
    """capi.SB_PROTOTYPES against include/zeggs_hip_styles.h: the same names, disjoint from the other nine groups; per function the
    return kind, the parameter count, every parameter's kind and every device pointer's element type; the library exports them
    all; zeggs_version() is still 109, the gaze and snapshot versions still 1, zeggs_live_styles_version() is 1"""
    header = _header_prototypes()
    assert set(header) == set(capi.SB_PROTOTYPES) and len(header) == 5
    others = {n for g in _OTHERS for n in getattr(capi, g + "PROTOTYPES")}
    assert not set(capi.SB_PROTOTYPES) & others
    assert not set(capi.SB_STRUCTS) & {n for g in _OTHERS for n in getattr(capi, g + "STRUCTS")}
    assert {b for _, _, ps in header.values() for b, depth in ps if depth == 0} <= set(_SCALARS)       # no struct by value
    structs = {n: c for g in (*_OTHERS, "SB_") for n, c in getattr(capi, g + "STRUCTS").items()}
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
    assert '#include "zeggs_hip_gaze.h"' in text and "zeggs_version() >= 109" in text
    L, api = ops.lib(), capi.api()
    assert L.zeggs_version() == 109 and L.zeggs_live_snapshot_version() == 1 and L.zeggs_live_gaze_version() == 1
    assert L.zeggs_live_styles_version() == 1
    for n in header:
        assert hasattr(L, n), f"libzeggs_hip.so does not export {n}"
        assert getattr(api, n).argtypes is not None and getattr(L, n).argtypes is None


def test_style_struct_mirrors_are_the_tenth_header():
    structs = _header_structs()
    assert set(structs) == set(capi.SB_STRUCTS) == {"ZeggsStyleBankDims", "ZeggsStyleMix"}
    for name, fields in structs.items():
        mirror = capi.SB_STRUCTS[name]._fields_
        assert [f for f, _ in mirror] == [f for f, _, _, _ in fields], name
        for (f, ctype), (_, base, depth, n) in zip(mirror, fields):
            want = ctypes.c_void_p if depth else _CTYPES[base]
            assert ctype is (want * n if n else want) or (n and ctype._type_ is want and ctype._length_ == n), (name, f)
    assert (ctypes.sizeof(capi.StyleBankDims), ctypes.sizeof(capi.StyleMix)) == (12, 112)
    text = _header_text()
    assert int(re.search(r"#define ZEGGS_STYLE_MAX_TERMS (\d+)", text).group(1)) == ops.STYLE_MAX_TERMS == oracle_sb.MAX_TERMS == 8
    assert int(re.search(r"#define ZEGGS_STYLE_MAX_SLOTS (\d+)", text).group(1)) == ops.STYLE_MAX_SLOTS == 4096
    assert capi.StyleMix.weight.size == 4 * 8 and capi.StyleMix.slot.size == 4 * 8


# ----------------------------------------------------------------------------- 3. refusals of the library
def _dims(rows=4, st=64, capacity=6):
    return capi.StyleBankDims(rows, st, capacity)


def _mixes(*rows):
    arr = (capi.StyleMix * len(rows))()
    for q, w in zip(arr, rows):
        w = dict(dict(k=5, k_style=0, fade_style=0, weight=(1.0,), slot=(0,), temperature=0.0, row=0, terms=None, eps_row=-1, reset=0), **w)
        n = len(w["slot"])
        q.slot[:] = list(w["slot"]) + [0] * (8 - n)
        q.weight[:] = list(w["weight"]) + [0.0] * (8 - len(w["weight"]))
        q.k, q.k_style, q.fade_style, q.temperature = w["k"], w["k_style"], w["fade_style"], w["temperature"]
        q.row, q.terms, q.eps_row, q.reset = w["row"], n if w["terms"] is None else w["terms"], w["eps_row"], w["reset"]
    return arr


BANK, BANK_BYTES = ctypes.c_void_p(0x900000), 6 * 2 * 64 * 4


def test_bank_size():
    api = capi.api()
    assert api.zeggs_live_style_bank_bytes(_dims()) == BANK_BYTES and api.zeggs_live_style_bank_bytes(_dims(64, 1, 4096)) == 4096 * 2 * 4
    for bad in (_dims(0), _dims(65), _dims(4, 0), _dims(4, 64, 0), _dims(4, 64, 4097)):
        assert api.zeggs_live_style_bank_bytes(bad) == 0
    assert "a bank of 4097 slots" in api.zeggs_last_error().decode()


@pytest.mark.parametrize("what,rows,dev,eps,match", [
    ("a row out of range", [dict(row=4)], None, None, "record 0: row 4 of 4"),
    ("a negative row", [dict(row=0), dict(row=-1)], 0x7000, None, "record 1: row -1 of 4"),
    ("a row twice", [dict(row=2), dict(row=1), dict(row=2)], 0x7000, None, "record 2: row 2 twice"),
    ("no term", [dict(terms=0)], None, None, r"record 0: 0 terms \(1..8\)"),
    ("nine terms", [dict(row=1), dict(row=0, terms=9)], 0x7000, None, r"record 1: 9 terms \(1..8\)"),
    ("a slot out of range", [dict(slot=(0, 6), weight=(1.0, 1.0))], None, None, "record 0: term 1: slot 6 of 6"),
    ("a negative slot", [dict(slot=(-1,))], None, None, "record 0: term 0: slot -1 of 6"),
    ("a NaN weight", [dict(slot=(0, 1, 2), weight=(1.0, 1.0, float("nan")))], None, None, "record 0: term 2: the weight is not finite"),
    ("an infinite weight", [dict(weight=(float("inf"),))], None, None, "record 0: term 0: the weight is not finite"),
    ("a negative k", [dict(k=-1)], None, None, "record 0: negative frame -1"),
    ("a negative style frame", [dict(k_style=-3)], None, None, "record 0: negative style frame -3"),
    ("a negative style fade", [dict(fade_style=-2)], None, None, "record 0: negative style fade -2"),
    ("a negative temperature", [dict(temperature=-0.5)], None, None, "record 0: temperature -0.5"),
    ("a NaN temperature", [dict(temperature=float("nan"))], None, None, "record 0: temperature nan"),
    ("an infinite temperature", [dict(temperature=float("inf"))], None, None, "record 0: temperature inf"),
    ("a noise slice out of range", [dict(eps_row=4, temperature=1.0)], None, 0x50000, "record 0: noise slice 4 of 4"),
    ("a noise slice below -1", [dict(eps_row=-2)], None, 0x50000, "record 0: noise slice -2 of 4"),
    ("noise without a noise tensor", [dict(row=1), dict(row=0, eps_row=2, temperature=1.0)], 0x7000, None, "record 1: noise asked for with a NULL noise tensor"),
    ("two records without a device copy", [dict(row=0), dict(row=1)], None, None, "must also be in device memory"),
    ("more records than rows", [dict(row=i % 4) for i in range(5)], 0x7000, None, "5 records for 4 rows"),
])
def test_style_mix_refuses_on_the_host(what, rows, dev, eps, match):
    """every refusal comes before the launch (the addresses are never followed, there is no device here), with the record named"""
    d, arr = _dims(), _mixes(*rows)
    dev_p = ctypes.cast(ctypes.c_void_p(dev), ctypes.POINTER(capi.StyleMix)) if dev else None
    with pytest.raises(RuntimeError, match="zeggs_live_style_mix: live style mix: .*" + match):
        capi.api().zeggs_live_style_mix(d, arr, dev_p, len(rows), BANK, BANK_BYTES, eps, 4, 0x10000, 0x20000, None)
    assert ops.lib().zeggs_live_style_mix(ctypes.byref(d), arr, ctypes.c_void_p(dev or 0), len(rows), BANK, ctypes.c_size_t(BANK_BYTES),
                                          ctypes.c_void_p(eps or 0), 4, ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), None) == -1


def test_style_entry_points_check_bank_slot_and_tensors():
    api, d = capi.api(), _dims()
    with pytest.raises(RuntimeError, match="bank too small"):
        api.zeggs_live_style_mix(d, _mixes({}), None, 1, BANK, BANK_BYTES - 1, None, 0, 0x10000, 0x20000, None)
    with pytest.raises(RuntimeError, match="NULL bank"):
        api.zeggs_live_style_put(d, None, BANK_BYTES, 0, 0x10000, 64, None)
    with pytest.raises(RuntimeError, match="misaligned bank"):
        api.zeggs_live_style_put(d, ctypes.c_void_p(0x900002), BANK_BYTES, 0, 0x10000, 64, None)
    for slot in (-1, 6):
        with pytest.raises(RuntimeError, match=f"put: slot {slot} of 6"):
            api.zeggs_live_style_put(d, BANK, BANK_BYTES, slot, 0x10000, 64, None)
    for E in (0, 63, 65, 127, 192):
        with pytest.raises(RuntimeError, match=f"put: a row of {E} floats"):
            api.zeggs_live_style_put(d, BANK, BANK_BYTES, 0, 0x10000, E, None)
    with pytest.raises(RuntimeError, match="put: NULL or misaligned row"):
        api.zeggs_live_style_put(d, BANK, BANK_BYTES, 0, None, 128, None)
    with pytest.raises(RuntimeError, match="mix: NULL style tensor"):
        api.zeggs_live_style_mix(d, _mixes({}), None, 1, BANK, BANK_BYTES, None, 0, None, 0x20000, None)
    with pytest.raises(RuntimeError, match="mix: NULL style tensor"):
        api.zeggs_live_style_mix(d, _mixes({}), None, 1, BANK, BANK_BYTES, None, 0, 0x10000, 0x10000, None)
    with pytest.raises(RuntimeError, match="mix: misaligned tensor"):
        api.zeggs_live_style_mix(d, _mixes({}), None, 1, BANK, BANK_BYTES, None, 0, 0x10000, 0x20002, None)
    out = (ctypes.c_float * 128)()
    with pytest.raises(RuntimeError, match="read: slot 6 of 6"):
        api.zeggs_live_style_read(d, BANK, BANK_BYTES, 6, None, None, -1, ctypes.addressof(out), None)
    with pytest.raises(RuntimeError, match="read: row 4 of 4"):
        api.zeggs_live_style_read(d, BANK, BANK_BYTES, -1, 0x10000, 0x20000, 4, ctypes.addressof(out), None)
    with pytest.raises(RuntimeError, match="read: row 1 of 4 .slot 2"):
        api.zeggs_live_style_read(d, BANK, BANK_BYTES, 2, 0x10000, 0x20000, 1, ctypes.addressof(out), None)
    with pytest.raises(RuntimeError, match="read: NULL output"):
        api.zeggs_live_style_read(d, BANK, BANK_BYTES, 0, None, None, -1, None, None)
    with pytest.raises(RuntimeError, match="live styles: 65 rows"):
        api.zeggs_live_style_put(_dims(65), BANK, 1 << 20, 0, 0x10000, 64, None)
    # nothing to do: no launch, no error
    assert api.zeggs_live_style_mix(d, None, None, 0, BANK, BANK_BYTES, None, 0, None, None, None) == 0


# ----------------------------------------------------------------------------- 4. the Python side
@pytest.mark.parametrize("bad,match", [("on", "None, True or a dict"), (dict(slots=4), "keys"), (dict(capacity=0), "capacity 0"),
                                       (dict(capacity=4097), "capacity 4097"), (dict(capacity=2.5), "capacity 2.5"), (dict(terms=9), "terms 9"),
                                       (dict(terms=0), "terms 0"), (1.0, "None, True or a dict")])
def test_styles_options_are_checked_at_construction(bad, match):
    with pytest.raises(ValueError, match=match):
        live.LiveServer(None, None, {}, CONF, 1 / 60.0, styles=bad)


def test_styles_options_defaults():
    assert live.styles_options(None) is None and live.styles_options(False) is None
    assert live.styles_options(True) == dict(net=None, capacity=64, terms=8)
    net = object()
    assert live.styles_options(dict(net=net, capacity=np.int64(5), terms=2)) == dict(net=net, capacity=5, terms=2)


NAMES = {"calm": 0, "angry": 3, "style": 4}


def test_named_styles_are_parsed():
    assert live.style_terms("calm", NAMES) == [(0, 1.0)]
    assert live.style_terms({"calm": 0.25, "angry": 2}, NAMES) == [(0, 0.25), (3, 2.0)]
    assert live.style_terms([("angry", 0.5), ("calm", -0.5), ("angry", np.float32(0.5))], NAMES) == [(3, 0.5), (0, -0.5), (3, 0.5)]
    assert live.style_terms((("calm", 0),), NAMES) == [(0, 0.0)]
    got = live.style_request("angry", NAMES)
    assert got == dict(terms=[(3, 1.0)], fade=0, temperature=0.0, seed=None)
    got = live.style_request(dict(style={"calm": 1, "angry": 1}, fade=np.int64(12), temperature=0.5, seed=7), NAMES)
    assert got == dict(terms=[(0, 1.0), (3, 1.0)], fade=12, temperature=0.5, seed=7)
    assert live.style_request({"style": 0.5}, NAMES)["terms"] == [(4, 0.5)]               # a mix of the style NAMED "style"
    assert live.style_request(dict(style="calm", temperature=None), NAMES)["temperature"] == 0.0


@pytest.mark.parametrize("req,error,match", [
    ("sad", ValueError, "no style 'sad' in the bank"), ({"calm": 1.0, "sad": 1.0}, ValueError, "no style 'sad'"),
    ([("calm", 1.0), (3, 1.0)], ValueError, "no style 3"), ({}, ValueError, r"0 terms \(1..2"), ({"calm": 1, "angry": 1, "style": 1}, ValueError, r"3 terms \(1..2"),
    ({"calm": float("nan")}, ValueError, "the weight of 'calm'"), ({"calm": "much"}, ValueError, "the weight of 'calm'"),
    ({"calm": float("inf")}, ValueError, "the weight of 'calm'"), ({"calm": 1e39}, ValueError, "the weight of 'calm'"), ({"calm": True}, ValueError, "the weight of 'calm'"),
    (["calm", "angry"], TypeError, "a list of .name, weight. pairs"), (3.5, TypeError, "a style is a tensor, a name"),
    (dict(style="calm", fade=-1), ValueError, "fade -1"), (dict(style="calm", fade=1.5), ValueError, "fade 1.5"),
    (dict(style="calm", temperature=-1.0), ValueError, "temperature -1.0"), (dict(style="calm", temperature=float("nan")), ValueError, "temperature nan"),
    (dict(style="calm", temperature="hot"), ValueError, "temperature 'hot'"), (dict(style="calm", seed=3), ValueError, "seed 3"),
    (dict(style="calm", temperature=1.0, seed=1.5), ValueError, "seed 1.5"), (dict(style="calm", speed=2), ValueError, "a style or a dict"),
    (dict(style=torch.zeros(4)), TypeError, "named styles only"),
])
def test_style_requests_are_checked_on_the_host(req, error, match):
    with pytest.raises(error, match=match):
        live.style_request(req, NAMES, 2)


class _Plain:
    """what the calls look at of a server before they refuse"""
    _sb = None
    _sids = {}
    _styles_on = live.LiveServer._styles_on


@pytest.mark.parametrize("call", [
    lambda s: live.LiveServer.add_style(s, "calm", np.zeros(4, np.float32)), lambda s: live.LiveServer.remove_style(s, "calm"),
    lambda s: live.LiveServer.styles(s), lambda s: live.LiveServer.set_style(s, 0, "calm"), lambda s: live.LiveServer.set_style(s, 0, {"calm": 1.0}, fade=3),
    lambda s: live.LiveServer.set_style_many(s, {0: "calm"}), lambda s: live.LiveServer.style(s, 0)],
    ids=["add_style", "remove_style", "styles", "set_style-name", "set_style-dict", "set_style_many", "style"])
def test_a_server_without_the_bank_names_the_option(call):
    with pytest.raises(ValueError, match=r"named styles are off \(LiveServer\(styles=True\)\)"):
        call(_Plain())


class _Bank:
    """a server's bank bookkeeping without a device: the checks of add_style / remove_style come before anything is enqueued"""
    _styles_on = live.LiveServer._styles_on
    add_style, remove_style, styles = live.LiveServer.add_style, live.LiveServer.remove_style, live.LiveServer.styles

    def __init__(self, capacity=2, net=None):
        self._sb, self.styles_conf, self._style_names = object(), dict(net=net, capacity=capacity, terms=8), {}
        self.sty_old, self.dev = torch.zeros(3, 4), "cpu"


def test_add_style_checks_before_anything_is_enqueued(monkeypatch):
    put = []
    monkeypatch.setattr(ops, "live_style_put", lambda sb, slot, enc: put.append((slot, enc.clone())))
    s = _Bank()
    with pytest.raises(ValueError, match=r"an example needs the style encoder \(LiveServer\(styles=dict\(net=style_net\)\)\)"):
        s.add_style("calm", "calm.bvh")
    with pytest.raises(ValueError, match="an example needs the style encoder"):
        s.add_style("calm", np.zeros((30, 9), np.float32))
    with pytest.raises(ValueError, match="a vector of 5 floats, the model's styles have 4"):
        s.add_style("calm", np.zeros(5, np.float32))
    with pytest.raises(ValueError, match="a name is a string"):
        s.add_style(3, np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="trim"):
        s.add_style("calm", np.zeros(4, np.float32), trim=(0, 3))
    assert put == [] and s.styles() == {}
    assert s.add_style("calm", np.arange(4, dtype=np.float64)) == 0 and s.add_style("angry", torch.ones(4)) == 1
    assert s.styles() == dict(calm=0, angry=1) and [p[0] for p in put] == [0, 1] and put[0][1].dtype == torch.float32
    with pytest.raises(RuntimeError, match=r"the bank is full, all 2 slots are in use \(LiveServer\(styles=dict\(capacity=\.\.\.\)\)"):
        s.add_style("sad", np.zeros(4, np.float32))
    assert s.add_style("calm", np.ones(4, np.float32)) == 0 and len(put) == 3           # an existing name keeps its slot
    with pytest.raises(ValueError, match="no style 'sad' in the bank"):
        s.remove_style("sad")
    s.remove_style("calm")
    assert s.styles() == dict(angry=1) and s.add_style("sad", np.zeros(4, np.float32)) == 0    # the freed slot is the next one taken
    got = s.styles()
    got["x"] = 9
    assert s.styles() == dict(angry=1, sad=0)                                         # a copy


def test_a_tensor_style_takes_no_sampling_arguments():
    with pytest.raises(ValueError, match="temperature / seed sample a named style"):
        live.LiveServer.set_style(_Plain(), 0, torch.zeros(4), temperature=1.0)
    with pytest.raises(ValueError, match="temperature / seed sample a named style"):
        live.LiveServer.set_style(_Plain(), 0, torch.zeros(4), seed=3)
