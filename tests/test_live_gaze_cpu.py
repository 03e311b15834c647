"""Host-only parts of LiveServer's moving gaze: the shared schedule header on the host (tests/host/gaze_math_check.cpp, plain and
under sanitizers) against the float64 oracle (tests/live_gaze_oracle.py), include/zeggs_hip_gaze.h against zeggs/capi.py, every
refusal that comes before a launch, and gaze_to_model().  No GPU needed -- the library loads on the CPU for host-only calls."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import live_gaze_oracle as oracle_gz
from zeggs import capi, live, ops

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "zeggs_hip_gaze.h"
CONF = dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True, normalize_mel_bins=True,
            normalize_range=True, min_clipping=1e-5, sampling_rate=16000, mel_fmin=20, mel_fmax=7600, n_mel_channels=80,
            filter_length=800, hop_length=200, resample_method="linear", normalize_loudness=False)
PATHS, EASES, SPACES = ("line", "arc"), ("linear", "smooth"), ("world", "root")


# ----------------------------------------------------------------------------- 1. csrc/gaze_math.h on the host, against the oracle
def _cxx():
    return shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")


def _schedule(v):
    """13 numbers of a row -> the oracle's schedule"""
    f = np.array(v[:9], np.float32)
    return dict(start=f[0:3], end=f[3:6], pivot=f[6:9], path=PATHS[int(v[9])], ease=EASES[int(v[10])], k=int(v[11]), fade=int(v[12]))


def _close(got, want):
    """the bound of the issue, per component: |got - float32(oracle)| <= 2^-23 max(1, |oracle|)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want.astype(np.float32).astype(np.float64))
    return bool((err <= oracle_gz.bound(want)).all()), float((err / oracle_gz.bound(want)).max())


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_schedule_arithmetic_on_the_host_equals_the_oracle(tmp_path, flags):
    """tests/host/gaze_math_check.cpp: a stand-alone program over the header the kernels use (its head says what it walks); once
    plain, once under the address and undefined-behaviour sanitizers (host code with its own main, run directly).  Every row
    of its table is recomputed by the oracle from the row's own inputs; the names say that every case was walked."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "gaze_math_check"
    b = subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "gaze_math_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "gaze_math_check: ok"
    names, worst = set(), 0.0
    for line in lines[:-1]:
        kind, name, *rest = line.split()
        bar = rest.index("|")
        v, got = [float(x) for x in rest[:bar]], [float(x) for x in rest[bar + 1:]]
        names.add(name)
        if kind == "point":
            assert len(v) == 14 and len(got) == 3, line
            ok, e = _close(got, oracle_gz.point(_schedule(v), int(v[13])))
        elif kind == "resolve":
            assert len(v) == 10 and len(got) == 3, line
            ok, e = _close(got, oracle_gz.resolve(v[0:3], v[3:7], v[7:10]))
        else:
            assert kind == "apply" and len(v) == 13 + 6 + 13 and len(got) == 9, line
            k, fade, space, path, ease, has_pivot = (int(x) for x in v[13:19])
            s = oracle_gz.apply(_schedule(v), k, v[19:22], fade=fade, space=SPACES[space], path=PATHS[path], ease=EASES[ease],
                                pivot=v[22:25] if has_pivot else None, rpos=v[25:28], rrot=v[28:32])
            ok, e = _close(got, np.concatenate([s["start"], s["end"], s["pivot"]]))
        worst = max(worst, e)
        assert ok, (line, e)
    print(f"{len(lines) - 1} rows, worst error {worst:.3f} of the bound")
    want = {f"line_fade{f}_ease{e}" for f in (0, 1, 12) for e in (0, 1)} | {f"arc_{d}deg_len{n}_ease{e}" for d in (1, 90, 179) for n in (0, 1) for e in (0, 1)}
    want |= {"fallback_same_direction", "fallback_opposite_direction", "fallback_target_on_pivot", "fallback_start_on_pivot", "not_unit_length",
             "negative_w_not_unit", "second_in_the_fade_root_arc", "third_in_the_fade_root_pivot", "after_second", "after_third"}
    assert want <= names, want - names


def test_oracle_properties():
    """what the oracle must do by the text alone: the weight is style_weight, both paths begin at P(0) and end at P(1), the arc
    keeps the distance from the pivot on a line and turns by the angle's share, each fallback is the line, and a track through
    an unfinished fade is continuous"""
    for f, k, fade in ((3, 7, 0), (6, 7, 0), (7, 7, 0), (9, 7, 12), (19, 7, 12), (40, 7, 12), (7, 7, 1), (8, 7, 1)):
        assert oracle_gz.weight(f, k, fade) == live.style_weight(f, k, fade)
    c = np.array([0.1, 1.5, -0.2])
    a, b = c + 2.0 * np.array([1.0, 0.0, 0.0]), c + 3.0 * np.array([0.0, 0.0, 1.0])
    for w in (0.0, 0.25, 0.5, 1.0):
        p = oracle_gz.path_point(a, b, c, "arc", w)
        assert abs(np.linalg.norm(p - c) - (2.0 + w)) < 1e-12
        assert abs(np.arctan2(p[2] - c[2], p[0] - c[0]) - w * np.pi / 2) < 1e-12
        assert np.allclose(oracle_gz.path_point(a, b, c, "line", w), (1 - w) * a + w * b, atol=0, rtol=0)
    for end in (c + 2.0 * (a - c), c - (a - c), c):
        assert np.array_equal(oracle_gz.path_point(a, end, c, "arc", 0.3), oracle_gz.path_point(a, end, c, "line", 0.3))
    g0 = np.array([1.0, 1.5, 3.0], np.float32)
    tr = oracle_gz.track(40, g0, [dict(k=10, target=[-2.0, 1.0, 2.0], fade=12), dict(k=16, target=[0.0, 2.0, 4.0], fade=5, path="arc", pivot=c)])
    assert np.array_equal(tr[:10], np.tile(g0.astype(np.float64), (10, 1))) and np.allclose(tr[22:], [0.0, 2.0, 4.0])
    assert np.abs(np.diff(tr, axis=0)).max() < 1.0          # no jump where the second set took over


# ----------------------------------------------------------------------------- 2. the ninth header against capi.GZ_*
# (the rules tests/test_live_loudness_cpu.py applies to the third header)
_SCALARS = {"int": "int", "long": "long", "size_t": "size_t", "uint64_t": "uint64", "float": "float", "double": "double"}
_ELEMENTS = {"float": "f32*", "double": "f64*", "int": "i32*", "unsigned": "i32*", "int64_t": "i64*", "long": "i64*",
             "long long": "i64*", "uint8_t": "u8*", "unsigned char": "u8*", "char": "u8*", "void": "any*"}
_C_WORDS = {"int", "long", "unsigned", "char", "float", "double", "void", "size_t", "uint64_t", "int64_t", "uint8_t"}
_CTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
           "double": ctypes.c_double}
_OTHERS = ("", "EXT_", "LOUD_", "RS_", "FR_", "RT_", "RF_", "SNAP_")


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


def test_gaze_prototypes_are_the_ninth_header():
    """capi.GZ_PROTOTYPES against include/zeggs_hip_gaze.h: the same names, disjoint from the other eight groups; per function the
    return kind, the parameter count, every parameter's kind and every device pointer's element type; the library exports them
    all; zeggs_version() is still 109, zeggs_live_snapshot_version() still 1, zeggs_live_gaze_version() is 1"""
    header = _header_prototypes()
    assert set(header) == set(capi.GZ_PROTOTYPES) and len(header) == 7
    others = {n for g in _OTHERS for n in getattr(capi, g + "PROTOTYPES")}
    assert not set(capi.GZ_PROTOTYPES) & others
    assert not set(capi.GZ_STRUCTS) & {n for g in _OTHERS for n in getattr(capi, g + "STRUCTS")}
    assert {b for _, _, ps in header.values() for b, depth in ps if depth == 0} <= set(_SCALARS)       # no struct by value
    structs = {n: c for g in (*_OTHERS, "GZ_") for n, c in getattr(capi, g + "STRUCTS").items()}
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
    assert '#include "zeggs_hip_snapshot.h"' in text and "zeggs_version() >= 109" in text
    L, api = ops.lib(), capi.api()
    assert L.zeggs_version() == 109 and L.zeggs_live_snapshot_version() == 1 and L.zeggs_live_gaze_version() == 1
    for n in header:
        assert hasattr(L, n), f"libzeggs_hip.so does not export {n}"
        assert getattr(api, n).argtypes is not None and getattr(L, n).argtypes is None


def test_gaze_struct_mirrors_are_the_ninth_header():
    structs = _header_structs()
    assert set(structs) == set(capi.GZ_STRUCTS) == {"ZeggsGazeDims", "ZeggsGazeSet", "ZeggsGazeCond"}
    for name, fields in structs.items():
        mirror = capi.GZ_STRUCTS[name]._fields_
        assert [f for f, _ in mirror] == [f for f, _, _, _ in fields], name
        for (f, ctype), (_, base, depth, n) in zip(mirror, fields):
            want = ctypes.c_void_p if depth else _CTYPES[base]
            assert ctype is (want * n if n else want) or (n and ctype._type_ is want and ctype._length_ == n), (name, f)
    assert (ctypes.sizeof(capi.GazeDims), ctypes.sizeof(capi.GazeSet), ctypes.sizeof(capi.GazeCond)) == (8, 64, 40)
    text = _header_text()
    assert int(re.search(r"#define ZEGGS_GAZE_READ_WORDS (\d+)", text).group(1)) == 16
    assert int(re.search(r"#define ZEGGS_GAZE_ROW_BYTES (\d+)", text).group(1)) == 64
    for table, prefix in ((ops.GAZE_SPACES, ""), (ops.GAZE_PATHS, ""), (ops.GAZE_EASES, "")):
        for word, code in table.items():
            assert int(re.search(rf"#define ZEGGS_GAZE_{prefix}{word.upper()} (\d+)", text).group(1)) == code


# ----------------------------------------------------------------------------- 3. refusals
@pytest.mark.parametrize("bad,match", [("on", "None, True or a dict"), (dict(easing="smooth"), "keys"), (dict(ease="cubic"), "ease 'cubic'"),
                                       (1.0, "None, True or a dict")])
def test_gaze_options_are_checked_at_construction(bad, match):
    with pytest.raises(ValueError, match=match):
        live.LiveServer(None, None, {}, CONF, 1 / 60.0, gaze=bad)


def test_gaze_options_defaults():
    assert live.gaze_options(None) is None and live.gaze_options(False) is None
    assert live.gaze_options(True) == dict(ease="linear") and live.gaze_options(dict(ease="smooth")) == dict(ease="smooth")


class _Plain:
    """what the three calls look at of a server before they refuse"""
    _gz = None
    _sids = {}
    _gaze_on = live.LiveServer._gaze_on
    _gaze_read = live.LiveServer._gaze_read


def _gaze_attribute(s):
    """what LiveServer.__init__ makes of its gaze tensor: the rows [R, T, 3], and the call gaze(sid)"""
    import weakref
    g = torch.zeros(2, 5, 3).as_subclass(live._GazeRows)
    g._server = weakref.ref(s)
    return g


@pytest.mark.parametrize("call", [lambda s: live.LiveServer.set_gaze(s, 0, [0, 0, 1]), lambda s: live.LiveServer.set_gaze_many(s, {0: [0, 0, 1]}),
                                  lambda s: _gaze_attribute(s)(0)], ids=["set_gaze", "set_gaze_many", "gaze"])
def test_a_server_without_the_stage_names_the_option(call):
    with pytest.raises(ValueError, match=r"the moving gaze is off \(LiveServer\(gaze=True\)\)"):
        call(_Plain())


def test_the_gaze_attribute_is_still_the_rows_tensor():
    """`gaze` is the call of the issue and the tensor the server has always had under that name: indexing, in-place writes and
    arithmetic see a plain tensor with the same storage"""
    s = _Plain()
    g = _gaze_attribute(s)
    g[1] = torch.tensor([1.0, 2.0, 3.0])
    g[0].fill_(7.0)
    assert g.shape == (2, 5, 3) and g.is_contiguous() and float(g[1, 4, 2]) == 3.0 and float(g.sum()) == 7.0 * 15 + 6.0 * 5
    assert type(g[0]) is torch.Tensor and type(g + 1) is torch.Tensor and g[1:2, :1].expand(1, 4, 3).contiguous().data_ptr() != g.data_ptr()
    assert g[1].data_ptr() == g.data_ptr() + 4 * 15


@pytest.mark.parametrize("req,match", [
    (dict(target=[0, 0, 1], fade=-1), "fade -1"), (dict(target=[0, 0, 1], fade=1.5), "fade 1.5"), (dict(target=[0, 0]), "the target is three finite"),
    (dict(target=[0, float("nan"), 1]), "the target is three finite"), (dict(target=[0, float("inf"), 1]), "the target is three finite"),
    (dict(target=[0, 1e39, 1]), "the target is three finite"), (dict(target="there"), "the target is three finite"),
    (dict(target=[0, 0, 1], pivot=[0, 0, 0, 0]), "the pivot is three finite"), (dict(target=[0, 0, 1], pivot=[0, float("nan"), 0]), "the pivot is three finite"),
    (dict(target=[0, 0, 1], space="local"), "space 'local'"), (dict(target=[0, 0, 1], path="spline"), "path 'spline'"),
    (dict(target=[0, 0, 1], ease="cubic"), "ease 'cubic'"), (dict(target=[0, 0, 1], path="arc"), "needs a pivot"),
    (dict(fade=3), "a target or a dict"), (dict(target=[0, 0, 1], speed=3), "a target or a dict"),
])
def test_set_gaze_requests_are_checked_on_the_host(req, match):
    with pytest.raises(ValueError, match=match):
        live.gaze_request(req)


def test_set_gaze_request_defaults():
    got = live.gaze_request([1, 2, 3], "smooth")
    assert got["target"].tolist() == [1.0, 2.0, 3.0] and got["target"].dtype == np.float64
    assert {k: got[k] for k in ("fade", "space", "path", "pivot", "ease")} == dict(fade=0, space="world", path="line", pivot=None, ease="smooth")
    got = live.gaze_request(dict(target=(0, 1, 2), fade=np.int64(12), space="root", path="arc", ease="linear"), "smooth")
    assert (got["fade"], got["space"], got["path"], got["ease"], got["pivot"]) == (12, "root", "arc", "linear", None)


def _dims(rows=4, ST=64):
    return capi.GazeDims(rows, ST)


def _sets(*rows):
    arr = (capi.GazeSet * len(rows))()
    for q, w in zip(arr, rows):
        w = dict(dict(target=(0.0, 1.5, 2.0), pivot=(0.0, 0.0, 0.0), k=5, fade=0, row=0, space=0, path=0, ease=0, has_pivot=0), **w)
        q.target[:], q.pivot[:] = w["target"], w["pivot"]
        q.k, q.fade, q.row, q.space, q.path, q.ease, q.has_pivot = (w[k] for k in ("k", "fade", "row", "space", "path", "ease", "has_pivot"))
    return arr


def _conds(*rows):
    arr = (capi.GazeCond * len(rows))()
    for q, w in zip(arr, rows):
        w = dict(dict(k0=4, k_style=0, fade_style=0, row=0, out_row=0, n=5), **w)
        q.k0, q.k_style, q.fade_style, q.row, q.out_row, q.n = (w[k] for k in ("k0", "k_style", "fade_style", "row", "out_row", "n"))
    return arr


def test_gaze_state_size_and_spans():
    api = capi.api()
    assert api.zeggs_live_gaze_state_bytes(_dims(4)) == 4 * 64 and api.zeggs_live_gaze_state_bytes(_dims(64, 1)) == 64 * 64
    for bad in (_dims(0), _dims(65), _dims(4, 0)):
        assert api.zeggs_live_gaze_state_bytes(bad) == 0
    lg = type("LG", (), dict(d=_dims(8)))
    assert [ops.live_gaze_spans(lg, r) for r in (0, 3, 7)] == [[(0, 64)], [(192, 64)], [(448, 64)]]
    for row in (-1, 8):
        with pytest.raises(RuntimeError, match=f"live gaze spans: row {row} of 8"):
            ops.live_gaze_spans(lg, row)
    with pytest.raises(RuntimeError, match="room for 0 spans"):
        api.zeggs_live_gaze_spans(_dims(8), 0, (capi.SnapSpan * 1)(), 0)


@pytest.mark.parametrize("what,rows,dev,match", [
    ("a row out of range", [dict(row=4)], None, "record 0: row 4 of 4"),
    ("a negative row", [dict(row=0), dict(row=-1)], 0x7000, "record 1: row -1 of 4"),
    ("a row twice", [dict(row=2), dict(row=1), dict(row=2)], 0x7000, "record 2: row 2 twice"),
    ("frame 0", [dict(k=0)], None, "record 0: frame 0"),
    ("a negative fade", [dict(fade=-1)], None, "record 0: negative fade -1"),
    ("an unknown space", [dict(space=2)], None, "record 0: space 2"),
    ("an unknown path", [dict(row=1), dict(row=0, path=7)], 0x7000, "record 1: path 7"),
    ("an unknown ease", [dict(ease=-1)], None, "record 0: ease -1"),
    ("a NaN in the target", [dict(target=(0.0, float("nan"), 1.0))], None, "record 0: the target is not finite"),
    ("an infinite pivot", [dict(pivot=(float("inf"), 0.0, 0.0), has_pivot=1)], None, "record 0: the pivot is not finite"),
    ("a world-space arc without a pivot", [dict(path=1)], None, "record 0: an arc in world space needs a pivot"),
    ("two records without a device copy", [dict(row=0), dict(row=1)], None, "must also be in device memory"),
    ("more records than rows", [dict(row=i % 4) for i in range(5)], 0x7000, "5 records for 4 rows"),
])
def test_gaze_set_refuses_on_the_host(what, rows, dev, match):
    """every refusal comes before the launch (the addresses are never followed, there is no device here), with the record named"""
    d, arr = _dims(), _sets(*rows)
    dev_p = ctypes.cast(ctypes.c_void_p(dev), ctypes.POINTER(capi.GazeSet)) if dev else None
    with pytest.raises(RuntimeError, match="zeggs_live_gaze_set: live gaze set: .*" + match):
        capi.api().zeggs_live_gaze_set(d, arr, dev_p, len(rows), 0x10000, 3, 0x20000, 4, ctypes.c_void_p(0x900000), 4 * 64, None)
    assert ops.lib().zeggs_live_gaze_set(ctypes.byref(d), arr, ctypes.c_void_p(dev or 0), len(rows), ctypes.c_void_p(0x10000), ctypes.c_long(3),
                                         ctypes.c_void_p(0x20000), ctypes.c_long(4), ctypes.c_void_p(0x900000), ctypes.c_size_t(4 * 64), None) == -1


def test_gaze_set_in_root_space_needs_the_root_state():
    d = _dims()
    for rpos, rrot, ld in ((None, 0x20000, 3), (0x10000, None, 3), (0x10002, 0x20000, 3), (0x10000, 0x20000, 2)):
        with pytest.raises(RuntimeError, match="root space needs the rows' root state|root strides"):
            capi.api().zeggs_live_gaze_set(d, _sets(dict(space=1)), None, 1, rpos, ld, rrot, 4, ctypes.c_void_p(0x900000), 4 * 64, None)


@pytest.mark.parametrize("what,rows,dev,match", [
    ("a row out of range", [dict(row=4)], None, "record 0: row 4 of 4"),
    ("a row twice", [dict(row=1, out_row=0), dict(row=1, out_row=1)], 0x7000, "record 1: row 1 twice"),
    ("an output slice out of range", [dict(out_row=3)], None, "record 0: output slice 3 of 3"),
    ("an output slice twice", [dict(row=0, out_row=2), dict(row=1, out_row=2)], 0x7000, "record 1: output slice 2 twice"),
    ("no frames", [dict(n=0)], None, r"record 0: 0 frames \(1..5\)"),
    ("more frames than the stride", [dict(n=6)], None, r"record 0: 6 frames \(1..5\)"),
    ("a negative frame", [dict(k0=-1)], None, "record 0: negative frame -1"),
    ("a negative style fade", [dict(fade_style=-2)], None, "record 0: negative style fade -2"),
    ("two records without a device copy", [dict(row=0, out_row=0), dict(row=1, out_row=1)], None, "must also be in device memory"),
    ("more records than output slices", [dict(row=i, out_row=i % 3) for i in range(4)], 0x7000, "4 records for 4 rows and 3 output slices"),
])
def test_condition_refuses_on_the_host(what, rows, dev, match):
    d, arr = _dims(), _conds(*rows)
    dev_p = ctypes.cast(ctypes.c_void_p(dev), ctypes.POINTER(capi.GazeCond)) if dev else None
    with pytest.raises(RuntimeError, match="zeggs_live_condition: live condition: .*" + match):
        capi.api().zeggs_live_condition(d, arr, dev_p, len(rows), ctypes.c_void_p(0x900000), 4 * 64, 0x10000, 0x20000, 0x30000, 0x40000, 3, 5, None)


def test_gaze_entry_points_check_state_row_and_tensors():
    api, d, state = capi.api(), _dims(), ctypes.c_void_p(0x900000)
    with pytest.raises(RuntimeError, match="state too small"):
        api.zeggs_live_gaze_set(d, _sets({}), None, 1, 0x10000, 3, 0x20000, 4, state, 4 * 64 - 1, None)
    with pytest.raises(RuntimeError, match="NULL state"):
        api.zeggs_live_gaze_reset(d, None, 4 * 64, 0, 0x10000, None)
    with pytest.raises(RuntimeError, match="misaligned state"):
        api.zeggs_live_gaze_reset(d, ctypes.c_void_p(0x900004), 4 * 64, 0, 0x10000, None)
    with pytest.raises(RuntimeError, match="reset: row 4 of 4"):
        api.zeggs_live_gaze_reset(d, state, 4 * 64, 4, 0x10000, None)
    with pytest.raises(RuntimeError, match="reset: NULL or misaligned gaze"):
        api.zeggs_live_gaze_reset(d, state, 4 * 64, 0, None, None)
    with pytest.raises(RuntimeError, match="read: row 9 of 4"):
        api.zeggs_live_gaze_read(d, state, 4 * 64, 9, 1, ctypes.addressof((ctypes.c_double * 16)()), None)
    with pytest.raises(RuntimeError, match="read: NULL output"):
        api.zeggs_live_gaze_read(d, state, 4 * 64, 0, 1, None, None)
    with pytest.raises(RuntimeError, match="live gaze: 65 rows"):
        api.zeggs_live_gaze_reset(_dims(65), state, 65 * 64, 0, 0x10000, None)
    with pytest.raises(RuntimeError, match="live condition: NULL tensor"):
        api.zeggs_live_condition(d, _conds({}), None, 1, state, 4 * 64, 0x10000, 0x20000, None, 0x40000, 3, 5, None)
    with pytest.raises(RuntimeError, match="live condition: misaligned tensor"):
        api.zeggs_live_condition(d, _conds({}), None, 1, state, 4 * 64, 0x10000, 0x20002, 0x30000, 0x40000, 3, 5, None)
    with pytest.raises(RuntimeError, match="a stride of 0 frames"):
        api.zeggs_live_condition(d, _conds({}), None, 1, state, 4 * 64, 0x10000, 0x20000, 0x30000, 0x40000, 3, 0, None)
    # nothing to do: no launch, no error
    assert api.zeggs_live_gaze_set(d, None, None, 0, None, 0, None, 0, state, 4 * 64, None) == 0
    assert api.zeggs_live_condition(d, None, None, 0, state, 4 * 64, None, None, None, None, 3, 5, None) == 0


# ----------------------------------------------------------------------------- 4. gaze_to_model
def _rotate(q, v):
    t = 2.0 * np.cross(q[1:], v)
    return v + q[0] * t + np.cross(q[1:], t)


def _unit(rng):
    q = rng.standard_normal(4)
    return q / np.linalg.norm(q)


def test_gaze_to_model_inverts_the_documented_rebasing():
    """x' = start_rot ref_rot^-1 (x - ref_pos) + start_pos (open()'s docstring), on seeded placements: gaze_to_model(x') is x to
    1e-12 in float64; the identity placement changes nothing"""
    rng = np.random.default_rng(11)
    inv = lambda q: q * np.array([1.0, -1.0, -1.0, -1.0])  # noqa: E731
    for _ in range(20):
        x, ref_pos, start_pos = (rng.standard_normal(3) * 3.0 for _ in range(3))
        ref_rot, start_rot = _unit(rng), _unit(rng)
        placed = _rotate(start_rot, _rotate(inv(ref_rot), x - ref_pos)) + start_pos
        back = live.gaze_to_model(placed, ref_pos, ref_rot, start_pos, start_rot)
        assert back.dtype == np.float64 and np.abs(back - x).max() <= 1e-12
    x, ref_pos, ref_rot = rng.standard_normal(3), rng.standard_normal(3), _unit(rng)
    assert np.abs(live.gaze_to_model(x, ref_pos, ref_rot, ref_pos, ref_rot) - x).max() <= 1e-12
    assert np.array_equal(live.gaze_to_model(x, np.zeros(3), [1.0, 0.0, 0.0, 0.0], np.zeros(3), [1.0, 0.0, 0.0, 0.0]), x)
    # float32 inputs are taken up to float64 first: no float32 arithmetic inside
    got = live.gaze_to_model(np.float32([1, 2, 3]), np.float32([0.1, 0.2, 0.3]), np.float32(ref_rot), [0, 0, 1], start_rot)
    want = _rotate(np.float32(ref_rot).astype(np.float64), _rotate(inv(start_rot), np.float64([1, 2, 2]))) + np.float32([0.1, 0.2, 0.3]).astype(np.float64)
    assert np.abs(got - want).max() <= 1e-15 * 10
