"""Host-only parts of LiveServer.push_many (zeggs/live.py: plan_push; include/zeggs_hip_live.h against zeggs/capi.py; the refusals
zeggs_copy_segments makes before it launches anything): no GPU needed -- the library loads on the CPU for host-only calls."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from zeggs import audio, capi, live, ops

ROOT = Path(__file__).resolve().parent.parent
FS, FPS, TICK, WIDTH = 16000, 60.0, 4, 3
MEL = audio.MelDims(800, 200, 80, FS, FPS, 1e-5, 0.0, 0)


def _first_sample(k):
    return ops.mel_window_first_sample(MEL, k)


def _ready(n):
    return min(ops.mel_frames_ready(MEL, n), audio.n_anim_frames(n, FS, FPS) - 1)


# ----------------------------------------------------------------------------- plan_push against push()'s own rule
class _RefRow:
    """one row as LiveServer.push() / _features() keep it, on NumPy: the window holds sample indices, a feature row its frame number"""

    def __init__(self, cap, shared):
        self.w, self.n, self.base = np.full(cap, -1, np.int64), 0, 0
        self.n_feat, self.fbase, self.n_ring, self.kd = 0, 0, 0, 1
        self.shared = shared                      # {"FC": .}: the block size is the server's, not the row's
        self.feats = np.full(shared["FC"], -1, np.int64)
        self.events = set()

    def push(self, m):
        if m == 0:
            return
        w = self.w
        if self.n - self.base + m > w.size:
            nb = max(self.base, min(_first_sample(self.n_feat), self.n))
            keep = w[nb - self.base:self.n - self.base].copy()
            self.events.add("window compacted")
            if keep.size + m > w.size:
                w = self.w = np.full(keep.size + m, -1, np.int64)
                self.events.add("window grown")
            w[:keep.size] = keep
            self.base = nb
        w[self.n - self.base:self.n - self.base + m] = np.arange(self.n, self.n + m)
        self.n += m
        k0, k1, FC = self.n_feat, _ready(self.n), self.shared["FC"]
        if k1 <= k0:
            return
        if self.feats.size < FC:                 # (another row grew the block)
            self.feats = np.concatenate([self.feats, np.full(FC - self.feats.size, -1, np.int64)])
        pend = k0 - self.n_ring
        if k0 - self.fbase + (k1 - k0) > FC:
            keep = self.feats[self.n_ring - self.fbase:k0 - self.fbase].copy()
            self.events.add("features compacted")
            if pend + (k1 - k0) > FC:
                FC = self.shared["FC"] = pend + (k1 - k0)
                self.feats = np.concatenate([self.feats, np.full(FC - self.feats.size, -1, np.int64)])
                self.events.add("feature block grown")
            self.feats[:pend] = keep
            self.fbase = self.n_ring
        self.feats[k0 - self.fbase:k1 - self.fbase] = np.arange(k0, k1)
        self.n_feat = k1

    def drain(self):
        while True:
            p = live.plan_step([dict(n_feat=self.n_feat, n_ring=self.n_ring, kd=self.kd)], TICK, live.ring_depth(31, TICK))[0]
            if p is None:
                return
            self.n_ring += p["n_new"]
            self.kd = p["k1"]


def _spans(copies, bufs):
    """(source span, destination span) of every copy as (buffer identity, first float, one past the last)"""
    return [((id(bufs[s]), so, so + c), (id(bufs[d]), do, do + c)) for s, so, d, do, c in copies]


def _disjoint(a, b):
    return a[0] != b[0] or a[2] <= b[1] or b[2] <= a[1]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_plan_push_is_push_row_by_row(seed):
    """3 rows, 40 calls with chunks of 0..3000 samples into windows of 4096 and feature blocks of 24 rows, steps in between as
    step() would take them (now and then none, so features pile up): after every call the copies of the plan, executed on NumPy,
    leave what push() per row leaves -- the window holds samples base .. n - 1, the pending feature rows are where the encoder
    looks for them, the four counters and the block size agree -- and no copy overlaps another's destination or its own source"""
    rng = np.random.default_rng(seed)
    R, CAP, FC0 = 3, 4096, 24
    shared = {"FC": FC0}
    ref = [_RefRow(CAP, shared) for _ in range(R)]
    win = [np.full(CAP, -1, np.int64) for _ in range(R)]
    alt = [np.full(CAP, -1, np.int64) for _ in range(R)]
    FC = FC0
    feats = [np.full(FC * WIDTH, -1, np.int64) for _ in range(R)]
    n_ops = set()
    for call in range(40):
        lens = [int(rng.choice([0, int(rng.integers(1, 3001))], p=[0.15, 0.85])) for _ in range(R)]
        state = [dict(n=x.n, base=x.base, n_feat=x.n_feat, fbase=x.fbase, n_ring=x.n_ring) for x in ref]
        plan = live.plan_push(state, [w.size for w in win], lens, FC, WIDTH, _first_sample, _ready)
        for x, m in zip(ref, lens):
            x.push(m)
        # ---- what the server does with a plan: growth, the two launches, the mel rows, the swaps
        if plan["FC"] > FC:
            FC = plan["FC"]
            feats = [np.concatenate([f, np.full(FC * WIDTH - f.size, -1, np.int64)]) for f in feats]
        for i, p in enumerate(plan["rows"]):
            if p["swap"] and alt[i].size < p["cap"]:
                alt[i] = np.full(p["cap"], -1, np.int64)
        pos, stage = 0, np.full(plan["n_stage"], -1, np.int64)
        for i, m in enumerate(lens):
            stage[pos:pos + m] = np.arange(state[i]["n"], state[i]["n"] + m)
            pos += m
        assert pos == plan["n_stage"]
        bufs = {("stage", None): stage}
        scratch = [np.full(FC * WIDTH, -1, np.int64) for _ in range(R)]
        for i in range(R):
            bufs.update({("win", i): win[i], ("alt", i): alt[i], ("feats", i): feats[i], ("scratch", i): scratch[i]})
        for copies in (plan["segs"], plan["segs_back"]):
            assert len(copies) <= 3 * R
            spans = _spans(copies, bufs)
            for a, (src_a, dst_a) in enumerate(spans):
                assert dst_a[1] >= 0 and dst_a[2] <= bufs[copies[a][2]].size and src_a[1] >= 0 and src_a[2] <= bufs[copies[a][0]].size
                for b, (_, dst_b) in enumerate(spans):
                    assert _disjoint(src_a, dst_b), (call, a, b)
                    assert a == b or _disjoint(dst_a, dst_b), (call, a, b)
            for s, so, d, do, c in copies:
                assert c > 0
                bufs[d][do:do + c] = bufs[s][so:so + c]
        n_ops.add(1 + bool(plan["segs"]) + bool(plan["segs_back"]) + 2 * any(p["k1"] > p["k0"] for p in plan["rows"]))
        for i, p in enumerate(plan["rows"]):
            if p["swap"]:
                win[i], alt[i] = alt[i], win[i]
            for k in range(p["k0"], p["k1"]):
                feats[i][(k - p["fbase"]) * WIDTH:(k - p["fbase"] + 1) * WIDTH] = k
            assert p["k1"] - p["fbase"] <= FC
        # ---- against the per-row rule
        assert FC == shared["FC"]
        for i, (x, p) in enumerate(zip(ref, plan["rows"])):
            assert (p["n"], p["base"], p["n_feat"], p["fbase"]) == (x.n, x.base, x.n_feat, x.fbase), (call, i)
            assert win[i].size == x.w.size == p["cap"]
            assert np.array_equal(win[i][:x.n - x.base], np.arange(x.base, x.n)), (call, i)
            assert np.array_equal(x.w[:x.n - x.base], np.arange(x.base, x.n))
            assert x.base <= _first_sample(x.n_feat)
            pend = np.arange(x.n_ring, x.n_feat)
            assert np.array_equal(feats[i].reshape(-1, WIDTH)[pend - x.fbase], np.repeat(pend[:, None], WIDTH, 1)), (call, i)
            assert np.array_equal(x.feats[pend - x.fbase], pend)
        if rng.random() < 0.6:
            for x in ref:
                x.drain()
    seen = set().union(*(x.events for x in ref))
    assert {"window compacted", "features compacted", "feature block grown"} <= seen, seen
    assert max(n_ops) == 5 and min(n_ops) >= 1


def test_plan_push_grows_a_window_for_one_large_chunk():
    """a single chunk that does not fit beside what must stay: the plan asks for a larger alternate buffer and swaps into it"""
    state = [dict(n=5000, base=3000, n_feat=_ready(5000), fbase=0, n_ring=0)]
    plan = live.plan_push(state, [4096], [9000], 40, WIDTH, _first_sample, _ready)
    p = plan["rows"][0]
    keep = 5000 - p["base"]
    assert p["swap"] and p["cap"] == keep + 9000 > 4096 and p["base"] == _first_sample(state[0]["n_feat"]) > 3000
    assert plan["segs"][0] == (("win", 0), p["base"] - 3000, ("alt", 0), 0, keep)
    assert plan["segs"][1] == (("stage", None), 0, ("alt", 0), keep, 9000)
    assert plan["FC"] == p["k1"] - p["k0"] + state[0]["n_feat"] > 40      # ... and more frames than a block of 40 holds


# ----------------------------------------------------------------------------- the second header against capi.EXT_*
# (the parsing helpers of tests/test_abi.py, for include/zeggs_hip_live.h)
_SCALARS = {"int": "int", "long": "long", "size_t": "size_t", "uint64_t": "uint64", "float": "float", "double": "double"}
_ELEMENTS = {"float": "f32*", "double": "f64*", "int": "i32*", "unsigned": "i32*", "int64_t": "i64*", "long": "i64*",
             "long long": "i64*", "uint8_t": "u8*", "unsigned char": "u8*", "char": "u8*", "void": "any*"}
_C_WORDS = {"int", "long", "unsigned", "char", "float", "double", "void", "size_t", "uint64_t", "int64_t", "uint8_t"}
_CTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
           "double": ctypes.c_double}


def _header_text():
    return re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "zeggs_hip_live.h").read_text(), flags=re.S)


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


def test_extension_prototypes_are_the_second_header():
    """capi.EXT_PROTOTYPES against include/zeggs_hip_live.h by the rules test_abi.py applies to the main header: the same names; per
    function the return kind, the parameter count, every parameter's kind and every device pointer's element type; the library
    exports them all, the header includes the main one and names the version, and PROTOTYPES is still the main header's set"""
    header = _header_prototypes()
    assert set(header) == set(capi.EXT_PROTOTYPES) and len(header) == 6
    assert not set(capi.EXT_PROTOTYPES) & set(capi.PROTOTYPES) and len(capi.PROTOTYPES) == 122 and len(capi.STRUCTS) == 21
    assert {b for _, _, ps in header.values() for b, depth in ps if depth == 0} <= set(_SCALARS)       # no struct by value
    structs = {**capi.STRUCTS, **capi.EXT_STRUCTS}
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
            elif kind == "str":
                assert (base, depth) == ("char", 1), where
            elif kind == "stream":
                assert (base, depth) == ("void", 1), where
            elif kind == "host*":
                assert depth >= 1, where
            elif base.startswith("Zeggs"):
                assert kind == base + "*" and depth == 1 and base in structs, where
            else:
                assert depth == 1 and kind == _ELEMENTS[base], where
    text = (ROOT / "include" / "zeggs_hip_live.h").read_text()
    assert '#include "zeggs_hip.h"' in text
    L, api = ops.lib(), capi.api()
    assert L.zeggs_version() >= 107 and "zeggs_version() >= 107" in text
    for n in header:
        assert hasattr(L, n), f"libzeggs_hip.so does not export {n}"
        assert getattr(api, n).argtypes is not None and getattr(L, n).argtypes is None


def test_extension_struct_mirrors_are_the_second_header():
    structs = _header_structs()
    assert set(structs) == set(capi.EXT_STRUCTS) == {"ZeggsMelRow", "ZeggsSeg"}
    for name, fields in structs.items():
        mirror = capi.EXT_STRUCTS[name]._fields_
        assert [f for f, _ in mirror] == [f for f, _, _, _ in fields], name
        for (f, ctype), (_, base, depth, n) in zip(mirror, fields):
            want = ctypes.c_void_p if depth else _CTYPES[base]
            assert ctype is (want * n if n else want), (name, f)
    assert ctypes.sizeof(capi.Seg) == 24 and ctypes.sizeof(capi.MelRow) == 56
    assert int(re.search(r"#define ZEGGS_MAX_SEGMENTS (\d+)", _header_text()).group(1)) == 256


# ----------------------------------------------------------------------------- zeggs_copy_segments: refused on the host
def _segs(*triples):
    arr = (capi.Seg * len(triples))()
    for g, (src, dst, count) in zip(arr, triples):
        g.src, g.dst, g.count = src, dst, count
    return arr


@pytest.mark.parametrize("what,triples,match", [
    ("a source that overlaps its destination", [(0x10000, 0x10000 + 4 * 99, 100)], "source of segment 0 overlaps the destination of segment 0"),
    ("two destinations that overlap", [(0x10000, 0x20000, 64), (0x11000, 0x20000 + 4 * 63, 8)], "destinations of segments 0 and 1 overlap"),
    ("a source inside another segment's destination", [(0x10000, 0x20000, 64), (0x20000 + 4 * 10, 0x30000, 8)],
     "source of segment 1 overlaps the destination of segment 0"),
    ("a negative count", [(0x10000, 0x20000, 8), (0x30000, 0x40000, -1)], "segment 1: negative count"),
    ("a misaligned pointer", [(0x10002, 0x20000, 8)], "segment 0: NULL or misaligned"),
    ("too many segments", [(0x100000 + 64 * i, 0x900000 + 64 * i, 4) for i in range(257)], r"257 segments \(0\.\.256\)"),
])
def test_copy_segments_refuses_on_the_host(what, triples, match):
    """every refusal comes before the launch (the addresses are never followed, there is no device here), with the segment named"""
    arr = _segs(*triples)
    with pytest.raises(RuntimeError, match="zeggs_copy_segments: copy segments: .*" + match):
        capi.api().zeggs_copy_segments(arr, ctypes.cast(ctypes.c_void_p(0x7000), ctypes.POINTER(capi.Seg)), len(triples), None)
    assert ops.lib().zeggs_copy_segments(arr, ctypes.c_void_p(0x7000), len(triples), None) == -1


def test_copy_segments_accepts_nothing_to_do():
    """n = 0 and segments of count 0 (their pointers are not looked at) succeed without a launch"""
    api = capi.api()
    assert api.zeggs_copy_segments(None, None, 0, None) == 0
    assert api.zeggs_copy_segments(_segs((0, 0, 0), (0x10000, 0x10000, 0)), None, 2, None) == 0
