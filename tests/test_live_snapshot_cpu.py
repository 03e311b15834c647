"""Host-only parts of LiveServer.snapshot() / restore(): the span rules of csrc/snapshot_math.h on the host
(tests/host/snapshot_check.cpp, plain and under sanitizers, and against the library's own span reports),
include/zeggs_hip_snapshot.h against zeggs/capi.py, the blob format (built on the host from synthetic sections, parsed by
live.snapshot_info, every refusal naming its field or section) and every refusal of zeggs_live_pack / zeggs_live_unpack that
comes before a launch.  No GPU needed -- the library loads on the CPU for host-only calls."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_live_loudness_cpu as third
from zeggs import capi, live, ops

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "zeggs_hip_snapshot.h"


# ----------------------------------------------------------------------------- 1. csrc/snapshot_math.h on the host
def _library_spans(words):
    """the library's report for a line of the check program's table, or None where the library refuses the dims"""
    api, family, args = capi.api(), words[0], [int(w) for w in words[1:]]
    if family == "loudness":
        fs, nb = args[:2]
        d = capi.LoudDims(fs, 64, nb, 1, -20.0, -30.0, 30.0, (ctypes.c_double * 10)(*[1.0] * 10))
        return ops._spans(api.zeggs_live_loudness_spans, d, 63), args[2:], api.zeggs_live_loudness_state_bytes(d)
    if family == "resample":
        d = capi.ResampleDims(64, args[0])
        return ops._spans(api.zeggs_resample_spans, d, 63), args[1:], api.zeggs_resample_state_bytes(d)
    d = capi.FramesDims(64, args[0], 20, 7, 0)
    if family == "frames":
        return ops._spans(api.zeggs_live_frames_spans, d, 63), args[1:], api.zeggs_live_frames_state_bytes(d)
    if family == "retime":
        return ops._spans(api.zeggs_live_retime_spans, d, 63), args[1:], api.zeggs_live_retime_state_bytes(d)
    if args[1] == 0:          # (the header's arithmetic takes a ring of no frames; the library's dims check does not)
        return None
    return ops._spans(api.zeggs_live_refilter_spans, d, args[1], 63), args[2:], api.zeggs_live_refilter_state_bytes(d, args[1])


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_span_rules_on_the_host(tmp_path, flags):
    """tests/host/snapshot_check.cpp: a stand-alone program over the header the library reports its spans from (its head says
    what it walks: 1, 5 and 75 joints, max_half 0, 4 and 16, histories 2 and 3072, loudness rings of 1 and 2^20 blocks, rows 1, 2
    and 64; the span rules of the eighth header, and row 0 of 1 against row 63 of 64); once plain, once under the address and
    undefined-behaviour sanitizers (host code with its own main, run directly); the spans it prints for row 63 of 64 are the
    library's own, and they end where the library's state block ends"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "snapshot_check"
    b = subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "snapshot_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe), "--table"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "snapshot_check: ok"
    seen = set()
    for line in lines[:-1]:
        words = line.split()
        got = _library_spans(words)
        seen.add(words[0])
        if got is None:
            continue
        spans, flat, nbytes = got
        assert [x for s in spans for x in s] == flat, line
        assert sum(spans[-1]) == nbytes, line               # row 63 of 64 is the last thing in the block
    assert seen == {"loudness", "resample", "frames", "retime", "refilter"} and len(lines) == 4 + 2 + 3 * (1 + 1 + 3) + 1


def test_span_reports_refuse_on_the_host():
    api = capi.api()
    d = capi.FramesDims(4, 5, 20, 7, 0)
    one, two = (capi.SnapSpan * 1)(), (capi.SnapSpan * 2)()
    assert api.zeggs_live_frames_spans(d, 3, one, 1) == 1 and (one[0].offset, one[0].bytes) == (64 + 3 * 296, 296)
    assert api.zeggs_live_retime_spans(d, 0, one, 1) == 1 and (one[0].offset, one[0].bytes) == (64, 296 + 208)
    assert api.zeggs_live_refilter_spans(d, 10, 1, one, 1) == 1 and (one[0].offset, one[0].bytes) == (64 + 296 + 20 * 208, 296 + 20 * 208)
    for fn, args, match in ((api.zeggs_live_frames_spans, (d, 4, one, 1), "row 4 of 4"), (api.zeggs_live_retime_spans, (d, -1, one, 1), "row -1 of 4"),
                            (api.zeggs_live_refilter_spans, (d, 40, 0, one, 1), "max_half 40"), (api.zeggs_live_frames_spans, (d, 0, one, 0), "room for 0 spans"),
                            (api.zeggs_live_frames_spans, (d, 0, None, 1), "room for 0 spans"),
                            (api.zeggs_resample_spans, (capi.ResampleDims(2, 0), 0, one, 1), "history of 0"),
                            (api.zeggs_resample_spans, (capi.ResampleDims(2, 8), 2, one, 1), "row 2 of 2")):
        with pytest.raises(RuntimeError, match=match):
            fn(*args)
    ld = capi.LoudDims(16000, 3, 600, 1, -20.0, -30.0, 30.0, (ctypes.c_double * 10)(*[1.0] * 10))
    with pytest.raises(RuntimeError, match="room for 1 spans, the row has 2"):
        api.zeggs_live_loudness_spans(ld, 0, one, 1)
    assert api.zeggs_live_loudness_spans(ld, 2, two, 2) == 2
    row = 128 + 8 * (6400 + 1200)
    assert [(s.offset, s.bytes) for s in two] == [(2 * row, 128), (2 * row + 128, row - 128)]
    assert ops.lib().zeggs_live_frames_spans(ctypes.byref(d), 9, one, 1) == -1


# ----------------------------------------------------------------------------- 2. the eighth header against capi.SNAP_*
@pytest.fixture
def eighth(monkeypatch):
    monkeypatch.setattr(third, "HEADER", HEADER)
    return third


def test_snapshot_prototypes_are_the_eighth_header(eighth):
    """capi.SNAP_PROTOTYPES against include/zeggs_hip_snapshot.h: the same names; per function the return kind, the parameter
    count and every parameter's kind; the library exports them all; zeggs_live_snapshot_version() is 1 and the other versions
    are what they were; the new source is built"""
    header = eighth._header_prototypes()
    assert set(header) == set(capi.SNAP_PROTOTYPES) and len(header) == 8
    others = (set(capi.PROTOTYPES) | set(capi.EXT_PROTOTYPES) | set(capi.LOUD_PROTOTYPES) | set(capi.RS_PROTOTYPES) | set(capi.FR_PROTOTYPES) |
              set(capi.RT_PROTOTYPES) | set(capi.RF_PROTOTYPES))
    assert not set(capi.SNAP_PROTOTYPES) & others
    assert not set(capi.SNAP_STRUCTS) & (set(capi.STRUCTS) | set(capi.EXT_STRUCTS) | set(capi.LOUD_STRUCTS) | set(capi.RS_STRUCTS) | set(capi.FR_STRUCTS) |
                                         set(capi.RT_STRUCTS) | set(capi.RF_STRUCTS))
    assert {b for _, _, ps in header.values() for b, depth in ps if depth == 0} <= set(eighth._SCALARS)       # no struct by value
    for name, (rbase, rdepth, params) in header.items():
        ret, kinds = capi.signature(name)
        want = {("int", 0): ("status", "mask", "int"), ("long", 0): ("long",), ("size_t", 0): ("size_t",), ("char", 1): ("str",)}
        assert ret in want[(rbase, rdepth)], (name, ret)
        assert len(kinds) == len(params), name
        for i, (kind, (base, depth)) in enumerate(zip(kinds, params)):
            where = (name, i, kind, base, depth)
            assert kind in capi.KINDS, where
            if depth == 0:
                assert kind == eighth._SCALARS[base], where
            elif kind == "stream":
                assert (base, depth) == ("void", 1), where
            elif kind == "host*":
                assert depth >= 1, where
            elif base.startswith("Zeggs"):
                assert kind == base + "*" and depth == 1 and base in {**capi.SNAP_STRUCTS, **capi.FR_STRUCTS, **capi.LOUD_STRUCTS, **capi.RS_STRUCTS}, where
            else:
                assert depth == 1 and kind == eighth._ELEMENTS[base], where
    text = HEADER.read_text()
    assert '#include "zeggs_hip_refilter.h"' in text and "zeggs_live_snapshot_version() >= 1" in text
    L, api = ops.lib(), capi.api()
    assert L.zeggs_version() == 109 and L.zeggs_live_frames_version() == 1 and L.zeggs_live_retime_version() == 1 and L.zeggs_live_refilter_version() == 1
    assert L.zeggs_live_snapshot_version() == 1 and api.zeggs_live_snapshot_version() == 1
    for n in header:
        assert hasattr(L, n), f"libzeggs_hip.so does not export {n}"
        assert getattr(api, n).argtypes is not None and getattr(L, n).argtypes is None
    build = (ROOT / "ubisoft-laforge-zeroeggs_amd" / "csrc" / "build.sh").read_text()
    assert " live_snapshot " in build and "../../include/zeggs_hip_snapshot.h" in build
    assert (ops.SNAP_MAX_SPANS, ops.SNAP_MAX_SEGMENTS) == (2, 65535) and "#define ZEGGS_SNAP_MAX_SPANS 2" in text and "#define ZEGGS_SNAP_MAX_SEGMENTS 65535" in text


def test_snapshot_struct_mirror_is_the_eighth_header(eighth):
    structs = eighth._header_structs()
    assert set(structs) == set(capi.SNAP_STRUCTS) == {"ZeggsSnapSpan", "ZeggsSnapSeg"}
    for name, fields in structs.items():
        mirror = capi.SNAP_STRUCTS[name]._fields_
        assert [f for f, _ in mirror] == [f for f, _, _, _ in fields], name
        for (f, ctype), (_, base, depth, n) in zip(mirror, fields):
            want = ctypes.c_void_p if depth else eighth._CTYPES[base]
            assert ctype is want and n is None, (name, f)
    assert ctypes.sizeof(capi.SnapSpan) == 16 and ctypes.sizeof(capi.SnapSeg) == 24
    assert ops.SnapSeg is capi.SnapSeg and ops.SnapSpan is capi.SnapSpan


# ----------------------------------------------------------------------------- 3. the blob format
FP = {k: float(3 + 2 * i) for i, k in enumerate(live.SNAP_FINGERPRINT)}


def _row(**over):
    vals = dict(dict.fromkeys(live.SNAP_ROW, 0), n=5000, base=1200, n_feat=40, fbase=30, n_ring=34, kd=9, k_style=9, fade=12, rt_half=-1,
                offsets_itemsize=8, offsets_count=15)
    vals.update(over)
    return np.array([vals[k] for k in live.SNAP_ROW], "<i8")


def _sections(rng):
    """synthetic sections with sizes that are no multiples of 16, so that every boundary has padding in front of it"""
    s = dict(row=_row(), offsets=rng.standard_normal(15), window=rng.standard_normal(3800).astype(np.float32),
             feats=rng.standard_normal((10, 81)).astype(np.float32), ring=rng.standard_normal(35 * 3).astype(np.float32),
             h=rng.standard_normal(2 * 7).astype(np.float32), pose=rng.standard_normal(81).astype(np.float32),
             rpos=rng.standard_normal(3).astype(np.float32), rrot=rng.standard_normal(4).astype(np.float32),
             gaze=rng.standard_normal(15).astype(np.float32), sty_old=rng.standard_normal(5).astype(np.float32),
             sty_new=rng.standard_normal(5).astype(np.float32), loudness=rng.integers(0, 255, 128 + 16 + 8 * 31, dtype=np.uint8),
             head=rng.integers(0, 255, 296 + 4, dtype=np.uint8))
    return s


def test_blob_format_round_trip():
    """a blob built on the host from synthetic sections: snapshot_info returns the header -- format, version, sid, every fingerprint
    field, the row counters -- and the table; every section starts on a 16-byte boundary, holds its bytes, and what lies between
    two sections is zero; a section a stream does not have is in the table with 0 bytes"""
    rng = np.random.default_rng(3)
    sec = _sections(rng)
    blob = live.snapshot_build(41, 1, FP, sec)
    assert blob.dtype == np.uint8 and blob.ndim == 1 and blob[:8].tobytes() == b"ZEGGSNAP"
    info = live.snapshot_info(blob)
    assert (info["format"], info["version"], info["sid"], info["nbytes"]) == (live.SNAP_FORMAT, 1, 41, blob.size)
    assert info["fingerprint"] == FP and list(info["fingerprint"]) == list(live.SNAP_FINGERPRINT)
    assert info["row"] == dict(zip(live.SNAP_ROW, _row().tolist()))
    assert list(info["sections"]) == list(live.SNAP_SECTIONS)
    covered = np.zeros(blob.size, bool)
    end = 0
    for name, (off, nb) in info["sections"].items():
        assert off % 16 == 0 and off >= end, name
        want = np.ascontiguousarray(sec[name]).tobytes() if name in sec else b""
        assert nb == len(want) and blob[off:off + nb].tobytes() == want, name
        covered[off:off + nb] = True
        end = off + nb
    assert info["sections"]["resample"][1] == 0 and blob.size % 16 == 0 and blob.size - end < 16
    first = info["sections"]["row"][0]
    assert not blob[first:][~covered[first:]].any()
    assert live.snapshot_info(blob.tobytes()) == info == live.snapshot_info(bytearray(blob.tobytes()))
    assert live.snapshot_layout([0] * len(live.SNAP_SECTIONS))[1] % 16 == 0


def _patched(blob, at, dtype, value):
    b = blob.copy()
    b[at:at + np.dtype(dtype).itemsize] = np.frombuffer(np.array([value], dtype).tobytes(), np.uint8)
    return b


def test_parser_refuses_with_the_field_or_section_named():
    rng = np.random.default_rng(4)
    blob = live.snapshot_build(7, 1, FP, _sections(rng))
    info = live.snapshot_info(blob)
    with pytest.raises(ValueError, match="magic b'ZEGGSNAQ'"):
        live.snapshot_info(_patched(blob, 7, "u1", ord("Q")))
    with pytest.raises(ValueError, match="format version 2 "):
        live.snapshot_info(_patched(blob, 8, "<u4", 2))
    with pytest.raises(ValueError, match="44 fingerprint fields"):
        live.snapshot_info(_patched(blob, 24, "<u4", 44))
    with pytest.raises(ValueError, match="total length"):
        live.snapshot_info(_patched(blob, 32, "<u8", blob.size + 16))
    # a truncation at every section boundary, and one byte short of the end
    cuts = sorted({off for off, _ in info["sections"].values()} | {off + nb for off, nb in info["sections"].values()})
    for cut in cuts:
        if cut < blob.size:
            # (a cut inside the padding behind the last bytes of the last section leaves every section whole: the total says so)
            with pytest.raises(ValueError, match="section '\\w+' ends at byte \\d+, the blob has %d: truncated|total length %d bytes" % (cut, cut)):
                live.snapshot_info(blob[:cut])
    with pytest.raises(ValueError, match="truncated|total length %d bytes" % (blob.size - 1)):
        live.snapshot_info(blob[:-1])
    for cut in (0, 20, live._SNAP_HEAD + 8):
        with pytest.raises(ValueError, match="truncated"):
            live.snapshot_info(blob[:cut])
    with pytest.raises(ValueError, match="total length %d bytes" % (blob.size + 16)):
        live.snapshot_info(np.concatenate([blob, np.zeros(16, np.uint8)]))
    # a section length that disagrees with the table: each entry of the table changed in turn, to a size with another padded
    # length (the next section is then not where the layout puts it) and to one with the same (the row counters or the total say so)
    o_tab = live._SNAP_HEAD + 8 * len(live.SNAP_FINGERPRINT)
    for i, name in enumerate(live.SNAP_SECTIONS):
        off, nb = info["sections"][name]
        later = live.SNAP_SECTIONS[i + 1] if i + 1 < len(live.SNAP_SECTIONS) else None
        with pytest.raises(ValueError, match="section '%s' at offset" % later if later else "section '%s' ends at byte" % name):
            live.snapshot_info(_patched(blob, o_tab + 24 * i + 16, "<u8", nb + 32))
        with pytest.raises(ValueError, match="section '%s' at offset %d" % (name, off + 16)):
            live.snapshot_info(_patched(blob, o_tab + 24 * i + 8, "<u8", off + 16))
        with pytest.raises(ValueError, match="section %d is of kind 99" % i):
            live.snapshot_info(_patched(blob, o_tab + 24 * i, "<u4", 99))
    # the sections whose sizes the row counters fix
    sec = _sections(rng)
    for name, over, match in (("window", dict(n=5001), "section 'window' has 15200 bytes, its row counters ask for 15204"),
                              ("offsets", dict(offsets_count=18), "section 'offsets' has 120 bytes, its row counters ask for 144")):
        with pytest.raises(ValueError, match=match):
            live.snapshot_info(live.snapshot_build(7, 1, FP, dict(sec, row=_row(**over))))
    with pytest.raises(ValueError, match="section 'row' has 160 bytes, 168 expected"):
        live.snapshot_info(live.snapshot_build(7, 1, FP, dict(sec, row=_row()[:-1])))


def test_every_fingerprint_field_is_compared():
    """restore()'s configuration check on the parsed header: each field changed in turn raises a ValueError that names it and
    both values; the fields are those the issue lists (the weights and the statistics are not among them)"""
    blob = live.snapshot_build(7, 1, FP, _sections(np.random.default_rng(5)))
    live.snapshot_check_fingerprint(live.snapshot_info(blob)["fingerprint"], FP)
    o_fp = live._SNAP_HEAD
    for i, k in enumerate(live.SNAP_FINGERPRINT):
        got = live.snapshot_info(_patched(blob, o_fp + 8 * i, "<f8", FP[k] + 1.0))["fingerprint"]
        with pytest.raises(ValueError, match=f"a server with {k} = {FP[k] + 1.0!r}, this one has {k} = {FP[k]!r}"):
            live.snapshot_check_fingerprint(got, FP)
    need = {"tick", "fs", "fps", "FC", "ring_depth", "ring_width", "H", "ST", "PO", "speech_width", "KW", "loudness", "frames_joints", "frames_what",
            "frames_order", "frames_seq", "retime_max_L", "filter_half_max", "resample_zero_crossings"}
    assert need <= set(live.SNAP_FINGERPRINT) and len(set(live.SNAP_FINGERPRINT)) == len(live.SNAP_FINGERPRINT) == 43
    assert {f"mel_{f}" for f, _ in capi.MelDims._fields_} <= set(live.SNAP_FINGERPRINT)


# ----------------------------------------------------------------------------- 4. refusals of the two launches
GOOD = [dict(src=0x10000, dst_offset=0, bytes=4096), dict(src=0x20000, dst_offset=4096, bytes=12), dict(src=0x30004, dst_offset=4112, bytes=70000)]
BLOB_BYTES = 4112 + 70000


def _segs(*over):
    arr = (capi.SnapSeg * len(over))()
    for q, base, o in zip(arr, GOOD, over):
        for k, v in dict(base, **o).items():
            setattr(q, k, v)
    return arr


@pytest.mark.parametrize("what,over,match", [
    ("a NULL pointer", [dict(), dict(src=0)], "record 1: NULL or misaligned pointer"),
    ("a misaligned pointer", [dict(src=0x10002)], "record 0: NULL or misaligned pointer"),
    ("a size that is no multiple of 4", [dict(), dict(), dict(bytes=70001)], "record 2: 70001 bytes is no multiple of 4"),
    ("a misaligned blob offset", [dict(), dict(dst_offset=4098)], "record 1: blob offset 4098 is no multiple of 4"),
    ("a record past the blob", [dict(), dict(), dict(bytes=70004)], "record 2: blob offset 4112 \\+ 70004 bytes is past the blob's 74112"),
    ("an offset past the blob", [dict(dst_offset=1 << 40)], "record 0: blob offset 1099511627776 \\+ 4096 bytes is past the blob's 74112"),
    ("two records whose blob ranges overlap", [dict(), dict(dst_offset=4092)], "the blob ranges of records 0 and 1 overlap"),
    ("an overlap found after sorting", [dict(dst_offset=4112), dict(), dict(dst_offset=0)], "the blob ranges of records 1 and 2 overlap"),
    ("records without a device copy", [dict(), dict(), dict()], "must also be in device memory"),
])
def test_pack_and_unpack_refuse_on_the_host(what, over, match):
    """every refusal comes before the launch (the addresses are never followed, there is no device here), with the record named"""
    arr, api, blob = _segs(*over), capi.api(), ctypes.c_void_p(0x4000000)
    for fn, who in ((api.zeggs_live_pack, "live pack"), (api.zeggs_live_unpack, "live unpack")):
        with pytest.raises(RuntimeError, match=f"{fn.__name__}: {who}: .*{match}"):
            fn(arr, None, len(over), blob, BLOB_BYTES, None)
    assert ops.lib().zeggs_live_pack(arr, None, len(over), blob, ctypes.c_size_t(BLOB_BYTES), None) == -1


def test_pack_and_unpack_check_the_blob_and_the_count():
    api, dev = capi.api(), ctypes.cast(ctypes.c_void_p(0x7000), ctypes.POINTER(capi.SnapSeg))
    for fn in (api.zeggs_live_pack, api.zeggs_live_unpack):
        assert fn(None, None, 0, None, 0, None) == 0                      # nothing to do: no launch, no error
        assert fn(_segs(dict(bytes=0, src=0)), None, 1, None, 0, None) == 0
        with pytest.raises(RuntimeError, match="NULL or misaligned blob"):
            fn(_segs(dict()), dev, 1, None, BLOB_BYTES, None)
        with pytest.raises(RuntimeError, match="NULL or misaligned blob"):
            fn(_segs(dict()), dev, 1, ctypes.c_void_p(0x4000002), BLOB_BYTES, None)
        with pytest.raises(RuntimeError, match="record 0: its state side lies inside the blob"):
            fn(_segs(dict(src=0x4000100)), dev, 1, ctypes.c_void_p(0x4000000), BLOB_BYTES, None)
        with pytest.raises(RuntimeError, match="65536 records"):
            fn(_segs(dict()), dev, 65536, ctypes.c_void_p(0x4000000), BLOB_BYTES, None)
        with pytest.raises(RuntimeError, match="-1 records"):
            fn(_segs(dict()), dev, -1, ctypes.c_void_p(0x4000000), BLOB_BYTES, None)
        with pytest.raises(RuntimeError, match="NULL records"):
            fn(None, dev, 2, ctypes.c_void_p(0x4000000), BLOB_BYTES, None)
