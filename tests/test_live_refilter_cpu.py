"""Host-only parts of the filter stage of LiveServer's re-timing output head: the float64 oracle (tests/live_refilter_oracle.py)
against the frames oracle on a pose held still, against tones above and below half the output rate and against itself under any
cutting of the stream, the filter's table and its own frequency response, the counting rule, the shared header on the host
(tests/host/refilter_math_check.cpp, plain and under sanitizers, and against the Python restatement),
include/zeggs_hip_refilter.h against zeggs/capi.py, every refusal that comes before a launch, and the ValueErrors of
LiveServer(retime=dict(filter=...)) and open(filtered=).  No GPU needed -- the library loads on the CPU for host-only calls."""
import ctypes
import shutil
import subprocess
import types
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import live_frames_oracle as fo
import live_refilter_oracle as rf
import live_retime_oracle as ro
import test_live_loudness_cpu as third
from zeggs import audio, capi, live, ops, synth

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "zeggs_hip_refilter.h"
CONF = dict(third.CONF, normalize_loudness=False)
SKELETONS = dict(fo.SKELETONS, rig=list(synth.PARENTS))
T_IN = 48
# the GPU test's cases (tests/test_gpu_live_refilter.py): skeleton, and the seed of fo.inputs(J, 48, seed)
GPU_CASES = {"one": 1, "tree": 1, "rig": 2}
LEFT_OUT_CAP = 0.10


def _seq(name):
    return fo.TREE_SEQ if name == "tree" else ops.frames_seq(SKELETONS[name])


# ----------------------------------------------------------------------------- 1. the table
def test_resample_table_is_the_table_it_was():
    """audio.resample_table after its body moved into audio.sinc_table: bit for bit the formula as it stood, at the audio
    converter's defaults and at others"""
    for fi, fo_, kw in ((48000, 16000, {}), (44100, 16000, dict(zero_crossings=16, rolloff=0.9, beta=8.0)), (8000, 16000, {}), (22050, 16000, dict(beta=0.0))):
        o = dict(dict(zero_crossings=64, rolloff=0.95, beta=10.0), **kw)
        tab, (L, M, WL) = audio.resample_table(fi, fo_, **kw)
        assert (L, M) == audio.resample_ratio(fi, fo_) and WL == o["zero_crossings"] * max(L, M)
        H = -(-WL // L)
        num = np.arange(L, dtype=np.int64)[:, None] + (H - np.arange(2 * H + 1, dtype=np.int64))[None, :] * L
        t, W, c = num / float(L), WL / float(L), o["rolloff"] * min(1.0, L / float(M))
        inside = np.abs(num) < WL
        r = np.where(inside, t / W, 0.0)
        h = c * np.sinc(c * t) * np.i0(o["beta"] * np.sqrt(1.0 - r * r)) / np.i0(o["beta"])
        assert tab.tobytes() == np.ascontiguousarray(np.where(inside, h, 0.0)).tobytes(), (fi, fo_)


@pytest.mark.parametrize("ratio", rf.RATIOS + ((1, 4), (1024, 1023)), ids=lambda r: f"{r[0]}over{r[1]}")
def test_table_is_the_definition_with_unit_gain_per_phase(ratio):
    """ops.refilter_table against the oracle's element-by-element statement of the definition; every phase row sums to 1 (the
    sum in ascending j) to the rounding of its terms; H = ceil(Z max(L, M) / L); before the division the rows are audio.sinc_table's"""
    L, M = ratio
    for opts in (rf.DEFAULTS, dict(zero_crossings=2, rolloff=1.0, beta=0.0), dict(zero_crossings=8, rolloff=0.5, beta=9.0)):
        if L > 64 and opts is not rf.DEFAULTS:
            continue
        tab, H = ops.refilter_table(L, M, **opts)
        want, Hw = rf.table(L, M, **opts)
        assert H == Hw == rf.half(L, M, opts["zero_crossings"]) == ops.refilter_half(L, M, opts["zero_crossings"]) and tab.shape == (L, 2 * H + 1)
        assert np.abs(tab - want).max() <= 4e-16
        raw, WL = audio.sinc_table(L, M, **opts)
        assert WL == opts["zero_crossings"] * max(L, M)
        for phase in range(0, L, max(1, L // 7)):
            s = t = 0.0
            for j in range(2 * H + 1):
                s, t = s + raw[phase, j], t + tab[phase, j]
            assert np.array_equal(tab[phase], raw[phase] / s) and abs(t - 1.0) <= (2 * H + 1) * 2.0 ** -53      # (one rounding a term)


def test_table_refuses_what_the_filter_does_not_take():
    for L, M in ((1025, 1024), (1, 5), (2, 9), (0, 1)):
        with pytest.raises(ValueError, match=f"the ratio {L} / {M}"):
            ops.refilter_table(L, M)
    for bad, match in ((dict(zero_crossings=9), "zero_crossings 9"), (dict(zero_crossings=0), "zero_crossings 0"), (dict(zero_crossings=2.5), "zero_crossings 2.5"),
                       (dict(rolloff=0.0), "rolloff 0.0"), (dict(rolloff=1.5), "rolloff 1.5"), (dict(beta=-1.0), "beta -1.0"),
                       (dict(beta=float("nan")), "beta nan"), (dict(width=3), "keys"), ("sharp", "True or a dict")):
        with pytest.raises(ValueError, match=match):
            ops.refilter_options(bad)
    assert ops.refilter_options(None) == ops.refilter_options(True) == ops.REFILTER_DEFAULTS == rf.DEFAULTS


def test_the_default_tables_own_response():
    """where the tone bounds come from: the default table's float64 response, every phase row, recomputed from the table the
    product builds -- at most 0.001 in the stop band (20 Hz at 24 frames a second: 0.0008; 25 Hz at 30: 0.0003; 25 and 29 Hz at
    29.97: 0.001 and 0.0006) and within 0.002 of 1 at 3 Hz (1.0014 at 24, the worst phase); the tone tests ask 0.01 and 0.99"""
    for (L, M), stop in (((2, 5), (20,)), ((1, 2), (25,)), ((500, 1001), (25, 29))):
        tab, H = ops.refilter_table(L, M)
        for f in stop:
            worst = rf.response(tab, H, f).max()
            print(f"{L}/{M}: {f} Hz -> {worst:.6f}")
            assert worst <= 0.001, (L, M, f, worst)
        g = rf.response(tab, H, 3.0)
        print(f"{L}/{M}: 3 Hz -> {g.min():.6f} .. {g.max():.6f}")
        assert np.abs(g - 1.0).max() <= 0.002, (L, M, g.min(), g.max())


# ----------------------------------------------------------------------------- 2. a pose held still
@pytest.mark.parametrize("ratio", rf.RATIOS, ids=lambda r: f"{r[0]}over{r[1]}")
def test_a_pose_held_still_stays_that_pose(ratio):
    """a random pose of the tree held for 48 frames, placed and not: every output of every output frame (n_out(48) of them)
    equals the frames oracle's frame of that pose within 1e-12 -- unit DC gain per phase.  (The root's rotation is given as a
    unit quaternion in float64: a float32 one lies 1e-8 off the unit sphere, the frames oracle hands it out as it is and the
    filter's division by the norm brings it back.  The joints' two-axis rows are the random pose's times 4096: the decoding
    divides an axis by |v| + 1e-10, which leaves a quaternion of unit-length rows 3e-11 off the sphere -- the decoder's guard, not
    the filter's gain; with rows this long it is below 1e-13.)"""
    L, M = ratio
    tab, H = rf.table(L, M)
    x = fo.inputs(5, 1, 7)
    x["rrot"] = x["rrot"].astype(np.float64) / np.linalg.norm(x["rrot"].astype(np.float64), axis=-1, keepdims=True)
    x["ltxy"] = x["ltxy"] * np.float32(4096.0)
    held = {k: np.repeat(v, T_IN, axis=0) for k, v in x.items()}
    for place in (None, fo.PLACE):
        for order in ("zyx", "xzy"):
            o = rf.frames(held["rpos"], held["rrot"], held["lpos"], held["ltxy"], SKELETONS["tree"], fo.TREE_SEQ, L, M, tab, H, place, order)
            want = fo.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], SKELETONS["tree"], fo.TREE_SEQ, place, order)
            assert len(o["k"]) == ro.n_out(T_IN, L, M)
            for key in ("root_pos", "root_rot", "lrot", "lpos", "gpos", "grot", "bvh"):
                err = np.abs(o[key] - want[key][0:1]).max()
                assert err <= 1e-12, (key, err, place is not None, order)


# ----------------------------------------------------------------------------- 3. tones
# The amplitude of a sequence of angles is its largest |angle|, for the input and for an output alike, over the frames whose
# taps all lie inside the stream (no held frame).  The 20 Hz tone at 60 frames a second has three samples a period, 0 and
# +-0.866e-3: that is the input's amplitude, and the unfiltered 24-frame output -- whose even frames ARE such samples --
# shows it whole.  (A least-squares fit of a 4 Hz sinusoid to the unfiltered output gives 0.75e-3: its odd frames are the
# midpoints of two samples, half the size.  The filtered bounds hold under either measure.)
T_TONE = 120


def _tone(L, M, f, filtered):
    x, ang = rf.tone_inputs(T_TONE, f)
    tab, H = rf.table(L, M)
    if filtered:
        o = rf.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], [-1], [0], L, M, tab, H)
    else:
        o = ro.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], [-1], [0], L, M)
    N = ro.n_out(T_TONE, L, M)
    keep = rf.interior(N, T_TONE, L, M, H)
    assert keep.sum() >= 20
    return np.abs(rf.tone_angle(o["lrot"][:, 0])[keep]).max(), np.abs(ang).max(), o, keep


def test_tones_at_24_frames_a_second():
    """the case that shows the feature: 20 Hz at 2 / 5 -- the unfiltered oracle shows the 4 Hz alias at >= 0.9 of the input
    amplitude (it changes sign within 4 output frames: 4 Hz at 24), the filtered oracle at <= 0.01 of it; a 3 Hz tone keeps
    >= 0.99 of its amplitude through the filter (and no more than 1.01)"""
    alias, amp, o, keep = _tone(2, 5, 20, False)
    a = rf.tone_angle(o["lrot"][:, 0])[keep]
    fit = np.linalg.lstsq(np.stack([np.sin(2 * np.pi * 4 / 24 * np.arange(len(a))), np.cos(2 * np.pi * 4 / 24 * np.arange(len(a)))], 1), a, rcond=None)[0]
    print(f"20 Hz at 24: input {amp:.3e}, unfiltered {alias:.3e} ({alias / amp:.3f}); least-squares 4 Hz component {np.hypot(*fit):.3e}")
    assert amp == pytest.approx(rf.TONE_AMP * np.sin(np.pi / 3), rel=1e-9)
    assert alias >= 0.9 * amp
    spec = np.abs(np.fft.rfft(a[:24 * (len(a) // 24)]))
    assert np.argmax(spec) * 24.0 / (24 * (len(a) // 24)) == 4.0          # the strongest line of the output is 4 Hz
    left, _, _, _ = _tone(2, 5, 20, True)
    print(f"20 Hz at 24: filtered {left:.3e} ({left / amp:.5f})")
    assert left <= 0.01 * amp
    kept, amp3, _, _ = _tone(2, 5, 3, True)
    print(f"3 Hz at 24: filtered {kept:.6e} of {amp3:.6e} ({kept / amp3:.5f})")
    assert amp3 == pytest.approx(rf.TONE_AMP, rel=1e-9) and 0.99 * amp3 <= kept <= 1.01 * amp3


@pytest.mark.parametrize("ratio,f", [((1, 2), 25), ((1, 2), 29), ((500, 1001), 25), ((500, 1001), 29)], ids=["30fps-25Hz", "30fps-29Hz", "2997fps-25Hz", "2997fps-29Hz"])
def test_tones_at_30_and_2997_frames_a_second(ratio, f):
    """25 and 29 Hz at 1 / 2 and 500 / 1001: the filtered output is <= 0.01 of the input amplitude; the unfiltered one is not"""
    left, amp, _, _ = _tone(*ratio, f, True)
    alias, _, _, _ = _tone(*ratio, f, False)
    print(f"{f} Hz at {ratio[0]}/{ratio[1]}: input {amp:.3e}, unfiltered {alias / amp:.3f}, filtered {left / amp:.5f}")
    assert left <= 0.01 * amp and alias >= 0.5 * amp


# ----------------------------------------------------------------------------- 4. counting and cuts
@pytest.mark.parametrize("ratio", rf.RATIOS + ((1, 4), (5, 12), (8, 1), (1024, 4095)), ids=lambda r: f"{r[0]}over{r[1]}")
def test_counting_rule(ratio):
    """nf is monotone and 0 up to H frames; the frames emitted after n inputs are those whose last tap k + H has arrived; nf(n)
    + tail = n_out(n) with a tail that is never negative; the counts of any cut add up; ops.refilter_n_out is the same rule"""
    L, M = ratio
    rng = np.random.default_rng(L * 7 + M)
    for Z in (1, 4, 8):
        H = rf.half(L, M, Z)
        counts = [rf.nf(n, L, M, H) for n in range(300)]
        assert all(b >= a for a, b in zip(counts, counts[1:])) and not any(counts[:H + 1]) and counts[H + 1] >= 1
        for n in range(300):
            N = counts[n]
            assert ops.refilter_n_out(n, L, M, H) == N and rf.emitted(n, L, M, H, False) == N
            assert N == 0 or ro.position(N - 1, L, M)[0] + H <= n - 1
            assert ro.position(N, L, M)[0] + H >= n
            tail = ro.n_out(n, L, M) - N
            assert tail >= 0 and rf.emitted(n, L, M, H, True) == N + tail
        cuts, n, total = rng.integers(0, 22, 30).tolist(), 0, 0
        for c in cuts:
            total, n = total + rf.nf(n + c, L, M, H) - rf.nf(n, L, M, H), n + c
        assert total == rf.nf(n, L, M, H)


@pytest.mark.parametrize("ratio", rf.RATIOS, ids=lambda r: f"{r[0]}over{r[1]}")
def test_any_cutting_of_48_frames_gives_the_same_outputs(ratio):
    """the oracle as a running stream (each call sees only the frames delivered so far, the tail leaves with a final record that
    brings no frame) in one call of 48, forty-eight of 1, 5 + 1 + 14 + 28 and random cuts: the same numbers, bit for bit, as
    the whole closed stream at once; the calls' counts follow nf, and their sum is n_out(48)"""
    L, M = ratio
    tab, H = rf.table(L, M)
    x = fo.inputs(5, T_IN, 1)
    full = fo.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], SKELETONS["tree"], fo.TREE_SEQ, fo.PLACE)
    loc = (full["root_pos"], full["raw"]["root_rot"], full["raw"]["lrot"], full["lpos"])
    whole = rf.filter_locals(*loc, L, M, tab, H)[:4]
    rng = np.random.default_rng(5)
    rand = []
    while sum(rand) < T_IN:
        rand.append(min(int(rng.integers(1, 12)), T_IN - sum(rand)))
    for cuts in ([48], [1] * 48, [5, 1, 14, 28], rand):
        got, counts = rf.stream_locals(*loc, L, M, tab, H, cuts)
        assert sum(counts) == ro.n_out(T_IN, L, M) and counts[-1] == ro.n_out(T_IN, L, M) - rf.nf(T_IN, L, M, H)
        n = 0
        for c, e in zip(cuts, counts):
            assert e == rf.nf(n + c, L, M, H) - rf.nf(n, L, M, H)
            n += c
        for g, w in zip(got, whole):
            assert g.tobytes() == w.tobytes(), cuts
    # final on the last record that brings frames is the same stream
    got, counts = rf.stream_locals(*loc, L, M, tab, H, [20, 28], final=False)
    assert sum(counts) == rf.nf(T_IN, L, M, H)


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_oracle_alone_meets_the_gpu_tests_conditions(name):
    """for the seeds and ratios of tests/test_gpu_live_refilter.py the oracle alone leaves at most 10 % of a case's output frames
    out by the Euler rule (|sin| of the middle angle <= 0.999), in both channel orders, with and without the placement"""
    x = fo.inputs(len(SKELETONS[name]), T_IN, GPU_CASES[name])
    for L, M in rf.RATIOS:
        tab, H = rf.table(L, M)
        for order in ("zyx", "xzy"):
            for place in (None, fo.PLACE):
                o = rf.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], SKELETONS[name], _seq(name), L, M, tab, H, place, order)
                assert len(o["k"]) == ro.n_out(T_IN, L, M)
                assert rf.left_out(o) <= LEFT_OUT_CAP, (name, L, M, order, place is not None, rf.left_out(o))


# ----------------------------------------------------------------------------- 5. csrc/refilter_math.h on the host
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_refilter_rules_on_the_host(tmp_path, flags):
    """tests/host/refilter_math_check.cpp: a stand-alone program over the header the kernel uses (its head says what it walks --
    the counting, and every ring slot a tap reads, for cuts of 1 to 20 frames, H = 1 .. 32 and every ratio class); once plain,
    once under the address and undefined-behaviour sanitizers (host code with its own main, run directly); the table it prints
    -- H, nf, the state sizes -- equals the Python restatement and the library's own state size"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "refilter_math_check"
    b = subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "refilter_math_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe), "--table"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "refilter_math_check: ok"
    seen = set()
    for line in lines[:-1]:
        words = line.split()
        if words[0] == "ratio":
            L, M, Z, H = (int(w) for w in words[1:5])
            assert H == rf.half(L, M, Z) == ops.refilter_half(L, M, Z)
            assert [int(c) for c in words[6:]] == [rf.nf(n, L, M, H) for n in range(61)], (L, M, Z)
            seen.add((L, M))
        else:
            J, mh, row_bytes, state_bytes = (int(w) for w in words[1:])
            d = capi.FramesDims(64, J, 20, 7, 0)
            assert capi.api().zeggs_live_refilter_state_bytes(d, mh) == state_bytes == (3 * J * 4 + 7) // 8 * 8 + 64 * row_bytes
            assert row_bytes == 120 + (4 + 8 * J) * 4 + 2 * mh * (7 + 9 * J) * 4
            seen.add((J, mh, "state"))
    assert set(rf.RATIOS) <= seen and {(75, 16, "state"), (1, 4, "state")} <= seen


# ----------------------------------------------------------------------------- 6. the seventh header against capi.RF_*
@pytest.fixture
def seventh(monkeypatch):
    monkeypatch.setattr(third, "HEADER", HEADER)
    return third


def test_refilter_prototypes_are_the_seventh_header(seventh):
    """capi.RF_PROTOTYPES against include/zeggs_hip_refilter.h: the same names; per function the return kind, the parameter count
    and every parameter's kind; the library exports them all; zeggs_live_refilter_version() is 1 and the other versions are
    what they were; the new source is built"""
    header = seventh._header_prototypes()
    assert set(header) == set(capi.RF_PROTOTYPES) and len(header) == 5
    others = (set(capi.PROTOTYPES) | set(capi.EXT_PROTOTYPES) | set(capi.LOUD_PROTOTYPES) | set(capi.RS_PROTOTYPES) | set(capi.FR_PROTOTYPES) |
              set(capi.RT_PROTOTYPES))
    assert not set(capi.RF_PROTOTYPES) & others
    assert not set(capi.RF_STRUCTS) & (set(capi.STRUCTS) | set(capi.EXT_STRUCTS) | set(capi.LOUD_STRUCTS) | set(capi.RS_STRUCTS) | set(capi.FR_STRUCTS) |
                                       set(capi.RT_STRUCTS))
    assert {b for _, _, ps in header.values() for b, depth in ps if depth == 0} <= set(seventh._SCALARS)       # no struct by value
    for name, (rbase, rdepth, params) in header.items():
        ret, kinds = capi.signature(name)
        want = {("int", 0): ("status", "mask", "int"), ("long", 0): ("long",), ("size_t", 0): ("size_t",), ("char", 1): ("str",)}
        assert ret in want[(rbase, rdepth)], (name, ret)
        assert len(kinds) == len(params), name
        for i, (kind, (base, depth)) in enumerate(zip(kinds, params)):
            where = (name, i, kind, base, depth)
            assert kind in capi.KINDS, where
            if depth == 0:
                assert kind == seventh._SCALARS[base], where
            elif kind == "stream":
                assert (base, depth) == ("void", 1), where
            elif kind == "host*":
                assert depth >= 1, where
            elif base.startswith("Zeggs"):
                assert kind == base + "*" and depth == 1 and base in {**capi.RF_STRUCTS, **capi.FR_STRUCTS}, where
            else:
                assert depth == 1 and kind == seventh._ELEMENTS[base], where
    text = HEADER.read_text()
    assert '#include "zeggs_hip_retime.h"' in text and "zeggs_live_refilter_version() >= 1" in text
    L, api = ops.lib(), capi.api()
    assert L.zeggs_version() == 109 and L.zeggs_live_frames_version() == 1 and L.zeggs_live_retime_version() == 1
    assert L.zeggs_live_refilter_version() == 1 and api.zeggs_live_refilter_version() == 1
    for n in header:
        assert hasattr(L, n), f"libzeggs_hip.so does not export {n}"
        assert getattr(api, n).argtypes is not None and getattr(L, n).argtypes is None
    build = (ROOT / "ubisoft-laforge-zeroeggs_amd" / "csrc" / "build.sh").read_text()
    assert " live_refilter " in build and "../../include/zeggs_hip_refilter.h" in build


def test_refilter_struct_mirror_is_the_seventh_header(seventh):
    structs = seventh._header_structs()
    assert set(structs) == set(capi.RF_STRUCTS) == {"ZeggsRefilterRow"}
    for name, fields in structs.items():
        mirror = capi.RF_STRUCTS[name]._fields_
        assert [f for f, _ in mirror] == [f for f, _, _, _ in fields], name
        for (f, ctype), (_, base, depth, n) in zip(mirror, fields):
            want = ctypes.c_void_p if depth else seventh._CTYPES[base]
            assert ctype is want and n is None, (name, f)
    assert ctypes.sizeof(capi.RefilterRow) == 120 and ops.RefilterRow is capi.RefilterRow
    # the record is ZeggsRetimeRow plus table, half, final: the shared fields sit where they sit there
    for f, _ in capi.RetimeRow._fields_:
        assert getattr(capi.RefilterRow, f).offset == getattr(capi.RetimeRow, f).offset, f
    assert capi.RefilterRow.table.offset == ctypes.sizeof(capi.RetimeRow) and capi.RefilterRow.half.offset == 112


# ----------------------------------------------------------------------------- 7. refusals
J5 = 5


def _dims(rows=4, J=J5, max_frames=20, what=7, order=0):
    return capi.FramesDims(rows, J, max_frames, what, order)


# 24 from 60, H = 10: nf(24) - nf(20) = 6 - 4
GOOD = dict(pose=0x10000, rpos=0x20000, rrot=0x30000, local=0x40000, world=0x50000, bvh=0x60000, pose_ld=6 + 15 * J5, rpos_ld=3, rrot_ld=4,
            row=0, count=4, L=2, M=5, n_in=20, outputs=2, table=0x80000, half=10, final=0)
STATE = ctypes.c_void_p(0x900000)
MAX_HALF = 16


def _recs(*rows):
    arr = (capi.RefilterRow * len(rows))()
    for q, over in zip(arr, rows):
        for k, v in dict(GOOD, **over).items():
            setattr(q, k, v)
    return arr


def test_refilter_state_size():
    """the tables, then per row the plain head's row and the ring of 2 max_half raw frames; refused dims or max_half give 0"""
    api = capi.api()
    assert api.zeggs_live_refilter_state_bytes(_dims(4, 5), 10) == 64 + 4 * (120 + 176 + 20 * 208)
    assert api.zeggs_live_refilter_state_bytes(_dims(64, 75), 16) == 904 + 64 * (120 + 2416 + 32 * 2728)
    assert api.zeggs_live_refilter_state_bytes(_dims(1, 1, 1, 1), 1) == 16 + 120 + 48 + 2 * 64
    for bad, mh, match in ((_dims(0), 4, "0 rows"), (_dims(65), 4, "65 rows"), (_dims(J=0), 4, "0 joints"), (_dims(max_frames=0), 4, "max_frames 0"),
                           (_dims(what=0), 4, "what = 0"), (_dims(order=1 | (0 << 2) | (2 << 4)), 4, "channel order"), (_dims(), 0, "max_half 0"),
                           (_dims(), 33, "max_half 33"), (_dims(), -1, "max_half -1")):
        assert api.zeggs_live_refilter_state_bytes(bad, mh) == 0
        assert match in api.zeggs_last_error().decode(), api.zeggs_last_error().decode()


@pytest.mark.parametrize("what,rows,dev,match", [
    ("a row out of range", [dict(row=4)], None, "record 0: row 4 of 4"),
    ("a row twice", [dict(row=2), dict(row=1), dict(row=2)], 0x7000, "record 2: row 2 twice"),
    ("a negative count", [dict(count=-1)], None, "record 0: negative count -1"),
    ("more input frames than max_frames", [dict(), dict(row=1, count=21)], 0x7000, "record 1: 21 frames, max_frames is 20"),
    ("a negative input counter", [dict(n_in=-1)], None, "record 0: input counter -1"),
    ("an input counter past 2^40", [dict(), dict(row=1, n_in=(1 << 40) + 1)], 0x7000, "record 1: input counter 1099511627777"),
    ("a ratio of 9 / 1", [dict(L=9, M=1)], None, "record 0: ratio 9 / 1 is above 8"),
    ("M = 0", [dict(M=0)], None, "record 0: ratio 2 / 0 \\(1 <= L, M <= 4096\\)"),
    ("a ratio that is not reduced", [dict(L=4, M=10)], None, "record 0: ratio 4 / 10 is not in lowest terms"),
    ("a filtered row with L above 1024", [dict(L=1025, M=1024, half=4)], None, "record 0: a filtered row at ratio 1025 / 1024 \\(L <= 1024 and M <= 4 L\\)"),
    ("a filtered row below a quarter of the rate", [dict(), dict(row=1, L=1, M=5, half=20)], 0x7000, "record 1: a filtered row at ratio 1 / 5"),
    ("a negative half", [dict(half=-1)], None, "record 0: negative half -1"),
    ("a half no Z gives at the ratio", [dict(half=9)], None, "record 0: half 9 is no ceil\\(Z max\\(L, M\\) / L\\) for Z = 1 .. 8 at 2 / 5"),
    ("a half above max_half", [dict(half=18)], None, "record 0: half 18, max_half is 16"),
    ("a NULL table", [dict(table=0)], None, "record 0: NULL or misaligned table"),
    ("a misaligned table", [dict(), dict(row=1, table=0x80004)], 0x7000, "record 1: NULL or misaligned table"),
    ("final = 2", [dict(final=2)], None, "record 0: final = 2 \\(0 or 1\\)"),
    ("the unfiltered count as outputs", [dict(outputs=1)], None, "record 0: 1 outputs disagree with nf\\(24\\) - nf\\(20\\) = 2 at 2 / 5, half 10"),
    ("a running record that claims the tail", [dict(outputs=6)], None, "record 0: 6 outputs disagree with nf\\(24\\) - nf\\(20\\) = 2"),
    # (a final record at 24 inputs brings the stream to n_out(24) = 10 frames: 6 more than nf(20) = 4)
    ("a final record without its tail", [dict(final=1)], None, "record 0: 2 outputs disagree with n_out\\(24\\) - nf\\(20\\) = 6"),
    ("an empty final record without its tail", [dict(count=0, n_in=24, final=1, outputs=0)], None,
     "record 0: 0 outputs disagree with n_out\\(24\\) - nf\\(24\\) = 4"),
    ("an empty final record without a destination", [dict(count=0, n_in=24, final=1, outputs=4, bvh=0)], None, "record 0: NULL or misaligned BVH destination"),
    ("an unfiltered record that claims a tail", [dict(half=0, table=0, final=1, outputs=6)], None,
     "record 0: 6 outputs disagree with n_out\\(24\\) - n_out\\(20\\) = 2 at 2 / 5"),
    ("a NULL pose", [dict(pose=0)], None, "record 0: NULL or misaligned source"),
    ("a pose row that is too short", [dict(pose_ld=6 + 9 * J5 - 1)], None, "record 0: leading dimensions 50, 3, 4"),
    ("a NULL LOCAL destination", [dict(local=0)], None, "record 0: NULL or misaligned LOCAL destination"),
    ("a NULL WORLD destination", [dict(), dict(row=1, world=0)], 0x7000, "record 1: NULL or misaligned WORLD destination"),
    ("a misaligned BVH destination", [dict(bvh=0x60004)], None, "record 0: NULL or misaligned BVH destination"),
    ("two records without a device copy", [dict(), dict(row=1)], None, "must also be in device memory"),
    ("more records than rows", [dict(row=i % 4) for i in range(5)], 0x7000, "5 records for 4 rows"),
])
def test_refilter_refuses_on_the_host(what, rows, dev, match):
    """every refusal comes before the launch (the addresses are never followed, there is no device here), with the record named"""
    d, arr = _dims(), _recs(*rows)
    nbytes = capi.api().zeggs_live_refilter_state_bytes(d, MAX_HALF)
    dev_p = ctypes.cast(ctypes.c_void_p(dev), ctypes.POINTER(capi.RefilterRow)) if dev else None
    with pytest.raises(RuntimeError, match="zeggs_live_frames_refiltered: refilter: .*" + match):
        capi.api().zeggs_live_frames_refiltered(d, MAX_HALF, arr, dev_p, len(rows), STATE, nbytes, None)
    assert ops.lib().zeggs_live_frames_refiltered(ctypes.byref(d), MAX_HALF, arr, ctypes.c_void_p(dev or 0), len(rows), STATE, ctypes.c_size_t(nbytes),
                                                  None) == -1


def test_refilter_entry_points_check_dims_state_tables_and_row():
    api, d = capi.api(), _dims()
    nbytes = api.zeggs_live_refilter_state_bytes(d, MAX_HALF)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    with pytest.raises(RuntimeError, match="state too small"):       # (the unfiltered head's state does not do, nor one of a smaller max_half)
        api.zeggs_live_frames_refiltered(d, MAX_HALF, _recs({}), None, 1, STATE, api.zeggs_live_retime_state_bytes(d), None)
    with pytest.raises(RuntimeError, match="state too small"):
        api.zeggs_live_frames_refiltered(d, MAX_HALF, _recs({}), None, 1, STATE, api.zeggs_live_refilter_state_bytes(d, 10), None)
    with pytest.raises(RuntimeError, match="NULL state"):
        api.zeggs_live_refilter_reset(d, MAX_HALF, None, nbytes, 0, None, None, None, None, 0, None)
    with pytest.raises(RuntimeError, match="misaligned state"):
        api.zeggs_live_frames_refiltered(d, MAX_HALF, _recs({}), None, 1, ctypes.c_void_p(0x900004), nbytes, None)
    with pytest.raises(RuntimeError, match="max_half 40"):
        api.zeggs_live_frames_refiltered(d, 40, _recs({}), None, 1, STATE, 1 << 30, None)
    with pytest.raises(RuntimeError, match="2000 joints"):
        api.zeggs_live_frames_refiltered(_dims(J=2000), MAX_HALF, _recs({}), None, 1, STATE, 1 << 30, None)
    for parents, match in ((ints(0, 0, 1, 2, 3), "parents\\[0\\] = 0"), (ints(-1, 0, 2, 1, 1), "parents\\[2\\] = 2")):
        with pytest.raises(RuntimeError, match="refilter prepare: " + match):
            api.zeggs_live_refilter_prepare(d, MAX_HALF, parents, ints(0, 1, 2, 3, 4), STATE, nbytes, None)
    with pytest.raises(RuntimeError, match="refilter prepare: seq\\[2\\] = 1: seq is no permutation"):
        api.zeggs_live_refilter_prepare(d, MAX_HALF, ints(-1, 0, 0, 1, 2), ints(0, 1, 1, 2, 3), STATE, nbytes, None)
    with pytest.raises(RuntimeError, match="reset: row 4 of 4"):
        api.zeggs_live_refilter_reset(d, MAX_HALF, STATE, nbytes, 4, None, None, None, None, 0, None)
    with pytest.raises(RuntimeError, match="row 1: a placement needs"):
        api.zeggs_live_refilter_reset(d, MAX_HALF, STATE, nbytes, 1, (ctypes.c_float * 3)(), (ctypes.c_float * 4)(1.0), None, (ctypes.c_double * 4)(1.0), 1, None)
    # nothing to do: no launch, no error -- no records, records without a frame that are not final, a final one without a tail
    assert api.zeggs_live_frames_refiltered(d, MAX_HALF, None, None, 0, STATE, nbytes, None) == 0
    idle = _recs(dict(count=0, outputs=0, pose=0, local=0), dict(count=0, outputs=0, row=3, bvh=0, half=0, table=0),
                 dict(count=0, n_in=0, outputs=0, final=1, row=2, pose=0))
    assert api.zeggs_live_frames_refiltered(d, MAX_HALF, idle, None, 3, STATE, nbytes, None) == 0


# ----------------------------------------------------------------------------- 8. LiveServer(retime=dict(filter=...)) and open(filtered=...)
PARENTS = SKELETONS["tree"]
FR = dict(parents=PARENTS)


@pytest.mark.parametrize("kw,match", [
    (dict(retime=dict(filter=True)), "needs frames"),
    (dict(frames=FR, retime=dict(filter="sharp")), "retime filter: .*True or a dict"),
    (dict(frames=FR, retime=dict(filter=dict(zero_crossings=9))), "retime filter: .*zero_crossings 9"),
    (dict(frames=FR, retime=dict(filter=dict(rolloff=0.0))), "retime filter: .*rolloff 0.0"),
    (dict(frames=FR, retime=dict(filter=dict(taps=9))), "retime filter: .*keys"),
    (dict(frames=FR, retime=dict(filter=True, min_rate=12)), "min_rate 12 on a server at 60.0 frames per second is below a quarter of it, 15.0"),
    (dict(frames=FR, retime=dict(filter=True, min_rate=90)), "min_rate 90 is above the server's own 60.0"),
    (dict(frames=FR, retime=dict(filter=True, min_rate=0)), "min_rate: .*not a positive rate"),
    (dict(frames=FR, retime=dict(min_rate=24)), "min_rate 24 sizes the filter's history: it needs filter"),
    (dict(frames=FR, retime=dict(filter=False, min_rate=24)), "min_rate 24 sizes the filter's history"),
])
def test_filter_options_are_checked_at_construction(kw, match):
    """before any weight is looked at"""
    with pytest.raises(ValueError, match=match):
        live.LiveServer(None, None, {}, CONF, 1 / 60.0, **kw)


def test_filter_options_defaults():
    """without `filter` the options are what they were; with it: the checked filter, min_rate (default: the lowest rate that
    keeps H_max <= 16, never below fps / 4) and H_max = ceil(Z fps / min_rate)"""
    fc = live.frames_options(FR)
    assert live.retime_options(True, fc, 60.0) == dict(max_rate=Fraction(60), ratio=(1, 1)) == live.retime_options(dict(filter=None), fc, 60.0)
    assert live.retime_options(dict(filter=False, max_rate=120), fc, 60.0) == dict(max_rate=Fraction(120), ratio=(2, 1))
    got = live.retime_options(dict(filter=True, max_rate=120), fc, 60.0)
    assert got == dict(max_rate=Fraction(120), ratio=(2, 1), filter=rf.DEFAULTS, min_rate=Fraction(15), half_max=16)
    assert live.retime_options(dict(filter={}), fc, 60.0)["filter"] == rf.DEFAULTS
    for filt, min_rate, want in ((dict(zero_crossings=8), None, (30, 16)), (dict(zero_crossings=1), None, (15, 4)), (dict(zero_crossings=2), None, (15, 8)),
                                 (True, 24, (24, 10)), (True, 30, (30, 8)), (True, 60, (60, 4)), (True, (24000, 1001), (Fraction(24000, 1001), 11)),
                                 (dict(zero_crossings=8), 15, (15, 32)), (dict(zero_crossings=3, rolloff=0.9), 25, (25, 8))):
        got = live.retime_options(dict(filter=filt, min_rate=min_rate), fc, 60.0)
        assert (got["min_rate"], got["half_max"]) == want, (filt, min_rate)
    assert live.retime_options(dict(filter=True), fc, 50.0)["min_rate"] == Fraction(25, 2)
    assert set(live.RETIME_DEFAULTS) == {"max_rate", "min_rate", "filter"}


def test_open_checks_filtered_before_it_touches_a_row():
    """on stubs with nothing but what the checks read: filtered=True on a server without the filter stage, a ratio the filter
    does not take and a rate below min_rate each raise ValueError naming both rates; what open() makes of the rest"""
    tables = []

    def stub(conf):
        fr = types.SimpleNamespace(table=lambda L, M: tables.append((L, M)) or dict(half=rf.half(L, M), table="tab"))
        me = types.SimpleNamespace(fs=16000, _loud=None, _fr=fr, fps=60.0, retime_conf=conf)
        me._frame_rate = lambda rate: live.LiveServer._frame_rate(me, rate)
        return me

    def opened(conf, **kw):
        return live.LiveServer.open(stub(conf), None, None, **kw)
    fc = live.frames_options(FR)
    off, plain = None, live.retime_options(dict(max_rate=120), fc, 60.0)
    filt = live.retime_options(dict(max_rate=120, filter=True, min_rate=24), fc, 60.0)
    wide = live.retime_options(dict(max_rate=480, filter=True), fc, 60.0)
    with pytest.raises(ValueError, match="filtered=True at frame_rate 30 .* 60.0 frames per second: the filter stage is off"):
        opened(plain, frame_rate=30, filtered=True)
    with pytest.raises(ValueError, match="filtered=True at frame_rate 60.0 .* 60.0 frames per second: the filter stage is off"):
        opened(off, filtered=True)
    with pytest.raises(ValueError, match="frame_rate 20 .* 60.0 frames per second is below its min_rate 24.0"):
        opened(filt, frame_rate=20)
    with pytest.raises(ValueError, match="frame_rate 12 .* 60.0 frames per second is the ratio 1 / 5: a filtered stream takes L <= 1024 and M <= 4 L"):
        opened(wide, frame_rate=12)
    with pytest.raises(ValueError, match="frame_rate .* 60.0 frames per second is the ratio 2000 / 1001: a filtered stream"):
        opened(wide, frame_rate=(120000, 1001))
    with pytest.raises(ValueError, match="frame_rate 90 .* re-timing is off"):            # the earlier checks come first, as they did
        opened(off, frame_rate=90, filtered=True)
    assert not tables
    of = lambda conf, rate, filtered: live.LiveServer._filter_of(stub(conf), live.LiveServer._frame_rate(stub(conf), rate), rate, filtered)  # noqa: E731
    assert of(off, None, None) is None and of(off, None, False) is None
    assert of(plain, 30, None) == dict(L=1, M=2, n_in=0, n_out=0) == of(plain, 30, False)
    assert of(filt, 24, None) == dict(L=2, M=5, n_in=0, n_out=0, half=10, table="tab")
    assert of(filt, None, None) == dict(L=1, M=1, n_in=0, n_out=0, half=0, table=None) == of(filt, 60, False)
    assert of(filt, None, True) == dict(L=1, M=1, n_in=0, n_out=0, half=4, table="tab")              # the jitter filter
    assert of(filt, 120, None)["half"] == 4 and of(filt, 30, False)["half"] == 0 and of(filt, 20, False)["half"] == 0
    assert of(wide, 12, False) == dict(L=1, M=5, n_in=0, n_out=0, half=0, table=None)                # point sampling takes it
    assert tables == [(2, 5), (1, 1), (2, 1)]


def test_frame_delay_is_the_filters_half():
    rows = {0: types.SimpleNamespace(rt=dict(L=2, M=5, half=10)), 1: types.SimpleNamespace(rt=dict(L=1, M=2, half=0)),
            2: types.SimpleNamespace(rt=dict(L=1, M=2)), 3: types.SimpleNamespace(rt=None)}
    me = types.SimpleNamespace(fps=60.0, _row=lambda sid: (sid, rows[sid]))
    assert live.LiveServer.frame_delay(me, 0) == (10, 10 / 60.0)
    assert live.LiveServer.frame_delay(me, 1) == live.LiveServer.frame_delay(me, 2) == live.LiveServer.frame_delay(me, 3) == (0, 0.0)


def test_live_refilter_refuses_a_half_above_its_ring():
    """ops.LiveRefilter.table on a stub: a ratio whose H is above max_half is refused before anything is uploaded"""
    me = types.SimpleNamespace(tables={}, options=dict(rf.DEFAULTS), max_half=8)
    with pytest.raises(ValueError, match="the ratio 2 / 5 needs 10 input frames to either side, max_half is 8"):
        ops.LiveRefilter.table(me, 2, 5)
    with pytest.raises(ValueError, match="the ratio 1 / 5"):
        ops.LiveRefilter.table(me, 1, 5)
