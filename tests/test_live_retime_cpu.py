"""Host-only parts of LiveServer's re-timing output head: the float64 oracle (tests/live_retime_oracle.py) against the frames
oracle, against analytic motion and against itself, the counting rule, the shared header on the host
(tests/host/retime_math_check.cpp, plain and under sanitizers, and against the Python restatement), include/zeggs_hip_retime.h
against zeggs/capi.py, every refusal that comes before a launch, and the ValueErrors of LiveServer(retime=) and
open(frame_rate=).  No GPU needed -- the library loads on the CPU for host-only calls."""
import ctypes
import shutil
import subprocess
import types
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import live_frames_oracle as fo
import live_retime_oracle as ro
import test_live_loudness_cpu as third
from oracle import anim as oanim
from zeggs import capi, live, ops, synth

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "zeggs_hip_retime.h"
CONF = dict(third.CONF, normalize_loudness=False)
SKELETONS = dict(fo.SKELETONS, rig=list(synth.PARENTS))
# the GPU test's cases (tests/test_gpu_live_retime.py): skeleton, and the seed of fo.inputs(J, 20, seed)
GPU_CASES = {"one": 1, "tree": 1, "rig": 10}


def _seq(name):
    return fo.TREE_SEQ if name == "tree" else ops.frames_seq(SKELETONS[name])


def _oracle(name, L, M, place=None, order="zyx", T=20):
    x = fo.inputs(len(SKELETONS[name]), T, GPU_CASES.get(name, 1))
    return x, ro.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], SKELETONS[name], _seq(name), L, M, place, order)


# ----------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("name", ["one", "tree", "rig"])
def test_oracle_at_one_to_one_is_the_frames_oracle(name):
    """L = M = 1: every output, the signs included, equals live_frames_oracle.frames exactly"""
    for place in (None, fo.PLACE):
        x, o = _oracle(name, 1, 1, place, "xzy")
        want = fo.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], SKELETONS[name], _seq(name), place, "xzy")
        assert o["on"].all() and o["k"].tolist() == list(range(20))
        for key in ("root_pos", "root_rot", "lrot", "lpos", "gpos", "grot", "bvh", "mid_sin"):
            assert np.array_equal(o[key], want[key]), key


@pytest.mark.parametrize("M", [2, 3])
def test_oracle_going_down_is_every_mth_frame(M):
    """1 / 2 and 1 / 3: positions and BVH rows of every second / third frame exactly, quaternions up to their sign"""
    x, o = _oracle("tree", 1, M, fo.PLACE)
    want = fo.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], SKELETONS["tree"], fo.TREE_SEQ, fo.PLACE)
    pick = slice(0, 20, M)
    assert o["on"].all() and o["k"].tolist() == list(range(0, 20, M)) and len(o["k"]) == ro.n_out(20, 1, M)
    for key in ("root_pos", "lpos", "gpos", "bvh"):
        assert np.array_equal(o[key], want[key][pick]), key
    for key in ("root_rot", "lrot", "grot"):
        assert np.array_equal(np.abs(o[key]), np.abs(want[key][pick])), key
        q = o[key].reshape(len(o["k"]), -1, 4)
        assert (q[0, :, 0] >= 0.0).all() and (np.sum(q[1:] * q[:-1], axis=-1) >= 0.0).all(), key


@pytest.mark.parametrize("rate", [24, 90, 120])
def test_oracle_follows_a_constant_turn_about_the_skew_axis(rate):
    """a joint turning about the skew axis by 0.25 rad a frame, and a root turning about it by 0.1 rad a frame, as exact float64
    quaternions in the staging (the two-axis decoding is the frames oracle's business, not re-timing's): at 24, 90 and 120 frames a
    second every output frame is the rotation by the angle at its own time, to 1e-12 -- the shortest arc at constant speed"""
    L, M = ro.ratio(rate)
    T = 27                                                # more than a full turn of the joint
    ang = lambda step, t: fo.q_axis(step * np.asarray(t, np.float64), np.broadcast_to(fo.SKEW, (len(t), 3)))  # noqa: E731
    frames_in = np.arange(T)
    lrot = ang(fo.TURN_STEP, frames_in)[:, None]
    rr = ang(0.1, frames_in)
    zeros = np.zeros((T, 3))
    _, rr_o, lrot_o, _, on, k = ro.retime_locals(zeros, rr, lrot, zeros[:, None], L, M)
    N = ro.n_out(T, L, M)
    times = np.arange(N) * M / L                          # in input frames
    assert len(on) == N and times[-1] <= T - 1 < times[-1] + M / L and (on == (np.arange(N) * M % L == 0)).all()
    for got, want in ((lrot_o[:, 0], ang(fo.TURN_STEP, times)), (rr_o, ang(0.1, times))):
        s = np.where(np.sum(got * want, axis=-1, keepdims=True) < 0.0, -1.0, 1.0)
        assert np.abs(got - s * want).max() <= 1e-12
    # through the whole oracle, two-axis encoding in float64: the same rotation, as far as the decoding's own 1e-10 guard lets it
    xy = fo.oanim.q_mul_vec(lrot, np.array([1.0, 0.0, 0.0])), fo.oanim.q_mul_vec(lrot, np.array([0.0, 1.0, 0.0]))
    o = ro.frames(zeros, rr, zeros[:, None], np.stack(xy, axis=-2), [-1], [0], L, M)
    q = o["lrot"][:, 0] / np.linalg.norm(o["lrot"][:, 0], axis=-1, keepdims=True)
    assert np.abs(np.abs(np.sum(q * ang(fo.TURN_STEP, times), axis=-1)) - 1.0).max() <= 1e-12
    assert (np.sum(o["lrot"][1:, 0] * o["lrot"][:-1, 0], axis=-1) > 0.0).all() and o["lrot"][0, 0, 0] >= 0.0


@pytest.mark.parametrize("ratio", [(2, 5), (3, 2), (2, 1), (500, 1001)])
def test_oracle_keeps_a_straight_line_straight(ratio):
    """root and lpos moving on a straight line at constant speed: every output frame lies on it at its own time (1e-12 of the
    coordinates' size), with and without rotations going on"""
    L, M = ratio
    T, J = 20, 3
    rng = np.random.default_rng(3)
    t = np.arange(T)[:, None]
    rp = rng.standard_normal(3) * 10.0 + t * rng.standard_normal(3)
    lp = rng.standard_normal((J, 3)) * 5.0 + t[:, None] * rng.standard_normal((J, 3)) * 0.1
    rr, lrot = fo.smooth(T, 1, rng)[:, 0], fo.smooth(T, J, rng)
    rp_o, _, _, lp_o, _, _ = ro.retime_locals(rp, rr, lrot, lp, L, M)
    times = (np.arange(ro.n_out(T, L, M)) * M / L)[:, None]
    assert np.abs(rp_o - (rp[0] + times * (rp[1] - rp[0]))).max() <= 1e-12 * 30.0
    assert np.abs(lp_o - (lp[0] + times[:, None] * (lp[1] - lp[0]))).max() <= 1e-12 * 30.0


def test_oracle_between_frames_is_the_head_on_interpolated_locals():
    """a frame between two inputs: unit local quaternions on the shorter arc between the neighbours' (either sign of the far end),
    a child's world position its parent's transform applied to the interpolated local position, signs continuous over the OUTPUT
    sequence and w >= 0 on output 0"""
    x, o = _oracle("tree", 3, 2, fo.PLACE)
    full = fo.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], SKELETONS["tree"], fo.TREE_SEQ, fo.PLACE)
    N = ro.n_out(20, 3, 2)
    assert len(o["on"]) == N == 29 and o["on"].tolist() == [m % 3 == 0 for m in range(N)]
    mid = ~o["on"]
    a, b = full["raw"]["lrot"][o["k"][mid]], full["raw"]["lrot"][o["k"][mid] + 1]
    q = o["raw"]["lrot"][mid]
    assert np.abs(np.linalg.norm(q, axis=-1) - 1.0).max() < 1e-15
    da, db, dab = (np.abs(np.sum(u * v, axis=-1)) for u, v in ((q, a), (q, b), (a, b)))
    assert (da >= dab - 1e-12).all() and (db >= dab - 1e-12).all()          # between the two, on the short side
    p = SKELETONS["tree"][3]
    assert np.abs(o["gpos"][:, 3] - (oanim.q_mul_vec(o["grot"][:, p], o["lpos"][:, 3]) + o["gpos"][:, p])).max() < 1e-9
    for key in ("root_rot", "lrot", "grot"):
        u = o[key].reshape(N, -1, 4)
        assert (u[0, :, 0] >= 0.0).all() and (np.sum(u[1:] * u[:-1], axis=-1) > 0.0).all(), key


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_oracle_alone_meets_the_gpu_tests_conditions(name):
    """for the seeds and ratios of tests/test_gpu_live_retime.py the oracle alone leaves at most 5 % of a case's output frames out
    by the Euler rule (|sin| of the middle angle <= 0.999), in both channel orders, with and without the placement"""
    for L, M in ro.RATIOS:
        for order in ("zyx", "xzy"):
            for place in (None, fo.PLACE):
                _, o = _oracle(name, L, M, place, order)
                assert len(o["on"]) == ro.n_out(20, L, M)
                assert ro.left_out(o) <= 0.05, (name, L, M, order, place is not None, ro.left_out(o))


# ----------------------------------------------------------------------------- 2. the counting rule
def test_rates_reduce_to_the_documented_ratios():
    for rate, want in ro.RATES.items():
        assert ro.ratio(rate) == want and ops.retime_ratio(rate, 60.0) == want and ops.retime_ratio(rate, 60) == want, rate
        assert capi.api().zeggs_live_retime_version() == 1
    assert ops.retime_ratio(29.97, 60.0) == (999, 2000) and ops.retime_ratio((30000, 1001), 60.0) == (500, 1001)
    assert ops.retime_ratio(Fraction(24000, 1001), 60.0) == (400, 1001) and ops.retime_ratio(np.float32(30.0), 60.0) == (1, 2)
    assert ops.retime_ratio(25, 50) == (1, 2) and ops.retime_ratio(60, 60.0) == (1, 1)
    for bad, match in ((540, "9 / 1"), (60 * Fraction(4097, 4096), "4097 / 4096"), (Fraction(60, 4097), "1 / 4097"), (0, "not a positive rate"),
                       (-30, "not a positive rate"), (float("nan"), "not a positive rate"), ("fast", "not a positive rate"),
                       (True, "not a positive rate"), ((30, 0), "not a positive rate")):
        with pytest.raises(ValueError, match=match) as e:
            ops.retime_ratio(bad, 60.0)
        assert "60.0" in str(e.value)                      # both rates are named
    for bad in (540, Fraction(60, 4097), 0):
        with pytest.raises(ValueError):
            ro.ratio(bad)


@pytest.mark.parametrize("ratio", ro.RATIOS + ((1000, 1001), (4096, 4095), (1, 4096)))
def test_counting_rule(ratio):
    """n_out is monotone from n_out(1) = 1; the counts of any cut add up to n_out(n); the last frame emitted needs no input >= n and
    the next one does; ops.retime_* are the same rule"""
    L, M = ratio
    rng = np.random.default_rng(L * 5000 + M)
    assert ro.n_out(0, L, M) == 0 and ro.n_out(1, L, M) == 1
    counts = [ro.n_out(n, L, M) for n in range(400)]
    assert all(b >= a for a, b in zip(counts, counts[1:]))
    for n in range(1, 400):
        N = counts[n]
        assert ro.last_needed(N - 1, L, M) <= n - 1 < ro.last_needed(N, L, M), n
        assert ops.retime_n_out(n, L, M) == N and ops.retime_position(N, L, M) == ro.position(N, L, M)
    for _ in range(20):
        cuts, n, total = rng.integers(0, 22, 30).tolist(), 0, 0
        for c in cuts:
            got = ro.n_out(n + c, L, M) - ro.n_out(n, L, M)
            assert 0 <= got <= ops.retime_max_outputs(c, L, M)
            n, total = n + c, total + got
        assert total == ro.n_out(n, L, M)


# ----------------------------------------------------------------------------- 3. csrc/retime_math.h on the host
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_retime_rules_on_the_host(tmp_path, flags):
    """tests/host/retime_math_check.cpp: a stand-alone program over the header the kernel uses (its head says what it walks); once
    plain, once under the address and undefined-behaviour sanitizers (host code with its own main, run directly); the table it
    prints -- n_out, the positions, the bound on a record's outputs, the state and LDS sizes -- equals the Python restatement"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "retime_math_check"
    b = subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "retime_math_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe), "--table"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "retime_math_check: ok"
    seen = set()
    for line in lines[:-1]:
        words = line.split()
        if words[0] == "ratio":
            L, M = int(words[1]), int(words[2])
            counts, where, most = (part.split() for part in " ".join(words[3:]).split("|"))
            assert [int(c) for c in counts] == [ro.n_out(n, L, M) for n in range(46)], (L, M)
            assert [tuple(int(v) for v in w.split(":")) for w in where] == [ro.position(m, L, M) for m in range(31)], (L, M)
            assert int(most[0]) == ops.retime_max_outputs(20, L, M)
            seen.add((L, M))
        else:
            J, row_bytes, state_bytes, pass_frames, lds = (int(w) for w in words[1:])
            d = capi.FramesDims(64, J, 20, 7, 0)
            assert capi.api().zeggs_live_retime_state_bytes(d) == state_bytes == (3 * J * 4 + 7) // 8 * 8 + 64 * row_bytes
            assert row_bytes == 120 + (4 + 8 * J) * 4 + ((7 + 9 * J) * 4 + 7) // 8 * 8
            assert pass_frames == min(65536 // (56 * (J + 1)), 161) and lds == pass_frames * 56 * (J + 1)
            seen.add(J)
    assert set(ro.RATIOS) <= seen and {1, 5, 75} <= seen


# ----------------------------------------------------------------------------- 4. the sixth header against capi.RT_*
@pytest.fixture
def sixth(monkeypatch):
    monkeypatch.setattr(third, "HEADER", HEADER)
    return third


def test_retime_prototypes_are_the_sixth_header(sixth):
    """capi.RT_PROTOTYPES against include/zeggs_hip_retime.h: the same names; per function the return kind, the parameter count and
    every parameter's kind; the library exports them all; zeggs_live_retime_version() is 1, zeggs_version() still 109 and
    zeggs_live_frames_version() still 1; the new source is built, in front of live_resample"""
    header = sixth._header_prototypes()
    assert set(header) == set(capi.RT_PROTOTYPES) and len(header) == 5
    others = (set(capi.PROTOTYPES) | set(capi.EXT_PROTOTYPES) | set(capi.LOUD_PROTOTYPES) | set(capi.RS_PROTOTYPES) | set(capi.FR_PROTOTYPES))
    assert not set(capi.RT_PROTOTYPES) & others
    assert not set(capi.RT_STRUCTS) & (set(capi.STRUCTS) | set(capi.EXT_STRUCTS) | set(capi.LOUD_STRUCTS) | set(capi.RS_STRUCTS) | set(capi.FR_STRUCTS))
    assert {b for _, _, ps in header.values() for b, depth in ps if depth == 0} <= set(sixth._SCALARS)       # no struct by value
    for name, (rbase, rdepth, params) in header.items():
        ret, kinds = capi.signature(name)
        want = {("int", 0): ("status", "mask", "int"), ("long", 0): ("long",), ("size_t", 0): ("size_t",), ("char", 1): ("str",)}
        assert ret in want[(rbase, rdepth)], (name, ret)
        assert len(kinds) == len(params), name
        for i, (kind, (base, depth)) in enumerate(zip(kinds, params)):
            where = (name, i, kind, base, depth)
            assert kind in capi.KINDS, where
            if depth == 0:
                assert kind == sixth._SCALARS[base], where
            elif kind == "stream":
                assert (base, depth) == ("void", 1), where
            elif kind == "host*":
                assert depth >= 1, where
            elif base.startswith("Zeggs"):
                assert kind == base + "*" and depth == 1 and base in {**capi.RT_STRUCTS, **capi.FR_STRUCTS}, where
            else:
                assert depth == 1 and kind == sixth._ELEMENTS[base], where
    text = HEADER.read_text()
    assert '#include "zeggs_hip_frames.h"' in text and "zeggs_live_retime_version() >= 1" in text
    L, api = ops.lib(), capi.api()
    assert L.zeggs_version() == 109 and L.zeggs_live_frames_version() == 1
    assert L.zeggs_live_retime_version() == 1 and api.zeggs_live_retime_version() == 1
    for n in header:
        assert hasattr(L, n), f"libzeggs_hip.so does not export {n}"
        assert getattr(api, n).argtypes is not None and getattr(L, n).argtypes is None
    build = (ROOT / "ubisoft-laforge-zeroeggs_amd" / "csrc" / "build.sh").read_text()
    assert " live_frames live_retime live_resample\"" in build and "../../include/zeggs_hip_retime.h" in build


def test_retime_struct_mirror_is_the_sixth_header(sixth):
    structs = sixth._header_structs()
    assert set(structs) == set(capi.RT_STRUCTS) == {"ZeggsRetimeRow"}
    for name, fields in structs.items():
        mirror = capi.RT_STRUCTS[name]._fields_
        assert [f for f, _ in mirror] == [f for f, _, _, _ in fields], name
        for (f, ctype), (_, base, depth, n) in zip(mirror, fields):
            want = ctypes.c_void_p if depth else sixth._CTYPES[base]
            assert ctype is want and n is None, (name, f)
    assert ctypes.sizeof(capi.RetimeRow) == 104 and ops.RetimeRow is capi.RetimeRow
    # the fields it shares with the fifth header's record sit where they sit there
    for f in ("pose", "rpos", "rrot", "local", "world", "bvh", "pose_ld", "rpos_ld", "rrot_ld"):
        assert getattr(capi.RetimeRow, f).offset == getattr(capi.FramesRow, f).offset, f


# ----------------------------------------------------------------------------- 5. refusals
J5 = 5


def _dims(rows=4, J=J5, max_frames=20, what=7, order=0):
    return capi.FramesDims(rows, J, max_frames, what, order)


GOOD = dict(pose=0x10000, rpos=0x20000, rrot=0x30000, local=0x40000, world=0x50000, bvh=0x60000, pose_ld=6 + 15 * J5, rpos_ld=3, rrot_ld=4,
            row=0, count=4, L=3, M=2, n_in=10, outputs=6)       # n_out(14) - n_out(10) at 3 / 2: 20 - 14
STATE = ctypes.c_void_p(0x900000)


def _recs(*rows):
    arr = (capi.RetimeRow * len(rows))()
    for q, over in zip(arr, rows):
        for k, v in dict(GOOD, **over).items():
            setattr(q, k, v)
    return arr


def test_retime_state_size():
    """the tables, then per row the plain head's row and the raw frame (7 + 9J floats, padded to 8 bytes); refused dims give 0"""
    api = capi.api()
    assert api.zeggs_live_retime_state_bytes(_dims(4, 5)) == 64 + 4 * (120 + 176 + 208)
    assert api.zeggs_live_retime_state_bytes(_dims(64, 75)) == 904 + 64 * (120 + 2416 + 2728)
    assert api.zeggs_live_retime_state_bytes(_dims(1, 1, 1, 1)) == 16 + 120 + 48 + 64
    for d in (_dims(4, 5), _dims(64, 75)):
        assert api.zeggs_live_retime_state_bytes(d) > api.zeggs_live_frames_state_bytes(d)
    for bad, match in ((_dims(0), "0 rows"), (_dims(65), "65 rows"), (_dims(J=0), "0 joints"), (_dims(J=1025), "1025 joints"),
                       (_dims(max_frames=0), "max_frames 0"), (_dims(max_frames=4097), "max_frames 4097"), (_dims(what=0), "what = 0"),
                       (_dims(what=8), "what = 8"), (_dims(order=1 | (0 << 2) | (2 << 4)), "channel order")):
        assert api.zeggs_live_retime_state_bytes(bad) == 0
        assert match in api.zeggs_last_error().decode(), api.zeggs_last_error().decode()


@pytest.mark.parametrize("what,rows,dev,match", [
    ("a row out of range", [dict(row=4)], None, "record 0: row 4 of 4"),
    ("a row twice", [dict(row=2), dict(row=1), dict(row=2)], 0x7000, "record 2: row 2 twice"),
    ("a negative count", [dict(count=-1)], None, "record 0: negative count -1"),
    ("more input frames than max_frames", [dict(), dict(row=1, count=21)], 0x7000, "record 1: 21 frames, max_frames is 20"),
    ("a negative input counter", [dict(n_in=-1)], None, "record 0: input counter -1"),
    ("an input counter past 2^40", [dict(), dict(row=1, n_in=(1 << 40) + 1)], 0x7000, "record 1: input counter 1099511627777"),
    # (at 1 / 2 three inputs after 10 emit 2 frames, after 9 only 1)
    ("a counter that is one behind", [dict(L=1, M=2, count=3, n_in=9, outputs=2)], None,
     "record 0: 2 outputs disagree with n_out\\(12\\) - n_out\\(9\\) = 1 at 1 / 2"),
    ("one output too many", [dict(), dict(row=1, outputs=7)], 0x7000, "record 1: 7 outputs disagree with n_out\\(14\\) - n_out\\(10\\) = 6"),
    ("no output where the rule gives some", [dict(outputs=0)], None, "record 0: 0 outputs disagree"),
    ("outputs of a record without input", [dict(count=0, outputs=1)], None, "record 0: 1 outputs disagree with n_out\\(10\\) - n_out\\(10\\) = 0"),
    ("the plain head's count as outputs at 1 / 2", [dict(L=1, M=2, outputs=4)], None, "record 0: 4 outputs disagree .* = 2 at 1 / 2"),
    ("a ratio of 9 / 1", [dict(L=9, M=1)], None, "record 0: ratio 9 / 1 is above 8"),
    ("L = 4097", [dict(), dict(row=2, L=4097, M=4096)], 0x7000, "record 1: ratio 4097 / 4096 \\(1 <= L, M <= 4096\\)"),
    ("M = 0", [dict(M=0)], None, "record 0: ratio 3 / 0 \\(1 <= L, M <= 4096\\)"),
    ("a ratio that is not reduced", [dict(L=6, M=4)], None, "record 0: ratio 6 / 4 is not in lowest terms"),
    ("a NULL pose", [dict(pose=0)], None, "record 0: NULL or misaligned source"),
    ("a misaligned root rotation", [dict(), dict(row=3, rrot=0x30002)], 0x7000, "record 1: NULL or misaligned source"),
    ("a pose row that is too short", [dict(pose_ld=6 + 9 * J5 - 1)], None, "record 0: leading dimensions 50, 3, 4"),
    ("a NULL LOCAL destination", [dict(local=0)], None, "record 0: NULL or misaligned LOCAL destination"),
    ("a NULL WORLD destination", [dict(), dict(row=1, world=0)], 0x7000, "record 1: NULL or misaligned WORLD destination"),
    ("a NULL BVH destination", [dict(bvh=0)], None, "record 0: NULL or misaligned BVH destination"),
    ("a misaligned BVH destination", [dict(bvh=0x60004)], None, "record 0: NULL or misaligned BVH destination"),
    ("a misaligned LOCAL destination", [dict(local=0x40002)], None, "record 0: NULL or misaligned LOCAL destination"),
    ("two records without a device copy", [dict(), dict(row=1)], None, "must also be in device memory"),
    ("more records than rows", [dict(row=i % 4) for i in range(5)], 0x7000, "5 records for 4 rows"),
])
def test_retime_refuses_on_the_host(what, rows, dev, match):
    """every refusal comes before the launch (the addresses are never followed, there is no device here), with the record named"""
    d, arr = _dims(), _recs(*rows)
    nbytes = capi.api().zeggs_live_retime_state_bytes(d)
    dev_p = ctypes.cast(ctypes.c_void_p(dev), ctypes.POINTER(capi.RetimeRow)) if dev else None
    with pytest.raises(RuntimeError, match="zeggs_live_frames_retimed: retime: .*" + match):
        capi.api().zeggs_live_frames_retimed(d, arr, dev_p, len(rows), STATE, nbytes, None)
    assert ops.lib().zeggs_live_frames_retimed(ctypes.byref(d), arr, ctypes.c_void_p(dev or 0), len(rows), STATE, ctypes.c_size_t(nbytes), None) == -1


def test_retime_entry_points_check_dims_state_tables_and_row():
    api, d = capi.api(), _dims()
    nbytes = api.zeggs_live_retime_state_bytes(d)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    with pytest.raises(RuntimeError, match="state too small"):       # (the plain head's state does not do)
        api.zeggs_live_frames_retimed(d, _recs({}), None, 1, STATE, api.zeggs_live_frames_state_bytes(d), None)
    with pytest.raises(RuntimeError, match="NULL state"):
        api.zeggs_live_retime_reset(d, None, nbytes, 0, None, None, None, None, 0, None)
    with pytest.raises(RuntimeError, match="misaligned state"):
        api.zeggs_live_frames_retimed(d, _recs({}), None, 1, ctypes.c_void_p(0x900004), nbytes, None)
    with pytest.raises(RuntimeError, match="2000 joints"):
        api.zeggs_live_frames_retimed(_dims(J=2000), _recs({}), None, 1, STATE, 1 << 30, None)
    # a bit that is off: its destination is not looked at; a record that emits nothing needs no destination at all
    with pytest.raises(RuntimeError, match="record 0: NULL or misaligned BVH destination"):
        api.zeggs_live_frames_retimed(_dims(what=4), _recs(dict(local=0, world=0, bvh=0)), None, 1, STATE, nbytes, None)
    for parents, match in ((ints(0, 0, 1, 2, 3), "parents\\[0\\] = 0"), (ints(-1, 0, 2, 1, 1), "parents\\[2\\] = 2")):
        with pytest.raises(RuntimeError, match="retime prepare: " + match):
            api.zeggs_live_retime_prepare(d, parents, ints(0, 1, 2, 3, 4), STATE, nbytes, None)
    with pytest.raises(RuntimeError, match="retime prepare: seq\\[2\\] = 1: seq is no permutation"):
        api.zeggs_live_retime_prepare(d, ints(-1, 0, 0, 1, 2), ints(0, 1, 1, 2, 3), STATE, nbytes, None)
    with pytest.raises(RuntimeError, match="reset: row 4 of 4"):
        api.zeggs_live_retime_reset(d, STATE, nbytes, 4, None, None, None, None, 0, None)
    with pytest.raises(RuntimeError, match="row 1: a placement needs"):
        api.zeggs_live_retime_reset(d, STATE, nbytes, 1, (ctypes.c_float * 3)(), (ctypes.c_float * 4)(1.0), None, (ctypes.c_double * 4)(1.0), 1, None)
    # nothing to do: no launch, no error
    assert api.zeggs_live_frames_retimed(d, None, None, 0, STATE, nbytes, None) == 0
    assert api.zeggs_live_frames_retimed(d, _recs(dict(count=0, outputs=0, pose=0, local=0), dict(count=0, outputs=0, row=3, bvh=0)), None, 2,
                                         STATE, nbytes, None) == 0


# ----------------------------------------------------------------------------- 6. LiveServer(retime=...) and open(frame_rate=...)
PARENTS = SKELETONS["tree"]


@pytest.mark.parametrize("kw,match", [
    (dict(retime=True), "needs frames"), (dict(retime=dict(max_rate=120)), "needs frames"), (dict(retime={}), "needs frames"),
    (dict(frames=dict(parents=PARENTS), retime="fast"), "None, True or a dict"), (dict(frames=dict(parents=PARENTS), retime=dict(rate=120)), "keys"),
    (dict(frames=dict(parents=PARENTS), retime=dict(max_rate=540)), "max_rate.*540.*60.0.*9 / 1"),
    (dict(frames=dict(parents=PARENTS), retime=dict(max_rate=30)), "max_rate 30 is below the server's own 60.0"),
    (dict(frames=dict(parents=PARENTS), retime=dict(max_rate=0)), "max_rate.*not a positive rate"),
])
def test_retime_options_are_checked_at_construction(kw, match):
    """before any weight is looked at"""
    with pytest.raises(ValueError, match=match):
        live.LiveServer(None, None, {}, CONF, 1 / 60.0, **kw)


def test_retime_options_defaults():
    fc = live.frames_options(dict(parents=PARENTS))
    assert live.retime_options(None, fc, 60.0) is None and live.retime_options(None, None, 60.0) is None
    assert live.retime_options(True, fc, 60.0) == dict(max_rate=Fraction(60), ratio=(1, 1)) == live.retime_options({}, fc, 60.0)
    assert live.retime_options(dict(max_rate=120), fc, 60.0) == dict(max_rate=Fraction(120), ratio=(2, 1))
    assert live.retime_options(dict(max_rate=(120000, 1001)), fc, 60.0)["ratio"] == (2000, 1001)
    assert set(live.FRAMES_DEFAULTS) == {"parents", "names", "what", "order", "text"}       # `retime` is an argument of its own


def test_open_checks_the_frame_rate_before_it_touches_a_row():
    """on stubs with nothing but what the checks read: a frame rate on a server without re-timing, a ratio the kernel does not
    take and a rate above max_rate each raise ValueError naming both rates; open()'s earlier checks still come first"""
    stub = lambda conf: types.SimpleNamespace(fs=16000, _loud=None, _fr=object(), fps=60.0, retime_conf=conf,  # noqa: E731
                                              _frame_rate=lambda fr: live.LiveServer._frame_rate(stub_now[0], fr))
    stub_now = [None]

    def opened(conf, **kw):
        stub_now[0] = stub(conf)
        return live.LiveServer.open(stub_now[0], None, None, **kw)
    fc = live.frames_options(dict(parents=PARENTS))
    off, same, up = None, live.retime_options(True, fc, 60.0), live.retime_options(dict(max_rate=120), fc, 60.0)
    with pytest.raises(ValueError, match="frame_rate 30 .* 60.0 frames per second: re-timing is off"):
        opened(off, frame_rate=30)
    with pytest.raises(ValueError, match="frame rate 540 .* 60.0 .* 9 / 1"):
        opened(up, frame_rate=540)
    with pytest.raises(ValueError, match="frame rate .* 60.0 .* 1 / 4097"):
        opened(up, frame_rate=Fraction(60, 4097))
    with pytest.raises(ValueError, match="frame rate -24 .* 60.0 .*not a positive rate"):
        opened(up, frame_rate=-24)
    with pytest.raises(ValueError, match="frame_rate 90 .* 60.0 frames per second is above its max_rate 60.0"):
        opened(same, frame_rate=90)
    with pytest.raises(ValueError, match="frame_rate 240 .* 60.0 frames per second is above its max_rate 120.0"):
        opened(up, frame_rate=240)
    with pytest.raises(ValueError, match="both or neither"):              # the placement's check comes first, as it did
        opened(off, frame_rate=30, start_position=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="a gain needs running loudness"):
        opened(off, frame_rate=30, gain=2.0)
    # what open() makes of a rate it takes
    stub_now[0] = stub(up)
    assert live.LiveServer._frame_rate(stub_now[0], None) == dict(L=1, M=1, n_in=0, n_out=0)
    assert live.LiveServer._frame_rate(stub_now[0], 90) == dict(L=3, M=2, n_in=0, n_out=0)
    assert live.LiveServer._frame_rate(stub_now[0], (30000, 1001))["M"] == 1001 and live.LiveServer._frame_rate(stub(off), None) is None


def test_frames_cat_keeps_the_first_frame0():
    parts = [dict(bvh=np.zeros((2, 6)), text=b"ab", frame0=7), dict(bvh=np.zeros((0, 6)), text=b"", frame0=9), dict(bvh=np.ones((1, 6)), text=b"c", frame0=9)]
    got = live.frames_cat(parts)
    assert got["frame0"] == 7 and got["text"] == b"abc" and got["bvh"].shape == (3, 6)
