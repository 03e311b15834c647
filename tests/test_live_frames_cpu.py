"""Host-only parts of LiveServer's output head: the float64 oracle (tests/live_frames_oracle.py) against itself and against
oracle/anim.py, the shared layout header on the host (tests/host/frames_math_check.cpp, plain and under sanitizers),
include/zeggs_hip_frames.h against zeggs/capi.py, every refusal that comes before a launch, and the ValueErrors of LiveServer and
open().  No GPU needed -- the library loads on the CPU for host-only calls."""
import ctypes
import re
import shutil
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

import live_frames_oracle as fo
import test_live_loudness_cpu as third
from oracle import anim as oanim
from zeggs import capi, live, ops, synth

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "zeggs_hip_frames.h"
CONF = dict(third.CONF, normalize_loudness=False)
SKELETONS = dict(fo.SKELETONS, rig=list(synth.PARENTS))


def _seq(name):
    return fo.TREE_SEQ if name == "tree" else ops.frames_seq(SKELETONS[name])


# ----------------------------------------------------------------------------- 1. the oracle against itself
def test_bvh_seq_is_the_headers_joint_order():
    from zeggs import anim
    for name, parents in SKELETONS.items():
        assert ops.frames_seq(parents) == anim.bvh_header(np.zeros((len(parents), 3)), parents)[1], name
    assert ops.frames_seq(SKELETONS["tree"]) == fo.TREE_SEQ != list(range(5))
    for bad in ([], [0, 0], [-1, 1], [-1, 0, 2], [-1, -1]):
        with pytest.raises(ValueError, match="parents"):
            ops.frames_seq(bad)


@pytest.mark.parametrize("name", list(SKELETONS))
@pytest.mark.parametrize("order", ["zyx", "xzy"])
def test_oracle_bvh_rows_are_bvh_channels_in_file_order(name, order):
    """the BVH rows equal oracle.anim.bvh_channels reordered by seq, with and without the placement"""
    parents, seq = SKELETONS[name], _seq(name)
    x = fo.inputs(len(parents), 20, fo.seed_for(name, 20))
    for place in (None, fo.PLACE):
        o = fo.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], parents, seq, place, order)
        pos, eul = oanim.bvh_channels(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], *(place or (None, None)), order=order)
        assert o["bvh"].shape == (20, 3 + 3 * len(parents)) and o["bvh"].dtype == np.float64
        assert np.array_equal(o["bvh"][:, :3], pos[:, 0])
        for k, j in enumerate(seq):
            assert np.array_equal(o["bvh"][:, 3 + 3 * k:6 + 3 * k], eul[:, j])
        # the conditions the GPU test states for its inputs hold on the oracle alone
        dot, w0 = fo.sign_margins(o)
        assert dot > 1e-3 and w0 > 1e-3 and (np.abs(o["mid_sin"]) <= 0.999).all()


def test_oracle_world_of_one_joint_is_the_placed_root_composed_with_local():
    x = fo.inputs(1, 20, 3)
    for place in (None, fo.PLACE):
        o = fo.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], [-1], [0], place)
        want_q = oanim.q_mul(o["raw"]["root_rot"], o["raw"]["lrot"][:, 0])
        want_p = oanim.q_mul_vec(o["raw"]["root_rot"], o["lpos"][:, 0]) + o["root_pos"]
        assert np.array_equal(o["gpos"][:, 0], want_p)
        assert np.array_equal(np.abs(o["grot"][:, 0]), np.abs(want_q)) and np.array_equal(o["grot"][:, 0], fo.unroll(want_q))
        assert np.abs(np.linalg.norm(o["grot"], axis=-1) - 1.0).max() < 1e-6      # (the root quaternion is a float32 one)
    # without a placement the root is the input's, with one frame 0 stands where it was put
    assert np.array_equal(fo.placed_root(x["rpos"], x["rrot"])[0], x["rpos"].astype(np.float64))
    rp, rr = fo.placed_root(x["rpos"], x["rrot"], fo.PLACE)
    assert np.abs(rp[0] - fo.PLACE[0]).max() < 1e-12 and np.abs(np.abs(rr[0]) - np.abs(fo.PLACE[1])).max() < 1e-6


def test_oracle_world_is_fk_and_signs_are_continuous():
    parents = SKELETONS["rig"]
    x = fo.inputs(75, 20, fo.seed_for("rig", 20))
    o = fo.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], parents, _seq("rig"), fo.PLACE)
    for key in ("root_rot", "lrot", "grot"):
        q = o[key].reshape(20, -1, 4)
        assert (q[0, :, 0] >= 0.0).all() and (np.sum(q[1:] * q[:-1], axis=-1) > 0.0).all(), key
        assert np.array_equal(np.abs(q), np.abs(o["raw"][key].reshape(20, -1, 4)))
    # a child's world position: its parent's transform applied to its local position
    j, p = 40, parents[40]
    assert np.abs(o["gpos"][:, j] - (oanim.q_mul_vec(o["grot"][:, p], o["lpos"][:, j]) + o["gpos"][:, p])).max() < 1e-9


def test_full_turns_flip_the_raw_sign_once_per_turn():
    """the sign-rule inputs: full turns about x, y, z and a skew axis in steps of 0.25 rad, through the two-axis encoding with
    its scaled, skewed second axis: exactly one raw sign flip per turn, |dot| >= 0.99 between neighbours (0.9922 = cos(0.125))"""
    for axis in fo.TURN_AXES:
        q = oanim.q_from_xform(oanim.xform_from_xy(fo.xy_of(fo.full_turn(27, axis)).astype(np.float64)))
        flips, dot = fo.raw_flips(q)
        print(f"axis {np.round(axis, 3)}: {flips} flip, min |dot| {dot:.4f}")
        assert flips == 1 and 0.99 <= dot < 0.9923
        u = fo.unroll(q)
        assert fo.raw_flips(u)[0] == 0 and u[0, 0] >= 0.0
    x = fo.inputs(5, 20, 1)
    o = fo.frames(x["rpos"], x["rrot"], x["lpos"], x["ltxy"], SKELETONS["chain"], list(range(5)))
    assert [fo.raw_flips(o["raw"]["lrot"][:, j])[0] for j in (1, 2, 3, 4)] == [1, 1, 1, 1]      # the turns complete inside the record


# ----------------------------------------------------------------------------- 2. csrc/frames_math.h on the host
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_frames_layout_rules_on_the_host(tmp_path, flags):
    """tests/host/frames_math_check.cpp: a stand-alone program over the header the kernel uses (its head says what it walks);
    once plain, once under the address and undefined-behaviour sanitizers (host code with its own main, run directly)"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "frames_math_check"
    b = subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "frames_math_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "frames_math_check: ok"


# ----------------------------------------------------------------------------- 3. the fifth header against capi.FR_*
# (the parser of tests/test_live_loudness_cpu.py, pointed at the fifth header)
@pytest.fixture
def fifth(monkeypatch):
    monkeypatch.setattr(third, "HEADER", HEADER)
    return third


def test_frames_prototypes_are_the_fifth_header(fifth):
    """capi.FR_PROTOTYPES against include/zeggs_hip_frames.h: the same names; per function the return kind, the parameter count,
    every parameter's kind and every device pointer's element type; the library exports them all, zeggs_version() is still 109,
    zeggs_live_resample_version() 1 and zeggs_live_frames_version() 1; the tables of the other four headers are the size they were"""
    header = fifth._header_prototypes()
    assert set(header) == set(capi.FR_PROTOTYPES) and len(header) == 5
    assert (len(capi.PROTOTYPES), len(capi.STRUCTS), len(capi.EXT_PROTOTYPES), len(capi.EXT_STRUCTS)) == (122, 21, 6, 2)
    assert (len(capi.LOUD_PROTOTYPES), len(capi.LOUD_STRUCTS), len(capi.RS_PROTOTYPES), len(capi.RS_STRUCTS)) == (5, 2, 6, 2)
    others = set(capi.PROTOTYPES) | set(capi.EXT_PROTOTYPES) | set(capi.LOUD_PROTOTYPES) | set(capi.RS_PROTOTYPES)
    assert not set(capi.FR_PROTOTYPES) & others
    assert not set(capi.FR_STRUCTS) & (set(capi.STRUCTS) | set(capi.EXT_STRUCTS) | set(capi.LOUD_STRUCTS) | set(capi.RS_STRUCTS))
    assert {b for _, _, ps in header.values() for b, depth in ps if depth == 0} <= set(fifth._SCALARS)       # no struct by value
    for name, (rbase, rdepth, params) in header.items():
        ret, kinds = capi.signature(name)
        want = {("int", 0): ("status", "mask", "int"), ("long", 0): ("long",), ("size_t", 0): ("size_t",), ("char", 1): ("str",)}
        assert ret in want[(rbase, rdepth)], (name, ret)
        assert len(kinds) == len(params), name
        for i, (kind, (base, depth)) in enumerate(zip(kinds, params)):
            where = (name, i, kind, base, depth)
            assert kind in capi.KINDS, where
            if depth == 0:
                assert kind == fifth._SCALARS[base], where
            elif kind == "stream":
                assert (base, depth) == ("void", 1), where
            elif kind == "host*":
                assert depth >= 1, where
            elif base.startswith("Zeggs"):
                assert kind == base + "*" and depth == 1 and base in capi.FR_STRUCTS, where
            else:
                assert depth == 1 and kind == fifth._ELEMENTS[base], where
    text = HEADER.read_text()
    assert '#include "zeggs_hip.h"' in text and "zeggs_live_frames_version() >= 1" in text
    L, api = ops.lib(), capi.api()
    assert L.zeggs_version() == 109 and L.zeggs_live_resample_version() == 1
    assert L.zeggs_live_frames_version() == 1 and api.zeggs_live_frames_version() == 1
    for n in header:
        assert hasattr(L, n), f"libzeggs_hip.so does not export {n}"
        assert getattr(api, n).argtypes is not None and getattr(L, n).argtypes is None
    build = (ROOT / "ubisoft-laforge-zeroeggs_amd" / "csrc" / "build.sh").read_text()
    assert " live_frames " in build and " live_resample\"" in build and "../../include/zeggs_hip_frames.h" in build


def test_frames_struct_mirrors_are_the_fifth_header(fifth):
    structs = fifth._header_structs()
    assert set(structs) == set(capi.FR_STRUCTS) == {"ZeggsFramesDims", "ZeggsFramesRow"}
    for name, fields in structs.items():
        mirror = capi.FR_STRUCTS[name]._fields_
        assert [f for f, _ in mirror] == [f for f, _, _, _ in fields], name
        for (f, ctype), (_, base, depth, n) in zip(mirror, fields):
            want = ctypes.c_void_p if depth else fifth._CTYPES[base]
            assert ctype is want and n is None, (name, f)
    assert ctypes.sizeof(capi.FramesRow) == 80 and ctypes.sizeof(capi.FramesDims) == 20
    defs = dict(re.findall(r"#define (ZEGGS_FRAMES_\w+) (\d+)", fifth._header_text()))
    assert {k[len("ZEGGS_FRAMES_"):].lower(): int(v) for k, v in defs.items()} == ops.FRAMES_WHAT == dict(local=1, world=2, bvh=4)
    assert ops.frames_what(("local", "world", "bvh")) == 7 and ops.frames_what("bvh") == 4 and ops.frames_what(["world", "world"]) == 2


# ----------------------------------------------------------------------------- 4. refusals
J5 = 5


def _dims(rows=4, J=J5, max_frames=20, what=7, order=0):
    return capi.FramesDims(rows, J, max_frames, what, order)


GOOD = dict(pose=0x10000, rpos=0x20000, rrot=0x30000, local=0x40000, world=0x50000, bvh=0x60000, pose_ld=6 + 15 * J5, rpos_ld=3, rrot_ld=4,
            row=0, count=4)
STATE = ctypes.c_void_p(0x900000)


def _recs(*rows):
    arr = (capi.FramesRow * len(rows))()
    for q, over in zip(arr, rows):
        for k, v in dict(GOOD, **over).items():
            setattr(q, k, v)
    return arr


def test_frames_state_size():
    """the tables (3 J ints, padded to 8 bytes), then per row 14 doubles, two flags and 4 + 8J floats; refused dims give 0"""
    api = capi.api()
    assert api.zeggs_live_frames_state_bytes(_dims(4, 5)) == 64 + 4 * (120 + 176)
    assert api.zeggs_live_frames_state_bytes(_dims(64, 75)) == 904 + 64 * (120 + 2416)
    assert api.zeggs_live_frames_state_bytes(_dims(1, 1, 1, 1, capi.BvhDims(order=0).order)) == 16 + 120 + 48
    for bad, match in ((_dims(0), "0 rows"), (_dims(65), "65 rows"), (_dims(J=0), "0 joints"), (_dims(J=1025), "1025 joints"),
                       (_dims(max_frames=0), "max_frames 0"), (_dims(max_frames=4097), "max_frames 4097"), (_dims(what=0), "what = 0"),
                       (_dims(what=8), "what = 8"), (_dims(order=1 | (0 << 2) | (2 << 4)), "channel order"),
                       (_dims(order=2 | (0 << 2) | (1 << 4)), "channel order")):
        assert api.zeggs_live_frames_state_bytes(bad) == 0
        assert match in api.zeggs_last_error().decode(), api.zeggs_last_error().decode()
    from zeggs import anim
    for order in ("zyx", "xzy"):      # the two orders to_euler has, as the server packs them
        assert api.zeggs_live_frames_state_bytes(_dims(order=anim._to_euler_order(order))) > 0


@pytest.mark.parametrize("what,rows,dev,match", [
    ("a row out of range", [dict(row=4)], None, "record 0: row 4 of 4"),
    ("a negative row", [dict(), dict(row=-1)], 0x7000, "record 1: row -1 of 4"),
    ("a row twice", [dict(row=2), dict(row=1), dict(row=2)], 0x7000, "record 2: row 2 twice"),
    ("a negative count", [dict(count=-1)], None, "record 0: negative count -1"),
    ("more frames than max_frames", [dict(), dict(row=1, count=21)], 0x7000, "record 1: 21 frames, max_frames is 20"),
    ("a NULL pose", [dict(pose=0)], None, "record 0: NULL or misaligned source"),
    ("a NULL root position", [dict(rpos=0)], None, "record 0: NULL or misaligned source"),
    ("a misaligned root rotation", [dict(), dict(row=3, rrot=0x30002)], 0x7000, "record 1: NULL or misaligned source"),
    ("a misaligned pose", [dict(pose=0x10001)], None, "record 0: NULL or misaligned source"),
    ("a pose row that is too short", [dict(pose_ld=6 + 9 * J5 - 1)], None, "record 0: leading dimensions 50, 3, 4"),
    ("a root rotation row that is too short", [dict(rrot_ld=3)], None, "record 0: leading dimensions 81, 3, 3"),
    ("a NULL LOCAL destination", [dict(local=0)], None, "record 0: NULL or misaligned LOCAL destination"),
    ("a NULL WORLD destination", [dict(), dict(row=1, world=0)], 0x7000, "record 1: NULL or misaligned WORLD destination"),
    ("a NULL BVH destination", [dict(bvh=0)], None, "record 0: NULL or misaligned BVH destination"),
    ("a misaligned BVH destination", [dict(bvh=0x60004)], None, "record 0: NULL or misaligned BVH destination"),
    ("a misaligned LOCAL destination", [dict(local=0x40002)], None, "record 0: NULL or misaligned LOCAL destination"),
    ("two records without a device copy", [dict(), dict(row=1)], None, "must also be in device memory"),
    ("more records than rows", [dict(row=i % 4) for i in range(5)], 0x7000, "5 records for 4 rows"),
])
def test_frames_refuses_on_the_host(what, rows, dev, match):
    """every refusal comes before the launch (the addresses are never followed, there is no device here), with the record named"""
    d, arr = _dims(), _recs(*rows)
    nbytes = capi.api().zeggs_live_frames_state_bytes(d)
    dev_p = ctypes.cast(ctypes.c_void_p(dev), ctypes.POINTER(capi.FramesRow)) if dev else None
    with pytest.raises(RuntimeError, match="zeggs_live_frames: frames: .*" + match):
        capi.api().zeggs_live_frames(d, arr, dev_p, len(rows), STATE, nbytes, None)
    assert ops.lib().zeggs_live_frames(ctypes.byref(d), arr, ctypes.c_void_p(dev or 0), len(rows), STATE, ctypes.c_size_t(nbytes), None) == -1


def test_frames_entry_points_check_dims_state_tables_and_row():
    api, d = capi.api(), _dims()
    nbytes = api.zeggs_live_frames_state_bytes(d)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    with pytest.raises(RuntimeError, match="state too small"):
        api.zeggs_live_frames(d, _recs({}), None, 1, STATE, nbytes - 1, None)
    with pytest.raises(RuntimeError, match="NULL state"):
        api.zeggs_live_frames_reset(d, None, nbytes, 0, None, None, None, None, 0, None)
    with pytest.raises(RuntimeError, match="misaligned state"):
        api.zeggs_live_frames(d, _recs({}), None, 1, ctypes.c_void_p(0x900004), nbytes, None)
    # a J whose frame does not fit the LDS, and a max_frames out of range, are refused with the dims by every entry
    with pytest.raises(RuntimeError, match="2000 joints"):
        api.zeggs_live_frames(_dims(J=2000), _recs({}), None, 1, STATE, 1 << 30, None)
    with pytest.raises(RuntimeError, match="max_frames 5000"):
        api.zeggs_live_frames(_dims(max_frames=5000), _recs({}), None, 1, STATE, 1 << 30, None)
    # a bit that is off: its destination is not looked at
    with pytest.raises(RuntimeError, match="record 0: NULL or misaligned BVH destination"):
        api.zeggs_live_frames(_dims(what=4), _recs(dict(local=0, world=0, bvh=0)), None, 1, STATE, nbytes, None)
    # the skeleton tables
    for parents, match in ((ints(0, 0, 1, 2, 3), "parents\\[0\\] = 0"), (ints(-1, 0, 2, 1, 1), "parents\\[2\\] = 2"),
                           (ints(-1, 0, 1, 4, 2), "parents\\[3\\] = 4"), (ints(-1, -1, 0, 1, 2), "parents\\[1\\] = -1")):
        with pytest.raises(RuntimeError, match="frames prepare: " + match):
            api.zeggs_live_frames_prepare(d, parents, ints(0, 1, 2, 3, 4), STATE, nbytes, None)
    for seq, match in ((ints(0, 1, 1, 2, 3), "seq\\[2\\] = 1"), (ints(0, 1, 2, 3, 5), "seq\\[4\\] = 5"), (ints(-1, 1, 2, 3, 4), "seq\\[0\\] = -1")):
        with pytest.raises(RuntimeError, match="frames prepare: " + match + ": seq is no permutation"):
            api.zeggs_live_frames_prepare(d, ints(-1, 0, 0, 1, 2), seq, STATE, nbytes, None)
    with pytest.raises(RuntimeError, match="NULL parents / seq"):
        api.zeggs_live_frames_prepare(d, None, ints(0, 1, 2, 3, 4), STATE, nbytes, None)
    # the row that opens
    with pytest.raises(RuntimeError, match="reset: row 4 of 4"):
        api.zeggs_live_frames_reset(d, STATE, nbytes, 4, None, None, None, None, 0, None)
    f3, f4 = (ctypes.c_float * 3)(), (ctypes.c_float * 4)(1.0)
    with pytest.raises(RuntimeError, match="row 1: a placement needs"):
        api.zeggs_live_frames_reset(d, STATE, nbytes, 1, f3, f4, None, (ctypes.c_double * 4)(1.0), 1, None)
    # nothing to do: no launch, no error
    assert api.zeggs_live_frames(d, None, None, 0, STATE, nbytes, None) == 0
    assert api.zeggs_live_frames(d, _recs(dict(count=0, pose=0, local=0), dict(count=0, row=3, bvh=0)), None, 2, STATE, nbytes, None) == 0


# ----------------------------------------------------------------------------- 5. LiveServer(frames=...) and open()
PARENTS = SKELETONS["tree"]


@pytest.mark.parametrize("bad,match", [
    (dict(what=("local",)), "needs the skeleton"), (dict(parents=None), "needs the skeleton"), (dict(parents=PARENTS, what=("local", "globe")), "what"),
    (dict(parents=PARENTS, what=()), "what"), (dict(parents=PARENTS, what=7), "what|iterable"), (dict(parents=PARENTS, what=("local", "world"), text=True), "text=True"),
    (dict(parents=PARENTS, order="yzx"), "order 'yzx'"), (dict(parents=[0, 0, 1]), "parents"), (dict(parents=[-1, 0, 2]), "parents"),
    (dict(parents=PARENTS, names=["a", "b"]), "2 names for 5 joints"), (dict(parent=PARENTS), "keys"), ("bvh", "a dict with keys"),
])
def test_frames_options_are_checked_at_construction(bad, match):
    """before any weight is looked at"""
    with pytest.raises((ValueError, TypeError), match=match):
        live.LiveServer(None, None, {}, CONF, 1 / 60.0, frames=bad)
    with pytest.raises(ValueError):
        live.LiveServer(None, None, {}, CONF, 1 / 60.0, frames=bad)


def test_frames_options_defaults():
    assert live.frames_options(None) is None
    o = live.frames_options(dict(parents=np.asarray(PARENTS)))
    assert o == dict(parents=PARENTS, names=None, what=("local", "world", "bvh"), mask=7, order="zyx", text=False, seq=fo.TREE_SEQ)
    o = live.frames_options(dict(parents=PARENTS, what=("bvh", "local"), order="xzy", text=True, names=list("abcde")))
    assert o["what"] == ("local", "bvh") and o["mask"] == 5 and o["order"] == "xzy" and o["text"] is True and o["names"] == list("abcde")


def test_a_placement_comes_whole_and_needs_the_head():
    """open() decides before it touches a row"""
    assert live.frames_placement(None, None) is None
    pos, rot = live.frames_placement([1, 2, 3], (1, 0, 0, 0))
    assert pos.dtype == rot.dtype == np.float64 and pos.tolist() == [1.0, 2.0, 3.0] and rot.tolist() == [1.0, 0.0, 0.0, 0.0]
    off, on = types.SimpleNamespace(fs=16000, _loud=None, _fr=None), types.SimpleNamespace(fs=16000, _loud=None, _fr=object())
    for stub in (off, on):
        with pytest.raises(ValueError, match="both or neither"):
            live.LiveServer.open(stub, None, None, start_position=[0.0, 0.0, 0.0])
        with pytest.raises(ValueError, match="both or neither"):
            live.LiveServer.open(stub, None, None, start_rotation=[1.0, 0.0, 0.0, 0.0])
        with pytest.raises(ValueError, match="quaternion \\[4\\]"):
            live.LiveServer.open(stub, None, None, start_position=[0.0, 0.0, 0.0], start_rotation=[1.0, 0.0, 0.0])
        with pytest.raises(ValueError, match="quaternion \\[4\\]"):
            live.LiveServer.open(stub, None, None, start_position=[0.0, float("nan"), 0.0], start_rotation=[1.0, 0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="needs the output head"):
        live.LiveServer.open(off, None, None, start_position=[0.0, 0.0, 0.0], start_rotation=[1.0, 0.0, 0.0, 0.0])


def test_the_packed_block_unpacks_to_the_documented_arrays():
    """frames_unpack: [BVH rows | LOCAL | WORLD] of all records, an area whose bit is off missing, arrays that own their memory"""
    J, counts = 3, [2, 0, 5]
    N = sum(counts)
    for mask in (7, 5, 2, 4):
        nb = live.frames_block_bytes(N, J, mask)
        assert nb == N * ((12 * 8 if mask & 4 else 0) + (28 * 4 if mask & 1 else 0) + (21 * 4 if mask & 2 else 0))
        buf = np.zeros(nb, np.uint8)
        o_loc = N * 96 * bool(mask & 4)
        if mask & 4:
            buf[:o_loc].view(np.float64)[:] = np.arange(N * 12)
        if mask & 1:
            buf[o_loc:o_loc + N * 112].view(np.float32)[:] = 1000 + np.arange(N * 28)
        if mask & 2:
            buf[nb - N * 84:].view(np.float32)[:] = 5000 + np.arange(N * 21)
        got = live.frames_unpack(buf, counts, J, mask)
        assert len(got) == 3 and all(set(g) == {k for n in ("local", "world", "bvh") if mask & ops.FRAMES_WHAT[n] for k in ops.FRAMES_KEYS[n]}
                                     for g in got)
        a = got[2]
        if mask & 4:
            assert a["bvh"].shape == (5, 12) and a["bvh"][0, 0] == 2 * 12 and a["bvh"].dtype == np.float64 and got[1]["bvh"].shape == (0, 12)
        if mask & 1:
            assert [a[k].shape for k in ("root_pos", "root_rot", "lrot", "lpos")] == [(5, 3), (5, 4), (5, 3, 4), (5, 3, 3)]
            assert a["root_pos"][0, 0] == 1000 + 2 * 28 and a["root_rot"][0, 0] == a["root_pos"][0, 0] + 3
            assert a["lrot"][0, 0, 0] == a["root_pos"][0, 0] + 7 and a["lpos"][0, 0, 0] == a["root_pos"][0, 0] + 7 + 12
        if mask & 2:
            assert a["gpos"].shape == (5, 3, 3) and a["grot"].shape == (5, 3, 4) and a["grot"][1, 0, 0] == 5000 + 3 * 21 + 9
        buf[:] = 0
        assert all(v.any() for g in (got[0], got[2]) for v in g.values())      # nothing aliases the block


# ----------------------------------------------------------------------------- the head's three forms behind one table
class _Recorder:
    """stands in for the typed API: every call is written down, none reaches the library (a size query answers 64 bytes)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 64 if name.endswith("_state_bytes") else 0
        return call


HEAD_FORMS = {
    "frames": (ops.LiveFrames, capi.FramesRow, capi.FR_PROTOTYPES,
               ["zeggs_live_frames_state_bytes", "zeggs_live_frames_prepare", "zeggs_live_frames_reset", "zeggs_live_frames", "zeggs_live_frames_spans"]),
    "retime": (ops.LiveRetime, capi.RetimeRow, capi.RT_PROTOTYPES,
               ["zeggs_live_retime_state_bytes", "zeggs_live_retime_prepare", "zeggs_live_retime_reset", "zeggs_live_frames_retimed", "zeggs_live_retime_spans"]),
    "refilter": (ops.LiveRefilter, capi.RefilterRow, capi.RF_PROTOTYPES,
                 ["zeggs_live_refilter_state_bytes", "zeggs_live_refilter_prepare", "zeggs_live_refilter_reset", "zeggs_live_frames_refiltered",
                  "zeggs_live_refilter_spans"]),
}


@pytest.mark.parametrize("form", list(HEAD_FORMS))
def test_each_head_form_reaches_its_own_entry_points_and_no_other(form, monkeypatch):
    """ops.LiveFrames' table of entry points, which the constructor, the one reset, the one launch and live_frames_spans read: an
    object of each form calls the five entry points of its own header (the span report: the eighth's), in the order asked and
    nothing else, with its own record type behind rows_dev; max_half follows the dims in every call of the filtered form and in
    none of the others; the six names of the headers' calls are the two shared functions.  No device: the API is a recorder."""
    cls, record, protos, names = HEAD_FORMS[form]
    assert all(n in protos or n in capi.SNAP_PROTOTYPES for n in names)
    rec = _Recorder()
    monkeypatch.setattr(ops, "api", lambda: rec)
    monkeypatch.setattr(ops, "_stream", lambda: "stream")
    args = (4, SKELETONS["tree"], 20) + ((16,) if form == "refilter" else ())
    head = cls(*args, device="cpu")
    extra = (16,) if form == "refilter" else ()
    assert head.extra == extra and head.record is record
    rows = (record * 4)()
    ops.live_head_reset(head, 2)
    ops.live_head_reset(head, 3, [0, 0, 0], [1, 0, 0, 0], [1, 2, 3], [0, 1, 0, 0])
    ops.live_head_launch(head, rows, 1)
    ops.live_head_launch(head, rows, 3, 0x7000)
    ops.live_frames_spans(head, 1)
    assert [c[0] for c in rec.calls] == [names[0], names[1], names[2], names[2], names[3], names[3], names[4]]
    for name, a in rec.calls:
        assert a[0] is head.d and a[1:1 + len(extra)] == extra, name
    tail = [a[1 + len(extra):] for _, a in rec.calls]           # what follows the dims and, on the filtered form, max_half
    assert tail[0] == () and len(tail[1]) == 5 and list(tail[1][0]) == SKELETONS["tree"] and tail[1][2:] == (head.state, 64, "stream")
    assert tail[2] == (head.state, 64, 2, None, None, None, None, 0, "stream")
    assert tail[3][:3] == (head.state, 64, 3) and [list(v) for v in tail[3][3:7]] == [[0, 0, 0], [1, 0, 0, 0], [1, 2, 3], [0, 1, 0, 0]]
    assert tail[3][7:] == (1, "stream")
    assert tail[4] == (rows, None, 1, head.state, 64, "stream")
    assert tail[5][0] is rows and isinstance(tail[5][1], ctypes.POINTER(record)) and tail[5][2:] == (3, head.state, 64, "stream")
    assert ctypes.cast(tail[5][1], ctypes.c_void_p).value == 0x7000
    assert tail[6][0] == 1 and len(tail[6]) == 3 and tail[6][2] == ops.SNAP_MAX_SPANS
    assert ops.live_frames_reset is ops.live_retime_reset is ops.live_refilter_reset is ops.live_head_reset
    assert ops.live_frames is ops.live_frames_retimed is ops.live_frames_refiltered is ops.live_head_launch
