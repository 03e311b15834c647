"""Host-only parts of the planting stage of live serving (feet that stay planted: contact lock and leg IK): the float64 oracle
(tests/live_plant_oracle.py) against the properties the definition promises and the conditions the GPU tests lean on, the shared
header csrc/plant_math.h on the host (tests/host/plant_math_check.cpp, plain and under sanitizers) against numbers the oracle
wrote, include/zeggs_hip_plant.h against zeggs/capi.py, and every refusal that comes before a launch.  No GPU needed -- the
library loads on the CPU for host-only calls."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import live_plant_oracle as po
import test_live_gaze_cpu as ninth
from zeggs import capi, live, ops, synth

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "zeggs_hip_plant.h"
CASES = [("walker", 1), ("walker", 2), ("rig", 1), ("rig", 2)]
U = 2.0 ** -53                     # unit roundoff of float64


def _fk(c, f, ch, q3):
    """the chain's world points and rotations in frame f with the local rotations q3 of (u, m, e): the oracle's own FK statement"""
    J = len(c["parents"])
    lpos, ltxy = po.split(c["pose"][f], J)
    lrot = po.local_rotations(ltxy)
    for j, q in zip(c["idx"][ch], q3):
        lrot[j] = q
    return po.chain_fk(lrot, lpos.astype(np.float64), c["rpos"][f], c["rrot"][f], c["parents"], c["idx"][ch])


def _depth(c, ch):
    n, a = 3, c["parents"][c["idx"][ch][0]]
    while a >= 0:
        n, a = n + 1, c["parents"][a]
    return n + 1                   # (the root's fold)


# ----------------------------------------------------------------------------- 1. the oracle against the definition's promises
@pytest.mark.parametrize("name,seed", CASES)
def test_the_solve_keeps_what_it_promises(name, seed):
    """on every solved (frame, chain): the bone lengths l1, l2 are kept, H is where it was, the solved ankle is on T and the foot's
    world rotation is what it was -- each to a bound made of the float64 rounding of the operations between the inputs and the
    value times the lengths involved: a quaternion product or a rotation of a vector costs at most 8 U relative, so a vector of
    length l turned by a product of n quaternions of unit length (to n 8 U) is off by at most 2 n 8 U l; every other float of
    the row, lpos among them, is the same bits"""
    c = po.case(name, seed)
    d, J = c["det"], len(c["parents"])
    assert d["solved"].sum() >= 40
    worst = dict(l1=0.0, l2=0.0, H=0.0, A=0.0, rot=0.0)
    for f, ch in zip(*np.nonzero(d["solved"])):
        n = _depth(c, ch)
        before, after = _fk(c, f, ch, d["lrot0"][f, ch]), _fk(c, f, ch, d["lrot"][f, ch])
        assert np.array_equal(before["A"], d["A"][f, ch]) and np.array_equal(before["H"], d["H"][f, ch])
        l1, l2 = po.norm(before["K"] - before["H"]), po.norm(before["A"] - before["K"])
        scale = np.abs(before["H"]).max() + l1 + l2
        per_turn = 2.0 * 8.0 * U
        # the angles come out of acos at interior angles of at least 2.5 degrees (the reach limit: stretch 0.999): 1 / sin < 23
        bound_pos = (n + 6) * per_turn * (l1 + l2) * 23.0 + 16.0 * U * scale
        e = dict(l1=abs(po.norm(after["K"] - after["H"]) - l1) / (4.0 * per_turn * l1), l2=abs(po.norm(after["A"] - after["K"]) - l2) / (6.0 * per_turn * l2),
                 H=np.abs(after["H"] - before["H"]).max() / (16.0 * U * scale), A=po.norm(after["A"] - d["T"][f, ch]) / bound_pos,
                 rot=min(np.abs(after["ge"] - before["ge"]).max(), np.abs(after["ge"] + before["ge"]).max()) / ((n + 8) * per_turn))
        for k, v in e.items():
            worst[k] = max(worst[k], v)
            assert v <= 1.0 or (k == "H" and np.array_equal(after["H"], before["H"])), (name, seed, f, ch, k, v)
    print({k: round(v, 4) for k, v in worst.items()})
    # the rows: only the ltxy of the chains' joints of solved frames differ from the input
    lo = 6 + 3 * J
    differs = c["out"].view(np.uint32) != c["pose"].view(np.uint32)
    allowed = np.zeros_like(differs)
    for f, ch in zip(*np.nonzero(d["solved"])):
        for j in c["idx"][ch]:
            allowed[f, lo + 6 * j:lo + 6 * j + 6] = True
    assert not (differs & ~allowed).any() and differs.any()
    assert np.array_equal(po.split(c["out"], J)[0].view(np.uint32), po.split(c["pose"], J)[0].view(np.uint32))


@pytest.mark.parametrize("name,seed", CASES)
def test_targets_hold_still_and_never_jump(name, seed):
    """a held span whose target the reach limit leaves alone is ONE point, the same bits; and from any frame to the next the target
    moves by no more than the unconstrained ankle does plus one step of the fade (the largest difference of g over one frame times
    the offset of the last release) -- where the reach limit pulls, plus twice what H moved and what the reach changed (a
    projection onto a ball is no expansion; the ball moves with H) -- plus the rounding of the sums, 16 U times the coordinates"""
    c = po.case(name, seed)
    d, opt = c["det"], c["opt"]
    N = opt["release"]
    g_step = max(po.fade(k, N) - po.fade(k + 1, N) for k in range(N))
    held, T = c["contacts"].astype(bool), d["T"]
    reach = opt["stretch"] * (np.linalg.norm(d["K"] - d["H"], axis=-1) + np.linalg.norm(d["A"] - d["K"], axis=-1))
    pulled = np.linalg.norm(T - d["H"], axis=-1) >= reach * (1.0 - 1e-12)
    spans = 0
    for ch in range(held.shape[1]):
        for f in range(1, held.shape[0]):
            if held[f, ch] and held[f - 1, ch] and not pulled[f, ch] and not pulled[f - 1, ch]:
                assert np.array_equal(T[f, ch], T[f - 1, ch]), (f, ch)
                spans += 1
            jump = po.norm(T[f, ch] - T[f - 1, ch])
            bound = po.norm(d["A"][f, ch] - d["A"][f - 1, ch]) + g_step * max(d["o0"][f, ch], d["o0"][f - 1, ch]) + 16.0 * U * np.abs(d["A"][f, ch]).max()
            if pulled[f, ch] or pulled[f - 1, ch]:
                bound += 2.0 * po.norm(d["H"][f, ch] - d["H"][f - 1, ch]) + abs(reach[f, ch] - reach[f - 1, ch])
            assert jump <= bound, (name, seed, f, ch, jump, bound)
    assert spans >= 30
    # a release keeps the target where it was: the frame a chain leaves HELD has the held point as its target (before the reach limit)
    for ch in range(held.shape[1]):
        for f in range(1, held.shape[0]):
            if held[f - 1, ch] and not held[f, ch] and not pulled[f, ch] and not pulled[f - 1, ch]:
                assert np.abs(T[f, ch] - T[f - 1, ch]).max() <= 16.0 * U * np.abs(T[f, ch]).max()


@pytest.mark.parametrize("name,seed", CASES)
def test_the_inputs_are_the_walk_the_tests_need(name, seed):
    """the scripted walk: each foot alternately stands and swings, a stance lasts at least 6 frames at a speed under v_on, one held
    foot is dragged past the slack, one chain re-enters in an unfinished fade, the reach limit binds in at least one frame, the
    knees stay between 20 and 160 degrees -- and (the condition of the GPU test, which compares ALL frames and chains) every
    comparison of the definition is decided by a relative margin above 1e-6"""
    c = po.case(name, seed)
    d, opt, held = c["det"], c["opt"], c["contacts"].astype(bool)
    knees = po.knee_angles(d)
    assert 20.0 < knees.min() and knees.max() < 160.0
    speed = np.linalg.norm(np.diff(d["A"], axis=0), axis=-1) / opt["dt"]
    for ch in range(2):
        runs = [len(r) for r in "".join("1" if h else "0" for h in held[:, ch]).split("0") if r]
        assert len(runs) >= 2 and max(runs) >= 6 and (~held[:, ch]).sum() >= 8, (ch, runs)
        both = held[1:, ch] & held[:-1, ch]
        assert speed[both, ch].max() < opt["speed"][1]
    entries = [(f, ch) for f in range(1, len(held)) for ch in range(2) if held[f, ch] and not held[f - 1, ch]]
    assert any(0 < d["k"][f - 1, ch] < opt["release"] and d["o0"][f - 1, ch] > 0.0 for f, ch in entries), "no re-entry in an unfinished fade"
    by = {}
    for f, ch, what, lhs, rhs in d["margins"]:
        by.setdefault(what, []).append((f, ch, lhs, rhs))
    assert set(by) == {"v_on", "h_on", "v_off", "h_off", "slack", "reach", "bend", "swing"}
    releases = [(f, ch) for f in range(1, len(held)) for ch in range(2) if held[f - 1, ch] and not held[f, ch]]
    over = {what: {(f, ch) for f, ch, lhs, rhs in by[what] if lhs > rhs} for what in ("slack", "v_off", "h_off")}
    assert [x for x in releases if x in over["slack"] and x not in over["v_off"] and x not in over["h_off"]], "no foot dragged past the slack"
    assert any(lhs > rhs for _, _, lhs, rhs in by["reach"]), "the reach limit never binds"
    margin, which = po.min_margin(d["margins"])
    assert margin > 1e-6, which
    assert any(0 < r[0] for r in by["v_on"] if r[2] <= r[3]) and c["contacts"].any() and not c["contacts"].all()


def test_cuts_and_thresholds_that_never_plant():
    """the oracle itself: a sequence cut into calls with the states carried on gives the bits of the whole, and thresholds that no
    frame meets leave every row as it was"""
    c = po.case("walker", 1)
    for cuts in ((3, 17, 20), (7, 1, 32), (1,) * 40):
        states, outs, flags, a = [po.new_state() for _ in c["idx"]], [], [], 0
        for n in cuts:
            o, k = po.plant(c["pose"][a:a + n], c["rpos"][a:a + n], c["rrot"][a:a + n], c["parents"], c["idx"], c["opt"], states)
            outs.append(o), flags.append(k)
            a += n
        assert np.array_equal(np.concatenate(outs).view(np.uint32), c["out"].view(np.uint32)) and np.array_equal(np.concatenate(flags), c["contacts"])
    never = po.options(speed=(0.0, 0.0), height=(-1e9, -1e9))
    o, k = po.plant(c["pose"], c["rpos"], c["rrot"], c["parents"], c["idx"], never)
    assert np.array_equal(o.view(np.uint32), c["pose"].view(np.uint32)) and not k.any()


# ----------------------------------------------------------------------------- 2. csrc/plant_math.h on the host, against the oracle
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_plant_arithmetic_on_the_host_equals_the_oracle(tmp_path, flags):
    """tests/host/plant_math_check.cpp: a stand-alone program over the header the kernel uses (its head says what it reads and
    prints); once plain, once under the address and undefined-behaviour sanitizers (host code with its own main, run directly).
    The oracle writes the unconstrained chains of both skeletons' walks; the program's contact flags and solve decisions must be
    the oracle's exactly, its targets the oracle's to 64 U times the coordinates, its ltxy the oracle's float32 to 2^-23"""
    cxx = ninth._cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "plant_math_check"
    b = subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "plant_math_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    worst = 0.0
    for name, seed in (("walker", 1), ("rig", 2)):
        c = po.case(name, seed)
        d, opt, J = c["det"], c["opt"], len(c["parents"])
        T, C = c["contacts"].shape
        rows = [" ".join(repr(float(x)) for x in (C, T, opt["dt"], *opt["speed"], *opt["height"], opt["ground"], opt["slack"], opt["stretch"], opt["release"]))]
        for f in range(T):
            for ch in range(C):
                v = np.concatenate([d["H"][f, ch], d["K"][f, ch], d["A"][f, ch], d["gp"][f, ch], d["root"][f, ch], d["lrot0"][f, ch].reshape(-1)])
                rows.append(" ".join(repr(float(x)) for x in v))
        table = tmp_path / f"{name}.txt"
        table.write_text("\n".join(rows) + "\n")
        r = subprocess.run([str(exe), str(table)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.strip().splitlines()
        assert lines[-1] == "plant_math_check: ok" and len(lines) == T * C + 1
        out_xy = po.split(c["out"], J)[1]
        for line in lines[:-1]:
            head, tgt, xy = line.split("|")
            _, f, ch, held, solved = head.split()
            f, ch = int(f), int(ch)
            assert int(held) == c["contacts"][f, ch] and bool(int(solved)) == bool(d["solved"][f, ch]), line
            got_t = np.array([float(x) for x in tgt.split()])
            assert np.abs(got_t - d["T"][f, ch]).max() <= 64.0 * U * np.abs(d["T"][f, ch]).max(), line
            got = np.array([float(x) for x in xy.split()]).reshape(3, 6)
            if d["solved"][f, ch]:
                want = np.stack([out_xy[f, j].reshape(6) for j in c["idx"][ch]]).astype(np.float64)
                e = np.abs(got - want).max()
                worst = max(worst, e)
                assert e <= 2.0 ** -23, (line, e)
    print(f"worst ltxy error {worst:.3g}")


# ----------------------------------------------------------------------------- 3. the eleventh header against capi.PL_*
@pytest.fixture
def eleventh(monkeypatch):
    monkeypatch.setattr(ninth, "HEADER", HEADER)
    return ninth


def test_plant_prototypes_are_the_eleventh_header(eleventh):
    """capi.PL_PROTOTYPES against include/zeggs_hip_plant.h: the same names, disjoint from the other ten groups; per function the
    return kind, the parameter count, every parameter's kind and every device pointer's element type; the library exports them
    all; zeggs_version() is still 109 and zeggs_live_plant_version() is 1; the unit is in build.sh"""
    header = eleventh._header_prototypes()
    assert set(header) == set(capi.PL_PROTOTYPES) and len(header) == 6
    groups = (*eleventh._OTHERS, "GZ_", "SB_")
    assert not set(capi.PL_PROTOTYPES) & {n for g in groups for n in getattr(capi, g + "PROTOTYPES")}
    assert not set(capi.PL_STRUCTS) & {n for g in groups for n in getattr(capi, g + "STRUCTS")}
    structs = {n: c for g in (*groups, "PL_") for n, c in getattr(capi, g + "STRUCTS").items()}
    for name, (rbase, rdepth, params) in header.items():
        ret, kinds = capi.signature(name)
        want = {("int", 0): ("status", "mask", "int"), ("size_t", 0): ("size_t",)}
        assert ret in want[(rbase, rdepth)], (name, ret)
        assert len(kinds) == len(params), name
        for i, (kind, (base, depth)) in enumerate(zip(kinds, params)):
            where = (name, i, kind, base, depth)
            assert kind in capi.KINDS, where
            if depth == 0:
                assert kind == eleventh._SCALARS[base], where
            elif kind == "stream":
                assert (base, depth) == ("void", 1), where
            elif kind == "host*":
                assert depth >= 1, where
            elif base.startswith("Zeggs"):
                assert kind == base + "*" and depth == 1 and base in structs, where
            else:
                assert depth == 1 and kind == eleventh._ELEMENTS[base], where
    text = HEADER.read_text()
    assert '#include "zeggs_hip_snapshot.h"' in text and "zeggs_version() >= 109" in text
    L, api = ops.lib(), capi.api()
    assert L.zeggs_version() == 109 and L.zeggs_live_plant_version() == 1 and api.zeggs_live_plant_version() == 1
    for n in header:
        assert hasattr(L, n), f"libzeggs_hip.so does not export {n}"
        assert getattr(api, n).argtypes is not None and getattr(L, n).argtypes is None
    build = (ROOT / "ubisoft-laforge-zeroeggs_amd" / "csrc" / "build.sh").read_text()
    assert " live_plant " in build and "../../include/zeggs_hip_plant.h" in build


def test_plant_struct_mirrors_are_the_eleventh_header(eleventh):
    structs = eleventh._header_structs()
    assert set(structs) == set(capi.PL_STRUCTS) == {"ZeggsPlantDims", "ZeggsPlantRow"}
    for name, fields in structs.items():
        mirror = capi.PL_STRUCTS[name]._fields_
        assert [f for f, _ in mirror] == [f for f, _, _, _ in fields], name
        for (f, ctype), (_, base, depth, n) in zip(mirror, fields):
            want = ctypes.c_void_p if depth else eleventh._CTYPES[base]
            assert ctype is want and n is None, (name, f)
    assert (ctypes.sizeof(capi.PlantDims), ctypes.sizeof(capi.PlantRow)) == (88, 80)
    text = eleventh._header_text()
    assert int(re.search(r"#define ZEGGS_PLANT_MAX_CHAINS (\d+)", text).group(1)) == ops.PLANT_MAX_CHAINS == 4
    assert int(re.search(r"#define ZEGGS_PLANT_CHAIN_BYTES (\d+)", text).group(1)) == 88


# ----------------------------------------------------------------------------- 4. refusals
WALK = (po.WALK_PARENTS, po.WALK_NAMES)


@pytest.mark.parametrize("bad,match", [
    ("auto", "True or a dict"), (dict(chain="auto"), "keys"), (dict(chains="legs"), "chains 'legs'"), (dict(chains=[]), r"0 chains \(1..4\)"),
    (dict(chains=[(1, 2, 3)] * 5), r"5 chains \(1..4\)"), (dict(chains=[(1, 2)]), r"chain \(1, 2\) is not"),
    (dict(chains=[("RightUpLeg", "RightLeg", "RightHeel")]), r"chain \('RightUpLeg', 'RightLeg', 'RightHeel'\): no joint named 'RightHeel'"),
    (dict(chains=[(1, 2, 9)]), r"chain \(1, 2, 9\): joint 9"), (dict(chains=[(1, 2, 4)]), r"chain \(1, 2, 4\) is no chain"),
    (dict(chains=[(1, 3, 4)]), r"chain \(1, 3, 4\) is no chain"), (dict(chains=[(1, 2, 3), (2, 3, 4)]), r"chain \(2, 3, 4\) shares a joint"),
    (dict(speed=(3.0, 2.0)), "speed"), (dict(speed=(-1.0, 2.0)), "speed"), (dict(speed=2.0), "speed"), (dict(height=(3.0, 2.0)), "height"),
    (dict(height=(0.0, float("inf"))), "height"), (dict(ground=float("nan")), "ground"), (dict(slack=-1.0), "slack"), (dict(release=-1), "release"),
    (dict(release=2.5), "release"), (dict(stretch=0.0), "stretch"), (dict(stretch=1.5), "stretch"),
])
def test_plant_options_are_checked_on_the_host(bad, match):
    with pytest.raises(ValueError, match="plant: .*" + match):
        ops.plant_options(bad, *WALK)


def test_plant_options_defaults_and_auto():
    o = ops.plant_options(True, *WALK)
    assert o["chains"] == [(1, 2, 3), (5, 6, 7)] and o["stretch"] == 0.999 and o["ground"] == 0.0 and o["release"] >= 0
    assert o["speed"][0] <= o["speed"][1] and o["height"][0] <= o["height"][1] and set(o) == set(ops.PLANT_DEFAULTS)
    rig = ops.plant_options(dict(chains="auto"), synth.PARENTS, synth.BONE_NAMES)["chains"]
    assert rig == po.chain_indices(po.RIG_CHAINS, synth.BONE_NAMES) and len(rig) == 2
    assert ops.plant_options(dict(chains=[("LeftUpLeg", 6, "LeftFoot")]), *WALK)["chains"] == [(5, 6, 7)]
    with pytest.raises(ValueError, match="chains 'auto' needs joint names"):
        ops.plant_options(True, po.WALK_PARENTS, None)
    with pytest.raises(ValueError, match="chains 'auto' needs joint names"):
        ops.plant_options(True, po.WALK_PARENTS, [f"j{i}" for i in range(9)])


def test_a_server_refuses_plant_without_frames_and_bad_options():
    conf, dt = ninth.CONF, 1 / 60.0
    with pytest.raises(ValueError, match=r"plant corrects the rows the output head reads: it needs frames=dict\(parents=...\)"):
        live.LiveServer(None, None, {}, conf, dt, plant=True)
    with pytest.raises(ValueError, match="plant: .*is no chain"):
        live.LiveServer(None, None, {}, conf, dt, frames=dict(parents=po.WALK_PARENTS, names=po.WALK_NAMES), plant=dict(chains=[(1, 2, 4)]))
    with pytest.raises(ValueError, match="chains 'auto' needs joint names"):
        live.LiveServer(None, None, {}, conf, dt, frames=dict(parents=po.WALK_PARENTS), plant=True)
    assert live.plant_options(None, None) is None and live.plant_options(False, None) is None


def _dims(rows=4, J=9, max_frames=8, chains=2, release=4, dt=1 / 60.0, v=(1.0, 2.0), h=(1.0, 2.0), ground=0.0, slack=5.0, stretch=0.999):
    return capi.PlantDims(rows, J, max_frames, chains, release, 0, dt, v[0], v[1], h[0], h[1], ground, slack, stretch)


def _recs(*rows):
    arr = (capi.PlantRow * len(rows))()
    for q, w in zip(arr, rows):
        w = dict(dict(pose=0x10000, rpos=0x20000, rrot=0x30000, out=0x40000, contacts=0x50000, pose_ld=141, rpos_ld=3, rrot_ld=4, out_ld=141, row=0,
                      count=4), **w)
        for k, v in w.items():
            setattr(q, k, v)
    return arr


STATE = ctypes.c_void_p(0x900000)


def test_plant_state_size_and_spans():
    api = capi.api()
    assert api.zeggs_live_plant_state_bytes(_dims(4)) == 88 + 4 * 352 and api.zeggs_live_plant_state_bytes(_dims(64, 75)) == 352 + 64 * 352
    for bad, msg in ((_dims(0), "0 rows"), (_dims(65), "65 rows"), (_dims(J=2), "2 joints"), (_dims(max_frames=0), "max_frames 0"), (_dims(chains=0), "0 chains"),
                     (_dims(chains=5), "5 chains"), (_dims(release=-1), "release -1"), (_dims(dt=0.0), "frame time 0"), (_dims(v=(3.0, 2.0)), "speed thresholds"),
                     (_dims(h=(3.0, 2.0)), "height thresholds"), (_dims(ground=float("nan")), "ground"), (_dims(slack=-1.0), "slack -1"),
                     (_dims(stretch=0.0), "stretch 0")):
        assert api.zeggs_live_plant_state_bytes(bad) == 0 and msg in api.zeggs_last_error().decode(), msg
    lp = type("LP", (), dict(d=_dims(8)))
    assert [ops.live_plant_spans(lp, r) for r in (0, 3, 7)] == [[(88, 352)], [(88 + 3 * 352, 352)], [(88 + 7 * 352, 352)]]
    for row in (-1, 8):
        with pytest.raises(RuntimeError, match=f"plant spans: row {row} of 8"):
            ops.live_plant_spans(lp, row)
    with pytest.raises(RuntimeError, match="room for 0 spans"):
        api.zeggs_live_plant_spans(_dims(8), 0, (capi.SnapSpan * 1)(), 0)


@pytest.mark.parametrize("what,chains,match", [
    ("an index out of range", [1, 2, 9, 5, 6, 7], r"chain 0 \(1, 2, 9\): a joint outside 0 .. 8"),
    ("no chain", [1, 2, 3, 5, 6, 8], r"chain 1 \(5, 6, 8\) is no chain: parents\[6\] = 5, parents\[8\] = 7"),
    ("a joint twice", [1, 2, 3, 1, 2, 3], r"chain 1 \(1, 2, 3\) shares a joint"),
])
def test_plant_prepare_names_the_chain_it_refuses(what, chains, match):
    api, d = capi.api(), _dims()
    parents = (ctypes.c_int * 9)(*po.WALK_PARENTS)
    with pytest.raises(RuntimeError, match="zeggs_live_plant_prepare: plant prepare: " + match):
        api.zeggs_live_plant_prepare(d, parents, (ctypes.c_int * 6)(*chains), STATE, 88 + 4 * 352, None)
    with pytest.raises(RuntimeError, match=r"parents\[3\] = 5"):
        api.zeggs_live_plant_prepare(d, (ctypes.c_int * 9)(-1, 0, 1, 5, 3, 0, 5, 6, 7), (ctypes.c_int * 6)(1, 2, 3, 5, 6, 7), STATE, 88 + 4 * 352, None)
    with pytest.raises(RuntimeError, match="NULL parents / chains"):
        api.zeggs_live_plant_prepare(d, parents, None, STATE, 88 + 4 * 352, None)


@pytest.mark.parametrize("what,rows,dev,match", [
    ("a row out of range", [dict(row=4)], None, "record 0: row 4 of 4"),
    ("a negative row", [dict(row=0), dict(row=-1)], 0x7000, "record 1: row -1 of 4"),
    ("a row twice", [dict(row=2), dict(row=1), dict(row=2)], 0x7000, "record 2: row 2 twice"),
    ("a negative count", [dict(count=-1)], None, "record 0: negative count -1"),
    ("too many frames", [dict(count=9)], None, "record 0: 9 frames, max_frames is 8"),
    ("a NULL source", [dict(row=1), dict(row=0, rpos=None)], 0x7000, "record 1: NULL or misaligned source"),
    ("a misaligned source", [dict(pose=0x10002)], None, "record 0: NULL or misaligned source"),
    ("a short pose row", [dict(pose_ld=140)], None, r"record 0: leading dimensions 140, 3, 4 \(at least 141, 3, 4 floats\)"),
    ("a short root row", [dict(rrot_ld=3)], None, "record 0: leading dimensions 141, 3, 3"),
    ("a NULL destination", [dict(out=None)], None, "record 0: NULL or misaligned destination"),
    ("the source as the destination", [dict(out=0x10000)], None, "record 0: the destination is the source"),
    ("a short destination row", [dict(out_ld=100)], None, "record 0: destination leading dimension 100"),
    ("NULL contact flags", [dict(contacts=None)], None, "record 0: NULL contact flags"),
    ("two records without a device copy", [dict(row=0), dict(row=1)], None, "must also be in device memory"),
    ("a misaligned device copy", [dict(row=0), dict(row=1)], 0x7004, "misaligned recs_dev"),
    ("more records than rows", [dict(row=i % 4) for i in range(5)], 0x7000, "5 records for 4 rows"),
])
def test_plant_refuses_on_the_host(what, rows, dev, match):
    """every refusal comes before the launch (the addresses are never followed, there is no device here), with the record named"""
    d, arr = _dims(), _recs(*rows)
    dev_p = ctypes.cast(ctypes.c_void_p(dev), ctypes.POINTER(capi.PlantRow)) if dev else None
    with pytest.raises(RuntimeError, match="zeggs_live_plant: plant: .*" + match):
        capi.api().zeggs_live_plant(d, arr, dev_p, len(rows), STATE, 88 + 4 * 352, None)
    assert ops.lib().zeggs_live_plant(ctypes.byref(d), arr, ctypes.c_void_p(dev or 0), len(rows), STATE, ctypes.c_size_t(88 + 4 * 352), None) == -1


def test_plant_entry_points_check_state_and_row():
    api, d = capi.api(), _dims()
    with pytest.raises(RuntimeError, match="state too small"):
        api.zeggs_live_plant(d, _recs({}), None, 1, STATE, 88 + 4 * 352 - 1, None)
    with pytest.raises(RuntimeError, match="NULL state"):
        api.zeggs_live_plant_reset(d, None, 88 + 4 * 352, 0, None)
    with pytest.raises(RuntimeError, match="misaligned state"):
        api.zeggs_live_plant_reset(d, ctypes.c_void_p(0x900004), 88 + 4 * 352, 0, None)
    with pytest.raises(RuntimeError, match="reset: row 4 of 4"):
        api.zeggs_live_plant_reset(d, STATE, 88 + 4 * 352, 4, None)
    with pytest.raises(RuntimeError, match="NULL records"):
        api.zeggs_live_plant(d, None, None, 1, STATE, 88 + 4 * 352, None)
    # nothing to do: no launch, no error
    assert api.zeggs_live_plant(d, None, None, 0, STATE, 88 + 4 * 352, None) == 0
    assert api.zeggs_live_plant(d, _recs(dict(count=0, pose=None)), None, 1, STATE, 88 + 4 * 352, None) == 0


# ----------------------------------------------------------------------------- 5. the snapshot's fingerprint
def test_the_fingerprint_grows_only_with_plant():
    """a blob of a server without `plant` has the header it always had (len(SNAP_FINGERPRINT) fields); one with `plant` carries
    SNAP_FINGERPRINT_PLANT's fields behind them, and the two kinds do not restore into each other: the field counts differ"""
    sizes = [0] * len(live.SNAP_SECTIONS)
    sizes[live.SNAP_SECTIONS.index("row")] = 8 * len(live.SNAP_ROW)
    plain = {k: float(i) for i, k in enumerate(live.SNAP_FINGERPRINT)}
    planted = dict(plain, **{k: float(100 + i) for i, k in enumerate(live.SNAP_FINGERPRINT_PLANT)})
    a = live.snapshot_build(5, 1, plain, dict(row=np.zeros(len(live.SNAP_ROW), "<i8")))
    b = live.snapshot_build(5, 1, planted, dict(row=np.zeros(len(live.SNAP_ROW), "<i8")))
    assert len(b) >= len(a) + 8 * len(live.SNAP_FINGERPRINT_PLANT) - 15
    ia, ib = live.snapshot_info(a), live.snapshot_info(b)
    assert ia["fingerprint"] == plain and ib["fingerprint"] == planted and list(ib["fingerprint"]) == [*live.SNAP_FINGERPRINT, *live.SNAP_FINGERPRINT_PLANT]
    assert live.snapshot_layout(sizes) == live.snapshot_layout(sizes, len(live.SNAP_FINGERPRINT))
    live.snapshot_check_fingerprint(ia["fingerprint"], plain)
    live.snapshot_check_fingerprint(ib["fingerprint"], planted)
    with pytest.raises(ValueError, match="taken from a server with plant, this one has none"):
        live.snapshot_check_fingerprint(ib["fingerprint"], plain)
    with pytest.raises(ValueError, match="taken from a server without plant"):
        live.snapshot_check_fingerprint(ia["fingerprint"], planted)
    with pytest.raises(ValueError, match="plant_slack = 106.0, this one has plant_slack = 7.0"):
        live.snapshot_check_fingerprint(ib["fingerprint"], dict(planted, plant_slack=7.0))
    assert {"plant_chains", "plant_v_on", "plant_v_off", "plant_h_on", "plant_h_off", "plant_ground", "plant_slack", "plant_release",
            "plant_stretch"} == set(live.SNAP_FINGERPRINT_PLANT)
