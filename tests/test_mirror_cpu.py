"""Left/right mirroring without a GPU: the tables of zeggs/anim.py (mirror_pairs, mirror_table, the named layouts) against the float64
oracle (oracle/anim.py, unchanged), the table check on the host (tests/host/mirror_table_check.cpp over csrc/mirror_table.h, plain and
under the sanitizers), include/zeggs_hip_mirror.h against zeggs/capi.py, and the conf key of the dataset builder.

The statement under test: with the mirror plane x = 0, a mirrored take is the original with paired joints exchanged, x positions and
the angles about y and z negated -- and every feature array of the mirrored take is the signed, joint-permuted array of the original:
a permutation plus sign flips, no arithmetic.  The oracle computes both sides in float64; they must be EQUAL in every value (IEEE
equality: a zero's sign is the one thing a sum like 0 - 0 x does not carry through a reflection, and no consumer reads it), for the
16 arrays, in three channel orders, on a rig whose left and right offsets are deliberately not reflections of each other.
"""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import anim as oa
from zeggs import anim, capi, data_pipeline, synth

ROOT = Path(__file__).resolve().parent.parent
FEATURES = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "lrot", "ltxy", "lvel", "lvrt", "cpos", "crot", "ctxy", "cvel", "cvrt",
            "gaze_pos", "gaze_dir")                     # the order of preprocess_animation's tuple
NAMES = ["Hips", "Spine", "Spine2", "Neck", "Head", "HeadEnd", "LeftShoulder", "LeftArm", "RightShoulder", "RightArm", "LeftUpLeg",
         "LeftLeg", "RightUpLeg", "RightLeg"]
PARENTS = [-1, 0, 1, 2, 3, 4, 2, 6, 2, 8, 0, 10, 0, 12]
PAIRS = [0, 1, 2, 3, 4, 5, 8, 9, 6, 7, 12, 13, 10, 11]
ORDERS = ("zyx", "xzy", "yzx")


def rig_take(order, frames=40, seed=3):
    """14 joints: Hips, Spine2, Head, an unsided leaf, arm pairs at depth 3 / 4 and leg pairs at depth 1 / 2; the offsets of a pair are
    NOT reflections of each other (up to 4 % of the bone)"""
    rng = np.random.default_rng(seed)
    J = len(NAMES)
    off = rng.normal(0.0, 10.0, (J, 3))
    for j, p in enumerate(PAIRS):
        if p > j:
            off[p] = off[j] * np.array([-1.0, 1.0, 1.0]) * (1.0 + rng.uniform(-0.04, 0.04, 3))
        elif p == j:
            off[j, 0] = 0.01 * np.linalg.norm(off[j, 1:])     # (an unsided joint a little off the plane)
    off[0] = [0.0, 90.0, 0.0]
    t = np.linspace(0.0, 1.0, frames)[:, None, None]
    rot = rng.normal(0.0, 40.0, (1, J, 3)) + 70.0 * np.sin(2 * np.pi * (t * rng.uniform(0.5, 2.0, (1, J, 3)) + rng.uniform(0, 1, (1, J, 3))))
    pos = np.repeat(off[None], frames, axis=0)
    pos[:, 0] += np.cumsum(rng.normal(0.0, 0.8, (frames, 3)), axis=0)
    return dict(rotations=rot, positions=pos, offsets=off, parents=np.asarray(PARENTS, np.int32), names=list(NAMES), order=order,
                frametime=1.0 / 60.0)


def same_values(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.isfinite(a).all()) and np.array_equal(a, b)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_CACHE = {}


def both_sides(order):
    """-> (features of the original, features of the mirrored take), the oracle's float64 / float32 arrays; computed once"""
    if order not in _CACHE:
        take = rig_take(order)
        _CACHE[order] = (oa.preprocess_animation(take), oa.preprocess_animation(anim.mirror_take(take)))
    return _CACHE[order]


def commutes(order, table_of):
    """per feature: is the mirrored take's array the table applied to the original's"""
    plain, mirrored = both_sides(order)
    return {n: same_values(anim.mirror_rows_host(a, table_of(n)), b) for n, a, b in zip(FEATURES, plain, mirrored)}


# ----------------------------------------------------------------------------- 1. the features commute with the mirror
@pytest.mark.parametrize("order", ORDERS)
def test_features_of_the_mirrored_take_are_the_table_applied_to_the_features(order):
    pairs = anim.mirror_pairs(NAMES, PARENTS)
    assert pairs == PAIRS
    take = rig_take(order)
    assert 0.0 < anim.mirror_take(take)["asymmetry"] < 0.2
    ok = commutes(order, lambda n: anim.mirror_table(n, pairs))
    assert all(ok.values()), [n for n, v in ok.items() if not v]
    plain, mirrored = both_sides(order)
    for n, a, b in zip(FEATURES, plain, mirrored):             # bit for bit, except the sign of a zero: nothing else may differ
        via = anim.mirror_rows_host(a, anim.mirror_table(n, pairs))
        bits = {4: np.uint32, 8: np.uint64}[via.dtype.itemsize]
        differ = via.view(bits) != np.ascontiguousarray(b).view(bits)
        assert ((via == 0.0) & (b == 0.0))[differ].all(), n
    assert sum(not same_values(a, b) for a, b in zip(plain, mirrored)) == 16          # (the reflection changes every array)


@pytest.mark.parametrize("order", ORDERS)
def test_wrong_tables_do_not_commute(order):
    """the negative controls: a vector signed as a pseudo-vector, a pair left unswapped, an Euler sign by the channel's place"""
    pairs = anim.mirror_pairs(NAMES, PARENTS)

    def swapped_kind(n):          # vec <-> axial
        (kind, scope), = anim.named_layout(n)
        return anim.mirror_table([({"vec": "axial", "axial": "vec"}.get(kind, kind), scope)], pairs)
    ok = commutes(order, swapped_kind)
    assert not any(ok[n] for n in FEATURES if anim.named_layout(n)[0][0] in ("vec", "axial")), ok
    unswapped = list(pairs)
    unswapped[6], unswapped[8] = 6, 8              # the shoulders stay where they are
    ok = commutes(order, lambda n: anim.mirror_table(n, unswapped))
    assert not any(ok[n] for n in ("lpos", "lrot", "ltxy", "lvrt", "cpos", "crot", "ctxy", "cvel", "cvrt")), ok     # (lvel: 0 below the root)
    # the take itself, mirrored with the sign of channel i taken from i and not from the axis letter: (+, -, -) whatever the order
    take = rig_take(order)
    good = anim.mirror_take(take)
    by_place = anim.mirror_rows_host(take["rotations"], anim.mirror_table([("axial", "joint")], pairs))
    if order == "xzy":           # x is the first channel there: place and letter give the same signs
        assert same_values(by_place, good["rotations"])
        return
    assert not same_values(by_place, good["rotations"])
    wrong = dict(zip(FEATURES, oa.preprocess_animation(dict(good, rotations=by_place))))
    right = dict(zip(FEATURES, both_sides(order)[1]))
    differ = [n for n in FEATURES if not same_values(wrong[n], right[n])]
    print(order, "an Euler sign by place changes", differ)
    assert {"lrot", "ltxy", "lvrt", "cpos", "crot", "ctxy"} <= set(differ)


@pytest.mark.parametrize("order", ORDERS)
def test_world_positions_of_the_mirrored_take_are_the_reflected_partners(order):
    """geometry, without the tables: float64 forward kinematics of the mirrored channels against the x-negated world positions of the
    partner joints of the original.  Bound: a level of the chain is a rotation of a vector and a sum (<= 16 roundings of 2^-53
    relative to the lengths involved), so depth x 16 x 2^-53 x (the root's distance + the chain's bone lengths).  The rig is NOT
    symmetric: joint j of the mirrored take hangs on the reflected bone of its partner, so it lands on the partner's reflection"""
    take = rig_take(order)
    fk = lambda t: oa.q_fk(oa.q_from_euler(np.radians(t["rotations"]), t["order"]), t["positions"].copy(), t["parents"])[1]  # noqa: E731
    got = fk(anim.mirror_take(take))
    want = fk(take)[:, PAIRS] * np.array([-1.0, 1.0, 1.0])
    assert float(np.abs(got - fk(take)).max()) > 1.0
    depth = [0] * len(PARENTS)
    for j in range(1, len(PARENTS)):
        depth[j] = depth[PARENTS[j]] + 1
    reach = np.abs(take["positions"][:, 0]).max() + np.linalg.norm(take["offsets"][1:], axis=-1).sum()
    bound = (max(depth) + 1) * 16 * 2.0 ** -53 * reach
    err = float(np.abs(got - want).max())
    print(f"{order}: world positions differ by {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ----------------------------------------------------------------------------- 2. involution, pairing errors, edge cases
def test_twice_is_the_identity_bit_for_bit():
    rng = np.random.default_rng(5)
    for order in ORDERS:
        take = rig_take(order)
        take["rotations"][3, 2] = [-0.0, np.inf, np.nan]
        back = anim.mirror_take(anim.mirror_take(take))
        assert all(same_bits(back[k], take[k]) for k in ("rotations", "positions", "offsets"))
        assert back["names"] == take["names"] and back["order"] == order and back["frametime"] == take["frametime"]
    pairs75 = anim.mirror_pairs(synth.BONE_NAMES, synth.PARENTS)
    for pairs, J in ((PAIRS, 14), (pairs75, 75)):
        for name in FEATURES + tuple("Y_" + n for n in FEATURES) + ("rotations", "positions", "decoder_in", "decoder_out", "example"):
            table = anim.check_mirror_table(anim.mirror_table(name, pairs, order="yzx"))
            for dt in (np.float32, np.float64):
                x = rng.standard_normal((5, table.size)).astype(dt)
                x[0, 0], x[1, -1] = -0.0, np.nan
                once = anim.mirror_rows_host(x, table)
                assert same_bits(anim.mirror_rows_host(once, table), x), name
                assert name in ("root_rot",) or not same_bits(once, x) or table.size < 3, name
    assert anim.mirror_table("decoder_in", pairs75).size == synth.POSE_IN and anim.mirror_table("decoder_out", pairs75).size == synth.POSE_OUT
    assert anim.mirror_table("example", pairs75).size == synth.POSE_IN and anim.mirror_table("Y_ltxy", pairs75).size == 6 * synth.NJ


def test_table_entries_are_source_and_sign():
    t = anim.mirror_table([("vec", "single"), ("quat", "joint"), ("same", "single", 2), ("euler:yzx", "joint")], [1, 0]).view(np.uint32)
    src, neg = (t & 0x7FFFFFFF).tolist(), (t >> 31).tolist()
    assert src == [0, 1, 2, 7, 8, 9, 10, 3, 4, 5, 6, 11, 12, 16, 17, 18, 13, 14, 15]
    assert neg == [1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 1, 1, 0]
    assert anim.segment_signs("txy") == (1, -1, -1, -1, 1, 1) and anim.segment_signs("euler:xzy") == (1, -1, -1)
    with pytest.raises(ValueError, match="unknown segment kind"):
        anim.mirror_table([("spinor", "joint")], [0])
    with pytest.raises(ValueError, match="not a rotation channel order"):
        anim.mirror_table([("euler:xxy", "joint")], [0])
    with pytest.raises(ValueError, match="no row layout called"):
        anim.mirror_table("Y_audio", [0])


def test_pairing_errors_name_the_joint():
    with pytest.raises(ValueError, match="'LeftArm' has no partner \\('RightArm' is not a joint\\)"):
        anim.mirror_pairs(NAMES[:9], PARENTS[:9])
    moved = list(PARENTS)
    moved[9] = 2                                    # RightArm hangs under Spine2, LeftArm under LeftShoulder
    with pytest.raises(ValueError, match="not an automorphism"):
        anim.mirror_pairs(NAMES, moved)
    with pytest.raises(ValueError, match="'LeftArm'|'RightArm'"):
        anim.mirror_pairs(NAMES, moved)
    assert anim.resolve_pairs({"LeftShoulder": "RightShoulder", "LeftArm": "RightArm", 10: 12, 11: 13}, NAMES, PARENTS) == PAIRS
    assert anim.resolve_pairs(PAIRS, NAMES, PARENTS) == PAIRS and anim.resolve_pairs("auto", NAMES, PARENTS) == PAIRS
    with pytest.raises(ValueError, match="pairs with"):
        anim.resolve_pairs([1, 2, 0] + list(range(3, 14)), NAMES, PARENTS)
    assert anim.mirror_pairs(["Root", "L_Hand", "R_Hand"], [-1, 0, 0], left="L_", right="R_") == [0, 2, 1]


def test_only_the_x_plane():
    take = rig_take("zyx", frames=4)
    for call in (lambda: anim.mirror_pairs(NAMES, PARENTS, axis="y"), lambda: anim.mirror_table("lpos", PAIRS, axis="y"),
                 lambda: anim.mirror_take(take, axis="z"), lambda: anim.mirror_rows(None, "lpos", PAIRS, axis="y")):
        with pytest.raises(NotImplementedError, match="x = 0"):
            call()


def test_asymmetry_is_reported_and_refused_on_request():
    take = rig_take("zyx", frames=4)
    a = anim.mirror_take(take)["asymmetry"]
    assert a == anim.rig_asymmetry(take["offsets"], PAIRS) and 0.0 < a < 0.2
    assert anim.mirror_take(take, symmetry_tol=a)["asymmetry"] == a
    with pytest.raises(ValueError, match="asymmetry"):
        anim.mirror_take(take, symmetry_tol=a / 2)
    sym = dict(take, offsets=take["offsets"].copy())
    for j, p in enumerate(PAIRS):
        sym["offsets"][j] = take["offsets"][min(j, p)] * ([1.0, 1.0, 1.0] if j <= p else [-1.0, 1.0, 1.0])
        if j == p:
            sym["offsets"][j, 0] = 0.0
    assert anim.mirror_take(sym, symmetry_tol=0.0)["asymmetry"] == 0.0
    m = anim.mirror_take(take)
    assert same_bits(m["offsets"], take["offsets"][PAIRS] * np.array([-1.0, 1.0, 1.0]))


def test_the_bijection_check_of_the_library():
    """zeggs_mirror_table_check and zeggs_mirror_plan_create refuse before anything touches a device (there is none here)"""
    api = capi.api()
    arr = lambda *v: np.asarray(v, dtype=np.uint32).view(np.int32)  # noqa: E731
    assert api.zeggs_mirror_version() == 1
    assert api.zeggs_mirror_table_check(arr(1, 0 | 0x80000000, 2).ctypes.data, 3) == 0
    for bad, msg in ((arr(0, 0, 2), "column 1: source 0 is also the source of column 0"), (arr(0, 3, 1), "column 1: source 3 of 3 columns"),
                     (arr(0x80000001, 1), "column 1: source 1 is also the source of column 0")):
        with pytest.raises(RuntimeError, match="zeggs_mirror_table_check: mirror table: " + msg):
            api.zeggs_mirror_table_check(bad.ctypes.data, int(bad.size))
        with pytest.raises(ValueError, match=msg):
            anim.check_mirror_table(bad)
        plan = ctypes.c_void_p(123)
        with pytest.raises(RuntimeError, match="zeggs_mirror_plan_create: mirror table: " + msg):
            api.zeggs_mirror_plan_create(bad.ctypes.data, int(bad.size), ctypes.addressof(plan))
        assert plan.value is None
    big = np.arange(3073, dtype=np.int32)
    with pytest.raises(RuntimeError, match="3073 columns \\(1..3072\\)"):
        api.zeggs_mirror_table_check(big.ctypes.data, 3073)
    with pytest.raises(RuntimeError, match="not a plan"):
        api.zeggs_mirror_rows(None, None, None, 1, 4, None)
    assert api.zeggs_mirror_plan_free(None) == 0


def _cxx():
    return shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_table_check_on_the_host(tmp_path, flags):
    """tests/host/mirror_table_check.cpp: a stand-alone program over the header the library uses (its head says what it walks); once
    plain, once under the address and undefined-behaviour sanitizers (host code with its own main, run directly)"""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "mirror_table_check"
    b = subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Wextra", "-o", str(exe), str(ROOT / "tests" / "host" / "mirror_table_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "mirror_table_check: ok"


def test_prototypes_are_the_twelfth_header():
    """capi.MR_PROTOTYPES against include/zeggs_hip_mirror.h: the same names, disjoint from every other group, the parameter counts
    and return kinds; the library exports them; zeggs_version() is what it was; the unit and the header are in build.sh"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "zeggs_hip_mirror.h").read_text(), flags=re.S)
    header = {name: (ret.strip(), [] if params.strip() in ("", "void") else params.split(","))
              for ret, name, params in re.findall(r"([A-Za-z_][\w \*]*?)\b(zeggs_\w+)\s*\(([^()]*)\)\s*;", text)}
    assert set(header) == set(capi.MR_PROTOTYPES) and len(header) == 6
    others = [g for g in dir(capi) if g.endswith("PROTOTYPES") and g != "MR_PROTOTYPES"]
    assert len(others) == 11 and not set(capi.MR_PROTOTYPES) & {n for g in others for n in getattr(capi, g)}
    for name, (ret, params) in header.items():
        kind, kinds = capi.signature(name)
        assert ret == "int" and kind in ("status", "mask", "int") and len(kinds) == len(params), name
        for p, k in zip(params, kinds):
            assert (k == "int") == (p.split()[0] == "int" and "*" not in p) and (k == "long") == (p.split()[0] == "long"), (name, p, k)
        assert hasattr(capi.raw(), name)
    assert capi.api().zeggs_version() == 109
    assert int(re.search(r"#define ZEGGS_MIRROR_MAX_COLS (\d+)", text).group(1)) == 3072
    build = (ROOT / "ubisoft-laforge-zeroeggs_amd" / "csrc" / "build.sh").read_text()
    assert " mirror " in build and "../../include/zeggs_hip_mirror.h" in build


# ----------------------------------------------------------------------------- 3. the conf key of the dataset builder
def test_a_conf_without_mirror_is_untouched_and_a_malformed_one_is_refused(tmp_path):
    conf = synth.pipeline_conf(tmp_path)
    before = repr(conf)
    data_pipeline.check_conf(conf)
    assert repr(conf) == before and "mirror" not in conf and data_pipeline.mirror_options(conf) is None
    assert data_pipeline.mirror_options(dict(conf, mirror=False)) is None
    assert data_pipeline.mirror_options(dict(conf, mirror=True)) == dict(suffix="_mirror", pairs="auto")
    assert data_pipeline.mirror_options(dict(conf, mirror={"suffix": "_m", "pairs": {"LeftArm": "RightArm"}})) == dict(suffix="_m", pairs={"LeftArm": "RightArm"})
    for bad in ("yes", 1, ["_mirror"], {"sufix": "_m"}, {"suffix": ""}, {"suffix": 3}, {"suffix": "_m.bvh"}, {"pairs": "left"}, {"pairs": [0, 1.5]},
                {"pairs": {"LeftArm": None}}):
        with pytest.raises(ValueError, match="mirror"):
            data_pipeline.check_conf(dict(conf, mirror=bad))
    assert not (tmp_path / "processed").exists()                  # refused before anything is written


def test_which_rows_get_a_mirrored_take():
    info = [dict(anim_bvh=n) for n in ("a.bvh", "b.bvh", "b_mirror.bvh", "c_mirror.bvh", "d.bvh")]
    assert data_pipeline.mirror_plan_of_info(info, "_mirror") == ["a_mirror.bvh", None, None, None, "d_mirror.bvh"]
    assert data_pipeline.mirrored_name("001_Neutral_0.bvh", "_mirror") == "001_Neutral_0_mirror.bvh"
    assert data_pipeline.trimmed_name(data_pipeline.mirrored_name("a.bvh", "_mirror"), 0.9) == "a_mirror_x_0_9"


def test_cli_mirror_switches(tmp_path, monkeypatch):
    """`prepare --mirror` sets the conf key the builder reads (and leaves a conf without the switch as it is); `generate
    --mirror-style` reaches generate_gesture() and, with --batch, every Job (all stubbed: no GPU)"""
    import json
    from zeggs import cli
    import zeggs.generate as zg
    seen = []
    monkeypatch.setattr(data_pipeline, "data_pipeline", lambda conf, **k: seen.append(conf))
    cf = tmp_path / "c.json"
    cf.write_text(json.dumps(synth.pipeline_conf(tmp_path)))
    assert cli.main(["prepare", "-c", str(cf)]) == 0 and cli.main(["prepare", "-c", str(cf), "--mirror"]) == 0
    assert "mirror" not in seen[0] and seen[1]["mirror"] is True and data_pipeline.mirror_options(seen[1]) == dict(suffix="_mirror", pairs="auto")
    calls = []
    monkeypatch.setattr(zg, "generate_gesture", lambda **k: calls.append(k))
    monkeypatch.setattr(zg, "generate_gestures", lambda jobs, **k: calls.append(jobs))
    of = tmp_path / "o.json"
    of.write_text(json.dumps({"train_opt": {"resume": False}, "net_opt": {},
                              "paths": {"base_path": str(tmp_path), "path_processed_data": "data", "output_dir": str(tmp_path / "out"),
                                        "models_dir": str(tmp_path / "models")}}))
    base = ["generate", "-o", str(of), "-s", "ex.bvh", "-a", "a.wav"]
    assert cli.main(base) == 0 and cli.main(base + ["--mirror-style"]) == 0
    assert calls[0]["mirror_style"] is False and calls[1]["mirror_style"] is True
    assert cli.main(base + ["-b", "2"]) == 0 and cli.main(base + ["-b", "2", "--mirror-style"]) == 0
    assert [j.mirror_style for j in calls[2]] == [False] and [j.mirror_style for j in calls[3]] == [True]
