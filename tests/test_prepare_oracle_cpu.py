"""tests/prepare_oracle.py against itself (no GPU): known answers of the float64 restatements, every mutation of PREPARE_BUGS seen by
its named case at 10 bounds or more (a differing element for the bit-exact audio output), and the loudness signals hold what their
names claim.  The bounds are those tests/test_gpu_prepare_kernels.py holds the kernels to."""
import numpy as np
import pytest

import prepare_oracle as po
from oracle import anim as oanim
from oracle import loudness as olo
from zeggs import audio
from zeggs import data_pipeline as dp


def by_id(table, id):
    return next(c for c in table if c["id"] == id)


def test_tables_have_unique_ids_and_cover_what_they_name():
    for table in (po.AUDIO_CASES, po.CENTER_CASES, po.ROT_CASES, po.STATS_CASES, po.LOUD_CASES):
        ids = [c["id"] for c in table]
        assert len(set(ids)) == len(ids)
    assert {c["r"] for c in po.STATS_CASES} == {1, 2047, 2048, 2049, 4096, 6150}
    assert {c["d"] for c in po.STATS_CASES} == {1, 2, 5, 33, 64, 65, 130}
    assert {c["mask"] for c in po.STATS_CASES} == {"all", "one", "mid-slab-out", "first-slab-out", "ranges"}
    assert {po.stats_tcol(c["d"]) for c in po.STATS_CASES} == {1, 2, 8, 64}
    assert {c["j"] for c in po.ROT_CASES} == {1, 2, 3, 16, 17, 75}
    assert {c["n"] for c in po.ROT_CASES} == {"4", "5", "6", "C+3", "C+4", "C+5", "2C+H+5"}
    assert {c["m"] for c in po.ROT_CASES} == {"1", "2", "N", "2N-1", "0.9N", "1.1N"}
    for j in (1, 2, 3, 16, 17, 75):
        mine = [c for c in po.ROT_CASES if c["j"] == j]
        assert any(c["n"] in po.ROT_MULTI_CHUNK for c in mine) and any(c["m"] != "N" for c in mine), j
    big = by_id(po.AUDIO_CASES, "grid-stride")
    assert min(big["end"], big["n"]) - big["start"] > po.GRID_EDGE
    assert len(by_id(po.AUDIO_CASES, "k4096")["intervals"]) == po.AUDIO_MAX_INTERVALS


# ----------------------------------------------------------------------------- known answers
def test_silence_cut_with_one_interval_over_everything_is_the_plain_slice():
    case = by_id(po.AUDIO_CASES, "one")
    w = po.audio_wav(case)
    assert np.signbit(w[w == 0.0]).any() and not np.signbit(w[w == 0.0]).all()
    got = po.silence_cut(w, [[0, len(w)]], 1000, 8000)
    assert np.array_equal(got.view(np.uint32), w[1000:8000].view(np.uint32))
    assert len(po.silence_cut(w, [[0, len(w)]], 9000, len(w) + 500)) == len(w) - 9000
    assert not po.silence_cut(w, [], 0, len(w)).any()


@pytest.mark.parametrize("case", po.CENTER_CASES, ids=[c["id"] for c in po.CENTER_CASES])
def test_center_inputs_and_known_answers(case):
    pos, rot = po.center_inputs(case)
    order = case["order"]
    # the inputs: the Euler angles say the rotation they were made from, and no middle angle comes near the gimbal
    heading, pitch, roll = po.CENTER_ROOTS[case["root"]]
    q0 = oanim.q_from_euler(np.radians(rot[0, 0]), order)
    want = oanim.q_mul(po.axis_quat(-heading if (case["root"] == "yaw" and case["n"] % 2) else heading, "y"),
                       oanim.q_mul(po.axis_quat(pitch, "x"), po.axis_quat(roll, "z")))
    assert min(np.abs(q0 - want).max(), np.abs(q0 + want).max()) < 1e-12
    assert np.abs(po.middle_angle(rot)).max() <= 70.0
    new_p, new_r = po.center(pos, rot, order, 0)
    assert np.abs(po.asin_angle(new_r[:, 0], order)).max() <= 70.0
    # frame 0's root lands on the y axis, at its own height
    assert new_p[0, 0, 0] == 0.0 and new_p[0, 0, 2] == 0.0 and new_p[0, 0, 1] == pos[0, 0, 1]
    assert np.array_equal(new_p[:, 1:], pos[:, 1:]) and np.array_equal(new_r[:, 1:], rot[:, 1:])
    off = q0 * np.array([1.0, 0.0, 1.0, 0.0])
    s = float(off @ off)
    f = po.center_horizontal_factor(off)
    d_in, d_out = pos[:, 0] - pos[:1, 0], new_p[:, 0] - new_p[:1, 0]
    hor = lambda d: np.hypot(d[:, 0], d[:, 2])  # noqa: E731
    assert np.allclose(d_out[:, 1], d_in[:, 1], rtol=0, atol=1e-10)
    assert np.allclose(hor(d_out), f * hor(d_in), rtol=1e-12, atol=1e-10)
    if case["root"] == "upright":          # pure yaw at frame 0: (w, 0, y, 0) is the whole unit quaternion, the centring is rigid
        assert abs(s - 1.0) < 1e-12 and abs(f - 1.0) < 1e-12
    if case["root"] == "tilted":           # 40 degrees of pitch, 25 of roll: |o| ~ 0.9, horizontal distances shrink by f (not by |o|^2)
        assert 0.88 < np.sqrt(s) < 0.94 and abs(f - np.sqrt(1.0 - 4.0 * off[2] ** 2 * (1.0 - s))) < 1e-15
        assert 0.9 < f < 0.97 and abs(f - s) > 0.05
    if case["root"] == "yaw":
        assert abs(heading) > 90.0
    r32_p, r32_r = po.center(pos, rot, order, 1)
    assert np.array_equal(r32_p[:, 0], new_p[:, 0].astype(np.float32).astype(np.float64))
    assert np.array_equal(r32_r[:, 0], new_r[:, 0].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("case", po.ROT_CASES, ids=[c["id"] for c in po.ROT_CASES])
def test_rot_inputs_turn_and_cross(case):
    c, h, _ = dp.spline_chunk()
    n, m = po.rot_sizes(case, c, h)
    e = po.rot_inputs(case, n)
    j = case["j"]
    assert e.shape == (n, j, 3) and np.abs(e[:, :, 1:]).max() <= 70.0
    jump = np.diff(e[:, j - 1, 0])
    assert (jump < -180.0).any() and (j == 1 or (jump > 180.0).any())       # (a wrap: the step minus a turn)
    for order in ("zyx", "xzy"):
        out, q = po.rot_stretch(e, m, order, with_quats=True)
        assert out.shape == (m, j, 3)
        assert np.any(q[:, 0, 0] < -0.5) and np.any(q[:, j - 1, 0] < 0.0)


def test_masked_stats_known_answers():
    x = np.array([[1.0, 5.0], [2.0, 5.0], [9.0, 9.0], [3.0, 5.0]], dtype=np.float32)
    mean, std, pooled = po.masked_stats(x, np.array([1, 1, 0, 1], dtype=bool))
    assert np.array_equal(mean, [2.0, 5.0]) and std[1] == 0.0 and abs(std[0] - np.sqrt(2.0 / 3.0)) < 1e-15
    assert abs(pooled[0] - np.std([1.0, 2.0, 3.0, 5.0, 5.0, 5.0])) < 1e-15
    for case in po.STATS_CASES:
        x, mask = po.stats_inputs(case)
        mean, std, pooled = po.masked_stats(x, mask)
        sel = x[mask].astype(np.float64)
        assert mask.any() and np.allclose(mean, sel.mean(axis=0), rtol=1e-14, atol=0) and np.allclose(std, sel.std(axis=0), rtol=1e-9, atol=1e-12)
        assert np.allclose(pooled, sel.std(), rtol=1e-12, atol=0)
        if case["d"] > 1:
            assert std[1] == 0.0
        if case["r"] > 1 and mask.sum() > 1:
            assert abs(mean[0] - 1e4) < 1.0 and 1e-3 < std[0] < 3e-2
        nslab = -(-case["r"] // po.STATS_SLAB)
        empty = [b for b in range(nslab) if not mask[b * po.STATS_SLAB:(b + 1) * po.STATS_SLAB].any()]
        assert bool(empty) == (case["mask"] in ("mid-slab-out", "first-slab-out") or case["id"] == "R2049-D1-one"), case["id"]


# ----------------------------------------------------------------------------- loudness
@pytest.mark.parametrize("case", po.LOUD_CASES, ids=[c["id"] for c in po.LOUD_CASES])
def test_loudness_restatement_is_the_meter_and_the_signals_hold_what_they_claim(case):
    x = po.loud_signal(case)
    rate = case["rate"]
    assert len(x) == case["n"] and np.array_equal(x, x.astype(np.float32).astype(np.float64))
    lo, _ = audio.gating_blocks(len(x), rate)
    z = po.block_energies(x, rate)
    assert len(z) == len(lo)
    if case["id"] in ("rate-8000", "n-3200", "chunk-64", "blocks-1025"):       # (the Meter's own loop is slow: one case of each kind)
        for dt in (np.float64, np.float32):
            assert po.loudness(x.astype(dt), rate) == olo.Meter(rate).integrated_loudness(x.astype(dt))
    lv, gamma = po.block_levels(z), po.relative_gate(z)
    under, between, over = lv < -70.0, (lv >= -70.0) & (lv <= gamma), (lv > gamma) & (lv > -70.0)
    assert over.any() and np.isfinite(po.gated_loudness(z))
    if case["id"] == "n-3200":
        assert len(z) == 1 and -(-len(x) // case["chunk"]) == 1
    if case["kind"] == "speech" and case["n"] >= 2 * rate:
        assert under.any() and between.any()
    if case["kind"] == "gate":
        k = int(case["id"].split("-")[1])
        assert len(z) == k and po.gate_samples(k) == case["n"]
        first = slice(0, po.GATE_STRIDE)
        assert under[first].any() and between[first].any() and over[first].any()
        if k == po.GATE_STRIDE + 1:        # one block past the stride: it can be of one kind only -- the kind that counts
            assert over[po.GATE_STRIDE]
        if k > po.GATE_STRIDE + 1:
            rest = slice(po.GATE_STRIDE, None)
            assert under[rest].any() and between[rest].any() and over[rest].any()


def test_sine_known_answer():
    """a full-scale 997 Hz sine at 48 kHz reads -3.01 LKFS (BS.1770), and 20 dB less of it 20 LU less"""
    full, tenth = po.loudness(po.sine(amplitude=1.0), 48000), po.loudness(po.sine(amplitude=0.1), 48000)
    assert abs(full + 3.01) < po.SINE_TOL and abs(tenth - (full - 20.0)) < 1e-5


def test_gate_tie_sits_on_the_relative_gate():
    lv, gamma = po.block_levels(po.GATE_TIE), po.relative_gate(po.GATE_TIE)
    assert lv[1] == gamma and lv[0] > gamma
    assert po.gated_loudness(po.GATE_TIE) == -0.691 + 10.0 * np.log10(1.9)


# ----------------------------------------------------------------------------- every mutation is seen
def _audio_seen(bug, case):
    w = po.audio_wav(case)
    args = (w, case["intervals"], case["start"], case["end"])
    a, b = po.silence_cut(*args), po.silence_cut(*args, bug=bug)
    return float("inf") if (a.shape != b.shape or not np.array_equal(a, b)) else 0.0


def _center_seen(bug, case):
    pos, rot = po.center_inputs(case)
    (p0, r0), (p1, r1) = po.center(pos, rot, case["order"], 0), po.center(pos, rot, case["order"], 0, bug=bug)
    return max(np.abs(p1 - p0).max() / po.POS_TOL, po.angle_diff(r1, r0).max() / po.DEG_TOL)


def _rot_seen(bug, case):
    c, h, _ = dp.spline_chunk()
    n, m = po.rot_sizes(case, c, h)
    e = po.rot_inputs(case, n)
    return max(po.angle_diff(po.rot_stretch(e, m, order, bug=bug), po.rot_stretch(e, m, order)).max() / po.DEG_TOL for order in ("zyx", "xzy"))


def _stats_seen(bug, case):
    x, mask = po.stats_inputs(case)
    return max(np.max(np.abs(b - a) / po.stats_bound(a)) for a, b in zip(po.masked_stats(x, mask), po.masked_stats(x, mask, bug=bug)))


def _loud_seen(bug, case):
    x = po.loud_signal(case)
    return abs(po.loudness(x, case["rate"], bug, case["chunk"]) - po.loudness(x, case["rate"])) / po.LUFS_TOL64


def _gate_seen(bug, case):
    return abs(po.gated_loudness(po.GATE_TIE, bug) - po.gated_loudness(po.GATE_TIE)) / po.LUFS_TOL64


SEEN = {"audio": (po.AUDIO_CASES, _audio_seen), "center": (po.CENTER_CASES, _center_seen), "rot": (po.ROT_CASES, _rot_seen),
        "stats": (po.STATS_CASES, _stats_seen), "loudness": (po.LOUD_CASES, _loud_seen), "gate": ((dict(id="tie"),), _gate_seen)}


@pytest.mark.parametrize("bug", sorted(po.PREPARE_BUGS))
def test_every_mutation_is_at_least_ten_bounds_away(bug):
    group, case_id = po.PREPARE_BUGS[bug]
    table, seen = SEEN[group]
    distance = seen(bug, by_id(table, case_id))
    print(f"{bug}: case {case_id} lands {distance:.3g} bounds from the clean oracle")
    assert distance >= 10.0


def test_the_issue_s_mutations_are_all_there():
    assert len(po.PREPARE_BUGS) == 15 and {g for g, _ in po.PREPARE_BUGS.values()} == set(SEEN)
