"""The proof that tests/test_gpu_anim_dims.py can fail (no GPU needed): every case it runs meets, on the intermediates of the float64
oracle (oracle/anim.py), the conditions helpers.anim_clip / bvh_case / bvh_pole_case were built for, and a restatement of each
plausible kernel mistake moves the oracle's result by at least 10x the bound the GPU file holds the device to.

Conditions (features): sign flips of consecutive raw quaternions inside the unroll kernel's groups of eight, in its scalar tail and
twice in a row for one joint; no frame-to-frame half turn; the facing direction 10 degrees off -z and reaching +-160; gaze
candidates that change sign in x and z with the middle order statistics more than 1e-3 apart (a y column of N equal values comes
with every clip: root_pos.y = look.y = 0); N bit-equal candidates in the static_head variant; a motionless joint whose lvrt is
exactly 0.  Conditions (BVH rows): at least 8 items in each from_xform branch wherever a case has 32 items or more (the smaller
ones have T J = 1 ... 6 items: the GPU file asserts per branch that HAS items, and that the cases together reach all four); near-pole
rows within 2e-6 of |sin| = 1, exact-pole rows with |sin| > 1 ahead of the clamp.
"""
import numpy as np
import pytest

import helpers as H
from oracle import anim as oa

FACTOR = 10.0
BVH_SHAPES = [(J, T) for J in (1, 3, 65) for T in (1, 2, 300)]


@pytest.mark.parametrize("case", H.ANIM_CASES, ids=H.anim_case_id)
def test_clip_meets_its_conditions(case):
    rig, N, var = case
    clip, R = H.anim_case_clip(case), H.anim_roles(rig)
    I = H.anim_intermediates(clip)
    rot = clip["rotations"]
    assert rot.dtype == np.float64 and (rot > -180.0).all() and (rot <= 180.0).all()
    parents = clip["parents"]
    assert parents[0] == -1 and all(parents[i] < i for i in range(1, len(parents)))
    neg = I["d"] < 0.0                                       # neg[i - 1]: frame i flips against frame i - 1
    group, tail = H.anim_unroll_ranges(N)
    assert len(group) + len(tail) == N - 1
    if len(group):
        assert neg[:8].any(), "no flip inside the first group of eight (frames 1 ... 8)"
        assert all(neg[g - 1:g + 7].any() for g in group[::8]), "a group of eight without a flip"
    if len(tail):
        assert neg[[i - 1 for i in tail]].any(), "no flip in the scalar tail"
    assert (neg[1:] & neg[:-1]).any(), "no joint flips in two consecutive frames"
    assert np.abs(I["d"]).min() > 0.1 and I["rel_w"].min() > 0.1          # far from a half turn between frames: dq_abs has no tie
    assert np.abs(I["facing"]).max() <= 170.0 + 1e-9 and I["look_len"].min() > 0.1
    cand = I["cand"]
    assert (cand[:, 1] == 0.0).all()                         # the column of N equal values
    if var.get("static_head"):
        assert (cand == cand[0]).all()
    else:
        assert I["facing"].min() <= -160.0 and I["facing"].max() >= 160.0
        srt = np.sort(cand, axis=0)
        lo, hi = max((N - 1) // 2 - 1, 0), min(N // 2 + 1, N - 1)
        for c in (0, 2):
            assert cand[:, c].min() < 0.0 < cand[:, c].max(), f"gaze column {c} keeps its sign"
            assert np.diff(srt[lo:hi + 1, c]).min() > 1e-3, f"gaze column {c}: ties around the median"
    ref = H.anim_oracle(clip)
    assert all(np.isfinite(a).all() for a in ref)
    if R["static"] is not None:
        s = R["static"]
        assert (rot[:, s] == rot[0, s]).all() and s != 0
        lvrt = ref[H.ANIM_FEATURES.index("lvrt")]
        assert (lvrt[:, s] == 0.0).all()                     # dq_to_helical at n = 0


def _worst_ratio(ref, bad):
    errs = H.anim_errors(bad, ref)
    return max(errs[n] / H.anim_bound(n) for n in errs)


# (bug, the smallest case that exercises it)
ANIM_CONTROLS = [("no_unroll", ("j3", 4, {})), ("unroll_by_raw_sign", ("j3", 4, {})), ("unroll_by_raw_sign", ("j1", 10, {})),
                 ("median_lower_middle", ("j3", 4, {})), ("median_by_bit_pattern", ("j3", 4, {})),
                 ("median_by_bit_pattern", ("j3", 5, {})), ("hips_spine2_exchanged", ("j3", 4, {})),
                 ("root_vel_same_frame", ("j3", 4, {}))]


@pytest.mark.parametrize("bug,case", ANIM_CONTROLS, ids=lambda v: v if isinstance(v, str) else H.anim_case_id(v))
def test_feature_controls_move_the_oracle(bug, case):
    assert case in H.ANIM_CASES and bug in oa.ANIM_BUGS
    clip = H.anim_case_clip(case)
    ratio = _worst_ratio(H.anim_oracle(clip), H.anim_oracle(clip, bug=bug))
    assert ratio >= FACTOR, (bug, ratio)


def test_unroll_controls_at_every_frame_count():
    """the two wrong unrollings show at every (rig, N) the GPU file runs: each has a joint that flips twice in a row"""
    for case in H.ANIM_CASES:
        clip = H.anim_case_clip(case)
        ref = H.anim_oracle(clip)
        for bug in ("no_unroll", "unroll_by_raw_sign"):
            assert _worst_ratio(ref, H.anim_oracle(clip, bug=bug)) >= FACTOR, (case, bug)


@pytest.mark.parametrize("J,T", BVH_SHAPES)
def test_bvh_rows_reach_every_branch(J, T):
    x = H.bvh_case(J, T, seed=100 * J + T)
    assert all(x[k].dtype == np.float32 for k in ("root_pos", "root_rot", "lpos", "ltxy"))
    counts = np.bincount(x["branch"].ravel(), minlength=4)
    if T * J >= 32:
        assert counts.min() >= 8, counts
    # scaled and sheared: neither row is a unit vector, the two are not orthogonal
    xy = x["ltxy"].astype(np.float64)
    n0, n1 = np.linalg.norm(xy[..., 0, :], axis=-1), np.linalg.norm(xy[..., 1, :], axis=-1)
    assert n0.min() >= 0.29 and n0.max() <= 3.01
    if T * J >= 32:
        assert n0.min() < 0.6 and n0.max() > 2.0
    assert (np.abs(np.sum(xy[..., 0, :] * xy[..., 1, :], axis=-1)) > 0.02 * n0 * n1).all()


def test_bvh_cases_together_reach_every_branch():
    seen = np.zeros(4, int)
    for J, T in BVH_SHAPES:
        seen += np.bincount(H.bvh_case(J, T, seed=100 * J + T)["branch"].ravel(), minlength=4)
    assert seen.min() >= 8, seen
    x = H.bvh_case(64, 4, seed=0)                            # 64 items per group, seed 0: 64 land in each branch
    assert np.bincount(x["branch"].ravel(), minlength=4).tolist() == [64, 64, 64, 64]


def _bvh_moved(x, order, start, bug):
    pos, eul = H.bvh_oracle(x, order, start)
    bpos, beul = H.bvh_oracle(x, order, start, bug=bug)
    return max(float(np.abs(bpos - pos).max()) / H.BVH_POS_BOUND, float(H.euler_quat_error(beul, eul, order).max()) / H.BVH_QUAT_BOUND)


@pytest.mark.parametrize("branch", [1, 2, 3])
def test_trace_formula_in_another_branch_moves_the_oracle(branch):
    """the smallest case with an item in the branch: J = 3, T = 2; the half turns are what the trace formula cannot do"""
    x = H.bvh_case(3, 2, seed=302)
    assert (x["branch"] == branch).any()
    for order in ("zyx", "xzy"):
        assert _bvh_moved(x, order, None, f"trace_for_branch_{branch}") >= FACTOR


@pytest.mark.parametrize("order", ["zyx", "xzy"])
def test_table_controls_move_the_expected_rows(order):
    """seq ignored, the chunk's own first frame as re-basing reference, xzy written as zyx: each moves the expected table of the
    smallest table case (J = 3, T = 20, chunk [7, 8)) by >= 10x the bound"""
    x, seq = H.bvh_case(3, 20, seed=320), H.bvh_table_seq(3)
    assert seq[0] != 0 and sum(s != i for i, s in enumerate(seq)) * 2 >= len(seq)
    for t0, t1 in ((0, 7), (7, 8), (8, 20)):
        want = H.bvh_table_expected(x, seq, order, H.BVH_START, t0, t1)
        for bug in ("seq_ignored", "chunk_reference", "xzy_as_zyx"):
            if (bug == "chunk_reference" and t0 == 0) or (bug == "xzy_as_zyx" and order == "zyx"):
                continue
            pe, qe, _ = H.bvh_table_errors(H.bvh_table_expected(x, seq, order, H.BVH_START, t0, t1, bug=bug), want, order)
            assert max(pe / H.BVH_POS_BOUND, qe / H.BVH_QUAT_BOUND) >= FACTOR, (bug, t0, pe, qe)


@pytest.mark.parametrize("J", [1, 3, 65])
def test_table_sequences_permute(J):
    seq = H.bvh_table_seq(J)
    assert sorted(seq) == list(range(J))
    if J > 1:
        assert seq[0] != 0 and sum(s != i for i, s in enumerate(seq)) * 2 >= J


@pytest.mark.parametrize("order", ["zyx", "xzy"])
def test_pole_rows(order):
    mid = H.BVH_ASIN_OUTPUT[order]
    for k in (1, 2, 3):
        x = H.bvh_pole_case(order, k)
        s = H.bvh_raw_sin(x, order)
        assert (np.abs(s) < 1.0).all() and (s > 0).any() and (s < 0).any()
        if k == 3:
            assert (1.0 - np.abs(s)).max() < 2e-6
        _, eul = H.bvh_oracle(x, order)
        assert np.abs(np.abs(eul[..., mid]) - (90.0 - 10.0 ** -k)).max() < 5e-4       # (the 1e-10 of the row normalisation is 2.8e-4 degrees at k = 3)
    x = H.bvh_pole_case(order, None)
    s = H.bvh_raw_sin(x, order)
    assert (np.abs(s[:, 0]) > 1.0).all() and (s[:, 0] > 0).any() and (s[:, 0] < 0).any()        # the clamp has work to do
    _, eul = H.bvh_oracle(x, order)
    assert np.isfinite(eul).all() and np.abs(np.abs(eul[..., mid]) - 90.0).max() < 1e-3
    assert (np.abs(eul[:, 0, mid]) == 90.0).all()
