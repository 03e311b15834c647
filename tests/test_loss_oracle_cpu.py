"""CPU side of tests/test_gpu_loss.py: the oracle pieces it relies on, the near-kink condition of every case, and the negative
controls that prove the per-slice comparison sharp.  Nothing here needs a GPU.

Negative controls.  Each corruption of the ORACLE (oracle/loss.py BUGS) restates a plausible bug of csrc/loss.hip.  The corrupted
float64 gradients are handed to the very comparison the GPU test runs (helpers.loss_oracle_at_kinks: free sides on the near-kink
elements, then every slice against its own largest entry) and must miss the 3e-4 bound by more than 10x in at least one case of
CONTROL_CASES.  OLD view = what tests/test_gpu_parity.py::test_loss_forward_backward_vs_oracle sees: B = 3, T = 7, yaw-only root
rotations, one max-norm over the packed gradient at 3e-4, the 18 terms at rtol 3e-5.  Measured (float64; the tests print the
figures and assert the OLD_VIEW table):

  corruption                 worst slice / bound over CONTROL_CASES    OLD view: packed gradient (3e-4)   terms (3e-5)
  cvel_without_cross         1 000x .. 3 600x                          caught, 3.3e-1                     caught
  last_child_detached        220x .. 4 200x                            caught, 4.7e-1                     BLIND (backward only)
  joint0_local_unreplaced    3 300x .. 5 700x                          caught, 8.1e-1                     caught
  rootvel_own_rotation       520x .. 5 300x                            caught, 4.4e-3 (15x its bound)     caught
  diff_across_windows        1 800x .. 5 800x (*)                      caught, 5.1e-1                     caught
  n2_with_T                  440x .. 1 800x (T = 2) (*)                caught, 1.4e-1                     caught
  rmat_normalised            32x .. 117x (*)                           caught, 4.5e-3 (15x its bound)     caught (the old prediction
                                                                       blends two unit quaternions: its norm is below 1)
  gaze_q_not_inverse         29x .. 95x (*)                            caught, 3.5e-2                     caught
  one sign flipped           per term, smallest .. largest over SIGN_CASES: root_pos 7x .. 1 900x, root_rot 14x .. 530x, root_vel
                             180x .. 2 300x, root_vrt 570x .. 1 800x, lpos 61x .. 6 200x, lrot 30x .. 1 700x, lvel 390x .. 3 000x,
                             lvrt 65x .. 5 200x, cpos 2.0x .. 41x, crot 2.8x .. 160x, cvel 120x .. 2 400x, cvrt 250x .. 1 300x,
                             ldvl 2 000x .. 5 400x, ldvt 1 100x .. 2 700x, cdvl 61x .. 330x, cdvt 6.9x .. 410x, gaze 30x .. 1 300x
                             OLD view: MISSES the flipped sign in lrot (2.8e-4), cpos (1.6e-4) and crot (1.7e-5 of the packed maximum)
  (*) 0x in rig-3x7-general-lvel, as it must be: lvel does not reach that term.

So on its own fixture the old gradient check does catch the eight restated bugs (the synthetic rig's joint rotations are redrawn
every frame -- angular velocities of ~25 rad / s -- which makes cvel large there), two of them by a factor 15 only; what it cannot
see is a single wrong sign in lrot, cpos or crot, and the per-slice view separates every one of them by two to four orders of
magnitude.  Where the finite-difference terms exist (weights 7 / dt = 420 and 8 / dt = 480 in the same slices) one sign of cpos
(0.1) or crot (3) is only 2-3x the bound; at T = 1 it is 40x -- hence SIGN_CASES.
"""
import numpy as np
import pytest
import torch

import helpers
from oracle import loss as oloss
from zeggs import synth

BOUND = helpers.LOSS_GRAD_BOUND
ALL_CASES = helpers.LOSS_CASES + helpers.LOSS_MOVED_CASES
CONTROL_CASES = [("rig", 3, 7, "general"), ("rig", 2, 8, "general"), ("rig", 2, 2, "general"), ("rig", 3, 7, "general", "lvel"),
                 ("star17", 10, 7, "general"), ("tree40", 3, 7, "general")]
OLD_CASE = ("rig", 3, 7, "yaw")
# does the OLD view catch it: (gradients, terms)
OLD_VIEW = dict(cvel_without_cross=(True, True), last_child_detached=(True, False), joint0_local_unreplaced=(True, True),
                rootvel_own_rotation=(True, True), diff_across_windows=(True, True), n2_with_T=(True, True),
                rmat_normalised=(True, True), gaze_q_not_inverse=(True, True))
OLD_VIEW_MISSES_SIGN_OF = {5, 8, 9}         # lrot, cpos, crot
SIGN_CASES = [("rig", 10, 7, "general"), ("rig", 3, 1, "general"), ("rig", 2, 2, "general"), ("chain12", 3, 7, "general"),
              ("star17", 10, 7, "general")]


def _f64(ts):
    return [t.double() for t in ts]


def test_skeletons_reach_the_paths_they_are_named_for():
    """level widths of the parent tables (csrc/loss.hip: LOSS_LW = 16 joints per level for the LDS walk, MAXJ = 256, 8 waves)"""
    def widths(par):
        depth = []
        for i, p in enumerate(par):
            assert (p == -1) if i == 0 else (0 <= p < i)
            depth.append(0 if i == 0 else depth[p] + 1)
        return list(np.bincount(depth))
    w = {k: widths(v) for k, v in helpers.LOSS_SKELETONS.items()}
    assert w["rig"] == [1, 3, 3, 5, 5, 5, 3, 3, 5, 12, 10, 10, 10]
    assert w["j1"] == [1] and w["chain12"] == [1] * 12
    assert max(w["star16"]) == 16 and max(w["star17"]) == 17 and max(w["star20"]) == 20
    assert len(helpers.LOSS_SKELETONS["tree40"]) == 40 and max(w["tree40"]) <= 16
    assert len(helpers.LOSS_SKELETONS["j256"]) == 256 and w["j256"] == [1] + [15] * 17
    # a joint with several children on every multi-level skeleton but the chain
    assert all(max(np.bincount(np.asarray(helpers.LOSS_SKELETONS[k][1:]))) >= 2 for k in ("rig", "tree40", "j256", "star16"))


def test_fixtures_have_the_rotations_they_claim():
    d = helpers.loss_case(("rig", 3, 7, "general"))
    Wq, Oq = d["W"][1], d["O"][1]
    assert float((Wq.norm(dim=-1) - 1).abs().max()) < 1e-6 and bool((Wq[..., 0] < 0).any()) and bool((Wq[..., 0] > 0).any())
    assert bool((Wq[..., 1].abs() > 0.05).any()) and bool((Wq[..., 3].abs() > 0.05).any())        # not yaw-only
    n = Oq.norm(dim=-1)
    assert 0.7 <= float(n.min()) < 0.85 and 1.15 < float(n.max()) <= 1.3
    y = helpers.loss_case(OLD_CASE)
    assert float(y["W"][1][..., 1].abs().max()) == 0.0 and float(y["W"][1][..., 3].abs().max()) == 0.0
    m = helpers.loss_case(("rig", 2, 8, "general", "lvel"))
    for n_, o, w in zip(helpers.LOSS_GROUPS, m["O"], m["W"]):
        assert torch.equal(o, w) == (n_ != "lvel")


def test_sides_are_linear_and_leave_the_value_alone():
    """training_loss(sides=...) fixes the derivative of |x| at listed elements; the value does not move, and the gradient is
    base + sum (side - sign) / (18 n) dx_e / d input: what helpers.loss_oracle_at_kinks relies on."""
    d = helpers.loss_case(("tree40", 2, 8, "general"))
    loss0, terms0, g0 = helpers.loss_oracle(d)
    picks = {10: ([5, 77], [0.0, 1.0]), 14: ([3], [-1.0]), 1: ([17], [0.0])}
    loss1, terms1, g1 = helpers.loss_oracle(d, sides=picks)
    assert torch.equal(loss0, loss1) and torch.equal(terms0, terms1)
    O = [o.double().requires_grad_(True) for o in d["O"]]
    x = oloss.term_arguments(O, _f64(d["W"]), d["gaze"].double(), d["parents"], synth.DT)
    lin = [g.clone() for g in g0[:8]]
    for k, (idx, sd) in picks.items():
        for j, s in zip(idx, sd):
            xe = x[k].flatten()[j]
            D = torch.autograd.grad(xe, O, retain_graph=True, allow_unused=True)
            lin = [a if b is None else a + (s - float(torch.sign(xe.detach()))) / (18.0 * x[k].numel()) * b for a, b in zip(lin, D)]
    assert max(helpers.relerr(a, b) for a, b in zip(lin, g1[:8])) < 1e-12
    assert max(helpers.relerr(a, b) for a, b in zip(g0[:8], g1[:8])) > 1e-3          # (the picks did change something)


def test_without_the_difference_terms_at_one_frame():
    """T = 1: the reference's four finite-difference terms are means over nothing (NaN); the comparison leaves them out"""
    d = helpers.loss_case(("rig", 3, 1, "general"))
    full, _ = oloss.training_loss(_f64(d["O"]), _f64(d["W"]), d["gaze"].double(), d["parents"], synth.DT)
    assert bool(torch.isnan(full))
    loss, terms, grads = helpers.loss_oracle(d)
    assert bool(torch.isfinite(loss)) and float(terms[list(oloss.DIFF_TERMS)].abs().max()) == 0.0
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    assert abs(float(terms.sum() / 18.0) - float(loss)) < 1e-15


@pytest.mark.parametrize("case", ALL_CASES, ids=helpers.loss_case_id)
def test_near_kink_condition_and_float32_oracle_through_the_gpu_comparison(case):
    """Every case of the GPU matrix has at most 16 term elements within 16x the float32 envelope of their kink (seeds chosen for
    it), and the ORACLE run in float32 passes the comparison the device is put through (terms, loss, every gradient slice, sign
    freedom on the near elements only): the bounds are within reach of a float32 implementation -- measured here: worst slice
    1.9e-7 .. 1.0e-6 over all cases, 0-4 near elements per case (0-7 on another host: the
    envelope is the host's float32 arithmetic), so no slice needs a bound taken from the float32 oracle's own error."""
    d = helpers.loss_case(case)
    near, env = helpers.loss_near_elements(d)
    assert len(near) <= helpers.LOSS_NEAR_MAX, (len(near), near[:20])
    l32, t32, g32 = helpers.loss_oracle(d, torch.float32)
    loss, terms, grads, near, chosen = helpers.loss_oracle_at_kinks(d, _f64(g32[:8]))
    np.testing.assert_allclose(t32.numpy(), terms.numpy(), **helpers.LOSS_TERM_BOUND)
    assert abs(float(l32) - float(loss)) < helpers.LOSS_BOUND * abs(float(loss))
    k, e = helpers.worst_slice(helpers.slice_errors(_f64(g32[:8]), grads[:8]))
    print(f"\n{helpers.loss_case_id(case)}: {len(near)} near, float32 oracle worst slice {k} {e:.2e}")
    assert e < BOUND, (k, e, near, chosen)
    if len(case) > 4:      # one group moved: which terms are exactly zero
        assert {i for i in range(17) if float(terms[i]) != 0.0} == helpers.LOSS_REACH[case[4]]
        assert {i for i in range(17) if float(t32[i]) != 0.0} == helpers.LOSS_REACH[case[4]]


def _through_the_comparison(d, got):
    """worst slice error of `got` in the GPU test's comparison, as a multiple of the bound"""
    _, _, grads, near, chosen = helpers.loss_oracle_at_kinks(d, got)
    return helpers.worst_slice(helpers.slice_errors(got, grads[:8]))[1] / BOUND


@pytest.mark.parametrize("bug", oloss.BUGS)
def test_negative_control_kernel_bugs_exceed_the_gpu_bound(bug):
    seps = {}
    for case in CONTROL_CASES:
        d = helpers.loss_case(case)
        _, _, bad = helpers.loss_oracle(d, bug=bug)
        seps[helpers.loss_case_id(case)] = _through_the_comparison(d, bad[:8])
    d = helpers.loss_case(OLD_CASE)
    _, terms, good = helpers.loss_oracle(d)
    _, bterms, bad = helpers.loss_oracle(d, bug=bug)
    old_g = helpers.packed_error(bad[:8], good[:8])
    old_t = float(((bterms - terms).abs() / (1e-7 / 3e-5 + terms.abs())).max())
    print(f"\n{bug}: worst slice / bound per case " + ", ".join(f"{k} {v:.0f}x" for k, v in seps.items()) +
          f"; OLD view: packed gradient {old_g:.2e} (bound 3e-4), terms {old_t:.2e} (bound 3e-5)")
    assert max(seps.values()) > 10, seps
    assert (old_g > 3e-4, old_t > 3e-5) == OLD_VIEW[bug], (old_g, old_t)
    assert not 0.8 * 3e-4 < old_g < 1.25 * 3e-4 and not 0.8 * 3e-5 < old_t < 1.25 * 3e-5      # (the table is not a coin toss)


def test_negative_control_one_flipped_sign_is_not_absorbed_by_the_kink_rule():
    """What the kink rule must NOT absorb: the sign of ONE element that is not near its kink, flipped (in turn: the largest
    element of each of the 17 terms).  In every case of SIGN_CASES the comparison, with its free sides on the near elements,
    still fails; and for every term it fails by more than 10x in at least one case.  (Where the finite-difference terms exist
    they carry weights 7 / dt = 420 and 8 / dt = 480 into the lpos / ltxy slices: one sign of cpos -- 0.1 -- is then 2x the bound,
    not 10x.  At T = 1 those terms are absent and the same flip is 40x the bound; the four finite-difference terms themselves are
    measured at T >= 2.)"""
    old = helpers.loss_case(OLD_CASE)
    _, _, old_good = helpers.loss_oracle(old)
    seps, missed, nnear = {}, set(), 0
    for case in SIGN_CASES:
        d = helpers.loss_case(case)
        near, _ = helpers.loss_near_elements(d)
        nnear += len(near)
        xs = helpers.loss_term_args(d, torch.float64)
        for k in range(17):
            if d["T"] == 1 and k in oloss.DIFF_TERMS:
                continue
            x = xs[k].flatten()
            j = int(x.abs().argmax())
            assert (k, j) not in near
            _, _, bad = helpers.loss_oracle(d, sides={k: ([j], [-float(torch.sign(x[j]))])})
            seps.setdefault(oloss.LOSS_NAMES[k], {})[helpers.loss_case_id(case)] = _through_the_comparison(d, bad[:8])
    assert nnear >= 1                                                # (the rule had something to play with)
    xo = helpers.loss_term_args(old, torch.float64)
    for k in range(17):
        jo = int(xo[k].abs().argmax())
        _, _, old_bad = helpers.loss_oracle(old, sides={k: ([jo], [-float(torch.sign(xo[k].flatten()[jo]))])})
        if helpers.packed_error(old_bad[:8], old_good[:8]) <= 3e-4:
            missed.add(k)
    print("\none flipped sign, worst slice / bound (smallest .. largest over the cases): " +
          ", ".join(f"{k} {min(v.values()):.1f}x .. {max(v.values()):.0f}x" for k, v in seps.items()) +
          f"; the OLD view misses it in terms {sorted(missed)}")
    assert all(min(v.values()) > 1 for v in seps.values()), seps
    assert all(max(v.values()) > 10 for v in seps.values()), seps
    assert missed == OLD_VIEW_MISSES_SIGN_OF
