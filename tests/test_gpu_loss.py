"""The FK loss kernels (csrc/loss.hip) against the float64 oracle: per gradient group, per skeleton, per frame layout.

Before this file the 877 lines of csrc/loss.hip had ONE direct comparison with the oracle (test_gpu_parity.py::
test_loss_forward_backward_vs_oracle): B = 3, T = 7, the 75-joint rig, yaw-only unit root quaternions, one max-norm over the packed
gradient.  Here: 28 cases (frame layouts, skeletons, general non-unit root quaternions) x loss_lds 1 / 0, 16 cases with ONE input
group moved, every gradient slice (root groups whole, joint groups per joint) against its OWN largest entry, and the entry points
the engine uses (prepared truth half, gscale, unit_grad).  tests/test_loss_oracle_cpu.py proves on the CPU that the comparison is
sharp: eight restated kernel bugs and one flipped sign each miss the bound by more than 10x (table there).

Which case reaches which kernel / path (csrc/loss.hip, zeggs_loss_fwd_bwd_ex):
  loss_terms_k   (T % 4 != 0, one workgroup per feature row)        every x7 case, rig-2x2, rig-3x1
  loss_terms4_k  (T % 4 == 0, four frames per thread, 2 workgroups per row, partial sums)   every x8 case, rig-1x4 (one quad:
                 the first of the two split workgroups gets nothing), rig-1x12 (three quads, split 1 + 2), rig-5x28 (35 quads,
                 neighbours fetched across quad edges inside a window), j256-2x4
  frame kernels, one 64-lane workgroup per side with dead lanes     3x7 (21 frames), 2x8, 1x4, 1x12, 2x2, 3x1, 2x4
  ... two workgroups, 6 live lanes in the second, a window across the 63|64 boundary      10x7 (70 frames)
  ... three workgroups, windows across both boundaries                                     rig-5x28 (140 frames)
  LDS walk (levels handed on through the 147 KB message buffers)    loss_lds = 1 and no level wider than LOSS_LW = 16: rig (widths
                 1 3 3 5 5 5 3 3 5 12 10 10 10), j1 (one level, no message, the root fetched on its own), chain12 (levels of one
                 joint: seven idle waves at every barrier), star16 (a level of exactly 16: second round of the 8 waves full, message
                 slots 12-15), tree40, j256 (MAXJ: Levels / Children tables full, 17 levels of 15)
  table walk (levels handed on through the feature tables in global memory)   every loss_lds = 0 case, and star17 / star20 with
                 loss_lds = 1: chosen by maxw > LOSS_LW while the kernels were launched WITH the dynamic LDS
  T = 1 (rig-3x1): the reference's four finite-difference terms are means over nothing (NaN); the device returns 0 for them --
                 pinned -- and the other 14 terms and all gradients are compared with an oracle that leaves those four out.

L1 kinks (helpers.loss_near_elements): an element of a term's argument within 16x the float32-vs-float64 envelope of the ORACLE
(per term and joint) may take either sign on the device; the comparison takes, per near element, the side that brings the oracle
closest (helpers.loss_oracle_at_kinks; elements and sides go into the assertion message).  Near elements met: 0-7 per case (0-4 where
the host's float32 arithmetic differs; at most 16 allowed, asserted on the CPU for every case and again here); on the MI355X the oracle's own side was the closest for every one of them in
all 88 runs -- the rule has not had to flip a sign yet.

Bounds: none new.  Terms rtol 3e-5 / atol 1e-7, loss 3e-5, gradient slices 3e-4, KL gradients 1e-5 (those of the old test).
Measured on an MI355X over the 88 runs, error of the worst slice of a group against that slice's own largest entry:
  root_pos 0 .. 2.6e-7   root_rot 4.9e-8 .. 7.8e-7   root_vel 0 .. 2.2e-7   root_vrt 0 .. 2.9e-7
  lpos 8.1e-8 .. 1.3e-6  ltxy 8.2e-8 .. 1.3e-6       lvel 0 .. 8.9e-7       lvrt 0 .. 1.4e-6
  (0: slices the moved group does not reach -- exactly zero in the oracle, and required to be exactly zero on the device)
  terms 5.4e-8 .. 1.6e-6, loss 4e-10 .. 2.8e-7, mu / logvar gradients 3.9e-8 .. 1.6e-7.
The float32 ORACLE against the float64 one is at 1.6e-7 .. 1.0e-6 on the same slices: the kernels are as close to float64 as
torch's own float32, so no slice needed a bound taken from the float32 oracle's error.  Run time on the MI355X: the 92 tests of
this file 7.2 s, oracle included (slowest case 0.3 s); `test_gpu_parity.py -k loss_forward_backward` 0.2 s for its two cases.

Bugs found, none in the kinematics or the analytic backward:
  * The 18 terms and the loss were not reproducible from call to call: loss_terms_k added its rows' sums to the 18 words with
    global float atomics, loss_kl_final_k added loss_terms4_k's partial sums with LDS float atomics from 16 waves -- the same
    inputs gave terms 1-2 ulp apart (seen: 1.5e-5 on a term of 40, the loss in its 7th digit), so a prepared truth half, gscale
    or unit_grad "changed" the loss although every gradient was bitwise the same.  Both kernels now leave per-row partial sums
    and loss_kl_final_k adds them in a fixed order (per 64-partial chunk, then one wave per term over the chunks); the entry-point
    tests below hold terms and loss bitwise.
  * zeggs_loss_fwd_bwd_ex refused J > 256 only AFTER it had launched the two transposes, and both entry points accepted a
    workspace smaller than zeggs_loss_workspace_bytes states; the checks now sit ahead of every launch
    (test_gpu_parity.py::test_c_abi_rejects_bad_arguments_loudly).
"""

import numpy as np
import pytest
import torch

import helpers
from oracle import loss as oloss
from zeggs import ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
g = lambda t: t.to(DEV)  # noqa: E731
KLW = oloss.kl_weight(helpers.LOSS_KL_ITERATION)


class _lds:
    """option loss_lds for a block (0: the table walk in global memory), the default behind it"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        ops.set_option("loss_lds", self.v)

    def __exit__(self, *exc):
        ops.set_option("loss_lds", 1)
        return False


def _inputs(d):
    """the device tensors of a case: prediction (pose, root_pos, root_rot), truth (the same three), gaze, parents"""
    O, W = d["O"], d["W"]
    return (g(helpers.pack_pose(*O[2:])), g(O[0]), g(O[1]), g(helpers.pack_pose(*W[2:])), g(W[0]), g(W[1]), g(d["gaze"]),
            torch.as_tensor(d["parents"], dtype=torch.int32, device=DEV))


def _device(d, upstream=None, **kw):
    """ops.training_loss + backward on a case -> (loss, terms[19], [8 gradients in LOSS_GROUPS order, dmu, dlogvar]) on the host,
    float32 as the device left them"""
    op, orp, orr, wp, wrp, wrr, gz, parents = _inputs(d)
    op, orp, orr = op.requires_grad_(True), orp.requires_grad_(True), orr.requires_grad_(True)
    mu, lv = g(d["mu"]).requires_grad_(True), g(d["logvar"]).requires_grad_(True)
    loss, terms = ops.training_loss(op, orp, orr, wp, wrp, wrr, gz, parents, synth.DT, mu, lv, kl_weight=KLW, **kw)
    (loss if upstream is None else upstream * loss).backward()
    torch.cuda.synchronize()
    J = len(d["parents"])
    grads = [orp.grad, orr.grad] + list(helpers.unpack_pose_tree(op.grad, J)) + [mu.grad, lv.grad]
    return loss.detach().cpu(), terms.detach().cpu(), [x.detach().cpu() for x in grads]


def _compare(case, d, loss, terms, grads, loss_lds):
    """terms and loss at the bounds of test_gpu_parity.py::test_loss_forward_backward_vs_oracle; gradients per slice, each against
    its own largest entry, against the float64 oracle with the device's sides on the near-kink elements"""
    got = [x.double() for x in grads[:8]]
    loss64, terms64, ref, near, chosen = helpers.loss_oracle_at_kinks(d, got)
    note = f"{helpers.loss_case_id(case)}: near {near}, sides (element, oracle's, taken) {chosen}"
    errs = helpers.slice_errors(got, ref[:8])
    grp = {}
    for k, v in errs.items():
        n = k.partition("[")[0]
        grp[n] = max(grp.get(n, 0.0), v)
    tdev = terms[:18].double()
    terr = float(((tdev - terms64).abs() / terms64.abs().clamp_min(1e-30))[terms64 != 0].max())
    e_mu, e_lv = helpers.relerr(grads[8], ref[8]), helpers.relerr(grads[9], ref[9])
    print(f"\nMEASURED {helpers.loss_case_id(case)} loss_lds={loss_lds} "
          f"near={len(near)} flipped={sum(1 for _, a, b in chosen if a != b)} terms={terr:.1e} "
          f"loss={abs(float(loss) - float(loss64)) / abs(float(loss64)):.1e} " + " ".join(f"{k}={v:.1e}" for k, v in grp.items()) +
          f" mu={e_mu:.1e} logvar={e_lv:.1e}")
    np.testing.assert_allclose(tdev.numpy(), terms64.numpy(), err_msg=note, **helpers.LOSS_TERM_BOUND)
    if d["T"] == 1:        # the device's four finite-difference terms are 0 where the reference has a mean over nothing
        assert float(terms[list(oloss.DIFF_TERMS)].abs().max()) == 0.0
    assert abs(float(loss) - float(loss64)) < helpers.LOSS_BOUND * abs(float(loss64)), note
    assert float(terms[18]) == float(loss)
    k, e = helpers.worst_slice(errs)
    assert e < helpers.LOSS_GRAD_BOUND, f"slice {k}: {e:.2e}; " + note
    assert e_mu < helpers.LOSS_KL_BOUND and e_lv < helpers.LOSS_KL_BOUND, (e_mu, e_lv)
    return terms64


# ----------------------------------------------------------------------------- 3. frame layouts and skeletons
@pytest.mark.parametrize("loss_lds", [1, 0])
@pytest.mark.parametrize("case", helpers.LOSS_CASES, ids=helpers.loss_case_id)
def test_loss_case_vs_oracle(case, loss_lds):
    d = helpers.loss_case(case)
    with _lds(loss_lds):
        loss, terms, grads = _device(d)
    _compare(case, d, loss, terms, grads, loss_lds)


# ----------------------------------------------------------------------------- 4. one group moved at a time
@pytest.mark.parametrize("loss_lds", [1, 0])
@pytest.mark.parametrize("case", helpers.LOSS_MOVED_CASES, ids=helpers.loss_case_id)
def test_one_group_moved_vs_oracle(case, loss_lds):
    """prediction = truth bit for bit except ONE input group: every term that group does not reach is exactly 0 on the device (both
    sides run the same arithmetic) as in the oracle, and the gradients that are left -- e.g. those of lpos, ltxy, lvrt, root_rot
    through cvel (0.06) alone when lvel moves -- are compared on their own scale, slice by slice."""
    d = helpers.loss_case(case)
    with _lds(loss_lds):
        loss, terms, grads = _device(d)
    terms64 = _compare(case, d, loss, terms, grads, loss_lds)
    reach = helpers.LOSS_REACH[case[4]]
    assert {i for i in range(17) if float(terms[i]) != 0.0} == reach
    assert {i for i in range(17) if float(terms64[i]) != 0.0} == reach


# ----------------------------------------------------------------------------- 5. entry points
def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("B,T", [(3, 7), (2, 8)])
def test_prepared_truth_is_bitwise_the_unprepared_call(B, T):
    """ops.loss_prepare_truth + truth_ws (the engine's default path): loss, terms and every gradient bitwise equal to the call
    that runs the truth half itself; a workspace prepared for batch A and prepared again for batch B gives B's result."""
    dA, dB = helpers.loss_case(("rig", B, T, "general")), helpers.loss_case(("rig", B, T, "general", "lpos"))
    plain = {k: _device(d) for k, d in (("A", dA), ("B", dB))}
    assert not torch.equal(plain["A"][1], plain["B"][1])

    def prepare(d, ws=None):
        _, _, _, wp, wrp, wrr, gz, parents = _inputs(d)
        return ops.loss_prepare_truth(wp, wrp, wrr, gz, parents, synth.DT, ws=ws)
    ws = prepare(dA)
    assert _same(_device(dA, truth_ws=ws), plain["A"])
    ws2 = prepare(dB, ws=ws)
    assert ws2.data_ptr() == ws.data_ptr()                          # the same workspace, used again
    assert _same(_device(dB, truth_ws=ws2), plain["B"])


@pytest.mark.parametrize("B,T", [(3, 7), (2, 8)])
def test_gscale_and_upstream_gradient_scale_bitwise(B, T):
    """gscale = 0.25: terms unchanged, gradients bitwise a quarter; unit_grad = True equals False under upstream gradient 1;
    upstream gradient 2 doubles them bitwise (powers of two: exact in float32)."""
    d = helpers.loss_case(("rig", B, T, "general"))
    one = _device(d)
    quarter = _device(d, gscale=0.25)
    assert torch.equal(one[0], quarter[0]) and torch.equal(one[1], quarter[1])
    assert all(torch.equal(0.25 * a, b) for a, b in zip(one[2], quarter[2]))
    assert all(float(a.abs().max()) > 0 for a in one[2])
    assert _same(_device(d, unit_grad=True), one)
    two = _device(d, upstream=2.0)
    assert all(torch.equal(2.0 * a, b) for a, b in zip(one[2], two[2]))
