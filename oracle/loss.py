"""Oracle restatement of the training loss (torch CPU, differentiable).

TEST INFRASTRUCTURE -- see oracle/__init__.py.

Reference: ZEGGS/train.py:276-421 (FK + 17 weighted L1 terms + KL, sum / 18),
ZEGGS/anim/txform.py:10-34 (xform_fk_vel, xform_orthogonalize_from_xy),
ZEGGS/modules.py:673 (normalize), :745-789 (KL weight / KL divergence).
"""
import math

import torch

from .nets import _cross, quat_inv_mul_vec, quat_mul_vec, quat_to_xform

LOSS_NAMES = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "lrot", "lvel", "lvrt",
              "cpos", "crot", "cvel", "cvrt", "ldvl", "ldvt", "cdvl", "cdvt", "gaze", "kl")
LOSS_WEIGHTS = (0.1, 10.0, 0.1, 5.0, 15.0, 15.0, 10.0, 7.0,
                0.1, 3.0, 0.06, 1.25, 7.0, 8.0, 0.06, 1.25, 10.0)


def _norm(x):
    return torch.sqrt(torch.sum(x * x, dim=-1, keepdim=True))


def orthogonalize_from_xy(xy, eps=1e-10):
    """txform.py:23-34: xy [..., 2, 3] -> rotation matrices [..., 3, 3] whose
    COLUMNS are the normalised x, y, z axes."""
    x = xy[..., 0, :]
    z = _cross(x, xy[..., 1, :])
    y = _cross(z, x)
    rows = torch.stack([x / (_norm(x) + eps), y / (_norm(y) + eps), z / (_norm(z) + eps)], dim=-2)
    return rows.transpose(-1, -2)


def fk_vel(lmat, lpos, lvrt, lvel, parents, bug=None):
    """txform.py:10-20; joints axis is -3 for lmat, -2 for vectors."""
    gr, gp, gt, gv = [lmat[..., 0, :, :]], [lpos[..., 0, :]], [lvrt[..., 0, :]], [lvel[..., 0, :]]

    def mv(m, v):
        return torch.matmul(m, v[..., None])[..., 0]

    lost = set()
    if bug == "last_child_detached":      # a parent of several children never receives its last child's backward message
        kids = {}
        for i in range(1, len(parents)):
            kids.setdefault(int(parents[i]), []).append(i)
        lost = {k[-1] for k in kids.values() if len(k) >= 2}
    for i in range(1, len(parents)):
        p = int(parents[i])
        pr, pp, pt, pv = gr[p], gp[p], gt[p], gv[p]
        if i in lost:
            pr, pp, pt, pv = pr.detach(), pp.detach(), pt.detach(), pv.detach()
        rp = mv(pr, lpos[..., i, :])
        gp.append(pp + rp)
        gr.append(torch.matmul(pr, lmat[..., i, :, :]))
        gt.append(pt + mv(pr, lvrt[..., i, :]))
        gv.append(pv + mv(pr, lvel[..., i, :]) + (0 if bug == "cvel_without_cross" else _cross(pt, rp)))
    return (torch.stack(gr, dim=-3), torch.stack(gp, dim=-2),
            torch.stack(gt, dim=-2), torch.stack(gv, dim=-2))


def kl_weight(iteration):
    """modules.py:745-761,773-788: min(logistic(0.005 (it - 7500)), 0.2)"""
    v = 1.0 / (1.0 + math.exp(-0.005 * (iteration - 7500)))
    return min(v, 0.2)


# Restatements of plausible kernel bugs (negative controls: tests/test_loss_oracle_cpu.py).  `bug` is one of these names or None.
BUGS = ("cvel_without_cross", "last_child_detached", "joint0_local_unreplaced", "rootvel_own_rotation",
        "diff_across_windows", "n2_with_T", "rmat_normalised", "gaze_q_not_inverse")
DIFF_TERMS = (12, 13, 14, 15)                     # the four finite-difference terms (mean over nothing at T = 1)


def _world(root_pos, root_rot, root_vel, root_vrt, lpos, ltxy, lvel, lvrt, bug=None):
    """train.py:277-322 for one side (O_ or W_)."""
    lmat = orthogonalize_from_xy(ltxy)
    # root velocities rotated by the PREVIOUS frame's root rotation (frame 0 by itself)
    prev_rot = torch.cat([root_rot[:, 0:1], root_rot[:, :-1]], dim=1)
    if bug == "rootvel_own_rotation":
        prev_rot = root_rot
    rvel = quat_mul_vec(prev_rot, root_vel)
    rvrt = quat_mul_vec(prev_rot, root_vrt)
    r_lpos0 = quat_mul_vec(root_rot, lpos[:, :, 0])
    lpos0 = r_lpos0 + root_pos
    lmat0 = torch.matmul(quat_to_xform(root_rot), lmat[:, :, 0])
    lvel0 = rvel + quat_mul_vec(root_rot, lvel[:, :, 0]) + _cross(rvrt, r_lpos0)
    lvrt0 = rvrt + quat_mul_vec(root_rot, lvrt[:, :, 0])
    lpos = torch.cat([lpos0.unsqueeze(2), lpos[:, :, 1:]], dim=2)
    lmat = torch.cat([lmat0.unsqueeze(2), lmat[:, :, 1:]], dim=2)
    lvel = torch.cat([lvel0.unsqueeze(2), lvel[:, :, 1:]], dim=2)
    lvrt = torch.cat([lvrt0.unsqueeze(2), lvrt[:, :, 1:]], dim=2)
    return rvel, rvrt, lpos, lmat, lvel, lvrt


def loss_features(O, W, gaze_pos, parents, bug=None):
    """The 13 pairs (prediction, ground truth) of feature tensors behind the 17 L1 terms, in LOSS_NAMES order for terms 0-11 and
    the gaze pair last; the finite-difference terms 12-15 reuse pairs 4 (lpos), 5 (ltxy), 8 (cpos), 9 (cmat)."""
    O_rvel, O_rvrt, O_lpos, O_lmat, O_lvel, O_lvrt = _world(*O, bug=bug)
    W_rvel, W_rvrt, W_lpos, W_lmat, W_lvel, W_lvrt = _world(*W, bug=bug)
    O_cmat, O_cpos, O_cvrt, O_cvel = fk_vel(O_lmat, O_lpos, O_lvrt, O_lvel, parents, bug=bug)
    W_cmat, W_cpos, W_cvrt, W_cvel = fk_vel(W_lmat, W_lpos, W_lvrt, W_lvel, parents, bug=bug)

    def normalize(x, eps=1e-8):                                   # modules.py:673
        return x / (_norm(x) + eps)

    def rmat(q):
        return quat_to_xform(q / _norm(q) if bug == "rmat_normalised" else q)

    O_rmat, W_rmat = rmat(O[1]), rmat(W[1])
    rot = quat_mul_vec if bug == "gaze_q_not_inverse" else quat_inv_mul_vec
    W_gaze = rot(W[1], normalize(gaze_pos - W[0]))                 # train.py:336
    O_gaze = rot(O[1], normalize(gaze_pos - O[0]))                 # train.py:337
    O_l, W_l = (O_lpos, O_lvel, O_lvrt), (W_lpos, W_lvel, W_lvrt)
    if bug == "joint0_local_unreplaced":                           # the "local" terms on the joint 0 the network emitted
        O_l, W_l = (O[4], O[6], O[7]), (W[4], W[6], W[7])
    return [(O[0], W[0]), (O_rmat, W_rmat), (O_rvel, W_rvel), (O_rvrt, W_rvrt),
            (O_l[0], W_l[0]), (O[5], W[5]), (O_l[1], W_l[1]), (O_l[2], W_l[2]),
            (O_cpos, W_cpos), (O_cmat, W_cmat), (O_cvel, W_cvel), (O_cvrt, W_cvrt), (O_gaze, W_gaze)]


def term_arguments(O, W, gaze_pos, parents, dt, bug=None):
    """x[k], k = 0..16: the tensor whose mean |.| is term k (the weighted difference w (a - b) of a feature pair, or of its
    finite differences along time; [B, T or T - 1, ...], the joint axis -- terms 4..15 -- is axis 2)."""
    f = loss_features(O, W, gaze_pos, parents, bug=bug)
    wt = LOSS_WEIGHTS

    def d(w, ab):
        return w * (ab[0] - ab[1])

    def dd(w, ab):                                                 # train.py:355-393
        a, b = ab
        if bug == "diff_across_windows":                           # over the flattened B T axis
            a, b = a.reshape(1, -1, *a.shape[2:]), b.reshape(1, -1, *b.shape[2:])
        return w * ((a[:, 1:] - a[:, :-1]) / dt - (b[:, 1:] - b[:, :-1]) / dt)

    return [d(wt[k], f[k]) for k in range(12)] + [dd(wt[12], f[4]), dd(wt[13], f[5]), dd(wt[14], f[8]), dd(wt[15], f[9]),
                                                  d(wt[16], f[12])]


def abs_with_sides(x, sides):
    """|x| whose derivative at the listed elements is the given side: sides = (flat indices, values in {-1, 0, +1}).  The value
    is |x| everywhere -- both one-sided derivatives (and everything between) are subgradients of |.| at a kink."""
    y = torch.abs(x)
    if sides is None or len(sides[0]) == 0:
        return y
    idx = torch.as_tensor(sides[0], dtype=torch.long)
    s = torch.as_tensor(sides[1], dtype=x.dtype)
    xf = x.flatten()[idx]
    corr = (s - torch.sign(xf.detach())) * (xf - xf.detach())      # value 0, derivative (side - sign)
    return y.flatten().index_add(0, idx, corr).reshape(x.shape)


def training_loss(O, W, gaze_pos, parents, dt, mu=None, logvar=None, iteration=0, sides=None, skip=(), bug=None):
    """O, W: 8-tuples (root_pos, root_rot, root_vel, root_vrt, lpos, ltxy, lvel, lvrt)
    of [B, T, ...] tensors (prediction / ground truth).  Returns (loss, terms[18]).
    sides: {term index: (flat indices into term_arguments()[k], sides)} -- see abs_with_sides; skip: terms left out (value 0:
    DIFF_TERMS at T = 1, where the reference takes a mean over nothing); bug: one of BUGS (negative controls)."""
    x = term_arguments(O, W, gaze_pos, parents, dt, bug=bug)
    T = O[0].shape[1]
    terms = []
    for k in range(17):
        if k in skip:
            terms.append(torch.zeros((), dtype=O[0].dtype))
            continue
        t = torch.mean(abs_with_sides(x[k], None if sides is None else sides.get(k)))
        if bug == "n2_with_T" and k in DIFF_TERMS:
            t = t * ((T - 1) / T)
        terms.append(t)
    if mu is not None and logvar is not None:                      # train.py:397-400
        kl = torch.mean(-0.5 * torch.mean(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))
        terms.append(kl_weight(iteration) * kl)
    else:
        terms.append(torch.zeros((), dtype=O[0].dtype))
    loss = sum(terms) / 18.0
    return loss, torch.stack([t.detach() for t in terms])
