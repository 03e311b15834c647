"""Helpers of the held-out evaluation tests: the per-window oracle, built from oracle.loss only, and device plumbing."""
import numpy as np
import torch

import helpers
from oracle import loss as oloss
from zeggs import synth

COLS = 22
EVAL_CASES = list(helpers.LOSS_CASES) + [("rig", 2, 70, "general"), ("rig", 1, 300, "general")]


def rows_oracle(data, dtype=torch.float64, bug=None, with_kl=True):
    """[B, 22] in `dtype` of a helpers.loss_case: columns 0..16 the mean |.| of oracle.loss.term_arguments per window (the four
    finite-difference ones 0 at T = 1), 17 the unweighted KL of the window, 18 the mean distance of the cpos pair of
    oracle.loss.loss_features, 19 the distance of the root positions at the last frame, 20 / 21 the mean norm of the cvel pair.
    bug = "diff_across_windows": oracle.loss takes the differences over the flattened B T axis; a window then owns the T
    differences that START in it (T - 1 for the last one)."""
    O, W = [o.to(dtype) for o in data["O"]], [w.to(dtype) for w in data["W"]]
    gaze, parents = data["gaze"].to(dtype), data["parents"]
    B, T = O[0].shape[:2]
    with torch.no_grad():
        x = oloss.term_arguments(O, W, gaze, parents, synth.DT, bug=bug)
        f = oloss.loss_features(O, W, gaze, parents, bug=bug)
    rows = torch.zeros(B, COLS, dtype=dtype)
    for b in range(B):
        for k in range(17):
            if k in oloss.DIFF_TERMS and x[k].shape[0] == 1 and B * T > 1 and bug == "diff_across_windows":
                part = x[k][0, b * T:min((b + 1) * T, B * T - 1)]
            elif k in oloss.DIFF_TERMS and T == 1:
                continue
            else:
                part = x[k][b]
            rows[b, k] = part.abs().mean() if part.numel() else 0.0
        if with_kl:
            mu, lv = data["mu"][b].to(dtype), data["logvar"][b].to(dtype)
            rows[b, 17] = -0.5 * torch.mean(1 + lv - mu.pow(2) - lv.exp())
        rows[b, 18] = (f[8][0][b] - f[8][1][b]).norm(dim=-1).mean()
        rows[b, 19] = (O[0][b, -1] - W[0][b, -1]).norm()
        rows[b, 20] = f[10][0][b].norm(dim=-1).mean()
        rows[b, 21] = f[10][1][b].norm(dim=-1).mean()
    return rows


def with_row_as_truth(data, b):
    """the case with window b's prediction replaced by its truth (posterior = prior for its KL: mu = logvar = 0)"""
    O = [o.clone() for o in data["O"]]
    for o, w in zip(O, data["W"]):
        o[b] = w[b]
    mu, lv = data["mu"].clone(), data["logvar"].clone()
    mu[b], lv[b] = 0.0, 0.0
    return dict(data, O=O, mu=mu, logvar=lv)


def permuted(data, perm):
    perm = torch.as_tensor(perm)
    return dict(data, O=[o[perm] for o in data["O"]], W=[w[perm] for w in data["W"]], gaze=data["gaze"][perm],
                mu=data["mu"][perm], logvar=data["logvar"][perm])


def device_inputs(d, dev="cuda:0"):
    """(o_pose, o_rpos, o_rrot, w_pose, w_rpos, w_rrot, gaze, parents) of a case on the device"""
    O, W = d["O"], d["W"]
    g = lambda t: t.to(dev).contiguous()  # noqa: E731
    return (g(helpers.pack_pose(*O[2:])), g(O[0]), g(O[1]), g(helpers.pack_pose(*W[2:])), g(W[0]), g(W[1]), g(d["gaze"]),
            torch.as_tensor(d["parents"], dtype=torch.int32, device=dev))


def plan_dataset(ranges, window, seed=3):
    """a CPU engine.DeviceDataset whose TRAINING ranges are `ranges` (frames up to the last range's end)"""
    from zeggs import engine
    ranges = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    n = int(ranges[:, 1].max()) + 5 if len(ranges) else 5
    data = synth.make_processed(1, 0, n, seed=seed)
    data["ranges_train"] = ranges.astype(np.int32)
    data["ranges_train_labels"] = np.zeros(len(ranges), np.int32)
    return engine.DeviceDataset(data, window, torch.device("cpu"))
