"""The decoder with UNTIED statistics and at every branch of the root's quaternion exponential: every decoder path against
oracle.nets.decoder_rollout in float64 directly (never kernel against kernel).

Why: synth.make_stats() and both recorded statistics files have out_mean == in_mean[:PO] exactly, so the (mu_o - mu_i) term of every
fold of the statistics into the weights (decoder_fast.hip merge_prep_k / cvec, tp_common.h cv0 / p1x, train_dual.hip,
decode_persistent.hip, the unfolded form and its BPTT in decoder.hip) was zero in every test; and with them the half turn per frame
h = dt / 2 |root_vrt| stays in [2.8e-3, 6.4e-3], one of the three branches (h < 1e-5: quat_normalize([1, x]); h < 1: polynomials;
h >= 1: libm) of quat_exp_mul (root_step) and quat_exp_ctx with qexp_bwd_ctx / qexp_bwd_coef (root_bwd / root_prepare), all in
dec_math.h, the one statement every decoder kernel calls.  helpers.decoder_stats(kind) gives the statistics, tests/test_decoder_stats_oracle_cpu.py proves on the
CPU that every case lies in its branch and that each bound below trips on the bug it is meant for.

Which case launches which kernels (helpers.DEC_TRAIN_CASES / DEC_INFER_CASES; every case asserts it):
  generic (2, 6)            decoder_fast = 0: per-step GEMMs, dec_devec_k / dec_devec_bwd_k (decoder.hip)
  stage (5, 6), (33, 4)     fragment-packed stage launches forward and backward (decoder_fast.hip), both persistent kernels off
  tp16-tiles4=0/1 (5, 6)    persistent training forward, one 16-row tile (train_persistent.hip); stage BPTT
  tp4 (17, 5)               persistent training forward on 4-row tiles (two batch tiles); stage BPTT
  dual (17, 5)              dual-chain forward (train_dual.hip); stage BPTT
  bptt (5, 6), (17, 5), (40, 4)   persistent forward + persistent BPTT sweep (train_bwd_persistent.hip), one sweep and two (B > 32)
  film (5, 6)               FiLM decoder: merged EPI_HID_MERGED fold and W3 on the stage launches (the persistent kernels decline)
  h512 (2, 6)               nhidden = 512 stage kernels
  ring (3, 7)               no_grad ring path, MFMA stage kernels
  b1-persistent (1, 6), (1, 37)   weight-stationary B = 1 decode (decode_persistent.hip)
  b1-stage-gemv / -mfma     B = 1 stage launches: GEMV kernels / stage_variant 1024 (the chained launches are not part of the default
                            build: the option is refused, test_gpu_parity.py::test_chained_decode_launches_match_plain_launches)
  batch-chunk4 (3, 9)       ops.BatchDecode: 3 clips, chunks of 4 frames, resumed twice (zeggs_decoder_fwd_batch)
  entry points              zeggs_devectorize_output_fwd / _bwd, zeggs_vectorize_input_fwd / _bwd (funcs.hip), per row
  pack key                  ops.decoder_prepare with other statistics than the call that follows

Measured on an MI355X, worst over kinds and weightings (outputs: max |device - oracle64| over the 8 groups; root_rot on still / zero
against its own bound (T - 1) 1e-6; gradients: worst slice of helpers.decoder_grad_slices relative to its own largest entry):
  path (B, T)             outputs tied / untied / still / brisk / spin [/ zero]          worst gradient slice over kinds
  generic (2, 6)          8.1e-7  7.9e-7  7.9e-7  4.0e-6  3.4e-6                         3.5e-6
  stage (5, 6)            9.7e-7  1.0e-6  1.0e-6  3.7e-6  3.9e-6                         6.3e-6
  stage (33, 4)           1.0e-6  1.0e-6  1.0e-6  4.0e-6  4.1e-6                         3.4e-6
  tp16-tiles4=0 (5, 6)    8.9e-7  8.4e-7  8.4e-7  3.7e-6  3.9e-6                         2.5e-6
  tp16-tiles4=1 (5, 6)    8.9e-7  8.4e-7  8.4e-7  3.7e-6  3.9e-6                         2.4e-6
  tp4 (17, 5)             9.8e-7  1.1e-6  9.7e-7  4.0e-6  3.9e-6                         3.3e-6
  dual (17, 5)            8.3e-7  8.5e-7  8.5e-7  4.0e-6  3.9e-6                         4.9e-6
  bptt (5, 6)             8.9e-7  8.4e-7  8.4e-7  3.7e-6  3.9e-6                         2.7e-6
  bptt (17, 5)            9.8e-7  1.1e-6  9.7e-7  4.0e-6  3.9e-6                         3.6e-6
  bptt (40, 4)            1.2e-6  1.2e-6  1.2e-6  4.0e-6  4.0e-6                         2.9e-6
  film (5, 6)             6.1e-7  5.8e-7  5.8e-7  3.5e-6  3.9e-6                         4.7e-6
  h512 (2, 6)             8.0e-7  8.0e-7  8.0e-7  3.3e-6  3.8e-6                         7.2e-6 (spin, GRU layer 0 speech columns)
  ring (3, 7)             8.4e-7  8.0e-7  8.0e-7  3.9e-6  4.0e-6  8.0e-7
  b1-persistent (1, 6)    4.4e-7  4.5e-7  4.5e-7  3.5e-6  2.9e-6  4.5e-7
  b1-persistent (1, 37)   7.9e-7  8.6e-7  8.6e-7  4.5e-6  7.2e-6  8.6e-7
  b1-stage-gemv (1, 37)   6.2e-7  5.9e-7  5.9e-7  6.7e-6  9.1e-6  6.3e-7
  b1-stage-mfma (1, 37)   7.4e-7  7.7e-7  7.7e-7  9.3e-6  9.2e-6  7.7e-7
  batch-chunk4 (3, 9)     9.1e-7  9.0e-7  9.0e-7  3.6e-6  3.9e-6  9.0e-7
  root_rot on still / zero: <= 2.8e-8 per step (bound 1e-6 per step; 5.7e-7 over the 36 steps of (1, 37)); packs of other statistics
  dropped: outputs 1.0e-6, gradients 1.3e-6; entry points: row gradients <= 2.9e-6 of the row's largest entry (h = 2.8, root_rot)
  No case needed a wider bound and no kernel was found wrong: the float32 oracle itself reaches 4.0e-6 / 5.0e-6 on these cases.
  Under `root` weighting on `still` the output layer's bias entries [3:6] are 5e-5 ... 1.5e-4 of the tensor's largest entry (printed
  per case): their own error is 3e-8 ... 2.2e-7.
"""
import contextlib
import copy
import warnings

import numpy as np
import pytest
import torch

import helpers as H
from oracle import nets as onets
from zeggs import generate, ops, synth
from zeggs import modules as zmod

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEFAULTS = dict(decoder_fast=1, tp_dual=0, tp_tiles4=1, train_persistent=1, bwd_persistent=1, persistent=1, stage_variant=0)
TRAIN_OPTIONS = {"generic": dict(decoder_fast=0), "stage": dict(train_persistent=0, bwd_persistent=0),
                 "tp16-tiles4=0": dict(tp_tiles4=0, bwd_persistent=0), "tp16-tiles4=1": dict(bwd_persistent=0),
                 "tp4": dict(bwd_persistent=0), "dual": dict(tp_dual=1, bwd_persistent=0), "bptt": {}, "film": {}, "h512": {}}
# which persistent kernels (zeggs_persistent_state index) must have run; every other state must be unchanged by the case
TRAIN_RAN = {"generic": (), "stage": (), "tp16-tiles4=0": (1,), "tp16-tiles4=1": (1,), "tp4": (1,), "dual": (1,), "bptt": (1, 2),
             "film": (), "h512": ()}
INFER_OPTIONS = {"ring": {}, "b1-persistent": {}, "b1-stage-gemv": dict(persistent=0),
                 "b1-stage-mfma": dict(persistent=0, stage_variant=1024), "batch-chunk4": {}}
INFER_RAN = {"ring": (), "b1-persistent": (0,), "b1-stage-gemv": (), "b1-stage-mfma": (), "batch-chunk4": (1,)}


def g(t):
    return t.to(DEV)


@contextlib.contextmanager
def options(**kw):
    """library switches for one case (tp_dual before train_persistent, as the dual-chain tests set them); every switch this file
    touches goes back to its default afterwards; a give-up warning of a persistent kernel is an error here"""
    try:
        for k in DEFAULTS:
            if k in kw:
                ops.set_option(k, kw[k])
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            yield
    finally:
        for k, v in DEFAULTS.items():
            ops.set_option(k, v)


def _states():
    return [ops.lib().zeggs_persistent_state(k) for k in (0, 1, 2)]


def _assert_ran(before, ran, tag):
    after = _states()
    for k in (0, 1, 2):
        if k in ran:
            assert after[k] == 1, (tag, "persistent kernel %d did not run (state %d)" % (k, after[k]))
        else:
            assert after[k] == before[k], (tag, k, before, after)


_NETS = {}


def _net(tag):
    if tag not in _NETS:
        _NETS[tag] = copy.deepcopy(H.decoder_net(tag)).to(DEV)
    return _NETS[tag]


def _stats(kind):
    s = H.decoder_stats(kind, device=DEV)
    return [s[k] for k in ("in_mean", "in_std", "out_mean", "out_std")]


def _train(net, B, T, kind, wt, stats=None):
    """one training-mode rollout + backward of the case on the device -> (8 outputs, {name: gradient})"""
    de = _net(net).train()
    de.zero_grad()
    case = H.decoder_case(B, T)
    sp, sy = g(case["speech"]).requires_grad_(True), g(case["style"]).requires_grad_(True)
    out = de(*[g(t) for t in case["fp"]], g(case["gaze"]), sp, sy, None, *(stats or _stats(kind)), synth.DT)
    sum((o * g(w)).sum() for o, w in zip(out, H.decoder_weighting(wt, B, T))).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in de.named_parameters()}
    grads["speech"], grads["style"] = sp.grad.cpu(), sy.grad.cpu()
    return [o.detach().cpu() for o in out], grads


def _check_training(tag, net, B, T, kind, wt, out, grads):
    ref, gref = H.decoder_oracle_cached(net, B, T, kind, wt)
    H.assert_half_turns(kind, ref)                       # from the oracle's own root_vrt, before looking at the device
    eo = H.decoder_output_errors(out, ref)
    eg = H.decoder_slice_errors(grads, gref)
    worst = max(eg, key=eg.get)
    print(f"STATS {tag} ({B}, {T}) {kind} {wt}: outputs {max(eo.values()):.2e} root_rot {eo['root_rot']:.2e} gradients {eg[worst]:.2e} "
          f"({worst})")
    if kind == "still" and wt == "root":
        last = "recurrent_decoder." + ("layer3" if net == "film" else "layer2")
        r = gref[last + ".bias"]
        print(f"      rows [3:6] of {last}.bias are {float(r[3:6].abs().max() / r.abs().max()):.1e} of its largest entry; their own "
              f"error {eg[last + '.bias[3:6]']:.2e}, the whole tensor's {eg[last + '.bias']:.2e}")
    H.assert_decoder_outputs(kind, out, ref, T)
    H.assert_decoder_grads(grads, gref, (tag, kind, wt))


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("kind,wt", H.DEC_TRAIN_KINDS, ids=_id)
@pytest.mark.parametrize("path,net,B,T", H.DEC_TRAIN_CASES, ids=_id)
def test_training_path_vs_float64_oracle(path, net, B, T, kind, wt):
    """forward outputs and every gradient slice of one training path under one statistics kind and weighting"""
    with options(**TRAIN_OPTIONS[path]):
        before = _states()
        out, grads = _train(net, B, T, kind, wt)
        _assert_ran(before, TRAIN_RAN[path], path)
    _check_training(path, net, B, T, kind, wt, out, grads)


def _infer(path, B, T, kind):
    de = _net("main").eval()
    case = H.decoder_case(B, T)
    stats = _stats(kind)
    with torch.no_grad():
        if path != "batch-chunk4":
            out = de(*[g(t) for t in case["fp"]], g(case["gaze"]), g(case["speech"]), g(case["style"]), None, *stats, synth.DT)
            torch.cuda.synchronize()
            return [o.cpu() for o in out]
        # B clips of T frames on B rows in chunks of 4 frames: T = 9 is 3 + 3 + 2 new frames, the last chunk padded to the 4
        # frames the sweep needs; every chunk resumes from the state the one before left
        bd = ops.BatchDecode(de, B, 4, 64, 64, *stats, synth.DT)
        assert bd.sweep
        fp = case["fp"]
        pose0 = torch.cat([fp[i].reshape(B, -1) for i in range(2, 8)], dim=1)
        firsts = [tuple(g(t[b:b + 1]).contiguous() for t in (pose0, fp[0], fp[1], case["gaze"][:, 0])) for b in range(B)]
        plan = generate.plan_slots([T] * B, B, 4)
        assert len(plan) == 3
        acc, infos = [[[], [], []] for _ in range(B)], []
        for pieces, pose, rpos, rrot in generate.decode_plan(bd, firsts, [g(case["speech"][b]) for b in range(B)],
                                                             [g(case["style"][b]) for b in range(B)], plan, infos=infos):
            for r, j, k, n in pieces:
                for a, t in zip(acc[j], (pose, rpos, rrot)):
                    a.append(t[r, 0 if k == 0 else 1:n + 1].cpu())
        torch.cuda.synchronize()
        assert [i["path"] for i in infos] == ["persistent"] * 3 and ops.batch_last_path() == "persistent"
        pose, rpos, rrot = (torch.stack([torch.cat(a[i]) for a in acc]) for i in range(3))
        return [rpos, rrot] + list(H.unpack_pose(pose))


@pytest.mark.parametrize("kind", H.DEC_INFER_KINDS)
@pytest.mark.parametrize("path,B,T", H.DEC_INFER_CASES, ids=_id)
def test_inference_path_vs_float64_oracle(path, B, T, kind):
    """forward only; `zero`: a half turn of exactly 0 (out_std[3:6] = 0), finite and equal to the oracle under the bounds of `still`"""
    if path == "batch-chunk4" and ops.lib().zeggs_persistent_state(1) != 1:
        _train("main", 17, 5, "tied", "all")             # (the sweep's first use on a process is validated by a training rollout)
    ref, _ = H.decoder_oracle_cached("main", B, T, kind)
    H.assert_half_turns(kind, ref)
    with options(**INFER_OPTIONS[path]):
        before = _states()
        out = _infer(path, B, T, kind)
        _assert_ran(before, INFER_RAN[path], path)
    eo = H.decoder_output_errors(out, ref)
    print(f"STATS {path} ({B}, {T}) {kind} -: outputs {max(eo.values()):.2e} root_rot {eo['root_rot']:.2e}")
    H.assert_decoder_outputs(kind, out, ref, T)


# ----------------------------------------------------------------------------- the stand-alone entry points (funcs.hip)
ENTRY_H = (0.0, 3e-7, 4e-6, 2.5e-5, 1e-3, 0.02, 0.3, 0.97, 0.999, 1.001, 1.4, 2.8)


def _entry_stats(dtype, device="cpu"):
    """untied statistics with out_mean[3:6] = -out_std[3:6]: pred[3:6] = 1 is then a turn of EXACTLY zero in float32 and float64
    (1 * s - s), with a non-zero mean in the way"""
    s = H.decoder_stats("untied", dtype, device)
    s["out_mean"][3:6] = -s["out_std"][3:6]
    return s


def test_devectorize_entry_point_at_every_branch_per_row():
    """zeggs_devectorize_output_fwd / _bwd, one call of 12 rows whose half turn takes ENTRY_H -- both sides of 1e-5 and of 1 --
    against oracle.nets.devectorize_output in float64 PER ROW (a per-batch maximum would hide a small-angle row behind a large one):
    values 1e-4 max(1, |ref|), gradients 2e-5 of the row's largest entry (test_gpu_reference_side.py::
    test_vectorize_devectorize_vs_oracle).  Row 0 (h = 0) is forward only: the reference's gradient is NaN there, the kernel's must
    be finite."""
    B, J = len(ENTRY_H), synth.NJ
    s32, s64 = _entry_stats(torch.float32), _entry_stats(torch.float64)
    rng = np.random.default_rng(21)
    pred = rng.standard_normal((B, synth.POSE_OUT))
    u = rng.standard_normal((B, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    vrt = u * (2.0 * np.asarray(ENTRY_H) / synth.DT)[:, None]
    pred[:, 3:6] = (vrt - s64["out_mean"][3:6].numpy()) / s64["out_std"][3:6].numpy()
    pred[0, 3:6] = 1.0
    pred = torch.as_tensor(pred.astype(np.float32))
    q = torch.as_tensor(rng.standard_normal((B, 4)).astype(np.float32))
    q = q / q.norm(dim=-1, keepdim=True)
    rp0 = torch.as_tensor(rng.standard_normal((B, 3)).astype(np.float32)) * 50
    pr, rp, rq = pred.double().requires_grad_(), rp0.double().requires_grad_(), q.double().requires_grad_()
    ref = onets.devectorize_output(pr, rp, rq, J, synth.DT, s64["out_mean"], s64["out_std"])
    h = 0.5 * synth.DT * ref[3].detach().norm(dim=-1)
    assert float(h[0]) == 0.0
    for i in range(1, B):                                # the rows are where they are meant to be, same side of both branch points
        assert abs(float(h[i]) / ENTRY_H[i] - 1.0) < 1e-2, (i, float(h[i]))
        assert (float(h[i]) < 1e-5) == (ENTRY_H[i] < 1e-5) and (float(h[i]) < 1.0) == (ENTRY_H[i] < 1.0)
    ws = [torch.as_tensor(np.random.default_rng(30 + i).standard_normal(tuple(o.shape))) for i, o in enumerate(ref)]
    sum((o[1:] * w[1:]).sum() for o, w in zip(ref, ws)).backward()          # (row 0 stays out of the reference's backward)
    pg, rpg, rqg = (t.to(DEV).requires_grad_() for t in (pred, rp0, q))
    outs = zmod.devectorize_output(pg, rpg, rqg, B, J, synth.DT, g(s32["out_mean"]), g(s32["out_std"]))
    sum((o * g(w.float())).sum() for o, w in zip(outs, ws)).backward()
    torch.cuda.synchronize()
    for i in range(B):
        for n, o, r in zip(H.DEC_NAMES, outs, ref):
            e = float((o[i].detach().cpu().double() - r[i].detach()).abs().max())
            assert e < 1e-4 * max(1.0, float(r[i].detach().abs().max())), (ENTRY_H[i], n, e)
        for k, a, b in (("pred", pg, pr), ("root_pos", rpg, rp), ("root_rot", rqg, rq)):
            got = a.grad[i].cpu().double()
            assert bool(torch.isfinite(got).all()), (ENTRY_H[i], k)
            if i > 0:
                scale = max(1e-6, float(b.grad[i].abs().max()))
                e = float((got - b.grad[i]).abs().max()) / scale
                print(f"STATS entry h={ENTRY_H[i]:g} {k}: gradient error {e:.2e} of the row's largest entry")
                assert e < 2e-5, (ENTRY_H[i], k, e)
    # the norm of new_root_rot: the small branch loses 1e-5, the others nothing (unit root_rot)
    nrm = outs[1].detach().cpu().double().norm(dim=-1)
    for i in range(B):
        want = 1.0 / (1.0 + 1e-5) if ENTRY_H[i] < 1e-5 else 1.0
        assert abs(float(nrm[i]) - want) < 1e-6, (ENTRY_H[i], float(nrm[i]))


def test_vectorize_entry_point_untied_statistics_per_row():
    """zeggs_vectorize_input_fwd / _bwd with the untied statistics, per row, bounds of test_vectorize_devectorize_vs_oracle"""
    B, J = 12, synth.NJ
    s32, s64 = _entry_stats(torch.float32), _entry_stats(torch.float64)
    rng = np.random.default_rng(22)
    t = lambda *sh: torch.as_tensor(rng.standard_normal(sh).astype(np.float32))  # noqa: E731
    q = t(B, 4)
    P = [t(B, 3) * 50, q / q.norm(dim=-1, keepdim=True), t(B, 3), t(B, 3), t(B, J, 3) * 10, t(B, J, 2, 3), t(B, J, 3), t(B, J, 3),
         t(B, 3) * 100]
    ref_in = [p.double().requires_grad_() for p in P]
    xr = onets.vectorize_input(*ref_in, s64["in_mean"], s64["in_std"])
    w = torch.as_tensor(rng.standard_normal(tuple(xr.shape)))
    (xr * w).sum().backward()
    got_in = [p.to(DEV).requires_grad_() for p in P]
    x = zmod.vectorize_input(*got_in, None, g(s32["in_mean"]), g(s32["in_std"]))
    (x * g(w.float())).sum().backward()
    torch.cuda.synchronize()
    for i in range(B):
        assert float((x[i].detach().cpu().double() - xr[i].detach()).abs().max()) < 1e-4 * max(1.0, float(xr[i].detach().abs().max())), i
        for k, a, b in zip(H.DEC_NAMES + ("gaze_pos",), got_in, ref_in):
            scale = max(1e-6, float(b.grad[i].abs().max()))
            assert float((a.grad[i].cpu().double() - b.grad[i]).abs().max()) < 2e-5 * scale, (i, k)


# ----------------------------------------------------------------------------- the key of the prepared packs (ops.decoder_prepare)
def test_prepared_packs_are_keyed_by_the_statistics():
    """ops.decoder_prepare folds the four statistics vectors into the weight packs.  Packs made with statistics A must not serve a
    training-mode decoder_core with statistics B (same weights, same dimensions): the call must make its own and meet the bounds
    against the oracle at B.  The legitimate order (prepare with B, run with B) picks the packs up (prepared_hits) and meets the
    same bounds."""
    net, B, T, wt = "main", 17, 5, "all"
    with options():
        _train(net, B, T, "tied", wt)                    # validates both persistent kernels on this process
        assert _states()[1:] == [1, 1]
        de = _net(net).train()
        A, Bs = _stats("tied"), _stats("untied")
        side = ops.side_stream(DEV)
        ctx = ops.EngineContext()
        with ops.use(ctx):
            mask = ops.decoder_prepare(de, B, T, 64, 64, *A, synth.DT, side)
            assert mask > 0 and ctx.prepared is not None
            out, grads = _train(net, B, T, "untied", wt, stats=Bs)
            assert ctx.prepared_hits == 0 and ctx.prepared is None           # dropped, not picked up
            _check_training("stale-packs", net, B, T, "untied", wt, out, grads)
            mask = ops.decoder_prepare(de, B, T, 64, 64, *Bs, synth.DT, side)
            assert mask > 0
            out, grads = _train(net, B, T, "untied", wt, stats=Bs)
            assert ctx.prepared_hits == 1 and ctx.prepared is None
            _check_training("own-packs", net, B, T, "untied", wt, out, grads)
        assert _states()[1:] == [1, 1]
