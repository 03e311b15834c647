"""The decoder at other skeletons, encoding sizes and hidden widths: every decoder path against oracle.nets.decoder_rollout in
float64 directly (never kernel against kernel), at rigs and widths that reach the tile edges of PO, XD, the conditioning blocks and
the GRU unit tiles, and both sides of every limit of the four *_supported predicates.

Why: PI, PO, SP, ST and H are free dimensions of the C ABI and of modules.Decoder, but every other decoder test builds one family
(75 joints: PI = 1134, PO = 1131; SP = ST = 64; H in {512, 768, 1024}).  helpers.DEC_DIM_RIGS / DEC_DIM_NETS name the rigs and
decoders, helpers.DEC_DIM_TRAIN_CASES / DEC_DIM_INFER_CASES the (path, decoder, B, T, statistics kind) of this file, and
helpers.decoder_dim_ran which persistent kernels each case must have run -- from the limits as the kernel files state them, checked
against a table written by hand in tests/test_decoder_dims_oracle_cpu.py, which also shows on the CPU that the float32 oracle stays
within a quarter of every bound used here and that each tile edge moves the outputs by >= 10x their bound when its weights are zeroed.

Per-frame operand buffers of the three persistent kernels (csrc/decoder_ws.h carve_dec / carve_dec_batch against what the launches
walk; XB = 256 NB floats per k-block, NB = (B + 15) / 16; T frames each, frames 1 .. T - 1 walked):
  buffer   allocated per frame            walked per frame                                          depends on
  G0xf     max(201, 64 + KBX + 64) x XB   201 blocks x XB: [hid 64 | gaze 1 | cond 8 | h0 64 | h1 64]   nothing (B only); was 64 + KBX + 64:
           (was (64 + KBX + 64) x XB in   (dec_tp_zero, tp_cond, tp_xfrag, the sweep, the dual chain)    SHORT for XD <= 1152, see below
           the training carve)
  G1xf     128 blocks x XB                128 x XB: [h0_t 64 | h1_{t-1} 64]                          nothing
  G3xf     (64 + KBC) x XB                64 + KBC: [h1_t 64 | cond_{t+1} KBC], KBC <= 8             SP + ST (KBC = (SP + ST + 15) / 16)
  bp_opy   nTPO x 512                     KBY x 512, KBY = (PO + 15) / 16 = nTPO (<= 72)             PO
  bp_op1   4 H x 32                       OPS = 4 H x 32 (op_idx: 32 batch rows of one sweep)        H (= 1024)
  bp_op0   4 H x 32                       OPS, and frame t + 1 <= T - 1                              H
  bp_opd   H x 32                         H x 32                                                     H
  bp_sp    9 x 32                         NSP = 9 root / gaze columns x 32 rows                      nothing
  pgran    36864 bytes in all             3 x 1024 + 5 x 256 granules of 8 bytes = 34816, then the    PO <= 1280 = 5 x 256 pose columns
                                          error word (dp_errword)                                    (dec_persistent_supported)
  Found: G0xf of the TRAINING carve was sized by 64 + KBX + 64 blocks per frame while every launch walks 201; for KBX < 73
  (XD <= 1152: every rig below 68 joints at SP + ST = 128) the last frames ran over into G1xf / G3xf.  carve_dec and carve_dec_batch
  now both size it by zeggs_tp::tp_g0_blocks (decoder_ws.h, where TKB0 is stated once): the 201 blocks walked; rigs with KBX > 73
  keep their 64 + KBX + 64 (207 at 75 joints), the sizes tests/test_abi.py pins.  Every other buffer is allocated as walked
  (tests/host/dec_ws_check.cpp asserts all of this on the host).

Which case launches which kernels: the paths of tests/test_gpu_decoder_stats.py (same options), plus `default` / `b1-default`: no
switch set, the limits alone decide -- j77: the rollout runs and the BPTT sweep declines (nTPO = 73), the decode kernel declines
(2 H + XD = 3340); j86: all three decline (PO = 1296); wide-cond: the rollout and the decode kernel decline (SP + ST = 164), the
BPTT sweep has no such limit and runs behind the stage forward; FiLM and H != 1024: stage launches only; h24-generic: H % 16 != 0,
the fast path declines (the library has no query for "generic or stage": the case asserts the results and that no persistent
kernel's state moved).

Measured on an MI355X (outputs: max |device - oracle64| over the 8 groups; gradients: worst slice of helpers.decoder_grad_slices
relative to its own largest entry; bounds 1e-4 / 3e-4):
  training: outputs / worst gradient slice
  decoder        stage (5, 6)      tp16-tiles4=0 / =1 (5, 6)   tp4 (17, 5)       dual (17, 5)      bptt (5, 6)  (17, 5)  (40, 4)             bptt (5, 6) tied
  j24            3.5e-6 / 1.1e-6   3.5e-6 / 9.4e-7 / 9.3e-7    2.7e-6 / 9.9e-7   2.7e-6 / 1.0e-6   3.5e-6 / 7.7e-7  2.7e-6 / 7.8e-7  4.8e-6 / 8.6e-7   2.8e-6 / 6.7e-7
  j6             2.3e-6 / 1.3e-6   2.3e-6 / 1.1e-6 / 1.1e-6    3.3e-6 / 9.6e-7   3.3e-6 / 9.3e-7   -                -                3.6e-6 / 1.0e-6   2.2e-6 / 1.1e-6
  j1             3.9e-6 / 3.1e-6   - / 3.7e-6 / 3.1e-6         -                 -                 3.7e-6 / 3.1e-6  -                -                 3.7e-6 / 3.2e-6
  j76            -                 -                           -                 -                 2.6e-6 / 8.3e-7  -                -                 3.6e-6 / 1.1e-6
  j77 default (5, 6): 2.0e-6 / 1.5e-6, tied 3.1e-6 / 1.2e-6 (ran: the rollout only);  j86 default (5, 4): 1.4e-6 / 1.6e-6, tied
  8.6e-7 / 1.3e-6 (none ran);  wide-cond stage (5, 6): 4.3e-6 / 1.4e-6, tied 6.5e-6 / 1.4e-6, default 4.3e-6 / 1.3e-6 (ran: the BPTT sweep only)
  decoder        generic (2, 6)    stage (5, 6)      stage (33, 4)
  h16            2.7e-6 / 4.7e-6   2.4e-6 / 3.3e-6   3.1e-6 / 1.6e-6
  h48            1.9e-6 / 1.2e-6   4.5e-6 / 1.9e-6   4.0e-6 / 1.4e-6
  h80            1.2e-6 / 1.2e-6   4.8e-6 / 1.2e-6   3.1e-6 / 1.0e-6
  film-j24-h48 (5, 6): 3.6e-6 / 1.6e-6;  h24-generic (2, 6): 2.4e-6 / 1.7e-6
  inference: outputs
  decoder        b1-persistent (1, 6)   b1-stage-gemv / -mfma (1, 6)   ring (3, 7)   batch-chunk4 (3, 9)
  j24            1.4e-6                 1.4e-6 / 1.4e-6                9.5e-7        2.3e-6
  j6             1.5e-6                 1.5e-6 / 1.5e-6                2.8e-6        2.9e-6
  j1 1.4e-6, j76 1.1e-6 (b1-persistent);  b1-default: j77 6.8e-7, j86 4.7e-7, wide-cond 8.6e-7 (the decode kernel declined);  wide-cond ring 2.6e-6
  h16 / h48 / h80: ring 3.6e-6 / 3.6e-6 / 2.9e-6, b1-stage-gemv = -mfma 6.7e-7 / 1.1e-6 / 6.8e-7;  film-j24-h48 ring 3.4e-6
  The output figures are those of the float32 oracle itself on the same cases (root_pos is 20 .. 60 units from the origin: half a
  unit in the last place is 1.9e-6), which is why different kernels share them.  No case needed a wider bound; with the carve of
  G0xf corrected before the first run of a small rig, no kernel was found wrong.
"""
import contextlib
import copy
import warnings

import pytest
import torch

import helpers as H
from zeggs import generate, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEFAULTS = dict(decoder_fast=1, tp_dual=0, tp_tiles4=1, train_persistent=1, bwd_persistent=1, persistent=1, stage_variant=0)


def g(t):
    return t.to(DEV)


@contextlib.contextmanager
def options(**kw):
    """library switches for one case (tp_dual before train_persistent); every switch this file touches goes back to its default
    afterwards; a give-up warning of a persistent kernel is an error here"""
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


def _stats(net, kind):
    s = H.decoder_dim_stats(net, kind, device=DEV)
    return [s[k] for k in ("in_mean", "in_std", "out_mean", "out_std")]


def _train(net, B, T, kind):
    """one training-mode rollout + backward of the case on the device, weighting `all` -> (8 outputs, {name: gradient})"""
    d = H.decoder_dims(net)
    de = _net(net).train()
    de.zero_grad()
    case = H.decoder_dim_case(d["rig"], B, T)
    sp, sy = g(case["speech"]).requires_grad_(True), g(case["style"]).requires_grad_(True)
    out = de(*[g(t) for t in case["fp"]], g(case["gaze"]), sp, sy, None, *_stats(net, kind), synth.DT)
    sum((o * g(w)).sum() for o, w in zip(out, H.decoder_weighting("all", B, T, d["J"]))).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in de.named_parameters()}
    grads["speech"], grads["style"] = sp.grad.cpu(), sy.grad.cpu()
    return [o.detach().cpu() for o in out], grads


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("path,net,B,T,kind", H.DEC_DIM_TRAIN_CASES, ids=_id)
def test_training_path_vs_float64_oracle(path, net, B, T, kind):
    """forward outputs and every gradient slice of one training path on one decoder"""
    ran = H.decoder_dim_ran(path, net)
    with options(**H.DEC_DIM_TRAIN_OPTIONS[path]):
        before = _states()
        out, grads = _train(net, B, T, kind)
        _assert_ran(before, ran, (path, net))
    ref, gref = H.decoder_dim_oracle_cached(net, B, T, kind, "all")
    H.assert_half_turns(kind, ref)
    eo = H.decoder_output_errors(out, ref)
    eg = H.decoder_slice_errors(grads, gref)
    worst = max(eg, key=eg.get)
    print(f"DIMS {net} {path} ({B}, {T}) {kind} ran={ran}: outputs {max(eo.values()):.2e} gradients {eg[worst]:.2e} ({worst})")
    H.assert_decoder_outputs(kind, out, ref, T)
    H.assert_decoder_grads(grads, gref, (path, net, kind))


def _infer(path, net, B, T, kind):
    d = H.decoder_dims(net)
    de = _net(net).eval()
    case = H.decoder_dim_case(d["rig"], B, T)
    stats = _stats(net, kind)
    with torch.no_grad():
        if path != "batch-chunk4":
            out = de(*[g(t) for t in case["fp"]], g(case["gaze"]), g(case["speech"]), g(case["style"]), None, *stats, synth.DT)
            torch.cuda.synchronize()
            return [o.cpu() for o in out]
        # B clips of T frames on B rows in chunks of 4 frames (T = 9: 3 + 3 + 2 new frames), each chunk resuming from the last
        want = "persistent" if H.decoder_dim_limits(net)["tp"] else "stage"
        bd = ops.BatchDecode(de, B, 4, d["SP"], d["ST"], *stats, synth.DT)
        assert bool(bd.sweep) == (want == "persistent")
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
        assert [i["path"] for i in infos] == [want] * 3 and ops.batch_last_path() == want
        pose, rpos, rrot = (torch.stack([torch.cat(a[i]) for a in acc]) for i in range(3))
        return [rpos, rrot] + list(H.unpack_pose_tree(pose, d["J"]))


@pytest.mark.parametrize("path,net,B,T,kind", H.DEC_DIM_INFER_CASES, ids=_id)
def test_inference_path_vs_float64_oracle(path, net, B, T, kind):
    """forward only: the ring, the B = 1 decode kernel and stage launches, the batch decode"""
    ran = H.decoder_dim_ran(path, net)
    if path == "batch-chunk4" and ran and ops.lib().zeggs_persistent_state(1) != 1:
        with options():
            _train(net, 17, 5, "tied")                   # (the sweep's first use on a process is validated by a training rollout)
    ref, _ = H.decoder_dim_oracle_cached(net, B, T, kind)
    H.assert_half_turns(kind, ref)
    with options(**H.DEC_DIM_INFER_OPTIONS[path]):
        before = _states()
        out = _infer(path, net, B, T, kind)
        _assert_ran(before, ran, (path, net))
    eo = H.decoder_output_errors(out, ref)
    print(f"DIMS {net} {path} ({B}, {T}) {kind} ran={ran}: outputs {max(eo.values()):.2e}")
    H.assert_decoder_outputs(kind, out, ref, T)
