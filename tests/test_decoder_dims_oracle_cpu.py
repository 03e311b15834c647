"""CPU side of tests/test_gpu_decoder_dims.py (no GPU): what makes the device comparison at other skeletons, encoding sizes and
hidden widths meaningful.
  (i)   attainable bounds: on every (decoder, B, T, statistics kind) the GPU file runs, the FLOAT32 oracle stays within a quarter of
        every bound the GPU file applies to the device (outputs, norm of root_rot, every gradient slice) against the float64 oracle
  (ii)  the inputs exercise the edges: with the weights of the last (partial) tile of PO, of XD or of H zeroed in the oracle, the
        outputs of every shape of that decoder move by >= 10x their bound (and, on the training shape, some gradient slice does too)
  (iii) the expectation table helpers.decoder_dim_limits / decoder_dim_ran against the limits written out by hand per rig

Measured (this file):
  (i)   float32 oracle: outputs <= 6.5e-6 (bound 1e-4), worst gradient slice <= 4.7e-6 (bound 3e-4), half turn per frame in
        [4.9e-3, 3.9e-2] everywhere (the polynomial branch, as `tied` / `untied` at 75 joints)
  (ii)  outputs: PO edge 3300x ... 29000x, H edge 540x ... 6600x, XD edge 36x ... 230x (the one to five last style columns; FiLM: the
        last speech column); gradients on the training shape: >= 400x, the XD edge in dstyle (FiLM: dspeech)"""
import pytest
import torch

import helpers as H

QUARTER = 0.25
TRAIN_SHAPES = H.decoder_dim_shapes(True)
INFER_SHAPES = H.decoder_dim_shapes(False)


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _assert_outputs_quarter(kind, o32, ref, T):
    eo = H.assert_decoder_outputs(kind, o32, ref, T)                    # the assertions the GPU file makes ...
    assert max(eo.values()) < QUARTER * H.DEC_OUT_BOUND, eo             # ... and a quarter of each
    if kind != "tied":
        assert float(H.root_norm_change(o32).abs().max()) < QUARTER * 2e-6
    return eo


@pytest.mark.parametrize("net,B,T,kind", TRAIN_SHAPES, ids=_id)
def test_float32_oracle_within_a_quarter_of_every_bound(net, B, T, kind):
    """(i) training shapes: outputs and every slice of helpers.decoder_grad_slices; the half turn stays in the polynomial branch"""
    ref, gref = H.decoder_dim_oracle_cached(net, B, T, kind, "all")
    lo, hi = H.assert_half_turns(kind, ref)
    o32, g32 = H.decoder_dim_oracle_cached(net, B, T, kind, "all", torch.float32)
    eo = _assert_outputs_quarter(kind, o32, ref, T)
    eg = H.decoder_slice_errors(g32, gref)
    worst = max(eg, key=eg.get)
    print(f"{net} ({B}, {T}) {kind}: h in [{lo:.2e}, {hi:.2e}]; float32 oracle outputs {max(eo.values()):.2e}, worst gradient slice "
          f"{eg[worst]:.2e} ({worst})")
    assert eg[worst] < QUARTER * min(H.DEC_GRAD_BOUND, *(H.DEC_SLICE_BOUNDS.get(k, H.DEC_GRAD_BOUND) for k in eg)), (worst, eg[worst])
    d = H.decoder_dims(net)
    for k in ("speech", "style"):                                      # the slices follow the rig's widths
        assert gref[k].shape[-1] == (d["SP"] if k == "speech" else d["ST"])
    slices = H.decoder_grad_slices(gref)
    p = "recurrent_decoder."
    assert slices[p + "layer0.weight[:, pose[6:]]"].shape[1] == d["PO"] - 6 and slices[p + "layer0.weight[:, gaze]"].shape[1] == 3
    assert slices[p + "layer0.weight[:, speech]"].shape[1] == d["SP"]
    assert slices[p + "layer1.weight_ih_l0[:, hid]"].shape[1] == d["H"]
    if d["film"]:
        assert p + "layer0.weight[:, style]" not in slices and slices[p + "layer3.bias[3:6]"].numel() == 3
    else:
        assert slices[p + "layer0.weight[:, style]"].shape[1] == d["ST"] and slices[p + "layer2.bias[3:6]"].numel() == 3
        assert slices[p + "layer1.weight_ih_l0[:, style]"].shape[1] == d["ST"]


@pytest.mark.parametrize("net,B,T,kind", INFER_SHAPES, ids=_id)
def test_float32_oracle_within_a_quarter_of_every_bound_inference(net, B, T, kind):
    """(i) inference shapes: outputs"""
    ref, _ = H.decoder_dim_oracle_cached(net, B, T, kind)
    H.assert_half_turns(kind, ref)
    o32, _ = H.decoder_dim_oracle_cached(net, B, T, kind, None, torch.float32)
    eo = _assert_outputs_quarter(kind, o32, ref, T)
    print(f"{net} ({B}, {T}) {kind}: float32 oracle outputs {max(eo.values()):.2e}")


@pytest.mark.parametrize("edge", ("PO", "XD", "H"))
@pytest.mark.parametrize("net", sorted(H.DEC_DIM_NETS))
def test_every_tile_edge_carries_signal(net, edge):
    """(ii) helpers.decoder_edge_zeroed: the oracle with the edge's weights zeroed against the oracle, on EVERY shape of the decoder
    (untied): outputs >= 10x DEC_OUT_BOUND -- the inference paths have nothing but outputs to show an edge with --, and on the
    decoder's first training shape some gradient slice >= 10x DEC_GRAD_BOUND as well"""
    lo, hi = H.decoder_dim_edges(net)[edge]
    d = H.decoder_dims(net)
    assert 0 <= lo < hi == d[edge] and hi - lo <= (5 if edge == "H" else 16)
    de = H.decoder_edge_zeroed(net, edge)
    shapes = [s for s in H.decoder_dim_shapes() if s[0] == net and s[3] == "untied"]
    first = next(c[1:] for c in H.DEC_DIM_TRAIN_CASES if c[1] == net)
    for _, B, T, kind in shapes:
        ref, _ = H.decoder_dim_oracle_cached(net, B, T, kind)
        ob, _ = H.decoder_dim_oracle(net, B, T, kind, de=de)
        eo = max(H.decoder_output_errors(ob, ref).values())
        print(f"{net} {edge} [{lo}:{hi}] ({B}, {T}): outputs move by {eo:.2e} = {eo / H.DEC_OUT_BOUND:.0f}x the bound")
        assert eo >= 10 * H.DEC_OUT_BOUND, (net, edge, B, T, eo)
    _, B, T, kind = first
    _, gref = H.decoder_dim_oracle_cached(net, B, T, kind, "all")
    _, gb = H.decoder_dim_oracle(net, B, T, kind, "all", de=de)
    eg = H.decoder_slice_errors(gb, gref)
    worst = max(eg, key=eg.get)
    print(f"{net} {edge} ({B}, {T}): gradient slice {worst} moves by {eg[worst]:.2e} = {eg[worst] / H.DEC_GRAD_BOUND:.0f}x the bound")
    assert eg[worst] >= 10 * H.DEC_GRAD_BOUND, (net, edge, worst, eg[worst])


# (iii) by hand, per decoder: (PO, XD, SP + ST, KBC, nTPO, 2 H + XD) and which kernels take it.  T = true, F = false.
#   fast: H % 16 == 0 and PO >= 16                 (decoder_fast.hip dec_fast_supported; PI == PO + 3 holds for every rig)
#   tp:   fast, normal, H == 1024, 16 <= PO <= 1280, SP + ST <= 128, 1 <= KBC <= 8               (train_persistent.hip)
#   bp:   fast, normal, H == 1024, PO >= 16, nTPO = (PO + 15) / 16 <= 72, XD <= 2048             (train_bwd_persistent.hip)
#   dp:   normal, H == 1024, 2 H + XD <= 3328, SP + ST <= 128, 6 <= PO <= 1280                   (decode_persistent.hip)
T_, F_ = True, False
BY_HAND = {
    # tag           PO = 6 + 15 J   XD = PO + 3 + SP + ST    SP+ST KBC nTPO 2H+XD   fast tp  bp  dp
    "j24":          (6 + 15 * 24,   366 + 3 + 64 + 64,       128,  8,  23,  2545,   T_,  T_, T_, T_),   # KBC = 8 <= 8; 2545 <= 3328
    "j6":           (6 + 15 * 6,    96 + 3 + 32 + 16,        48,   3,  6,   2195,   T_,  T_, T_, T_),
    "j1":           (6 + 15 * 1,    21 + 3 + 8 + 4,          12,   1,  2,   2084,   T_,  T_, T_, T_),   # PO = 21 >= 16
    "j76":          (6 + 15 * 76,   1146 + 3 + 64 + 64,      128,  8,  72,  3325,   T_,  T_, T_, T_),   # nTPO = 72 <= 72; 3325 <= 3328
    "j77":          (6 + 15 * 77,   1161 + 3 + 64 + 64,      128,  8,  73,  3340,   T_,  T_, F_, F_),   # nTPO = 73 > 72; 3340 > 3328
    "j86":          (6 + 15 * 86,   1296 + 3 + 64 + 64,      128,  8,  81,  3475,   T_,  F_, F_, F_),   # PO = 1296 > 1280; nTPO = 81
    "wide-cond":    (6 + 15 * 24,   366 + 3 + 100 + 64,      164,  11, 23,  2581,   T_,  F_, T_, F_),   # SP + ST = 164 > 128; bp: no such limit
    "h16":          (96,            147,                     48,   3,  6,   179,    T_,  F_, F_, F_),   # H != 1024
    "h48":          (96,            147,                     48,   3,  6,   243,    T_,  F_, F_, F_),
    "h80":          (96,            147,                     48,   3,  6,   307,    T_,  F_, F_, F_),
    "film-j24-h48": (366,           366 + 3 + 64,            64,   4,  23,  529,    T_,  F_, F_, F_),   # FiLM: the style is no step input
    "h24-generic":  (96,            147,                     48,   3,  6,   195,    F_,  F_, F_, F_),   # 24 % 16 = 8
}
# which persistent kernels (zeggs_persistent_state index: 0 decode, 1 rollout, 2 BPTT) each path of the GPU file must have run
RAN_BY_HAND = {
    ("stage", "j24"): (), ("tp16-tiles4=0", "j24"): (1,), ("tp16-tiles4=1", "j24"): (1,), ("tp4", "j24"): (1,), ("dual", "j24"): (1,),
    ("bptt", "j24"): (1, 2), ("b1-persistent", "j24"): (0,), ("b1-stage-gemv", "j24"): (), ("b1-stage-mfma", "j24"): (), ("ring", "j24"): (),
    ("batch-chunk4", "j24"): (1,),
    ("stage", "j6"): (), ("tp16-tiles4=0", "j6"): (1,), ("tp16-tiles4=1", "j6"): (1,), ("tp4", "j6"): (1,), ("dual", "j6"): (1,),
    ("bptt", "j6"): (1, 2), ("b1-persistent", "j6"): (0,), ("b1-stage-gemv", "j6"): (), ("b1-stage-mfma", "j6"): (), ("ring", "j6"): (),
    ("batch-chunk4", "j6"): (1,),
    ("stage", "j1"): (), ("tp16-tiles4=1", "j1"): (1,), ("bptt", "j1"): (1, 2), ("b1-persistent", "j1"): (0,),
    ("bptt", "j76"): (1, 2), ("b1-persistent", "j76"): (0,),
    ("default", "j77"): (1,), ("b1-default", "j77"): (),               # the rollout runs, the BPTT sweep and the decode kernel decline
    ("default", "j86"): (), ("b1-default", "j86"): (),
    ("stage", "wide-cond"): (), ("default", "wide-cond"): (2,), ("ring", "wide-cond"): (), ("b1-default", "wide-cond"): (),
    ("default", "film-j24-h48"): (), ("ring", "film-j24-h48"): (), ("default", "h24-generic"): (),
}
for _h in ("h16", "h48", "h80"):
    for _p in ("generic", "stage", "ring", "b1-stage-gemv", "b1-stage-mfma"):
        RAN_BY_HAND[(_p, _h)] = ()


@pytest.mark.parametrize("net", sorted(H.DEC_DIM_NETS))
def test_expectation_table_agrees_with_the_limits_by_hand(net):
    PO, XD, C, KBC, nTPO, two_h_xd, fast, tp, bp, dp = BY_HAND[net]
    d = H.decoder_dims(net)
    assert (d["PO"], d["XD"], d["SP"] + (0 if d["film"] else d["ST"])) == (PO, XD, C) and d["PI"] == PO + 3
    assert ((C + 15) // 16, (PO + 15) // 16, 2 * d["H"] + XD) == (KBC, nTPO, two_h_xd)
    assert H.decoder_dim_limits(net) == dict(fast=fast, tp=tp, bp=bp, dp=dp)


def test_every_case_has_an_expectation_by_hand():
    cases = {(c[0], c[1]) for c in H.DEC_DIM_TRAIN_CASES + H.DEC_DIM_INFER_CASES}
    assert cases == set(RAN_BY_HAND)
    for path, net in sorted(cases):
        assert H.decoder_dim_ran(path, net) == RAN_BY_HAND[(path, net)], (path, net)
    for c in H.DEC_DIM_TRAIN_CASES:
        assert c[0] in H.DEC_DIM_TRAIN_OPTIONS and c[2] <= 40 and 4 <= c[3] <= 9
    for c in H.DEC_DIM_INFER_CASES:
        assert c[0] in H.DEC_DIM_INFER_OPTIONS and c[2] <= 40 and 4 <= c[3] <= 9
    for rig in H.DEC_DIM_RIGS:                                         # `tied` on one case per rig
        assert any(H.DEC_DIM_NETS[c[1]][0] == rig and c[4] == "tied" for c in H.DEC_DIM_TRAIN_CASES), rig


def test_the_75_joint_helpers_are_unchanged():
    """the joint-count argument of decoder_weighting defaults to today's weights; the new rigs leave the 75-joint caches alone"""
    a, b = H.decoder_weighting("all", 2, 4), H.decoder_weighting("all", 2, 4, 75)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[4].shape == (2, 4, 75, 3)
    assert H.decoder_weighting("all", 2, 4, 6)[5].shape == (2, 4, 6, 2, 3)
    case = H.decoder_dim_case("j6", 3, 5)
    q, txy = case["fp"][1].double(), case["fp"][5].double()
    assert float((q.norm(dim=-1) - 1).abs().max()) < 1e-6
    assert float(((txy * txy).sum(-1) - 1).abs().max()) < 1e-6 and float((txy[:, :, 0] * txy[:, :, 1]).sum(-1).abs().max()) < 1e-6
    PI, PO, st = H.decoder_rig(6, 32, 16, "tied")
    assert (PI, PO) == (99, 96) and torch.equal(st["out_mean"], st["in_mean"][:PO]) and int((st["out_std"] == 0).sum()) == 96 // 28
    _, _, su = H.decoder_rig(6, 32, 16, "untied")
    assert not torch.equal(su["out_mean"], su["in_mean"][:PO]) and torch.equal(su["in_std"], st["in_std"])
