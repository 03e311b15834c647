"""CPU side of tests/test_gpu_decoder_stats.py (no GPU): the float64 oracle alone shows that every (shape, statistics kind) of the
GPU file lies in the branch of the quaternion exponential it is meant for, and that the GPU file's bounds are sharp -- each bug
model below moves the float64 oracle by a stated multiple of the bound that is meant to trip.  The float32 oracle against the
float64 oracle on the same cases is the yardstick of those bounds.

Measured (float64 oracle, this file, over every shape and the three decoders):
  half turn h = dt / 2 |root_vrt|: tied [1.8e-3, 1.2e-2], untied [7.6e-3, 2.4e-2], still [2.0e-8, 9.9e-7], brisk [0.942, 0.954],
    spin [1.189, 1.202], zero 0 exactly
  (i)   fold without (mu_o - mu_i): worst output group 0.26 ... 1.3 (bound 1e-4), every gradient tensor >= 3.4e-3 (bound 3e-4)
  (ii)  eps = 0 on `still`: root_rot (T - 1) 1e-5 (5.0e-5 at T = 6) = 9.95x ... 10x its bound (T - 1) 1e-6; every other output group
        <= 4.9e-5 and every gradient slice <= 1.4e-4: only the tightened root_rot bound and the norm assertion see it
  (iii) gaze gradient cut, `root` weighting: worst slice >= 3.6e-3 (bound 3e-4) at every kind; `still` / `untied`: output-layer weight
        rows [3:6] 9.6e-3 ... 5.0e-2, and on `still` no whole tensor exceeds 3.2e-4 -- the bias entries [3:6] are 5e-5 ... 1.5e-4 of
        their tensor's largest entry
  (iv)  stale fold (packs of A under B): worst output group 0.40 ... 1.0
  float32 oracle: outputs <= 4.0e-6 (root_rot 6.6e-7), every gradient slice <= 5.0e-6"""
import pytest
import torch

import helpers as H

TRAIN_SHAPES = sorted({c[1:] for c in H.DEC_TRAIN_CASES})
CONTROL_KINDS = ("untied", "still", "brisk", "spin")


def _last(net):
    return "recurrent_decoder." + ("layer3" if net == "film" else "layer2")


@pytest.mark.parametrize("net,B,T", H.decoder_shapes())
def test_every_kind_lies_in_its_branch(net, B, T):
    """the conditions of helpers.DEC_TURN_RANGE, and the norm of root_rot: it loses (T - 1) 1e-5 on `still` / `zero` (the small
    branch divides by |(1, x)| + 1e-5) and nothing otherwise"""
    for kind in H.DEC_INFER_KINDS:
        outs, _ = H.decoder_oracle_cached(net, B, T, kind)
        lo, hi = H.assert_half_turns(kind, outs)
        dn = H.root_norm_change(outs)
        print(f"{net} ({B}, {T}) {kind}: h in [{lo:.3e}, {hi:.3e}], norm change {float(dn.abs().max()):.3e}")
        if kind in ("still", "zero"):
            assert float((dn + (T - 1) * H.DEC_SMALL_EPS).abs().max()) < (T - 1) * 1e-7
        else:
            assert float(dn.abs().max()) < 1e-14
        assert all(bool(torch.isfinite(o).all()) for o in outs)


def test_kinds_differ_where_they_should():
    t, u = H.decoder_stats("tied"), H.decoder_stats("untied")
    PO = t["out_mean"].numel()
    assert float((t["in_mean"][:PO] - t["out_mean"]).abs().max()) == 0.0           # today's special point
    shift = (u["out_mean"] - u["in_mean"][:PO]) / u["in_std"][:PO]
    const = u["out_std"] == 0
    assert int(const.sum()) == 40 and float(shift[const].abs().min()) > 1e-3       # constant channels with a non-zero shift
    assert float(shift.abs().max()) > 1.0
    for k in ("in_mean", "in_std"):
        for kind in H.DEC_INFER_KINDS:
            assert torch.equal(H.decoder_stats(kind)[k], t[k])


@pytest.mark.parametrize("net,B,T", TRAIN_SHAPES)
def test_control_fold_without_the_mean_shift(net, B, T):
    """(i) in_mean[:PO] := out_mean -- what a fold that drops (mu_o - mu_i) computes: >= 100x the output bound on the worst output
    group, >= 5x the gradient bound on EVERY parameter tensor, dspeech and dstyle, at every kind and weighting"""
    for kind in CONTROL_KINDS:
        st = H.decoder_stats(kind)
        PO = st["out_mean"].numel()
        bug = dict(st, in_mean=torch.cat([st["out_mean"], st["in_mean"][PO:]]))
        for wt in ("all", "root"):
            outs, grads = H.decoder_oracle_cached(net, B, T, kind, wt)
            ob, gb = H.decoder_oracle(H.decoder_net(net), H.decoder_case(B, T), bug, H.decoder_weighting(wt, B, T))
            eo = max(H.decoder_output_errors(ob, outs).values())
            eg = {k: H.relerr(gb[k], grads[k]) for k in grads}
            worst = min(eg, key=eg.get)
            print(f"{net} ({B}, {T}) {kind} {wt}: outputs {eo:.2e} = {eo / H.DEC_OUT_BOUND:.0f}x, least gradient {eg[worst]:.2e} = "
                  f"{eg[worst] / H.DEC_GRAD_BOUND:.1f}x ({worst})")
            assert eo >= 100 * H.DEC_OUT_BOUND, (kind, wt, eo)
            assert eg[worst] >= 5 * H.DEC_GRAD_BOUND, (kind, wt, worst, eg[worst])


@pytest.mark.parametrize("net,B,T", TRAIN_SHAPES)
def test_control_small_branch_replaced_by_the_formula(net, B, T):
    """(ii) quat_exp(x, eps = 0) on `still`: root_rot moves by (T - 1) 1e-5, more than 9x its bound (T - 1) 1e-6; every other
    output group stays below the 1e-4 bound and every gradient slice below 3e-4 -- the tightened root_rot bound (and the norm
    assertion) is what catches it, no gradient bound could"""
    for wt in ("all", "root"):
        outs, grads = H.decoder_oracle_cached(net, B, T, "still", wt)
        ob, gb = H.decoder_oracle_cached(net, B, T, "still", wt, bug="eps0")
        eo = H.decoder_output_errors(ob, outs)
        eg = max(H.decoder_slice_errors(gb, grads).values())
        print(f"{net} ({B}, {T}) still {wt}: root_rot {eo['root_rot']:.3e} = {eo['root_rot'] / ((T - 1) * 1e-6):.2f}x its bound, other "
              f"outputs <= {max(v for k, v in eo.items() if k != 'root_rot'):.1e}, gradient slices <= {eg:.1e}")
        assert eo["root_rot"] > 9 * (T - 1) * 1e-6
        assert max(eo.values()) < H.DEC_OUT_BOUND and eg < H.DEC_GRAD_BOUND
        dn = H.root_norm_change(ob)
        assert float(dn.abs().max()) < 1e-9                      # the norm deficit is gone: the norm assertion trips as well


@pytest.mark.parametrize("net,B,T", TRAIN_SHAPES)
def test_control_gaze_gradient_cut(net, B, T):
    """(iii) detach inside vectorize_input, `root` weighting: some slice is off by >= 10x the bound at every kind.  Where: NOT in rows
    [0:3] of the output layer (root_vel reaches the gaze direction through root_pos only: <= 3.3e-4 of the slice).  On `still` and
    `untied` it is in rows [3:6] of the output layer's weight (root_vrt turns the frame the gaze direction is expressed in), >= 10x
    the bound at every shape, and on `still` NOWHERE else: no whole tensor reaches twice the bound -- that is what the slices are
    for.  On `brisk` / `spin` the turn per frame is large, the cut spreads over every tensor (dstyle, the CellStateEncoder) and rows
    [3:6] are not always the worst (2.7e-3 = 9x at (40, 4) brisk, where dstyle has 3.6e-3): there the worst slice is asserted."""
    for kind in CONTROL_KINDS:
        _, grads = H.decoder_oracle_cached(net, B, T, kind, "root")
        _, gb = H.decoder_oracle_cached(net, B, T, kind, "root", bug="gaze_detached")
        e = H.decoder_slice_errors(gb, grads)
        w36, b36 = e[_last(net) + ".weight[3:6]"], e[_last(net) + ".bias[3:6]"]
        whole = max(v for k, v in e.items() if "[" not in k)
        r = grads[_last(net) + ".bias"]
        ratio = float(r[3:6].abs().max() / r.abs().max())
        print(f"{net} ({B}, {T}) {kind}: weight rows [3:6] {w36:.2e} = {w36 / H.DEC_GRAD_BOUND:.0f}x, bias [3:6] {b36:.2e}, worst whole "
              f"tensor {whole:.2e}; bias rows [3:6] / largest entry = {ratio:.1e}")
        assert max(e.values()) >= 10 * H.DEC_GRAD_BOUND, (kind, max(e.values()))
        if kind in ("still", "untied"):
            assert w36 >= 10 * H.DEC_GRAD_BOUND, (kind, w36)
        if kind == "still":
            assert whole < 2 * H.DEC_GRAD_BOUND and ratio < 1e-3, (whole, ratio)


@pytest.mark.parametrize("A,Bk", [("tied", "untied"), ("untied", "tied"), ("untied", "spin")])
def test_control_stale_fold(A, Bk):
    """(iv) the weight packs fold statistics A, the call runs with statistics B (ops.decoder_prepare's packs picked up by a
    decoder_core with other statistics), at the shape of the pack test: >= 100x the output bound"""
    net, B, T = "main", 17, 5
    outs, _ = H.decoder_oracle_cached(net, B, T, Bk)
    ob, _ = H.decoder_oracle_cached(net, B, T, Bk, bug=("stale_fold", H.decoder_stats(A)))
    eo = max(H.decoder_output_errors(ob, outs).values())
    print(f"packs of {A} under {Bk}: outputs {eo:.2e} = {eo / H.DEC_OUT_BOUND:.0f}x")
    assert eo >= 100 * H.DEC_OUT_BOUND
    same, _ = H.decoder_oracle_cached(net, B, T, Bk, bug=("stale_fold", H.decoder_stats(Bk)))      # the model itself is exact
    assert max(H.decoder_output_errors(same, outs).values()) < 1e-12


@pytest.mark.parametrize("net,B,T", TRAIN_SHAPES)
def test_float32_oracle_yardstick(net, B, T):
    """the float32 oracle against the float64 oracle: what single precision costs on these cases, a tenth of the wider-bound
    threshold of helpers.DEC_SLICE_BOUNDS at the most (no slice qualifies for a wider bound)"""
    for kind, wt in H.DEC_TRAIN_KINDS:
        outs, grads = H.decoder_oracle_cached(net, B, T, kind, wt)
        o32, g32 = H.decoder_oracle(H.decoder_net(net), H.decoder_case(B, T), H.decoder_stats(kind), H.decoder_weighting(wt, B, T),
                                    torch.float32)
        eo = H.assert_decoder_outputs(kind, o32, outs, T)
        e = H.decoder_slice_errors(g32, grads)
        k = max(e, key=e.get)
        print(f"{net} ({B}, {T}) {kind} {wt}: float32 oracle outputs {max(eo.values()):.2e}, root_rot {eo['root_rot']:.2e}, worst "
              f"gradient slice {e[k]:.2e} ({k})")
        assert max(eo.values()) < 1e-5 and e[k] < 3e-5
        assert not H.DEC_SLICE_BOUNDS or all(v > 3e-4 for v in H.DEC_SLICE_BOUNDS.values())
