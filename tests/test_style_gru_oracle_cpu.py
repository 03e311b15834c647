"""The float64 oracle of the recurrent style encoder (oracle/nets.py style_encoder_gru) at every shape of helpers.STYLE_GRU_ROWS,
without a GPU.  tests/test_gpu_style_gru_dims.py holds the device to this oracle at those shapes; one fixture (variants.npz) pins
the oracle to the reference, at H = 512 only.  Here, at every (H, S, B, L) of the matrix:

  * the oracle agrees with a restatement written from torch's own layers -- F.conv1d, F.relu, nn.GRU(H, H, 1, batch_first=True,
    bidirectional=True) taking output[:, -1], F.linear -- to 1e-12 absolute on the outputs and 1e-12 of a gradient's largest entry
    (float64; measured 6e-17 .. 1.3e-15 and 2.8e-16 .. 8.6e-16);
  * float32 torch on the CPU is within 5e-6 of the float64 oracle on the outputs (measured 1.1e-7 .. 9.4e-7): the floor under the
    device's output bound of 5e-5;
  * the gradient of weight_hh_l0_reverse is exactly zero (only output[:, -1] is used: the reverse direction takes one step from the
    zero state), and that of weight_hh_l0 is exactly zero at L = 1.

Negative controls, at one (B, L) of every row of the matrix and at the inference shape (512, 1, 40): four wrong encoders -- (a) the
reverse direction fed x[0] instead of x[L - 1], (b) b_hn added outside r * (...), (c) unit H - 1 of the final forward state zeroed
(a dropped partial tile), (d) the last batch row's final state replaced by its neighbour's -- are each more than 10x the device
bounds (outputs 5e-5, gradients 3e-4 of the largest entry) away from the oracle, on outputs and on the worst parameter gradient.
Measured: outputs >= 1.7e-2 ((c) at H = 512, B = 1, L = 40), gradients >= 0.28 ((d) at H = 512, B = 49, L = 3)."""
import pytest
import torch
import torch.nn.functional as F

import helpers

T = helpers.STYLE_GRU_TEMPERATURE
P = "encoder."
GRU_NAMES = [n + sfx for sfx in ("", "_reverse") for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
POINTS = helpers.style_gru_points()
# one (B, L) per row with L >= 2 and B >= 2 (every control applies), and the inference shape (no neighbour row: (a) - (c))
CONTROL_POINTS = [(16, 8, 17, 2), (48, 64, 17, 2), (80, 20, 33, 3), (512, 64, 49, 3), (512, 64, 1, 40), (800, 64, 32, 2),
                  (24, 64, 5, 4), (30, 64, 3, 5), (512, 64, 65, 2)]


def _ids(points):
    return ["H{}-S{}-B{}-L{}".format(*p[:4]) for p in points]


def _vae(out, eps, S):
    mu, logvar = out[:, :S], out[:, S:]
    return mu + eps * torch.exp(0.5 * logvar) / T, mu, logvar


def _finish(outs, wts, w):
    sum((o * wt.to(o.dtype)).sum() for o, wt in zip(outs, wts)).backward()
    return tuple(o.detach() for o in outs), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in w.items()}


def restated(st, x, eps, wts, dtype):
    """the encoder from torch's own layers in `dtype` -> ((z, mu, logvar), {state-dict name: gradient})"""
    w = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in st.state_dict().items()}
    H = w[P + "convs.0.conv.weight"].shape[0]
    gru = torch.nn.GRU(H, H, 1, batch_first=True, bidirectional=True).to(dtype)
    gru.load_state_dict({n: w[P + "rnn_layer." + n].detach() for n in GRU_NAMES})
    h = F.relu(F.conv1d(x.to(dtype).transpose(1, 2), w[P + "convs.0.conv.weight"], w[P + "convs.0.conv.bias"], padding=1))
    h = F.relu(F.conv1d(h, w[P + "convs.2.conv.weight"], w[P + "convs.2.conv.bias"], padding=1))
    y, _ = gru(h.transpose(1, 2))
    out = F.linear(y[:, -1], w[P + "projection_layer.linear_layer.weight"], w[P + "projection_layer.linear_layer.bias"])
    outs, grads = _finish(_vae(out, eps.to(dtype), eps.shape[1]), wts, w)
    for n in GRU_NAMES:
        grads[P + "rnn_layer." + n] = getattr(gru, n).grad
    return outs, grads


def _cell(x, h, w_ih, w_hh, b_ih, b_hh, bhn_outside):
    H = h.shape[-1]
    gi, gh = F.linear(x, w_ih, b_ih), F.linear(h, w_hh)
    r = torch.sigmoid(gi[:, :H] + gh[:, :H] + b_hh[:H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H] + b_hh[H:2 * H])
    if bhn_outside:
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:] + b_hh[2 * H:])
    else:
        n = torch.tanh(gi[:, 2 * H:] + r * (gh[:, 2 * H:] + b_hh[2 * H:]))
    return (1.0 - z) * n + z * h


def by_hand(st, x, eps, wts, wrong=None):
    """the encoder step by step in float64; wrong = None (the encoder itself) or one of "a" .. "d" (module docstring)"""
    w = helpers.f64_weights(st)
    x = x.double()
    h = F.relu(F.conv1d(x.transpose(1, 2), w[P + "convs.0.conv.weight"], w[P + "convs.0.conv.bias"], padding=1))
    h = F.relu(F.conv1d(h, w[P + "convs.2.conv.weight"], w[P + "convs.2.conv.bias"], padding=1)).transpose(1, 2)
    B, L, H = h.shape
    fw = [w[P + "rnn_layer." + n] for n in GRU_NAMES[:4]]
    rv = [w[P + "rnn_layer." + n] for n in GRU_NAMES[4:]]
    hf = torch.zeros(B, H, dtype=h.dtype)
    for t in range(L):
        hf = _cell(h[:, t], hf, *fw, bhn_outside=wrong == "b")
    hb = _cell(h[:, 0 if wrong == "a" else L - 1], torch.zeros(B, H, dtype=h.dtype), *rv, bhn_outside=wrong == "b")
    if wrong == "c":
        hf = torch.cat([hf[:, :H - 1], torch.zeros(B, 1, dtype=h.dtype)], dim=1)
    if wrong == "d":
        hf = torch.cat([hf[:B - 1], hf[B - 2:B - 1]], dim=0)
    out = F.linear(torch.cat([hf, hb], dim=-1), w[P + "projection_layer.linear_layer.weight"],
                   w[P + "projection_layer.linear_layer.bias"])
    return _finish(_vae(out, eps.double(), eps.shape[1]), wts, w)


def _out_err(a, b):
    return max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))


@pytest.mark.parametrize("H,S,B,L,path", POINTS, ids=_ids(POINTS))
def test_oracle_equals_torch_layers(H, S, B, L, path):
    st = helpers.build_style_gru(H, S)
    x, eps, wts = helpers.style_gru_case(H, S, B, L)
    outs, grads = helpers.oracle_style(st, x, eps, wts, temperature=T)
    r_outs, r_grads = restated(st, x, eps, wts, torch.float64)
    e_out, e_grad = _out_err(outs, r_outs), helpers.worst_relerr(r_grads, grads)
    f_outs, _ = restated(st, x, eps, wts, torch.float32)
    e_f32 = _out_err(outs, f_outs)
    print(f"\ngru oracle H={H} S={S} B={B} L={L}: vs torch layers outputs {e_out:.1e} gradients {e_grad:.1e}; float32 outputs {e_f32:.1e}")
    assert e_out <= 1e-12 and e_grad <= 1e-12, (e_out, e_grad)
    assert e_f32 < 5e-6, e_f32
    for o in outs:
        assert o.shape == (B, S)
    assert torch.count_nonzero(grads[P + "rnn_layer.weight_hh_l0_reverse"]) == 0
    assert grads[P + "rnn_layer.weight_hh_l0"].shape == (3 * H, H)
    if L == 1:
        assert torch.count_nonzero(grads[P + "rnn_layer.weight_hh_l0"]) == 0
    else:
        assert torch.count_nonzero(grads[P + "rnn_layer.weight_hh_l0"]) > 0


@pytest.mark.parametrize("H,S,B,L", CONTROL_POINTS, ids=_ids(CONTROL_POINTS))
def test_wrong_encoders_are_far_from_the_oracle(H, S, B, L):
    st = helpers.build_style_gru(H, S)
    x, eps, wts = helpers.style_gru_case(H, S, B, L)
    outs, grads = helpers.oracle_style(st, x, eps, wts, temperature=T)
    h_outs, h_grads = by_hand(st, x, eps, wts)
    assert _out_err(outs, h_outs) <= 1e-12 and helpers.worst_relerr(h_grads, grads) <= 1e-12      # the controls' base is the oracle
    kinds = [k for k in "abcd" if not (k == "a" and L < 2) and not (k == "d" and B < 2)]
    assert len(kinds) >= 3
    for kind in kinds:
        w_outs, w_grads = by_hand(st, x, eps, wts, wrong=kind)
        e_out, e_grad = _out_err(outs, w_outs), helpers.worst_relerr(w_grads, grads)
        print(f"\ngru control ({kind}) H={H} S={S} B={B} L={L}: outputs {e_out:.1e}, worst gradient {e_grad:.1e}")
        assert e_out >= 10 * helpers.STYLE_GRU_OUT_BOUND, (kind, e_out)
        assert e_grad >= 10 * helpers.STYLE_GRU_GRAD_BOUND, (kind, e_grad)


def test_control_points_cover_every_row():
    rows = {(H, S, path) for H, S, _, path in helpers.STYLE_GRU_ROWS}
    pts = {p[:4]: p[4] for p in POINTS}
    assert {(H, S, pts[(H, S, B, L)]) for H, S, B, L in CONTROL_POINTS} == rows


def test_relu_sites_sees_the_gru_oracle():
    """helpers.oracle_at_kinks is of use to the device test only if the oracle's two ReLUs go through F.relu"""
    st = helpers.build_style_gru(16, 8)
    x, eps, wts = helpers.style_gru_case(16, 8, 2, 3)
    with helpers.relu_sites() as rs:
        helpers.oracle_style(st, x, eps, wts, temperature=T)
    assert rs.n == 2
