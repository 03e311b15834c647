"""The recurrent style encoder (style_encoder.type = "gru": csrc/style_gru.hip, sg_fast_* in csrc/decoder_fast.hip) at other hidden
widths, batch blocks, encoding sizes and lengths than the one architecture of tests/test_gpu_parity.py (H = 512, B = 2 / 19 / 32 /
35, backward at L >= 7 only).

Every case of helpers.STYLE_GRU_ROWS runs forward + backward of sum(z wz + mu wm + logvar wl) in .train() mode (the encoder has no
dropout) on seeded randn inputs and is compared
  * with the float64 oracle (oracle/nets.py, pinned at these very shapes by tests/test_style_gru_oracle_cpu.py, which also shows
    that four wrong encoders are > 10x these bounds away): outputs max |got - ref| < 5e-5, every parameter gradient in full
    relerr < 3e-4 -- the bounds of test_gpu_parity.py::test_gru_style_encoder_stage_path_batch; the two ReLUs through
    helpers.oracle_at_kinks;
  * exactly: weight_hh_l0_reverse.grad == 0 everywhere (one step from the zero state), weight_hh_l0.grad == 0 at L = 1 (Hs[0] = 0);
  * fast rows: with the same run under decoder_fast = 0 (a product and a gate kernel per frame): outputs 2e-5, gradients 1e-4, the
    cross-path bounds of the same existing test.
Which path serves a case is asserted without a hook: zeggs_style_encoder_gru_workspace_bytes is larger under decoder_fast = 1 than
under decoder_fast = 0 exactly when sg_fast_supported(B, H) holds (carve_sg adds sg_fast_carve's buffers then).

Dispatch (launch_stage_f: NB = ceil(B / 16) blocks of 16 batch rows; the launch is split in two over the batch when every tile count
is below 160 and NB is even; forward tiles nT5 = ceil(H / 5), backward tiles nTH = H / 16; stage_k<rows blocks per workgroup,
family 0 forward / 1 backward, waves>; sg_args clears `gemv`, so B = 1 is an MFMA launch with 15 padded rows):
  H    S   (B, L)                              forward                       backward
  16   8   (1,1) (1,2) (16,3)                  <1,0,8>                       <1,1,8>      nT5 = 4, last tile 1 live unit; one k-block:
           (17,2)                              <1,0,8> split                 <1,1,8> split  seven of eight waves get none; (1,1): the
                                                                                          only backward launch has nseg == 0
  48   64  (17,2)                              <1,0,8> split                 <1,1,8> split  nT5 = 10, nTH = 3 (whole tiles)
           (48,3)                              <3,0,16>                      <3,1,16>
  80   20  (33,3)                              <3,0,16>                      <3,1,16>     projection width 40
           (64,2)                              <2,0,8> split                 <2,1,8> split
  512  64  (1,40)                              <1,0,8>                       <1,1,8>      the shape of generate_gesture()
           (49,3) (64,1) (64,2)                <2,0,8> split                 <2,1,8> split  49: last block of 16 has one live row;
                                                                                          (64,1): nseg == 0 only, four blocks
  800  64  (1,2)                               <1,0,8>                       <1,1,8>      nT5 = 160: forward never split, last tile
           (32,2)                              <2,0,8>                       <1,1,8> split  full; nTH = 50: backward split
           (64,2)                              <4,0,16> (one k-block per     <2,1,8> split
                                               buffer)
  24   64  (5,4)                               generic (H % 16 == 8)
  30   64  (3,5)                               generic; rows of no buffer 16-byte aligned
  512  64  (65,2)                              generic (B > 64)

Three further tests: the bytes behind the workspace (raw ABI, a pattern behind `workspace_bytes`), the refusals of the raw ABI, and
the independence of a batch row from its company (padded rows must not leak into live ones).

Found by this file: zeggs_style_encoder_gru_fwd / _bwd accepted a workspace up to 255 bytes shorter than
zeggs_style_encoder_gru_workspace_bytes asks for (the carve's end, not the size the library reports, was what they checked); they
now refuse anything below the reported size, as the loss and the batched mel entry points do.  No kernel was wrong.

Measured on an MI355X (outputs: max |got - ref| over z, mu, logvar; gradients: relerr of the worst parameter tensor; bounds 5e-5 /
3e-4 against the oracle, 2e-5 / 1e-4 fast against generic):
  H     path      vs oracle: outputs       gradients           fast vs generic: outputs   gradients
  16    fast      7.9e-8 .. 1.5e-6         3.1e-7 .. 1.9e-6    1.2e-7 .. 2.4e-7           1.3e-7 .. 3.2e-7
  48    fast      1.3e-6 .. 1.5e-6         1.5e-6              2.4e-7                     1.7e-7 .. 2.4e-7
  80    fast      1.5e-6 .. 1.7e-6         9.6e-7 .. 2.1e-6    2.4e-7                     1.8e-7 .. 1.9e-7
  512   fast      5.0e-7 .. 1.9e-6         5.0e-7 .. 1.5e-6    0 .. 4.8e-7                1.1e-7 .. 4.2e-7
  800   fast      5.8e-7 .. 2.2e-6         5.6e-7 .. 1.3e-6    2.4e-7 .. 4.8e-7           2.3e-7 .. 4.3e-7
  24    generic   1.0e-6                   1.9e-6
  30    generic   9.1e-7                   2.1e-6
  512   generic   1.9e-6 (B = 65)          1.3e-6
Two cases had one ReLU unit within helpers.KINK of its kink (H 512, B 64, L 1 and H 800, B 64, L 2); no other case had any.  Rows
0..4 of the B = 49 call equal the B = 5 call exactly, row 0 of B = 16 and the B = 1 call differ by 1.2e-6.  The 23 tests take 4.3 s
in one process, the float64 oracle included."""
import pytest
import torch

import helpers
from zeggs import ops, synth
from zeggs.capi import STYLE_GRU_FIELDS, StyleGruDims, StyleGruPtrs, api

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = helpers.STYLE_GRU_TEMPERATURE
OUT_BOUND, GRAD_BOUND = helpers.STYLE_GRU_OUT_BOUND, helpers.STYLE_GRU_GRAD_BOUND
CROSS_OUT_BOUND, CROSS_GRAD_BOUND = 2e-5, 1e-4      # test_gpu_parity.py::test_gru_style_encoder_stage_path_batch, fast vs generic
POINTS = helpers.style_gru_points()
W_HH, W_HH_R = "encoder.rnn_layer.weight_hh_l0", "encoder.rnn_layer.weight_hh_l0_reverse"
g = lambda t: t.to(DEV)  # noqa: E731


class _generic_path:
    """decoder_fast = 0 inside the block, the default (1) behind it"""

    def __enter__(self):
        ops.set_option("decoder_fast", 0)

    def __exit__(self, *exc):
        ops.set_option("decoder_fast", 1)
        return False


def _ws_bytes(B, L, H, O):
    return int(api().zeggs_style_encoder_gru_workspace_bytes(StyleGruDims(B, L, synth.POSE_IN, H, O)))


def _run(st, x, eps, wts):
    st.zero_grad(set_to_none=True)
    outs = st(g(x), T, eps=g(eps))
    sum((o * g(w)).sum() for o, w in zip(outs, wts)).backward()
    torch.cuda.synchronize()
    return tuple(o.detach().cpu().double() for o in outs), {k: p.grad.detach().clone() for k, p in st.named_parameters()}


def _out_err(a, b):
    return max(float((x.double().cpu() - y.double().cpu()).abs().max()) for x, y in zip(a, b))


@pytest.mark.parametrize("H,S,B,L,path", POINTS, ids=["H{}-S{}-B{}-L{}-{}".format(*p) for p in POINTS])
def test_gru_style_encoder_dims(H, S, B, L, path):
    ws_fast = _ws_bytes(B, L, H, 2 * S)
    with _generic_path():
        ws_generic = _ws_bytes(B, L, H, 2 * S)
    assert ws_fast >= ws_generic and (ws_fast > ws_generic) == (path == "fast"), (ws_fast, ws_generic)
    assert (path == "fast") == (H % 16 == 0 and 1 <= B <= 64)                          # sg_fast_supported
    st = helpers.build_style_gru(H, S).to(DEV).train()
    x, eps, wts = helpers.style_gru_case(H, S, B, L)
    outs, grads = _run(st, x, eps, wts)
    for o in outs:
        assert o.shape == (B, S) and bool(torch.isfinite(o).all())
    ref_outs, ref_grads, near, flipped = helpers.oracle_at_kinks(
        lambda: helpers.oracle_style(st, x, eps, wts, temperature=T), grads)
    e_out, e_grad = _out_err(outs, ref_outs), helpers.worst_relerr(grads, ref_grads)
    msg = f"\ngru H={H} S={S} B={B} L={L} {path}: outputs {e_out:.2e}, worst gradient {e_grad:.2e}, near kinks {len(near)}"
    e_xo = e_xg = None
    if path == "fast":
        with _generic_path():
            outs2, grads2 = _run(st, x, eps, wts)
        e_xo, e_xg = _out_err(outs, outs2), helpers.worst_relerr(grads, grads2)
        msg += f"; fast vs generic outputs {e_xo:.2e}, gradients {e_xg:.2e}"
    print(msg)
    assert e_out < OUT_BOUND, e_out
    for k in ref_grads:
        assert helpers.relerr(grads[k], ref_grads[k]) < GRAD_BOUND, k
    assert int(torch.count_nonzero(grads[W_HH_R])) == 0
    if L == 1:
        assert int(torch.count_nonzero(grads[W_HH])) == 0
    else:
        assert int(torch.count_nonzero(grads[W_HH])) > 0
    if path == "fast":
        assert e_xo < CROSS_OUT_BOUND, e_xo
        for k in grads:
            assert helpers.relerr(grads[k], grads2[k]) < CROSS_GRAD_BOUND, k
        assert int(torch.count_nonzero(grads2[W_HH_R])) == 0 and (L > 1 or int(torch.count_nonzero(grads2[W_HH])) == 0)


# ----------------------------------------------------------------------------- the raw ABI
def _params(st):
    """the parameter tensors in the order of ZeggsStyleGruParams (ops.style_encoder_gru)"""
    enc = st.encoder
    r, pl = enc.rnn_layer, enc.projection_layer.linear_layer
    ps = [enc.convs[0].conv.weight, enc.convs[0].conv.bias, enc.convs[2].conv.weight, enc.convs[2].conv.bias, r.weight_ih_l0,
          r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0, r.weight_ih_l0_reverse, r.weight_hh_l0_reverse, r.bias_ih_l0_reverse,
          r.bias_hh_l0_reverse, pl.weight, pl.bias]
    assert len(ps) == len(STYLE_GRU_FIELDS)
    return [p.detach().contiguous() for p in ps]


GUARD, GUARD_BYTE, WS_BYTE = 4096, 0xA5, 0x7F


@pytest.mark.parametrize("H,S,B,L", [(16, 8, 17, 2), (80, 20, 33, 3), (512, 64, 49, 3)])
def test_workspace_guard_and_raw_abi_equals_the_binding(H, S, B, L):
    """Forward + backward through the raw ABI in a workspace of exactly `workspace_bytes` (pre-filled with 0x7f bytes: 3.4e38 as a
    float, so that a read of bytes nobody wrote would show) followed by 4 KiB of 0xa5: the pattern is intact afterwards, and the
    outputs and all 14 gradients equal those of the binding the module calls (ops.style_encoder_gru and its backward, in a workspace
    of torch.empty) bit for bit.  Both run inside ops.fixed_order_gemms() and on the calling thread (the switch is the thread's, so
    the binding's backward is called directly instead of through autograd's worker): without it the products split their
    contraction over workgroups and combine with float atomics, whose order changes from call to call.  The column sums keep their
    atomics; at these shapes (L B <= 147 rows, at most two row chunks) a sum of two terms onto zero has one value in either order."""
    st = helpers.build_style_gru(H, S).to(DEV).train()
    x, _, _ = helpers.style_gru_case(H, S, B, L)
    x = g(x).contiguous()
    gen = torch.Generator().manual_seed(B * L)
    dout = g(torch.randn(B, 2 * S, generator=gen))
    with ops.fixed_order_gemms():
        out_m = ops.style_encoder_gru(x, st.encoder)
        rets = ops._StyleGruFn.backward(out_m.grad_fn, dout)
        assert rets[0] is None and len(rets) == 15 and all(r is not None for r in rets[1:])
        grads_m = [r.clone() for r in rets[1:]]
        out_m = out_m.detach().clone()
        torch.cuda.synchronize()

        d = StyleGruDims(B, L, synth.POSE_IN, H, 2 * S)
        need = _ws_bytes(B, L, H, 2 * S)
        buf = torch.empty(need + GUARD, dtype=torch.uint8, device=DEV)
        buf[:need] = WS_BYTE
        buf[need:] = GUARD_BYTE
        params = _params(st)
        out = torch.full((B, 2 * S), 7.0, device=DEV)
        grads = [torch.full_like(p, 7.0) for p in params]
        P, G = ops._ptrs(StyleGruPtrs, STYLE_GRU_FIELDS, params), ops._ptrs(StyleGruPtrs, STYLE_GRU_FIELDS, grads)
        api().zeggs_style_encoder_gru_fwd(d, P, x, out, buf, need, ops._stream())
        api().zeggs_style_encoder_gru_bwd(d, P, dout, G, buf, need, ops._stream())
        torch.cuda.synchronize()
    assert bool((buf[need:] == GUARD_BYTE).all()), "bytes behind the workspace were written"
    assert torch.equal(out, out_m)
    for name, a, b in zip(STYLE_GRU_FIELDS, grads, grads_m):
        assert torch.equal(a, b), name
    assert ops.lib().zeggs_gemm_fixed_order(0) == 0          # the thread is as it was


def test_raw_abi_refusals():
    """a workspace one byte short of what the library asks for, an empty batch, an empty sequence: each is refused with its message
    before anything is launched (the output buffer keeps its pattern)"""
    H, S, B, L = 16, 8, 17, 2
    st = helpers.build_style_gru(H, S).to(DEV)
    x = g(helpers.style_gru_case(H, S, B, L)[0]).contiguous()
    params = _params(st)
    P = ops._ptrs(StyleGruPtrs, STYLE_GRU_FIELDS, params)
    need = _ws_bytes(B, L, H, 2 * S)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    out = torch.full((B, 2 * S), 7.0, device=DEV)
    for dims, nbytes, msg in ((StyleGruDims(B, L, synth.POSE_IN, H, 2 * S), need - 1, "workspace too small"),
                              (StyleGruDims(0, L, synth.POSE_IN, H, 2 * S), need, "empty batch or sequence"),
                              (StyleGruDims(B, 0, synth.POSE_IN, H, 2 * S), need, "empty batch or sequence")):
        with pytest.raises(RuntimeError, match=msg):
            api().zeggs_style_encoder_gru_fwd(dims, P, x, out, ws, nbytes, ops._stream())
        assert ops.lib().zeggs_style_encoder_gru_fwd(*_raw_args(dims, P, x, out, ws, nbytes)) != 0
        assert msg in ops.lib().zeggs_last_error().decode()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    # the backward holds the workspace to the same size
    grads = [torch.empty_like(p) for p in params]
    G = ops._ptrs(StyleGruPtrs, STYLE_GRU_FIELDS, grads)
    with pytest.raises(RuntimeError, match="workspace too small"):
        api().zeggs_style_encoder_gru_bwd(StyleGruDims(B, L, synth.POSE_IN, H, 2 * S), P, out, G, ws, need - 1, ops._stream())
    # and the exact size is accepted
    api().zeggs_style_encoder_gru_fwd(StyleGruDims(B, L, synth.POSE_IN, H, 2 * S), P, x, out, ws, need, ops._stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any())


def _raw_args(dims, P, x, out, ws, nbytes):
    import ctypes as C
    return (C.byref(dims), C.byref(P), ops._p(x), ops._p(out), ops._p(ws), C.c_size_t(nbytes), ops._stream())


def test_a_row_does_not_depend_on_its_company():
    """H = 512: rows 0..4 of a B = 49 call (four blocks, split launch, the last block one live row) equal the B = 5 call on those rows,
    and the row of a B = 1 call (15 padded rows) equals row 0 of a B = 16 call, within the cross-path output bound (the k-split over
    the waves differs with the instantiation, so not bit for bit).  A padded batch row leaking into a live one would show here."""
    H, S, L = 512, 64, 3
    st = helpers.build_style_gru(H, S).to(DEV).train()
    x, eps, _ = helpers.style_gru_case(H, S, 49, L)

    def fwd(rows):
        with torch.no_grad():
            outs = st(g(x[rows].contiguous()), T, eps=g(eps[rows].contiguous()))
        torch.cuda.synchronize()
        return [o.cpu() for o in outs]

    full, five, sixteen, one = fwd(slice(0, 49)), fwd(slice(0, 5)), fwd(slice(0, 16)), fwd(slice(0, 1))
    e5 = _out_err([o[:5] for o in full], five)
    e1 = _out_err([o[:1] for o in sixteen], one)
    print(f"\ngru H=512 L=3: rows 0..4 of B=49 vs B=5 {e5:.2e}; row 0 of B=16 vs B=1 {e1:.2e}")
    assert e5 < CROSS_OUT_BOUND and e1 < CROSS_OUT_BOUND, (e5, e1)
    # (and the rows differ from each other by far more than that: the comparison is not between equal rows)
    assert float((full[1][0] - full[1][1]).abs().max()) > 1e3 * CROSS_OUT_BOUND
