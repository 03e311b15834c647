"""Training mode (dropout ON, VAE noise drawn inside the step) against a float64 oracle that is given THE DEVICE'S OWN masks.

Masks cannot be injected into the kernels, but they can be read back: zeggs_dropout(ones, n, p, seed) returns the keep-scale
of element i for (seed, i); include/zeggs_hip.h (beside zeggs_dropout) fixes each site's seed offset and element index, and
wrapping ops.next_seed tells which seed a call drew (helpers.recorded_seeds).  Each test runs the HIP path, rebuilds the masks
(and the VAE noise) the device used, and evaluates oracle/nets.py in float64 WITH those masks.  The oracle-with-masks is pinned to
the reference's training mode on the CPU (tests/test_oracle_golden.py, nets_train.npz / train_iter_dropout.npz), and the same file
proves that one wrong mask at any site of any shape below is > 10x the bounds used here (the negative controls).

Bounds (none new): outputs 2e-5 / parameter gradients 3e-4 (speech 1e-5 / 2e-4) -- those of
test_gpu_parity.py::test_style_encoder_forward_backward / test_speech_encoder_forward_backward, same relerr, same oracle;
engine step: those of test_gpu_parity.py::test_train_iteration_vs_reference, iteration 0.  Every parameter tensor is compared
in full.  Measured on an MI355X: outputs 1e-7 .. 1e-6, encoder gradients 3e-7 .. 2e-6, engine-step gradients 3e-6 .. 1.4e-5 of the
tensor's largest entry -- no bound had to be taken from the reference's own float32-vs-float64 gap (which train_iter_dropout.npz
records: 4.7e-4 at iteration 0 under dropout).  The file's 83 tests take 11 s there, the float64 oracle included.

Which case launches which kernel variant (the dispatch is a plain function of the width C, alignment and the options,
csrc/kernels.hip k_ln_fwd_fused / k_ln_bwd_fused, csrc/encoders.hip fuse0 / fuse, attention.hip attn_fused_supported):
  ln_*_fused4<32,1>   C <= 128, C % 4 == 0      E = 128 / 64 (every (512|130|520, 128) and (30, 64) case); H = 64 of (64, 520)
  ln_bwd_fused4<32,1,4>  the same, ln_bwd4 = 2  [512-128-*-ln_bwd4=2]
  ln_*_fused4<64,1>   128 < C <= 256            (200, 256) and (256, 192): H and E
  ln_*_fused4<64,2>   256 < C <= 512            H = 512
  ln_*_fused_k<2>     C <= 128 scalar lanes     H = 30 (C % 4 != 0, rows not 16-byte aligned); every ln_bwd4 = 0 case at E = 128
  ln_*_fused_k<8>     C > 128 scalar lanes      H = 130 (C % 4 != 0); ln_bwd4 = 0 at H = 512 and at (200, 256)
  unfused forward chain (k_layernorm_fwd_v, k_dropout_rows / k_dropout, k_pad_edges, k_add_rows_bcast, conv_gemm with bias)
  + ln_bwd_fused_k<16>  512 < C <= 1024         H = 520 of (520, 128), E = 520 of (64, 520)
  attention.hip DROP instantiations             every E = 128 case in training mode (fused_attention = 1), both
                                                attn_bwd_one_launch values
  GEMM + softmax_fwd_k (Pd) + softmax_bwd_k     E != 128 (head width != 32) and [*-fused_attention=0]
  act_bwd_k ys = 1 / keep, dropout_rows_k on padded buffers, k_dropout     the speech encoder cases
Until this file existed the BACKWARD of a width above 512 was refused (k_ln_bwd_fused: "C=520 > 512 unsupported") although the
forward ran: a style encoder with nhidden = 520 could not be trained.  The scalar-lane backward now serves rows up to 1024
floats; above that the refusal stays and is recorded with its message (test_style_backward_wider_than_1024_is_refused).
layernorm_bwd_k (k_layernorm_bwd_v) is launched by no encoder."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
from oracle import nets as onets
from oracle import radam as oradam
from zeggs import engine, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPTION_DEFAULTS = dict(fused_attention=1, attn_bwd_one_launch=1, ln_bwd4=1)
g = lambda t: t.to(DEV)  # noqa: E731


class _options:
    """set library options for a block, restore the defaults behind it"""

    def __init__(self, opts):
        self.opts = dict(opts)

    def __enter__(self):
        for k, v in self.opts.items():
            ops.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            ops.set_option(k, OPTION_DEFAULTS[k])
        return False


def _grads(module):
    return {k: p.grad.detach().cpu().double() for k, p in module.named_parameters()}


# ----------------------------------------------------------------------------- a. speech encoder
def _hip_speech(se, x, wgt, train):
    se.train(train)
    se.zero_grad()
    with helpers.recorded_seeds() as rec:
        out = se(g(x))
    (out * g(wgt)).sum().backward()
    torch.cuda.synchronize()
    return out.detach().cpu().double(), _grads(se), (rec.of("speech_encoder") if train else None), rec


@pytest.mark.parametrize("B,T", helpers.SPEECH_SHAPES)
@pytest.mark.parametrize("H,O", helpers.SPEECH_WIDTHS)
def test_speech_encoder_training_mode_vs_masked_oracle(H, O, B, T):
    """forward + every parameter gradient with dropout ON against the float64 oracle given the device's two masks (after each
    ELU, seed + 1 / seed + 2, element (b T + t) C + c); T = 31 and 15: the 31-tap replicate edges on a masked, padded buffer."""
    se = helpers.build_speech(H, O).to(DEV)
    x, wgt = helpers.speech_case(B, T, O, seed=300 + T)
    out, grads, seed, _ = _hip_speech(se, x, wgt, True)
    masks = helpers.device_masks_speech(seed, B, T, H, O)
    for m, p in zip(masks, onets.SPEECH_P):
        assert 0.4 * p < float((m == 0).double().mean()) < 1.6 * p + 0.02          # a mask, at roughly its rate
    ref_out, ref_grads = helpers.oracle_speech(se, x, wgt, masks)
    eo, eg = helpers.relerr(out, ref_out), helpers.worst_relerr(grads, ref_grads)
    print(f"\nspeech {H}/{O} B={B} T={T} training mode: output {eo:.2e}, worst gradient {eg:.2e}")
    assert eo < helpers.SPEECH_OUT_BOUND, eo
    for k in ref_grads:
        assert helpers.relerr(grads[k], ref_grads[k]) < helpers.SPEECH_GRAD_BOUND, k
    # the masks matter: without them the oracle is far away (the comparison above is not vacuous)
    assert helpers.relerr(out, helpers.oracle_speech(se, x, wgt, None)[0]) > 100 * helpers.SPEECH_OUT_BOUND


@pytest.mark.parametrize("B,T", helpers.SPEECH_SHAPES)
def test_speech_encoder_odd_widths_eval_mode_vs_oracle(B, T):
    """the width pair no other test builds (30 / 50: rows of neither buffer are 16-byte aligned), eval mode"""
    H, O = helpers.SPEECH_WIDTHS[1]
    se = helpers.build_speech(H, O).to(DEV)
    x, wgt = helpers.speech_case(B, T, O, seed=300 + T)
    out, grads, _, rec = _hip_speech(se, x, wgt, False)
    assert rec.draws == []                                                          # eval mode draws no seed
    ref_out, ref_grads = helpers.oracle_speech(se, x, wgt, None)
    assert helpers.relerr(out, ref_out) < helpers.SPEECH_OUT_BOUND
    for k in ref_grads:
        assert helpers.relerr(grads[k], ref_grads[k]) < helpers.SPEECH_GRAD_BOUND, k


# ----------------------------------------------------------------------------- b / c. style encoder
def _style_cases():
    out = []
    for (H, E), lengths in helpers.STYLE_MATRIX:
        for L in lengths:
            out.append((H, E, L, {}))
        two = lengths if (H, E) != (512, 128) else (77, 128)
        if E == 128:        # the fused attention kernels serve this width only: both paths, both backward forms
            for L in two:
                out.append((H, E, L, dict(fused_attention=0)))
                out.append((H, E, L, dict(attn_bwd_one_launch=0)))
        if (H, E) in ((512, 128), (200, 256)):
            for L in two:
                out.append((H, E, L, dict(ln_bwd4=0)))
                out.append((H, E, L, dict(ln_bwd4=2)))
    return out


def _case_id(c):
    H, E, L, opts = c
    return f"{H}-{E}-{L}" + "".join(f"-{k}={v}" for k, v in opts.items())


REFUSAL = r"ln_bwd_fused: C=1030 > 1024 unsupported"


def _hip_style(st, x, eps, wts, train, backward=True):
    st.train(train)
    st.zero_grad()
    with helpers.recorded_seeds() as rec:
        outs = st(g(x), 0.9, eps=g(eps))
    if backward:
        sum((o * g(w)).sum() for o, w in zip(outs, wts)).backward()
    torch.cuda.synchronize()
    return ([o.detach().cpu().double() for o in outs], _grads(st) if backward else None,
            rec.of("style_encoder_attn") if train else None, rec)


def _style_compare(H, E, L, opts, train, refused=False):
    B, S = helpers.style_batch(H, E, L), E // 2
    st = helpers.build_style(H, S).to(DEV)
    x, eps, wts = helpers.style_case(B, L, S, seed=400 + L)
    with _options(opts):
        if refused:
            outs, _, seed, _ = _hip_style(st, x, eps, wts, train, backward=False)
            with pytest.raises(RuntimeError, match=REFUSAL):
                _hip_style(st, x, eps, wts, train)
            torch.cuda.synchronize()
            grads = None
        else:
            outs, grads, seed, _ = _hip_style(st, x, eps, wts, train)
    masks = helpers.device_masks_style(seed, B, L, H, E) if train else None
    if train:
        for m, p in zip(masks, onets.STYLE_P):
            assert 0.4 * p < float((m == 0).double().mean()) < 1.6 * p + 0.02
    if grads is None:
        ref_outs, ref_grads = helpers.oracle_style(st, x, eps, wts, masks)
        near = flipped = []
    else:
        ref_outs, ref_grads, near, flipped = helpers.oracle_at_kinks(lambda: helpers.oracle_style(st, x, eps, wts, masks), grads)
    eo = max(helpers.relerr(a, b) for a, b in zip(outs, ref_outs))
    eg = helpers.worst_relerr(grads, ref_grads) if grads is not None else float("nan")
    print(f"\nstyle {H}/{E} B={B} L={L} {opts} {'training' if train else 'eval'} mode: outputs {eo:.2e}, worst gradient {eg:.2e}"
          + (f"; ReLU units at a kink {near}, other side taken for {flipped}" if near else ""))
    assert eo < helpers.STYLE_OUT_BOUND, eo
    if grads is not None:
        errs = {k: helpers.relerr(grads[k], ref_grads[k]) for k in ref_grads}
        assert max(errs.values()) < helpers.STYLE_GRAD_BOUND, {k: f"{v:.1e}" for k, v in errs.items() if v > 1e-5}
    if train:
        noask = helpers.oracle_style(st, x, eps, wts, None)[0]
        assert max(helpers.relerr(a, b) for a, b in zip(outs, noask)) > 100 * helpers.STYLE_OUT_BOUND


@pytest.mark.parametrize("case", _style_cases(), ids=_case_id)
def test_style_encoder_training_mode_vs_masked_oracle(case):
    """z / mu / logvar and every parameter gradient with dropout ON against the float64 oracle given the device's five masks
    (seed + 1 ... + 5; element (b L + l) C + c, attention ((b NH + h) L + q) L + k), over the (H, E) x L x option matrix that
    launches every LayerNorm / attention variant (module docstring)."""
    _style_compare(*case, train=True)


@pytest.mark.parametrize("case", [c for c in _style_cases() if (c[0], c[1]) != (512, 128)], ids=_case_id)
def test_style_encoder_other_widths_eval_mode_vs_oracle(case):
    """the same matrix in eval mode for the widths no other test builds"""
    _style_compare(*case, train=False)


@pytest.mark.parametrize("train", [True, False], ids=["training", "eval"])
def test_style_backward_wider_than_1024_is_refused(train):
    """nhidden = 1030: the forward (unfused chain) is the masked oracle's; the backward is refused with its message, not run"""
    (H, E), (L,) = helpers.STYLE_REFUSED
    _style_compare(H, E, L, {}, train, refused=True)


# ----------------------------------------------------------------------------- d. backward in parts, gathered-input entry
def _abi_style(st, x, dout, seed, parts):
    """zeggs_style_encoder_fwd_part + the backward through the raw ABI with dropout on: `parts` = (3,) one call, (1, 2) chain then
    the weight-gradient products -> (out [B, E], {field: gradient})"""
    enc = st.encoder
    params = [p.detach().contiguous() for p in ops.style_param_list(enc)]
    B, L, Cx = x.shape
    H, E = params[0].shape[0], params[4].shape[0]
    d = ops.StyleDims(B, L, Cx, H, E, 4, 1, int(seed))
    Lb = ops.lib()
    ws = ops._ws(int(Lb.zeggs_style_encoder_workspace_bytes(C.byref(d))), x.device)
    pos = ops.positional_table(L, E, x.device)
    out = torch.empty(B, E, device=x.device)
    P = ops._ptrs(ops.StylePtrs, ops.STYLE_FIELDS, params)
    ops._check(Lb.zeggs_style_encoder_fwd_part(C.byref(d), C.byref(P), ops._p(x), ops._p(pos), ops._p(out), ops._p(ws),
                                               C.c_size_t(ws.numel()), ops._stream(), 3), "fwd")
    grads = [torch.zeros_like(p) for p in params]
    G = ops._ptrs(ops.StylePtrs, ops.STYLE_FIELDS, grads)
    for part in parts:
        ops._check(Lb.zeggs_style_encoder_bwd_part(C.byref(d), C.byref(P), ops._p(dout), C.byref(G), ops._p(ws),
                                                   C.c_size_t(ws.numel()), ops._stream(), 1, part), f"bwd part {part}")
    torch.cuda.synchronize()
    return out.cpu().double(), dict(zip(ops.STYLE_FIELDS, (t.cpu().double() for t in grads)))


@pytest.mark.parametrize("B,L", [(2, 33), (3, 128)])
def test_style_backward_chain_plus_products_with_masks_on(B, L):
    """zeggs_style_encoder_bwd_part in training mode: the chain (part 1) followed by the six weight-gradient products (part 2)
    gives the gradients of the one-call backward (part 3) -- both held to the float64 oracle with the device's masks at the
    encoder bounds, and to each other at 1e-5 of the tensor's largest entry (the same arithmetic; only the order of the float
    atomics of the split products and column sums differs: some hundred ulp of 6e-8)."""
    _, _, st = helpers.build_nets()
    st = st.to(DEV)
    gen = torch.Generator().manual_seed(500 + L)
    x, dout = torch.randn(B, L, synth.POSE_IN, generator=gen), torch.randn(B, 128, generator=gen)
    seed = 123456789 + L
    out3, g3 = _abi_style(st, g(x), g(dout), seed, (3,))
    out12, g12 = _abi_style(st, g(x), g(dout), seed, (1, 2))
    masks = helpers.device_masks_style(seed, B, L, 512, 128)
    order = _field_order(st)

    def oracle():
        w = helpers.f64_weights(st)
        ref = onets.style_encoder_attn(w, x.double(), masks=masks)
        (ref * dout.double()).sum().backward()
        return ref.detach(), dict(zip(ops.STYLE_FIELDS, [w[n].grad for n in order]))
    for tag, out, gr in (("one call", out3, g3), ("chain + products", out12, g12)):
        ref, by_field, _, _ = helpers.oracle_at_kinks(oracle, gr)
        assert helpers.relerr(out, ref) < helpers.STYLE_OUT_BOUND, tag
        for k in ops.STYLE_FIELDS:
            assert helpers.relerr(gr[k], by_field[k]) < helpers.STYLE_GRAD_BOUND, (tag, k)
    worst = max(helpers.relerr(g12[k], g3[k]) for k in ops.STYLE_FIELDS)
    print(f"\nB={B} L={L}: chain + products vs one call: worst gradient difference {worst:.2e}")
    assert worst < 1e-5, worst


def _field_order(st):
    """the module's parameter names in the C-ABI order of ops.style_param_list"""
    by_ptr = {p.data_ptr(): n for n, p in st.named_parameters()}
    return [by_ptr[p.data_ptr()] for p in ops.style_param_list(st.encoder)]


def test_gathered_input_entry_in_training_mode_equals_the_copied_input_entry():
    """part & 4 (ops.style_input_buffer + gather_example: the example gathered straight into the workspace's padded input) with
    dropout ON at the same seed: z / mu / logvar equal the copied-input entry's bit for bit, the gradients to the float atomics'
    order (1e-5, see above); and both are the masked oracle's."""
    _, _, st = helpers.build_nets()
    st = st.to(DEV).train()
    B, L, W = 2, 16, synth.POSE_OUT
    gen = torch.Generator().manual_seed(77)
    frames = torch.randn(300, W, generator=gen)
    rows = torch.randint(0, 300, (B, L), generator=gen)
    mean, std = torch.randn(W + 3, generator=gen), torch.rand(W + 3, generator=gen) + 0.5
    eps = torch.randn(B, 64, generator=gen)
    wts = [torch.randn(B, 64, generator=gen) for _ in range(3)]
    ws, xp = ops.style_input_buffer(st.encoder, B, L, W + 3, True, DEV)
    ops.gather_example(g(frames), g(rows), g(mean), g(std), xp)

    def run(inp):
        st.zero_grad()
        ops.manual_seed(4242)
        with helpers.recorded_seeds() as rec:
            outs = st(inp, 1.0, eps=g(eps))
        sum((o * g(w)).sum() for o, w in zip(outs, wts)).backward()
        torch.cuda.synchronize()
        return [o.detach().clone() for o in outs], _grads(st), rec.of("style_encoder_attn")

    n0 = ops.COUNTERS.get("style_in_place", 0)
    x_copy = xp[:, 1:-1].clone()
    o_in, g_in, s_in = run(ops.example_view(ws, xp))
    assert ops.COUNTERS.get("style_in_place", 0) == n0 + 1
    o_cp, g_cp, s_cp = run(x_copy)
    assert ops.COUNTERS.get("style_in_place", 0) == n0 + 1 and s_in == s_cp
    for a, b in zip(o_in, o_cp):
        assert torch.equal(a, b)
    worst = max(helpers.relerr(g_in[k], g_cp[k]) for k in g_cp)
    print(f"\ngathered-input vs copied-input entry, training mode: outputs bit-equal, worst gradient difference {worst:.2e}")
    assert worst < 1e-5, worst
    masks = helpers.device_masks_style(s_in, B, L, 512, 128)
    ref_outs, ref_grads, _, _ = helpers.oracle_at_kinks(
        lambda: helpers.oracle_style(st, x_copy.cpu(), eps, wts, masks, temperature=1.0), g_in)
    assert max(helpers.relerr(a, b) for a, b in zip(o_in, ref_outs)) < helpers.STYLE_OUT_BOUND
    for k in ref_grads:
        assert helpers.relerr(g_in[k], ref_grads[k]) < helpers.STYLE_GRAD_BOUND, k


# ----------------------------------------------------------------------------- e. one engine step
def _engine_step(case, defer=False, iteration=0):
    se, de, st = [m.to(DEV).train() for m in helpers.build_nets()]
    data = helpers.engine_case_data(case)
    ds = engine.DeviceDataset(data, case["window"], torch.device(DEV))
    eng = engine.TrainEngine(se, de, st, ds, synth.PARENTS, synth.DT, lr=1e-4, eps=1e-5, noise_seed=case["noise_seed"],
                             defer_style_wgrads=defer)
    eng.iteration = iteration
    idx = helpers.engine_case_idx(case, len(ds))
    w_before = [p.detach().cpu().clone() for p in eng.params]
    with helpers.recorded_seeds() as rec:
        loss = eng.step(idx, case["L"])
    torch.cuda.synchronize()
    eng.flush()
    return eng, data, idx, w_before, loss, rec


@pytest.mark.parametrize("defer", [False, True], ids=["", "defer_style_wgrads"])
@pytest.mark.parametrize("case,iteration", [(helpers.ENGINE_CASES[0], 0), (helpers.ENGINE_CASES[1], 7500)],
                         ids=["B2-L16-it0", "B5-L33-it7500"])
def test_engine_step_training_mode_vs_masked_oracle(case, iteration, defer):
    """One TrainEngine.step with both encoders in .train() and the VAE noise drawn inside the step: the seeds the step drew are
    recorded, the seven masks and eps rebuilt from them, and the float64 oracle iteration evaluated with them -- loss, the 18
    terms, the gradient of all 44 tensors (in full), the weights after the step's fused RAdam against oracle/radam.py applied
    to the oracle's gradients.  Iteration 7500: the KL weight is at its cap 0.2 there (1e-16 at iteration 0), so the noise meets the KL term.
    Bounds of test_gpu_parity.py::test_train_iteration_vs_reference, iteration 0."""
    if defer and iteration == 0:
        case = dict(case, noise_seed=case["noise_seed"] + 100)
    B, T, L = case["B"], case["window"], case["L"]
    eng, data, idx, w_before, loss, rec = _engine_step(case, defer, iteration)
    assert eng.defer_style_wgrads == defer
    assert sorted(c for c, _ in rec.draws) == ["randn", "speech_encoder", "style_encoder_attn"], rec.draws
    masks = helpers.device_masks_speech(rec.of("speech_encoder"), B, T, 64, 64) + \
        helpers.device_masks_style(rec.of("style_encoder_attn"), B, L, 512, 128)
    eps = helpers.device_eps(rec.of("randn"), B, 64).double()
    assert abs(float(eps.mean())) < 0.5 and 0.5 < float(eps.std()) < 1.5
    audio_n, target, gaze, example_n, _ = helpers.host_batch(data, T, idx, L)
    mods = (eng.se, eng.de, eng.st)

    def oracle():
        ws = [{k: v.double().clone().requires_grad_(True) for k, v in zip(m.state_dict().keys(), wb)}
              for m, wb in zip(mods, _split(w_before, mods))]
        lo, te, ws = helpers.oracle_iteration_core(ws, audio_n, target, gaze, example_n, eps, iteration, masks=masks)
        return (lo.detach(), te.detach()), {i: v.grad for i, v in enumerate(v for w in ws for v in w.values())}
    got_all = {i: p.grad.detach().cpu().double() for i, p in enumerate(eng.params)}
    (ref_loss, ref_terms), refs, _, _ = helpers.oracle_at_kinks(oracle, got_all)
    np.testing.assert_allclose(float(loss.detach()), float(ref_loss), rtol=1e-5)
    np.testing.assert_allclose(eng.last_terms[:18].cpu().numpy(), ref_terms.numpy(), rtol=1e-4, atol=1e-6)
    assert len(refs) == len(eng.params) == 44
    worst = 0.0
    for i, (p, wb) in enumerate(zip(eng.params, w_before)):
        got, ref = got_all[i], refs[i]
        scale = max(1e-6, float(ref.abs().max()))
        e = float((got - ref).abs().max())
        worst = max(worst, e / scale)
        assert e < helpers.ENGINE_GRAD_BOUND * scale + 1e-8, f"param {i}: {e / scale:.2e} of the tensor's largest entry"
        pn, gn = wb.numpy().astype(np.float64).ravel().copy(), ref.numpy().ravel().copy()
        m, v = np.zeros_like(pn), np.zeros_like(pn)
        oradam.radam_step(pn, gn, m, v, 1, 1e-4, 1e-5)
        np.testing.assert_allclose(p.detach().cpu().numpy().ravel(), pn, atol=3e-7, err_msg=f"param {i} after RAdam")
    print(f"\nengine step B={B} L={L} iteration {iteration} defer={defer}: loss {float(loss):.6f} (oracle {float(ref_loss):.6f}), "
          f"worst gradient {worst:.2e} of the tensor's largest entry")


def _split(flat_list, mods):
    out, off = [], 0
    for m in mods:
        n = len(list(m.parameters()))
        assert n == len(m.state_dict())
        out.append(flat_list[off:off + n])
        off += n
    return out


def test_engine_step_replays_its_masks_from_the_noise_seed():
    """the same noise_seed -> the same three seeds (hence the same masks and noise) and a bit-equal loss; another noise_seed ->
    other seeds"""
    case = helpers.ENGINE_CASES[0]
    _, _, _, _, loss_a, rec_a = _engine_step(case)
    _, _, _, _, loss_b, rec_b = _engine_step(case)
    assert rec_a.draws == rec_b.draws and len(rec_a.draws) == 3
    assert torch.equal(loss_a, loss_b)
    _, _, _, _, _, rec_c = _engine_step(dict(case, noise_seed=case["noise_seed"] + 1))
    assert {s for _, s in rec_c.draws}.isdisjoint({s for _, s in rec_a.draws})
