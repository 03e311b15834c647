"""GPU parity tests: the HIP engine (through the C ABI) vs the CPU oracle and the
golden vectors produced by the reference.  Tolerances: forward outputs 1e-4 absolute
(north_star), gradients 2e-4 of the tensor's max |grad| (fp32 vs fp64 oracle)."""
import numpy as np
import pytest
import torch

import helpers
from oracle import anim as oanim
from oracle import loss as oloss
from oracle import nets as onets
from oracle import radam as oradam
from zeggs import ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def g(t):
    return t.to(DEV)


def relerr(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / max(1e-12, float(ref.abs().max())))


# ----------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(32, 3072, 2286), (2, 1131, 1024), (200, 70, 33), (513, 129, 1262), (64, 64, 16),
                                   (1, 5, 3)])
def test_gemm_layouts(M, N, K):
    torch.manual_seed(0)
    A, B = torch.randn(M, K), torch.randn(K, N)
    bias = torch.randn(N)
    ref = A.double() @ B.double()
    # NN
    C = torch.zeros(M, N, device=DEV)
    ops.gemm(g(A), g(B), C, M, N, K, (K, 1), (N, 1), (N, 1))
    assert relerr(C, ref) < 2e-6
    # NT (+bias, ELU)
    Bt = B.t().contiguous()
    ops.gemm(g(A), g(Bt), C, M, N, K, (K, 1), (1, K), (N, 1), bias=g(bias), act=1)
    assert relerr(C, torch.nn.functional.elu(ref + bias.double())) < 2e-6
    # TN with beta
    At = A.t().contiguous()
    C0 = torch.randn(M, N)
    C = g(C0.clone())
    ops.gemm(g(At), g(B), C, M, N, K, (1, M), (N, 1), (N, 1), beta=0.5, alpha=2.0)
    assert relerr(C, 2.0 * ref + 0.5 * C0.double()) < 2e-6


@pytest.mark.parametrize("Mc,N,K,lddy,ldx", [(8160, 1024, 1262, 1024, 2286), (8160, 3072, 1024, 3072, 1024),
                                             (8160, 1131, 1024, 1136, 1024), (2040, 2048, 1024, 3072, 1024), (70, 96, 80, 96, 80)])
def test_weight_gradient_with_bias_sums_in_one_launch(Mc, N, K, lddy, ldx):
    """zeggs_gemm_tn_bias (round 5): dW += dy^T x and db += column sums of dy -- where the barrier-free kernel takes the product, the
    sums come out of its own operand fragments (GemmArgs.asum: added inside the inline-asm wait statement; a compiler-level add on
    the asm loads' destination registers made the allocator copy them before the data had arrived, caught at K = 8160), else by a
    separate launch (the last shape).  The decoder's four weight-gradient shapes, both kernel variants, sums in the product / apart;
    accumulation onto existing values; against float64."""
    import ctypes as C
    torch.manual_seed(Mc + N)
    dy, x = torch.randn(Mc, lddy), torch.randn(Mc, ldx)
    W0, b0 = torch.randn(N, K), torch.randn(N)
    ref_w = W0.double() + dy[:, :N].double().T @ x[:, :K].double()
    ref_b = b0.double() + dy[:, :N].double().sum(0)
    L = ops.lib()
    dyd, xd = g(dy), g(x)
    try:
        for shield, asum in ((0, 0), (0, 1), (1, 0), (1, 1)):
            ops.set_option("gemm_direct_shield", shield)
            ops.set_option("gemm_direct_depth", 8 if shield else 4)
            ops.set_option("gemm_asum", asum)
            dW, db = g(W0.clone()), g(b0.clone())
            rc = L.zeggs_gemm_tn_bias(ops._p(dyd), C.c_long(lddy), ops._p(xd), C.c_long(ldx), ops._p(dW), C.c_long(K), Mc, N, K,
                                      C.c_float(1.0), ops._p(db), ops._stream())
            assert rc == 0, L.zeggs_last_error()
            ew = float((dW.cpu().double() - ref_w).abs().max() / ref_w.abs().max())
            eb = float((db.cpu().double() - ref_b).abs().max() / ref_b.abs().max())
            assert ew < 4e-6 and eb < 4e-6, (shield, asum, ew, eb)
    finally:
        ops.set_option("gemm_direct_shield", 0)
        ops.set_option("gemm_direct_depth", 4)
        ops.set_option("gemm_asum", 1)
        for k in ("gemm_direct_shield", "gemm_direct_depth", "gemm_asum"):
            ops._OPTIONS.pop(k, None)


@pytest.mark.parametrize("M,N,K,lda,ldb,kbatch", [(3072, 1024, 2040, 3072, 1024, 1), (1131, 1262, 1022, 1132, 2288, 1),
                                                  (197, 333, 1026, 200, 340, 1), (384, 128, 192, 384, 128, 7),
                                                  (3402, 512, 208, 1134, 512, 5), (130, 70, 2048, 131, 73, 1)])
def test_gemm_direct_stream_k_vs_float64_and_the_lds_kernel(M, N, K, lda, ldb, kbatch):
    """Round 5: the barrier-free / LDS-free stream-K TN product (gemm.hip: gemm_tn_direct_kernel -- operands straight from memory
    into the matrix-core operand registers, inline-asm loads with hand-counted vmcnt) on weight-gradient shapes: aligned and odd
    extents / strides, the batch-reduce form of the convolution weight gradients (kbatch > 1, overlapping A rows as conv_dw_gemm
    passes them), both wave tiles, three prefetch depths, accumulation onto an existing C -- every output entry against float64,
    and against the LDS-tiled stream-K kernel it replaces."""
    torch.manual_seed(M + N + K)
    overlap = kbatch > 1 and lda < M                       # conv weight gradient: A(m, k) = xp[k * lda + m], m < taps * lda
    rowsA = K + (M + lda - 1) // lda if overlap else K
    A = torch.randn(kbatch, rowsA, lda)
    B = torch.randn(kbatch, K, ldb)
    C0 = torch.randn(M, N)
    if overlap:
        Am = torch.stack([A[b].flatten()[(torch.arange(K)[:, None] * lda + torch.arange(M)[None, :])] for b in range(kbatch)])
    else:
        Am = A[:, :, :M]
    ref = torch.einsum("bkm,bkn->mn", Am.double(), B[:, :, :N].double())
    L = ops.lib()
    import ctypes as C

    def run(beta):
        Cd = g(C0.clone())
        Ad, Bd = g(A), g(B)
        if kbatch == 1:
            ops.gemm(Ad, Bd, Cd, M, N, K, (1, lda), (ldb, 1), (N, 1), beta=beta)
        else:       # the batch-reduce form has no Python wrapper: through the style encoder's own call shape (zeggs_gemm_kbatch)
            rc = L.zeggs_gemm_kbatch(ops._p(Ad), ops._p(Bd), ops._p(Cd), M, N, K, C.c_long(1), C.c_long(lda), C.c_long(ldb), C.c_long(1),
                                     C.c_long(N), C.c_long(1), kbatch, C.c_long(rowsA * lda), C.c_long(K * ldb), C.c_float(beta),
                                     ops._stream())
            assert rc == 0, L.zeggs_last_error()
        return Cd.cpu().double()

    outs = {}
    try:
        # (mode, workgroups per CU, pairs in flight, shield: the variant that allocates its SIMDs' whole register files -- what
        #  zeggs.engine.TrainEngine runs in its three-queue schedule)
        for mode, wgs, depth, shield in ((0, 0, 4, 0), (2, 1, 4, 0), (2, 2, 8, 0), (3, 2, 4, 0), (3, 3, 6, 0), (1, 0, 8, 0),
                                         (1, 0, 8, 1), (2, 0, 4, 1), (3, 0, 6, 1), (1, 0, 8, 2)):
            ops.set_option("gemm_direct", mode)
            ops.set_option("gemm_direct_wgs", wgs)
            ops.set_option("gemm_direct_depth", depth)
            ops.set_option("gemm_direct_shield", shield)
            for beta in (0.0, 1.0):
                got = run(beta)
                want = ref + beta * C0.double()
                err = float((got - want).abs().max() / want.abs().max())
                assert err < 3e-6, (mode, wgs, depth, shield, beta, err)
                outs[(mode, wgs, depth, beta, shield)] = got
    finally:
        ops.set_option("gemm_direct", 1)
        ops.set_option("gemm_direct_wgs", 0)
        ops.set_option("gemm_direct_depth", 4)
        ops.set_option("gemm_direct_shield", 0)
        for k in ("gemm_direct", "gemm_direct_wgs", "gemm_direct_depth", "gemm_direct_shield"):
            ops._OPTIONS.pop(k, None)          # back to "not chosen by the caller": a TrainEngine built later picks its own
    base = outs[(0, 0, 4, 0.0, 0)]
    for k, v in outs.items():
        if k[3] == 0.0:
            assert float((v - base).abs().max() / base.abs().max()) < 3e-6, k


@pytest.mark.parametrize("M,N,K", [(32, 1024, 1198), (32, 3072, 1131), (64, 1024, 1024), (33, 1000, 67), (17, 70, 64),
                                   (1, 2262, 1262), (48, 64, 4097)])
def test_gemm_skinny_nt_one_launch(M, N, K):
    """batch-sized y = act(x W^T + b) (skinny_nt_k: one launch instead of zero fill + split-K atomics + bias pass), with row
    strides / bases that are not 16-byte aligned (W_ih0[:, H:] of the decoder, the CellStateEncoder's 1198-wide input)"""
    torch.manual_seed(M + N + K)
    ldx, ldw, ldy = K + 3, K + 1022, N + 5
    xb, wb = torch.randn(M, ldx), torch.randn(N, ldw)
    bias = torch.randn(N)
    X, Wm = g(xb), g(wb)
    x, w = X[:, 1:1 + K], Wm[:, 1021:1021 + K]                       # odd element offsets

    class Raw:      # a strided view handed over as its first element's address (ops.gemm takes the strides separately)
        def __init__(self, t):
            self.t, self.is_cuda, self.dtype = t, True, t.dtype
        def is_contiguous(self):
            return True
        def data_ptr(self):
            return self.t.data_ptr()
    ref = x.double().cpu() @ w.double().cpu().t() + bias.double()
    for act, fn in ((0, lambda t: t), (1, torch.nn.functional.elu)):
        Y = torch.full((M, ldy), 7.0, device=DEV)
        ops.gemm(Raw(x), Raw(w), Y, M, N, K, (ldx, 1), (1, ldw), (ldy, 1), bias=g(bias), act=act)
        assert relerr(Y[:, :N], fn(ref)) < 2e-6
        assert bool((Y[:, N:] == 7.0).all())                          # nothing written past the N columns
        ops.set_option("gemm_skinny", 0)                              # the split-K recipe gives the same
        Y0 = torch.zeros(M, ldy, device=DEV)
        ops.gemm(Raw(x), Raw(w), Y0, M, N, K, (ldx, 1), (1, ldw), (ldy, 1), bias=g(bias), act=act)
        ops.set_option("gemm_skinny", 1)
        assert relerr(Y[:, :N], Y0[:, :N]) < 2e-6
    # NN (input gradients dx = dy W: W[k][n], four 4-byte loads down a column), accumulating onto an existing result
    wt = g(wb[:, 1021:1021 + K].t().contiguous())                     # [K, N]
    Y = torch.full((M, ldy), 0.5, device=DEV)
    ops.gemm(Raw(x), wt, Y, M, N, K, (ldx, 1), (N, 1), (ldy, 1), beta=1.0)
    assert relerr(Y[:, :N], ref - bias.double() + 0.5) < 2e-6 and bool((Y[:, N:] == 0.5).all())


def test_gemm_batched_and_overlapping_rows():
    torch.manual_seed(1)
    nb, T, Cc, Co, kw = 3, 37, 10, 7, 5
    xp = torch.randn(nb, T + kw - 1, Cc)
    Wf = torch.randn(kw * Cc, Co)
    out = torch.zeros(nb, T, Co, device=DEV)
    # conv as GEMM: rows overlap (sam = C), K = kw*C
    ops.gemm(g(xp), g(Wf), out, T, Co, kw * Cc, (Cc, 1), (Co, 1), (Co, 1), nbatch=nb,
             bs=((T + kw - 1) * Cc, 0, T * Co))
    w = Wf.reshape(kw, Cc, Co).permute(2, 1, 0).contiguous()            # [Co, C, kw]
    ref = torch.nn.functional.conv1d(xp.transpose(1, 2).double(), w.double()).transpose(1, 2)
    assert relerr(out, ref) < 2e-6


# ----------------------------------------------------------------------------- encoders
def _golden_nets(golden_dir):
    gd = np.load(golden_dir / "nets.npz")
    return gd, helpers.build_nets(), helpers.stats_tensors()


def test_speech_encoder_forward_backward(golden_dir):
    gd, (se, _, _), s = _golden_nets(golden_dir)
    x = (torch.as_tensor(gd["in_X_audio_features"]) - s["a_mean"]) / s["a_std"]
    se_g = se.to(DEV).eval()
    out = se_g(g(x))
    assert float((out.cpu() - torch.as_tensor(gd["speech"])).abs().max()) < 1e-4       # vs the reference
    # gradients vs fp64 oracle autograd, longer sequence (exercises the replicate edges)
    torch.manual_seed(5)
    x = torch.randn(3, 70, synth.N_AUDIO)
    wgt = torch.randn(3, 70, 64)
    w64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in se_g.state_dict().items()}
    (onets.speech_encoder(w64, x.double()) * wgt.double()).sum().backward()
    se_g.zero_grad()
    out = se_g(g(x))
    assert relerr(out, onets.speech_encoder({k: v.detach() for k, v in w64.items()}, x.double())) < 1e-5
    (out * g(wgt)).sum().backward()
    for k, p in se_g.named_parameters():
        assert relerr(p.grad, w64[k].grad) < 2e-4, k


def test_speech_encoder_dropout_training_mode():
    se, _, _ = helpers.build_nets()
    se = se.to(DEV).train()
    x = torch.randn(2, 40, synth.N_AUDIO, device=DEV)
    a = se(x)
    b = se(x)
    assert torch.isfinite(a).all() and not torch.allclose(a, b)      # masks differ call to call
    a.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in se.parameters())


def test_style_encoder_forward_backward(golden_dir):
    gd, (_, _, st), s = _golden_nets(golden_dir)
    ex = (torch.as_tensor(gd["in_example"]) - s["in_mean"]) / s["in_std"]
    st_g = st.to(DEV).eval()
    z, mu, logvar = st_g(g(ex), float(gd["temperature"]), eps=g(torch.as_tensor(gd["in_eps"])))
    for got, key in ((z, "style_z"), (mu, "style_mu"), (logvar, "style_logvar")):
        assert float((got.cpu() - torch.as_tensor(gd[key])).abs().max()) < 1e-4, key     # vs the reference
    # gradients vs fp64 oracle
    torch.manual_seed(6)
    B, L = 3, 21
    x = torch.randn(B, L, synth.POSE_IN)
    eps = torch.randn(B, 64)
    wz, wm, wl = torch.randn(B, 64), torch.randn(B, 64), torch.randn(B, 64)
    w64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in st_g.state_dict().items()}
    z, mu, lv = onets.style_encoder(w64, x.double(), eps.double(), 0.9)
    (z * wz.double() + mu * wm.double() + lv * wl.double()).sum().backward()
    st_g.zero_grad()
    zg, mug, lvg = st_g(g(x), 0.9, eps=g(eps))
    assert relerr(zg, z) < 2e-5 and relerr(mug, mu) < 2e-5 and relerr(lvg, lv) < 2e-5
    (zg * g(wz) + mug * g(wm) + lvg * g(wl)).sum().backward()
    for k, p in st_g.named_parameters():
        assert relerr(p.grad, w64[k].grad) < 3e-4, k


def test_style_encoder_dropout_training_mode():
    _, _, st = helpers.build_nets()
    st = st.to(DEV).train()
    x = torch.randn(2, 16, synth.POSE_IN, device=DEV)
    z, mu, lv = st(x)
    (z.sum() + mu.sum() + lv.sum()).backward()
    assert all(torch.isfinite(p.grad).all() for p in st.parameters())


# ----------------------------------------------------------------------------- decoder
def _first_pose(gd, idx=0):
    t = lambda k: torch.as_tensor(gd[k])  # noqa: E731
    return [t("in_Y_root_pos")[:, idx], t("in_Y_root_rot")[:, idx], t("in_Y_root_vel")[:, idx],
            t("in_Y_root_vrt")[:, idx], t("in_Y_lpos")[:, idx], t("in_Y_ltxy")[:, idx], t("in_Y_lvel")[:, idx],
            t("in_Y_lvrt")[:, idx]]


NAMES = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "ltxy", "lvel", "lvrt")


def test_decoder_forward_vs_reference(golden_dir):
    gd, (_, de, _), s = _golden_nets(golden_dir)
    de_g = de.to(DEV).eval()
    T = gd["speech"].shape[1]
    style = torch.as_tensor(gd["style_z"]).unsqueeze(1).repeat(1, T, 1)
    with torch.no_grad():
        out = de_g(*[g(t) for t in _first_pose(gd)], g(torch.as_tensor(gd["in_Y_gaze_pos"])),
                   g(torch.as_tensor(gd["speech"])), g(style), None, g(s["in_mean"]), g(s["in_std"]), g(s["out_mean"]),
                   g(s["out_std"]), synth.DT)
    for n, o in zip(NAMES, out):
        err = float((o.cpu() - torch.as_tensor(gd["O_" + n])).abs().max())
        assert err < 1e-4, f"{n}: {err}"


def test_decoder_backward_vs_oracle(golden_dir):
    gd, (_, de, _), s = _golden_nets(golden_dir)
    de_g = de.to(DEV).train()
    torch.manual_seed(7)
    B, T = 2, 6
    speech = torch.randn(B, T, 64) * 0.5
    style = torch.randn(B, T, 64) * 0.5
    gaze = torch.as_tensor(gd["in_Y_gaze_pos"])
    fp = _first_pose(gd)
    wts = [torch.randn(B, T, *o.shape[1:]) for o in fp]
    s64 = {k: v.double() for k, v in s.items()}
    w64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in de_g.state_dict().items()}
    sp64, sy64 = speech.double().requires_grad_(True), style.double().requires_grad_(True)
    O = onets.decoder_rollout(w64, *[t.double() for t in fp], gaze.double(), sp64, sy64, s64["in_mean"], s64["in_std"],
                              s64["out_mean"], s64["out_std"], synth.DT)
    sum((o * w.double()).sum() for o, w in zip(O, wts)).backward()
    de_g.zero_grad()
    spg, syg = g(speech).requires_grad_(True), g(style).requires_grad_(True)
    out = de_g(*[g(t) for t in fp], g(gaze), spg, syg, None, g(s["in_mean"]), g(s["in_std"]), g(s["out_mean"]),
               g(s["out_std"]), synth.DT)
    for n, o, r in zip(NAMES, out, O):
        assert float((o.detach().cpu().double() - r.detach()).abs().max()) < 1e-4, n
    sum((o * g(w)).sum() for o, w in zip(out, wts)).backward()
    assert relerr(spg.grad, sp64.grad) < 3e-4
    assert relerr(syg.grad, sy64.grad) < 3e-4
    for k, p in de_g.named_parameters():
        assert relerr(p.grad, w64[k].grad) < 3e-4, k


@pytest.mark.parametrize("H", [512, 768])
def test_decoder_other_hidden_width_vs_oracle(golden_dir, H):
    """`decoder.nhidden` other than the shipped 1024 (ZEGGS/train.py:129 honours the option): the persistent kernels are
    built for H = 1024 and decline, the fragment-packed stage kernels serve any H % 16 == 0 -- forward 1e-4 and every gradient
    3e-4 against the oracle in float64 at H = 512 / 768, and the stage path really was the one that ran (bench.py times the
    same width: `nhidden_512_b32`)."""
    from zeggs import modules
    gd, _, s = _golden_nets(golden_dir)
    torch.manual_seed(77)
    de_g = modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, 64, H, 2).to(DEV).train()
    B, T = 2, 9
    speech, style = torch.randn(B, T, 64) * 0.5, torch.randn(B, T, 64) * 0.5
    gaze = torch.as_tensor(gd["in_Y_gaze_pos"])[:, :1].repeat(1, T, 1)
    fp = _first_pose(gd)
    wts = [torch.randn(B, T, *o.shape[1:]) for o in fp]
    s64 = {k: v.double() for k, v in s.items()}
    w64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in de_g.state_dict().items()}
    sp64, sy64 = speech.double().requires_grad_(True), style.double().requires_grad_(True)
    O = onets.decoder_rollout(w64, *[t.double() for t in fp], gaze.double(), sp64, sy64, s64["in_mean"], s64["in_std"],
                              s64["out_mean"], s64["out_std"], synth.DT)
    sum((o * w.double()).sum() for o, w in zip(O, wts)).backward()
    spg, syg = g(speech).requires_grad_(True), g(style).requires_grad_(True)
    before = [ops.lib().zeggs_persistent_state(k) for k in (1, 2)]
    out = de_g(*[g(t) for t in fp], g(gaze), spg, syg, None, g(s["in_mean"]), g(s["in_std"]), g(s["out_mean"]),
               g(s["out_std"]), synth.DT)
    for n, o, r in zip(NAMES, out, O):
        assert float((o.detach().cpu().double() - r.detach()).abs().max()) < 1e-4, n
    sum((o * g(w)).sum() for o, w in zip(out, wts)).backward()
    assert [ops.lib().zeggs_persistent_state(k) for k in (1, 2)] == before       # not the H = 1024 persistent kernels
    assert relerr(spg.grad, sp64.grad) < 3e-4 and relerr(syg.grad, sy64.grad) < 3e-4
    for k, p in de_g.named_parameters():
        assert relerr(p.grad, w64[k].grad) < 3e-4, k
    # ... and the fragment-packed stage path agrees with the generic per-step GEMM path at this width
    try:
        ops.set_option("decoder_fast", 0)
        with torch.no_grad():
            ref = de_g(*[g(t) for t in fp], g(gaze), g(speech), g(style), None, g(s["in_mean"]), g(s["in_std"]),
                       g(s["out_mean"]), g(s["out_std"]), synth.DT)
    finally:
        ops.set_option("decoder_fast", 1)
    for n, o, r in zip(NAMES, out, ref):
        assert float((o.detach() - r).abs().max()) < 1e-4, n


def test_decoder_width512_vs_reference(golden_dir):
    """decoder.nhidden = 512 on the fragment-packed stage kernels against the REFERENCE at that width (width512.npz, B = 18,
    T = 8: outputs, input gradients in full, 512 samples of every parameter gradient of the reference's autograd)"""
    from zeggs import modules
    gd = np.load(golden_dir / "width512.npz")
    torch.manual_seed(5512)
    de = modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, 64, 512, 2)
    for k, v in de.state_dict().items():
        np.testing.assert_allclose(helpers.fingerprint(v), gd[f"fp_decoder.{k}"], rtol=1e-12, atol=0, err_msg=k)
    first, gaze, wts = helpers.width512_inputs(gd)
    s = helpers.stats_tensors()
    de_g = de.to(DEV).train()
    stat = [g(s[k]) for k in ("in_mean", "in_std", "out_mean", "out_std")]
    t = lambda k: torch.as_tensor(gd[k])  # noqa: E731
    spg, syg = g(t("in_speech")).requires_grad_(True), g(t("in_style")).requires_grad_(True)
    out = de_g(*[g(x) for x in first], g(gaze), spg, syg, None, *stat, synth.DT)
    for n, o in zip(NAMES, out):
        assert float((o.detach().cpu() - t("O_" + n)).abs().max()) < 1e-4, n
    sum((o * g(w)).sum() for o, w in zip(out, wts)).backward()
    assert relerr(spg.grad, t("d_speech")) < 3e-4 and relerr(syg.grad, t("d_style")) < 3e-4
    helpers.assert_grad_samples(gd, "decoder", [(k, p.grad) for k, p in de_g.named_parameters()], 3e-4)
    with torch.no_grad():
        out = de_g(*[g(x) for x in first], g(gaze), g(t("in_speech")), g(t("in_style")), None, *stat, synth.DT)
    for n, o in zip(NAMES, out):
        assert float((o.cpu() - t("O_" + n)).abs().max()) < 1e-4, n


# ----------------------------------------------------------------------------- loss
def _pack_pose(vel, vrt, lpos, ltxy, lvel, lvrt):
    B, T = vel.shape[:2]
    return torch.cat([vel, vrt, lpos.reshape(B, T, -1), ltxy.reshape(B, T, -1), lvel.reshape(B, T, -1),
                      lvrt.reshape(B, T, -1)], dim=-1)


@pytest.mark.parametrize("loss_lds", [1, 0])
def test_loss_forward_backward_vs_oracle(loss_lds):
    """loss_lds = 0: the frame kernels without their LDS message buffers (the level hand-off through the global tables: what a part
    that refuses 147 KB of dynamic LDS gets, and what skeletons with a level wider than 16 joints get anyway)."""
    ops.set_option("loss_lds", loss_lds)
    try:
        _loss_forward_backward_vs_oracle()
    finally:
        ops.set_option("loss_lds", 1)


def _loss_forward_backward_vs_oracle():
    stats = synth.make_stats()
    B, T = 3, 7
    rng = np.random.default_rng(4)
    Wc = [synth.make_clip(T, seed=90 + b, stats=stats) for b in range(B)]
    Oc = [synth.make_clip(T, seed=190 + b, stats=stats) for b in range(B)]
    tt = lambda cl, k: torch.as_tensor(np.stack([c[k] for c in cl]))  # noqa: E731
    keys = ("Y_root_pos", "Y_root_rot", "Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt")
    W = [tt(Wc, k) for k in keys]
    O = [tt(Oc, k) for k in keys]
    # make the prediction a perturbation of the ground truth (and a non-unit root quaternion, as the decoder produces)
    O = [w + 0.3 * (o - w) for o, w in zip(O, W)]
    gaze = tt(Wc, "Y_gaze_pos")
    mu, lv = torch.as_tensor(rng.standard_normal((B, 64)), dtype=torch.float32), \
        torch.as_tensor(0.3 * rng.standard_normal((B, 64)), dtype=torch.float32)
    it = 9000
    O64 = [o.double().requires_grad_(True) for o in O]
    mu64, lv64 = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
    loss64, terms64 = oloss.training_loss(O64, [w.double() for w in W], gaze.double(), synth.PARENTS, synth.DT, mu64,
                                          lv64, iteration=it)
    loss64.backward()
    op = g(_pack_pose(*O[2:])).requires_grad_(True)
    orp, orr = g(O[0]).requires_grad_(True), g(O[1]).requires_grad_(True)
    mug, lvg = g(mu).requires_grad_(True), g(lv).requires_grad_(True)
    parents = torch.as_tensor(synth.PARENTS, dtype=torch.int32, device=DEV)
    loss, terms = ops.training_loss(op, orp, orr, g(_pack_pose(*W[2:])), g(W[0]), g(W[1]), g(gaze), parents, synth.DT,
                                    mug, lvg, kl_weight=oloss.kl_weight(it))
    np.testing.assert_allclose(terms[:18].cpu().numpy(), terms64.numpy(), rtol=3e-5, atol=1e-7)
    assert abs(float(loss) - float(loss64)) < 3e-5 * abs(float(loss64))
    loss.backward()
    ref_pose = _pack_pose(*[o.grad for o in O64[2:]])
    assert relerr(op.grad, ref_pose) < 3e-4
    assert relerr(orp.grad, O64[0].grad) < 3e-4
    assert relerr(orr.grad, O64[1].grad) < 3e-4
    assert relerr(mug.grad, mu64.grad) < 1e-5 and relerr(lvg.grad, lv64.grad) < 1e-5


# ----------------------------------------------------------------------------- RAdam + full iteration
def test_radam_vs_reference(golden_dir):
    gd = np.load(golden_dir / "radam.npz")
    p = g(torch.as_tensor(gd["params"][0].copy()))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for i, gr in enumerate(gd["grads"]):
        rect, scale = oradam.radam_scalars(i + 1, float(gd["lr"]))
        ops.radam_step(p, g(torch.as_tensor(gr)), m, v, 0.9, 0.999, float(gd["eps"]), scale, rect)
        np.testing.assert_allclose(p.cpu().numpy(), gd["params"][i + 1], atol=2e-7)


@pytest.mark.parametrize("big,depth,shield", [(b, d, sh) for b in (0, 1) for d in (4, 6, 8) for sh in (0, 1)])
def test_direct_gemm_variant_selftest(big, depth, shield):
    """Every variant of the direct TN kernel (inline-asm operand loads with hand-counted waits: correctness depends on the compiler
    that built the library) against a float64 host sum -- the check the library itself runs at a variant's first use per process."""
    assert ops.lib().zeggs_gemm_direct_selftest(big, depth, shield) == 1


_DIRECT_FIRST_USE_CHILD = """
import ctypes as C, json, sys, threading
import torch
L = C.CDLL(sys.argv[1])
L.zeggs_last_error.restype = C.c_char_p
VARIANTS = [(b, d, sh) for b in (0, 1) for d in (4, 6, 8) for sh in (0, 1)]
states = lambda: {"%d/%d/%d" % v: L.zeggs_gemm_direct_state(*v) for v in VARIANTS}
def route():
    o = (C.c_int * 4)()
    L.zeggs_gemm_route_get(o)
    return list(o)
out = {"fresh": states()}
Mc, N, K, lddy, ldx = 1282, 130, 70, 131, 73          # GemmArgs 130 x 70 x 1282: 81 k-tiles, ragged tiles and strides
torch.manual_seed(Mc + N)
dy, x, W0, b0 = torch.randn(Mc, lddy), torch.randn(Mc, ldx), torch.randn(N, K), torch.randn(N)
ref_w = W0.double() + dy[:, :N].double().T @ x[:, :K].double()
ref_b = b0.double() + dy[:, :N].double().sum(0)
dyd, xd = dy.cuda(), x.cuda()
def product(dW, db, stream):
    rc = L.zeggs_gemm_tn_bias(C.c_void_p(dyd.data_ptr()), C.c_long(lddy), C.c_void_p(xd.data_ptr()), C.c_long(ldx),
                              C.c_void_p(dW.data_ptr()), C.c_long(K), Mc, N, K, C.c_float(1.0), C.c_void_p(db.data_ptr()),
                              C.c_void_p(stream))
    assert rc == 0, L.zeggs_last_error()
def errs(dW, db):
    return [float((dW.cpu().double() - ref_w).abs().max() / ref_w.abs().max()),
            float((db.cpu().double() - ref_b).abs().max() / ref_b.abs().max())]
# the warm-up: the variants of the engine's route, nothing else
L.zeggs_gemm_route(1, 1, 8, 0)
out["warm_rc"] = L.zeggs_gemm_direct_warm()
out["warmed"] = states()
# a capture: the variant runs unchecked and stays unchecked
L.zeggs_gemm_route(-1, -1, -1, -1)
dW, db = W0.cuda(), b0.cuda()
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    product(dW, db, torch.cuda.current_stream().cuda_stream)
out["after_capture"] = L.zeggs_gemm_direct_state(0, 4, 0)
graph.replay()
torch.cuda.synchronize()
out["captured"] = errs(dW, db)
# two threads meet an unchecked variant at the same moment, each on a stream of its own
gate, outs, failed = threading.Barrier(2), [(W0.cuda(), b0.cuda()) for _ in range(2)], []
torch.cuda.synchronize()
def worker(i):
    try:
        L.zeggs_gemm_route(3, 0, 6, 0)
        s = torch.cuda.Stream()
        gate.wait()
        product(outs[i][0], outs[i][1], s.cuda_stream)
        s.synchronize()
    except BaseException as e:
        failed.append(repr(e))
        gate.abort()
threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
for t in threads: t.start()
for t in threads: t.join()
out["thread_failures"] = failed
out["threads"] = [errs(*o) for o in outs]
out["after_threads"] = states()
dW, db = W0.cuda(), b0.cuda()
product(dW, db, torch.cuda.current_stream().cuda_stream)
torch.cuda.synchronize()
out["default_after"] = errs(dW, db)
out["route_after"] = route()
out["final"] = states()
print(json.dumps(out))
"""


def test_direct_gemm_first_use_warm_capture_and_two_threads():
    """The first use of the direct TN kernel's variants in a process of its own (the states are per process): nothing is checked
    before a launch; zeggs_gemm_direct_warm checks exactly the variants of the calling thread's route (the engine's: both wave
    tiles, shield, depth 8); a product captured into a graph runs its variant unchecked and leaves it unchecked; two threads that
    meet an unchecked variant together, each on its own stream, both get right results, the variant is ok afterwards and the direct
    kernel is still on.  zeggs_gemm_tn_bias at the smallest shape that reaches the stream-K family (81 k-tiles), ragged tiles and
    strides, accumulating, against float64."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _DIRECT_FIRST_USE_CHILD, str(ops._LIB_PATH)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    unchecked = {"%d/%d/%d" % (b, d, sh): -1 for b in (0, 1) for d in (4, 6, 8) for sh in (0, 1)}
    assert out["fresh"] == unchecked
    assert out["warm_rc"] == 0
    assert out["warmed"] == {**unchecked, "0/8/1": 1, "1/8/1": 1}
    assert out["after_capture"] == -1
    assert max(out["captured"]) < 4e-6, out["captured"]
    assert out["thread_failures"] == []
    assert max(max(e) for e in out["threads"]) < 4e-6, out["threads"]
    assert out["after_threads"] == {**unchecked, "0/8/1": 1, "1/8/1": 1, "0/6/0": 1}
    assert max(out["default_after"]) < 4e-6, out["default_after"]
    assert out["route_after"][0] != 0                   # no check failed: the direct kernel is not disabled
    assert out["final"] == {**unchecked, "0/8/1": 1, "1/8/1": 1, "0/6/0": 1, "0/4/0": 1}


@pytest.mark.parametrize("nplanes", [6, 9])
def test_bf16_split_tn_product_is_at_least_as_exact_as_the_fp32_matrix_cores(nplanes):
    """EXPERIMENT (option "gemm_split_bf16", default off; csrc/gemm_split.hip): the fp32 TN products of the training tail on the bf16
    matrix cores with an fp32-exact three-plane operand split.  Acceptance rule: on all five weight-gradient
    shapes the split's max AND RMS error against a float64 product is <= the native fp32 MFMA kernel's (the shielded direct kernel).
    (conv0 FORWARD is an NN product: this kernel is TN only -- it keeps the native path.)"""
    shapes = [("dW_hh", 3072, 1024, 8160, 3072, 1024), ("dW_ih0", 3072, 2286, 8160, 3072, 2288), ("dW_l2", 1131, 1024, 8160, 1132, 1024),
              ("dW_l0", 1024, 1262, 8160, 1024, 2288), ("conv0 dW", 3402, 512, 12288, 3404, 512)]
    keep = {k: ops._OPTIONS.get(k) for k in ("gemm_direct", "gemm_direct_shield", "gemm_direct_depth")}
    try:
        ops.set_option("gemm_direct", 1)
        ops.set_option("gemm_direct_shield", 1)
        ops.set_option("gemm_direct_depth", 8)
        for name, M, N, K, lda, ldb in shapes:
            torch.manual_seed(1)
            A, B = torch.randn(K, lda, device=DEV), torch.randn(K, ldb, device=DEV)
            ref = A[:, :M].double().t() @ B[:, :N].double()
            err = {}
            for npl in (0, nplanes):
                ops.set_option("gemm_split_bf16", npl)
                C = torch.zeros(M, N, device=DEV)
                ops.gemm(A, B, C, M, N, K, (1, lda), (ldb, 1), (N, 1))
                d = C.double() - ref
                err[npl] = (float(d.abs().max()), float(d.pow(2).mean().sqrt()))
            assert err[nplanes][0] <= err[0][0] and err[nplanes][1] <= err[0][1], (name, err)
    finally:
        ops.set_option("gemm_split_bf16", 0)
        for k, v in keep.items():
            if v is not None:
                ops.set_option(k, v)


def test_radam_weight_decay_vs_reference(golden_dir):
    """RAdam(weight_decay=0.05) of the reference (optimizers.py:88-95; radam_wd.npz) through the drop-in optimizer class: per-tensor
    launches and the flat-buffer form."""
    from zeggs import optimizers
    gd = np.load(golden_dir / "radam_wd.npz")
    for flat in (False, True):
        p = torch.nn.Parameter(g(torch.as_tensor(gd["params"][0].copy())))
        if flat:
            fp, fg = p.data.clone(), torch.zeros_like(p.data)
            p.data = fp.view_as(p)
        opt = optimizers.RAdam([p], lr=float(gd["lr"]), eps=float(gd["eps"]), weight_decay=float(gd["weight_decay"]))
        if flat:
            opt.attach_flat(fp, fg)
        for i, gr in enumerate(gd["grads"]):
            if flat:
                fg.copy_(g(torch.as_tensor(gr)))
            p.grad = g(torch.as_tensor(gr))
            opt.step()
            np.testing.assert_allclose(p.detach().cpu().numpy(), gd["params"][i + 1], atol=2e-7, err_msg=f"flat={flat} step {i + 1}")


def _engine_iteration(gd, it, nets, s):
    """One iteration of train_iter.npz through the engine's own fused loss: loss, terms, decoder outputs (pose, root pos, root rot)."""
    se, de, st = nets
    b = [g(torch.as_tensor(gd[f"it{it}_batch{j}"])) for j in range(11)]
    audio, rpos, rrot, rvel, rvrt, lpos, ltxy, lvel, lvrt, gaze, wstyle = b
    T = audio.shape[1]
    speech = se((audio - s["a_mean"]) / s["a_std"])
    z, mu, logvar = st((wstyle - s["in_mean"]) / s["in_std"], eps=g(torch.as_tensor(gd[f"it{it}_eps"])))
    pose0 = _pack_pose(rvel, rvrt, lpos, ltxy, lvel, lvrt)
    pose, orp, orr = ops.decoder_core(de, pose0[:, 0], rpos[:, 0], rrot[:, 0], gaze, speech,
                                      z.unsqueeze(1).repeat(1, T, 1), s["in_mean"], s["in_std"], s["out_mean"],
                                      s["out_std"], synth.DT)
    parents = torch.as_tensor(synth.PARENTS, dtype=torch.int32, device=DEV)
    loss, terms = ops.training_loss(pose, orp, orr, pose0, rpos, rrot, gaze, parents, synth.DT, mu, logvar,
                                    kl_weight=oloss.kl_weight(it))
    return loss, terms, (pose, orp, orr)


def test_train_iteration_vs_reference(golden_dir):
    """Both iterations of the reference train() recorded in train_iter.npz through the engine's own fused loss.
    Iteration 0: loss, 18 terms, gradient samples of all 44 tensors and the weights after the RAdam step against the reference's
    fp32 run.  Iteration 1 (round 5): after a FULL fused RAdam step the weights equal the reference's (3e-7),
    loss and terms equal the reference's; the gradients are held entry by entry (5e-4 of the tensor's largest) to the float64
    arbiter at the engine's own forward point (helpers.grads_at_forward_point: this iteration's loss gradient is dominated by one
    near-degenerate joint, its length moves by percent with the last bits of the forward outputs -- measured on the reference
    itself, tests/test_oracle_golden.py::test_iteration1_conditioning_and_the_forward_point_arbiter), and their DIRECTION to the
    reference's float64 run (train_iter_fp64.npz) at 1 - cos < 1e-4."""
    from zeggs.optimizers import RAdam
    gd = np.load(golden_dir / "train_iter.npz")
    g64 = np.load(golden_dir / "train_iter_fp64.npz")
    se, de, st = [m.to(DEV).train() for m in helpers.build_nets()]
    for m in (se, st):     # dropout was patched to identity when the golden vectors were recorded
        m.eval()
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    plist = [p for m in (se, de, st) for p in m.parameters()]
    opt = RAdam(plist, lr=1e-4, eps=1e-5)
    loss, terms, _ = _engine_iteration(gd, 0, (se, de, st), s)
    np.testing.assert_allclose(float(loss), gd["loss"][0], rtol=1e-5)
    np.testing.assert_allclose(terms[:18].cpu().numpy(), gd["terms"][0], rtol=1e-4, atol=1e-6)
    loss.backward()
    off = 0
    for i, p in enumerate(plist):
        idx = helpers.sample_idx(p.numel())
        got = p.grad.flatten()[torch.as_tensor(idx, device=DEV)].cpu().numpy()
        ref = gd["it0_grad_samples"][off:off + len(idx)]
        scale = max(1e-6, float(np.abs(ref).max()))
        assert np.abs(got - ref).max() < 5e-4 * scale + 1e-8, f"param {i}"
        pw = p.detach().flatten()[torch.as_tensor(idx, device=DEV)].clone()
        gw = p.grad.flatten()[torch.as_tensor(idx, device=DEV)].clone()
        m, v = torch.zeros_like(pw), torch.zeros_like(pw)
        rect, sc = oradam.radam_scalars(1, 1e-4)
        ops.radam_step(pw, gw, m, v, 0.9, 0.999, 1e-5, sc, rect)
        np.testing.assert_allclose(pw.cpu().numpy(), gd["it0_weight_samples"][off:off + len(idx)], atol=2e-7)
        off += len(idx)
    # ---- iteration 1: full fused RAdam step, then the second recorded batch
    opt.step()
    opt.zero_grad(set_to_none=True)
    w1 = np.concatenate([p.detach().flatten()[torch.as_tensor(helpers.sample_idx(p.numel()), device=DEV)].cpu().numpy()
                         for p in plist])
    np.testing.assert_allclose(w1, gd["it0_weight_samples"], atol=3e-7)
    loss, terms, (pose, orp, orr) = _engine_iteration(gd, 1, (se, de, st), s)
    np.testing.assert_allclose(float(loss), gd["loss"][1], rtol=2e-5)
    np.testing.assert_allclose(terms[:18].cpu().numpy(), gd["terms"][1], rtol=2e-4, atol=1e-6)
    loss.backward()
    O_e = [orp.detach(), orr.detach()] + [t.detach() for t in helpers.unpack_pose(pose.detach())]
    Gs, O64, gO = helpers.grads_at_forward_point(gd, 1, [helpers.sd(m) for m in (se, de, st)], O_e)
    dev_out = max(float((a.cpu().double().reshape(b_.shape) - b_).abs().max()) for a, b_ in zip(O_e, O64))
    assert dev_out < 1e-4, dev_out                                   # forward outputs: the north-star tolerance, vs float64
    ref64 = g64["it1_grad_samples64"]
    off, worst, worst_cos, ratios = 0, 0.0, 0.0, []
    for i, (p, r) in enumerate(zip(plist, Gs)):
        gp = p.grad.detach().cpu().double()
        scale = max(1e-12, float(r.abs().max()))
        e = float((gp - r).abs().max()) / scale
        worst = max(worst, e)
        assert e < 5e-4, f"iteration 1, param {i}: {e:.2e} of the tensor's largest entry (arbiter at the engine's forward point)"
        idx = helpers.sample_idx(p.numel())
        a_s, r_s = gp.flatten()[idx].numpy(), ref64[off:off + len(idx)]
        cosd = 1.0 - float(np.dot(a_s, r_s) / max(1e-300, np.linalg.norm(a_s) * np.linalg.norm(r_s)))
        worst_cos = max(worst_cos, cosd)
        ratios.append(float(np.linalg.norm(a_s) / max(1e-300, np.linalg.norm(r_s))))
        off += len(idx)
    assert off == len(ref64) and worst_cos < 1e-4, worst_cos
    jd = (O_e[5][1, 4, 0].cpu().double() - O64[5][1, 4, 0]).abs().max()
    print(f"\niteration 1 through the engine: outputs {dev_out:.1e} from float64 (the degenerate joint (1, 4, 0): {float(jd):.1e}), "
          f"gradients {worst:.1e} of max|g| from the forward-point arbiter, 1 - cos vs the reference's float64 run {worst_cos:.1e}, "
          f"length vs that run {min(ratios):.4f} .. {max(ratios):.4f} (the reference's own fp32 run: 1.0008 .. 1.0067)")


def test_gather_windows_and_rows():
    frames = torch.arange(50 * 7, dtype=torch.float32, device=DEV).reshape(50, 7)
    starts = torch.tensor([0, 13, 42], device=DEV)
    out = ops.gather_windows(frames, starts, 8)
    ref = torch.stack([frames[s:s + 8] for s in (0, 13, 42)])
    assert torch.equal(out, ref)                                          # indices bit-exact
    rows = torch.tensor([[3, 4, 4, 49], [0, 0, 1, 2]], device=DEV)
    assert torch.equal(ops.gather_rows(frames, rows), frames[rows])


# ----------------------------------------------------------------------------- fast (packed) vs generic decoder path
def _rollout_with_grads(de, B, T, seed, style_dim=64):
    torch.manual_seed(seed)
    stats = synth.make_stats()
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    clips = [synth.make_clip(T, seed=300 + b, stats=stats) for b in range(B)]
    tt = lambda k: g(torch.as_tensor(np.stack([c[k] for c in clips])))  # noqa: E731
    pose0 = _pack_pose(tt("Y_root_vel"), tt("Y_root_vrt"), tt("Y_lpos"), tt("Y_ltxy"), tt("Y_lvel"), tt("Y_lvrt"))[:, 0]
    speech = (torch.randn(B, T, 64, device=DEV) * 0.5).requires_grad_(True)
    style = (torch.randn(B, T, style_dim, device=DEV) * 0.5).requires_grad_(True)
    de.zero_grad()
    pose, rp, rr = ops.decoder_core(de, pose0.contiguous(), tt("Y_root_pos")[:, 0].contiguous(),
                                    tt("Y_root_rot")[:, 0].contiguous(), tt("Y_gaze_pos"), speech, style, s["in_mean"],
                                    s["in_std"], s["out_mean"], s["out_std"], synth.DT)
    wp, wr, wq = torch.randn_like(pose), torch.randn_like(rp), torch.randn_like(rr)
    ((pose * wp).sum() + (rp * wr).sum() + (rr * wq).sum()).backward()
    grads = {k: p.grad.clone() for k, p in de.named_parameters()}
    return (pose.detach(), rp.detach(), rr.detach()), grads, speech.grad.clone(), style.grad.clone()


@pytest.mark.parametrize("B,T", [(32, 12), (1, 9), (5, 7), (33, 5), (32, 2), (16, 3), (17, 4), (64, 6)])
def test_decoder_fast_path_matches_generic_path(B, T):
    _, de, _ = helpers.build_nets()
    de = de.to(DEV).train()
    try:
        ops.set_option("decoder_fast", 0)
        out0, g0, ds0, dy0 = _rollout_with_grads(de, B, T, 11)
        ops.set_option("decoder_fast", 1)
        out1, g1, ds1, dy1 = _rollout_with_grads(de, B, T, 11)
    finally:
        ops.set_option("decoder_fast", 1)
    for a, b in zip(out0, out1):
        assert float((a - b).abs().max()) < 2e-5
    assert relerr(ds1, ds0) < 1e-4 and relerr(dy1, dy0) < 1e-4
    for k in g0:
        assert relerr(g1[k], g0[k]) < 1e-4, k


def test_decoder_inference_ring_long_rollout():
    """no_grad path (2-slot ring buffers), B=1, 300 frames: fast == generic to fp32 rounding, and finite."""
    _, de, _ = helpers.build_nets()
    de = de.to(DEV).eval()
    B, T = 1, 300
    stats = synth.make_stats()
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    c = synth.make_clip(T, seed=5, stats=stats)
    tt = lambda k: g(torch.as_tensor(c[k][None]))  # noqa: E731
    pose0 = _pack_pose(tt("Y_root_vel"), tt("Y_root_vrt"), tt("Y_lpos"), tt("Y_ltxy"), tt("Y_lvel"), tt("Y_lvrt"))[:, 0]
    torch.manual_seed(3)
    speech, style = torch.randn(B, T, 64, device=DEV) * 0.5, torch.randn(B, T, 64, device=DEV) * 0.5
    outs = []
    try:
        for fast in (0, 1):
            ops.set_option("decoder_fast", fast)
            with torch.no_grad():
                outs.append(ops.decoder_core(de, pose0.contiguous(), tt("Y_root_pos")[:, 0].contiguous(),
                                             tt("Y_root_rot")[:, 0].contiguous(), tt("Y_gaze_pos"), speech, style,
                                             s["in_mean"], s["in_std"], s["out_mean"], s["out_std"], synth.DT))
    finally:
        ops.set_option("decoder_fast", 1)
    J = 75
    ltxy0, ltxy1 = outs[0][0][..., 6 + 3 * J:6 + 9 * J], outs[1][0][..., 6 + 3 * J:6 + 9 * J]
    assert torch.isfinite(outs[1][0]).all()
    assert float((ltxy0 - ltxy1).abs().max()) < 1e-4          # joint rotations (north_star tolerance)


# ----------------------------------------------------------------------------- audio front-end
def test_mel_features_vs_reference(golden_dir):
    from zeggs import audio
    gd = np.load(golden_dir / "mel.npz")
    for tag in "abc":
        wav, nfr = gd[f"{tag}_wav"], int(gd[f"{tag}_nframes"])
        assert audio.n_anim_frames(len(wav)) == nfr                          # integer, bit-exact
        assert audio.stft_frame_count(len(wav)) == gd[f"{tag}_mel"].shape[1]   # integer, bit-exact
        feat = audio.mel_features(wav, nfr).cpu().numpy()
        ref = gd[f"{tag}_feat"]
        np.testing.assert_array_equal(np.isnan(feat), np.isnan(ref))
        np.testing.assert_allclose(feat, ref, atol=2e-6, equal_nan=True)


def test_mel_unnormalised_bins_vs_reference(golden_dir):
    """audio_conf.normalize_mel_bins = false (ZEGGS/audio/spectrograms.py:431-440) through the drop-in preprocess_audio: the one
    non-shipped audio option value that has a device path (the filterbank is a host table either way)."""
    import json
    from zeggs import audio
    gd = np.load(golden_dir / "mel_nonorm.npz")
    conf = dict(sampling_rate=16000, filter_length=800, hop_length=200, n_mel_channels=80, mel_fmin=20, mel_fmax=7600,
                min_clipping=1e-5, pre_emphasis=False, pre_emph_coeff=0.97, real_amplitude=True, centered=True,
                normalize_mel_bins=False, normalize_range=True, normalize_loudness=False, resample_method="linear")
    for tag in "ab":
        wav, nfr = gd[f"{tag}_wav"], int(gd[f"{tag}_nframes"])
        feat = audio.preprocess_audio(wav, 60, nfr, conf, ["mel_spec", "energy"])
        ref = gd[f"{tag}_feat"]
        np.testing.assert_array_equal(np.isnan(feat), np.isnan(ref))
        np.testing.assert_allclose(feat, ref, atol=2e-6, equal_nan=True)
    json.dumps(conf)


@pytest.mark.parametrize("mel_fft", [1, 0])
def test_mel_pre_emphasis_and_raw_amplitude_vs_reference(golden_dir, mel_fft):
    """audio_conf.pre_emphasis = true (the high-pass inside the kernels' sample fetch, float64), real_amplitude = false (filterbank
    and clip floor x n_fft on the host), centered = false (no reflect padding, other frame count) and normalize_range = false (the
    stored value is 20 log10 s), alone and in pairs, through the drop-in preprocess_audio against the reference's (mel_options.npz); mel_fft = 0: the direct-DFT kernel (the matrix-core DFT stages float32 samples and steps aside
    when the pre-emphasis is on)."""
    from zeggs import audio
    gd = np.load(golden_dir / "mel_options.npz")
    base = dict(sampling_rate=16000, filter_length=800, hop_length=200, n_mel_channels=80, mel_fmin=20, mel_fmax=7600,
                min_clipping=1e-5, pre_emph_coeff=float(gd["pre_emph_coeff"]), centered=True, normalize_mel_bins=True,
                normalize_range=True, normalize_loudness=False, resample_method="linear")
    ops.set_option("mel_fft", mel_fft)
    try:
        for name, over in (("pre", dict(pre_emphasis=True)), ("raw", dict(real_amplitude=False)),
                           ("preraw", dict(pre_emphasis=True, real_amplitude=False)), ("unc", dict(centered=False)),
                           ("rawdb", dict(normalize_range=False)), ("uncrawdb", dict(centered=False, normalize_range=False))):
            conf = dict(base, pre_emphasis=False, real_amplitude=True)
            conf.update(over)
            for tag in "ab":
                wav, nfr = gd[f"{tag}_wav"], int(gd[f"{tag}_nframes"])
                feat = audio.preprocess_audio(wav, 60, nfr, conf, ["mel_spec", "energy"])
                ref = gd[f"{tag}_feat_{name}"]
                np.testing.assert_array_equal(np.isnan(feat), np.isnan(ref))
                np.testing.assert_allclose(feat, ref, atol=3e-6, rtol=3e-6, equal_nan=True, err_msg=f"{name} {tag}")
    finally:
        ops.set_option("mel_fft", 1)


def test_mel_resample_methods_vs_reference(golden_dir):
    """audio_conf.resample_method = "nearest" and "cubic" (the other two kinds scipy.interpolate.griddata takes for 1-D points, reference
    data_pipeline.py:65-79; "cubic" = not-a-knot spline over the whole table, solved on the device per column) through the drop-in
    preprocess_audio against the reference's (mel_resample.npz), centered and uncentered (NaN rows / extrapolated energy at the end);
    any other kind raises as griddata does; the streaming front-end takes "nearest" and refuses "cubic"."""
    import ctypes as C
    from zeggs import audio
    gd = np.load(golden_dir / "mel_resample.npz")
    base = dict(sampling_rate=16000, filter_length=800, hop_length=200, n_mel_channels=80, mel_fmin=20, mel_fmax=7600, min_clipping=1e-5,
                pre_emph_coeff=0.97, pre_emphasis=False, real_amplitude=True, normalize_mel_bins=True, normalize_range=True,
                normalize_loudness=False)
    for name, rm, ce in (("nearest", "nearest", True), ("cubic", "cubic", True), ("unc_nearest", "nearest", False), ("unc_cubic", "cubic", False)):
        conf = dict(base, resample_method=rm, centered=ce)
        for tag in "abc":
            wav, nfr = gd[f"{tag}_wav"], int(gd[f"{tag}_nframes"])
            feat = audio.preprocess_audio(wav, 60, nfr, conf, ["mel_spec", "energy"])
            ref = gd[f"{tag}_feat_{name}"]
            np.testing.assert_array_equal(np.isnan(feat), np.isnan(ref), err_msg=f"{name} {tag}")
            np.testing.assert_allclose(feat, ref, atol=3e-6, rtol=3e-6, equal_nan=True, err_msg=f"{name} {tag}")
    with pytest.raises(ValueError, match="Unknown interpolation method"):
        audio.preprocess_audio(gd["a_wav"], 60, 60, dict(base, resample_method="quadratic", centered=True), ["mel_spec", "energy"])
    with pytest.raises(RuntimeError, match="at least 4 STFT frames"):      # (scipy's interp1d raises for fewer points than the order needs, too)
        audio.mel_features(gd["a_wav"][:1300], 4, centered=False, resample_method="cubic")
    # long tables (the elimination runs in chunks of 64 rows, csrc/spline.hip: nine row counts across a chunk), against the oracle's recurrence
    from oracle import mel as omel
    for n in (16000 * 7 + 200 * r + 13 for r in range(9)):
        wav = synth.synth_wav(n, seed=n).astype(np.float32) / 32768.0
        nfr = audio.n_anim_frames(n)
        feat = audio.mel_features(wav, nfr, resample_method="cubic").cpu().numpy()
        ref = omel.preprocess_audio(wav, nfr, resample_method="cubic")
        np.testing.assert_array_equal(np.isnan(feat), np.isnan(ref))
        np.testing.assert_allclose(feat, ref, atol=3e-6, rtol=3e-6, equal_nan=True)
    # streaming ranges: "nearest" equals the offline table, "cubic" is refused by the C ABI
    L = ops.lib()
    L.zeggs_mel_frames_ready.restype = C.c_long
    L.zeggs_mel_range_workspace_bytes.restype = C.c_size_t
    n = 40000
    wav = synth.synth_wav(n, seed=23).astype(np.float32) / 32768.0
    nfr = audio.n_anim_frames(n)
    fb, min_clip = audio.mel_tables(800, 16000, 80, 20.0, 7600.0, 1e-5, True, True, DEV)
    w = g(torch.as_tensor(wav))

    def ranges(method):
        d = audio.MelDims(800, 200, 80, 16000, 60.0, float(min_clip), 0.0, audio.mel_flags(True, True, method))
        rows, k0 = [], 0
        for got in (9000, 17000, 31000, n):
            final = got == n
            k1 = nfr if final else int(L.zeggs_mel_frames_ready(C.byref(d), C.c_long(got)))
            if k1 <= k0:
                continue
            ws = torch.empty(int(L.zeggs_mel_range_workspace_bytes(C.byref(d), C.c_long(k0), C.c_long(k1))), dtype=torch.uint8, device=DEV)
            out = torch.empty(k1 - k0, 81, device=DEV)
            part = w[:got].contiguous()
            rc = L.zeggs_mel_features_range(C.byref(d), C.c_void_p(part.data_ptr()), C.c_long(got), int(final), C.c_void_p(fb.data_ptr()),
                                            C.c_long(k0), C.c_long(k1), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                            C.c_size_t(ws.numel()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            if rc != 0:
                return rc, L.zeggs_last_error().decode()
            rows.append(out)
            k0 = k1
        return 0, torch.cat(rows).cpu().numpy()

    rc, st = ranges("nearest")
    assert rc == 0
    np.testing.assert_allclose(st, audio.mel_features(wav, nfr, resample_method="nearest").cpu().numpy(), atol=1e-6, rtol=1e-6)
    rc, msg = ranges("cubic")
    assert rc != 0 and "WHOLE signal" in msg


@pytest.mark.parametrize("frames", ["4", "5", "6", "C+1", "C+2", "C+3", "2C+H+5"])
def test_mel_cubic_at_short_signals_vs_reference(frames):
    """resample_method = "cubic" where the spline solver (csrc/spline.hip, on the [STFT frames, 81] feature table) changes path: 4 STFT
    frames (the ends alone), 5 and 6 (the first interior rows), and one, two, three rows into the second chunk of C rows, and a table
    of more than two chunks plus their look-ahead of H rows -- against the oracle's preprocess_audio at the shipped dims."""
    from oracle import mel as omel
    from zeggs import audio, data_pipeline as dp
    c, h, _ = dp.spline_chunk()
    m = {"4": 4, "5": 5, "6": 6, "C+1": c + 1, "C+2": c + 2, "C+3": c + 3, "2C+H+5": 2 * c + h + 5}[frames]
    n = 200 * (m - 1) + 13      # (centred, n_fft 800, hop 200: a signal shorter than n_fft is extended to it and has 4 frames)
    assert audio.stft_frame_count(n) == m and n <= 35000
    wav = synth.synth_wav(n, seed=n).astype(np.float32) / 32768.0
    nfr = audio.n_anim_frames(n)
    feat = audio.mel_features(wav, nfr, resample_method="cubic").cpu().numpy()
    ref = omel.preprocess_audio(wav, nfr, resample_method="cubic")
    np.testing.assert_array_equal(np.isnan(feat), np.isnan(ref))
    np.testing.assert_allclose(feat, ref, atol=3e-6, rtol=3e-6, equal_nan=True)


@pytest.mark.parametrize("pre,real,centered,norm", [(0.0, True, True, True), (0.97, True, True, True), (0.0, False, False, True),
                                                    (0.97, True, False, False), (0.0, True, True, False)])
def test_mel_streaming_ranges_equal_offline_for_every_audio_option(pre, real, centered, norm):
    """the streaming form (zeggs_mel_features_range: rows [k0, k1) from the samples received so far, k1 bounded by
    zeggs_mel_frames_ready) against the offline table, for the shipped audio_conf and the option values that got a device path in round 6
    (pre-emphasis, raw amplitude, uncentered frames, raw dB range)"""
    import ctypes as C
    from zeggs import audio
    L = ops.lib()
    L.zeggs_mel_frames_ready.restype = C.c_long
    L.zeggs_mel_range_workspace_bytes.restype = C.c_size_t
    n = 40000
    wav = synth.synth_wav(n, seed=17).astype(np.float32) / 32768.0
    nfr = audio.n_anim_frames(n)
    full = audio.mel_features(wav, nfr, pre_emph=pre, real_amplitude=real, centered=centered, normalize_range=norm)
    fb, min_clip = audio.mel_tables(800, 16000, 80, 20.0, 7600.0, 1e-5, True, real, DEV)
    d = audio.MelDims(800, 200, 80, 16000, 60.0, float(min_clip), float(pre), audio.mel_flags(centered, norm))
    w = g(torch.as_tensor(wav))
    rows, k0 = [], 0
    for got in (9000, 17000, 31000, n):
        final = got == n
        k1 = nfr if final else int(L.zeggs_mel_frames_ready(C.byref(d), C.c_long(got)))
        if k1 <= k0:
            continue
        ws = torch.empty(int(L.zeggs_mel_range_workspace_bytes(C.byref(d), C.c_long(k0), C.c_long(k1))), dtype=torch.uint8, device=DEV)
        out = torch.empty(k1 - k0, 81, device=DEV)
        part = w[:got].contiguous()
        ops._check(L.zeggs_mel_features_range(C.byref(d), C.c_void_p(part.data_ptr()), C.c_long(got), int(final), C.c_void_p(fb.data_ptr()),
                                              C.c_long(k0), C.c_long(k1), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                              C.c_size_t(ws.numel()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mel_features_range")
        rows.append(out)
        k0 = k1
    st = torch.cat(rows).cpu().numpy()
    fu = full.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(st), np.isnan(fu))
    np.testing.assert_allclose(st, fu, atol=1e-6, rtol=1e-6, equal_nan=True)


def test_mel_fft_form_equals_the_dft_forms(golden_dir):
    """Round 4: the STFT as a real FFT (half-length complex mixed-radix Stockham transform in LDS + split, what the reference's
    np.fft.rfft computes) is the default; the fp64 matrix-core DFT (round 3) and the direct DFT stay behind options.  All three
    against the reference fixtures (2e-6) and against each other (1e-6: float64 spectra a few ulp apart, float32 features), on
    lengths that are / are not multiples of the hop, and on a clip shorter than one window."""
    from zeggs import audio
    gd = np.load(golden_dir / "mel.npz")
    wavs = {tag: (gd[f"{tag}_wav"], int(gd[f"{tag}_nframes"]), gd[f"{tag}_feat"]) for tag in "abc"}
    short = synth.synth_wav(700, seed=3).astype(np.float32) / 32768.0
    try:
        for tag, (wav, nfr, ref) in wavs.items():
            feats = {}
            for name, fft, mfma in (("fft", 1, 1), ("mfma", 0, 1), ("direct", 0, 0)):
                ops.set_option("mel_fft", fft)
                ops.set_option("mel_mfma", mfma)
                feats[name] = audio.mel_features(wav, nfr).cpu().numpy()
                np.testing.assert_array_equal(np.isnan(feats[name]), np.isnan(ref))
                np.testing.assert_allclose(feats[name], ref, atol=2e-6, equal_nan=True, err_msg=f"{tag} {name}")
            for name in ("mfma", "direct"):
                np.testing.assert_allclose(feats["fft"], feats[name], atol=1e-6, equal_nan=True, err_msg=f"{tag} fft vs {name}")
        outs = []
        for fft in (1, 0):
            ops.set_option("mel_fft", fft)
            outs.append(audio.mel_features(short, audio.n_anim_frames(len(short))).cpu().numpy())
        np.testing.assert_allclose(outs[0], outs[1], atol=1e-6, equal_nan=True)
        # round 5: ln(10^(v / 20)) is the affine map v ln(10) / 20 = ln(s) / range + ln(10) / 20; mode 2 (default): that map in float64;
        # mode 0: ln(s) and the energy's exp(2 y) on the hardware log2 / exp2; mode 1: the literal log / pow chain of
        # data_pipeline.py:62-63.  All three against the reference fixtures (2e-6) and against the literal chain
        ops.set_option("mel_fft", 1)
        for tag, (wav, nfr, ref) in wavs.items():
            f = {}
            for mode in (0, 1, 2):
                ops.set_option("mel_exact_log", mode)
                f[mode] = audio.mel_features(wav, nfr).cpu().numpy()
                np.testing.assert_allclose(f[mode], ref, atol=2e-6, equal_nan=True, err_msg=f"{tag} mode {mode}")
            np.testing.assert_allclose(f[2], f[1], atol=2.5e-7, rtol=2.5e-7, equal_nan=True, err_msg=tag)
            np.testing.assert_allclose(f[0], f[1], atol=1e-6, rtol=1e-6, equal_nan=True, err_msg=tag)
    finally:
        ops.set_option("mel_fft", 1)
        ops.set_option("mel_mfma", 1)
        ops.set_option("mel_exact_log", 2)


# ----------------------------------------------------------------------------- drop-in API end to end
def test_generate_gesture_vs_reference(golden_dir, tmp_path):
    """generate_gesture() (wav + exemplar BVH -> BVH) against the reference's own output for the same files."""
    import json
    import scipy.io.wavfile as wavfile
    from zeggs import anim, generate
    gd = np.load(golden_dir / "generate.npz")
    net, data, res = tmp_path / "net", tmp_path / "data", tmp_path / "res"
    net.mkdir(), data.mkdir()
    se, de, st = helpers.build_nets()
    torch.save(se, net / "speech_encoder.pt"), torch.save(de, net / "decoder.pt"), torch.save(st, net / "style_encoder.pt")
    np.savez(data / "stats.npz", **synth.make_stats())
    json.dump(synth.data_definition(), open(data / "data_definition.json", "w"))
    conf = dict(audio_conf=dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True,
                                normalize_mel_bins=True, normalize_range=True, min_clipping=1e-5, sampling_rate=16000,
                                mel_fmin=20, mel_fmax=7600, n_mel_channels=80, filter_length=800, hop_length=200,
                                resample_method="linear", normalize_loudness=False),
                audio_feature_type=["mel_spec", "energy"])
    json.dump(conf, open(data / "data_pipeline_conf.json", "w"))
    wavfile.write(tmp_path / "a.wav", 16000, gd["wav"])
    (tmp_path / "ex.bvh").write_bytes(gd["exemplar_bvh"].tobytes())
    enc = generate.generate_gesture(tmp_path / "a.wav", [(tmp_path / "ex.bvh", None)], net, data, res,
                                    style_encoding_type="example", blend_type="add", blend_ratio=[1.0],
                                    file_name="out", first_pose=tmp_path / "ex.bvh", temperature=1e8, seed=1234)
    assert float((enc.cpu() - torch.as_tensor(gd["encoding"])).abs().max()) < 1e-4
    # the pickle-free checkpoint twin (safetensors + arch.json) generates the same file
    from zeggs import compat
    compat.save_state(tmp_path / "net_st", se, de, st)
    enc2 = generate.generate_gesture(tmp_path / "a.wav", [(tmp_path / "ex.bvh", None)], tmp_path / "net_st", data, res,
                                     style_encoding_type="example", blend_type="add", blend_ratio=[1.0],
                                     file_name="out_st", first_pose=tmp_path / "ex.bvh", temperature=1e8, seed=1234)
    assert float((enc2 - enc).abs().max()) < 1e-5          # (split-K atomics: not bit-reproducible run to run)
    o1, o2 = anim.bvh_load(res / "out.bvh"), anim.bvh_load(res / "out_st.bvh")
    np.testing.assert_allclose(o2["rotations"], o1["rotations"], atol=2e-2)
    np.testing.assert_allclose(o2["positions"], o1["positions"], atol=2e-3)
    out = anim.bvh_load(res / "out.bvh")
    assert out["rotations"].shape == gd["out_rotations"].shape             # integer frame count: bit-exact
    assert (res / "out.wav").exists()
    # Euler angles in degrees as written with 6 decimals; compare as rotations to avoid +-180 wrap artefacts
    qa = oanim.q_from_euler(np.radians(out["rotations"].astype(np.float64)))
    qb = oanim.q_from_euler(np.radians(gd["out_rotations"].astype(np.float64)))
    ang = 2 * np.degrees(np.arccos(np.clip(np.abs(np.sum(qa * qb, axis=-1)), 0, 1)))
    assert ang.max() < 2e-2, ang.max()                                      # < 0.02 degrees on every joint / frame
    np.testing.assert_allclose(out["positions"][:, 0], gd["out_positions"][:, 0], atol=2e-3)


def _bvh_angle_deg(rot_a, rot_b):
    """largest angle (degrees) between two sets of zyx Euler channels, compared as rotations (no +-180 wrap artefacts)"""
    qa = oanim.q_from_euler(np.radians(np.asarray(rot_a, np.float64)))
    qb = oanim.q_from_euler(np.radians(np.asarray(rot_b, np.float64)))
    return float((2 * np.degrees(np.arccos(np.clip(np.abs(np.sum(qa * qb, axis=-1)), 0, 1)))).max())


def test_generate_gesture_branches_vs_reference(golden_dir, tmp_path):
    """The generate_gesture() branches beyond single-style / "add" / first_pose given, each against the REFERENCE's own
    run on the same files (tests/golden/generate_branches.npz, oracle/make_golden.py:gold_generate_branches): two styles
    "stitch" with blend_ratio [0.3, 0.7] (integer frame splits bit-exact, generate.py:280-298, helpers.py:26-37), two styles
    "add" (:299-308), label strings (:270-276), a pre-computed ndarray embedding (:264-269), first_pose=None with a
    (start, end)-trimmed last exemplar (:196-203, 313-354), audio_file=None (:84, 158, 282-284).
    Bounds: integers exact, encodings 1e-4, joint rotations of the BVH < 0.02 degrees, root positions 2e-3."""
    import json
    import scipy.io.wavfile as wavfile
    from zeggs import anim, generate
    gd = np.load(golden_dir / "generate_branches.npz")
    net, netl, data, res = tmp_path / "net", tmp_path / "net_label", tmp_path / "data", tmp_path / "res"
    net.mkdir(), netl.mkdir(), data.mkdir()
    se, de, st = helpers.build_nets()
    torch.save(se, net / "speech_encoder.pt"), torch.save(de, net / "decoder.pt"), torch.save(st, net / "style_encoder.pt")
    nlabels = len(synth.data_definition()["label_names"])
    sel, del_, _ = helpers.build_nets(style_size=nlabels)
    torch.save(sel, netl / "speech_encoder.pt"), torch.save(del_, netl / "decoder.pt")
    np.savez(data / "stats.npz", **synth.make_stats())
    json.dump(synth.data_definition(), open(data / "data_definition.json", "w"))
    conf = dict(audio_conf=dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True,
                                normalize_mel_bins=True, normalize_range=True, min_clipping=1e-5, sampling_rate=16000,
                                mel_fmin=20, mel_fmax=7600, n_mel_channels=80, filter_length=800, hop_length=200,
                                resample_method="linear", normalize_loudness=False),
                audio_feature_type=["mel_spec", "energy"])
    json.dump(conf, open(data / "data_pipeline_conf.json", "w"))
    WAV, A, Bx = tmp_path / "a.wav", tmp_path / "exa.bvh", tmp_path / "exb.bvh"
    wavfile.write(WAV, 16000, gd["wav"])
    A.write_bytes(gd["exa_bvh"].tobytes()), Bx.write_bytes(gd["exb_bvh"].tobytes())
    ratio = [float(r) for r in gd["blend_ratio"]]
    trim = tuple(int(v) for v in gd["trim"])
    label, emb = str(gd["label"]), gd["embedding"]
    # integer frame splits of "stitch": bit-exact
    assert generate.split_by_ratio(135, ratio) == gd["split_135"].tolist()
    common = dict(temperature=1e8, seed=1234)
    two = [(A, None), (Bx, None)]

    def run(tag, audio, styles, netdir, **kw):
        enc = generate.generate_gesture(audio, styles, netdir, data, res if audio is not None else None,
                                        file_name=tag if audio is not None else None, **kw, **common)
        if isinstance(enc, list):
            assert len(enc) == sum(k.startswith(f"{tag}_encoding") for k in gd.files)
            for i, e in enumerate(enc):
                assert tuple(e.shape) == gd[f"{tag}_encoding{i}"].shape
                assert float((e.cpu() - torch.as_tensor(gd[f"{tag}_encoding{i}"])).abs().max()) < 1e-4, tag
        else:
            assert tuple(enc.shape) == gd[f"{tag}_encoding"].shape, tag
            assert float((enc.cpu() - torch.as_tensor(gd[f"{tag}_encoding"])).abs().max()) < 1e-4, tag
        if audio is not None:
            out = anim.bvh_load(res / (tag + ".bvh"))
            assert out["rotations"].shape == gd[f"{tag}_rotations"].shape, tag          # frame count: bit-exact
            ang = _bvh_angle_deg(out["rotations"], gd[f"{tag}_rotations"])
            assert ang < 2e-2, (tag, ang)
            np.testing.assert_allclose(out["positions"][:, 0], gd[f"{tag}_root_positions"], atol=2e-3, err_msg=tag)
            assert (res / (tag + ".wav")).exists()
        return enc

    enc = run("stitch", WAV, two, net, style_encoding_type="example", blend_type="stitch", blend_ratio=ratio, first_pose=A)
    # the per-frame encoding switches styles exactly at the reference's split frame
    s0 = int(gd["split_135"][0][1])
    ref_enc = torch.as_tensor(gd["stitch_encoding"])
    assert float((ref_enc[0, s0 - 1] - ref_enc[0, s0]).abs().max()) > 1e-3         # (the fixture does switch there)
    assert float((enc[0, s0 - 1] - enc[0, 0]).abs().max()) == 0.0 and float((enc[0, s0] - enc[0, -1]).abs().max()) == 0.0
    run("add", WAV, two, net, style_encoding_type="example", blend_type="add", blend_ratio=ratio, first_pose=A)
    run("label", WAV, [label], netl, style_encoding_type="label", blend_type="add", blend_ratio=[1.0], first_pose=Bx)
    run("ndarray", WAV, [(emb, "given")], net, style_encoding_type="example", blend_type="add", blend_ratio=[1.0],
        first_pose=Bx)
    run("nofirst", WAV, [(A, None), (Bx, trim)], net, style_encoding_type="example", blend_type="add",
        blend_ratio=[0.6, 0.4], first_pose=None)
    run("noaudio_stitch", None, two, net, style_encoding_type="example", blend_type="stitch", blend_ratio=ratio)
    run("noaudio_add", None, two, net, style_encoding_type="example", blend_type="add", blend_ratio=ratio)
    run("noaudio_trim", None, [(Bx, trim)], net, style_encoding_type="example", blend_type="add", blend_ratio=[1.0])
    # first_pose as an already-parsed clip dictionary (generate.py:316-317) = the same file given as a path
    enc_d = generate.generate_gesture(WAV, [(emb, "given")], net, data, res, style_encoding_type="example", blend_type="add",
                                      blend_ratio=[1.0], file_name="ndarray_dict", first_pose=anim.bvh_load(Bx), **common)
    assert float((enc_d.cpu() - torch.as_tensor(gd["ndarray_encoding"])).abs().max()) < 1e-6
    o = anim.bvh_load(res / "ndarray_dict.bvh")
    assert _bvh_angle_deg(o["rotations"], gd["ndarray_rotations"]) < 2e-2
    # the seed fixes the VAE noise (generate.py:86-87): the same call twice at temperature 1 gives the same encoding, another seed
    # another one
    kw = dict(style_encoding_type="example", blend_type="add", blend_ratio=[1.0], temperature=1.0)
    e1 = generate.generate_gesture(None, [(A, None)], net, data, None, seed=77, **kw)
    e2 = generate.generate_gesture(None, [(A, None)], net, data, None, seed=77, **kw)
    e3 = generate.generate_gesture(None, [(A, None)], net, data, None, seed=78, **kw)
    assert float((e1 - e2).abs().max()) < 1e-5 and float((e1 - e3).abs().max()) > 1e-3       # (split-K atomics: not bitwise)
    # default file name (generate.py:391-392): audio_<wav stem>_label_<style name>
    generate.generate_gesture(WAV, [(emb, "given")], net, data, res, style_encoding_type="example", blend_type="add",
                              blend_ratio=[1.0], first_pose=Bx, **common)
    assert (res / "audio_a_label_given.bvh").exists() and (res / "audio_a_label_given.wav").exists()


def test_generate_gesture_streaming_writer_equals_one_launch(golden_dir, tmp_path, monkeypatch):
    """Long clips go through generate._decode_to_bvh_streaming (chunked persistent decode, BVH rows converted on the device per
    chunk and formatted by host threads underneath the next chunks): the file it writes equals the one-launch path's -- same
    header bytes, same frame count, joint rotations < 0.06 degrees, root positions 5e-3 -- for chunk sizes that do and do not
    divide the clip, including a single chunk, and the first-pose exemplar is parsed once."""
    import json
    import scipy.io.wavfile as wavfile
    from zeggs import anim, generate
    gd = np.load(golden_dir / "generate.npz")
    net, data, res = tmp_path / "net", tmp_path / "data", tmp_path / "res"
    net.mkdir(), data.mkdir()
    se, de, st = helpers.build_nets()
    torch.save(se, net / "speech_encoder.pt"), torch.save(de, net / "decoder.pt"), torch.save(st, net / "style_encoder.pt")
    np.savez(data / "stats.npz", **synth.make_stats())
    json.dump(synth.data_definition(), open(data / "data_definition.json", "w"))
    conf = dict(audio_conf=dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True,
                                normalize_mel_bins=True, normalize_range=True, min_clipping=1e-5, sampling_rate=16000,
                                mel_fmin=20, mel_fmax=7600, n_mel_channels=80, filter_length=800, hop_length=200,
                                resample_method="linear", normalize_loudness=False),
                audio_feature_type=["mel_spec", "energy"])
    json.dump(conf, open(data / "data_pipeline_conf.json", "w"))
    wavfile.write(tmp_path / "a.wav", 16000, synth.synth_wav(16000 * 12 + 777, seed=31))        # 12 s -> 723 frames
    (tmp_path / "ex.bvh").write_bytes(gd["exemplar_bvh"].tobytes())
    kw = dict(style_encoding_type="example", blend_type="add", blend_ratio=[1.0], first_pose=tmp_path / "ex.bvh",
              temperature=1e8, seed=1234)
    loads = []
    orig_load = anim.bvh_load
    monkeypatch.setattr(anim, "bvh_load", lambda f: (loads.append(str(f)), orig_load(f))[1])
    enc0 = generate.generate_gesture(tmp_path / "a.wav", [(tmp_path / "ex.bvh", None)], net, data, res, file_name="one", **kw)
    assert len(loads) == 1, loads                 # style exemplar == first pose: parsed once
    ref = anim.bvh_load(res / "one.bvh")
    head_ref = open(res / "one.bvh").read().split("MOTION")[0]
    for tag, chunk, block in (("c250", 250, 64), ("c361", 361, 1024), ("c1", 100000, 100)):
        monkeypatch.setattr(generate, "STREAM_MIN_FRAMES", 100)
        monkeypatch.setattr(generate, "STREAM_CHUNK", chunk)
        monkeypatch.setattr(generate, "STREAM_BLOCK", block)
        enc = generate.generate_gesture(tmp_path / "a.wav", [(tmp_path / "ex.bvh", None)], net, data, res, file_name=tag, **kw)
        assert float((enc - enc0).abs().max()) < 1e-5
        assert open(res / f"{tag}.bvh").read().split("MOTION")[0] == head_ref                  # hierarchy + offsets: same bytes
        out = anim.bvh_load(res / f"{tag}.bvh")
        assert out["rotations"].shape == ref["rotations"].shape == (723, 75, 3), out["rotations"].shape
        # (chunk boundaries re-enter the recurrence through the unmerged layer0: fp32 re-association of ~1e-6 per boundary, which the
        #  free-running random-init rollout carries and amplifies over the 723 frames -- measured 0.005 .. 0.022 degrees from run to
        #  run (split-K atomics in the prologue GEMMs); a state hand-over bug would show as degrees)
        assert _bvh_angle_deg(out["rotations"], ref["rotations"]) < 6e-2, tag
        np.testing.assert_allclose(out["positions"][:, 0], ref["positions"][:, 0], atol=5e-3, err_msg=tag)
        assert (res / f"{tag}.wav").read_bytes() == (tmp_path / "a.wav").read_bytes()


def test_train_api_label_conditioning_runs(tmp_path):
    """train() with style_encoding_type = "label" (configs_v2.json): no style encoder, one-hot label rows gathered per window (the row
    indices go through the dataset's pinned upload ring, engine.DeviceDataset.upload_indices), next batch prefetched behind every step."""
    from zeggs import train as train_mod
    from zeggs.train import train
    npz, jsn = synth.write_dataset(tmp_path / "data", n_train=3, n_valid=1, nframes=40, seed=5)
    net_opt = {"decoder": {"nhidden": 1024, "num_rnn_layers": 2, "rnn_cond": "normal"},
               "speech_encoder": {"nhidden": 64, "speech_encoding_size": 64},
               "style_encoder": {"nhidden": 512, "style_encoding_size": 64, "example_length": 16, "type": "attn", "use_vae": True}}
    train_opt = dict(niterations=0.004, batchsize=4, window=8, change_pace=True, learning_rate=1e-4, learning_rate_decay=0.995,
                     eps=1e-5, resume=False, use_gpu=True, thread_count=1, seed=1234, use_tensorboard=False,
                     style_encoding_type="label", generate_samples_step=100, use_script=False)
    (tmp_path / "models").mkdir(), (tmp_path / "logs").mkdir()
    assert train(tmp_path / "models", tmp_path / "logs", npz, jsn, train_opt, net_opt) is None
    eng = train_mod.last_engine
    assert eng.iteration >= 4 and eng.st is None and torch.isfinite(eng.last_terms).all()
    assert eng.prefetch_hits >= eng.iteration - 2            # every batch but an epoch's first came from the prefetch
    assert (tmp_path / "models" / "decoder.pt").exists() and not (tmp_path / "models" / "style_encoder.pt").exists()


def test_train_api_runs_and_checkpoints(tmp_path):
    """train() with the reference's option dictionaries on a tiny synthetic dataset: runs, loss finite, writes
    the reference's checkpoint layout (incl. iteration 0), and the checkpoints load back into generate-able nets."""
    from zeggs import compat
    from zeggs import train as train_mod
    from zeggs.train import train
    npz, jsn = synth.write_dataset(tmp_path / "data", n_train=2, n_valid=1, nframes=40, seed=3)
    net_opt = {"decoder": {"nhidden": 1024, "num_rnn_layers": 2, "rnn_cond": "normal"},
               "speech_encoder": {"nhidden": 64, "speech_encoding_size": 64},
               "style_encoder": {"nhidden": 512, "style_encoding_size": 64, "example_length": 16, "type": "attn",
                                 "use_vae": True}}
    train_opt = dict(niterations=0.004, batchsize=4, window=8, change_pace=True, learning_rate=1e-4,
                     learning_rate_decay=0.995, eps=1e-5, resume=False, use_gpu=True, thread_count=1, seed=1234,
                     use_tensorboard=True, style_encoding_type="example", generate_samples_step=3, use_script=False)
    (tmp_path / "models").mkdir(), (tmp_path / "logs").mkdir()
    assert train(tmp_path / "models", tmp_path / "logs", npz, jsn, train_opt, net_opt) is None     # like the reference
    eng = train_mod.last_engine
    # sample animations of the checkpoint iterations (train.py:516-760): 3 train + 3 valid clips, ground + prediction
    from zeggs import anim
    samples = sorted((tmp_path / "logs" / "samples").glob("iteration_0_*.bvh"))
    assert len(samples) == 12 and len(list((tmp_path / "logs" / "samples").glob("iteration_3_*.bvh"))) == 12
    for split in ("train", "valid"):
        gt = anim.bvh_load(next((tmp_path / "logs" / "samples").glob(f"iteration_0_{split}_ground_0_*.bvh")))
        pr = anim.bvh_load(next((tmp_path / "logs" / "samples").glob(f"iteration_0_{split}_predict_0_*.bvh")))
        assert gt["rotations"].shape == pr["rotations"].shape == (40, 75, 3)
        assert np.isfinite(pr["rotations"]).all() and np.isfinite(pr["positions"]).all()
        assert np.abs(gt["rotations"][0] - pr["rotations"][0]).max() < 1e-3     # frame 0 = the given first pose
        assert np.abs(gt["positions"][0] - pr["positions"][0]).max() < 1e-4
    # the loss terms of every iteration under logs/tb (SummaryWriter events, or scalars.jsonl without tensorboard)
    tb = list((tmp_path / "logs" / "tb").iterdir())
    assert tb
    if (tmp_path / "logs" / "tb" / "scalars.jsonl").exists():
        import json
        rows = [json.loads(x) for x in open(tmp_path / "logs" / "tb" / "scalars.jsonl")]
        assert len(rows) == eng.iteration and set(rows[0]["losses/losses"]) == set(train_mod.LOSS_TAGS)
        assert abs(sum(rows[-1]["losses/losses"].values()) / 18 - rows[-1]["losses/total_loss"]) < 1e-4
    assert eng.iteration >= 4 and torch.isfinite(eng.last_terms).all()
    # every parameter is saved in its own storage (not the engine's whole flat buffer per file)
    assert (tmp_path / "models" / "speech_encoder.pt").stat().st_size < 2 * 4 * sum(p.numel() for p in eng.se.parameters()) + 65536
    for f in ("speech_encoder.pt", "decoder.pt", "style_encoder.pt", "checkpoints.pt"):
        assert (tmp_path / "models" / f).exists() and (tmp_path / "models" / "0" / f).exists()
    de = compat.load_module(tmp_path / "models" / "decoder.pt", DEV)
    assert "recurrent_decoder.layer1.weight_hh_l1" in de.state_dict()
    ck = torch.load(tmp_path / "models" / "checkpoints.pt", weights_only=False)
    assert set(ck) == {"iteration", "epoch", "loss", "optimizer_state_dict"}


@pytest.mark.parametrize("B", [1, 2])
def test_decoder_gemv_decode_path_matches_mfma_path(B):
    """B <= 2 no_grad rollouts use the GEMV stage kernels; option bit 1024 forces the MFMA path for comparison."""
    _, de, _ = helpers.build_nets()
    de = de.to(DEV).eval()
    T = 40
    stats = synth.make_stats()
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    clips = [synth.make_clip(T, seed=500 + b, stats=stats) for b in range(B)]
    tt = lambda k: g(torch.as_tensor(np.stack([c[k] for c in clips])))  # noqa: E731
    pose0 = _pack_pose(tt("Y_root_vel"), tt("Y_root_vrt"), tt("Y_lpos"), tt("Y_ltxy"), tt("Y_lvel"), tt("Y_lvrt"))[:, 0]
    torch.manual_seed(9)
    speech, style = torch.randn(B, T, 64, device=DEV) * 0.5, torch.randn(B, T, 64, device=DEV) * 0.5
    outs = []
    try:
        for v in (1024, 0):
            ops.set_option("stage_variant", v)
            with torch.no_grad():
                outs.append(ops.decoder_core(de, pose0.contiguous(), tt("Y_root_pos")[:, 0].contiguous(),
                                             tt("Y_root_rot")[:, 0].contiguous(), tt("Y_gaze_pos"), speech, style,
                                             s["in_mean"], s["in_std"], s["out_mean"], s["out_std"], synth.DT))
    finally:
        ops.set_option("stage_variant", 0)
    for a, b in zip(outs[0], outs[1]):
        assert torch.isfinite(b).all()
        assert float((a - b).abs().max()) < 5e-5


@pytest.mark.parametrize("B", [1, 2])
def test_chained_decode_launches_match_plain_launches(B):
    """option "chain": consecutive stage launches alternate between two streams and hand over through device-side
    arrival counters (every launch fetches its weights while its predecessor runs).  Same arithmetic per stage up to the
    summation order of the dot products; every bounded wait must have been satisfied.  Since round 6 the chained kernels
    are part of measurement builds only (-DZEGGS_CHAIN: they spill at the occupancy run-ahead needs and lost to the persistent
    decode kernel): the default library must refuse the option instead of accepting and ignoring it."""
    try:
        ops.set_option("chain", 1)
    except RuntimeError as e:
        assert "ZEGGS_CHAIN" in str(e)
        ops.set_option("chain", 0)
        pytest.skip("chained launches are not part of this build")
    ops.set_option("chain", 0)
    _, de, _ = helpers.build_nets()
    de = de.to(DEV).eval()
    T = 400
    stats = synth.make_stats()
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    clips = [synth.make_clip(T, seed=600 + b, stats=stats) for b in range(B)]
    tt = lambda k: g(torch.as_tensor(np.stack([c[k] for c in clips])))  # noqa: E731
    pose0 = _pack_pose(tt("Y_root_vel"), tt("Y_root_vrt"), tt("Y_lpos"), tt("Y_ltxy"), tt("Y_lvel"), tt("Y_lvrt"))[:, 0]
    torch.manual_seed(9)
    speech, style = torch.randn(B, T, 64, device=DEV) * 0.5, torch.randn(B, T, 64, device=DEV) * 0.5
    outs = []
    try:
        ops.set_option("persistent", 0)          # the stage-launch path is under test here
        for v in (0, 1, 1):
            ops.set_option("chain", v)
            with torch.no_grad():
                outs.append(ops.decoder_core(de, pose0.contiguous(), tt("Y_root_pos")[:, 0].contiguous(),
                                             tt("Y_root_rot")[:, 0].contiguous(), tt("Y_gaze_pos"), speech, style,
                                             s["in_mean"], s["in_std"], s["out_mean"], s["out_std"], synth.DT))
            torch.cuda.synchronize()
            assert ops.last_decoder_chain_errors() == 0
    finally:
        ops.set_option("chain", 0)
        ops.set_option("persistent", 1)
    for a, b in zip(outs[0], outs[1]):
        assert torch.isfinite(b).all()
        assert float((a - b).abs().max()) < 5e-5
    for a, b in zip(outs[1], outs[2]):             # run to run: only the split-K atomics of the prologue GEMMs (2e-7) differ
        assert float((a - b).abs().max()) < 2e-5


@pytest.mark.parametrize("B,T,tiles4", [(32, 12, 1), (17, 6, 1), (5, 9, 1), (32, 4, 1), (64, 6, 1), (40, 5, 1), (32, 12, 0), (64, 6, 0)])
def test_persistent_training_forward_matches_stage_launches(B, T, tiles4):
    """option "train_persistent" (default on for batch <= 64): the forward rollout of a training step as one
    weight-stationary launch.  Outputs and, through the unchanged BPTT that consumes what the forward saved, every
    gradient must agree with the stage-launch forward.  tiles4: the GRU phases on 4-row v_mfma_f32_4x4x1 tiles (batch 17..32 and
    49..64; default) or on the 16-row tiles every batch size can use."""
    _, de, _ = helpers.build_nets()
    de = de.to(DEV).train()
    try:
        ops.set_option("tp_tiles4", tiles4)
        ops.set_option("train_persistent", 0)
        out0, g0, ds0, dy0 = _rollout_with_grads(de, B, T, 21)
        ops.set_option("train_persistent", 1)
        out1, g1, ds1, dy1 = _rollout_with_grads(de, B, T, 21)
        assert ops.lib().zeggs_persistent_state(1) == 1            # it really ran (validated, not fallen back)
    finally:
        ops.set_option("train_persistent", 1)
        ops.set_option("tp_tiles4", 1)
    for a, b in zip(out0, out1):
        assert float((a - b).abs().max()) < 2e-5
    assert relerr(ds1, ds0) < 1e-4 and relerr(dy1, dy0) < 1e-4
    for k in g0:
        assert relerr(g1[k], g0[k]) < 1e-4, k


@pytest.mark.parametrize("B,T", [(32, 6), (17, 5), (64, 4), (5, 4)])
def test_training_rollout_prologue_in_five_launches(B, T):
    """option "tp_prologue" (round 6, default on): in front of the persistent training rollout [dec_init | dec_fill_cond | tp_cond] run
    as ONE launch, [CellStateEncoder layer 0 | hid_1 | the step-1 pose product] as one (gemm.hip: skinny_multi_k), the two halves of
    the CellStateEncoder's last layer as one -- five launches instead of ten, the same arithmetic in the same order: outputs and
    gradients equal up to the atomics of the stream-K products (the weight fold of the packs, the weight gradients; measured 5e-7)."""
    _, de, _ = helpers.build_nets()
    de = de.to(DEV).train()
    try:
        ops.set_option("tp_prologue", 0)
        out0, g0, ds0, dy0 = _rollout_with_grads(de, B, T, 33)
        ops.set_option("tp_prologue", 1)
        out1, g1, ds1, dy1 = _rollout_with_grads(de, B, T, 33)
        assert ops.lib().zeggs_persistent_state(1) == 1
    finally:
        ops.set_option("tp_prologue", 1)
    for a, b in zip(out0, out1):
        assert float((a - b).abs().max()) < 5e-6, float((a - b).abs().max())
    assert relerr(ds1, ds0) < 1e-5 and relerr(dy1, dy0) < 1e-5
    for k in g0:
        assert relerr(g1[k], g0[k]) < 1e-5, k


@pytest.mark.parametrize("B,T,style_dim", [(32, 12, 64), (17, 6, 64), (20, 5, 9), (32, 4, 64), (27, 40, 64)])
def test_dual_chain_training_forward_matches_stage_launches(B, T, style_dim):
    """option "tp_dual" (off by default: measured slower than the single-chain sweep, profiles/r06_dual_chain_forward.txt): the
    forward rollout of batch 17..32 as TWO independent 16-row dependency chains in one launch (csrc/train_dual.hip -- per-wave class
    polls, LDS-counter reductions, every published vector loaded once, no workgroup barrier in the time loop).  Outputs and, through the
    unchanged BPTT that consumes what the forward saved, every gradient must agree with the stage-launch forward; a second run
    (steady state, no validation sync) too.  style_dim 9 = label conditioning (fewer conditioning k-blocks than waves)."""
    torch.manual_seed(77)
    from zeggs import modules
    if style_dim == 64:
        _, de, _ = helpers.build_nets()
    else:
        de = modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, style_dim, 1024, 2)
    de = de.to(DEV).train()
    try:
        ops.set_option("train_persistent", 0)
        out0, g0, ds0, dy0 = _rollout_with_grads(de, B, T, 21, style_dim)
        ops.set_option("tp_dual", 1)
        ops.set_option("train_persistent", 1)
        out1, g1, ds1, dy1 = _rollout_with_grads(de, B, T, 21, style_dim)
        assert ops.lib().zeggs_persistent_state(1) == 1            # it really ran (validated, not fallen back)
        out2, g2, ds2, dy2 = _rollout_with_grads(de, B, T, 21, style_dim)
    finally:
        ops.set_option("tp_dual", 0)
        ops.set_option("train_persistent", 1)
    for outx, gx, dsx, dyx in ((out1, g1, ds1, dy1), (out2, g2, ds2, dy2)):
        for a, b in zip(out0, outx):
            assert float((a - b).abs().max()) < 2e-5
        assert relerr(dsx, ds0) < 1e-4 and relerr(dyx, dy0) < 1e-4
        for k in g0:
            assert relerr(gx[k], g0[k]) < 1e-4, k


def test_dual_chain_training_forward_gives_up_cleanly():
    """the dual-chain sweep under "persistent_spin" = 0 (the first unsatisfied wait runs out): error word set, the validated first
    use falls back to the stage launches, results equal theirs."""
    _, de, _ = helpers.build_nets()
    de = de.to(DEV).train()
    try:
        ops.set_option("train_persistent", 0)
        out0, g0, ds0, dy0 = _rollout_with_grads(de, 32, 8, 21)
        ops.set_option("tp_dual", 1)
        ops.set_option("train_persistent", 1)          # (re-enabling resets the validation state: the next use is checked)
        ops.set_option("persistent_spin", 0)
        import warnings
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            out1, g1, ds1, dy1 = _rollout_with_grads(de, 32, 8, 21)
        # gave up either way: on a first (validated) use the library disables the kernel silently (state 0), after a validated use
        # earlier in the process the sticky status word reports it and ops warns; both redo the rollout on the stage launches
        assert ops.lib().zeggs_persistent_state(1) == 0 or any("training rollout" in str(w.message) for w in seen)
    finally:
        ops.set_option("persistent_spin", 1 << 21)
        ops.set_option("tp_dual", 0)
        ops.set_option("train_persistent", 1)
    for a, b in zip(out0, out1):
        assert torch.isfinite(b).all() and float((a - b).abs().max()) < 2e-5
    for k in g0:
        assert relerr(g1[k], g0[k]) < 1e-4, k


@pytest.mark.parametrize("B,T,style_dim", [(32, 12, 64), (17, 6, 64), (5, 9, 64), (1, 7, 64), (32, 3, 64), (20, 5, 9), (64, 6, 9),
                                           (40, 5, 64)])
def test_persistent_bptt_sweep_matches_stage_launches(B, T, style_dim):
    """option "bwd_persistent" (default on for batch <= 64): the backward decoder steps of a window as one weight-stationary
    launch on 4-row MFMA tiles (batch 33..64: two sweeps of <= 32 rows).  Same forward either way; every parameter gradient, dspeech and dstyle must agree with the
    stage-launch sweep (which the oracle / reference fixtures pin) to fp32 rounding.  style_dim 9 = label conditioning."""
    torch.manual_seed(1234)
    from zeggs import modules
    if style_dim == 64:
        _, de, _ = helpers.build_nets()
    else:
        de = modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, style_dim, 1024, 2)
    de = de.to(DEV).train()
    try:
        ops.set_option("bwd_persistent", 0)
        out0, g0, ds0, dy0 = _rollout_with_grads(de, B, T, 23, style_dim)
        ops.set_option("bwd_persistent", 1)
        out1, g1, ds1, dy1 = _rollout_with_grads(de, B, T, 23, style_dim)
        assert ops.lib().zeggs_persistent_state(2) == 1            # it really ran (validated, not fallen back)
        out2, g2, ds2, dy2 = _rollout_with_grads(de, B, T, 23, style_dim)      # steady state (no validation sync)
    finally:
        ops.set_option("bwd_persistent", 1)
    for a, b in zip(out0, out1):
        assert float((a - b).abs().max()) < 2e-5
    for gx, dsx, dyx in ((g1, ds1, dy1), (g2, ds2, dy2)):
        assert relerr(dsx, ds0) < 2e-5 and relerr(dyx, dy0) < 2e-5
        for k in g0:
            assert relerr(gx[k], g0[k]) < 2e-5, k


@pytest.mark.parametrize("T", [4, 5, 37, 600])
def test_persistent_decode_kernel_matches_stage_launches(T):
    """B=1 inference: the weight-stationary persistent kernel (one launch for all frames, weights in registers, data-tagged
    granule exchange between CUs) against the chain of stage launches; also deterministic and resumable (streaming state)."""
    _, de, _ = helpers.build_nets()
    de = de.to(DEV).eval()
    stats = synth.make_stats()
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    clip = synth.make_clip(max(T, 4), seed=611, stats=stats)
    tt = lambda k: g(torch.as_tensor(clip[k][None, :T]))  # noqa: E731
    pose0 = _pack_pose(tt("Y_root_vel"), tt("Y_root_vrt"), tt("Y_lpos"), tt("Y_ltxy"), tt("Y_lvel"), tt("Y_lvrt"))[:, 0]
    torch.manual_seed(10)
    speech, style = torch.randn(1, T, 64, device=DEV) * 0.5, torch.randn(1, T, 64, device=DEV) * 0.5
    outs = []
    try:
        for v in (0, 1, 1):
            ops.set_option("persistent", v)
            with torch.no_grad():
                outs.append(ops.decoder_core(de, pose0.contiguous(), tt("Y_root_pos")[:, 0].contiguous(),
                                             tt("Y_root_rot")[:, 0].contiguous(), tt("Y_gaze_pos"), speech, style,
                                             s["in_mean"], s["in_std"], s["out_mean"], s["out_std"], synth.DT))
            torch.cuda.synchronize()
    finally:
        ops.set_option("persistent", 1)
    assert ops.lib().zeggs_persistent_state(0) == 1               # validated on this process, not fallen back
    for a, b in zip(outs[0], outs[1]):
        assert torch.isfinite(b).all()
        assert float((a - b).abs().max()) < 5e-5
    for a, b in zip(outs[1], outs[2]):             # run to run: only the split-K atomics of the prologue GEMMs (2e-7) differ
        assert float((a - b).abs().max()) < 2e-5


# ----------------------------------------------------------------------------- edge cases
def _oracle_vs_hip_rollout(B, T, style_dim, tol=1e-4):
    torch.manual_seed(1234)
    from zeggs import modules
    de = modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, style_dim, 1024, 2)
    stats = synth.make_stats()
    s = helpers.stats_tensors()
    clips = [synth.make_clip(max(T, 4), seed=700 + b, stats=stats) for b in range(B)]
    tt = lambda k: torch.as_tensor(np.stack([c[k][:T] for c in clips]))  # noqa: E731
    torch.manual_seed(4)
    speech, style = torch.randn(B, T, 64) * 0.5, torch.randn(B, T, style_dim) * 0.5
    fp = [tt(k)[:, 0] for k in ("Y_root_pos", "Y_root_rot", "Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel",
                                "Y_lvrt")]
    with torch.no_grad():
        ref = onets.decoder_rollout(helpers.sd(de), *fp, tt("Y_gaze_pos"), speech, style, s["in_mean"], s["in_std"],
                                    s["out_mean"], s["out_std"], synth.DT)
        de = de.to(DEV).eval()
        out = de(*[g(t) for t in fp], g(tt("Y_gaze_pos")), g(speech), g(style), None, g(s["in_mean"]), g(s["in_std"]),
                 g(s["out_mean"]), g(s["out_std"]), synth.DT)
    for n, o, r in zip(NAMES, out, ref):
        assert o.shape == r.shape, n
        assert float((o.cpu() - r).abs().max()) < tol, n


def test_decoder_label_conditioning_dims():
    """configs_v2: style = one-hot over 19 labels (decoder input width 1217, W_ih0 [3072, 2241])."""
    _oracle_vs_hip_rollout(B=3, T=5, style_dim=19)


def test_decoder_b1_label_conditioning_vs_oracle():
    """B=1 with the label-conditioning width (one-hot over 19 labels): the persistent decode kernel against the oracle."""
    _oracle_vs_hip_rollout(B=1, T=12, style_dim=19)
    assert ops.lib().zeggs_persistent_state(0) == 1


def test_decoder_shortest_sequences():
    _oracle_vs_hip_rollout(B=2, T=2, style_dim=64)       # one generated frame
    _oracle_vs_hip_rollout(B=2, T=1, style_dim=64)       # nothing to generate: outputs = the given first pose


def test_decoder_batch_above_fast_path_limit_uses_generic_path():
    _oracle_vs_hip_rollout(B=65, T=3, style_dim=64)


def test_loss_is_zero_and_finite_when_prediction_equals_target():
    stats = synth.make_stats()
    c = synth.make_clip(6, seed=1, stats=stats)
    tt = lambda k: g(torch.as_tensor(c[k][None]))  # noqa: E731
    pose = _pack_pose(tt("Y_root_vel"), tt("Y_root_vrt"), tt("Y_lpos"), tt("Y_ltxy"), tt("Y_lvel"), tt("Y_lvrt"))
    parents = torch.as_tensor(synth.PARENTS, dtype=torch.int32, device=DEV)
    loss, terms = ops.training_loss(pose.clone().requires_grad_(True), tt("Y_root_pos"), tt("Y_root_rot"), pose,
                                    tt("Y_root_pos"), tt("Y_root_rot"), tt("Y_gaze_pos"), parents, synth.DT)
    assert float(loss) == 0.0 and float(terms[:18].abs().max()) == 0.0


# ----------------------------------------------------------------------------- animation kernels (csrc/anim.hip)
FEAT_NAMES = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "lrot", "ltxy", "lvel", "lvrt", "cpos", "crot",
              "ctxy", "cvel", "cvrt", "gaze_pos", "gaze_dir")


def test_anim_features_vs_oracle_and_reference(golden_dir, tmp_path):
    """exemplar BVH -> preprocess_animation on the device: float64 agreement with the NumPy oracle (1e-9) and with
    the reference's own output (its float32 steps bound that comparison: 2e-4)"""
    from zeggs import anim
    gd = np.load(golden_dir / "generate.npz")
    (tmp_path / "ex.bvh").write_bytes(gd["exemplar_bvh"].tobytes())
    clip = anim.bvh_load(tmp_path / "ex.bvh")
    dev = anim.preprocess_animation(clip, DEV)
    ora = oanim.preprocess_animation(clip)
    for n, a, b in zip(FEAT_NAMES, dev, ora):
        tol = 1e-6 if a.dtype == torch.float32 else 1e-9
        np.testing.assert_allclose(a.cpu().numpy(), np.asarray(b), atol=tol, rtol=tol, err_msg=n)
        np.testing.assert_allclose(a.cpu().numpy(), gd["feat_" + n], atol=2e-4, rtol=1e-4, err_msg=n)


@pytest.mark.parametrize("order", ["xyz", "yzx", "xzy"])
def test_anim_features_other_channel_orders_vs_oracle_and_reference(golden_dir, order):
    """BVH rotation channels in an order other than the rigs' "zyx" (ZEGGS/anim/bvh.py:54-60 reads it from the file, quat.from_euler
    takes any): the device features against the oracle (float64) and the reference's own output (anim_orders.npz)."""
    from zeggs import anim
    gd = np.load(golden_dir / "anim_orders.npz")
    clip = synth.make_bvh_clip(24, seed=31)
    clip["order"] = order
    dev = anim.preprocess_animation(clip, DEV)
    ora = oanim.preprocess_animation(clip)
    for n, a, b in zip(FEAT_NAMES, dev, ora):
        tol = 1e-6 if a.dtype == torch.float32 else 1e-9
        np.testing.assert_allclose(a.cpu().numpy(), np.asarray(b), atol=tol, rtol=tol, err_msg=n)
        np.testing.assert_allclose(a.cpu().numpy(), gd[f"{order}_{n}"], atol=1e-3 if "v" in n[1:] else 2e-4, rtol=1e-4, err_msg=n)


def test_pose_to_bvh_channel_order_xzy_vs_reference(golden_dir):
    """quat.to_euler's second order (ZEGGS/anim/quat.py:120-125) on the device: the same rotations as the reference's channels
    (compared as quaternions: euler angles are not unique at the poles); any other order raises as the reference does."""
    from zeggs import anim
    gd = np.load(golden_dir / "anim_orders.npz")
    lrot = gd["w_lrot"]
    T, J = lrot.shape[:2]
    # two-axis encoding of the rotations (what the decoder emits): the first two columns of the rotation matrix, as rows
    m = oanim.q_to_xform(lrot) if hasattr(oanim, "q_to_xform") else None
    if m is None:
        w, x, y, z = (lrot[..., i] for i in range(4))
        m = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                      np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                      np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    ltxy = np.stack([m[..., :, 0], m[..., :, 1]], axis=-2).astype(np.float32)
    g32 = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=DEV)  # noqa: E731
    rp, rr = np.zeros((T, 3)), np.tile(np.array([1.0, 0, 0, 0]), (T, 1))
    for order in ("xzy", "zyx"):
        _, eul = anim.bvh_channels(g32(rp), g32(rr), g32(np.zeros((T, J, 3))), g32(ltxy), order=order)
        qa = oanim.q_from_euler(np.radians(eul.cpu().numpy()), order)
        qb = oanim.q_from_euler(np.radians(gd[f"w_euler_{order}"]), order)
        assert np.abs(np.abs(np.sum(qa * qb, axis=-1)) - 1.0).max() < 1e-6, order       # (the two-axis rows went through float32)
    with pytest.raises(NotImplementedError, match="Cannot convert to ordering"):
        anim.bvh_channels(g32(rp), g32(rr), g32(np.zeros((T, J, 3))), g32(ltxy), order="yxz")


@pytest.mark.parametrize("nframes", [4, 5, 257, 1000])
def test_anim_features_sizes_and_median(nframes):
    """odd / even frame counts exercise both np.median branches of the gaze target; long clips the sign unrolling
    (rotations sweep through +-180 degrees so consecutive raw quaternions flip sign)"""
    from zeggs import anim
    clip = synth.make_bvh_clip(nframes, seed=nframes)
    rng = np.random.default_rng(nframes)
    clip["rotations"] = clip["rotations"].astype(np.float64)
    clip["rotations"][:, 3:9, 0] += np.linspace(0, 900, nframes)[:, None] + rng.standard_normal((nframes, 6))
    clip["rotations"] = (clip["rotations"] + 180.0) % 360.0 - 180.0        # wrapped channels, as BVH files store them
    raw = oanim.q_from_euler(np.radians(clip["rotations"]))
    assert nframes < 100 or (np.sum(raw[1:] * raw[:-1], axis=-1) < 0).any()   # the unrolling has work to do
    dev = anim.preprocess_animation(clip, DEV)
    ora = oanim.preprocess_animation(clip)
    for n, a, b in zip(FEAT_NAMES, dev, ora):
        tol = 2e-6 if a.dtype == torch.float32 else 1e-8
        np.testing.assert_allclose(a.cpu().numpy(), np.asarray(b), atol=tol, rtol=tol, err_msg=f"{n} N={nframes}")


def test_anim_features_rejects_short_clips():
    from zeggs import anim
    with pytest.raises(RuntimeError, match="at least 4 frames"):
        anim.preprocess_animation(synth.make_bvh_clip(3, seed=0), DEV)


def test_pose_to_bvh_vs_oracle_and_reference(golden_dir):
    """decoder outputs captured inside the reference's generate_gesture -> BVH channels on the device"""
    from zeggs import anim
    gd = np.load(golden_dir / "generate.npz")
    t = lambda k: torch.as_tensor(gd[k], device=DEV)  # noqa: E731
    for start in (None, (np.array([0, 0, 0]), np.array([1, 0, 0, 0])), (np.array([1.0, 2, 3]), np.array([0.6, 0, 0.8, 0]))):
        kw = {} if start is None else dict(start_position=start[0], start_rotation=start[1])
        pos, eul = anim.bvh_channels(t("dec_root_pos"), t("dec_root_rot"), t("dec_lpos"), t("dec_ltxy"), **kw)
        opos, oeul = oanim.bvh_channels(gd["dec_root_pos"], gd["dec_root_rot"], gd["dec_lpos"], gd["dec_ltxy"], **kw)
        np.testing.assert_allclose(pos.cpu().numpy(), opos, atol=1e-9)
        qa, qb = oanim.q_from_euler(np.radians(eul.cpu().numpy())), oanim.q_from_euler(np.radians(oeul))
        assert np.abs(np.abs(np.sum(qa * qb, axis=-1)) - 1.0).max() < 1e-12
    pos, eul = anim.bvh_channels(t("dec_root_pos"), t("dec_root_rot"), t("dec_lpos"), t("dec_ltxy"),
                                 start_position=np.array([0, 0, 0]), start_rotation=np.array([1, 0, 0, 0]))
    np.testing.assert_allclose(pos.cpu().numpy()[:, 0], gd["out_positions"][:, 0], atol=2e-5)     # out.bvh: 6 decimals
    qa = oanim.q_from_euler(np.radians(eul.cpu().numpy()))
    qb = oanim.q_from_euler(np.radians(gd["out_rotations"].astype(np.float64)))
    assert np.abs(np.abs(np.sum(qa * qb, axis=-1)) - 1.0).max() < 1e-9


# ----------------------------------------------------------------------------- option-surface variants
def _variant_nets():
    """rnn_cond="film" decoder and type="gru" style encoder, seed 4321 in the golden's construction order"""
    from zeggs import modules
    torch.manual_seed(4321)
    de = modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, 64, 1024, 2, rnn_cond="film")
    st = modules.StyleEncoder(synth.POSE_IN, 512, 64, type="gru", use_vae=True)
    return de, st


def test_film_decoder_forward_backward(golden_dir):
    """RecurrentDecoderFiLM: forward vs the reference's rollout (variants.npz), inference ring path vs the same,
    BPTT gradients vs the float64 oracle"""
    gd = np.load(golden_dir / "variants.npz")
    de, _ = _variant_nets()
    for k, v in de.state_dict().items():
        np.testing.assert_allclose(helpers.fingerprint(v), gd[f"fp_decoder.{k}"], rtol=1e-12, atol=0, err_msg=k)
    s = helpers.stats_tensors()
    t = lambda k: torch.as_tensor(gd[k])  # noqa: E731
    fp = [t("in_" + k)[:, 0] for k in ("Y_root_pos", "Y_root_rot", "Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy",
                                       "Y_lvel", "Y_lvrt")]
    gaze, speech, style = t("in_Y_gaze_pos"), t("in_speech"), t("in_style")
    de_g = de.to(DEV).train()
    stat = [g(s[k]) for k in ("in_mean", "in_std", "out_mean", "out_std")]
    with torch.no_grad():      # ring path
        out = de_g(*[g(x) for x in fp], g(gaze), g(speech), g(style), None, *stat, synth.DT)
    for n, o in zip(NAMES, out):
        assert float((o.cpu() - t("O_" + n)).abs().max()) < 1e-4, n
    B, T = speech.shape[:2]
    torch.manual_seed(3)
    wts = [torch.randn(B, T, *o.shape[1:]) for o in fp]
    s64 = {k: v.double() for k, v in s.items()}
    w64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in de_g.state_dict().items()}
    sp64, sy64 = speech.double().requires_grad_(True), style.double().requires_grad_(True)
    O = onets.decoder_rollout(w64, *[x.double() for x in fp], gaze.double(), sp64, sy64, s64["in_mean"], s64["in_std"],
                              s64["out_mean"], s64["out_std"], synth.DT)
    sum((o * w.double()).sum() for o, w in zip(O, wts)).backward()
    spg, syg = g(speech).requires_grad_(True), g(style).requires_grad_(True)
    out = de_g(*[g(x) for x in fp], g(gaze), spg, syg, None, *stat, synth.DT)
    for n, o, r in zip(NAMES, out, O):
        assert float((o.detach().cpu().double() - r.detach()).abs().max()) < 1e-4, n
        assert float((o.detach().cpu() - t("O_" + n)).abs().max()) < 1e-4, n      # training-mode path vs reference
    sum((o * g(w)).sum() for o, w in zip(out, wts)).backward()
    assert relerr(spg.grad, sp64.grad) < 3e-4
    assert relerr(syg.grad, sy64.grad) < 3e-4
    for k, p in de_g.named_parameters():
        assert relerr(p.grad, w64[k].grad) < 3e-4, k


@pytest.mark.parametrize("B,T", [(5, 6), (33, 4)])
def test_film_decoder_stage_path_batches(golden_dir, B, T):
    """RecurrentDecoderFiLM on the fragment-packed stage kernels at batches the variants fixture (B = 2) does not reach: the
    matrix-core inference path (B >= 3), two and three batch blocks, a style that changes every frame (the modulation vectors
    are per step: ZEGGS/modules.py:213-225 inside the frame loop :107-137).  Forward 1e-4 / gradients 3e-4 against the oracle in
    float64, and against the generic per-step GEMM path (option decoder_fast = 0)."""
    gd, _, s = _golden_nets(golden_dir)
    de, _ = _variant_nets()
    de_g = de.to(DEV).train()
    torch.manual_seed(100 + B)
    speech, style = torch.randn(B, T, 64) * 0.5, torch.randn(B, T, 64) * 0.5
    rep = lambda x: x.repeat((B + 1) // 2, *([1] * (x.dim() - 1)))[:B].clone()  # noqa: E731
    fp = [rep(x) for x in _first_pose(gd)]
    for x in fp:
        x += 0.01 * torch.randn_like(x)
    fp[1] = fp[1] / fp[1].norm(dim=-1, keepdim=True)
    gaze = rep(torch.as_tensor(gd["in_Y_gaze_pos"])[:, :1]).repeat(1, T, 1) + 0.05 * torch.randn(B, T, 3)
    wts = [torch.randn(B, T, *o.shape[1:]) for o in fp]
    s64 = {k: v.double() for k, v in s.items()}
    w64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in de_g.state_dict().items()}
    sp64, sy64 = speech.double().requires_grad_(True), style.double().requires_grad_(True)
    O = onets.decoder_rollout(w64, *[t.double() for t in fp], gaze.double(), sp64, sy64, s64["in_mean"], s64["in_std"],
                              s64["out_mean"], s64["out_std"], synth.DT)
    sum((o * w.double()).sum() for o, w in zip(O, wts)).backward()
    stat = [g(s[k]) for k in ("in_mean", "in_std", "out_mean", "out_std")]
    with torch.no_grad():      # ring path
        out = de_g(*[g(x) for x in fp], g(gaze), g(speech), g(style), None, *stat, synth.DT)
    for n, o, r in zip(NAMES, out, O):
        assert float((o.cpu().double() - r.detach()).abs().max()) < 1e-4, n
    spg, syg = g(speech).requires_grad_(True), g(style).requires_grad_(True)
    out = de_g(*[g(x) for x in fp], g(gaze), spg, syg, None, *stat, synth.DT)
    for n, o, r in zip(NAMES, out, O):
        assert float((o.detach().cpu().double() - r.detach()).abs().max()) < 1e-4, n
    sum((o * g(w)).sum() for o, w in zip(out, wts)).backward()
    assert relerr(spg.grad, sp64.grad) < 3e-4 and relerr(syg.grad, sy64.grad) < 3e-4
    for k, p in de_g.named_parameters():
        assert relerr(p.grad, w64[k].grad) < 3e-4, k
    fast_grads = {k: p.grad.clone() for k, p in de_g.named_parameters()}
    try:       # unfolded stage launches (5 per step and direction instead of 4) on the same inputs
        ops.set_option("stage_variant", 4096 + 8192)
        de_g.zero_grad()
        sp3 = g(speech).requires_grad_(True)
        unf = de_g(*[g(x) for x in fp], g(gaze), sp3, g(style), None, *stat, synth.DT)
        sum((o * g(w)).sum() for o, w in zip(unf, wts)).backward()
    finally:
        ops.set_option("stage_variant", 0)
    for n, o, r in zip(NAMES, out, unf):
        assert float((o.detach() - r.detach()).abs().max()) < 1e-4, n
    assert relerr(spg.grad, sp3.grad) < 1e-4
    for k, p in de_g.named_parameters():
        assert relerr(fast_grads[k], p.grad) < 1e-4, k
    try:       # the generic path on the same inputs
        ops.set_option("decoder_fast", 0)
        de_g.zero_grad()
        sp2, sy2 = g(speech).requires_grad_(True), g(style).requires_grad_(True)
        ref = de_g(*[g(x) for x in fp], g(gaze), sp2, sy2, None, *stat, synth.DT)
        sum((o * g(w)).sum() for o, w in zip(ref, wts)).backward()
    finally:
        ops.set_option("decoder_fast", 1)
    for n, o, r in zip(NAMES, out, ref):
        assert float((o.detach() - r.detach()).abs().max()) < 1e-4, n
    assert relerr(spg.grad, sp2.grad) < 1e-4 and relerr(syg.grad, sy2.grad) < 1e-4
    for k, p in de_g.named_parameters():
        assert relerr(fast_grads[k], p.grad) < 1e-4, k


def test_gru_style_encoder_forward_backward(golden_dir):
    """StyleEncoderGRU (+VAE): forward vs the reference, gradients vs the float64 oracle"""
    gd = np.load(golden_dir / "variants.npz")
    _, st = _variant_nets()
    for k, v in st.state_dict().items():
        np.testing.assert_allclose(helpers.fingerprint(v), gd[f"fp_style.{k}"], rtol=1e-12, atol=0, err_msg=k)
    s = helpers.stats_tensors()
    ex = (torch.as_tensor(gd["in_example"]) - s["in_mean"]) / s["in_std"]
    eps = torch.as_tensor(gd["in_eps"])
    st_g = st.to(DEV).train()
    exg = g(ex).requires_grad_(True)
    z, mu, lv = st_g(exg, 1.0, eps=g(eps))
    for a, k in ((z, "gru_z"), (mu, "gru_mu"), (lv, "gru_logvar")):
        assert float((a.detach().cpu() - torch.as_tensor(gd[k])).abs().max()) < 2e-5, k
    w64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in st_g.state_dict().items()}
    z64, mu64, lv64 = onets.style_encoder(w64, ex.double(), eps.double(), 1.0)
    torch.manual_seed(5)
    wz, wm, wl = torch.randn_like(z64), torch.randn_like(z64), torch.randn_like(z64)
    ((z64 * wz).sum() + (mu64 * wm).sum() + (lv64 * wl).sum()).backward()
    ((z * g(wz.float())).sum() + (mu * g(wm.float())).sum() + (lv * g(wl.float())).sum()).backward()
    for k, p in st_g.named_parameters():
        assert relerr(p.grad, w64[k].grad) < 3e-4, k


@pytest.mark.parametrize("B,T", [(1, 101), (3, 70)])
def test_film_decoder_inference_modulation_blocks(golden_dir, B, T):
    """FiLM inference over more frames than one block of modulation vectors (decoder_ws.h FILM_GB = 32: the ring of 2 x 32 frames
    wraps twice at T = 101) with a style that changes every frame: the stage path (B = 1: GEMV launches, B = 3: matrix-core
    launches) against the generic per-step path, which evaluates the two predictors frame by frame"""
    gd, _, s = _golden_nets(golden_dir)
    de, _ = _variant_nets()
    de_g = de.to(DEV).eval()
    torch.manual_seed(7 * B + T)
    speech, style = torch.randn(B, T, 64) * 0.5, torch.randn(B, T, 64) * 0.5
    rep = lambda x: x.repeat((B + 1) // 2, *([1] * (x.dim() - 1)))[:B].clone()  # noqa: E731
    fp = [rep(x) for x in _first_pose(gd)]
    gaze = rep(torch.as_tensor(gd["in_Y_gaze_pos"])[:, :1]).repeat(1, T, 1)
    stat = [g(s[k]) for k in ("in_mean", "in_std", "out_mean", "out_std")]
    with torch.no_grad():
        out = de_g(*[g(x) for x in fp], g(gaze), g(speech), g(style), None, *stat, synth.DT)
        try:
            ops.set_option("decoder_fast", 0)
            ref = de_g(*[g(x) for x in fp], g(gaze), g(speech), g(style), None, *stat, synth.DT)
        finally:
            ops.set_option("decoder_fast", 1)
    for n, o, r in zip(NAMES, out, ref):
        assert bool(torch.isfinite(o).all()), n
        assert float((o - r).abs().max()) < 5e-4 * max(1.0, float(r.abs().max())), n


def test_film_and_gru_variants_batch_vs_reference(golden_dir):
    """The stage-kernel path of rnn_cond = "film" and style type = "gru" against the REFERENCE at a batch of two 16-row blocks
    (B = 19, T = 12, exemplar 33, a style that changes every frame; variants_batch.npz: the reference's outputs, its autograd's
    input gradients in full and 512 samples of every parameter gradient): outputs 1e-4, style code 2e-5, gradients 3e-4 of the
    reference's max |g| (the float32 floor the round-3 verdict accepted for the gradient bound)."""
    gd = np.load(golden_dir / "variants_batch.npz")
    de, st = _variant_nets()
    first, gaze, example, wts, (wz, wm, wl) = helpers.variants_batch_inputs(gd)
    s = helpers.stats_tensors()
    de_g, st_g = de.to(DEV).train(), st.to(DEV).train()
    stat = [g(s[k]) for k in ("in_mean", "in_std", "out_mean", "out_std")]
    t = lambda k: torch.as_tensor(gd[k])  # noqa: E731
    z, mu, lv = st_g(g((example - s["in_mean"]) / s["in_std"]), 1.0, eps=g(t("in_eps")))
    for a, k in ((z, "gru_z"), (mu, "gru_mu"), (lv, "gru_logvar")):
        assert float((a.detach().cpu() - t(k)).abs().max()) < 2e-5, k
    spg, syg = g(t("in_speech")).requires_grad_(True), g(t("in_style")).requires_grad_(True)
    out = de_g(*[g(x) for x in first], g(gaze), spg, syg, None, *stat, synth.DT)
    for n, o in zip(NAMES, out):
        assert float((o.detach().cpu() - t("O_" + n)).abs().max()) < 1e-4, n
    (sum((o * g(w)).sum() for o, w in zip(out, wts)) + (z * g(wz)).sum() + (mu * g(wm)).sum() + (lv * g(wl)).sum()).backward()
    assert relerr(spg.grad, t("d_speech")) < 3e-4 and relerr(syg.grad, t("d_style")) < 3e-4
    helpers.assert_grad_samples(gd, "decoder", [(k, p.grad) for k, p in de_g.named_parameters()], 3e-4)
    helpers.assert_grad_samples(gd, "style", [(k, p.grad) for k, p in st_g.named_parameters()], 3e-4)
    with torch.no_grad():      # the inference ring (matrix-core stage launches at B >= 3, modulation vectors per frame)
        out = de_g(*[g(x) for x in first], g(gaze), g(t("in_speech")), g(t("in_style")), None, *stat, synth.DT)
    for n, o in zip(NAMES, out):
        assert float((o.cpu() - t("O_" + n)).abs().max()) < 1e-4, n


@pytest.mark.parametrize("B,L", [(32, 24), (35, 7)])
def test_gru_style_encoder_stage_path_batch(B, L):
    """StyleEncoderGRU with the forward-direction recurrence on the stage kernels (one launch per frame and direction) at
    batches of two / three 16-row blocks: outputs and every gradient against the oracle in float64 and against the generic
    per-step GEMM path (option decoder_fast = 0)"""
    _, st = _variant_nets()
    st_g = st.to(DEV).train()
    torch.manual_seed(L)
    ex, eps = torch.randn(B, L, synth.POSE_IN), torch.randn(B, 64)
    w64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in st_g.state_dict().items()}
    z64, mu64, lv64 = onets.style_encoder(w64, ex.double(), eps.double(), 1.0)
    wz, wm, wl = torch.randn_like(z64), torch.randn_like(z64), torch.randn_like(z64)
    ((z64 * wz).sum() + (mu64 * wm).sum() + (lv64 * wl).sum()).backward()

    def run():
        st_g.zero_grad()
        z, mu, lv = st_g(g(ex), 1.0, eps=g(eps))      # (the exemplar is data: the binding returns no gradient for it)
        ((z * g(wz.float())).sum() + (mu * g(wm.float())).sum() + (lv * g(wl.float())).sum()).backward()
        return z.detach(), mu.detach(), lv.detach(), {k: p.grad.clone() for k, p in st_g.named_parameters()}

    z, mu, lv, gr = run()
    for a, r in ((z, z64), (mu, mu64), (lv, lv64)):
        assert float((a.cpu().double() - r.detach()).abs().max()) < 5e-5
    for k in gr:
        assert relerr(gr[k], w64[k].grad) < 3e-4, k
    try:
        ops.set_option("decoder_fast", 0)
        z2, mu2, lv2, gr2 = run()
    finally:
        ops.set_option("decoder_fast", 1)
    assert float((z - z2).abs().max()) < 2e-5 and float((lv - lv2).abs().max()) < 2e-5
    for k in gr:
        assert relerr(gr[k], gr2[k]) < 1e-4, k
    # the same two frame sweeps captured into hipGraphs and replayed (option "sweep_graphs"): same launches, same results
    import ctypes
    c0, r0, c1, r1 = (ctypes.c_long(0) for _ in range(4))
    ops.lib().zeggs_sweep_graph_stats(ctypes.byref(c0), ctypes.byref(r0))
    try:
        ops.set_option("sweep_graphs", 1)
        z3, mu3, lv3, gr3 = run()
    finally:
        ops.set_option("sweep_graphs", 0)
    ops.lib().zeggs_sweep_graph_stats(ctypes.byref(c1), ctypes.byref(r1))
    assert (c1.value + r1.value) - (c0.value + r0.value) == 2
    assert float((z - z3).abs().max()) < 2e-6 and float((lv - lv3).abs().max()) < 2e-6
    for k in gr:
        assert relerr(gr[k], gr3[k]) < 1e-5, k


@pytest.mark.parametrize("L", [1, 2, 37])
def test_gru_style_encoder_sequence_lengths(L):
    """exemplars of 1 / 2 / odd lengths (the reverse direction always contributes exactly one step)"""
    _, st = _variant_nets()
    st_g = st.to(DEV).eval()
    torch.manual_seed(L)
    ex, eps = torch.randn(3, L, synth.POSE_IN), torch.randn(3, 64)
    z, mu, lv = st_g(g(ex), 1.0, eps=g(eps))
    z0, mu0, lv0 = onets.style_encoder(helpers.sd(st_g.cpu()), ex, eps, 1.0)
    assert float((z.cpu() - z0).abs().max()) < 5e-5 and float((lv.cpu() - lv0).abs().max()) < 5e-5


# ----------------------------------------------------------------------------- streaming inference
@pytest.mark.parametrize("seed,nsamp", [(0, 48000), (1, 40123)])
def test_streaming_matches_offline_generation(seed, nsamp):
    """any chunking of the audio yields the frames of the offline path (mel -> speech encoder -> decoder): integer
    frame count bit-exact, values to fp32 re-association (chunk boundaries re-enter through the unmerged layer0)"""
    from zeggs import anim, audio, stream
    se, de, _ = helpers.build_nets()
    se, de = se.to(DEV).eval(), de.to(DEV).eval()
    stats = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32, device=DEV) for k, v in synth.make_stats().items()}
    conf = dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True, normalize_mel_bins=True,
                normalize_range=True, min_clipping=1e-5, sampling_rate=16000, mel_fmin=20, mel_fmax=7600,
                n_mel_channels=80, filter_length=800, hop_length=200, resample_method="linear", normalize_loudness=False)
    wav = synth.synth_wav(nsamp, seed=seed).astype(np.float32) / 32768.0
    first = anim.preprocess_animation(synth.make_bvh_clip(8, seed=3), DEV)
    torch.manual_seed(seed)
    style = torch.randn(1, 64, device=DEV) * 0.5
    # offline
    n_frames = audio.n_anim_frames(len(wav))
    feats = torch.as_tensor(audio.preprocess_audio(wav, 60, n_frames, conf, ["mel_spec", "energy"]), device=DEV)
    with torch.no_grad():
        sp = se(((feats[None] - stats["audio_input_mean"]) / stats["audio_input_std"]).contiguous())
        f32 = lambda a: a[0:1].to(torch.float32).contiguous()  # noqa: E731
        rp, rr, rv, rw, lp, _, lt, lv, lw = first[:9]
        pose0 = torch.cat([f32(x).reshape(1, -1) for x in (rv, rw, lp, lt, lv, lw)], dim=1)
        gaze = f32(first[14]).repeat(n_frames, 1)[None].contiguous()
        ref = ops.decoder_core(de, pose0, f32(rp), f32(rr), gaze, sp, style.repeat(n_frames, 1)[None].contiguous(),
                               stats["anim_input_mean"], stats["anim_input_std"], stats["anim_output_mean"],
                               stats["anim_output_std"], synth.DT)
    # streamed with irregular chunks (some shorter than one STFT hop, some several seconds)
    gs = stream.GestureStream(se, de, first, style, stats, conf, synth.DT)
    rng = np.random.default_rng(seed)
    outs, pos = [], 0
    while pos < len(wav):
        n = int(rng.choice([37, 160, 1600, 5000, 16000]))
        outs.append(gs.push(wav[pos:pos + n]))
        pos += n
    outs.append(gs.finish())
    cat = lambda k: torch.cat([o[k] for o in outs if o], dim=0)  # noqa: E731
    assert cat("pose").shape[0] == n_frames == ref[0].shape[1]
    assert sum(1 for o in outs if o) >= 3                                   # frames really left incrementally
    for k, r in zip(("pose", "rpos", "rrot"), ref):
        assert float((cat(k) - r[0]).abs().max()) < 5e-5, k


def test_streaming_vs_the_reference_generate_gesture(golden_dir):
    """zeggs.stream.GestureStream against the REFERENCE directly (round 3 compared it with the offline HIP path only): the 2 s
    clip of generate.npz -- the reference's own generate_gesture() run, whose decoder outputs were captured on their way into
    the BVH conversion (oracle/make_golden.py:gold_generate) -- pushed through the stream in irregular chunks with the
    reference's style encoding, first pose and nets: joint rotations / positions / root trajectory of every frame 1e-4."""
    from zeggs import anim, stream
    gd = np.load(golden_dir / "generate.npz")
    se, de, _ = helpers.build_nets()
    se, de = se.to(DEV).eval(), de.to(DEV).eval()
    stats = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32, device=DEV) for k, v in synth.make_stats().items()}
    conf = dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True, normalize_mel_bins=True,
                normalize_range=True, min_clipping=1e-5, sampling_rate=16000, mel_fmin=20, mel_fmax=7600,
                n_mel_channels=80, filter_length=800, hop_length=200, resample_method="linear", normalize_loudness=False)
    wav = gd["wav"].astype(np.float32) / 32768.0
    clip = dict(rotations=gd["ex_rotations"], positions=gd["ex_positions"], offsets=gd["ex_offsets"], parents=gd["ex_parents"],
                names=synth.BONE_NAMES, order="zyx", frametime=synth.DT)
    first = anim.preprocess_animation(clip, DEV)
    style = torch.as_tensor(gd["encoding"][:, 0], device=DEV)            # the reference's own (per-frame constant) encoding
    gs = stream.GestureStream(se, de, first, style, stats, conf, synth.DT)
    outs, pos = [], 0
    for n in (700, 5000, 123, 9000, 16000, 1177):
        outs.append(gs.push(wav[pos:pos + n]))
        pos += n
    assert pos == len(wav)
    outs.append(gs.finish())
    cat = lambda k: torch.cat([o[k] for o in outs if o], dim=0).cpu().numpy()  # noqa: E731
    pose, rpos, rrot = cat("pose"), cat("rpos"), cat("rrot")
    T, J = gd["dec_ltxy"].shape[0], synth.NJ
    assert pose.shape[0] == T                                             # integer frame count: bit-exact
    assert np.abs(pose[:, 6 + 3 * J:6 + 9 * J].reshape(T, J, 2, 3) - gd["dec_ltxy"]).max() < 1e-4
    assert np.abs(pose[:, 6:6 + 3 * J].reshape(T, J, 3) - gd["dec_lpos"]).max() < 1e-4
    assert np.abs(rpos - gd["dec_root_pos"]).max() < 1e-4 and np.abs(rrot - gd["dec_root_rot"]).max() < 1e-4


# ----------------------------------------------------------------------------- BASELINE.json full size
def test_full_size_rollout_fast_equals_generic_and_is_linear_in_loss_weights():
    """configs[1] shape (B=32, T=256): the fragment-packed stage kernels (merged stages, batch split) and the generic
    per-step GEMM path are two independent implementations of the same recurrence -> outputs and all gradients agree;
    and BPTT is linear in the upstream gradient (2x the loss weights -> 2x every gradient)."""
    _, de, _ = helpers.build_nets()
    de = de.to(DEV).train()
    B, T = 32, 256
    try:
        ops.set_option("decoder_fast", 0)
        out0, g0, ds0, dy0 = _rollout_with_grads(de, B, T, 21)
        ops.set_option("decoder_fast", 1)
        out1, g1, ds1, dy1 = _rollout_with_grads(de, B, T, 21)
    finally:
        ops.set_option("decoder_fast", 1)
    for a, b in zip(out0, out1):
        assert torch.isfinite(a).all() and float((a - b).abs().max()) < 5e-4        # 255 chained steps of fp32 re-association
    assert relerr(ds1, ds0) < 2e-3 and relerr(dy1, dy0) < 2e-3
    for k in g0:
        assert relerr(g1[k], g0[k]) < 2e-3, k
    # linearity of the backward sweep in the upstream gradient
    torch.manual_seed(21)
    stats = synth.make_stats()
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    clips = [synth.make_clip(T, seed=300 + b, stats=stats) for b in range(B)]
    tt = lambda k: g(torch.as_tensor(np.stack([c[k] for c in clips])))  # noqa: E731
    pose0 = _pack_pose(tt("Y_root_vel"), tt("Y_root_vrt"), tt("Y_lpos"), tt("Y_ltxy"), tt("Y_lvel"), tt("Y_lvrt"))[:, 0]
    speech = (torch.randn(B, T, 64, device=DEV) * 0.5).requires_grad_(True)
    style = torch.randn(B, T, 64, device=DEV) * 0.5
    grads = []
    for scale in (1.0, 2.0):
        de.zero_grad()
        speech.grad = None
        pose, rp, rr = ops.decoder_core(de, pose0.contiguous(), tt("Y_root_pos")[:, 0].contiguous(),
                                        tt("Y_root_rot")[:, 0].contiguous(), tt("Y_gaze_pos"), speech, style, s["in_mean"],
                                        s["in_std"], s["out_mean"], s["out_std"], synth.DT)
        torch.manual_seed(5)
        wp = torch.randn_like(pose)
        (scale * (pose * wp).sum()).backward()
        grads.append((speech.grad.clone(), de.recurrent_decoder.layer1.weight_hh_l0.grad.clone()))
    assert relerr(grads[1][0], 2.0 * grads[0][0]) < 1e-4 and relerr(grads[1][1], 2.0 * grads[0][1]) < 1e-4


def test_decoder_rollout_is_graph_capturable():
    """the C ABI neither allocates nor synchronises: a whole no_grad rollout (hundreds of stage launches) can be captured
    into a HIP graph and replayed on new inputs (BASELINE.json configs[4]: graph-captured decode step)"""
    _, de, _ = helpers.build_nets()
    de = de.to(DEV).eval()
    B, T = 1, 48
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    stats = synth.make_stats()
    clip = synth.make_clip(T, seed=811, stats=stats)
    tt = lambda k: g(torch.as_tensor(clip[k][None]))  # noqa: E731
    pose0 = _pack_pose(tt("Y_root_vel"), tt("Y_root_vrt"), tt("Y_lpos"), tt("Y_ltxy"), tt("Y_lvel"), tt("Y_lvrt"))[:, 0].contiguous()
    rp0, rr0, gaze = tt("Y_root_pos")[:, 0].contiguous(), tt("Y_root_rot")[:, 0].contiguous(), tt("Y_gaze_pos")
    torch.manual_seed(12)
    speech, style = torch.randn(B, T, 64, device=DEV) * 0.5, torch.randn(B, T, 64, device=DEV) * 0.5
    run = lambda: ops.decoder_core(de, pose0, rp0, rr0, gaze, speech, style, s["in_mean"], s["in_std"], s["out_mean"],  # noqa: E731
                                   s["out_std"], synth.DT)
    with torch.no_grad():
        ref1 = [t.clone() for t in run()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()                                      # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, ref1):
            assert float((a - b).abs().max()) < 1e-6
        speech.copy_(torch.randn(B, T, 64, device=DEV) * 0.5)      # new input in the captured buffers
        graph.replay()
        torch.cuda.synchronize()
        ref2 = run()
        for a, b in zip(out, ref2):
            assert float((a - b).abs().max()) < 1e-6
        assert float((ref2[0] - ref1[0]).abs().max()) > 1e-3       # the replay really consumed the new speech


def test_decoder_training_step_is_graph_capturable():
    """forward rollout + BPTT of the decoder (both persistent sweeps, validated by a warm-up) captured into ONE HIP graph and
    replayed on new inputs: same gradients as the eager call"""
    _, de, _ = helpers.build_nets()
    de = de.to(DEV).train()
    B, T = 4, 7
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    stats = synth.make_stats()
    clips = [synth.make_clip(T, seed=820 + b, stats=stats) for b in range(B)]
    tt = lambda k: g(torch.as_tensor(np.stack([c[k] for c in clips])))  # noqa: E731
    pose0 = _pack_pose(tt("Y_root_vel"), tt("Y_root_vrt"), tt("Y_lpos"), tt("Y_ltxy"), tt("Y_lvel"), tt("Y_lvrt"))[:, 0].contiguous()
    rp0, rr0, gaze = tt("Y_root_pos")[:, 0].contiguous(), tt("Y_root_rot")[:, 0].contiguous(), tt("Y_gaze_pos")
    torch.manual_seed(13)
    speech = (torch.randn(B, T, 64, device=DEV) * 0.5).requires_grad_(True)
    style = torch.randn(B, T, 64, device=DEV) * 0.5
    wgt = torch.randn(B, T, synth.POSE_OUT, device=DEV)

    def step():
        de.zero_grad(set_to_none=False)
        if speech.grad is not None:
            speech.grad.zero_()
        pose, rp, rr = ops.decoder_core(de, pose0, rp0, rr0, gaze, speech, style, s["in_mean"], s["in_std"], s["out_mean"],
                                        s["out_std"], synth.DT)
        ((pose * wgt).sum() + rp.sum() + rr.sum()).backward()

    step()                                              # eager: validates the persistent kernels on this process
    torch.cuda.synchronize()
    assert ops.lib().zeggs_persistent_state(1) == 1 and ops.lib().zeggs_persistent_state(2) == 1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    with torch.no_grad():
        speech.copy_(torch.randn(B, T, 64, device=DEV) * 0.5)          # new input in the captured buffers
    graph.replay()
    torch.cuda.synchronize()
    got = (speech.grad.clone(), de.recurrent_decoder.layer1.weight_hh_l0.grad.clone(), de.recurrent_decoder.layer2.weight.grad.clone())
    step()                                              # eager on the same input
    torch.cuda.synchronize()
    ref = (speech.grad, de.recurrent_decoder.layer1.weight_hh_l0.grad, de.recurrent_decoder.layer2.weight.grad)
    for a, b in zip(got, ref):
        assert float(b.abs().max()) > 0 and relerr(a, b) < 2e-5


# ----------------------------------------------------------------------------- loud failures
def test_c_abi_rejects_bad_arguments_loudly():
    """error behaviour of the boundary: -1 + zeggs_last_error(), never a silent fallback"""
    import ctypes as C
    L = ops.lib()
    dev_buf = torch.zeros(1 << 16, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # decoder: pose_input_size must be pose_output_size + 3, batch / sequence must be non-empty, workspace must fit
    P, S = ops.DecPtrs(), ops.DecStats()
    for dims, msg in ((ops.DecDims(2, 4, 100, 90, 8, 8, 64, 0.016, 0), "pose_input_size"),
                      (ops.DecDims(0, 4, 93, 90, 8, 8, 64, 0.016, 0), "empty"),
                      (ops.DecDims(2, 4, 93, 90, 8, 8, 64, 0.016, 0), "workspace too small")):
        rc = L.zeggs_decoder_fwd(C.byref(dims), C.byref(P), C.byref(S), p(dev_buf), p(dev_buf), p(dev_buf), p(dev_buf),
                                 p(dev_buf), p(dev_buf), p(dev_buf), p(dev_buf), p(dev_buf), 0, p(dev_buf), C.c_size_t(16),
                                 stream)
        assert rc == -1 and msg in L.zeggs_last_error().decode(), (msg, L.zeggs_last_error())
    # loss: at most 256 joints, a non-empty batch, the workspace zeggs_loss_workspace_bytes states -- refused before any launch
    for (B, T, J), short, msg in (((2, 4, 257), 0, "more than 256 joints"), ((0, 4, 75), 0, "bad dims"),
                                  ((2, 4, 75), 1, "workspace too small")):
        ld = ops.LossDims(B, T, J, 64, 0.016)
        need = L.zeggs_loss_workspace_bytes(C.byref(ld))
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        big = torch.zeros(max(1, B) * T * (6 + 15 * J), device=DEV)
        par = torch.zeros(J, dtype=torch.int32, device=DEV)
        rc = L.zeggs_loss_fwd_bwd(C.byref(ld), p(par), p(big), p(big), p(big), p(big), p(big), p(big), p(big), p(big), p(big),
                                  C.c_float(0.1), p(big), p(big), p(big), p(big), p(big), p(big), C.c_float(1.0), p(ws),
                                  C.c_size_t(need - short), stream)
        assert rc == -1 and msg in L.zeggs_last_error().decode(), (msg, L.zeggs_last_error())
        if not short:
            continue
        rc = L.zeggs_loss_prepare_truth(C.byref(ld), p(par), p(big), p(big), p(big), p(big), p(ws), C.c_size_t(need - short), stream)
        assert rc == -1 and msg in L.zeggs_last_error().decode(), (msg, L.zeggs_last_error())
    # unknown option, bad mel dims, streaming range ahead of the received samples
    assert L.zeggs_set_option(b"no_such_option", 1) == -1 and b"unknown option" in L.zeggs_last_error()
    from zeggs import audio
    d = audio.MelDims(800, 200, 80, 16000, 60.0, 1e-5, 0.0, 0)
    rc = L.zeggs_mel_features_range(C.byref(d), p(dev_buf), C.c_long(3000), 0, p(dev_buf), C.c_long(0), C.c_long(50),
                                    p(dev_buf), p(dev_buf), C.c_size_t(1 << 18), stream)
    assert rc == -1 and b"not received yet" in L.zeggs_last_error()
    # product path without a GPU tensor
    with pytest.raises(RuntimeError, match="not on a GPU"):
        ops.normalize_rows_(torch.zeros(4, 4), torch.zeros(4), torch.ones(4))


def test_streaming_with_film_decoder_matches_offline():
    """the chunked decode entry point resumes the generic per-step path (rnn_cond="film") as well"""
    from zeggs import anim, audio, modules, stream
    se, _, _ = helpers.build_nets()
    torch.manual_seed(4321)
    de = modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, 64, 1024, 2, rnn_cond="film")
    se, de = se.to(DEV).eval(), de.to(DEV).eval()
    stats = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32, device=DEV) for k, v in synth.make_stats().items()}
    conf = dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True, normalize_mel_bins=True,
                normalize_range=True, min_clipping=1e-5, sampling_rate=16000, mel_fmin=20, mel_fmax=7600,
                n_mel_channels=80, filter_length=800, hop_length=200, resample_method="linear", normalize_loudness=False)
    wav = synth.synth_wav(20000, seed=2).astype(np.float32) / 32768.0
    first = anim.preprocess_animation(synth.make_bvh_clip(8, seed=3), DEV)
    style = torch.randn(1, 64, device=DEV) * 0.5
    n_frames = audio.n_anim_frames(len(wav))
    feats = torch.as_tensor(audio.preprocess_audio(wav, 60, n_frames, conf, ["mel_spec", "energy"]), device=DEV)
    with torch.no_grad():
        sp = se(((feats[None] - stats["audio_input_mean"]) / stats["audio_input_std"]).contiguous())
        f32 = lambda a: a[0:1].to(torch.float32).contiguous()  # noqa: E731
        rp, rr, rv, rw, lp, _, lt, lv, lw = first[:9]
        pose0 = torch.cat([f32(x).reshape(1, -1) for x in (rv, rw, lp, lt, lv, lw)], dim=1)
        ref = ops.decoder_core(de, pose0, f32(rp), f32(rr), f32(first[14]).repeat(n_frames, 1)[None].contiguous(), sp,
                               style.repeat(n_frames, 1)[None].contiguous(), stats["anim_input_mean"],
                               stats["anim_input_std"], stats["anim_output_mean"], stats["anim_output_std"], synth.DT)
    gs = stream.GestureStream(se, de, first, style, stats, conf, synth.DT)
    outs = [gs.push(wav[:7000]), gs.push(wav[7000:15000]), gs.push(wav[15000:]), gs.finish()]
    pose = torch.cat([o["pose"] for o in outs if o], dim=0)
    assert pose.shape[0] == n_frames and float((pose - ref[0][0]).abs().max()) < 5e-5


def test_cli_train_then_generate_end_to_end(tmp_path):
    """`python -m zeggs.cli train -o ...` then `generate -o <run>/options.json ...` (the reference's main.py / generate.py command
    lines) on a tiny synthetic data set: a run directory in the reference's layout, then a BVH + WAV pair from its checkpoints."""
    import json
    import scipy.io.wavfile as wavfile
    from zeggs import anim, cli
    synth.write_dataset(tmp_path / "data" / "processed_v1", n_train=2, n_valid=1, nframes=40, seed=3)
    conf = dict(audio_conf=dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True,
                                normalize_mel_bins=True, normalize_range=True, min_clipping=1e-5, sampling_rate=16000,
                                mel_fmin=20, mel_fmax=7600, n_mel_channels=80, filter_length=800, hop_length=200,
                                resample_method="linear", normalize_loudness=False),
                audio_feature_type=["mel_spec", "energy"])
    json.dump(conf, open(tmp_path / "data" / "processed_v1" / "data_pipeline_conf.json", "w"))
    options = {"paths": {"base_path": str(tmp_path), "path_processed_data": "data/processed_v1", "output_dir": None,
                         "models_dir": None},
               "net_opt": {"decoder": {"nhidden": 1024, "num_rnn_layers": 2, "rnn_cond": "normal"},
                           "speech_encoder": {"nhidden": 64, "speech_encoding_size": 64},
                           "style_encoder": {"nhidden": 512, "style_encoding_size": 64, "example_length": 16, "type": "attn",
                                             "use_vae": True}},
               "train_opt": dict(niterations=0.002, batchsize=4, window=8, change_pace=True, learning_rate=1e-4,
                                 learning_rate_decay=0.995, eps=1e-5, resume=False, use_gpu=True, thread_count=1, seed=1234,
                                 use_tensorboard=False, style_encoding_type="example", generate_samples_step=1000, use_script=False)}
    json.dump(options, open(tmp_path / "options.json", "w"))
    assert cli.main(["train", "-o", str(tmp_path / "options.json"), "-n", "tiny"]) == 0
    runs = list((tmp_path / "outputs").iterdir())
    assert len(runs) == 1 and (runs[0] / "saved_models" / "decoder.pt").exists() and (runs[0] / "logs").is_dir()
    assert json.load(open(runs[0] / "options.json"))["name"] == "tiny"
    anim.bvh_save(tmp_path / "ex.bvh", synth.make_bvh_clip(48, seed=5))
    wavfile.write(tmp_path / "a.wav", 16000, synth.synth_wav(16000, seed=2))
    assert cli.main(["generate", "-o", str(runs[0] / "options.json"), "-s", str(tmp_path / "ex.bvh"), "-a", str(tmp_path / "a.wav"),
                     "-n", "clip", "-fp", str(tmp_path / "ex.bvh"), "-t", "0.5", "-r", "3", "-f", "4", "40", "-g"]) == 0
    out = anim.bvh_load(runs[0] / "results" / "clip.bvh")
    assert out["rotations"].shape[1:] == (75, 3) and out["rotations"].shape[0] >= 50 and np.isfinite(out["rotations"]).all()
    assert (runs[0] / "results" / "clip.wav").exists()
