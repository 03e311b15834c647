"""Shared test helpers: seeded nets (reference construction order) and golden loading."""
import math

import numpy as np
import torch

from zeggs import modules, synth

SEED = 1234


def build_nets(style_size=64, use_vae=True, seed=SEED):
    """torch.manual_seed(seed); SpeechEncoder, Decoder, StyleEncoder -- the
    reference's construction order (train.py:118-139), so weights are
    bit-identical to the reference's random init."""
    torch.manual_seed(seed)
    se = modules.SpeechEncoder(synth.N_AUDIO, 64, 64)
    de = modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, style_size, 1024, 2)
    st = modules.StyleEncoder(synth.POSE_IN, 512, 64, type="attn", use_vae=use_vae)
    return se, de, st


def fingerprint(t):
    a = t.detach().double().flatten()
    return np.array([float(a.sum()), float(a.abs().sum())])


def sample_idx(numel):
    return np.unique((np.arange(97, dtype=np.int64) * 7919 + 13) % numel)


def sd(module, dtype=None):
    return {k: (v.detach().to(dtype) if dtype else v.detach()) for k, v in module.state_dict().items()}


def stats_tensors(dtype=torch.float32, device="cpu"):
    s = synth.make_stats()
    t = lambda k: torch.as_tensor(np.asarray(s[k]), dtype=dtype, device=device)  # noqa: E731
    return dict(a_mean=t("audio_input_mean"), a_std=t("audio_input_std"), in_mean=t("anim_input_mean"),
                in_std=t("anim_input_std"), out_mean=t("anim_output_mean"), out_std=t("anim_output_std"))


# ----------------------------------------------------------------------------- full-shape fixtures (oracle/make_golden_full.py)
GOLDEN = __import__("pathlib").Path(__file__).resolve().parent / "golden"
STAT_KEYS = ("audio_input_mean", "audio_input_std", "anim_input_mean", "anim_input_std", "anim_output_mean",
             "anim_output_std")


def real_stats(v="v1"):
    """The reference's own normalisation statistics (data/processed_v*/stats.npz), stored as a fixture."""
    s = np.load(GOLDEN / f"real_stats_{v}.npz")
    return {k: np.asarray(s[k]) for k in STAT_KEYS}


def real_stats_tensors(v="v1", dtype=torch.float32, device="cpu"):
    s = real_stats(v)
    t = lambda k: torch.as_tensor(np.asarray(s[k]), dtype=dtype, device=device)  # noqa: E731
    return dict(a_mean=t("audio_input_mean"), a_std=t("audio_input_std"), in_mean=t("anim_input_mean"),
                in_std=t("anim_input_std"), out_mean=t("anim_output_mean"), out_std=t("anim_output_std"))


def checksum(a):
    a = np.asarray(a, np.float64).ravel()
    return np.array([a.sum(), np.abs(a).sum()])


def full_decoder_inputs(st, B, T, seed):
    """The seeded decoder inputs of oracle/make_golden_full.py:decoder_inputs (same generator, same seeds)."""
    clips = [synth.make_clip_stats(T, seed=seed + b, stats=st) for b in range(B)]
    W = {k: torch.as_tensor(np.stack([c[k] for c in clips])) for k in clips[0]}
    rng = np.random.default_rng(seed + 7)
    speech = torch.as_tensor(rng.standard_normal((B, T, 64)).astype(np.float32) * 0.5)
    style = torch.as_tensor(np.repeat(rng.standard_normal((B, 1, 64)).astype(np.float32) * 0.5, T, axis=1))
    return W, speech, style


def assert_inputs_match(gd, W, speech, style):
    got = np.stack([checksum(W[k]) for k in sorted(W)] + [checksum(speech), checksum(style)])
    np.testing.assert_allclose(got, gd["in_check"], rtol=1e-9, err_msg="synthetic input generator drifted")


def pack_pose(vel, vrt, lpos, ltxy, lvel, lvrt):
    B, T = vel.shape[:2]
    return torch.cat([vel.reshape(B, T, -1), vrt.reshape(B, T, -1), lpos.reshape(B, T, -1), ltxy.reshape(B, T, -1),
                      lvel.reshape(B, T, -1), lvrt.reshape(B, T, -1)], dim=-1)


def full_dataset(gd, v):
    """The synthetic processed_data (dict) that oracle/make_golden_full.py:record_train_iteration trained on."""
    st = real_stats(v)
    return synth.make_processed(int(gd["n_train"]), 1, int(gd["nframes"]), int(gd["data_seed"]), int(gd["nlabels"]), st,
                                synth.make_clip_stats)


def long_decoder_inputs(st, T, seed):
    """The B=1 inputs of oracle/make_golden_full.py:long_decoder_inputs (a T-frame free-running decode: only the first
    pose, the gaze target and the speech / style encodings exist)."""
    c = synth.make_clip_stats(8, seed=seed, stats=st)
    W = {k: torch.as_tensor(v[None, :1]) for k, v in c.items() if k != "Y_gaze_pos"}
    rng = np.random.default_rng(seed + 7)
    gaze = np.array([[10.0, 150.0, 100.0]]) + synth._smooth(rng, T, 3, 2.0, k=241)
    W["Y_gaze_pos"] = torch.as_tensor(gaze[None].astype(np.float32))
    env = 0.5 + 0.25 * synth._smooth(rng, T, 1, 1.0, k=121)
    speech = torch.as_tensor((rng.standard_normal((1, T, 64)) * env[None]).astype(np.float32))
    style = torch.as_tensor(np.repeat(rng.standard_normal((1, 1, 64)).astype(np.float32) * 0.5, T, axis=1))
    return W, speech, style


def exemplar_rows(st, L, seed):
    """[L, 1134] un-normalised style-exemplar rows of a seeded clip (gaze slot zero, dataset.py:194)."""
    c = synth.make_clip_stats(L, seed=seed, stats=st)
    return np.concatenate([c["Y_root_vel"], c["Y_root_vrt"], c["Y_lpos"].reshape(L, -1), c["Y_ltxy"].reshape(L, -1),
                           c["Y_lvel"].reshape(L, -1), c["Y_lvrt"].reshape(L, -1), np.zeros((L, 3), np.float32)], axis=1)


def variants_batch_inputs(gd):
    """Inputs of tests/golden/variants_batch.npz that the fixture does not store (oracle/make_golden.py gold_variants_batch):
    first pose, gaze targets and exemplar rebuilt from the same deterministic synth clips, checked against the stored checksums;
    the weights of the differentiated scalar from the stored seed."""
    T, L = (int(v) for v in gd["clip_T_L"])
    B = gd["in_speech"].shape[0]
    stats = synth.make_stats()
    clips = [synth.make_clip(T + L, seed=170 + b, stats=stats) for b in range(B)]
    W = {k: torch.as_tensor(np.stack([c[k][:T] for c in clips])) for k in clips[0]}
    ex = []
    for c in clips:
        ex.append(np.concatenate([c["Y_root_vel"][T:T + L], c["Y_root_vrt"][T:T + L],
                                  c["Y_lpos"][T:T + L].reshape(L, -1), c["Y_ltxy"][T:T + L].reshape(L, -1),
                                  c["Y_lvel"][T:T + L].reshape(L, -1), c["Y_lvrt"][T:T + L].reshape(L, -1),
                                  np.zeros((L, 3), np.float32)], axis=1))
    example = torch.as_tensor(np.stack(ex))
    np.testing.assert_allclose(fingerprint(example), gd["sum_example"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(fingerprint(W["Y_gaze_pos"]), gd["sum_gaze"], rtol=1e-12, atol=0)
    first = [W[k][:, 0] for k in ("Y_root_pos", "Y_root_rot", "Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt")]
    names = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "ltxy", "lvel", "lvrt")
    gen = torch.Generator().manual_seed(int(gd["weight_seed"]))
    wts = [torch.randn(tuple(gd["O_" + n].shape), generator=gen) for n in names]
    wz, wm, wl = (torch.randn(B, 64, generator=gen) for _ in range(3))
    return first, W["Y_gaze_pos"], example, wts, (wz, wm, wl)


def assert_grad_samples(gd, tag, named_grads, tol):
    """parameter gradients against the reference's stored samples: |g - g_ref| <= tol * max |g_ref| at the sampled indices"""
    for k, gr in named_grads:
        idx = torch.as_tensor(gd[f"gidx_{tag}.{k}"])
        ref = torch.as_tensor(gd[f"gsamp_{tag}.{k}"]).double()
        got = gr.detach().cpu().flatten()[idx].double()
        scale = max(float(gd[f"gmax_{tag}.{k}"]), 1e-12)
        err = float((got - ref).abs().max()) / scale
        assert err < tol, (tag, k, err)


def width512_inputs(gd):
    """inputs of tests/golden/width512.npz (oracle/make_golden.py gold_width512) rebuilt from the deterministic synth clips"""
    T = int(gd["clip_T"])
    B = gd["in_speech"].shape[0]
    stats = synth.make_stats()
    clips = [synth.make_clip(T, seed=270 + b, stats=stats) for b in range(B)]
    W = {k: torch.as_tensor(np.stack([c[k][:T] for c in clips])) for k in clips[0]}
    np.testing.assert_allclose(fingerprint(W["Y_gaze_pos"]), gd["sum_gaze"], rtol=1e-12, atol=0)
    first = [W[k][:, 0] for k in ("Y_root_pos", "Y_root_rot", "Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt")]
    names = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "ltxy", "lvel", "lvrt")
    gen = torch.Generator().manual_seed(int(gd["weight_seed"]))
    wts = [torch.randn(tuple(gd["O_" + n].shape), generator=gen) for n in names]
    return first, W["Y_gaze_pos"], wts


# ----------------------------------------------------------------------------- iteration 1 of train_iter.npz (round 5)
POSE_SPLIT = (3, 3, 225, 450, 225, 225)       # root_vel, root_vrt, lpos, ltxy, lvel, lvrt in the packed pose row


def unpack_pose(pose):
    """[B, T, 1131] packed decoder output -> (root_vel, root_vrt, lpos, ltxy, lvel, lvrt) in the reference's shapes."""
    B, T = pose.shape[:2]
    vel, vrt, lpos, ltxy, lvel, lvrt = torch.split(pose, POSE_SPLIT, dim=-1)
    return vel, vrt, lpos.reshape(B, T, 75, 3), ltxy.reshape(B, T, 75, 2, 3), lvel.reshape(B, T, 75, 3), lvrt.reshape(B, T, 75, 3)


def grads_at_forward_point(g, it, state_dicts, O_point, kl_iteration=None):
    """The float64 arbiter for an iteration whose loss gradient is ill-conditioned in the FORWARD POINT (train_iter.npz,
    iteration 1: one root joint's predicted x / y axes are 0.86 degrees from antiparallel, so d loss / d output ~ 1 / |x cross y| and
    an output deviation of 5e-6 -- float32 forward rounding -- moves the length of the WHOLE gradient by 0.5 %: measured on the
    reference itself, oracle/make_golden.py: gold_train_iter_perturb and DESIGN.md section 4).  An fp32 implementation cannot be
    held to the fp64 gradient at the fp64 forward point closer than the reference's own fp32 run is; it CAN be held to

        G* = J64(theta)^T . grad_O loss64(O_point)          (+ the KL path through mu, logvar)

    i.e. the float64 network Jacobian applied to the float64 loss gradient evaluated AT THE IMPLEMENTATION'S OWN OUTPUTS O_point.
    state_dicts: (speech, decoder, style) float32 state dicts = the weights the implementation ran the iteration with;
    O_point: its 8 decoder outputs (root_pos, root_rot, root_vel, root_vrt, lpos, ltxy, lvel, lvrt), any float dtype.
    Returns (list of float64 gradient tensors in the reference optimizer's parameter order, float64 outputs of the oracle,
    float64 loss gradient w.r.t. the outputs at O_point)."""
    from oracle import loss as oloss
    from oracle import nets as onets
    from zeggs import synth
    dt = torch.float64
    s = {k: v.to(dt) for k, v in stats_tensors().items()}
    ws = [{k: v.detach().cpu().to(dt).clone().requires_grad_(True) for k, v in w.items()} for w in state_dicts]
    b = [torch.as_tensor(g[f"it{it}_batch{j}"]).to(dt) for j in range(11)]
    audio, rpos, rrot, rvel, rvrt, lpos, ltxy, lvel, lvrt, gaze, wstyle = b
    speech = onets.speech_encoder(ws[0], (audio - s["a_mean"]) / s["a_std"])
    z, mu, logvar = onets.style_encoder(ws[2], (wstyle - s["in_mean"]) / s["in_std"], torch.as_tensor(g[f"it{it}_eps"]).to(dt))
    T = audio.shape[1]
    O64 = onets.decoder_rollout(ws[1], rpos[:, 0], rrot[:, 0], rvel[:, 0], rvrt[:, 0], lpos[:, 0], ltxy[:, 0], lvel[:, 0],
                                lvrt[:, 0], gaze, speech, z.unsqueeze(1).repeat(1, T, 1), s["in_mean"], s["in_std"],
                                s["out_mean"], s["out_std"], synth.DT)
    Oe = [o.detach().cpu().to(dt).reshape(r.shape).clone().requires_grad_(True) for o, r in zip(O_point, O64)]
    loss_e, _ = oloss.training_loss(Oe, (rpos, rrot, rvel, rvrt, lpos, ltxy, lvel, lvrt), gaze, synth.PARENTS, synth.DT, mu,
                                    logvar, iteration=it if kl_iteration is None else kl_iteration)
    g_e = torch.autograd.grad(loss_e, Oe, retain_graph=True)
    (loss_e + sum((o * ge.detach()).sum() for o, ge in zip(O64, g_e))).backward()
    grads = [v.grad if v.grad is not None else torch.zeros_like(v) for w in (ws[0], ws[1], ws[2]) for v in w.values()]
    return grads, [o.detach() for o in O64], [x.detach() for x in g_e]


# ----------------------------------------------------------------------------- training mode: dropout masks and VAE noise
# Mask contract (include/zeggs_hip.h, beside zeggs_dropout): a site's mask is a pure function of (seed + offset, element index);
# element index = position in the contiguous [B * T, C] / [B * L, C] activation, attention ((b * NH + h) * L + q) * L + k;
# offsets: speech encoder +1, +2 (after each ELU), style encoder +1 ... +5 (both conv-stack LayerNorms, attention
# probabilities, attention output, feed-forward output).  zeggs_dropout(ones, n, p, seed) therefore returns the keep-scale.
def relerr(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / max(1e-12, float(ref.abs().max())))


def oracle_iteration_core(ws, audio_n, target, gaze, example_n, eps, it, masks=None):
    """Loss + gradients of one training iteration computed by the oracle.  ws: the three state dicts (speech, decoder, style)
    with requires_grad set; audio_n / example_n: normalised inputs; target: the 8 ground-truth tensors (root_pos, root_rot,
    root_vel, root_vrt, lpos, ltxy, lvel, lvrt); masks: None (eval-mode encoders) or the 7 keep-scales, speech sites first."""
    from oracle import loss as oloss
    from oracle import nets as onets
    dtype = audio_n.dtype
    s = {k: v.to(dtype) for k, v in stats_tensors().items()}
    speech = onets.speech_encoder(ws[0], audio_n, masks=None if masks is None else masks[:2])
    z, mu, logvar = onets.style_encoder(ws[2], example_n, eps, masks=None if masks is None else masks[2:])
    T = audio_n.shape[1]
    O = onets.decoder_rollout(ws[1], *[t[:, 0] for t in target], gaze, speech, z.unsqueeze(1).repeat(1, T, 1),
                              s["in_mean"], s["in_std"], s["out_mean"], s["out_std"], synth.DT)
    loss, terms = oloss.training_loss(O, tuple(target), gaze, synth.PARENTS, synth.DT, mu, logvar, iteration=it)
    loss.backward()
    return loss, terms, ws


def oracle_iteration(g, it, nets, s, dtype, masks=None):
    """oracle_iteration_core on iteration `it` of a train_iter*.npz record `g` with the weights of `nets`."""
    b = [torch.as_tensor(g[f"it{it}_batch{j}"]).to(dtype) for j in range(11)]
    audio, gaze, wstyle = b[0], b[9], b[10]
    sdd = {k: v.to(dtype) for k, v in s.items()}
    ws = [sd(m, dtype) for m in nets]
    for w in ws:
        for v in w.values():
            v.requires_grad_(True)
    return oracle_iteration_core(ws, (audio - sdd["a_mean"]) / sdd["a_std"], b[1:9], gaze,
                                 (wstyle - sdd["in_mean"]) / sdd["in_std"], torch.as_tensor(g[f"it{it}_eps"]).to(dtype), it,
                                 masks=masks)


def fixture_masks(g, prefix, dtype=torch.float64):
    """the keep-scales a fixture stores bit-packed (oracle/nets.py pack_keeps): speech sites [B, T, C] x 2, then the style
    encoder's five"""
    from oracle import nets as onets
    keeps = onets.unpack_keeps(g[prefix + "mask_bits"], g[prefix + "mask_shapes"], (3, 3, 3, 3, 4, 3, 3))
    return onets.keep_scales(keeps, onets.SPEECH_P + onets.STYLE_P, dtype)


def build_style(H, S, seed=SEED):
    """a seeded attention style encoder (VAE) of hidden width H and encoding size S (E = 2 S)"""
    torch.manual_seed(seed)
    return modules.StyleEncoder(synth.POSE_IN, H, S, type="attn", use_vae=True)


def build_speech(H, O, seed=SEED):
    torch.manual_seed(seed)
    return modules.SpeechEncoder(synth.N_AUDIO, H, O)


def speech_case(B, T, O, seed):
    """seeded inputs of a speech-encoder comparison: x [B, T, F], weights of the differentiated sum"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, synth.N_AUDIO, generator=gen), torch.randn(B, T, O, generator=gen)


def style_case(B, L, S, seed):
    """seeded inputs of a style-encoder comparison: x [B, L, 1134], eps [B, S], weights of z / mu / logvar"""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, L, synth.POSE_IN, generator=gen), torch.randn(B, S, generator=gen),
            [torch.randn(B, S, generator=gen) for _ in range(3)])


def build_style_gru(H, S, seed=SEED):
    """a seeded recurrent style encoder (type "gru", VAE) of hidden width H and encoding size S (projection width 2 S)"""
    torch.manual_seed(seed)
    return modules.StyleEncoder(synth.POSE_IN, H, S, type="gru", use_vae=True)


# The shape matrix of the recurrent style encoder (tests/test_style_gru_oracle_cpu.py pins the oracle at every point,
# tests/test_gpu_style_gru_dims.py runs the device there): (H, S, ((B, L), ...), path).  "fast": the forward-direction recurrence on
# the decoder's stage kernels (csrc/decoder_fast.hip sg_fast_supported: H % 16 == 0, 1 <= B <= 64), "generic": a product plus a gate
# kernel per frame.  Which stage_k instantiation each point launches: the docstring of tests/test_gpu_style_gru_dims.py.
STYLE_GRU_ROWS = (
    (16, 8, ((1, 1), (1, 2), (16, 3), (17, 2)), "fast"),
    (48, 64, ((17, 2), (48, 3)), "fast"),
    (80, 20, ((33, 3), (64, 2)), "fast"),
    (512, 64, ((1, 40), (49, 3), (64, 1), (64, 2)), "fast"),
    (800, 64, ((1, 2), (32, 2), (64, 2)), "fast"),
    (24, 64, ((5, 4),), "generic"),
    (30, 64, ((3, 5),), "generic"),
    (512, 64, ((65, 2),), "generic"),
)
STYLE_GRU_OUT_BOUND, STYLE_GRU_GRAD_BOUND = 5e-5, 3e-4        # tests/test_gpu_parity.py::test_gru_style_encoder_stage_path_batch
STYLE_GRU_TEMPERATURE = 1.0


def style_gru_points():
    """every (H, S, B, L, path) of STYLE_GRU_ROWS"""
    return [(H, S, B, L, path) for H, S, pts, path in STYLE_GRU_ROWS for B, L in pts]


def style_gru_case(H, S, B, L):
    """seeded inputs of one point (style_case: x [B, L, 1134], eps [B, S], weights of z / mu / logvar), seeded by the shape"""
    return style_case(B, L, S, seed=7000 + 131 * H + 17 * B + L)


def f64_weights(module):
    return {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in module.state_dict().items()}


def oracle_speech(module, x, wgt, masks=None):
    """float64 oracle: -> (output, {name: gradient}) of sum(out * wgt)"""
    from oracle import nets as onets
    w = f64_weights(module)
    out = onets.speech_encoder(w, x.double(), masks=masks)
    (out * wgt.double()).sum().backward()
    return out.detach(), {k: v.grad for k, v in w.items()}


def oracle_style(module, x, eps, wts, masks=None, temperature=0.9):
    """float64 oracle: -> ((z, mu, logvar), {name: gradient}) of sum(z wz + mu wm + logvar wl)"""
    from oracle import nets as onets
    w = f64_weights(module)
    outs = onets.style_encoder(w, x.double(), eps.double(), temperature, S=eps.shape[1], masks=masks)
    sum((o * wt.double()).sum() for o, wt in zip(outs, wts)).backward()
    return tuple(o.detach() for o in outs), {k: v.grad for k, v in w.items()}


def worst_relerr(got, ref):
    """largest relerr over a dict of tensors (every parameter in full)"""
    assert set(got) == set(ref)
    return max(relerr(got[k], ref[k]) for k in ref)


def corruptions(masks, ps, seed):
    """The negative controls of one mask set: for every site, (label, masks with that site REDRAWN at the same rate -- what a
    wrong seed offset or a transposed index gives) and (label, masks whose BACKWARD at that site uses the redrawn mask while the
    forward keeps the right one -- a backward that does not regenerate the forward's mask)."""
    from oracle import nets as onets
    other = onets.keep_scales(onets.draw_keeps([tuple(m.shape) for m in masks], ps, seed), ps, masks[0].dtype)
    out = []
    for i in range(len(masks)):
        fwd = list(masks)
        fwd[i] = other[i]
        out.append((f"site {i + 1} redrawn", True, fwd))
        bwd = list(masks)
        bwd[i] = (masks[i], other[i])
        out.append((f"site {i + 1} backward mask differs", False, bwd))
    return out


# ---- the device's own masks, read back through the public ABI
class recorded_seeds:
    """Context manager: wraps ops.next_seed and records (caller, seed) of every draw -- `caller` is the name of the ops function
    that drew ("speech_encoder", "style_encoder_attn", "randn").  Restores ops.next_seed on exit."""

    def __enter__(self):
        import sys
        from zeggs import ops
        self.ops, self.orig, self.draws = ops, ops.next_seed, []

        def next_seed():
            s = self.orig()
            self.draws.append((sys._getframe(1).f_code.co_name, s))
            return s
        ops.next_seed = next_seed
        return self

    def __exit__(self, *exc):
        self.ops.next_seed = self.orig
        return False

    def of(self, caller):
        got = [s for c, s in self.draws if c == caller]
        assert len(got) == 1, (caller, self.draws)
        return got[0]


def _device_keep_scale(shape, p, seed, device="cuda:0"):
    """zeggs_dropout on ones: element i of the contiguous array gets mask(seed, i) / (1 - p)"""
    import ctypes
    from zeggs import ops
    x = torch.ones(*shape, device=device, dtype=torch.float32)
    rc = ops.lib().zeggs_dropout(ctypes.c_void_p(x.data_ptr()), ctypes.c_long(x.numel()), ctypes.c_float(p),
                                 ctypes.c_uint64(int(seed)), ops._stream())
    assert rc == 0, ops.lib().zeggs_last_error().decode()
    torch.cuda.synchronize()
    m = x.cpu().double()
    keep = m != 0
    assert bool(((m - 1.0 / (1.0 - p)).abs() < 1e-6)[keep].all())      # every element is 0 or 1 / (1 - p)
    return keep.double() / (1.0 - p)                                    # the exact float64 scale


def device_masks_speech(seed, B, T, H, O):
    from oracle import nets as onets
    return [_device_keep_scale(sh, p, seed + 1 + i)
            for i, (sh, p) in enumerate(zip(onets.speech_mask_shapes(B, T, H, O), onets.SPEECH_P))]


def device_masks_style(seed, B, L, H, E, NH=4):
    from oracle import nets as onets
    return [_device_keep_scale(sh, p, seed + 1 + i)
            for i, (sh, p) in enumerate(zip(onets.style_mask_shapes(B, L, H, E, NH), onets.STYLE_P))]


def device_eps(seed, B, S, device="cuda:0"):
    from zeggs import ops
    return ops.randn((B, S), device, seed=seed).cpu()


# ---- the training-mode matrix (tests/test_gpu_training_mode.py runs it on the device, tests/test_oracle_golden.py proves on the
# CPU that a mask error at any site of any of these shapes is at least 10x the bounds)
SPEECH_OUT_BOUND, SPEECH_GRAD_BOUND = 1e-5, 2e-4      # tests/test_gpu_parity.py::test_speech_encoder_forward_backward
STYLE_OUT_BOUND, STYLE_GRAD_BOUND = 2e-5, 3e-4        # tests/test_gpu_parity.py::test_style_encoder_forward_backward
ENGINE_GRAD_BOUND = 5e-4                              # tests/test_gpu_parity.py::test_train_iteration_vs_reference, iteration 0
SPEECH_WIDTHS = ((64, 64), (30, 50))                  # (H, O); the second pair: neither width divisible by 4
SPEECH_SHAPES = ((3, 70), (1, 31), (2, 15), (2, 200))     # (B, T); the kernel is 31 wide: T = 31 and 15 are all replicate edge
# (H, E) -> lengths: every pair at one multiple of 32 and one other length, the default widths at all five
STYLE_MATRIX = (((512, 128), (9, 33, 77, 128, 200)), ((200, 256), (77, 128)), ((256, 192), (9, 128)), ((30, 64), (128, 200)),
                ((130, 128), (33, 128)), ((520, 128), (128, 200)), ((64, 520), (9, 128)))
STYLE_REFUSED = ((1030, 128), (9,))                   # forward only: the backward of a row wider than 1024 is refused
ENGINE_CASES = (dict(B=2, window=8, L=16, noise_seed=31, data_seed=41), dict(B=5, window=8, L=33, noise_seed=32, data_seed=42))


def style_batch(H, E, L):
    return 3 if (H, E) == (512, 128) else 2


def engine_case_data(case):
    return synth.make_processed(3, 0, case["window"] + 40, seed=case["data_seed"])


def engine_case_idx(case, n_windows):
    return np.random.default_rng(case["data_seed"]).permutation(n_windows)[:case["B"]]


def host_batch(data, window, idx, ex_len, dtype=torch.float64):
    """The batch of TrainEngine.step(idx, ex_len) rebuilt on the host in `dtype` from the processed data (reference
    dataset.py:98-204: windows, the example's rows with its empty gaze slot, normalisation as train.py:232-250).
    -> audio_n [B, T, F], target (8 tensors), gaze, example_n [B, L, 1134]"""
    from zeggs import engine
    ds = engine.DeviceDataset(data, window, torch.device("cpu"))
    f = lambda k: torch.as_tensor(np.asarray(data[k])).to(dtype)  # noqa: E731
    starts = ds.win_start[idx]
    win = lambda k: torch.stack([f(k)[s:s + window] for s in starts])  # noqa: E731
    audio_n = (win("X_audio_features") - f("audio_input_mean")) / f("audio_input_std")
    target = [win(k) for k in ("Y_root_pos", "Y_root_rot", "Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt")]
    rows = torch.as_tensor(ds.example_rows(idx, ex_len))
    n = len(data["Y_root_pos"])
    pose = torch.cat([f(k).reshape(n, -1) for k in ("Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt")], dim=1)
    ex = torch.cat([pose[rows], torch.zeros(*rows.shape, 3, dtype=dtype)], dim=-1)
    example_n = (ex - f("anim_input_mean")) / f("anim_input_std")
    return audio_n, target, win("Y_gaze_pos"), example_n, ds


# ---- ReLU kinks.  The style encoder has three ReLUs.  A unit whose float64 pre-activation is closer to zero than float32 can
# resolve lands on either side in a float32 implementation (here: by the run-to-run order of the float atomics of the first
# convolutions' split products), and its one-sided derivatives differ by 1: measured at (H, E) = (512, 128), B = 3, L = 33 -- one
# unit of the feed-forward ReLU at 4.2e-7 of the largest pre-activation moved the worst gradient by 1.2e-2 in 3 runs of 10, and
# flipping that one unit in the ORACLE reproduced the device's 20 gradient errors digit for digit.  Both one-sided derivatives are
# gradients of the same function at that point, so the oracle offers both: units with |pre| < KINK * max |pre| of their ReLU (an
# oracle-only criterion) are "near", and the comparison takes the assignment of sides closest to the device's gradients.
# KINK = 2^-20 = 16 units of float32 roundoff: a K-term float32 dot product carries ~ sqrt(K) 2^-24 of its rms (K = 3402 for the
# first convolution: 3.5e-6 of the rms, 5e-7 of the largest entry), doubled for the error of its inputs.
KINK = 2.0 ** -20


class relu_sites:
    """Context manager around an ORACLE evaluation: records the near-kink units of every F.relu call as (call number, flat index);
    the units listed in `flips` get the derivative of the other side (the value, |pre| ~ 0, is left alone)."""

    def __init__(self, flips=()):
        self.flips, self.near, self.n = set(flips), [], 0

    def __enter__(self):
        import torch.nn.functional as F
        self.F, self.orig = F, F.relu
        F.relu = self._relu
        return self

    def __exit__(self, *exc):
        self.F.relu = self.orig
        return False

    def _relu(self, t, *a, **k):
        site, self.n = self.n, self.n + 1
        y = self.orig(t, *a, **k)
        mag = t.detach().abs()
        self.near += [(site, int(j)) for j in (mag < KINK * mag.max()).flatten().nonzero().flatten()]
        for s, j in sorted(self.flips):
            if s == site:
                tj = t.flatten()[j]
                d = 1.0 if float(tj.detach()) <= 0 else -1.0               # derivative 1 instead of 0, or 0 instead of 1
                y = y.flatten().index_add(0, torch.tensor([j]), (d * (tj - tj.detach())).reshape(1)).reshape(t.shape)
        return y


def oracle_at_kinks(run, got):
    """run() -> (outs, {name: gradient}) evaluates a float64 oracle; got: the implementation's gradients.  -> (outs, grads, near,
    flipped): the oracle with, for every near-kink unit in turn, the side that brings it closer to `got` (no near unit: run())."""
    with relu_sites() as rs:
        outs, grads = run()
    near, flips = list(rs.near), set()
    assert len(near) <= 16, f"{len(near)} ReLU units within {KINK:.1e} of their kink"
    best = worst_relerr(got, grads)
    for unit in near:
        with relu_sites(flips | {unit}):
            _, alt = run()
        e = worst_relerr(got, alt)
        if e < best:
            best, grads, flips = e, alt, flips | {unit}
    return outs, grads, near, sorted(flips)


# ----------------------------------------------------------------------------- loss kernels (tests/test_gpu_loss.py)
# Fixtures for ANY parent table, the L1 kinks, and the per-slice gradient comparison.  tests/test_loss_oracle_cpu.py proves on the
# CPU that every case below meets the near-kink condition and that the comparison is sharp (negative controls).
LOSS_GROUPS = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "ltxy", "lvel", "lvrt")
LOSS_TERM_BOUND = dict(rtol=3e-5, atol=1e-7)          # tests/test_gpu_parity.py::test_loss_forward_backward_vs_oracle
LOSS_BOUND, LOSS_GRAD_BOUND, LOSS_KL_BOUND = 3e-5, 3e-4, 1e-5
LOSS_NEAR_MARGIN, LOSS_NEAR_MAX = 16, 16
LOSS_KL_ITERATION = 9000


def _tree40():
    rng = np.random.default_rng(40)
    return [-1] + [int(rng.integers(0, i)) for i in range(1, 40)]


LOSS_SKELETONS = {
    "rig": list(synth.PARENTS),                                     # 75 joints, 13 levels, widths 1 3 3 5 5 5 3 3 5 12 10 10 10
    "j1": [-1],                                                     # one level, no message
    "chain12": [-1] + list(range(11)),                              # every level one joint: seven idle waves at every barrier
    "star16": [-1] + [0] * 16,                                      # a level of exactly LOSS_LW joints: message slots 12-15
    "star17": [-1] + [0] * 17,                                      # wider than LOSS_LW: the table walk, chosen by maxw
    "star20": [-1] + [0] * 20,
    "tree40": _tree40(),                                            # seeded random tree, parents[i] < i
    "j256": [-1] + [0 if k == 0 else 1 + c * 17 + k - 1 for c in range(15) for k in range(17)],   # MAXJ; 17 levels of 15
}
# (skeleton, B, T, root rotations); ids "rig-3x7-general" ...
LOSS_CASES = ([("rig", 3, 7, "yaw")] +
              [("rig", B, T, "general") for B, T in ((3, 7), (2, 8), (1, 4), (1, 12), (2, 2), (10, 7), (5, 28), (3, 1))] +
              [(s, B, T, "general") for s in ("j1", "chain12", "star16", "star17", "star20", "tree40")
               for B, T in ((3, 7), (2, 8), (10, 7))] + [("j256", 2, 4, "general")])
LOSS_MOVED_CASES = [("rig", B, T, "general", grp) for B, T in ((3, 7), (2, 8)) for grp in LOSS_GROUPS]
# the terms a moved group reaches (every other term is exactly 0 when the rest of the prediction IS the ground truth)
LOSS_REACH = dict(root_pos={0, 4, 8, 12, 14, 16}, root_rot={1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16}, root_vel={2, 6, 10},
                  root_vrt={3, 6, 7, 10, 11}, lpos={4, 6, 8, 10, 12, 14}, ltxy={5, 8, 9, 10, 11, 13, 14, 15}, lvel={6, 10},
                  lvrt={7, 10, 11})


def loss_case_id(case):
    return "-".join([case[0], f"{case[1]}x{case[2]}", case[3]] + list(case[4:]))


def loss_case_seed(case):
    """one seed per case (chosen so that at most LOSS_NEAR_MAX elements are near a kink: tests/test_loss_oracle_cpu.py)"""
    s, B, T, root = case[:4]
    return 1000 * sorted(LOSS_SKELETONS).index(s) + 31 * B + T + (500 if root == "yaw" else 0)


def tree_clip(parents, nframes, seed, root="general"):
    """synth.make_clip for an arbitrary parent table: smooth motion of len(parents) joints, float32 arrays under the Y_* keys.
    root = "yaw": rotations (cos, 0, sin, 0) as synth.make_clip; "general": unit quaternions drifting around a random point of the
    sphere, w < 0 for odd seeds."""
    rng = np.random.default_rng(seed)
    J, n, S, DT = len(parents), nframes + 1, synth._smooth, synth.DT
    if root == "yaw":
        yaw = S(rng, n, 1, 0.4)[:, 0]
        root_rot = np.stack([np.cos(yaw / 2), np.zeros(n), np.sin(yaw / 2), np.zeros(n)], axis=1)
    else:
        c = rng.standard_normal(4)
        c[0] = -abs(c[0]) if seed % 2 else abs(c[0])
        q = c / np.linalg.norm(c) + S(rng, n, 4, 0.15)
        root_rot = q / np.linalg.norm(q, axis=1, keepdims=True)
    root_pos = np.cumsum(S(rng, n, 3, 0.5) * DT * 30, axis=0)
    root_vel = S(rng, n, 3, 6.0)
    root_vrt = S(rng, n, 3, 0.2)
    hel = S(rng, n, J * 3, 0.35).reshape(n, J, 3)               # smooth along TIME (angular velocities of a few rad / s)
    lrot = synth._quat_exp(hel / 2.0)
    ex = np.zeros((n, J, 3)); ex[..., 0] = 1.0
    ey = np.zeros((n, J, 3)); ey[..., 1] = 1.0
    ltxy = np.stack([synth._quat_mul_vec(lrot, ex), synth._quat_mul_vec(lrot, ey)], axis=2)
    lpos = rng.normal(0, 8.0, (1, J, 3)) + S(rng, n, J * 3, 0.05).reshape(n, J, 3)
    lvel = (lpos[1:] - lpos[:-1]) / DT
    lvrt = (hel[1:] - hel[:-1]) / DT
    gaze = np.array([[10.0, 150.0, 100.0]]) + rng.normal(0, 1.0, (1, 3)) + S(rng, n, 3, 2.0)
    f, m = np.float32, nframes
    return dict(Y_root_pos=root_pos[:m].astype(f), Y_root_rot=root_rot[:m].astype(f), Y_root_vel=root_vel[:m].astype(f),
                Y_root_vrt=root_vrt[:m].astype(f), Y_lpos=lpos[:m].astype(f), Y_ltxy=ltxy[:m].astype(f), Y_lvel=lvel.astype(f),
                Y_lvrt=lvrt.astype(f), Y_gaze_pos=gaze[:m].astype(f))


def loss_case(case):
    """-> dict(O, W: 8 float32 tensors [B, T, ...] (LOSS_GROUPS order), gaze, mu, logvar, parents, T).  Prediction O = W + 0.3 (O' -
    W) with O' another clip; "general" root rotations: the truth's, perturbed and scaled to norms 0.7 ... 1.3 (the decoder emits
    non-unit quaternions); "yaw": the fixture of test_gpu_parity.py::test_loss_forward_backward_vs_oracle (synth.make_clip).
    A fifth entry of the case names the ONE group that moves: every other group of the prediction is the truth bit for bit."""
    skel, B, T, root = case[:4]
    parents, seed = LOSS_SKELETONS[skel], loss_case_seed(case)
    rng = np.random.default_rng(seed + 7)
    keys = ["Y_" + n for n in LOSS_GROUPS]
    tt = lambda cl, k: torch.as_tensor(np.stack([c[k] for c in cl]))  # noqa: E731
    if root == "yaw":
        assert skel == "rig"
        stats = synth.make_stats()
        Wc = [synth.make_clip(T, seed=90 + b, stats=stats) for b in range(B)]
        Oc = [synth.make_clip(T, seed=190 + b, stats=stats) for b in range(B)]
    else:
        Wc = [tree_clip(parents, T, seed + 3 * b, root) for b in range(B)]            # seeds of both parities: w > 0 and w < 0
        Oc = [tree_clip(parents, T, seed + 100 + 3 * b, root) for b in range(B)]
    W = [tt(Wc, k) for k in keys]
    step = 1.0 if len(case) > 4 else 0.3          # (a group that moves alone moves all the way to the other clip)
    O = [w + step * (o - w) for o, w in zip([tt(Oc, k) for k in keys], W)]
    if root != "yaw":
        q = W[1].double() + 0.1 * torch.as_tensor(rng.standard_normal((B, T, 4)))
        q = q / q.norm(dim=-1, keepdim=True) * torch.as_tensor(rng.uniform(0.7, 1.3, (B, T, 1)))
        O[1] = q.float()
    if len(case) > 4:
        O = [o if n == case[4] else w.clone() for n, o, w in zip(LOSS_GROUPS, O, W)]
    mu = torch.as_tensor(rng.standard_normal((B, 64)), dtype=torch.float32)
    lv = torch.as_tensor(0.3 * rng.standard_normal((B, 64)), dtype=torch.float32)
    return dict(O=O, W=W, gaze=tt(Wc, "Y_gaze_pos"), mu=mu, logvar=lv, parents=parents, T=T)


def unpack_pose_tree(pose, J):
    B, T = pose.shape[:2]
    vel, vrt, lpos, ltxy, lvel, lvrt = torch.split(pose, (3, 3, 3 * J, 6 * J, 3 * J, 3 * J), dim=-1)
    return vel, vrt, lpos.reshape(B, T, J, 3), ltxy.reshape(B, T, J, 2, 3), lvel.reshape(B, T, J, 3), lvrt.reshape(B, T, J, 3)


def loss_slices(grads):
    """8 gradient tensors (LOSS_GROUPS order) -> {slice name: tensor}: the four root groups whole, the joint groups per joint."""
    out = {}
    for n, t in zip(LOSS_GROUPS, grads):
        if n.startswith("root"):
            out[n] = t
        else:
            for j in range(t.shape[2]):
                out[f"{n}[{j}]"] = t[:, :, j]
    return out


def slice_errors(got, ref):
    """per slice: max |got - ref| / max |ref| (each slice against its OWN largest entry); a slice whose reference is exactly zero
    must be exactly zero: its error is 0 or inf"""
    errs = {}
    for k, r in loss_slices(ref).items():
        gk = loss_slices_get(got, k)
        m = float(r.abs().max())
        if m == 0.0:
            errs[k] = 0.0 if float(gk.abs().max()) == 0.0 else float("inf")
        else:
            errs[k] = float((gk.double() - r.double()).abs().max()) / m
    return errs


def loss_slices_get(grads, key):
    n, _, j = key.partition("[")
    t = grads[LOSS_GROUPS.index(n)]
    return t if not j else t[:, :, int(j[:-1])]


def packed_error(got, ref):
    """the OLD view: one max-norm over the packed pose gradient, root_pos, root_rot (test_loss_forward_backward_vs_oracle)"""
    return max(relerr(pack_pose(*got[2:]), pack_pose(*ref[2:])), relerr(got[0], ref[0]), relerr(got[1], ref[1]))


def loss_term_args(data, dtype, bug=None):
    from oracle import loss as oloss
    with torch.no_grad():
        return oloss.term_arguments([o.to(dtype) for o in data["O"]], [w.to(dtype) for w in data["W"]], data["gaze"].to(dtype),
                                    data["parents"], synth.DT, bug=bug)


def loss_near_elements(data, x64=None):
    """L1 kinks.  |x| has two one-sided derivatives at 0: an element of a term's argument whose float64 value is below what float32
    forward kinematics can resolve gets either sign in a float32 implementation, and one flipped sign moves an input gradient by
    2 w / n.  The criterion is a MEASURED envelope taken from the oracle alone: per term and per joint (per term for the root and
    gaze terms) E = max |x32 - x64| over batch, frames and components, x32 / x64 the term arguments of the oracle run in float32 /
    float64 on the same float32 inputs; an element is near iff 0 < |x64| <= LOSS_NEAR_MARGIN E (exact zeros give sign 0 on both
    sides).  -> [(term, flat index)], {term: E}."""
    x32 = loss_term_args(data, torch.float32)
    x64 = loss_term_args(data, torch.float64) if x64 is None else [x.detach() for x in x64]
    near, env = [], {}
    for k, (a, b) in enumerate(zip(x32, x64)):
        if k in (12, 13, 14, 15) and data["T"] == 1:
            continue
        dev = (a.double() - b).abs()
        if 4 <= k <= 15:
            dims = [d for d in range(dev.dim()) if d != 2]
            E = dev.amax(dim=dims, keepdim=True)
        else:
            E = dev.amax().reshape([1] * dev.dim())
        env[k] = float(E.max())
        hit = ((b.abs() > 0) & (b.abs() <= LOSS_NEAR_MARGIN * E)).flatten().nonzero().flatten()
        near += [(k, int(j)) for j in hit]
    return near, env


def loss_oracle(data, dtype=torch.float64, bug=None, sides=None):
    """oracle of one case in `dtype`: -> (loss, terms[18], [the 8 input gradients in LOSS_GROUPS order, dmu, dlogvar]); T = 1: without
    the four finite-difference terms"""
    from oracle import loss as oloss
    O = [o.to(dtype).requires_grad_(True) for o in data["O"]]
    mu, lv = data["mu"].to(dtype).requires_grad_(True), data["logvar"].to(dtype).requires_grad_(True)
    skip = oloss.DIFF_TERMS if data["T"] == 1 else ()
    loss, terms = oloss.training_loss(O, [w.to(dtype) for w in data["W"]], data["gaze"].to(dtype), data["parents"], synth.DT, mu,
                                      lv, iteration=LOSS_KL_ITERATION, sides=sides, skip=skip, bug=bug)
    grads = torch.autograd.grad(loss, O + [mu, lv], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, O + [mu, lv])]
    return loss.detach(), terms, grads


def worst_slice(errs):
    k = max(errs, key=lambda n: errs[n])
    return k, errs[k]


def loss_oracle_at_kinks(data, got):
    """The float64 oracle with, for every near-kink element in turn, the side (-1, 0, +1) that brings its input gradients closest
    to `got` (8 tensors, LOSS_GROUPS order) in the worst slice.  The gradient is linear in the sides -- d loss / d input = base +
    sum over near elements (side - sign) / (18 n_term) d x_e / d input -- so one extra backward per near element is all it takes.
    -> (loss, terms, grads (8 + dmu, dlogvar), near, chosen: [((term, index), oracle's sign, side taken)])"""
    from oracle import loss as oloss
    O = [o.double().requires_grad_(True) for o in data["O"]]
    Wd, gz = [w.double() for w in data["W"]], data["gaze"].double()
    x = oloss.term_arguments(O, Wd, gz, data["parents"], synth.DT)
    near, _ = loss_near_elements(data, x)
    assert len(near) <= LOSS_NEAR_MAX, f"{len(near)} term elements within {LOSS_NEAR_MARGIN} x the float32 envelope of their kink"
    loss, terms, grads = loss_oracle(data)
    base, chosen = [g.clone() for g in grads[:8]], []
    for k, j in near:
        xe = x[k].flatten()[j]
        D = torch.autograd.grad(xe, O, retain_graph=True, allow_unused=True)
        D = [torch.zeros_like(o) if d is None else d / (18.0 * x[k].numel()) for d, o in zip(D, O)]
        s0 = float(torch.sign(xe.detach()))
        best = (worst_slice(slice_errors(got, base))[1], s0, base)
        for s in (-1.0, 0.0, 1.0):
            if s != s0:
                cand = [b + (s - s0) * d for b, d in zip(base, D)]
                e = worst_slice(slice_errors(got, cand))[1]
                if e < best[0]:
                    best = (e, s, cand)
        base = best[2]
        chosen.append(((k, j), s0, best[1]))
    return loss, terms, base + list(grads[8:]), near, chosen


# ----------------------------------------------------------------------------- decoder statistics kinds (tests/test_gpu_decoder_stats.py)
# The four statistics vectors of the decoder are independent arguments (reference Decoder.forward), but synth.make_stats() and both
# recorded stats files have out_mean == in_mean[:PO] exactly, and with them the root's half turn per frame h = dt / 2 |root_vrt|
# stays in [2.8e-3, 6.4e-3]: one of the three branches of every quaternion exponential (dec_math.h) and a zero (mu_o - mu_i) term
# in every fold of the statistics into the weights.  tests/test_decoder_stats_oracle_cpu.py proves on the CPU that every case below
# lies in the branch it is meant for and that the comparison is sharp (negative controls).
DEC_KINDS = ("tied", "untied", "still", "brisk", "spin")
DEC_TURN = dict(still=(0.0, 0.0, 0.0), brisk=(52.0, -83.0, 58.0), spin=(70.0, -110.0, 60.0))      # out_mean[3:6]: |.| = 0, 113.8, 143.5
# the open interval of h = dt / 2 |root_vrt| (frames 1 .. T-1 of the float64 oracle) that a kind must keep at every shape; h is at
# least 2x away from the branch point 1e-5 on either side everywhere (the function is discontinuous there)
DEC_TURN_RANGE = dict(tied=(1e-3, 0.1), untied=(1e-3, 0.1), still=(0.0, 2e-6), brisk=(0.9, 0.995), spin=(1.05, 1.5), zero=(-1.0, 1e-300))
DEC_OUT_BOUND, DEC_GRAD_BOUND = 1e-4, 3e-4            # tests/test_gpu_parity.py::test_decoder_backward_vs_oracle
DEC_SMALL_EPS = 1e-5                                  # reference tquat.py:50-51, 94-99: quat_exp's branch point and quat_normalize's eps
DEC_NAMES = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "ltxy", "lvel", "lvrt")
DEC_KEYS = tuple("Y_" + n for n in DEC_NAMES)
# A slice may have a bound wider than DEC_GRAD_BOUND only if the FLOAT32 ORACLE's own error on it exceeds 3e-5: {slice: 10 x that
# measured error}.  None does (float32 oracle <= 3.4e-7 on every slice, tests/test_decoder_stats_oracle_cpu.py).
DEC_SLICE_BOUNDS = {}


def decoder_stats(kind, dtype=torch.float32, device="cpu"):
    """-> dict(in_mean, in_std, out_mean, out_std) derived from synth.make_stats(); float32 values, cast to `dtype`.
    tied: today's set (out_mean == in_mean[:PO]).  untied: out_mean ~ N(0, 1) from its own generator, out_std[3:6] = (0.8, 1.1,
    0.6); the 40 zero entries of out_std stay -- constant channels whose (mu_o - mu_i) / sigma_i is not zero.  still / brisk / spin:
    untied with out_mean[3:6] = DEC_TURN[kind] (still: out_std[3:6] = 1e-4) -- the small-angle branch, the top of the polynomial
    range, the libm branch.  zero: still with out_std[3:6] = 0, a half turn of exactly 0 (forward only: the reference's own
    gradient is NaN there, 0 * inf behind the sqrt)."""
    s = synth.make_stats()
    im, isd = np.asarray(s["anim_input_mean"], np.float32), np.asarray(s["anim_input_std"], np.float32)
    om, osd = np.asarray(s["anim_output_mean"], np.float32).copy(), np.asarray(s["anim_output_std"], np.float32).copy()
    assert kind in DEC_KINDS + ("zero",), kind
    if kind != "tied":
        assert int((osd == 0).sum()) == 40 and not bool((osd[:6] == 0).any())
        om = np.random.default_rng(2024).standard_normal(synth.POSE_OUT).astype(np.float32)
        osd[3:6] = (0.8, 1.1, 0.6)
        if kind in ("still", "zero"):
            om[3:6], osd[3:6] = 0.0, (1e-4 if kind == "still" else 0.0)
        elif kind != "untied":
            om[3:6] = DEC_TURN[kind]
    t = lambda a: torch.as_tensor(a).to(dtype).to(device)  # noqa: E731
    return dict(in_mean=t(im), in_std=t(isd), out_mean=t(om), out_std=t(osd))


_DEC_NETS, _DEC_CASES = {}, {}


def decoder_net(tag):
    """(cached; callers move a deepcopy to the device) the seeded decoders of the statistics tests: "main" (build_nets), "film" (rnn_cond="film", the construction of
    test_gpu_parity._variant_nets), "h512" (nhidden = 512); the tags of DEC_DIM_NETS: decoders at other dimensions (below)"""
    if tag not in _DEC_NETS:
        if tag == "main":
            _DEC_NETS[tag] = build_nets()[1]
        elif tag in DEC_DIM_NETS:
            _DEC_NETS[tag] = _decoder_dim_net(tag)
        else:
            assert tag in ("film", "h512"), tag
            torch.manual_seed(4321 if tag == "film" else 77)
            _DEC_NETS[tag] = (modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, 64, 1024, 2, rnn_cond="film") if tag == "film"
                              else modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, 64, 512, 2))
    return _DEC_NETS[tag]


def decoder_case(B, T):
    """float32 inputs of a [B, T] rollout: clips of synth.make_clip, speech / style seeded as test_gpu_parity._oracle_vs_hip_rollout
    -> dict(fp: the 8 first-pose tensors (DEC_NAMES order), gaze [B, T, 3], speech, style [B, T, 64]); cached, read-only"""
    if (B, T) in _DEC_CASES:
        return _DEC_CASES[(B, T)]
    stats = synth.make_stats()
    clips = [synth.make_clip(max(T, 4), seed=700 + b, stats=stats) for b in range(B)]
    tt = lambda k: torch.as_tensor(np.stack([c[k][:T] for c in clips]))  # noqa: E731
    gen = torch.Generator().manual_seed(4)
    speech, style = torch.randn(B, T, 64, generator=gen) * 0.5, torch.randn(B, T, 64, generator=gen) * 0.5
    _DEC_CASES[(B, T)] = dict(fp=[tt(k)[:, 0] for k in DEC_KEYS], gaze=tt("Y_gaze_pos"), speech=speech, style=style, B=B, T=T)
    return _DEC_CASES[(B, T)]


def decoder_weighting(name, B, T, J=synth.NJ):
    """weights of the differentiated sum over the 8 outputs.  "all": seeded normal weights on everything; "root": on root_pos and
    root_rot of the LAST frame only -- every gradient then arrives through the root adjoint carried over T - 1 steps and through the
    gaze direction."""
    shapes = [(B, T, 3), (B, T, 4), (B, T, 3), (B, T, 3), (B, T, J, 3), (B, T, J, 2, 3), (B, T, J, 3), (B, T, J, 3)]
    gen = torch.Generator().manual_seed(11)
    wts = [torch.randn(*sh, generator=gen) for sh in shapes]
    if name == "root":
        for i, w in enumerate(wts):
            if i >= 2:
                w.zero_()
            else:
                w[:, :-1] = 0.0
    else:
        assert name == "all", name
    return wts


class oracle_bug:
    """Context manager around an ORACLE evaluation: one of the bug models of the negative controls.
    "eps0": quat_exp(x, eps=0) in the root integration -- the polynomial / libm formula where the small branch is due;
    "gaze_detached": the gaze direction's gradient to root_pos / root_rot cut (detach inside vectorize_input);
    ("stale_fold", stats A): the pose fed back to the next step is de-normalised with the out_mean / out_std of A while the outputs
    use the call's own -- what a fold of A into the weight packs gives under a call with other statistics."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        from oracle import nets as onets
        self.onets, self.saved = onets, (onets.quat_from_helical, onets.vectorize_input, onets.devectorize_output)
        qfh, vec, dev = self.saved
        model = self.model
        if model == "eps0":
            onets.quat_from_helical = lambda x, eps=0.0: onets.quat_exp(x / 2.0, 0.0)
        elif model == "gaze_detached":
            onets.vectorize_input = lambda rp, rr, *rest: vec(rp.detach(), rr.detach(), *rest)
        elif isinstance(model, tuple) and model[0] == "stale_fold":
            A, last = model[1], [None]

            def dev_(pred, *a):
                last[0] = pred
                return dev(pred, *a)

            def vec_(*a):
                v = vec(*a)
                if last[0] is None:
                    return v
                im, isd = a[-2], a[-1]
                PO = last[0].shape[1]
                fb = (last[0] * A["out_std"].to(v.dtype) + A["out_mean"].to(v.dtype) - im[:PO]) / isd[:PO]
                return torch.cat([fb, v[:, PO:]], dim=1)
            onets.devectorize_output, onets.vectorize_input = dev_, vec_
        elif model is not None:
            raise ValueError(model)
        return self

    def __exit__(self, *exc):
        self.onets.quat_from_helical, self.onets.vectorize_input, self.onets.devectorize_output = self.saved
        return False


def decoder_oracle(de, case, stats, wts=None, dtype=torch.float64, bug=None):
    """oracle.nets.decoder_rollout of one case in `dtype` -> (8 outputs, {name: gradient} or None).  Gradients (wts given) of
    sum(out * wts) w.r.t. every parameter, "speech" and "style"."""
    from oracle import nets as onets
    w = {k: v.detach().cpu().to(dtype).clone().requires_grad_(wts is not None) for k, v in de.state_dict().items()}
    sp = case["speech"].detach().clone().to(dtype).requires_grad_(wts is not None)
    sy = case["style"].detach().clone().to(dtype).requires_grad_(wts is not None)
    s = {k: v.to(dtype) for k, v in stats.items()}
    with oracle_bug(bug), torch.set_grad_enabled(wts is not None):
        O = onets.decoder_rollout(w, *[t.to(dtype) for t in case["fp"]], case["gaze"].to(dtype), sp, sy, s["in_mean"], s["in_std"],
                                  s["out_mean"], s["out_std"], synth.DT)
        if wts is None:
            return [o.detach() for o in O], None
        sum((o * wt.to(dtype)).sum() for o, wt in zip(O, wts)).backward()
    grads = {k: v.grad for k, v in w.items()}
    grads["speech"], grads["style"] = sp.grad, sy.grad
    return [o.detach() for o in O], grads


_DEC_ORACLE = {}


def decoder_oracle_cached(net, B, T, kind, weighting=None, dtype=torch.float64, bug=None):
    """decoder_oracle of (decoder_net(net), decoder_case(B, T), decoder_stats(kind), decoder_weighting(weighting)), computed once
    per process and left unchanged: the paths of one shape share it"""
    key = (net, B, T, kind, weighting, dtype, bug if not isinstance(bug, tuple) else None)
    if isinstance(bug, tuple) or key not in _DEC_ORACLE:
        wts = None if weighting is None else decoder_weighting(weighting, B, T)
        res = decoder_oracle(decoder_net(net), decoder_case(B, T), decoder_stats(kind), wts, dtype, bug)
        if isinstance(bug, tuple):
            return res
        _DEC_ORACLE[key] = res
    return _DEC_ORACLE[key]


def half_turns(outs):
    """h = dt / 2 |root_vrt| of the generated frames 1 .. T-1 (what the root integration exponentiates) -> (min, max)"""
    h = 0.5 * synth.DT * outs[3][:, 1:].double().norm(dim=-1)
    return float(h.min()), float(h.max())


def assert_half_turns(kind, outs):
    """the branch condition of a kind, from the float64 oracle's own root_vrt"""
    lo, hi = half_turns(outs)
    a, b = DEC_TURN_RANGE[kind]
    assert a < lo and hi < b, (kind, lo, hi)
    assert hi < DEC_SMALL_EPS / 2 or lo > 2 * DEC_SMALL_EPS, (kind, lo, hi)
    return lo, hi


def decoder_grad_slices(grads):
    """{name: gradient} of a decoder -> {slice: tensor}: every tensor whole, and the parts of the three matrices whose blocks see
    different shares of the root chain -- output layer (layer2, FiLM: layer3) rows [0:3] root_vel, [3:6] root_vrt, [6:] joints;
    layer0 columns: pose [0:6], [6:PO], gaze, speech, style; GRU layer 0 input columns: hid [:H] and the same groups behind it."""
    out = dict(grads)
    p = "recurrent_decoder."
    last = p + ("layer3" if p + "layer3.weight" in grads else "layer2")
    for a, b in ((0, 3), (3, 6), (6, None)):
        out[f"{last}.weight[{a}:{b}]"] = grads[last + ".weight"][a:b]
        out[f"{last}.bias[{a}:{b}]"] = grads[last + ".bias"][a:b]
    PO = grads[last + ".bias"].shape[0]
    SP = grads["speech"].shape[-1]
    XD = grads[p + "layer0.weight"].shape[1]
    cols = [("pose[0:6]", 0, 6), ("pose[6:]", 6, PO), ("gaze", PO, PO + 3), ("speech", PO + 3, PO + 3 + SP)]
    if XD > PO + 3 + SP:
        cols.append(("style", PO + 3 + SP, XD))
    H = grads[p + "layer1.weight_hh_l0"].shape[1]
    for n, a, b in cols:
        out[f"{p}layer0.weight[:, {n}]"] = grads[p + "layer0.weight"][:, a:b]
        out[f"{p}layer1.weight_ih_l0[:, {n}]"] = grads[p + "layer1.weight_ih_l0"][:, H + a:H + b]
    out[f"{p}layer1.weight_ih_l0[:, hid]"] = grads[p + "layer1.weight_ih_l0"][:, :H]
    return out


def decoder_slice_errors(got, ref):
    """per slice of decoder_grad_slices: max |got - ref| / max |ref| (each slice against its OWN largest entry); a slice whose
    reference is exactly zero must be exactly zero: its error is 0 or inf (the shape of slice_errors above)"""
    gs, rs = decoder_grad_slices(got), decoder_grad_slices(ref)
    errs = {}
    for k, r in rs.items():
        gk = gs[k].detach().double().cpu()
        m = float(r.abs().max())
        if m == 0.0:
            errs[k] = 0.0 if float(gk.abs().max()) == 0.0 else float("inf")
        else:
            errs[k] = float((gk - r.double()).abs().max()) / m
    return errs


def decoder_output_errors(got, ref):
    """per output group: max |got - ref|"""
    return {n: float((o.detach().double().cpu().reshape(r.shape) - r.double()).abs().max()) for n, o, r in zip(DEC_NAMES, got, ref)}


def root_norm_change(outs):
    """|root_rot[:, -1]| - |root_rot[:, 0]| per row"""
    q = outs[1].detach().double().cpu()
    return q[:, -1].norm(dim=-1) - q[:, 0].norm(dim=-1)


def assert_decoder_outputs(kind, got, ref, T):
    """The output assertions of one case against the float64 oracle `ref`: every group within DEC_OUT_BOUND; still / zero: root_rot
    within (T - 1) 1e-6 -- a tenth of the norm deficit (T - 1) 1e-5 that the small branch's division by (|.| + 1e-5) produces and
    the other branches would not -- and the norm of root_rot loses (T - 1) 1e-5 within (T - 1) 1e-6; the other kinds keep the norm
    within 2e-6.  -> the errors per group."""
    errs = decoder_output_errors(got, ref)
    for o in got:
        assert bool(torch.isfinite(o).all()), kind
    for n, e in errs.items():
        assert e < DEC_OUT_BOUND, (kind, n, e)
    dn = root_norm_change(got)
    if kind in ("still", "zero"):
        assert errs["root_rot"] < (T - 1) * 1e-6, (kind, errs["root_rot"])
        assert float((dn + (T - 1) * DEC_SMALL_EPS).abs().max()) < (T - 1) * 1e-6, (kind, dn)
    elif kind != "tied":
        assert float(dn.abs().max()) < 2e-6, (kind, dn)
    return errs


def assert_decoder_grads(got, ref, tag=""):
    """every parameter tensor, dspeech, dstyle and every slice of decoder_grad_slices within its bound of the float64 oracle, each
    relative to its own largest oracle entry -> the errors per slice"""
    errs = decoder_slice_errors(got, ref)
    bad = {k: e for k, e in errs.items() if not e < DEC_SLICE_BOUNDS.get(k, DEC_GRAD_BOUND)}
    assert not bad, (tag, bad)
    return errs


# (path, decoder, B, T) of tests/test_gpu_decoder_stats.py: the smallest shapes at which each path runs -- T >= 4 for the persistent
# forward, T >= 3 for the persistent sweep; B = 5: one 16-row tile, 17: two tiles (4-row form / dual chain), 33 / 40: three tiles
# and the two-sweep BPTT
DEC_TRAIN_CASES = (("generic", "main", 2, 6), ("stage", "main", 5, 6), ("stage", "main", 33, 4), ("tp16-tiles4=0", "main", 5, 6),
                   ("tp16-tiles4=1", "main", 5, 6), ("tp4", "main", 17, 5), ("dual", "main", 17, 5), ("bptt", "main", 5, 6),
                   ("bptt", "main", 17, 5), ("bptt", "main", 40, 4), ("film", "film", 5, 6), ("h512", "h512", 2, 6))
DEC_TRAIN_KINDS = (("tied", "all"),) + tuple((k, w) for k in ("untied", "still", "brisk", "spin") for w in ("all", "root"))
DEC_INFER_CASES = (("ring", 3, 7), ("b1-persistent", 1, 6), ("b1-persistent", 1, 37), ("b1-stage-gemv", 1, 6), ("b1-stage-gemv", 1, 37),
                   ("b1-stage-mfma", 1, 6), ("b1-stage-mfma", 1, 37), ("batch-chunk4", 3, 9))
DEC_INFER_KINDS = ("tied", "untied", "still", "brisk", "spin", "zero")


def decoder_shapes():
    """every (decoder, B, T) the GPU file runs"""
    return sorted({c[1:] for c in DEC_TRAIN_CASES} | {("main", B, T) for _, B, T in DEC_INFER_CASES})


# ----------------------------------------------------------------------------- the decoder at other dimensions
# (tests/test_gpu_decoder_dims.py on the device, tests/test_decoder_dims_oracle_cpu.py on the CPU.)  Everything above builds ONE
# family: synth.NJ = 75 joints (PI = 1134, PO = 1131), SP = ST = 64, H in {512, 768, 1024}.  PI, PO, SP, ST and H are free
# dimensions of the C ABI; the rigs and widths below reach the tile edges of each of them and both sides of every limit of the
# four *_supported predicates.
# rig: (J joints, SP speech columns, ST style columns); PO = 6 + 15 J, PI = PO + 3, XD = PI + SP + ST
DEC_DIM_RIGS = {"j24": (24, 64, 64),           # KBX = 32: the per-frame operand of the rollout (201 blocks) is wider than 64 + KBX + 64
                "j6": (6, 32, 16),             # PO = 96 (a multiple of 16), XD = 147 (16 * 9 + 3), KBC = 3
                "j1": (1, 8, 4),               # PO = 21 (the fast path needs 16), KBC = 1
                "j76": (76, 64, 64),           # nTPO = 72: the widest rig all three persistent kernels accept
                "j77": (77, 64, 64),           # nTPO = 73: the BPTT sweep and the decode kernel (2 H + XD = 3340) decline
                "j86": (86, 64, 64),           # PO = 1296 > 1280: every persistent kernel declines
                "wide-cond": (24, 100, 64)}    # SP + ST = 164 > 128, KBC = 11: the rollout and the decode kernel decline
# decoder tag: (rig, H, rnn_cond)
DEC_DIM_NETS = {"j24": ("j24", 1024, "normal"), "j6": ("j6", 1024, "normal"), "j1": ("j1", 1024, "normal"),
                "j76": ("j76", 1024, "normal"), "j77": ("j77", 1024, "normal"), "j86": ("j86", 1024, "normal"),
                "wide-cond": ("wide-cond", 1024, "normal"),
                "h16": ("j6", 16, "normal"),   # nT5 = 4, last GRU unit tile: 1 unit
                "h48": ("j6", 48, "normal"),   # nT5 = 10, last tile: 3 units
                "h80": ("j6", 80, "normal"),   # nT5 = 16, last tile: a full 5
                "film-j24-h48": ("j24", 48, "film"),
                "h24-generic": ("j6", 24, "normal")}      # H % 16 != 0: the fast path declines


def decoder_dims(net):
    """-> dict(J, SP, ST, PO, PI, XD, H, film) of a tag of DEC_DIM_NETS (XD: the step input, without the style under FiLM)"""
    rig, Hn, cond = DEC_DIM_NETS[net]
    J, SP, ST = DEC_DIM_RIGS[rig]
    PO = 6 + 15 * J
    film = cond == "film"
    return dict(rig=rig, J=J, SP=SP, ST=ST, PO=PO, PI=PO + 3, XD=PO + 3 + SP + (0 if film else ST), H=Hn, film=film)


def decoder_rig(J, SP, ST, kind="untied", dtype=torch.float32, device="cpu"):
    """-> (PI, PO, dict(in_mean, in_std, out_mean, out_std)) of a J-joint rig, seeded by (J, SP, ST): the construction of
    synth.make_stats / decoder_stats at another width.  tied: out_mean == in_mean[:PO]; untied: out_mean ~ N(0, 1) from its own
    generator and out_std[3:6] = (0.8, 1.1, 0.6).  out_std keeps PO // 28 exact zeros behind the six root columns (constant
    channels; 40 of 1131 at J = 75)."""
    assert kind in ("tied", "untied"), kind
    PO = 6 + 15 * J
    PI = PO + 3
    rng = np.random.default_rng(1000 * J + 10 * SP + ST)
    im = rng.normal(0.0, 1.0, PI).astype(np.float32)
    isd = rng.uniform(0.5, 2.0, PI).astype(np.float32)
    om = im[:PO].copy()
    osd = rng.uniform(0.3, 1.5, PO).astype(np.float32)
    osd[6 + rng.choice(PO - 6, PO // 28, replace=False)] = 0.0
    if kind == "untied":
        om = np.random.default_rng(2024 + J).standard_normal(PO).astype(np.float32)
        osd[3:6] = (0.8, 1.1, 0.6)
    t = lambda a: torch.as_tensor(a).to(dtype).to(device)  # noqa: E731
    return PI, PO, dict(in_mean=t(im), in_std=t(isd), out_mean=t(om), out_std=t(osd))


def decoder_dim_stats(net, kind, dtype=torch.float32, device="cpu"):
    d = decoder_dims(net)
    return decoder_rig(d["J"], d["SP"], d["ST"], kind, dtype, device)[2]


def _decoder_dim_net(tag):
    d = decoder_dims(tag)
    torch.manual_seed(5000 + sorted(DEC_DIM_NETS).index(tag))
    kw = dict(rnn_cond="film") if d["film"] else {}
    return modules.Decoder(d["PI"], d["PO"], d["SP"], d["ST"], d["H"], 2, **kw)


_DEC_DIM_CASES = {}


def _random_rotations(rng, n):
    """n rotation matrices [n, 3, 3] from uniformly random unit quaternions"""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)


def decoder_dim_case(rig, B, T):
    """float32 inputs of a [B, T] rollout on a rig of DEC_DIM_RIGS, the dict of decoder_case: unit root quaternions (general, not
    yaw only), ltxy = the first two axes of a random rotation per joint (orthonormal rows), velocities as finite differences of a
    smooth track (the scales of synth.make_clip), a gaze target 180 units away, speech / style ~ 0.5 N(0, 1); cached, read-only"""
    key = (rig, B, T)
    if key in _DEC_DIM_CASES:
        return _DEC_DIM_CASES[key]
    J, SP, ST = DEC_DIM_RIGS[rig]
    rng = np.random.default_rng(31 * J + 7 * B + T)
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    track = np.stack([synth._smooth(rng, 2, 3 + 3 * J, 0.05) for _ in range(B)])        # [B, 2, 3 + 3 J]: root and joint positions
    vel = (track[:, 1] - track[:, 0]) / synth.DT
    hel = np.stack([synth._smooth(rng, 2, 3 + 3 * J, 0.02) for _ in range(B)])          # helical angles: their difference is vrt
    vrt = (hel[:, 1] - hel[:, 0]) / synth.DT
    R = _random_rotations(rng, B * J).reshape(B, J, 3, 3)
    ltxy = np.stack([R[..., :, 0], R[..., :, 1]], axis=2)                                # [B, J, 2, 3]
    lpos = rng.normal(0, 8.0, (1, J, 3)) + track[:, 0, 3:].reshape(B, J, 3)
    fp = [f(rng.standard_normal((B, 3)) * 20.0), f(q), f(vel[:, :3] * 30), f(vrt[:, :3]), f(lpos), f(ltxy),
          f(vel[:, 3:].reshape(B, J, 3)), f(vrt[:, 3:].reshape(B, J, 3))]
    gaze = f(np.tile(np.array([[[10.0, 150.0, 100.0]]]), (B, T, 1)) + rng.normal(0, 1.0, (B, 1, 3)))
    gen = torch.Generator().manual_seed(4 + J)
    speech, style = torch.randn(B, T, SP, generator=gen) * 0.5, torch.randn(B, T, ST, generator=gen) * 0.5
    _DEC_DIM_CASES[key] = dict(fp=fp, gaze=gaze, speech=speech, style=style, B=B, T=T, J=J)
    return _DEC_DIM_CASES[key]


def decoder_dim_oracle(net, B, T, kind, weighting=None, dtype=torch.float64, de=None):
    """decoder_oracle of a DEC_DIM_NETS decoder (or `de`, a modified copy of it) on its rig's case and statistics"""
    d = decoder_dims(net)
    wts = None if weighting is None else decoder_weighting(weighting, B, T, d["J"])
    return decoder_oracle(de or decoder_net(net), decoder_dim_case(d["rig"], B, T), decoder_dim_stats(net, kind), wts, dtype)


_DEC_DIM_ORACLE = {}


def decoder_dim_oracle_cached(net, B, T, kind, weighting=None, dtype=torch.float64):
    """the float64 (or float32) oracle of a case, computed once per process and left unchanged"""
    key = (net, B, T, kind, weighting, dtype)
    if key not in _DEC_DIM_ORACLE:
        _DEC_DIM_ORACLE[key] = decoder_dim_oracle(net, B, T, kind, weighting, dtype)
    return _DEC_DIM_ORACLE[key]


def decoder_dim_limits(net):
    """Which kernels take a decoder's dimensions, from the limits as the kernel files state them (never by asking the library;
    tests/test_decoder_dims_oracle_cpu.py holds the same table written by hand).  Batch and frame counts are the case's business:
    every case here has B <= 64 and T >= 4.
      fast    decoder_fast.hip  dec_fast_supported:        H % 16 == 0, PI == PO + 3, PO >= 16
      tp      train_persistent.hip  dec_tp_supported:      normal, H == 1024, 16 <= PO <= 1280 (5 x 256 columns), SP + ST <= 128,
                                                           1 <= KBC <= 8; on the fast path only
      bp      train_bwd_persistent.hip  dec_bp_supported:  normal, H == 1024, PO >= 16, (PO + 15) / 16 <= 72, XD <= 2048; fast path only
      dp      decode_persistent.hip  dec_persistent_supported:  normal, H == 1024, 2 H + XD <= 3328 (26 x 128), SP + ST <= 128,
                                                           6 <= PO <= 1280"""
    d = decoder_dims(net)
    PO, XD, Hn, C = d["PO"], d["XD"], d["H"], d["SP"] + d["ST"]
    KBC = (C + 15) // 16
    big = Hn == 1024 and not d["film"]
    fast = Hn % 16 == 0 and d["PI"] == PO + 3 and PO >= 16
    return dict(fast=fast,
                tp=fast and big and 16 <= PO <= 1280 and C <= 128 and 1 <= KBC <= 8,
                bp=fast and big and PO >= 16 and (PO + 15) // 16 <= 72 and XD <= 2048,
                dp=big and 2 * Hn + XD <= 3328 and C <= 128 and 6 <= PO <= 1280)


# path -> library switches (the defaults otherwise) and which persistent kernels it asks for; "default" / "b1-default": no switch,
# whatever the limits give
DEC_DIM_TRAIN_OPTIONS = {"generic": dict(decoder_fast=0), "stage": dict(train_persistent=0, bwd_persistent=0),
                         "tp16-tiles4=0": dict(tp_tiles4=0, bwd_persistent=0), "tp16-tiles4=1": dict(bwd_persistent=0),
                         "tp4": dict(bwd_persistent=0), "dual": dict(tp_dual=1, bwd_persistent=0), "bptt": {}, "default": {}}
DEC_DIM_INFER_OPTIONS = {"ring": {}, "b1-persistent": {}, "b1-default": {}, "b1-stage-gemv": dict(persistent=0),
                         "b1-stage-mfma": dict(persistent=0, stage_variant=1024), "batch-chunk4": {}}
_DEC_DIM_WANTS = {"generic": (), "stage": (), "tp16-tiles4=0": ("tp",), "tp16-tiles4=1": ("tp",), "tp4": ("tp",), "dual": ("tp",),
                  "bptt": ("tp", "bp"), "default": ("tp", "bp"), "ring": (), "b1-persistent": ("dp",), "b1-default": ("dp",),
                  "b1-stage-gemv": (), "b1-stage-mfma": (), "batch-chunk4": ("tp",)}
_DEC_DIM_STATE = dict(dp=0, tp=1, bp=2)        # the index of zeggs_persistent_state


def decoder_dim_ran(path, net):
    """the persistent kernels (zeggs_persistent_state indices) that must have run for a path on a decoder: those the path asks for
    and the limits grant"""
    lim = decoder_dim_limits(net)
    return tuple(sorted(_DEC_DIM_STATE[k] for k in _DEC_DIM_WANTS[path] if lim[k]))


def _dim_train(net, *cases):
    return [(p, net, B, T, k) for p, B, T, k in cases]


_U, _TI = "untied", "tied"
_PER_WIDTH_TRAIN = (("generic", 2, 6, _U), ("stage", 5, 6, _U), ("stage", 33, 4, _U))
_PER_WIDTH_INFER = (("ring", 3, 7, _U), ("b1-stage-gemv", 1, 6, _U), ("b1-stage-mfma", 1, 6, _U))
# (path, decoder, B, T, statistics kind); weighting `all` throughout.  Shapes: the smallest that reach each path (DEC_TRAIN_CASES).
DEC_DIM_TRAIN_CASES = tuple(
    _dim_train("j24", ("stage", 5, 6, _U), ("tp16-tiles4=0", 5, 6, _U), ("tp16-tiles4=1", 5, 6, _U), ("tp4", 17, 5, _U),
               ("dual", 17, 5, _U), ("bptt", 5, 6, _U), ("bptt", 17, 5, _U), ("bptt", 40, 4, _U), ("bptt", 5, 6, _TI)) +
    _dim_train("j6", ("stage", 5, 6, _U), ("tp16-tiles4=0", 5, 6, _U), ("tp16-tiles4=1", 5, 6, _U), ("tp4", 17, 5, _U),
               ("dual", 17, 5, _U), ("bptt", 40, 4, _U), ("bptt", 5, 6, _TI)) +
    _dim_train("j1", ("stage", 5, 6, _U), ("tp16-tiles4=1", 5, 6, _U), ("bptt", 5, 6, _U), ("bptt", 5, 6, _TI)) +
    _dim_train("j76", ("bptt", 5, 6, _U), ("bptt", 5, 6, _TI)) +
    _dim_train("j77", ("default", 5, 6, _U), ("default", 5, 6, _TI)) +         # the rollout runs, the BPTT sweep declines
    _dim_train("j86", ("default", 5, 4, _U), ("default", 5, 4, _TI)) +         # both decline
    _dim_train("wide-cond", ("stage", 5, 6, _U), ("stage", 5, 6, _TI),
               ("default", 5, 6, _U)) +          # the rollout declines; the BPTT sweep has no limit on SP + ST and runs
    _dim_train("h16", *_PER_WIDTH_TRAIN) + _dim_train("h48", *_PER_WIDTH_TRAIN) + _dim_train("h80", *_PER_WIDTH_TRAIN) +
    _dim_train("film-j24-h48", ("default", 5, 6, _U)) +
    _dim_train("h24-generic", ("default", 2, 6, _U)))
_B1 = (("b1-persistent", 1, 6, _U), ("b1-stage-gemv", 1, 6, _U), ("b1-stage-mfma", 1, 6, _U), ("ring", 3, 7, _U),
       ("batch-chunk4", 3, 9, _U))
DEC_DIM_INFER_CASES = tuple(
    _dim_train("j24", *_B1) + _dim_train("j6", *_B1) + _dim_train("j1", ("b1-persistent", 1, 6, _U)) +
    _dim_train("j76", ("b1-persistent", 1, 6, _U)) + _dim_train("j77", ("b1-default", 1, 6, _U)) +
    _dim_train("j86", ("b1-default", 1, 6, _U)) + _dim_train("wide-cond", ("ring", 3, 7, _U), ("b1-default", 1, 6, _U)) +
    _dim_train("h16", *_PER_WIDTH_INFER) + _dim_train("h48", *_PER_WIDTH_INFER) + _dim_train("h80", *_PER_WIDTH_INFER) +
    _dim_train("film-j24-h48", ("ring", 3, 7, _U)))
# Bounds: DEC_OUT_BOUND / DEC_GRAD_BOUND through assert_decoder_outputs / assert_decoder_grads, as tests/test_gpu_decoder_stats.py.
# A case whose FLOAT32 ORACLE is not within a quarter of them would get 4 x that oracle's own distance here, with the measured value
# beside it; none does (tests/test_decoder_dims_oracle_cpu.py::test_float32_oracle_within_a_quarter_of_every_bound).


def decoder_dim_shapes(training=None):
    """every (decoder, B, T, kind) the GPU file runs: training cases, inference cases, or both"""
    tr = {c[1:] for c in DEC_DIM_TRAIN_CASES}
    inf = {c[1:] for c in DEC_DIM_INFER_CASES}
    return sorted(tr if training is True else inf if training is False else tr | inf)


def decoder_dim_edges(net):
    """the last (partial) tile of each tiled dimension of a decoder -> dict(PO=(lo, hi) rows of the output layer, XD=(lo, hi)
    columns of the step input, H=(lo, hi) GRU units): 16-wide tiles of PO and XD, 5-unit tiles of H (nT5 = (H + 4) / 5)"""
    d = decoder_dims(net)
    last16 = lambda n: (16 * ((n + 15) // 16 - 1), n)  # noqa: E731
    return dict(PO=last16(d["PO"]), XD=last16(d["XD"]), H=(5 * ((d["H"] + 4) // 5 - 1), d["H"]))


def decoder_edge_zeroed(net, edge):
    """a copy of the decoder with the weights of one edge of decoder_dim_edges zeroed: PO -- those rows of the output layer (weight
    and bias); XD -- those columns of layer0 and of GRU layer 0's input weights (behind its H hid columns); H -- those units: their
    rows (gates r, z, n) of both GRU layers' weights and biases"""
    import copy
    de = copy.deepcopy(decoder_net(net))
    d = decoder_dims(net)
    lo, hi = decoder_dim_edges(net)[edge]
    r, Hn = de.recurrent_decoder, d["H"]
    sd_ = dict(r.named_parameters())
    with torch.no_grad():
        if edge == "PO":
            last = "layer3" if d["film"] else "layer2"
            sd_[last + ".weight"][lo:hi] = 0.0
            sd_[last + ".bias"][lo:hi] = 0.0
        elif edge == "XD":
            sd_["layer0.weight"][:, lo:hi] = 0.0
            sd_["layer1.weight_ih_l0"][:, Hn + lo:Hn + hi] = 0.0
        else:
            assert edge == "H", edge
            for k, v in sd_.items():
                if k.startswith("layer1."):
                    for gate in range(3):
                        v[gate * Hn + lo:gate * Hn + hi] = 0.0
    return de


# ---- RAdam (tests/test_radam_oracle_cpu.py measures and proves on the CPU, tests/test_gpu_radam.py runs the device).
# Errors are counted in float32 ROUNDINGS: |got - float64 oracle| / (2^-24 * scale), per element and step, every scale taken from
# the float64 oracle -- v: v itself; m: the same moving average taken over |g|; p: |p0| + sum_t |p_t - p_{t-1}| (+ RADAM_UNDERFLOW,
# below).  Where a scale is zero (an element that never saw a gradient) the value must be EXACTLY the oracle's.
# RADAM_REF_ROUNDINGS: the worst distance of the reference's own float32 run (tests/golden/radam_steps.npz: 4 configurations, 3
# tensors, 12 steps) from the float64 oracle, as test_radam_oracle_cpu.py::test_yardstick_reference_float32_run_vs_float64_oracle
# measures it on the committed fixture.  RADAM_BOUND = 4 x that, per array, is what every device comparison allows: the margin
# covers the kernel's FMA contraction and its other order of the same few operations per step (division and sqrtf are correctly
# rounded on both sides).
# RADAM_UNDERFLOW: float32 has no rounding finer than its smallest normal number, 2^-126 -- below it results lose bits or (on the
# device, which flushes denormals) become zero, so (1 - beta2) g g carries an absolute error of up to 2^-126 however small v is.
# Every non-zero scale therefore gets 2^-126 * 2^24 added: one "rounding" is never less than 2^-126.  That reaches only v < 2e-31,
# |g| < 1e-14 -- real gradients have such entries (the engine test met v = 0 against 1e-50), the recipe's (|g| >= 1e-9, v >= 1e-21)
# do not, and sqrt(v) there is 1e-10 of eps.
RADAM_UNDERFLOW = 2.0 ** -102
RADAM_REF_ROUNDINGS = dict(p=6.5, m=4.2, v=7.0)            # measured 6.48, 4.17, 6.91 -> RADAM_BOUND 26, 16.8, 28
RADAM_BOUND = {k: 4.0 * r for k, r in RADAM_REF_ROUNDINGS.items()}
RADAM_BUGS = ("eps_dropped", "eps_inside_sqrt", "eps_squared", "step_one_behind", "lr_decay_one_step_late", "weight_decay_after_update",
              "betas_exchanged", "update_in_the_no_update_branch")
RADAM_F32_COMPLEMENTS = "float32_complements"        # 1.f - beta formed in float32 (what radam_k did): recorded, not a control
_RADAM_FIXTURE = {}


def radam_fixture():
    """radam_steps.npz -> (gd, configs): configs[c] = one dict per tensor (p0, g [steps, n], lr, betas, weight_decay,
    degenerated_to_sgd and the reference's p, m, v [steps, n]).  Loaded once, read-only."""
    if not _RADAM_FIXTURE:
        gd = np.load(GOLDEN / "radam_steps.npz")
        configs = []
        for c in range(int(gd["n_configs"])):
            per = []
            for t, grp in enumerate(gd[f"c{c}_group_of"]):
                steps = int(gd["steps"])
                d = dict(p0=gd[f"p0_{t}"].reshape(-1), g=gd[f"g_{t}"].reshape(steps, -1), shape=gd[f"p0_{t}"].shape,
                         lr=float(gd[f"c{c}_lr"][grp]), betas=tuple(float(b) for b in gd[f"c{c}_betas"][grp]),
                         weight_decay=float(gd[f"c{c}_weight_decay"]), degenerated_to_sgd=bool(gd[f"c{c}_degenerated_to_sgd"]),
                         group=int(grp))
                d.update({k: gd[f"c{c}_{k}_{t}"].reshape(steps, -1) for k in "pmv"})
                for a in d.values():
                    if isinstance(a, np.ndarray):
                        a.setflags(write=False)
                per.append(d)
            configs.append(per)
        _RADAM_FIXTURE["v"] = (gd, configs)
    return _RADAM_FIXTURE["v"]


def radam_lr(lr, step, decay_before=9, decay=0.995):
    """the fixture's schedule: lr x 0.995 before step 9 (1-based), as train.py:166-172 sets it on param_groups"""
    return lr * decay if step >= decay_before else lr


def radam_step64(p, g, m, v, step, lr, eps, beta1, beta2, weight_decay, degenerated_to_sgd, bug=None):
    """oracle/radam.py's float64 step restated with a switch for ONE wrong line (bug=None: bit-equal to oracle.radam.radam_step,
    which test_radam_oracle_cpu.py asserts) -- the negative controls of the RAdam bound."""
    from oracle import radam as oradam
    b1, b2 = (beta2, beta1) if bug == "betas_exchanged" else (beta1, beta2)
    c1, c2 = 1 - b1, 1 - b2
    if bug == RADAM_F32_COMPLEMENTS:
        c1, c2 = float(np.float32(1) - np.float32(b1)), float(np.float32(1) - np.float32(b2))
    v *= b2
    v += c2 * g * g
    m *= b1
    m += c1 * g
    rect, scale = oradam.radam_scalars(max(step - 1, 1) if bug == "step_one_behind" else step, lr, beta1, beta2, degenerated_to_sgd)
    if scale is None:
        if bug != "update_in_the_no_update_branch":
            return
        scale = lr / (1 - beta1 ** step)
    if weight_decay != 0 and bug != "weight_decay_after_update":
        p += (-weight_decay * lr) * p
    if rect:
        den = np.sqrt(v + eps) if bug == "eps_inside_sqrt" else np.sqrt(v) + (0.0 if bug == "eps_dropped" else eps * eps if bug == "eps_squared" else eps)
        with np.errstate(divide="ignore", invalid="ignore"):
            p += (-scale) * (m / den)
    else:
        p += (-scale) * m
    if weight_decay != 0 and bug == "weight_decay_after_update":
        p += (-weight_decay * lr) * p


def radam_oracle_run(p0, grads, steps, lr, eps, betas=(0.9, 0.999), weight_decay=0.0, degenerated_to_sgd=True, bug=None, lr_of=radam_lr):
    """The float64 trajectory from (p0, m = v = 0) over the 1-based step numbers `steps` (grads[i] at steps[i]).
    -> dict of [len(steps), n] float64 arrays: p, m, v and their rounding scales sp, sm, sv."""
    p, m, v = p0.astype(np.float64), np.zeros(p0.shape, np.float64), np.zeros(p0.shape, np.float64)
    mabs, path = np.zeros_like(p), np.abs(p)
    out = {k: [] for k in ("p", "m", "v", "sp", "sm", "sv")}
    for g, step in zip(grads, steps):
        g = g.astype(np.float64)
        before = p.copy()
        lr_t = lr_of(lr, step - 1 if bug == "lr_decay_one_step_late" else step)
        radam_step64(p, g, m, v, step, lr_t, eps, betas[0], betas[1], weight_decay, degenerated_to_sgd, bug)
        mabs = betas[0] * mabs + (1 - betas[0]) * np.abs(g)
        path = path + np.abs(p - before)
        for k, a in zip(("p", "m", "v", "sp", "sm", "sv"), (p, m, v, path, mabs, v)):
            out[k].append(a.copy())
    return {k: np.stack(a) for k, a in out.items()}


def radam_roundings(got, ref, scale, finite_only=False):
    """worst |got - ref| / (2^-24 scale) over all elements; where scale == 0 the value must be exactly ref's (inf otherwise).
    finite_only (the negative controls, whose wrong line may divide 0 by 0): the worst over the elements where `got` is finite."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, err / (2.0 ** -24 * (scale + RADAM_UNDERFLOW)), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(got), r, 0.0 if finite_only else np.inf)
    return float(r.max()) if r.size else 0.0


def radam_worst(got, ref):
    """got: dict p, m, v [steps, n] (float32); ref: radam_oracle_run's dict -> worst roundings per array"""
    return {k: radam_roundings(got[k], ref[k], ref["s" + k]) for k in "pmv"}


def assert_radam(got, ref, tag=""):
    worst = radam_worst(got, ref)
    for k in "pmv":
        assert worst[k] <= RADAM_BOUND[k], f"{tag}: {k} is {worst[k]:.1f} float32 roundings from the float64 oracle (bound {RADAM_BOUND[k]:.1f})"
    return worst


def radam_roundings_torch(got, ref, scale):
    """radam_roundings for torch tensors on any device (the engine's flat buffer: 25 M elements, compared where they live)"""
    err = (got.double() - ref).abs()
    r = torch.where(scale > 0, err / (2.0 ** -24 * (scale + RADAM_UNDERFLOW)), torch.where(err == 0, 0.0, float("inf")).to(err.dtype))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def radam_teacher_forced(before, g, after, step, lr, eps, betas=(0.9, 0.999), weight_decay=0.0, degenerated_to_sgd=True):
    """One step judged on its own: the float64 oracle's step `step` applied to float64 copies of the state BEFORE the step
    (before = (p, m, v) float32 tensors) with the gradient the step used, against the state after it.  The scales are the
    trajectory's restricted to this step -- v: v; m: beta1 |m_before| + (1 - beta1) |g|; p: |p_before| + |p - p_before| -- never
    larger than the trajectory's, so RADAM_BOUND holds a fortiori.  -> worst roundings per array"""
    from oracle import radam as oradam
    p, m, v = (t.double().clone() for t in before)
    g = g.double()
    sm = betas[0] * m.abs() + (1 - betas[0]) * g.abs()
    sp = p.abs()
    oradam.radam_step(p, g, m, v, step, lr, eps, betas[0], betas[1], weight_decay, degenerated_to_sgd)
    sp = sp + (p - before[0].double()).abs()
    return {k: radam_roundings_torch(a, r, s) for k, a, r, s in zip("pmv", after, (p, m, v), (sp, sm, v))}


# ----------------------------------------------------------------------------- fused attention kernels (tests/test_gpu_attention.py)
# csrc/attention.hip through zeggs_test_attention_fwd / _bwd against plain float64 softmax attention.  tests/test_attention_oracle_cpu.py
# measures on the CPU what float32 itself costs at every case below (the floors) and proves that the comparison is sharp
# (negative controls).
ATTN_HD = 32
ATTN_P = 0.1
LOG2E = 1.4426950408889634
ATTN_FAMILIES = ("mild", "g3", "g6", "lastkey", "onehot", "offset", "equal")
ATTN_CLASS = dict(mild="mild", equal="mild", g3="peaked", lastkey="peaked", onehot="peaked", offset="peaked", g6="extreme")


def attn_class(family, L):
    """the class whose bounds a case is held to: the family's, except `lastkey` at L = 2 -- "cancel": the last key holds all but
    p ~ 2e-4 of every row, so dS = P p (dP_1 - dP_0) and with it ALL of dQ and dK is a 2e-4 share of the terms it is the difference
    of (float32 leaves 6e-8 / 2e-4 of it uncertain).  Kept apart so that its floor does not widen the peaked bounds tenfold."""
    return "cancel" if (family, L) == ("lastkey", 2) else ATTN_CLASS[family]


ATTN_TENSORS = ("O", "lse2", "dQ", "dK", "dV", "dsum", "dbias")
ATTN_SMALL = 1e-3        # a gradient section whose float64 maximum is below this share of the dV section's is compared on dV's scale
# (family, B, NH, L, p)
ATTN_SHAPE_CASES = ([("mild", 2, 4, L, 0.0) for L in (1, 2, 31, 32, 33, 64, 127, 128, 129, 160, 257)] +
                    [("mild", 1, 1, 33, 0.0), ("mild", 3, 2, 129, 0.0), ("mild", 1, 8, 65, 0.0)])
ATTN_REGIME_CASES = ([(f, 2, 4, L, 0.0) for f in ATTN_FAMILIES for L in (33, 129, 257)] +
                     [(f, 2, 4, L, 0.0) for f in ("lastkey", "onehot", "equal") for L in (1, 2, 160)])
ATTN_DROPOUT_CASES = [(f, 2, 4, L, ATTN_P) for f in ("mild", "g3", "lastkey") for L in (33, 129, 257)]
ATTN_WRAP = dict(B=270, NH=1, L=4000, p=ATTN_P, heads=(0, 267, 268, 269), seed=90210)      # element 2^32: head 268, row 1741, key 3296
# THE BOUNDS.  Per family class and tensor: 4 x the largest error of the FLOAT32 evaluation of attention_oracle against its float64
# evaluation over the class's cases above (the p = 0.1 cases with the masks of hash_keep_scale; the wrap case's four heads count as
# mild), in the measure of attention_errors.  The margin of 4 is for what the kernels do differently from torch's float32: the
# 32-key tile order and matrix-core accumulation, v_exp_f32 / v_log_f32 at 1 ulp, log2 e folded into the query scale.  Floors as
# test_attention_oracle_cpu.py::test_float32_floors_are_within_a_quarter_of_the_bounds measures them (it asserts floor <= bound / 4):
ATTN_FLOORS = {
    "mild": dict(O=1.15e-6, lse2=1.35e-7, grad=2.6e-6, dsum=8.4e-7, dbias=6.7e-7),        # measured 1.12e-6 1.29e-7 2.52e-6 8.15e-7 6.51e-7
    "peaked": dict(O=6.5e-6, lse2=3.2e-7, grad=8.3e-6, dsum=8.2e-6, dbias=4.2e-6),        # measured 6.31e-6 3.13e-7 8.03e-6 7.95e-6 4.04e-6
    "extreme": dict(O=8.3e-6, lse2=2.15e-7, grad=7.7e-6, dsum=1.0e-5, dbias=4.8e-6),      # measured 8.05e-6 2.07e-7 7.49e-6 9.68e-6 4.68e-6
    "cancel": dict(O=7.2e-8, lse2=1.75e-7, grad=6.4e-5, dsum=7.0e-8, dbias=5.7e-5),       # measured 6.99e-8 1.68e-7 6.18e-5 6.72e-8 5.54e-5
}
# (worst cases: mild O 2x4x257 with dropout, gradients `equal` at 257; peaked O and dsum `offset` at 129 / 257, gradients `offset` at 33;
# extreme: g6 at 129 / 257; cancel = `lastkey` at L = 2 alone, attn_class.  lse2 is relative to max(1, max |lse2|): 10 (mild) ... 260
# (g6) in base 2.)
# The float32 restatement runs its backward in the kernels' form (attention_oracle(d_from_o=True): D = rowsum(dO . O) from the output).
# With autograd's form -- D = sum_k P_k dP_k, whose roundings cancel against the minuend's -- the `lastkey` L = 2 floors are 2.1e-5 /
# 9.3e-6 instead of 6.2e-5 / 5.5e-5 and the MI355X kernels measured 7.2e-5 (dQ) / 8.2e-5 (dbias) there: the one excess the first device
# run found, explained by that rounding, which was then added to the restatement (and `equal`'s dQ floor rose from 1.1e-6 to 2.5e-6).
# No floor or bound was taken from the kernels' output.
ATTN_BOUND = {c: {k: 4.0 * v for k, v in f.items()} for c, f in ATTN_FLOORS.items()}
ATTN_BUGS = ("O_row", "dQ_row", "dK_row", "dV_row", "key_L", "mask_transposed", "bwd_mask_redrawn", "dsum_undropped",
             "lse_natural", "dK_without_ln2")       # + the hash's high word ignored: hash_keep_scale(bug="hi_ignored")


def attn_bound_key(tensor):
    return "grad" if tensor in ("dQ", "dK", "dV") else tensor


def attn_case_id(case):
    f, B, NH, L, p = case
    return f"{f}-{B}x{NH}x{L}" + ("-drop" if p > 0 else "")


def attn_case_seed(case):
    f, B, NH, L, p = case
    return 7000 + 1000 * ATTN_FAMILIES.index(f) + 37 * B + 5 * NH + L


def attn_mask_seed(case):
    return 0x1234567800000000 + attn_case_seed(case)        # (both words of the seed are in use)


def attention_case(family, B, NH, L, seed):
    """seeded inputs of one comparison -> (qkv [B, L, 3E], dO [B, L, E]) float32, E = 32 NH.  `u` is a unit vector per head.
    mild: randn (logit std 1); g3 / g6: q and k times 3 / 6 (logit std 9 / 36: peaked rows, largest probability 1.0);
    lastkey: q += 4 u, key L-1 += 12 u (the row maximum is the last key -- in the partial tile when L % 32 != 0);
    onehot: q += 6 u, key 0 += 40 u (the first probability of nearly every row is exactly 1.0 in float32, the others underflow);
    offset: q and k += 20 u (a common logit offset of 70 nats that the max subtraction must cancel);
    equal: all keys identical (the softmax is exactly uniform)."""
    assert family in ATTN_FAMILIES, family
    gen = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, L, NH, ATTN_HD, generator=gen) for _ in range(3))
    dO = torch.randn(B, L, NH * ATTN_HD, generator=gen)
    u = torch.randn(NH, ATTN_HD, generator=gen)
    u = u / u.norm(dim=-1, keepdim=True)
    if family in ("g3", "g6"):
        g = 3.0 if family == "g3" else 6.0
        q, k = q * g, k * g
    elif family == "lastkey":
        q = q + 4.0 * u
        k[:, L - 1] += 12.0 * u
    elif family == "onehot":
        q = q + 6.0 * u
        k[:, 0] += 40.0 * u
    elif family == "offset":
        q, k = q + 20.0 * u, k + 20.0 * u
    elif family == "equal":
        k = k[:, :1].expand(B, L, NH, ATTN_HD)
    E = NH * ATTN_HD
    return torch.cat([t.reshape(B, L, E) for t in (q, k, v)], dim=-1).contiguous(), dO


def attention_oracle(qkv, dO, NH, keep=None, dtype=torch.float64, bug=None, d_from_o=False):
    """Plain softmax attention + autograd in `dtype`: scores q k^T / sqrt(32), softmax, times the keep-scale `keep` [B, NH, L, L]
    (None: no dropout), times v.  -> (O [B, L, E], lse2 [B NH, L] = logsumexp(s) log2 e, dqkv [B, L, 3E] of sum(O dO),
    dsum [B NH, L] = rowsum(dO . O) per head, dbias [3E] = the column sums of dqkv).
    d_from_o: the backward in the form the kernels use, dS = P (dPd keep - D) with D = rowsum(dO . O) taken from the output (the
    same function; in float64 equal to autograd's to rounding, in float32 it carries the rounding of that separate dot product).
    bug: one of ATTN_BUGS, the negative controls -- a model of one wrong line of the kernels; the *_row and key_L bugs touch the
    last query row (key) of the last head of the last batch entry only."""
    assert bug is None or bug in ATTN_BUGS, bug
    B, L, E3 = qkv.shape
    E = E3 // 3
    hd = E // NH
    x = qkv.detach().to(dtype).clone().requires_grad_(True)
    g = dO.detach().to(dtype)
    heads = lambda t: t.reshape(B, L, NH, hd).transpose(1, 2)  # noqa: E731  [B, NH, L, hd]
    q, k, v = heads(x[..., :E]), heads(x[..., E:2 * E]), heads(x[..., 2 * E:])
    m = None if keep is None else keep.to(dtype)
    if bug == "mask_transposed" and m is not None:
        m = m.transpose(-1, -2)
    if bug == "key_L":           # the clamped copy of key L-1 takes part as key L (last head of the last batch entry)
        sel = torch.zeros(B, NH, 1, 1, dtype=dtype)
        sel[-1, -1] = 1.0
        k = torch.cat([k, k[:, :, -1:]], dim=2)
        v = torch.cat([v, v[:, :, -1:]], dim=2)
        if m is not None:
            m = torch.cat([m, m[..., -1:]], dim=-1)
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    if bug == "key_L":
        s = torch.cat([s[..., :-1], s[..., -1:] + torch.log(sel)], dim=-1)       # every other head: -inf, the key does not exist
    P = torch.softmax(s, dim=-1)
    Pd = P if m is None else P * m
    if bug == "bwd_mask_redrawn" and m is not None:      # the backward sees another mask of the same rate
        other = m.roll(1, dims=-1)
        Pd = P * other + (P * m - P * other).detach()
    Oh = torch.matmul(Pd, v)                                                       # [B, NH, L, hd]
    gh = heads(g)
    if d_from_o or (bug == "dsum_undropped" and m is not None):
        # the kernels' backward (the flash-attention form): dS = P (dPd keep - D) with D = rowsum(dO . O) formed from the STORED
        # output, a dot product of its own -- in autograd's softmax backward D is sum_k P_k dP_k, the same dP as in the minuend, so
        # the roundings of dP cancel in dP - D wherever one key holds nearly all of the row (dS = P p (dP_1 - dP_0) at L = 2).
        # The bug forms D from the undropped probabilities.
        Os = torch.matmul(P, v) if bug == "dsum_undropped" else Oh
        D = (gh * Os).sum(-1, keepdim=True).detach()
        dPd = torch.matmul(gh, v.detach().transpose(-1, -2))
        dS = P.detach() * ((dPd if m is None else dPd * m) - D)
        s_lin = (s * dS).sum()                        # its gradient w.r.t. q and k is dS pushed through the scores
        v_lin = (torch.matmul(Pd.detach(), v) * gh).sum()
        (dx,) = torch.autograd.grad(s_lin + v_lin, x)
        dsum = D.squeeze(-1)
    else:
        (dx,) = torch.autograd.grad((Oh * gh).sum(), x)
        dsum = (gh * Oh.detach()).sum(-1)
    O = Oh.detach().transpose(1, 2).reshape(B, L, E).clone()
    lse2 = torch.logsumexp(s.detach(), dim=-1) * (1.0 if bug == "lse_natural" else LOG2E)
    dx = dx.clone()
    if bug == "O_row":
        O[-1, -1, E - hd:] *= 1.0 + 1e-3
    if bug in ("dQ_row", "dK_row", "dV_row"):
        sec = ("dQ_row", "dK_row", "dV_row").index(bug)
        dx[-1, -1, sec * E + E - hd:(sec + 1) * E] *= 1.0 + 1e-3
    if bug == "dK_without_ln2":
        dx[..., E:2 * E] *= LOG2E
    return O, lse2.reshape(B * NH, L), dx, dsum.reshape(B * NH, L), dx.sum(dim=(0, 1))


def attention_errors(got, ref):
    """(O, lse2, dqkv, dsum, dbias) of an implementation against the float64 oracle's -> {tensor: error} over ATTN_TENSORS.
    O, dsum: relerr (max |d| over the tensor's max).  lse2: max |d| / max(1, max |lse2|).  dQ / dK / dV: relerr of the section of
    dqkv, on the dV section's scale when the section's own float64 maximum is below ATTN_SMALL of it (dQ and dK of `onehot`, dQ of
    `equal`, dQ and dK at L = 1: their true value is ~ 0).  dbias: the worst of its three sections, each measured the same way (the
    dK section is a sum of rows of dS, each of which sums to zero).  An entry of `got` may be None: left out."""
    ref = [t.detach().double().cpu() for t in ref]
    E = ref[0].shape[-1]
    out = {}

    def sections(g, r):
        vmax = float(r[..., 2 * E:].abs().max())
        errs = []
        for i in range(3):
            gs, rs = g[..., i * E:(i + 1) * E], r[..., i * E:(i + 1) * E]
            scale = float(rs.abs().max())
            if scale < ATTN_SMALL * vmax:
                scale = vmax
            errs.append(float((gs - rs).abs().max()) / max(scale, 1e-300))
        return errs
    g = [None if t is None else t.detach().double().cpu().reshape(r.shape) for t, r in zip(got, ref)]
    if g[0] is not None:
        out["O"] = relerr(g[0], ref[0])
    if g[1] is not None:
        out["lse2"] = float((g[1] - ref[1]).abs().max()) / max(1.0, float(ref[1].abs().max()))
    if g[2] is not None:
        out["dQ"], out["dK"], out["dV"] = sections(g[2], ref[2])
    if g[3] is not None:
        out["dsum"] = relerr(g[3], ref[3])
    if g[4] is not None:
        out["dbias"] = max(sections(g[4], ref[4]))
    return out


def assert_attention(errs, cls, tag=""):
    """every error of attention_errors within ATTN_BOUND of the class `cls` (attn_class)"""
    bound = ATTN_BOUND[cls]
    bad = {k: (e, bound[attn_bound_key(k)]) for k, e in errs.items() if not e <= bound[attn_bound_key(k)]}
    assert not bad, (tag, cls, bad)


# ---- the mask hash of csrc/common.h restated in NumPy (hash_key, mix32k, the (lo, hi) form of dropout_scale_fast):
# tests/test_gpu_attention.py pins it bit for bit to zeggs_dropout, and draws from it the masks beyond element 2^32
def _mix32(x, k2=None):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(17); x *= np.uint32(0xed5ad4bb)      # noqa: E702
    x ^= x >> np.uint32(11)
    if k2 is not None:
        x += np.uint32(k2)
    x *= np.uint32(0xac4c1b51)
    x ^= x >> np.uint32(15); x *= np.uint32(0x31848bab)      # noqa: E702
    x ^= x >> np.uint32(14)
    return x


def hash_key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    with np.errstate(over="ignore"):
        a = _mix32(np.array([((seed & 0xffffffff) * 0x9E3779B1 & 0xffffffff) ^ (seed >> 32)], dtype=np.uint32))
        b = _mix32(a ^ np.uint32(0x85ebca6b))
    return int(a[0]), int(b[0])


def hash_keep_scale(seed, start, n, p, bug=None):
    """keep-scale (float64: 0 or 1 / (1 - p), the value _device_keep_scale returns) of the elements start .. start + n - 1 of a
    mask; bug = "hi_ignored": the high word of the 64-bit element index dropped (a negative control)."""
    idx = np.arange(int(start), int(start) + int(n), dtype=np.uint64)
    lo, hi = (idx & np.uint64(0xffffffff)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
    if bug == "hi_ignored":
        hi = np.zeros_like(hi)
    else:
        assert bug is None, bug
    a, b = hash_key(seed)
    with np.errstate(over="ignore"):
        h = _mix32((lo ^ ((hi << np.uint32(16)) | (hi >> np.uint32(16)))) + np.uint32(a), b)
    pf = np.float32(p)
    u = (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.where(u < pf, 0.0, 1.0 / (1.0 - p))


def attention_keep(seed, B, NH, L, p, heads=None, bug=None):
    """the attention site's keep-scale [B, NH, L, L] (element ((b NH + h) L + q) L + k) from hash_keep_scale; heads: only these
    flat head numbers b NH + h -> [len(heads), 1, L, L]"""
    if heads is None:
        return torch.as_tensor(hash_keep_scale(seed, 0, B * NH * L * L, p, bug)).reshape(B, NH, L, L)
    return torch.as_tensor(np.stack([hash_keep_scale(seed, bh * L * L, L * L, p, bug) for bh in heads])).reshape(len(heads), 1, L, L)


# ----------------------------------------------------------------------------- the GEMM launcher, route by route (tests/test_gpu_gemm_routes.py)
# launch_gemm of csrc/gemm.hip through ops.gemm on buffers of the test's own, every route it can choose (the route log of
# zeggs_test_gemm_route_log says which one a call took), against the float64 product.  tests/test_gemm_oracle_cpu.py measures on
# the CPU what float32 itself costs at every case (the floors) and proves that the comparison is sharp (GEMM_BUGS).
GEMM_CANARY_TAIL = 4096         # floats behind every output (and one float in front of it in the "odd" variant)
GEMM_CANARY = 1234.5
GEMM_VARIANTS = ("aligned", "odd")      # odd: every base pointer one float past a 16-byte boundary, odd leading dimensions of A and B
GEMM_BUGS = ("last_ktile", "k_term", "segment_twice", "edge_row", "bias_shift", "act_before_bias", "beta_on_partials",
             "batch_neighbour_A", "conv_no_overlap", "alpha_omitted")
GEMM_SPLITTING = ("m32-split", "mid-split", "streamk-direct", "streamk-lds-128x128", "streamk-lds-256x128", "splitk")
_T64, _M32 = ("tile-64x64", 1, 64, 64), ("m32", 1, 32, 128)
_SK128, _SK256 = ("streamk-lds-128x128", 0, 128, 128), ("streamk-lds-256x128", 0, 256, 128)


def _gemm_case(M, N, K, layout, route, fixed, **kw):
    """One row of the matrix.  route / fixed: (route name, splitk, BM, BN) the log must show with default routing / inside
    ops.fixed_order_gemms(); no_mid / no_streamk: the same with the option gemm_mid_split / gemm_streamk at 0 (None: not run).
    lda: the conv form, A(m, k) = xp[m lda + k] with lda < K (overlapping rows).  sample: floors and mutations over gemm_sample_rows only."""
    c = dict(M=M, N=N, K=K, layout=layout, route=route, fixed=fixed, alpha=1.0, beta=0.0, bias=False, act=0, ldc=None, nbatch=1,
             lda=None, no_mid=None, no_streamk=None, sample=False)
    assert not set(kw) - set(c), kw
    c.update(kw)
    c["id"] = (f"{M}x{N}x{K}-{layout}" + (f"-x{c['nbatch']}" if c["nbatch"] > 1 else "") + (f"-conv{c['lda']}" if c["lda"] else "") +
               (f"-a{c['alpha']:g}" if c["alpha"] != 1.0 else "") + (f"-b{c['beta']:g}" if c["beta"] else "") +
               ("-bias" if c["bias"] else "") + ("", "-elu", "-relu")[c["act"]] + (f"-ldc{c['ldc']}" if c["ldc"] else ""))
    # which mutations of GEMM_BUGS apply: the first three rows everywhere; the others where the case has what they break
    split = route[0] in GEMM_SPLITTING
    c["bugs"] = tuple(b for b, on in (
        ("last_ktile", True), ("k_term", True), ("edge_row", True), ("segment_twice", split), ("bias_shift", c["bias"]),
        ("act_before_bias", c["bias"] and c["act"] != 0), ("beta_on_partials", split and c["beta"] != 0.0),
        ("batch_neighbour_A", c["nbatch"] > 1), ("conv_no_overlap", c["lda"] is not None), ("alpha_omitted", c["alpha"] != 1.0)) if on)
    return c


# The smallest shapes that reach each route (launch_gemm's rules replayed by hand; the route log on the device is the arbiter).
# act: 0 none, 1 ELU, 2 ReLU.  Layouts: NN A [M, K] B [K, N]; NT B [N, K]; TN A [K, M].
GEMM_CASES = (
    _gemm_case(5, 70, 250, "TN", ("m32-split", 4, 32, 128), _M32),
    _gemm_case(31, 130, 257, "NT", ("m32-split", 4, 32, 128), _M32, alpha=0.5, bias=True, act=1, ldc=135),     # fill + bias pass on strided rows
    _gemm_case(32, 129, 1000, "TN", ("m32-split", 15, 32, 128), _M32, beta=1.0),                               # no fill: onto a loaded C
    _gemm_case(17, 200, 300, "TN", _M32, _M32, alpha=2.0, beta=0.5),
    _gemm_case(33, 1000, 67, "NT", ("skinny", 1, 48, 16), ("skinny", 1, 48, 16), bias=True, act=1),
    _gemm_case(450, 200, 250, "NN", ("mid-split", 2, 64, 64), _T64, no_mid=_T64),
    _gemm_case(449, 193, 251, "NT", ("mid-split", 2, 64, 64), _T64, no_mid=_T64, bias=True, act=2, ldc=197),   # bias pass, ld > N
    _gemm_case(450, 200, 250, "TN", ("mid-split", 2, 64, 64), _T64, no_mid=_T64, beta=1.0),                    # accumulating
    _gemm_case(100, 130, 300, "NN", ("mid-split", 3, 64, 64), _T64, no_mid=_T64, nbatch=6, bias=True, act=1),  # batched flat C: bsC = M ldc
    _gemm_case(512, 256, 270, "NN", ("mid-split", 2, 64, 64), _T64, no_mid=_T64, lda=90),                      # overlapping rows, 3 taps
    _gemm_case(130, 70, 1266, "NN", _SK128, _T64, no_streamk=("splitk", 5, 128, 128)),
    _gemm_case(257, 129, 1281, "NT", _SK128, _T64, no_streamk=("splitk", 5, 128, 128), beta=1.0),
    _gemm_case(300, 128, 1290, "NN", _SK128, _T64, no_streamk=("splitk", 5, 128, 128), lda=430),               # conv_flat's form
    _gemm_case(130, 70, 1267, "TN", _SK128, _T64, no_streamk=("splitk", 5, 128, 128)),                         # odd K: direct refuses
    _gemm_case(130, 70, 1266, "TN", ("streamk-direct", 0, 128, 128), _T64, no_streamk=("splitk", 5, 128, 128)),
    _gemm_case(3072, 2048, 1280, "NN", _SK256, ("half", 1, 128, 64), no_streamk=("splitk", 5, 128, 128), sample=True),
    _gemm_case(3000, 2049, 1270, "NN", _SK256, ("tile-128x128", 1, 128, 128), no_streamk=("splitk", 5, 128, 128), sample=True),
    _gemm_case(513, 129, 1262, "NN", ("splitk", 4, 128, 128), _T64, no_streamk=("splitk", 4, 128, 128)),
    _gemm_case(40, 1000, 1100, "TN", ("splitk", 4, 64, 64), _T64, no_streamk=("splitk", 4, 64, 64)),           # not "big": M <= 64
    _gemm_case(1000, 40, 1100, "NN", ("splitk", 4, 64, 64), _T64, no_streamk=("splitk", 4, 64, 64)),
    _gemm_case(2100, 2048, 40, "NT", ("half", 1, 128, 64), ("half", 1, 128, 64), bias=True, act=1),
    _gemm_case(1030, 1800, 24, "NN", ("tile-128x128", 1, 128, 128), ("tile-128x128", 1, 128, 128), bias=True, act=2),   # ragged edges
    _gemm_case(200, 70, 33, "NN", _T64, _T64),
)
GEMM_ROUTES_COVERED = ("skinny", "m32-split", "m32", "mid-split", "streamk-direct", "streamk-lds-128x128", "streamk-lds-256x128",
                       "splitk", "half", "tile-128x128", "tile-64x64")
# THE BOUNDS.  Per case: 4 x the floor, the largest error (gemm_error) of the FLOAT32 evaluation of gemm_oracle -- one running sum
# over k per element -- against its float64 evaluation, the larger of the two alignment variants' (the two 6-million-element cases:
# over gemm_sample_rows).  The margin of 4 is for the different but equally long summation orders of the matrix-core k-pairs, the
# split segments and the atomics.  Floors as tests/test_gemm_oracle_cpu.py::test_float32_floors measures them (it asserts
# 2 x floor <= bound <= 8 x floor); nothing was taken from the device's output.
GEMM_FLOORS = {
    "5x70x250-TN": 1.4e-07,                             # measured 1.34e-07 (aligned) 1.21e-07 (odd)
    "31x130x257-NT-a0.5-bias-elu-ldc135": 1.8e-07,      # measured 1.74e-07 (aligned) 1.57e-07 (odd)
    "32x129x1000-TN-b1": 2.1e-07,                       # measured 2.06e-07 (aligned) 2.03e-07 (odd)
    "17x200x300-TN-a2-b0.5": 2e-07,                     # measured 1.71e-07 (aligned) 1.97e-07 (odd)
    "33x1000x67-NT-bias-elu": 2.2e-07,                  # measured 2.18e-07 (aligned) 2.08e-07 (odd)
    "450x200x250-NN": 3.2e-07,                          # measured 3.17e-07 (aligned) 2.6e-07 (odd)
    "449x193x251-NT-bias-relu-ldc197": 2.6e-07,         # measured 2.5e-07 (aligned) 2.51e-07 (odd)
    "450x200x250-TN-b1": 2.4e-07,                       # measured 2.14e-07 (aligned) 2.3e-07 (odd)
    "100x130x300-NN-x6-bias-elu": 3.2e-07,              # measured 2.57e-07 (aligned) 3.16e-07 (odd)
    "512x256x270-NN-conv90": 3.1e-07,                   # measured 2.98e-07 (aligned) 3.09e-07 (odd)
    "130x70x1266-NN": 2.6e-07,                          # measured 2.3e-07 (aligned) 2.52e-07 (odd)
    "257x129x1281-NT-b1": 2.6e-07,                      # measured 2.51e-07 (aligned) 2.21e-07 (odd)
    "300x128x1290-NN-conv430": 2.9e-07,                 # measured 2.4e-07 (aligned) 2.87e-07 (odd)
    "130x70x1267-TN": 2.7e-07,                          # measured 1.9e-07 (aligned) 2.6e-07 (odd)
    "130x70x1266-TN": 2.2e-07,                          # measured 2.13e-07 (aligned) 1.77e-07 (odd)
    "3072x2048x1280-NN": 3e-07,                         # measured 2.72e-07 (aligned) 2.91e-07 (odd)
    "3000x2049x1270-NN": 3e-07,                         # measured 2.92e-07 (aligned) 2.51e-07 (odd)
    "513x129x1262-NN": 2.9e-07,                         # measured 2.81e-07 (aligned) 2.52e-07 (odd)
    "40x1000x1100-TN": 2.4e-07,                         # measured 2.38e-07 (aligned) 2.13e-07 (odd)
    "1000x40x1100-NN": 2.5e-07,                         # measured 2.21e-07 (aligned) 2.44e-07 (odd)
    "2100x2048x40-NT-bias-elu": 4.1e-07,                # measured 4.02e-07 (aligned) 3.4e-07 (odd)
    "1030x1800x24-NN-bias-relu": 2.9e-07,               # measured 2.84e-07 (aligned) 2.84e-07 (odd)
    "200x70x33-NN": 2.1e-07,                            # measured 1.95e-07 (aligned) 2.02e-07 (odd)
}
GEMM_BOUND = {k: 4.0 * v for k, v in GEMM_FLOORS.items()}
_GEMM_DATA, _GEMM_TRUTH = {}, {}


def gemm_case_id(case):
    return case["id"]


def gemm_sample_rows(case):
    """the rows the floor of a `sample` case is taken on: every 128-row tile edge with its neighbours, every 64th row, the last"""
    M = case["M"]
    rows = {M - 1} | set(range(0, M, 64)) | {r + d for r in range(0, M, 128) for d in (-1, 0, 1)}
    return torch.as_tensor(sorted(r for r in rows if 0 <= r < M))


def _gemm_odd(n, odd):
    return n if not odd else n + 1 if n % 2 == 0 else n + 2


def gemm_case_data(case, variant="aligned"):
    """The buffers of one comparison, seeded, on the host (cached; leave them unchanged) -> dict: A, B flat float32 buffers with
    `off` floats in front of the operand, sa = (sam, sak), sb = (sbk, sbn), bs = (bsA, bsB, bsC) in elements, bias [N] or None,
    C the flat output buffer as the device gets it -- `off` canary floats, nbatch M rows of ldc (the N result columns NaN when
    beta = 0, else the loaded C0; the padding columns canary), GEMM_CANARY_TAIL canary floats -- ldc, and C0 [nbatch, M, N] or None."""
    key = (case["id"], variant)
    if key in _GEMM_DATA:
        return _GEMM_DATA[key]
    assert variant in GEMM_VARIANTS, variant
    odd = variant == "odd"
    off = 1 if odd else 0
    M, N, K, nb, lay = case["M"], case["N"], case["K"], case["nbatch"], case["layout"]
    gen = torch.Generator().manual_seed(9000 + 2 * [c["id"] for c in GEMM_CASES].index(case["id"]) + off)
    if case["lda"] is not None:
        assert lay == "NN"
        lda = case["lda"] + off
        sa, span_a = (lda, 1), (M - 1) * lda + K
    elif lay == "TN":
        lda = _gemm_odd(M, odd)
        sa, span_a = (1, lda), K * lda
    else:
        lda = _gemm_odd(K, odd)
        sa, span_a = (lda, 1), M * lda
    if lay == "NT":
        ldb = _gemm_odd(K, odd)
        sb, span_b = (1, ldb), N * ldb
    else:
        ldb = _gemm_odd(N, odd)
        sb, span_b = (ldb, 1), K * ldb
    ldc = case["ldc"] or N
    A = torch.randn(off + nb * span_a, generator=gen)
    B = torch.randn(off + nb * span_b, generator=gen)
    bias = torch.randn(N, generator=gen) if case["bias"] else None
    C0 = torch.randn(nb, M, N, generator=gen) if case["beta"] != 0.0 else None
    C = torch.full((off + nb * M * ldc + GEMM_CANARY_TAIL,), GEMM_CANARY)
    body = C[off:off + nb * M * ldc].view(nb, M, ldc)
    body[:, :, :N] = C0 if C0 is not None else float("nan")
    d = dict(A=A, B=B, C=C, C0=C0, bias=bias, off=off, sa=sa, sb=sb, ldc=ldc,
             bs=(span_a, span_b, M * ldc) if nb > 1 else (0, 0, 0), span=(span_a, span_b))
    _GEMM_DATA[key] = d
    return d


def gemm_operands(case, variant="aligned", dtype=torch.float64, bug=None):
    """A [nbatch, M, K], B [nbatch, K, N] as the kernel addresses them in the buffers of gemm_case_data, contiguous in `dtype`"""
    d = gemm_case_data(case, variant)
    M, N, K, nb = case["M"], case["N"], case["K"], case["nbatch"]
    (sam, sak), (sbk, sbn), (span_a, span_b) = d["sa"], d["sb"], d["span"]
    A = torch.as_strided(d["A"], (nb, M, K), (span_a, sam, sak), d["off"]).to(dtype).contiguous()
    B = torch.as_strided(d["B"], (nb, K, N), (span_b, sbk, sbn), d["off"]).to(dtype).contiguous()
    if bug == "conv_no_overlap":        # every tap reads the row's own first lda values: the rows do not reach into the next ones
        A = A[:, :, torch.arange(K) % sam].contiguous()
    if bug == "batch_neighbour_A":      # entry 1 reads entry 0's A
        A[1] = A[0]
    return A, B


def _gemm_segment(case):
    """the k-range [k0, k1) of the second split segment, as gemm_kernel cuts the 16-wide k-tiles (stream-K: in thirds)"""
    nkt = (case["K"] + 15) // 16
    S = case["route"][1] if case["route"][1] > 1 else 3
    return 16 * (nkt * 1 // S), min(case["K"], 16 * (nkt * 2 // S))


def gemm_oracle(case, dtype=torch.float64, variant="aligned", bug=None, rows=None):
    """act(alpha A B + bias + beta C0) of one case in `dtype` -> [nbatch, M (or len(rows)), N].  float64: the truth (torch.matmul);
    float32: one running sum over k per element, every product and every sum rounded (the floor).  rows: only these rows of M.
    bug: one of GEMM_BUGS, a model of one wrong line of the launcher or a kernel (the negative controls)."""
    assert bug is None or bug in GEMM_BUGS, bug
    d = gemm_case_data(case, variant)
    M, N, K = case["M"], case["N"], case["K"]
    A, B = gemm_operands(case, variant, dtype, bug)
    sel = torch.arange(M) if rows is None else rows
    A = A[:, sel].clone()
    if bug == "last_ktile":
        A[:, :, 16 * ((K - 1) // 16):] = 0
    if bug == "k_term":
        A[:, :, K // 2] = 0
    if bug == "segment_twice":
        k0, k1 = _gemm_segment(case)
        A[:, :, k0:k1] *= 2
    if dtype == torch.float64:
        acc = torch.matmul(A, B)
    else:
        acc = torch.zeros(A.shape[0], A.shape[1], N, dtype=dtype)
        for k in range(K):
            acc += A[:, :, k:k + 1] * B[:, k:k + 1, :]
    alpha = 1.0 if bug == "alpha_omitted" else case["alpha"]
    act = (lambda t: t, torch.nn.functional.elu, torch.relu)[case["act"]]
    v = acc * alpha if alpha != 1.0 else acc
    bias = None if d["bias"] is None else d["bias"].to(dtype)
    if bias is not None and bug == "bias_shift":
        bias = bias.roll(1)
    if bias is not None and bug != "act_before_bias":
        v = v + bias
    if case["beta"] != 0.0:
        c0 = d["C0"][:, sel].to(dtype) * case["beta"]
        v = v + c0 + (c0 if bug == "beta_on_partials" else 0)
    v = act(v)
    if bias is not None and bug == "act_before_bias":
        v = v + bias
    if bug == "edge_row":       # the first row of the last row tile (the last row where there is one tile) holds its upper neighbour's
        BM = case["route"][2]
        r = BM * ((M - 1) // BM) if M > BM else M - 1
        pos = {int(x): i for i, x in enumerate(sel)}
        v[:, pos[r]] = v[:, pos[r - 1]]
    return v


def gemm_denominator(case, variant="aligned", rows=None):
    """|alpha| sum_k |a_mk b_kn| + |beta c0_mn| + |bias_n| in float64: what an element's error is measured against"""
    d = gemm_case_data(case, variant)
    A, B = gemm_operands(case, variant)
    if rows is not None:
        A = A[:, rows]
    den = abs(case["alpha"]) * torch.matmul(A.abs(), B.abs())
    if d["bias"] is not None:
        den = den + d["bias"].double().abs()
    if case["beta"] != 0.0:
        den = den + abs(case["beta"]) * (d["C0"] if rows is None else d["C0"][:, rows]).double().abs()
    return den


def gemm_error(got, ref, den):
    """max over ALL elements of |got - ref| / den (per element: a wrong element of small magnitude cannot hide behind a large one)
    -> (error, (batch, row, column) where it fell).  A NaN in `got` is an infinite error."""
    e = (got.double() - ref).abs() / den
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    i = int(e.argmax())
    return float(e.flatten()[i]), tuple(int(x) for x in np.unravel_index(i, tuple(e.shape)))


def gemm_truth(case, variant="aligned"):
    """(float64 oracle, denominator) over every element, computed once per case and variant"""
    key = (case["id"], variant)
    if key not in _GEMM_TRUTH:
        _GEMM_TRUTH[key] = (gemm_oracle(case, torch.float64, variant), gemm_denominator(case, variant))
    return _GEMM_TRUTH[key]


def gemm_floor(case, variant="aligned"):
    """what the float32 running sum loses at this case, in the measure of gemm_error (`sample` cases: over gemm_sample_rows)"""
    rows = gemm_sample_rows(case) if case["sample"] else None
    ref, den = gemm_oracle(case, torch.float64, variant, rows=rows), gemm_denominator(case, variant, rows)
    return gemm_error(gemm_oracle(case, torch.float32, variant, rows=rows), ref, den)[0]


# ----------------------------------------------------------------------------- live serving at other dimensions
# (tests/test_gpu_live_dims.py on the device, tests/test_live_encoder_oracle_cpu.py on the host)
# The incremental speech encoder (csrc/live.hip) takes any F, any odd KW and any H, O that are multiples of 4 dividing 512; FRP =
# 512 / O output frames and FA = 512 / H feature rows go through one pass of its workgroup.  `bs`: the largest burst in steady
# state; the ring holds D = KW - 1 + bs frames, the least that admits it; `long`: the longest row, > 2 D frames.
LIVE_KERNEL_CASES = (
    dict(id="r64-81-64-64-31", F=81, H=64, O=64, KW=31, R=64, bs=23, long=150),     # every row active, 64 lengths
    dict(id="81-128-32-31", F=81, H=128, O=32, KW=31, R=3, bs=17, long=150),        # H != O, FRP = 16, FA = 4
    dict(id="81-32-128-31", F=81, H=32, O=128, KW=31, R=3, bs=23, long=150),        # FRP = 4, FA = 16
    dict(id="20-512-64-3", F=20, H=512, O=64, KW=3, R=3, bs=9, long=60),            # FA = 1
    dict(id="20-16-512-5", F=20, H=16, O=512, KW=5, R=3, bs=7, long=40),            # FRP = 1
    dict(id="3-4-4-1", F=3, H=4, O=4, KW=1, R=3, bs=129, long=600),                 # KW = 1, FRP = FA = 128
    dict(id="81-256-16-29", F=81, H=256, O=16, KW=29, R=3, bs=33, long=140),        # 64 144 bytes of LDS
)
LIVE_LDS_REFUSED = (81, 256, 16, 31)                                                # 66 192 bytes


def live_case_depth(case):
    return case["KW"] - 1 + case["bs"]


def live_case_lens(case):
    """row lengths.  R = 64: 1, 2, half, half + 1, KW - 1, KW and 58 other lengths up to case["long"], all different; R = 3: one of
    those six (by the case's position in the table), a middle row, the long row"""
    KW, half = case["KW"], (case["KW"] - 1) // 2
    short = sorted({n for n in (1, 2, half, half + 1, KW - 1, KW) if n >= 1})
    if case["R"] == 3:
        i = [c["id"] for c in LIVE_KERNEL_CASES].index(case["id"])
        FRP = 512 // case["O"]        # the middle row: long enough for the bursts 1, FRP - 1, FRP, FRP + 1 and bs, whole
        return [short[i % len(short)], max(live_case_depth(case) * 3 // 2 + 1, 3 * FRP + case["bs"] + 6), case["long"]]
    rng = np.random.default_rng(64)
    rest = [int(n) for n in rng.permutation(np.arange(3, case["long"])) if int(n) not in short][:case["R"] - len(short) - 1]
    lens = short + rest + [case["long"]]
    order = rng.permutation(len(lens))
    return [lens[i] for i in order]


def live_schedule(case):
    """The seeded burst schedule of a case -> dict(lens, D, feat_ld, out_ld, calls); calls[c][r] = (n_ring, k0, last, n_new,
    n_out, feat_off), the record of row r in launch c ((0, 0, -1, 0, 0, 0): the row takes no part -- not started yet or finished).

    Every row walks the same pattern of (burst, output policy) from its own starting point, begins at its own call, and what the
    pattern asks is cut to what the ring admits: a burst never overwrites a frame that a pending output still reads.  Bursts: 1,
    FRP - 1, FRP, FRP + 1, bs and D (whole, at a row's start: the largest the ring admits; cut to bs later); policies: all that is
    ready (-1), none (0: ring fill only, and the call after it brings no frames: output from the ring alone), at most n (> 0).
    Rows of at most KW frames arrive and end in ONE call.  feat_off = (call + row) % 4, and feat_ld / out_ld are the largest
    feat_off + n_new / n_out of the schedule: both limits are reached."""
    KW, R, D = case["KW"], case["R"], live_case_depth(case)
    half, FRP, bs = (KW - 1) // 2, 512 // case["O"], case["bs"]
    lens = live_case_lens(case)
    pattern = [(1, -1), (FRP - 1, -1), (FRP, -1), (FRP + 1, -1), (bs, -1), (2, 0), (0, -1), (D, -1), (3, 0), (0, 2), (bs, -1),
               (0, -1), (1, -1), (FRP + 1, 0), (0, -1), (2 * FRP + 1, -1)]
    rng = np.random.default_rng(1000 + len(case["id"]) + case["F"] + case["H"] + case["O"] + KW)
    start = [int(rng.integers(0, 6)) for _ in range(R)]
    phase = [7 if n > 2 * D and r % 2 == 0 else int(rng.integers(0, len(pattern))) for r, n in enumerate(lens)]   # 7: D at the start
    if R == 3:
        phase[1] = 0
    n_ring, done, step = [0] * R, [0] * R, [0] * R
    calls, c = [], 0
    idle = (0, 0, -1, 0, 0, 0)
    while any(done[r] < lens[r] for r in range(R)):
        recs = []
        for r, n in enumerate(lens):
            if c < start[r] or done[r] == n:
                recs.append(idle)
                continue
            b, pol = pattern[(phase[r] + step[r]) % len(pattern)]
            step[r] += 1
            if n <= KW:
                b, pol = n, -1                                           # delivered and ended in one call: every tap replicates
            room = D - n_ring[r] + max(0, done[r] - half)                # frames that fit without overwriting a frame still to be read
            n_new = max(0, min(b, n - n_ring[r], D, room))
            total = n_ring[r] + n_new
            ready = (n if total == n else max(done[r], total - half)) - done[r]
            n_out = ready if pol < 0 else min(pol, ready)
            if n_new == 0 and n_out == 0:
                n_out = ready
            if n_new == 0 and n_out == 0:                                # nothing pending: room >= D - KW + 1 >= 1
                n_new = 1
                total = n_ring[r] + 1
                n_out = (n if total == n else max(done[r], total - half)) - done[r]
            recs.append((n_ring[r], done[r], n - 1 if total == n else -1, n_new, n_out, (c + r) % 4))
            n_ring[r], done[r] = total, done[r] + n_out
        calls.append(recs)
        c += 1
        assert c < 4000
    return dict(lens=lens, D=D, calls=calls, feat_ld=max(rec[5] + rec[3] for recs in calls for rec in recs),
                out_ld=max(rec[4] for recs in calls for rec in recs))


def live_case_nets(case):
    """seeded Conv1d(F, H, 1), Conv1d(H, O, KW), Linear(O, O) on a plain namespace: what ops.LiveSpeech reads"""
    import types
    torch.manual_seed(SEED + case["F"] + case["H"] + case["O"] + case["KW"])
    nn = torch.nn
    return types.SimpleNamespace(layer0=nn.Conv1d(case["F"], case["H"], 1), layer1=nn.Conv1d(case["H"], case["O"], case["KW"]),
                                 layer2=nn.Linear(case["O"], case["O"]))


def live_case_weights(net):
    return {f"layer{i}.{k}": getattr(getattr(net, f"layer{i}"), k).detach() for i in range(3) for k in ("weight", "bias")}


_LIVE_DATA = {}


def live_case_data(case):
    """-> dict(net, mean, std [F] float32, feats: per row [n, F] float32 un-normalised, sched, ref: per row the float64 whole-row
    oracle [n, O]), computed once per case.  mean ~ N(0, 1) / 4, std in [0.5, 2]: (x - mean) / std in float32 loses about one unit
    of roundoff of |x| / std <= 4.5, nothing to cancellation."""
    if case["id"] not in _LIVE_DATA:
        from oracle import nets as onets
        net, sched = live_case_nets(case), live_schedule(case)
        rng = np.random.default_rng(SEED + 1)
        mean = torch.as_tensor((rng.standard_normal(case["F"]) / 4).astype(np.float32))
        std = torch.as_tensor(rng.uniform(0.5, 2.0, case["F"]).astype(np.float32))
        feats = [torch.as_tensor(rng.standard_normal((n, case["F"])).astype(np.float32)) * std + mean for n in sched["lens"]]
        w = {k: v.double() for k, v in live_case_weights(net).items()}
        with torch.no_grad():
            ref = [onets.speech_encoder(w, ((f.double() - mean.double()) / std.double())[None])[0] for f in feats]
        _LIVE_DATA[case["id"]] = dict(net=net, mean=mean, std=std, feats=feats, sched=sched, ref=ref)
    return _LIVE_DATA[case["id"]]


def live_feat_block(data, c):
    """the sliding feature block of launch c, [R, feat_ld, F]: row r's new frames n_ring .. n_ring + n_new - 1 from row feat_off
    on, 1e3 everywhere else (a frame read from the wrong place is far outside the bound)"""
    s = data["sched"]
    blk = torch.full((len(s["lens"]), s["feat_ld"], data["mean"].numel()), 1e3)
    for r, (n_ring, _, _, n_new, _, off) in enumerate(s["calls"][c]):
        blk[r, off:off + n_new] = data["feats"][r][n_ring:n_ring + n_new]
    return blk


# ---- the yardstick of tests/test_gpu_live.py, shared with tests/test_gpu_live_dims.py: the offline rollout and its bound
LIVE_DEV = "cuda:0"
LIVE_KEYS = ("pose", "rpos", "rrot")
LIVE_CONF = dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True, normalize_mel_bins=True,
                 normalize_range=True, min_clipping=1e-5, sampling_rate=16000, mel_fmin=20, mel_fmax=7600,
                 n_mel_channels=80, filter_length=800, hop_length=200, resample_method="linear", normalize_loudness=False)
_LIVE_CACHE = {}


def _live_cached(key, make):
    if key not in _LIVE_CACHE:
        _LIVE_CACHE[key] = make()
    return _LIVE_CACHE[key]


def live_nets():
    def make():
        se, de, _ = build_nets()
        return se.to(LIVE_DEV).eval(), de.to(LIVE_DEV).eval()
    return _live_cached("nets", make)


def live_stats():
    return _live_cached("stats", lambda: {k: torch.as_tensor(np.asarray(v), dtype=torch.float32, device=LIVE_DEV)
                                          for k, v in synth.make_stats().items()})


def live_first(seed):
    from zeggs import anim
    return _live_cached(("first", seed), lambda: anim.preprocess_animation(synth.make_bvh_clip(8, seed=seed), LIVE_DEV))


def live_wav(nsamp, seed):
    return _live_cached(("wav", nsamp, seed), lambda: synth.synth_wav(nsamp, seed=seed).astype(np.float32) / 32768.0)


def live_style(seed):
    return torch.randn(1, 64, device=LIVE_DEV, generator=torch.Generator(LIVE_DEV).manual_seed(seed)) * 0.5


def live_offline(wav, first, style_rows):
    """the offline path: style_rows [1, 64] (constant) or [n_frames, 64] -> (pose, rpos, rrot) [n_frames, .]"""
    from zeggs import audio, ops
    se, de = live_nets()
    st = live_stats()
    n_frames = audio.n_anim_frames(len(wav))
    feats = torch.as_tensor(audio.preprocess_audio(wav, 60, n_frames, LIVE_CONF, ["mel_spec", "energy"]), device=LIVE_DEV)
    with torch.no_grad():
        sp = se(((feats[None] - st["audio_input_mean"]) / st["audio_input_std"]).contiguous())
        f32 = lambda a: a[0:1].to(torch.float32).contiguous()  # noqa: E731
        rp, rr, rv, rw, lp, _, lt, lv, lw = first[:9]
        pose0 = torch.cat([f32(x).reshape(1, -1) for x in (rv, rw, lp, lt, lv, lw)], dim=1)
        gaze = f32(first[14]).repeat(n_frames, 1)[None].contiguous()
        style = style_rows if style_rows.shape[0] == n_frames else style_rows.repeat(n_frames, 1)
        ref = ops.decoder_core(de, pose0, f32(rp), f32(rr), gaze, sp, style[None].contiguous(), st["anim_input_mean"],
                               st["anim_input_std"], st["anim_output_mean"], st["anim_output_std"], synth.DT)
    return tuple(r[0] for r in ref)


def live_offline_cached(nsamp, wseed, fseed, sseed):
    return _live_cached(("offline", nsamp, wseed, fseed, sseed),
                        lambda: live_offline(live_wav(nsamp, wseed), live_first(fseed), live_style(sseed)))


def live_server(rows, tick, **kw):
    from zeggs import live
    se, de = live_nets()
    return live.LiveServer(se, de, live_stats(), LIVE_CONF, synth.DT, rows=rows, tick=tick, **kw)


def live_cat(parts):
    parts = [p for p in parts if p]
    return {k: torch.cat([p[k] for p in parts], dim=0) for k in LIVE_KEYS}


def live_err(got, ref):
    e = {}
    for k, r in zip(LIVE_KEYS, ref):
        assert got[k].shape == r.shape, (k, got[k].shape, r.shape)
        assert torch.isfinite(got[k]).all(), k
        e[k] = float((got[k] - r).abs().max())
    return e


def live_bound(srv):
    """1e-4 where the rows rode the sweep, 5e-5 otherwise -- and which of the two ran is asserted, not assumed"""
    from zeggs import ops
    path = ops.batch_last_path()
    assert path == ("persistent" if srv.bd.sweep else "stage"), (path, srv.bd.sweep)
    return 1e-4 if path == "persistent" else 5e-5


# ----------------------------------------------------------------------------- animation kernels (tests/test_gpu_anim_dims.py)
# Rigs, exemplar clips and decoder-side rows for csrc/anim.hip at other skeletons, frame counts and rotations than the one rig of
# tests/test_gpu_parity.py.  tests/test_anim_oracle_cpu.py proves on the CPU that every case below meets the conditions it was built
# for (on the oracle's intermediates) and that the comparison is sharp (negative controls).
ANIM_FEATURES = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "lrot", "ltxy", "lvel", "lvrt", "cpos", "crot", "ctxy", "cvel",
                 "cvrt", "gaze_pos", "gaze_dir")
ANIM_F64_BOUND, ANIM_F32_BOUND = 1e-9, 1e-6       # tests/test_gpu_parity.py::test_anim_features_vs_oracle_and_reference
BVH_POS_BOUND, BVH_QUAT_BOUND, BVH_ANGLE_BOUND = 1e-9, 1e-9, 1e-9      # ::test_pose_to_bvh_vs_oracle_and_reference; degrees
ANIM_ORDER_ZYX, ANIM_ORDER_XZY = 6, 24            # anim_math.h ORDER_ZYX / ORDER_XZY (0 stands for zyx)


class _OneJoint(list):
    """the names of the one-joint rig: Hips, Spine2 and Head are all joint 0 (the raw ABI takes it, the Python wrapper cannot)"""

    def index(self, name, *a):
        return 0


def _anim_rigs():
    def named(parents, **at):
        names = [f"joint_{i}" for i in range(len(parents))]
        for n, i in at.items():
            names[i] = n
        return parents, names

    def tree(n_fixed, J, seed):
        rng = np.random.default_rng(seed)
        return [int(rng.integers(0, i)) for i in range(n_fixed, J)]

    spine = [-1, 0, 1, 2, 3]                                       # Hips, Spine, Spine2, Neck, Head
    j24 = [-1, 0, 1, 2, 3, 4, 5,                                   # Root, Hips, Spine, Spine1, Spine2, Neck, Head
           1, 7, 8, 1, 10, 11,                                     # two legs below Hips
           4, 13, 14, 15, 4, 17, 18, 19,                           # two arms below Spine2
           6, 0, 22]                                               # a head end, a prop of two joints below Root
    return {
        "j3": named([-1, 0, 1], Hips=0, Spine2=1, Head=2),
        "j24-root": named(j24, Root=0, Hips=1, Spine2=4, Head=6),
        "j64": named(spine + tree(5, 64, 64), Hips=0, Spine2=2, Head=4),
        "j65": named(spine + tree(5, 64, 64) + [40], Hips=0, Spine2=2, Head=4),       # j64 and one joint in the unroll's second block
        "j130": named([-1] + list(range(44)) + tree(45, 130, 130), Hips=0, Spine2=20, Head=44),     # Head 44 levels deep
        "j1": ([-1], _OneJoint(["Hips"])),
    }


ANIM_RIGS = _anim_rigs()
# every features case of tests/test_gpu_anim_dims.py: (rig, N, variant); variant: {} | static_head | order | dt
ANIM_CASES = ([(r, 10, {}) for r in ANIM_RIGS] +
              [(r, N, {}) for r in ("j3", "j24-root") for N in (4, 5, 8, 9, 17, 64, 65)] +
              [(r, 17, {}) for r in ("j65", "j130")] +
              [("j24-root", N, dict(static_head=True)) for N in (9, 10)] +
              [("j24-root", 10, dict(order=o)) for o in ("xyz", "yzx", "xzy")] +
              [("j3", 10, dict(dt=dt)) for dt in (1.0 / 30.0, 1.0 / 120.0)])


def anim_case_id(case):
    rig, N, var = case
    return "-".join([rig, f"N{N}"] + [k if v is True else (f"dt{round(1 / v)}" if k == "dt" else str(v)) for k, v in var.items()])


def _ancestors(parents, j):
    out = []
    while parents[j] >= 0:
        j = parents[j]
        out.append(j)
    return out


def anim_roles(rig):
    """-> dict(hips, spine2, head, chain: the joints whose rotation reaches Hips, Spine2 or Head, sweep / alternate: the joints that
    carry a sign-flipping channel, static: the joint whose channels never change)"""
    parents, names = ANIM_RIGS[rig]
    J = len(parents)
    h, s, e = names.index("Hips"), names.index("Spine2"), names.index("Head")
    chain = sorted({h, s, e} | set(_ancestors(parents, h)) | set(_ancestors(parents, s)) | set(_ancestors(parents, e)))
    free = [j for j in range(J) if j not in chain]
    return dict(hips=h, spine2=s, head=e, chain=chain, static=s if J > 1 else None,
                sweep=[j for j in free if j % 4 in (1, 2)], alternate=[e] + [j for j in free if j % 4 == 3 or j == J - 1])


def anim_clip(rig, N, seed, order="zyx", dt=1.0 / 60.0, static_head=False):
    """A clip dict as synth.make_bvh_clip gives, for a rig of ANIM_RIGS: float64 Euler degrees in (-180, 180], channel order `order`.
      Hips      its yaw channel goes from -170 to +170 degrees over the clip, its other channels are 0 (165 where Hips has a parent,
                whose small rotations add to it, and on the one-joint rig): the facing direction stays 10 degrees off -z
      Head      its yaw goes from +175 to -150 degrees and its roll channel ALTERNATES between about +172 and -172 degrees: every raw
                dot product with the frame before is negative; where the roll is applied outside the yaw its half turn mirrors the yaw
                (the sweep runs the other way in the other orders), so Head's forward turns nearly twice about the vertical and the
                gaze candidates change sign in x and in z
      Spine2    (static) the same three angles in every frame
      others    smooth small motion; some (anim_roles: sweep) with a channel that advances ~95 degrees a frame through the wrap, some
                (alternate) with the alternating channel; the joints whose rotation reaches Hips, Spine2 or Head stay small
      positions offsets plus a smooth wobble of every joint, joint 0 travelling
    static_head: every joint between the root and Hips / Spine2 / Head keeps one pose and joint 0 its place: all N gaze candidates
    are the same three doubles."""
    parents, names = ANIM_RIGS[rig]
    J, R = len(parents), anim_roles(rig)
    rng = np.random.default_rng(seed)
    t = np.arange(N)
    u = t / (N - 1.0)
    ax = {c: order.index(c) for c in "xyz"}

    def smooth(shape, amp):
        f = rng.uniform(0.3, 1.5, shape)
        return amp * np.sin(2.0 * np.pi * f * u.reshape((N,) + (1,) * len(shape)) + rng.uniform(0, 2.0 * np.pi, shape))

    rot = smooth((J, 3), 9.0)
    for j in R["chain"]:
        rot[:, j] = smooth((3,), 2.0)
    for j in R["sweep"]:
        rot[:, j, j % 3] = (95.0 + 0.37 * j) * t + rng.uniform(0.0, 360.0) + rng.uniform(-3.0, 3.0, N)
    for j in R["alternate"]:
        rot[:, j, j % 3 if j != R["head"] else ax["z"]] = (1.0 - 2.0 * (t % 2)) * (172.0 - rng.uniform(0.0, 3.0, N))
    if J > 1:
        rot[:, R["head"], ax["y"]] = (1.0 if ax["z"] < ax["y"] else -1.0) * (175.0 - 325.0 * u)
        rot[:, R["head"], ax["x"]] = 0.0
        rot[:, R["static"]] = np.array([20.0, -35.0, 50.0])
    amp = 170.0 if R["hips"] == 0 and J > 1 else 165.0
    rot[:, R["hips"]] = 0.0
    rot[:, R["hips"], ax["y"]] = -amp + 2.0 * amp * u
    if J == 1:
        rot[:, 0, ax["z"]] = (1.0 - 2.0 * (t % 2)) * (172.0 - rng.uniform(0.0, 3.0, N))
    offsets = rng.normal(0.0, 6.0, (J, 3))
    offsets[:, 1] = np.abs(offsets[:, 1])
    offsets[0] = [0.0, 90.0, 0.0]
    pos = offsets[None] + smooth((J, 3), 0.4)
    pos[:, 0] += smooth((3,), 30.0) * np.array([1.0, 0.1, 1.0])
    if static_head:
        for j in R["chain"]:
            rot[:, j] = rot[N // 2, j]
            pos[:, j] = pos[N // 2, j]
    rot = 180.0 - (180.0 - rot) % 360.0               # into (-180, 180], as BVH files store the channels
    return dict(rotations=rot, positions=pos, offsets=offsets, parents=np.asarray(parents, np.int32), names=names, order=order,
                frametime=float(dt))


def anim_case_clip(case):
    rig, N, var = case
    return anim_clip(rig, N, seed=1000 * sorted(ANIM_RIGS).index(rig) + N, **var)


def anim_unroll_ranges(N):
    """the frames anim_unroll_k takes in its groups of eight and in its scalar tail"""
    g = 1 + 8 * ((N - 1) // 8)
    return range(1, g), range(g, N)


def anim_intermediates(clip):
    """what the conditions of a clip are stated on, from the oracle's own functions: d [N-1, J] raw dot products of consecutive
    frames, facing / look [N] angles (degrees from +z about y) of the projected Hips / Head forward, look_len [N] length of Head's
    forward before it is normalised, cand [N, 3] gaze candidates, rel_w [N-1, J] |w| of the unrolled frame-to-frame rotation"""
    from oracle import anim as oa
    names = clip["names"]
    raw = oa.q_from_euler(np.radians(clip["rotations"]), clip["order"])
    d = np.sum(raw[1:] * raw[:-1], axis=-1)
    lrot = oa.q_unroll(raw)
    grot, gpos = oa.q_fk(lrot, clip["positions"], clip["parents"])
    fwd = np.array([0.0, 0.0, 1.0])
    f = oa.q_mul_vec(grot[:, names.index("Hips")], fwd)
    l = oa.q_mul_vec(grot[:, names.index("Head")], fwd)
    lh = l * np.array([1.0, 0.0, 1.0])
    cand = gpos[:, names.index("Spine2")] * np.array([1.0, 0.0, 1.0]) + 100.0 * lh / np.linalg.norm(lh, axis=-1, keepdims=True)
    return dict(d=d, facing=np.degrees(np.arctan2(f[:, 0], f[:, 2])), look=np.degrees(np.arctan2(l[:, 0], l[:, 2])),
                look_len=np.linalg.norm(lh, axis=-1), cand=cand, rel_w=np.abs(oa.q_mul(lrot[1:], oa.q_inv(lrot[:-1]))[..., 0]))


def anim_oracle(clip, bug=None):
    from oracle import anim as oa
    return oa.preprocess_animation(clip, bug=bug)


def anim_errors(got, ref):
    """per feature array: max |got - ref| / (1 + |ref|): err <= bound is np.allclose with atol = rtol = bound"""
    out = {}
    for n, a, b in zip(ANIM_FEATURES, got, ref):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert a.shape == b.shape, (n, a.shape, b.shape)
        out[n] = float(np.max(np.abs(a - b) / (1.0 + np.abs(b)))) if np.isfinite(a).all() else float("inf")
    return out


def anim_bound(name):
    return ANIM_F32_BOUND if name in ("ltxy", "ctxy") else ANIM_F64_BOUND


# ---- decoder-side rows
def _q_to_xy(q):
    """unit quaternions -> two-axis rows [..., 2, 3]: the rotated x and y axes"""
    from oracle import anim as oa
    return np.stack([oa.q_mul_vec(q, np.array([1.0, 0.0, 0.0])), oa.q_mul_vec(q, np.array([0.0, 1.0, 0.0]))], axis=-2)


def _rows_from_quats(q, rng):
    """what the decoder emits for the rotations q: each row scaled by its own factor in [0.3, 3], the second sheared by 0.3 of the
    first, rounded to float32"""
    xy = _q_to_xy(q)
    x = xy[..., 0, :] * rng.uniform(0.3, 3.0, q.shape[:-1] + (1,))
    y = xy[..., 1, :] * rng.uniform(0.3, 3.0, q.shape[:-1] + (1,)) + 0.3 * x
    return np.stack([x, y], axis=-2).astype(np.float32)


def bvh_case(J, T, seed):
    """-> dict(root_pos [T, 3], root_rot [T, 4], lpos [T, J, 3], ltxy [T, J, 2, 3] float32, branch [T, J]: the branch of
    oracle.anim.q_from_xform each item takes).  Item i of the T J items belongs to group (i + seed) % 4: 0 rotations by up to 115 degrees about any axis
    (trace branch), 1 / 2 / 3 rotations by 150 ... 210 degrees about an axis near x / y / z, every fourth of those by 180 degrees exactly (there the
    trace formula divides by sqrt(tr + 1) = 0).  root_rot: general, norms 0.7 ... 1.3 (the decoder does not normalise)."""
    from oracle import anim as oa
    rng = np.random.default_rng(seed)
    n = T * J
    grp = (np.arange(n) + seed) % 4
    axis = np.where((grp > 0)[:, None], np.eye(3)[np.maximum(grp - 1, 0)] + 0.15 * rng.uniform(-1.0, 1.0, (n, 3)),
                    rng.standard_normal((n, 3)))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    ang = np.where(grp > 0, rng.uniform(150.0, 210.0, n), rng.uniform(-115.0, 115.0, n))      # trace = 1 + 2 cos(angle) > 0 below 120
    ang[((np.arange(n) // 4) % 4 == 0) & (grp > 0)] = 180.0
    q = oa.q_from_angle_axis(np.radians(ang), axis).reshape(T, J, 4)
    ltxy = _rows_from_quats(q, rng)
    rr = rng.standard_normal((T, 4))
    rr = rr / np.linalg.norm(rr, axis=-1, keepdims=True) * rng.uniform(0.7, 1.3, (T, 1))
    return dict(root_pos=rng.normal(0.0, 50.0, (T, 3)).astype(np.float32), root_rot=rr.astype(np.float32),
                lpos=rng.normal(0.0, 8.0, (T, J, 3)).astype(np.float32), ltxy=ltxy,
                branch=oa.xform_branch(oa.xform_from_xy(ltxy.astype(np.float64))))


BVH_START = (np.array([1.0, 2.0, 3.0]), np.array([0.6, 0.0, 0.8, 0.0]))      # the general start of test_pose_to_bvh_vs_oracle_and_reference
BVH_STARTS = dict(none=None, identity=(np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])), general=BVH_START)


def bvh_pole_case(order, k, seed=5):
    """rows whose middle Euler angle (zyx: the y angle, xzy: the z angle, the asin of quat.to_euler) is +-(90 - 10^-k) degrees, k = None:
    +-90 exactly; the other two angles random.  T = 8 frames of J = 3 joints; identity root with a float32 norm just above 1, so that
    joint 0 of the exact-pole rows has |sin| > 1 before the clamp.  -> bvh_case's dict + middle [T, J] the angle asked for"""
    from oracle import anim as oa
    rng = np.random.default_rng(seed + (0 if k is None else k))
    T, J = 8, 3
    build, mid = BVH_EULER_INVERSE[order][1], 1      # the composition quat.to_euler(order) inverts; its middle factor is the asin's
    e = rng.uniform(-180.0, 180.0, (T, J, 3))
    e[..., mid] = (1.0 - 2.0 * (np.arange(T * J).reshape(T, J) % 2)) * (90.0 - (0.0 if k is None else 10.0 ** -k))
    q = oa.q_from_euler(np.radians(e), build)
    if k is None:
        q[:, 0] = oa.q_from_euler(np.radians(e[:, 0] * (np.arange(3) == mid)), build)   # joint 0: the pole turn alone, w = +-component
    xy = _q_to_xy(q).astype(np.float32)
    rr = np.zeros((T, 4), np.float32)
    rr[:, 0] = np.nextafter(np.float32(1.0), np.float32(2.0)) if k is None else 1.0
    return dict(root_pos=np.zeros((T, 3), np.float32), root_rot=rr, lpos=rng.normal(0.0, 8.0, (T, J, 3)).astype(np.float32), ltxy=xy,
                middle=e[..., mid])


def bvh_raw_sin(case, order):
    """the UNCLAMPED argument of the asin of quat.to_euler per item (the oracle's quaternions, joint 0 with the root folded in)"""
    from oracle import anim as oa
    q = oa.q_from_xform(oa.xform_from_xy(case["ltxy"].astype(np.float64)))
    q[:, 0] = oa.q_mul(case["root_rot"].astype(np.float64), q[:, 0])
    w, x, y, z = (q[..., i] for i in range(4))
    return 2.0 * (x * y + z * w) if order == "xzy" else 2.0 * (w * y - z * x)


def bvh_oracle(case, order="zyx", start=None, bug=None, rows=None):
    """oracle.anim.bvh_channels of a bvh_case (rows: a slice of its frames, re-based on ITS first frame)"""
    from oracle import anim as oa
    r = slice(None) if rows is None else rows
    kw = {} if start is None else dict(start_position=start[0], start_rotation=start[1])
    return oa.bvh_channels(case["root_pos"][r], case["root_rot"][r], case["lpos"][r], case["ltxy"][r], order=order, bug=bug, **kw)


# quat.to_euler("xzy") returns (x angle, y angle, z angle = the asin) of the rotation Ry Rz Rx -- NOT the inverse of from_euler("xzy"), which
# composes Rx Rz Ry.  The exact inverse of each to_euler: (positions of the three outputs in from_euler's argument, its order).
BVH_EULER_INVERSE = dict(zyx=((0, 1, 2), "zyx"), xzy=((1, 2, 0), "yzx"))
BVH_ASIN_OUTPUT = dict(zyx=1, xzy=2)              # which output of to_euler is the asin (the "middle" angle)


def euler_to_quat(deg, order):
    """the rotation that quat.to_euler(order) turned into the degrees `deg` [..., 3]"""
    from oracle import anim as oa
    take, build = BVH_EULER_INVERSE[order]
    return oa.q_from_euler(np.radians(np.asarray(deg, np.float64)[..., list(take)]), build)


def euler_quat_error(got_deg, ref_deg, order):
    """Euler degrees [..., 3] -> per item || q_got - s q_ref ||_inf, s the sign that aligns the two quaternions"""
    qa, qb = euler_to_quat(got_deg, order), euler_to_quat(ref_deg, order)
    s = np.where(np.sum(qa * qb, axis=-1, keepdims=True) < 0.0, -1.0, 1.0)
    return np.abs(qa - s * qb).max(axis=-1)


def euler_angle_error(got_deg, ref_deg, order):
    """per item max |angle difference| in degrees (mod 360) where the oracle's middle angle is below 89 degrees, 0 elsewhere"""
    mid = BVH_ASIN_OUTPUT[order]
    diff = np.abs((got_deg - ref_deg + 180.0) % 360.0 - 180.0).max(axis=-1)
    return np.where(np.abs(ref_deg[..., mid]) < 89.0, diff, 0.0)


def bvh_table_seq(J):
    """a joint sequence for zeggs_pose_to_bvh_table that is no identity: reversed, then rotated by one where J is odd so that the middle
    joint moves too (J = 1: the only one there is)"""
    seq = list(range(J))[::-1]
    return seq[1:] + seq[:1] if J % 2 else seq


def bvh_table_expected(case, seq, order, start, t0=0, t1=None, bug=None):
    """rows [t0, t1) of the BVH motion block of the WHOLE clip: [root position | Euler angles of joint seq[0], seq[1], ...] from
    the oracle's bvh_channels.  bug: "seq_ignored" | "chunk_reference" (the chunk re-based on its own first frame) |
    "xzy_as_zyx" (negative controls)"""
    t1 = len(case["lpos"]) if t1 is None else t1
    if bug == "chunk_reference":
        pos, eul = bvh_oracle(case, order, start, rows=slice(t0, t1))
    else:
        pos, eul = bvh_oracle(case, "zyx" if bug == "xzy_as_zyx" else order, start)
        pos, eul = pos[t0:t1], eul[t0:t1]
    eul = eul if bug == "seq_ignored" else eul[:, list(seq)]
    return np.concatenate([pos[:, 0], eul.reshape(len(eul), -1)], axis=1)


def bvh_table_errors(got, want, order):
    """two motion-block tables [T, 3 + 3 J] -> (positions: max |got - want| / (1 + |want|), rotations: worst euler_quat_error, angles:
    worst euler_angle_error)"""
    T = len(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float("inf"), float("inf"), float("inf")
    ge, we = got[:, 3:].reshape(T, -1, 3), want[:, 3:].reshape(T, -1, 3)
    return (float(np.max(np.abs(got[:, :3] - want[:, :3]) / (1.0 + np.abs(want[:, :3])))), float(euler_quat_error(ge, we, order).max()),
            float(euler_angle_error(ge, we, order).max()))
