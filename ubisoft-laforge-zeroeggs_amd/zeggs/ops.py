"""Wrappers of libzeggs_hip.so (C ABI: include/zeggs_hip.h; the ctypes binding itself is zeggs/capi.py) + autograd glue.

PyTorch is used here only as plumbing: device memory (tensors), the current HIP
stream and autograd bookkeeping.  Every arithmetic op of the hot path is a call
into the hand-written gfx950 library.  There is deliberately NO fallback: if the
shared library is missing or a tensor is not on a GPU, these functions raise.
"""
import ctypes as C

import numpy as np
import torch

from . import capi
from .capi import (DEC_FIELDS, SPEECH_FIELDS, STATS_FIELDS, STYLE_FIELDS, STYLE_GRU_FIELDS, DecCall, DecDims, DecPtrs,  # noqa: F401
                   DecStats, FramesDims, FramesRow, GazeCond, GazeDims, GazeSet, HipLibraryMissing, LiveDims, LiveRow, LossDims, LoudDims, LoudRow, MelRow,
                   ResampleDims, ResampleRow, RefilterRow, RetimeRow, Seg, SnapSeg, SnapSpan, SpeechDims, SpeechPtrs,
                   StyleBankDims, StyleDims, StyleGruDims, StyleGruPtrs, StyleMix, StylePtrs, api)
from .capi import PlantDims, PlantRow  # noqa: E402,F401

_LIB_PATH = capi.LIB_PATH

COUNTERS = {}                                      # which optional paths ran (tests): "style_in_place"
STATUS_WORDS = 4                                   # ZEGGS_STATUS_WORDS
GAVE_UP = {1: "B=1 decode kernel", 2: "training rollout", 4: "BPTT sweep", 8: "batch decode sweep"}     # ZEGGS_GAVE_UP_* bits of status[0]


def lib():
    """The library (built by __graft_entry__.build() / csrc/build.sh) as tests, tools and the benchmark call it: return types
    set, arguments wrapped by the caller, return codes left to the caller.  The package itself calls capi.api()."""
    return capi.raw()


# _check / _p: for callers of lib() (the typed handle makes both checks itself)
def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {lib().zeggs_last_error().decode()}")


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("zeggs.ops: tensor is not on a GPU (the HIP engine has no CPU path)")
    if t.dtype not in (torch.float32, torch.int64, torch.int32, torch.uint8):
        raise RuntimeError(f"zeggs.ops: unsupported dtype {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError("zeggs.ops: tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


def _f32r(t):
    """_f32c for a tensor that a call only READS through its address (inference entry points: nothing is saved): what is float32
    and contiguous already goes as it is (0.5 us instead of 3 us per tensor on the per-chunk path of a stream)"""
    return t if t.dtype is torch.float32 and t.is_contiguous() else _f32c(t)


def _ws(nbytes, device):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


_seed_rng = np.random.default_rng(0x5EED)


def next_seed():
    rng = current().seed_rng
    return int((rng if rng is not None else _seed_rng).integers(1, 2 ** 62))


def manual_seed(s):
    """Seed of the dropout-mask / VAE-noise stream (counter-based hash inside the kernels).  Process-wide default stream; an
    EngineContext with its own `seed_rng` (TrainEngine(noise_seed=...)) draws from that instead."""
    global _seed_rng
    _seed_rng = np.random.default_rng(int(s))


# ----------------------------------------------------------------------------- per-engine call context
# What a training loop needs beyond the arguments of a call -- where gradients are written, the stream of the deferred
# weight-gradient GEMMs, the status words, hooks, a prepared workspace -- lives in an EngineContext OBJECT, not in module
# globals: `with ops.use(ctx):` makes it the context of the calling THREAD, every autograd Function captures the context of its
# forward and its backward (which autograd runs on another thread) uses that one.  Two engines stepping from two threads
# therefore never see each other's switches (tests/test_gpu_streams.py::test_two_engines_on_two_threads).
import threading  # noqa: E402


class EngineContext:
    def __init__(self):
        self.direct_grads = False          # *_bwd kernels write parameter gradients straight into the parameters' .grad
        self.wgrad_stream = None           # torch stream of the decoder's deferred weight-gradient GEMMs (ZeggsDecCall)
        self.status = None                 # device status words of the training-mode decoder calls (ZeggsDecCall.status)
        self.after_style_head = None       # hook fn(): the style encoder's first product is enqueued (engine.style_head_first)
        self.after_decoder_backward = None # hook fn(part): decoder gradients final in stream order (data-parallel exchange)
        self.decoder_grads_final = None    # hook fn(): runs on wgrad_stream behind ALL decoder gradients (early RAdam slice)
        self.prepared = None               # (key, workspace, event, mask) of decoder_prepare, until a forward picks it up
        self.prepared_hits = 0
        self.wgrad_keepalive = []          # workspaces the deferred GEMMs still read, until the caller joined wgrad_stream
        self.seed_rng = None               # own noise-seed generator (None: the process-wide stream of ops.manual_seed)
        self.gemm_route = None             # (direct, shield, depth, reserve) of THIS context's weight-gradient products (zeggs_gemm_route);
                                           # takes precedence over set_option("gemm_direct*") for them (-1 / None: the option)
        self.defer_style_wgrads = False    # the attention style encoder's backward enqueues its chain only and leaves its six weight-
        self.deferred_wgrads = []          # gradient products here as (event, fn()): the caller runs them on another stream and joins

    def release_wgrad_workspaces(self):
        """After the caller has made its stream wait for wgrad_stream: the decoder workspaces the deferred weight-gradient
        GEMMs were reading may go back to the allocator (kept alive here instead of `record_stream`-ed, see decoder_prepare)."""
        self.wgrad_keepalive.clear()

    def rng(self):
        return self.seed_rng if self.seed_rng is not None else _seed_rng


_DEFAULT_CTX = EngineContext()          # plain autograd use (tests, the reference's own loop): nothing special
_tls = threading.local()


def _route(ectx):
    """Entry of every call that launches matrix products: the GEMM routing of the context the call belongs to becomes the calling
    thread's (forward: the thread inside `ops.use`, backward: autograd's worker thread, with the context its forward captured).  One
    ctypes call when the thread's route changes, nothing otherwise."""
    r = ectx.gemm_route or (-1, -1, -1, -1)
    if getattr(_tls, "route", (-1, -1, -1, -1)) != r:
        api().zeggs_gemm_route(*[int(x) for x in r])
        _tls.route = r


def gemm_direct_warm():
    """The first-use check of every direct weight-gradient kernel variant the current context's route can select, now and on no
    caller stream (zeggs_gemm_direct_warm), so that no later product stops for it.  -> None, or why a check could not run (the
    first product that wants that variant tries again)."""
    _route(current())
    try:
        api().zeggs_gemm_direct_warm()
    except RuntimeError as e:
        return str(e)
    return None


def current():
    return getattr(_tls, "ctx", None) or _DEFAULT_CTX


class use:
    """`with ops.use(ctx):` -- ctx is the EngineContext of this thread inside the block."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.prev = getattr(_tls, "ctx", None)
        _tls.ctx = self.ctx
        return self.ctx

    def __exit__(self, *exc):
        _tls.ctx = self.prev
        _route(current())                  # the route goes with its context: a raw zeggs_gemm* caller gets the outer one's again


_SIDE_STREAMS = {}


def side_stream(device=None):
    """The library's low-priority second stream of `device` as a torch stream (zeggs_side_stream)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _SIDE_STREAMS:
        with torch.cuda.device(idx):
            h = C.c_void_p(0)
            api().zeggs_side_stream(C.byref(h))
            _SIDE_STREAMS[idx] = torch.cuda.ExternalStream(h.value, device=torch.device("cuda", idx))
    return _SIDE_STREAMS[idx]


def new_status(device):
    """Zeroed status words (ZeggsDecCall.status): [0] sticky ZEGGS_GAVE_UP_* bits, [1] optimizer steps skipped because of them."""
    t = torch.empty(STATUS_WORDS, dtype=torch.int32, device=device)
    fill_(t.view(torch.float32))
    return t


_PLAIN_TLS = threading.local()


def _plain_status(dev):
    """Status words of a decoder call made OUTSIDE an engine context: one per device and host thread (concurrent rollouts do not
    share it), held in thread-local storage so that it is freed with the thread (a dict keyed by thread id grew for
    ever in programs that spawn threads).  Cost to know about: the caller of such a call reads the word back right after the
    rollout -- ONE 4-byte device-to-host read (a host synchronisation) per rollout, forward and backward, and only once a
    persistent kernel has been validated on this process; an engine (ops.use(EngineContext) with a status of its own, as
    zeggs.engine.TrainEngine) never pays it -- it reads its words with a lag of three iterations."""
    per_dev = getattr(_PLAIN_TLS, "words", None)
    if per_dev is None:
        per_dev = _PLAIN_TLS.words = {}
    st = per_dev.get(dev.index)
    if st is None:
        st = per_dev[dev.index] = new_status(dev)
    return st


def _grad_targets(orig_params, params, ectx):
    """-> (tensors the backward kernel writes, values returned to autograd).  Direct mode (EngineContext.direct_grads, only
    engine.TrainEngine turns it on): the *_bwd entry points write parameter gradients STRAIGHT into the parameters' existing
    `.grad` tensors (views of the engine's flat gradient buffer) and the autograd Functions return None for them, so no
    AccumulateGrad add runs.  Semantics are OVERWRITE (every parameter is used by exactly one op per iteration); the `.grad`
    tensors MUST be zero when the backward starts (the engine zeroes its flat buffer once per step): the kernels are told so
    (`grads_zeroed`) and accumulate onto them instead of zero-filling each one first."""
    outs, rets = [], []
    for o, t in zip(orig_params, params):
        g = getattr(o, "grad", None) if ectx.direct_grads else None
        if g is not None and g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.shape == t.shape:
            outs.append(g)
            rets.append(None)
        else:
            e = torch.empty_like(t)
            outs.append(e)
            rets.append(e)
    return outs, rets


def fill_(t, value=0.0):
    api().zeggs_fill(t, t.numel(), value, _stream())
    return t


def scale_copy(src, dev_scale=None, alpha=1.0, out=None):
    """out = alpha * dev_scale[0] * src (dev_scale: 1-element device tensor or None)"""
    src = src if src.is_contiguous() else src.contiguous()
    out = torch.empty_like(src) if out is None else out
    api().zeggs_scale_copy(out, src, src.numel(), dev_scale, alpha, _stream())
    return out


def randn(shape, device, seed=None):
    """Standard normal samples from the library's counter-hash stream (seeded by ops.manual_seed)."""
    out = torch.empty(*shape, device=device, dtype=torch.float32)
    api().zeggs_randn(out, out.numel(), next_seed() if seed is None else int(seed), _stream())
    return out


def randn_into(view, seed=None):
    """randn() into a contiguous float32 slice of a persistent buffer: the same zeggs_randn launch, so view == randn(view.shape,
    seed=seed) bit for bit, and nothing is allocated"""
    if view.dtype is not torch.float32 or not view.is_contiguous():
        raise ValueError("randn_into: a contiguous float32 view")
    api().zeggs_randn(view, view.numel(), next_seed() if seed is None else int(seed), _stream())
    return view


class _BroadcastTimeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, T):
        z = _f32c(z)
        B, S = z.shape
        out = torch.empty(B, T, S, device=z.device, dtype=torch.float32)
        api().zeggs_broadcast_time(out, z, B, T, S, _stream())
        ctx.dims = (B, T, S)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, T, S = ctx.dims
        dz = torch.empty(B, S, device=dout.device, dtype=torch.float32)
        api().zeggs_sum_time(dz, _f32c(dout), B, T, S, _stream())
        return dz, None


def broadcast_time(z, T):
    """z [B,S] -> [B,T,S] contiguous (style_encoding.unsqueeze(1).repeat_interleave(T, 1), ZEGGS/train.py:256)"""
    return _BroadcastTimeFn.apply(z, int(T))


def _ptrs(cls, fields, tensors):
    s = cls()
    for f, t in zip(fields, tensors):
        setattr(s, f, t.data_ptr() if t is not None else None)
    return s


# ----------------------------------------------------------------------------- raw GEMM (tests)
def gemm(A, B, Cmat, M, N, K, sa, sb, sc, bias=None, nbatch=1, bs=(0, 0, 0), alpha=1.0, beta=0.0, act=0):
    api().zeggs_gemm(A, B, Cmat, bias, M, N, K, sa[0], sa[1], sb[0], sb[1], sc[0], sc[1], nbatch, bs[0], bs[1], bs[2], alpha, beta,
                     act, _stream())
    return Cmat


# ----------------------------------------------------------------------------- speech encoder
class _SpeechFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1, w2, b2, p, seed):
        x = _f32c(x)
        ctx.ectx = current()
        _route(ctx.ectx)
        ctx.orig = (w0, b0, w1, b1, w2, b2)
        params = [_f32c(t) for t in (w0, b0, w1, b1, w2, b2)]
        B, T, F = x.shape
        d = SpeechDims(B, T, F, w0.shape[0], w2.shape[0], w1.shape[2], float(p), int(seed))
        L = api()
        ws = _ws(L.zeggs_speech_encoder_workspace_bytes(d), x.device)
        out = torch.empty(B, T, d.O, device=x.device, dtype=torch.float32)
        P = _ptrs(SpeechPtrs, SPEECH_FIELDS, params)
        L.zeggs_speech_encoder_fwd(d, P, x, out, ws, ws.numel(), _stream())
        ctx.d, ctx.ws = d, ws
        ctx.save_for_backward(x, out, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out, *params = ctx.saved_tensors
        L = api()
        _route(ctx.ectx)
        grads, rets = _grad_targets(ctx.orig, params, ctx.ectx)
        P = _ptrs(SpeechPtrs, SPEECH_FIELDS, params)
        G = _ptrs(SpeechPtrs, SPEECH_FIELDS, grads)
        zeroed = int(ctx.ectx.direct_grads and all(r is None for r in rets))     # the engine zeroes its flat gradient buffer per step
        L.zeggs_speech_encoder_bwd_ex(ctx.d, P, x, out, _f32c(dout), G, ctx.ws, ctx.ws.numel(), _stream(), zeroed)
        return (None, *rets, None, None)


def speech_encoder(x, w0, b0, w1, b1, w2, b2, p=0.0):
    return _SpeechFn.apply(x, w0, b0, w1, b1, w2, b2, p, next_seed() if p > 0 else 0)


# ----------------------------------------------------------------------------- style encoder
_POS_CACHE = {}


def positional_table(length, dim, device):
    """Sinusoidal table of the reference PositionalEncoding (modules.py:450-459), built on the host exactly as
    the reference does (float32 torch ops) and cached on the device."""
    key = (dim, str(device))
    tab = _POS_CACHE.get(key)
    if tab is None or tab.shape[0] < length:
        n = max(length, 1024)
        pos = torch.arange(0, n, dtype=torch.float).unsqueeze(1)
        div = torch.exp(torch.arange(0, dim, 2).float() * (-np.log(10000.0) / dim))
        t = torch.zeros(n, dim)
        t[:, 0::2] = torch.sin(pos * div)
        t[:, 1::2] = torch.cos(pos * div)
        tab = t.to(device)
        _POS_CACHE[key] = tab
    return tab


def style_param_list(enc):
    """Parameters of a StyleEncoderAttn module in the C-ABI order (STYLE_FIELDS)."""
    c, b = enc.convs, enc.blocks[0]
    mha = b.attention.multi_head_attention
    return [c[0].conv.weight, c[0].conv.bias, c[2].weight, c[2].bias, c[4].conv.weight, c[4].conv.bias,
            c[6].weight, c[6].bias, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias,
            b.attention.layer_norm.weight, b.attention.layer_norm.bias,
            b.feed_forward.convs[0].conv.weight, b.feed_forward.convs[0].conv.bias,
            b.feed_forward.convs[2].conv.weight, b.feed_forward.convs[2].conv.bias,
            b.feed_forward.layer_norm.weight, b.feed_forward.layer_norm.bias]


class _StyleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos, dropout, seed, nheads, *params):
        ctx.ectx = current()
        _route(ctx.ectx)
        ctx.orig = params
        params = [_f32c(t) for t in params]
        B, Lx, Cx = x.shape
        H, E = params[0].shape[0], params[4].shape[0]
        d = StyleDims(B, Lx, Cx, H, E, nheads, int(dropout), int(seed))
        L = api()
        need = int(L.zeggs_style_encoder_workspace_bytes(d))
        # an example that style_input_buffer() + gather_example() put where the workspace keeps the first convolution's padded input:
        # the encoder runs IN that workspace and skips its own padding copy (zeggs_style_encoder_fwd_part, part | 4); anything that
        # does not match exactly (another shape, a copy of the tensor, a workspace of another size) takes the ordinary path
        ws, inplace = getattr(x, "_zeggs_style_ws", None), 0
        if ws is not None and x.dtype == torch.float32 and ws.numel() == need and x.stride() == ((Lx + 2) * Cx, Cx, 1) and \
                x.data_ptr() == ws.data_ptr() + int(L.zeggs_style_encoder_input_offset(d)) + 4 * Cx:
            inplace, xptr = 4, C.c_void_p(x.data_ptr())      # (a strided view of the padded buffer: by address)
            COUNTERS["style_in_place"] = COUNTERS.get("style_in_place", 0) + 1
        else:
            x = _f32c(x)
            ws, xptr = _ws(need, x.device), x
        out = torch.empty(B, E, device=x.device, dtype=torch.float32)
        P = _ptrs(StylePtrs, STYLE_FIELDS, params)
        hook = getattr(ctx.ectx, "after_style_head", None)
        if hook is not None:       # (an engine that releases its other queues once the chip-filling first product is enqueued)
            L.zeggs_style_encoder_fwd_part(d, P, xptr, pos, out, ws, ws.numel(), _stream(), 1 | inplace)
            hook()
            L.zeggs_style_encoder_fwd_part(d, P, xptr, pos, out, ws, ws.numel(), _stream(), 2 | inplace)
        else:
            L.zeggs_style_encoder_fwd_part(d, P, xptr, pos, out, ws, ws.numel(), _stream(), 3 | inplace)
        ctx.d, ctx.ws = d, ws
        ctx.save_for_backward(*params)
        return out

    @staticmethod
    def backward(ctx, dout):
        params = list(ctx.saved_tensors)
        L = api()
        _route(ctx.ectx)
        grads, rets = _grad_targets(ctx.orig, params, ctx.ectx)
        P = _ptrs(StylePtrs, STYLE_FIELDS, params)
        G = _ptrs(StylePtrs, STYLE_FIELDS, grads)
        zeroed = int(ctx.ectx.direct_grads and all(r is None for r in rets))
        dout = _f32c(dout)
        ectx = ctx.ectx
        if ectx.defer_style_wgrads and zeroed:
            # the chain now, on this stream; the six weight-gradient products later, where the caller puts them (they read the operands
            # the chain parked in the workspace: zeggs_style_encoder_bwd_part)
            L.zeggs_style_encoder_bwd_part(ctx.d, P, dout, G, ctx.ws, ctx.ws.numel(), _stream(), zeroed, 1)
            ev = torch.cuda.Event()
            ev.record()
            d, ws, keep = ctx.d, ctx.ws, (params, grads, dout)

            def products():
                _route(ectx)
                L.zeggs_style_encoder_bwd_part(d, P, keep[2], G, ws, ws.numel(), _stream(), zeroed, 2)
            ectx.deferred_wgrads.append((ev, products))
            return (None, None, None, None, None, *rets)
        L.zeggs_style_encoder_bwd_ex(ctx.d, P, dout, G, ctx.ws, ctx.ws.numel(), _stream(), zeroed)
        return (None, None, None, None, None, *rets)


class _StyleGruFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, *params):
        x = _f32c(x)
        ctx.ectx = current()
        _route(ctx.ectx)
        ctx.orig = params
        params = [_f32c(t) for t in params]
        B, Lx, Cx = x.shape
        d = StyleGruDims(B, Lx, Cx, params[0].shape[0], params[12].shape[0])
        L = api()
        ws = _ws(L.zeggs_style_encoder_gru_workspace_bytes(d), x.device)
        out = torch.empty(B, d.O, device=x.device, dtype=torch.float32)
        P = _ptrs(StyleGruPtrs, STYLE_GRU_FIELDS, params)
        L.zeggs_style_encoder_gru_fwd(d, P, x, out, ws, ws.numel(), _stream())
        ctx.d, ctx.ws = d, ws
        ctx.save_for_backward(*params)
        return out

    @staticmethod
    def backward(ctx, dout):
        params = list(ctx.saved_tensors)
        _route(ctx.ectx)
        grads, rets = _grad_targets(ctx.orig, params, ctx.ectx)
        P = _ptrs(StyleGruPtrs, STYLE_GRU_FIELDS, params)
        G = _ptrs(StyleGruPtrs, STYLE_GRU_FIELDS, grads)
        api().zeggs_style_encoder_gru_bwd(ctx.d, P, _f32c(dout), G, ctx.ws, ctx.ws.numel(), _stream())
        return (None, *rets)


def style_encoder_gru(x, enc):
    """StyleEncoderGRU.forward (reference modules.py:339-343) on the HIP engine"""
    g, pl = enc.rnn_layer, enc.projection_layer.linear_layer
    return _StyleGruFn.apply(x, enc.convs[0].conv.weight, enc.convs[0].conv.bias, enc.convs[2].conv.weight,
                             enc.convs[2].conv.bias, g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0,
                             g.weight_ih_l0_reverse, g.weight_hh_l0_reverse, g.bias_ih_l0_reverse, g.bias_hh_l0_reverse,
                             pl.weight, pl.bias)


def style_input_buffer(enc, B, L, Cx, training, device, ws=None):
    """A workspace of the attention style encoder for a [B, L, Cx] example whose padded-input region the CALLER fills
    (gather_example): -> (ws, xp [B, L + 2, Cx] view of it).  `xp[:, 1:-1]` carries the workspace with it (attribute
    _zeggs_style_ws); style_encoder_attn() on that tensor runs in this workspace without its padding copy.  `ws`: a buffer of an
    earlier call to use again when it still fits."""
    params = style_param_list(enc)
    d = StyleDims(int(B), int(L), int(Cx), params[0].shape[0], params[4].shape[0], 4, 1 if training else 0, 0)
    Lb = api()
    need = Lb.zeggs_style_encoder_workspace_bytes(d)
    if ws is None or ws.numel() != need or ws.device != torch.device(device):
        ws = _ws(need, device)
    off = Lb.zeggs_style_encoder_input_offset(d)
    xp = ws[off:off + 4 * B * (L + 2) * Cx].view(torch.float32).view(B, L + 2, Cx)
    return ws, xp


def example_view(ws, xp):
    """The [B, L, C] example inside the padded buffer `xp` of style_input_buffer(), tagged with its workspace."""
    ex = xp[:, 1:-1]
    ex._zeggs_style_ws = ws
    return ex


def gather_example(frames, rows, mean, std, out, pad=1):
    """zeggs_gather_example: frames [N, W], rows int64 [B, L], mean / std [Wo] -> out [B, L + 2 pad, Wo] (contiguous):
    normalised rows with the columns W.. zero BEFORE the normalisation (the example's empty gaze slot, reference dataset.py:194),
    edge rows zero."""
    B, Lr = rows.shape
    Wo = out.shape[2]
    assert out.shape == (B, Lr + 2 * pad, Wo) and out.is_contiguous() and mean.numel() == Wo and std.numel() == Wo
    api().zeggs_gather_example(frames, frames.shape[1], rows.contiguous(), int(B), int(Lr), _f32c(mean), _f32c(std), out, int(Wo),
                               int(pad), _stream())
    return out


def style_encoder_attn(x, enc, training):
    pos = positional_table(x.shape[1], enc.convs[6].normalized_shape[0], x.device)
    return _StyleFn.apply(x, pos, 1 if training else 0, next_seed() if training else 0, 4, *style_param_list(enc))


class _VaeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, eps, temperature, S):
        enc, eps = _f32c(enc), _f32c(eps)
        B = enc.shape[0]
        z, mu, lv = (torch.empty(B, S, device=enc.device, dtype=torch.float32) for _ in range(3))
        api().zeggs_vae_reparam_fwd(enc, eps, z, mu, lv, B, S, temperature, _stream())
        ctx.save_for_backward(enc, eps)
        ctx.t, ctx.S = temperature, S
        ctx.set_materialize_grads(False)
        return z, mu, lv

    @staticmethod
    def backward(ctx, dz, dmu, dlv):
        enc, eps = ctx.saved_tensors
        denc = torch.empty_like(enc)
        c = lambda g: _f32c(g) if g is not None else None  # noqa: E731
        api().zeggs_vae_reparam_bwd(enc, eps, c(dz), c(dmu), c(dlv), denc, enc.shape[0], ctx.S, ctx.t, _stream())
        return denc, None, None, None


def vae_reparam(enc, eps, temperature, S):
    """-> z, mu, logvar (contiguous [B,S] each; mu / logvar are the two halves of enc)"""
    return _VaeFn.apply(enc, eps, float(temperature), S)


# ----------------------------------------------------------------------------- decoder
def decoder_param_list(dec):
    r, c = dec.recurrent_decoder, dec.cell_state_encoder
    g = r.layer1
    ps = [r.layer0.weight, r.layer0.bias, g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0,
          g.weight_ih_l1, g.weight_hh_l1, g.bias_ih_l1, g.bias_hh_l1, r.layer2.weight, r.layer2.bias,
          c.layer0.weight, c.layer0.bias, c.layer1.weight, c.layer1.bias, c.layer2.weight, c.layer2.bias]
    if hasattr(r, "gammas_predictor"):      # RecurrentDecoderFiLM
        ps += [r.layer3.weight, r.layer3.bias, r.gammas_predictor.linear_layer.weight,
               r.gammas_predictor.linear_layer.bias, r.betas_predictor.linear_layer.weight,
               r.betas_predictor.linear_layer.bias]
    return ps


def _drop_prepared(ectx):
    """Forget a preparation nobody picked up (an eval / no_grad call, another batch size, an exception in between): the
    prepare kernels may still be WRITING the workspace on the side stream, and the block goes back to the current stream's
    pool -- so the current stream waits for them first."""
    prep, ectx.prepared = ectx.prepared, None
    if prep is not None:
        torch.cuda.current_stream().wait_event(prep[2])


def _versions(params):
    """autograd version counters of the weights a preparation was made from: an in-place torch operation on them in between (a
    loaded checkpoint, a replayed snapshot, a hand edit) makes the forward ignore the packs and make its own.  (The engine's
    own optimizer kernels write through raw pointers and do not count -- they run BEFORE the preparation.)"""
    return tuple(int(t._version) for t in params)


def _prepared_key(d, params, stats):
    """What a preparation is valid for: the dimensions, the weights AND the four statistics vectors -- the packs fold in_mean,
    in_std, out_mean, out_std into the weights (dec_fast_merge_prep, dec_tp_pack), so a call with other statistics must not pick
    them up."""
    return (d.B, d.T, d.PI, d.PO, d.SP, d.ST, d.H, d.film, tuple(t.data_ptr() for t in params), _versions(params),
            tuple(t.data_ptr() for t in stats), _versions(stats))


def decoder_prepare(dec, B, T, SP, ST, in_mean, in_std, out_mean, out_std, dt, stream, after=None):
    """Weight-only preparation of the NEXT training-mode decoder_core call of THIS context (ops.use) with these dimensions
    (zeggs_decoder_prepare) on `stream`, beside whatever the current stream does meanwhile (the encoders' forward); that
    call picks the prepared workspace up and waits for it.  The weights must not change in between."""
    ectx = current()
    _route(ectx)
    _drop_prepared(ectx)
    params = [_f32c(t) for t in decoder_param_list(dec)]
    stats = [_f32c(t) for t in (in_mean, in_std, out_mean, out_std)]
    PO, H = int(stats[2].numel()), dec.recurrent_decoder.layer1.hidden_size
    d = DecDims(int(B), int(T), PO + 3, PO, int(SP), int(ST), H, float(dt), 1 if len(params) == len(DEC_FIELDS) else 0)
    L = api()
    ws = _ws(L.zeggs_decoder_workspace_bytes(d, 1), params[0].device)
    P = _ptrs(DecPtrs, DEC_FIELDS, params)
    S = _ptrs(DecStats, STATS_FIELDS, stats)
    stream.wait_stream(torch.cuda.current_stream())       # the optimizer step that produced these weights
    # (no record_stream: the workspace belongs to the current stream's pool and its next user there -- the forward that picks
    #  it up, or whoever gets the block after it -- comes after a wait for `stream`; a recorded stream would park the block
    #  in the allocator's pending list, and every device synchronisation would then cost a few iterations of re-allocation)
    with torch.cuda.stream(stream):
        mask = L.zeggs_decoder_prepare(d, P, S, ws, ws.numel(), stream.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(stream)
        if after is not None:       # (more work of the caller for `stream`, behind the packs and outside what the forward waits for)
            after()
    if mask > 0:
        ectx.prepared = (_prepared_key(d, params, stats), ws, ev, int(mask))
    return int(mask)


def _warn_gave_up(bits, what, disabled=True):
    import warnings
    warnings.warn("zeggs: a persistent kernel gave up (" + ", ".join(n for b, n in GAVE_UP.items() if bits & b) +
                  "; another tenant on the GPU?); " + ("it is disabled for this process and " if disabled else "") + what +
                  " is redone on the stage kernels")


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pose0, rpos0, rrot0, gaze, speech, style, in_mean, in_std, out_mean, out_std, dt, H, grad_mode,
                *params):
        pose0, rpos0, rrot0, gaze, speech, style = (_f32c(t) for t in (pose0, rpos0, rrot0, gaze, speech, style))
        stats = [_f32c(t) for t in (in_mean, in_std, out_mean, out_std)]
        ectx = ctx.ectx = current()
        _route(ctx.ectx)
        ctx.orig = params
        params = [_f32c(t) for t in params]
        B, T, SP = speech.shape
        ST, PO = style.shape[2], pose0.shape[1]
        # needs_input_grad ignores torch.no_grad(): the caller's grad mode selects the BPTT workspace / ring path
        training = bool(grad_mode) and any(ctx.needs_input_grad)
        d = DecDims(B, T, PO + 3, PO, SP, ST, H, float(dt), 1 if len(params) == len(DEC_FIELDS) else 0)
        L = api()
        dev = pose0.device
        prep = ectx.prepared
        mask = 0
        if prep is not None and training and prep[0] == _prepared_key(d, params, stats):
            ectx.prepared = None
            _, ws, ev, mask = prep                          # packs of this step's weights, made on a second stream
            ectx.prepared_hits += 1
            torch.cuda.current_stream().wait_event(ev)
        else:
            _drop_prepared(ectx)                            # (waits for the side stream before the block is released)
            ws = _ws(L.zeggs_decoder_workspace_bytes(d, int(training)), pose0.device)
        pose = torch.empty(B, T, PO, device=dev, dtype=torch.float32)
        rpos = torch.empty(B, T, 3, device=dev, dtype=torch.float32)
        rrot = torch.empty(B, T, 4, device=dev, dtype=torch.float32)
        P = _ptrs(DecPtrs, DEC_FIELDS, params)
        S = _ptrs(DecStats, STATS_FIELDS, stats)
        capturing = torch.cuda.is_current_stream_capturing()
        # Give-up detection (ZeggsDecCall.status).  An engine passes ITS status words and looks at them itself (device-guarded
        # optimizer step, lagged read-back: engine.TrainEngine).  Every other caller gets a per-thread word that is inspected
        # right here, where a validated persistent kernel may have run: the outputs are consumed next (BVH export, sample
        # rendering, the reference's own loss / optimizer) and nothing else would notice.  No read-back -- and no host
        # synchronisation -- when no persistent kernel can have been involved, or inside a stream capture (there the NaN
        # poisoning of the outputs is what is left).
        own = None
        if training:
            status = ectx.status
            if status is None and not capturing and (_persistent_live(1) or _persistent_live(2)):
                status = own = _plain_status(dev)
        else:
            status = None
            if not capturing and B == 1 and _persistent_live(0):
                status = own = _plain_status(dev)
        call = DecCall(int(mask) & 1, 0, None, status.data_ptr() if status is not None else None, 0)

        def run():
            L.zeggs_decoder_fwd_ex(d, P, S, pose0, rpos0, rrot0, gaze, speech, style, pose, rpos, rrot, int(training), ws, ws.numel(),
                                   _stream(), call)
        run()
        if own is not None:
            bits = int(own[0].item())                      # one 4-byte read-back per rollout
            if bits:
                _warn_gave_up(bits, "the rollout")
                for name in ("persistent", "train_persistent", "bwd_persistent"):
                    set_option(name, 0)
                fill_(own.view(torch.float32))
                call.prepared = 0
                run()
        global _LAST_DECODER_WS
        if _CHAIN_DIAGNOSTICS:          # (diagnostic of the off-by-default "chain" option only: pins the workspace)
            _LAST_DECODER_WS = (d, int(training), ws)
        if training:
            ctx.d, ctx.ws = d, ws
            ctx.status, ctx.own_status = status, own is not None
            ctx.bwd_prepared = bool(mask & 2) and call.prepared != 0
            ctx.save_for_backward(gaze, pose, rpos, rrot, *stats, *params)
            ctx.set_materialize_grads(False)      # missing output gradients are zero-filled by our own kernel in backward
        return pose, rpos, rrot

    @staticmethod
    def backward(ctx, dpose, drpos, drrot):
        gaze, pose, rpos, rrot, *rest = ctx.saved_tensors
        stats, params = rest[:4], rest[4:]
        d = ctx.d
        ectx = ctx.ectx
        _route(ectx)
        L = api()
        dev = pose.device
        z = lambda g, ref: fill_(torch.empty_like(ref)) if g is None else _f32c(g)  # noqa: E731
        dpose, drpos, drrot = z(dpose, pose), z(drpos, rpos), z(drrot, rrot)
        grads, rets = _grad_targets(ctx.orig, params, ectx)
        dspeech = torch.empty(d.B, d.T, d.SP, device=dev, dtype=torch.float32)
        dstyle = torch.empty(d.B, d.T, d.ST, device=dev, dtype=torch.float32)
        P = _ptrs(DecPtrs, DEC_FIELDS, params)
        G = _ptrs(DecPtrs, DEC_FIELDS, grads)
        S = _ptrs(DecStats, STATS_FIELDS, stats)
        direct = ectx.direct_grads and all(r is None for r in rets)
        side = ectx.wgrad_stream if direct and not torch.cuda.is_current_stream_capturing() else None
        # with a gradient exchange waiting (engine hook) the deferred GEMMs come in two halves of the parameter order, so that
        # the all-reduce of one runs underneath the GEMMs of the other
        after = ectx.after_decoder_backward
        chunked = side is not None and after is not None
        call = DecCall(2 if ctx.bwd_prepared else 0, 0 if side is None else (2 if chunked else 1),
                       side.cuda_stream if side is not None else None,
                       ctx.status.data_ptr() if ctx.status is not None else None, int(direct))

        def run():
            L.zeggs_decoder_bwd_ex(d, P, S, gaze, pose, rpos, rrot, dpose, drpos, drrot, G, dspeech, dstyle, ctx.ws, ctx.ws.numel(),
                                   _stream(), call)
        run()
        if ctx.own_status and not torch.cuda.is_current_stream_capturing():
            # plain autograd use (no engine looking at the word later): the gradients go to the caller's optimizer next
            bits = int(ctx.status[0].item())
            if bits:
                _warn_gave_up(bits, "the BPTT sweep")
                for name in ("train_persistent", "bwd_persistent"):
                    set_option(name, 0)
                fill_(ctx.status.view(torch.float32))
                call.prepared = 0
                run()                   # the forward's saved activations are intact: only the sweep is repeated
        if side is not None:
            # the library has put the recurrent layers' weight-gradient GEMMs on its second stream (they read only what the
            # sweep left in the workspace), beside the CellStateEncoder / encoder backward on this one
            ectx.wgrad_keepalive.append(ctx.ws)      # read by `side` until the caller joins it (release_wgrad_workspaces)
            if chunked:
                side.wait_stream(torch.cuda.current_stream())       # the CellStateEncoder gradients come from this stream
                with torch.cuda.stream(side):
                    after(0)         # layer2, GRU layer 1, CellStateEncoder: final behind the GEMMs already on `side`
                    L.zeggs_decoder_wgrads(d, G, ctx.ws, ctx.ws.numel(), 4 | 8, side.cuda_stream)
                    after(1)         # layer0, GRU layer 0
            elif ectx.decoder_grads_final is not None:
                side.wait_stream(torch.cuda.current_stream())       # the CellStateEncoder gradients come from this stream
                with torch.cuda.stream(side):
                    ectx.decoder_grads_final()
        elif after is not None and direct:
            after(None)
        return (None, None, None, None, dspeech, dstyle, None, None, None, None, None, None, None, *rets)


_LAST_DECODER_WS = None
_CHAIN_DIAGNOSTICS = False      # set by set_option("chain", 1): keep the last decoder workspace for last_decoder_chain_errors()


def last_decoder_chain_errors():
    """Error word of the chained (run-ahead) stage launches of the most recent decoder rollout (option "chain"):
    0 = every device-side hand-off wait was satisfied.  Synchronises the device."""
    if _LAST_DECODER_WS is None:
        return 0
    d, training, ws = _LAST_DECODER_WS
    out = C.c_int(0)
    api().zeggs_decoder_chain_errors(d, training, ws, ws.numel(), C.byref(out))
    return int(out.value)


def decoder_core(dec, pose0, rpos0, rrot0, gaze, speech, style, in_mean, in_std, out_mean, out_std, dt):
    """-> pose [B,T,PO] (de-normalised output vectors), rpos [B,T,3], rrot [B,T,4]"""
    H = dec.recurrent_decoder.layer1.hidden_size
    return _DecoderFn.apply(pose0, rpos0, rrot0, gaze, speech, style, in_mean, in_std, out_mean, out_std, dt, H,
                            torch.is_grad_enabled(), *decoder_param_list(dec))


def decoder_rollout(dec, Z_root_pos, Z_root_rot, Z_root_vel, Z_root_vrt, Z_lpos, Z_ltxy, Z_lvel, Z_lvrt, gaze,
                    speech, style, in_mean, in_std, out_mean, out_std, dt):
    """Reference-shaped Decoder.forward: 8 tensors [B,T,...] (views of the engine's pose rows)."""
    B, J = Z_lpos.shape[0], Z_lpos.shape[1]
    pose0 = torch.cat([Z_root_vel.reshape(B, -1), Z_root_vrt.reshape(B, -1), Z_lpos.reshape(B, -1),
                       Z_ltxy.reshape(B, -1), Z_lvel.reshape(B, -1), Z_lvrt.reshape(B, -1)], dim=1)
    pose, rpos, rrot = decoder_core(dec, pose0, Z_root_pos, Z_root_rot, gaze, speech, style, in_mean, in_std,
                                    out_mean, out_std, dt)
    T = pose.shape[1]
    return (rpos, rrot, pose[..., 0:3], pose[..., 3:6], pose[..., 6:6 + 3 * J].reshape(B, T, J, 3),
            pose[..., 6 + 3 * J:6 + 9 * J].reshape(B, T, J, 2, 3),
            pose[..., 6 + 9 * J:6 + 12 * J].reshape(B, T, J, 3),
            pose[..., 6 + 12 * J:6 + 15 * J].reshape(B, T, J, 3))


def decoder_chunk(dec, pose0, rpos0, rrot0, gaze, speech, style, in_mean, in_std, out_mean, out_std, dt, h_in=None,
                  status=None):
    """Inference rollout resumed from a given state (zeggs_decoder_fwd_state_ex): frame 0 of the chunk is the last frame already
    produced (pose0 / rpos0 / rrot0; index 0 of gaze / speech / style belongs to it), h_in [2,B,H] the GRU state after it (None:
    first chunk, CellStateEncoder).  -> pose [B,N,PO], rpos, rrot, h_out [2,B,H].  Nothing is read back: `status` (device
    words, ops.new_status) collects a give-up bit of the persistent kernel for the CALLER to look at when it chooses to."""
    pose0, rpos0, rrot0, gaze, speech, style = (_f32r(t) for t in (pose0, rpos0, rrot0, gaze, speech, style))
    stats = [_f32r(t) for t in (in_mean, in_std, out_mean, out_std)]
    params = [_f32r(t) for t in decoder_param_list(dec)]
    B, N, SP = speech.shape
    PO, H = pose0.shape[1], dec.recurrent_decoder.layer1.hidden_size
    d = DecDims(B, N, PO + 3, PO, SP, style.shape[2], H, float(dt), 1 if len(params) == len(DEC_FIELDS) else 0)
    L = api()
    dev = pose0.device
    ws = _ws(L.zeggs_decoder_workspace_bytes(d, 0), dev)
    pose = torch.empty(B, N, PO, device=dev, dtype=torch.float32)
    rpos = torch.empty(B, N, 3, device=dev, dtype=torch.float32)
    rrot = torch.empty(B, N, 4, device=dev, dtype=torch.float32)
    h_out = torch.empty(2, B, H, device=dev, dtype=torch.float32)
    P = _ptrs(DecPtrs, DEC_FIELDS, params)
    S = _ptrs(DecStats, STATS_FIELDS, stats)
    call = DecCall(0, 0, None, status.data_ptr() if status is not None else None, 0)
    L.zeggs_decoder_fwd_state_ex(d, P, S, pose0, rpos0, rrot0, gaze, speech, style, pose, rpos, rrot,
                                 _f32r(h_in) if h_in is not None else None, h_out, ws, ws.numel(), _stream(), call)
    return pose, rpos, rrot, h_out


# ----------------------------------------------------------------------------- batch decode (many clips per rollout)
BATCH_PATHS = {0: None, 1: "persistent", 2: "stage"}


def batch_last_path():
    """Which path this thread's last decoder_batch_chunk took: "persistent" (the weight-stationary sweep), "stage" (the stage
    launches: unsupported dimensions, a sweep that is switched off or gave up) or None."""
    return BATCH_PATHS[api().zeggs_decoder_batch_last_path()]


class BatchDecode:
    """Workspace and weight packs of one job list on the batch decode (zeggs_decoder_batch_prepare: the weight-only work runs
    here, once, not per chunk).  `B` rows, chunks of at most `chunk` frames (frame 0 of a chunk included).  `sweep` tells
    whether these dimensions run on the weight-stationary sweep at all (else every chunk takes the stage launches)."""

    def __init__(self, dec, B, chunk, SP, ST, in_mean, in_std, out_mean, out_std, dt):
        self.stats = [_f32c(t) for t in (in_mean, in_std, out_mean, out_std)]
        self.params = [_f32c(t) for t in decoder_param_list(dec)]
        self.B, self.chunk, self.SP, self.ST = int(B), int(chunk), int(SP), int(ST)
        self.PO, self.H, self.dt = int(self.stats[2].numel()), dec.recurrent_decoder.layer1.hidden_size, float(dt)
        self.film = 1 if len(self.params) == len(DEC_FIELDS) else 0
        L = api()
        _route(current())
        d = self.dims(self.chunk)
        self.ws = _ws(L.zeggs_decoder_batch_workspace_bytes(d), self.params[0].device)
        self.P = _ptrs(DecPtrs, DEC_FIELDS, self.params)
        self.S = _ptrs(DecStats, STATS_FIELDS, self.stats)
        self.mask = L.zeggs_decoder_batch_prepare(d, self.P, self.S, self.ws, self.ws.numel(), _stream())
        self.sweep = self.mask != 0

    def dims(self, T, B=None):
        return DecDims(self.B if B is None else int(B), int(T), self.PO + 3, self.PO, self.SP, self.ST, self.H, self.dt, self.film)


def decoder_state_init(bd, pose0, rpos0, rrot0, gaze0, style0):
    """The CellStateEncoder alone (zeggs_decoder_state_init): first pose [n,PO], root state [n,3] / [n,4], gaze target [n,3] and
    style [n,ST] of frame 0 of n clips -> the GRU state [2,n,H] they start from (rows of a later decoder_batch_chunk's h_in)."""
    pose0, rpos0, rrot0, gaze0, style0 = (_f32c(t) for t in (pose0, rpos0, rrot0, gaze0, style0))
    n = pose0.shape[0]
    assert 1 <= n <= bd.B
    h = torch.empty(2, n, bd.H, device=pose0.device, dtype=torch.float32)
    d = bd.dims(1, n)
    api().zeggs_decoder_state_init(d, bd.P, bd.S, pose0, rpos0, rrot0, gaze0, style0, h, bd.ws, bd.ws.numel(), _stream())
    return h


def decoder_batch_chunk(bd, pose0, rpos0, rrot0, gaze, speech, style, h_in, status=None, info=None, stage=False):
    """One chunk of the batch decode (zeggs_decoder_fwd_batch), arguments as decoder_chunk with B = bd.B rows and N <= bd.chunk
    frames: frame 0 of the chunk is the last frame already produced of every row, h_in [2,B,H] the GRU state after it (rows that
    begin a clip: decoder_state_init).  -> pose [B,N,PO], rpos, rrot, h_out [2,B,H].  Rows are independent; what an idle row
    holds does not matter.  With `status` (ops.new_status) the word is read back after the chunk once the sweep has been
    validated on this process -- one 4-byte read per chunk: the next chunk starts from h_out --, and a chunk whose sweep gave up is
    redone on the stage launches right here (with non-finite gaze / speech / style values replaced by 0: only the sweep isolates a
    row's last valid frame from what follows it).  `info` (a dict) receives "path" and "gave_up"."""
    pose0, rpos0, rrot0, gaze, speech, style, h_in = (_f32c(t) for t in (pose0, rpos0, rrot0, gaze, speech, style, h_in))
    B, N, SP = speech.shape
    if B != bd.B or N > bd.chunk or N < 2 or SP != bd.SP or style.shape[2] != bd.ST:
        raise ValueError(f"decoder_batch_chunk: [{B},{N}] rows x frames on a BatchDecode of [{bd.B},<={bd.chunk}]")
    _route(current())
    L = api()
    dev = pose0.device
    d = bd.dims(N)
    pose = torch.empty(B, N, bd.PO, device=dev, dtype=torch.float32)
    rpos = torch.empty(B, N, 3, device=dev, dtype=torch.float32)
    rrot = torch.empty(B, N, 4, device=dev, dtype=torch.float32)
    h_out = torch.empty(2, B, bd.H, device=dev, dtype=torch.float32)
    watch = status is not None and not stage and not torch.cuda.is_current_stream_capturing() and _persistent_live(1)
    call = DecCall(bd.mask, 0, None, status.data_ptr() if status is not None else None, 0)

    def run(mode, gaze=gaze, speech=speech, style=style):
        L.zeggs_decoder_fwd_batch(d, bd.P, bd.S, pose0, rpos0, rrot0, gaze, speech, style, pose, rpos, rrot, h_in, h_out, bd.ws,
                                  bd.ws.numel(), _stream(), call, int(mode))
    run(1 if stage else 0)
    bits = 0
    if watch and batch_last_path() == "persistent":
        bits = int(status[0].item())
        if bits:
            _warn_gave_up(bits, "this chunk", disabled=False)
            COUNTERS["batch_chunks_redone"] = COUNTERS.get("batch_chunks_redone", 0) + 1
            fill_(status.view(torch.float32))
            # the stage launches do not keep what a row holds past its last valid frame away from that frame (0 * NaN in the
            # merged stage): the redo sees non-finite padding as 0, which is what the sweep made of it
            run(1, *(torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0) for t in (gaze, speech, style)))
    if info is not None:
        info["path"], info["gave_up"] = batch_last_path(), bits
    return pose, rpos, rrot, h_out


# ----------------------------------------------------------------------------- live serving (zeggs/live.py)
LIVE_MAX_ROWS = 64                 # ZEGGS_LIVE_MAX_ROWS


def mel_frames_ready(d, n_samples):
    """zeggs_mel_frames_ready (host only): animation frames computable from the first n_samples samples while the signal continues"""
    return api().zeggs_mel_frames_ready(d, int(n_samples))


MEL_FORMS = {0: None, 1: "fft", 2: "mfma", 3: "direct", 4: "fft_batch"}


def mel_last_form():
    """zeggs_mel_last_form: the STFT form this thread's last mel call enqueued -- 0 none yet, 1 FFT, 2 matrix-core DFT, 3 direct DFT,
    4 batched FFT (MEL_FORMS names them)"""
    return api().zeggs_mel_last_form()


def mel_window_first_sample(d, k0):
    """zeggs_mel_window_first_sample (host only): the smallest absolute sample index any frame >= k0 loads (d: audio.MelDims)"""
    return api().zeggs_mel_window_first_sample(d, int(k0))


def mel_range_workspace(d, n_frames, device, k0=0):
    """a workspace that serves every zeggs_mel_features_range / _window call of at most n_frames frames (k0: sized for the rows
    [k0, k0 + n_frames) exactly)"""
    return _ws(api().zeggs_mel_range_workspace_bytes(d, int(k0), int(k0) + int(n_frames)), device)


def _mel_out_fits(d, k0, k1, out):
    return out.shape[0] == k1 - k0 and out.shape[1] == d.n_mels + 1


def mel_features_window(d, wav_window, base, n_samples, final, filterbank, k0, k1, out, ws):
    """zeggs_mel_features_window: rows [k0, k1) of the feature table into `out` [k1 - k0, n_mels + 1] from a sliding window of the
    signal (wav_window[i] = sample base + i; n_samples = absolute count received so far)."""
    if not _mel_out_fits(d, k0, k1, out) or wav_window.numel() < n_samples - base:
        raise ValueError("mel_features_window: out / window do not match the range")
    api().zeggs_mel_features_window(d, wav_window, int(base), int(n_samples), int(bool(final)), filterbank, int(k0), int(k1), out, ws,
                                    ws.numel(), _stream())
    return out


def mel_features_range(d, wav, final, filterbank, k0, k1, out, ws):
    """zeggs_mel_features_range: the same rows from the whole signal received so far (`wav`: every sample from the first one on)"""
    if not _mel_out_fits(d, k0, k1, out):
        raise ValueError("mel_features_range: out does not match the range")
    api().zeggs_mel_features_range(d, wav, wav.numel(), int(bool(final)), filterbank, int(k0), int(k1), out, ws, ws.numel(), _stream())
    return out


class MelBatch:
    """The batched front-end's tables (zeggs_mel_batch_prepare: twiddles, window, packed filterbank -- once per dims and
    filterbank) and a workspace for calls of at most `rows` rows of at most `max_frames` feature rows each."""

    def __init__(self, d, filterbank, rows, max_frames, device):
        L = api()
        self.d, self.fb, self.rows = d, filterbank, int(rows)
        self.tables = _ws(L.zeggs_mel_batch_tables_bytes(d), device)
        L.zeggs_mel_batch_prepare(d, filterbank, self.tables, self.tables.numel(), _stream())
        self.resize(max_frames)

    def resize(self, max_frames):
        self.max_frames = int(max_frames)
        self.ws = _ws(api().zeggs_mel_batch_workspace_bytes(self.d, self.rows, self.max_frames), self.tables.device)


def _records(cls, address):
    """a device address as the pointer-to-record parameter of the second header's entry points (None: no device copy)"""
    return C.cast(C.c_void_p(int(address)), C.POINTER(cls)) if address else None


def mel_features_batch(mb, rows, n, rows_dev=None):
    """zeggs_mel_features_batch: rows[:n] a HOST array of MelRow (device addresses inside), `rows_dev` the device address of a copy
    of the same records (None: the library uploads them) -> what the call enqueued (2 launches on the FFT form whatever n is)"""
    if not 1 <= n <= mb.rows or max(r.k1 - r.k0 for r in rows[:n]) > mb.max_frames:
        raise ValueError("mel_features_batch: more rows or frames than the MelBatch was sized for")
    L = api()
    L.zeggs_mel_features_batch(mb.d, rows, _records(MelRow, rows_dev), int(n), mb.fb, mb.tables, mb.ws, mb.ws.numel(), _stream())
    return L.zeggs_mel_batch_last_ops()


def copy_segments(segs, n, segs_dev):
    """zeggs_copy_segments: segs[:n] a HOST array of Seg (device addresses, counts in floats), segs_dev the device address of a
    copy of the same records: ONE launch for all of them"""
    api().zeggs_copy_segments(segs, _records(Seg, segs_dev), int(n), _stream())


class LiveLoudness:
    """The running loudness state of `rows` live rows (include/zeggs_hip_loudness.h): the dims record -- `coef`, the K-weighting
    biquads for `fs` as [(b, a), (b, a)] (audio._kweighting), the estimate's look-back of `ring_blocks` gating blocks (10 per
    second), `warmup`, `target` LUFS, the gain's bounds in dB -- and the state buffer, every row reset to gain 1."""

    def __init__(self, fs, rows, ring_blocks, warmup, target, gain_db, coef, device):
        coef = [c for b, a in coef for c in (b[0], b[1], b[2], a[1], a[2])]
        self.d = LoudDims(int(fs), int(rows), int(ring_blocks), int(warmup), float(target), float(gain_db[0]), float(gain_db[1]),
                          (C.c_double * 10)(*coef))
        nbytes = api().zeggs_live_loudness_state_bytes(self.d)
        if nbytes == 0:
            raise ValueError(f"LiveLoudness: {api().zeggs_last_error().decode()}")
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        for r in range(int(rows)):
            live_loudness_reset(self, r, 1.0)


def live_loudness_reset(ll, row, gain=1.0):
    """zeggs_live_loudness_reset: the row starts from nothing at gain `gain`"""
    api().zeggs_live_loudness_reset(ll.d, ll.state, ll.state.numel(), int(row), float(gain), _stream())


def live_loudness_hold(ll, row, on=True):
    """zeggs_live_loudness_hold: freeze (or release) the row's gain; it goes on metering"""
    api().zeggs_live_loudness_hold(ll.d, ll.state, ll.state.numel(), int(row), int(bool(on)), _stream())


def live_loudness_push(ll, rows, n, rows_dev=None):
    """zeggs_live_loudness_push: rows[:n] a HOST array of LoudRow (device addresses, counts in samples), `rows_dev` the device address
    of a copy of the same records (None: one record, in the kernel arguments): ONE launch for all of them"""
    api().zeggs_live_loudness_push(ll.d, rows, _records(LoudRow, rows_dev), int(n), ll.state, ll.state.numel(), _stream())


def live_loudness_read(ll, row):
    """zeggs_live_loudness_read (waits for the stream) -> dict(lufs, gain, blocks, gated, held, samples, hold)"""
    out = (C.c_double * 8)()
    api().zeggs_live_loudness_read(ll.d, ll.state, ll.state.numel(), int(row), C.addressof(out), _stream())
    return dict(lufs=out[0], gain=out[1], blocks=int(out[2]), gated=int(out[3]), held=bool(out[4]), samples=int(out[5]), hold=bool(out[6]))


RS_F32, RS_S16 = 0, 1              # ZEGGS_RS_F32 / ZEGGS_RS_S16
RS_FORMATS = {"f32": RS_F32, "s16": RS_S16}


class LiveResample:
    """The rate converter of `rows` live rows (include/zeggs_hip_resample.h): the state -- per row a ring of past input samples,
    sized for the largest supported decimation at the server's `zero_crossings` -- and the coefficient tables on the device, one
    per input rate, built in float64 (audio.resample_table) and uploaded when a row first asks for the rate (open(), never on
    the tick path).  `fo`: the server's rate; `options`: audio.resample_options()."""

    def __init__(self, fo, rows, options, device):
        from . import audio
        self.fo, self.options, self.dev = int(fo), audio.resample_options(options), torch.device(device)
        self.d = ResampleDims(int(rows), 2 * self.options["zero_crossings"] * audio.RESAMPLE_MAX_DECIMATION)
        nbytes = api().zeggs_resample_state_bytes(self.d)
        if nbytes == 0:
            raise ValueError(f"LiveResample: {api().zeggs_last_error().decode()}")
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)
        self.tables = {}

    def table(self, fi):
        """-> dict(table: float64 tensor on the device, L, M, WL) for input rate `fi` (fi == fo: the pass-through table, one tap
        of 1.0); ValueError for a rate the converter does not take"""
        from . import audio
        fi = int(fi) if fi == int(fi) else fi
        if fi not in self.tables:
            if fi == self.fo:
                tab, (L, M, WL) = np.ones((1, 1)), (1, 1, 0)
            else:
                tab, (L, M, WL) = audio.resample_table(fi, self.fo, **self.options)
            self.tables[fi] = dict(table=torch.as_tensor(tab).to(self.dev).contiguous(), L=L, M=M, WL=WL)
        return self.tables[fi]


def live_resample_reset(rs, row):
    """zeggs_resample_reset: the row's history is all zeros"""
    api().zeggs_resample_reset(rs.d, rs.state, rs.state.numel(), int(row), _stream())


def live_resample_push(rs, rows, n, rows_dev=None):
    """zeggs_resample_push: rows[:n] a HOST array of ResampleRow (device addresses, the caller's counters), `rows_dev` the device
    address of a copy of the same records (None: one record, in the kernel arguments): ONE launch for all of them"""
    api().zeggs_resample_push(rs.d, rows, _records(ResampleRow, rows_dev), int(n), rs.state, rs.state.numel(), _stream())


FRAMES_WHAT = {"local": 1, "world": 2, "bvh": 4}              # ZEGGS_FRAMES_LOCAL / _WORLD / _BVH
FRAMES_KEYS = {"local": ("root_pos", "root_rot", "lrot", "lpos"), "world": ("gpos", "grot"), "bvh": ("bvh",)}


def frames_what(what):
    """("local", "world", "bvh") -> the bit mask of ZeggsFramesDims.what; ValueError for an unknown or an empty selection"""
    try:
        names = (what,) if isinstance(what, str) else tuple(what)
    except TypeError:
        names = ()
    if not names or any(not isinstance(n, str) or n not in FRAMES_WHAT for n in names):
        raise ValueError(f"frames: what {what!r} (one or more of {sorted(FRAMES_WHAT)})")
    return sum(FRAMES_WHAT[n] for n in set(names))


def frames_seq(parents):
    """the joint order of the BVH file (anim.bvh_header: depth first, children in index order) for `parents`; ValueError where
    the entry points would refuse the skeleton (parents[0] != -1, a parent that does not come before its child)"""
    parents = [int(p) for p in parents]
    if not parents or parents[0] != -1 or any(not 0 <= p < j for j, p in enumerate(parents) if j):
        raise ValueError("frames: parents[0] is -1 and every other joint's parent comes before it")
    children = [[j for j, p in enumerate(parents) if p == i] for i in range(len(parents))]
    seq, todo = [], [0]
    while todo:
        i = todo.pop()
        seq.append(i)
        todo.extend(reversed(children[i]))
    return seq


class LiveFrames:
    """The output head of `rows` live rows (include/zeggs_hip_frames.h): the dims record and the state buffer -- the skeleton
    tables (`parents`, and `seq`, the joint order of the BVH rows: frames_seq(parents) unless given) and per row the placement
    and the quaternions last emitted.  `what`: names or the bit mask; `order`: "zyx" or "xzy"."""

    # the form's entry points and its record (LiveRetime: the sixth header's, LiveRefilter: the seventh's) -- read by the constructor,
    # live_head_reset, live_head_launch and live_frames_spans; a server asks the head object, never which form it is
    state_bytes, prepare = "zeggs_live_frames_state_bytes", "zeggs_live_frames_prepare"
    reset, launch, spans = "zeggs_live_frames_reset", "zeggs_live_frames", "zeggs_live_frames_spans"
    record = FramesRow
    extra = ()                                   # what the entry points take behind the dims (LiveRefilter: max_half)

    def __init__(self, rows, parents, max_frames, what=("local", "world", "bvh"), order="zyx", seq=None, device="cuda"):
        from . import anim
        self.parents = [int(p) for p in parents]
        self.seq = frames_seq(self.parents) if seq is None else [int(k) for k in seq]
        self.what = what if isinstance(what, int) else frames_what(what)
        self.J = len(self.parents)
        self.d = FramesDims(int(rows), self.J, int(max_frames), self.what, anim._to_euler_order(order))
        nbytes = getattr(api(), self.state_bytes)(self.d, *self.extra)
        if nbytes == 0:
            raise ValueError(f"{type(self).__name__}: {api().zeggs_last_error().decode()}")
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        if len(self.seq) != self.J:
            raise ValueError(f"{type(self).__name__}: seq has {len(self.seq)} entries for {self.J} joints")
        getattr(api(), self.prepare)(self.d, *self.extra, (C.c_int * self.J)(*self.parents), (C.c_int * self.J)(*self.seq), self.state,
                                     self.state.numel(), _stream())
        self.local_floats, self.world_floats, self.bvh_doubles = 7 + 7 * self.J, 7 * self.J, 3 + 3 * self.J


def live_head_reset(lf, row, ref_pos=None, ref_rot=None, start_pos=None, start_rot=None):
    """the reset of lf's form (zeggs_live_frames_reset / zeggs_live_retime_reset / zeggs_live_refilter_reset): the row's next input
    frame is the first of a stream; with a placement (all four given) the root is re-based: start_rot ref_rot^-1 (x - ref_pos) +
    start_pos"""
    place = [ref_pos, ref_rot, start_pos, start_rot]
    reset = getattr(api(), lf.reset)
    if all(p is None for p in place):
        reset(lf.d, *lf.extra, lf.state, lf.state.numel(), int(row), None, None, None, None, 0, _stream())
        return
    arrs = [(t * n)(*[float(v) for v in p]) for p, t, n in zip(place, (C.c_float, C.c_float, C.c_double, C.c_double), (3, 4, 3, 4))]
    reset(lf.d, *lf.extra, lf.state, lf.state.numel(), int(row), *arrs, 1, _stream())


def live_head_launch(lf, rows, n, rows_dev=None):
    """the launch of lf's form (zeggs_live_frames / zeggs_live_frames_retimed / zeggs_live_frames_refiltered): rows[:n] a HOST array
    of lf.record (device addresses inside; the re-timing forms: the caller's counters; the filtered form: half = 0 for a row
    without the filter), `rows_dev` the device address of a copy of the same records (None: one record, in the kernel arguments):
    ONE launch for all of them"""
    getattr(api(), lf.launch)(lf.d, *lf.extra, rows, _records(lf.record, rows_dev), int(n), lf.state, lf.state.numel(), _stream())


# the names of the three headers' calls: the form is the head object's
live_frames_reset = live_retime_reset = live_refilter_reset = live_head_reset
live_frames = live_frames_retimed = live_frames_refiltered = live_head_launch


RETIME_MAX_TERM, RETIME_MAX_UP = 4096, 8         # csrc/retime_math.h: 1 <= L, M <= 4096 and L / M <= 8


def retime_ratio(frame_rate, fps):
    """frame_rate / fps = L / M in lowest terms -> (L, M).  `frame_rate`: an int, a fractions.Fraction, a (num, den) pair or a float
    (taken as Fraction(str(x))); `fps` likewise.  ValueError naming both rates for a rate that is not positive and for a ratio
    outside 1 <= L, M <= 4096, L / M <= 8."""
    from fractions import Fraction

    def frac(x):
        if isinstance(x, bool):
            raise TypeError
        if isinstance(x, (tuple, list)):
            num, den = x
            return Fraction(frac(num), frac(den))
        if isinstance(x, (float, np.floating)):
            return Fraction(str(float(x)))
        return Fraction(x)
    try:
        a, b = frac(frame_rate), frac(fps)
        if a <= 0 or b <= 0:
            raise ValueError
        r = a / b
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError(f"retime: frame rate {frame_rate!r} on a server at {fps!r} frames per second: not a positive rate") from None
    L, M = r.numerator, r.denominator
    if L > RETIME_MAX_TERM or M > RETIME_MAX_TERM or L > RETIME_MAX_UP * M:
        raise ValueError(f"retime: frame rate {frame_rate!r} on a server at {fps!r} frames per second is the ratio {L} / {M} "
                         f"(supported: 1 <= L, M <= {RETIME_MAX_TERM} in lowest terms and L / M <= {RETIME_MAX_UP})")
    return int(L), int(M)


def retime_n_out(n, L, M):
    """output frames a stream has emitted after n input frames: ((n - 1) L) div M + 1, 0 for n = 0"""
    return 0 if n < 1 else ((int(n) - 1) * int(L)) // int(M) + 1


def retime_position(m, L, M):
    """output frame m sits at input position m M / L -> (k, num): k + num / L"""
    return divmod(int(m) * int(M), int(L))


def retime_max_outputs(count, L, M):
    """the most output frames a record of `count` input frames can give: ceil(count L / M) + 1"""
    return 0 if count < 1 else -(-int(count) * int(L) // int(M)) + 1


class LiveRetime(LiveFrames):
    """The output head of `rows` live rows at each row's own frame rate (include/zeggs_hip_retime.h): LiveFrames' dims record and
    tables, the rows' state with the last input frame kept raw behind the plain head's fields.  `max_frames` bounds the INPUT
    frames of a record."""

    state_bytes, prepare = "zeggs_live_retime_state_bytes", "zeggs_live_retime_prepare"
    reset, launch, spans = "zeggs_live_retime_reset", "zeggs_live_frames_retimed", "zeggs_live_retime_spans"
    record = RetimeRow


REFILTER_MAX_L, REFILTER_MAX_DOWN, REFILTER_MAX_Z = 1024, 4, 8        # csrc/refilter_math.h: a filtered row has L <= 1024, M <= 4 L
REFILTER_DEFAULTS = dict(zero_crossings=4, rolloff=0.75, beta=5.0)


def refilter_options(options=None):
    """dict(zero_crossings, rolloff, beta) over REFILTER_DEFAULTS, checked: zero_crossings an integer 1 .. 8, 0 < rolloff <= 1,
    beta >= 0 and finite; True or None: the defaults.  Anything else raises ValueError."""
    if options is None or options is True:
        options = {}
    if not isinstance(options, dict) or set(options) - set(REFILTER_DEFAULTS):
        raise ValueError(f"refilter: filter is True or a dict with keys {sorted(REFILTER_DEFAULTS)}")
    o = dict(REFILTER_DEFAULTS, **options)
    try:
        Z, rolloff, beta = int(o["zero_crossings"]), float(o["rolloff"]), float(o["beta"])
    except (TypeError, ValueError):
        raise ValueError(f"refilter: options {options!r}") from None
    if isinstance(o["zero_crossings"], bool) or Z != o["zero_crossings"] or not 1 <= Z <= REFILTER_MAX_Z:
        raise ValueError(f"refilter: zero_crossings {o['zero_crossings']} (an integer 1 .. {REFILTER_MAX_Z})")
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"refilter: rolloff {rolloff} (0 < rolloff <= 1)")
    if not (np.isfinite(beta) and beta >= 0.0):
        raise ValueError(f"refilter: beta {beta} (>= 0)")
    return dict(zero_crossings=Z, rolloff=rolloff, beta=beta)


def refilter_half(L, M, zero_crossings):
    """H = ceil(W), W = zero_crossings max(L, M) / L: the input frames the filter reaches to either side (2 H + 1 taps)"""
    return -(-int(zero_crossings) * max(int(L), int(M)) // int(L))


def refilter_n_out(n, L, M, H):
    """output frames a filtered stream has emitted after n input frames while it runs: 0 for n <= H, else
    ((n - H) L - 1) div M + 1 (output m leaves with input frame k + H); a closed stream has retime_n_out(n)"""
    n, H = int(n), int(H)
    return 0 if n <= H else ((n - H) * int(L) - 1) // int(M) + 1


def refilter_table(L, M, zero_crossings=4, rolloff=0.75, beta=5.0):
    """The filter's coefficients in float64 -> (table [L, 2 H + 1], H): audio.sinc_table (the audio converter's h), each phase
    row divided by its own sum accumulated in ascending j -- unit DC gain per phase, a pose held still stays that pose.
    ValueError for a ratio a filtered row does not take (L > 1024 or M > 4 L)."""
    from . import audio
    L, M = int(L), int(M)
    if L < 1 or M < 1 or L > REFILTER_MAX_L or M > REFILTER_MAX_DOWN * L:
        raise ValueError(f"refilter: the ratio {L} / {M} (a filtered row takes L <= {REFILTER_MAX_L} and M <= {REFILTER_MAX_DOWN} L)")
    o = refilter_options(dict(zero_crossings=zero_crossings, rolloff=rolloff, beta=beta))
    table, _ = audio.sinc_table(L, M, o["zero_crossings"], o["rolloff"], o["beta"])
    total = np.zeros(L)
    for j in range(table.shape[1]):
        total = total + table[:, j]
    return np.ascontiguousarray(table / total[:, None]), refilter_half(L, M, o["zero_crossings"])


class LiveRefilter(LiveFrames):
    """The re-timing output head with its filter stage for `rows` live rows (include/zeggs_hip_refilter.h): LiveFrames' dims record
    and tables, per row the plain head's state and a ring of the last 2 max_half input frames, and the filter's tables per ratio
    on the device (`options`: refilter_options).  `max_frames` bounds the INPUT frames of a record, `max_half` the H of a row."""

    state_bytes, prepare = "zeggs_live_refilter_state_bytes", "zeggs_live_refilter_prepare"
    reset, launch, spans = "zeggs_live_refilter_reset", "zeggs_live_frames_refiltered", "zeggs_live_refilter_spans"
    record = RefilterRow

    def __init__(self, rows, parents, max_frames, max_half, options=None, what=("local", "world", "bvh"), order="zyx", seq=None, device="cuda"):
        self.max_half, self.options = int(max_half), refilter_options(options)
        self.extra = (self.max_half,)
        self.tables = {}
        super().__init__(rows, parents, max_frames, what, order, seq, device)

    def table(self, L, M):
        """-> dict(table: float64 tensor [L, 2 H + 1] on the device, half: H) for the ratio L / M, built and uploaded the first
        time a row opens at it; ValueError for a ratio a filtered row does not take or an H above max_half"""
        key = (int(L), int(M))
        if key not in self.tables:
            tab, H = refilter_table(*key, **self.options)
            if H > self.max_half:
                raise ValueError(f"refilter: the ratio {key[0]} / {key[1]} needs {H} input frames to either side, max_half is {self.max_half}")
            self.tables[key] = dict(table=torch.as_tensor(tab).to(self.state.device).contiguous(), half=H)
        return self.tables[key]


SNAP_MAX_SPANS, SNAP_MAX_SEGMENTS = 2, 65535       # ZEGGS_SNAP_MAX_SPANS / ZEGGS_SNAP_MAX_SEGMENTS


def _spans(fn, *args):
    """a span report of include/zeggs_hip_snapshot.h -> [(offset, bytes)] into the family's state block (host only)"""
    out = (SnapSpan * SNAP_MAX_SPANS)()
    n = fn(*args, out, SNAP_MAX_SPANS)
    return [(int(out[i].offset), int(out[i].bytes)) for i in range(n)]


def live_loudness_spans(ll, row):
    """zeggs_live_loudness_spans: where row `row` lives in ll.state -> [(offset, bytes)]"""
    return _spans(api().zeggs_live_loudness_spans, ll.d, int(row))


def live_resample_spans(rs, row):
    """zeggs_resample_spans: where row `row` lives in rs.state -> [(offset, bytes)]"""
    return _spans(api().zeggs_resample_spans, rs.d, int(row))


def live_frames_spans(lf, row):
    """zeggs_live_frames_spans / zeggs_live_retime_spans / zeggs_live_refilter_spans, by the head's form: where row `row` lives in
    lf.state -> [(offset, bytes)] (the skeleton tables in front of the rows are derived, not state: in no span)"""
    return _spans(getattr(api(), lf.spans), lf.d, *lf.extra, int(row))


def live_pack(segs, n, segs_dev, blob, blob_bytes):
    """zeggs_live_pack: segs[:n] a HOST array of SnapSeg (src: a device address; dst_offset, bytes: its place in the blob),
    segs_dev the device address of a copy of the same records, `blob` the blob's device address: ONE launch gathers them all"""
    api().zeggs_live_pack(segs, _records(SnapSeg, segs_dev), int(n), blob, int(blob_bytes), _stream())


def live_unpack(segs, n, segs_dev, blob, blob_bytes):
    """zeggs_live_unpack: the records of live_pack with the direction reversed -- `src` is written: ONE launch scatters them all"""
    api().zeggs_live_unpack(segs, _records(SnapSeg, segs_dev), int(n), blob, int(blob_bytes), _stream())


GAZE_SPACES = {"world": 0, "root": 1}              # ZEGGS_GAZE_WORLD / ZEGGS_GAZE_ROOT
GAZE_PATHS = {"line": 0, "arc": 1}                 # ZEGGS_GAZE_LINE / ZEGGS_GAZE_ARC
GAZE_EASES = {"linear": 0, "smooth": 1}            # ZEGGS_GAZE_LINEAR / ZEGGS_GAZE_SMOOTH


class LiveGaze:
    """The gaze schedules of `rows` live rows (include/zeggs_hip_gaze.h): the dims record -- `ST` floats per style row, which the
    condition launch writes beside the gaze rows -- and the state block, 64 bytes a row (zeroes: a row is reset when it opens)."""

    def __init__(self, rows, ST, device):
        self.d = GazeDims(int(rows), int(ST))
        nbytes = api().zeggs_live_gaze_state_bytes(self.d)
        if nbytes == 0:
            raise ValueError(f"LiveGaze: {api().zeggs_last_error().decode()}")
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=device)


def live_gaze_reset(lg, row, gaze0):
    """zeggs_live_gaze_reset: the row looks at gaze0 (a float32 tensor of 3 on the device) from now on"""
    api().zeggs_live_gaze_reset(lg.d, lg.state, lg.state.numel(), int(row), gaze0, _stream())


def live_gaze_set(lg, recs, n, rpos, rrot, recs_dev=None):
    """zeggs_live_gaze_set: recs[:n] a HOST array of GazeSet, `recs_dev` the device address of a copy of the same records (None: one
    record, in the kernel arguments); rpos [rows, 3] / rrot [rows, 4]: the rows' root state on the device: ONE launch"""
    api().zeggs_live_gaze_set(lg.d, recs, _records(GazeSet, recs_dev), int(n), rpos, rpos.stride(0), rrot, rrot.stride(0), lg.state,
                              lg.state.numel(), _stream())


def live_condition(lg, recs, n, sty_old, sty_new, gaze_out, style_out, recs_dev=None):
    """zeggs_live_condition: recs[:n] a HOST array of GazeCond (`recs_dev` as above); gaze_out [B, T, 3] and style_out [B, T, ST]
    take, in slice out_row, the gaze and style rows of the record's frames: ONE launch for all of them"""
    api().zeggs_live_condition(lg.d, recs, _records(GazeCond, recs_dev), int(n), lg.state, lg.state.numel(), sty_old, sty_new, gaze_out,
                               style_out, int(gaze_out.shape[0]), int(gaze_out.shape[1]), _stream())


def live_gaze_read(lg, row, frame):
    """zeggs_live_gaze_read (waits for the stream) -> dict(target: what `frame` looks at, k, fade, start, end, pivot, path, ease)"""
    out = (C.c_double * 16)()
    api().zeggs_live_gaze_read(lg.d, lg.state, lg.state.numel(), int(row), int(frame), C.addressof(out), _stream())
    v3 = lambda i: np.array(out[i:i + 3], np.float64).astype(np.float32)  # noqa: E731
    name = lambda table, v: [k for k, c in table.items() if c == int(v)][0]  # noqa: E731
    return dict(target=v3(0), k=int(out[3]), fade=int(out[4]), start=v3(5), end=v3(8), pivot=v3(11), path=name(GAZE_PATHS, out[14]),
                ease=name(GAZE_EASES, out[15]))


def live_gaze_spans(lg, row):
    """zeggs_live_gaze_spans: where row `row` lives in lg.state -> [(offset, bytes)]"""
    return _spans(api().zeggs_live_gaze_spans, lg.d, int(row))


PLANT_MAX_CHAINS = 4                                # ZEGGS_PLANT_MAX_CHAINS
PLANT_AUTO = (("RightUpLeg", "RightLeg", "RightFoot"), ("LeftUpLeg", "LeftLeg", "LeftFoot"))
# NOT tuned on captured motion (no dataset was at hand when they were chosen): speeds in model units a second, lengths in model units
PLANT_DEFAULTS = dict(chains="auto", speed=(15.0, 30.0), height=(12.0, 16.0), ground=0.0, slack=8.0, release=8, stretch=0.999)


def plant_options(plant, parents, names=None):
    """the `plant` options (a dict with keys of PLANT_DEFAULTS, or True: the defaults) against a skeleton -> dict(chains: [(u, m, e)]
    joint indices, speed, height, ground, slack, release, stretch).  A chain is three joints given by name or by index with
    parents[m] == u and parents[e] == m; "auto" picks PLANT_AUTO's triples where `names` holds them.  ValueError for anything
    else, the chain named: an unknown name, an index out of range, joints that are no chain, a joint in two chains, no chain or
    more than PLANT_MAX_CHAINS, thresholds with on > off, a negative slack or release, a stretch outside (0, 1]."""
    if plant is True:
        plant = {}
    if not isinstance(plant, dict) or set(plant) - set(PLANT_DEFAULTS):
        raise ValueError(f"plant: True or a dict with keys {sorted(PLANT_DEFAULTS)}")
    o = dict(PLANT_DEFAULTS, **plant)
    parents = [int(p) for p in parents]
    names = None if names is None else [str(n) for n in names]
    chains = o["chains"]
    if isinstance(chains, str):
        if chains != "auto":
            raise ValueError(f"plant: chains {chains!r} ('auto' or a list of (upper leg, lower leg, foot) triples)")
        chains = [c for c in PLANT_AUTO if names is not None and all(n in names for n in c)]
        if not chains:
            raise ValueError(f"plant: chains 'auto' needs joint names that hold {' or '.join(str(c) for c in PLANT_AUTO)}")
    try:
        chains = [tuple(c) for c in chains]
    except TypeError:
        raise ValueError(f"plant: chains {o['chains']!r} ('auto' or a list of (upper leg, lower leg, foot) triples)") from None
    if not 1 <= len(chains) <= PLANT_MAX_CHAINS:
        raise ValueError(f"plant: {len(chains)} chains (1..{PLANT_MAX_CHAINS})")
    out, taken = [], set()
    for c in chains:
        if len(c) != 3:
            raise ValueError(f"plant: chain {c!r} is not (upper leg, lower leg, foot)")
        idx = []
        for j in c:
            if isinstance(j, str):
                if names is None or j not in names:
                    raise ValueError(f"plant: chain {c!r}: no joint named {j!r}")
                idx.append(names.index(j))
            elif isinstance(j, (int, np.integer)) and not isinstance(j, bool) and 0 <= int(j) < len(parents):
                idx.append(int(j))
            else:
                raise ValueError(f"plant: chain {c!r}: joint {j!r} (a name or an index in 0..{len(parents) - 1})")
        u, m, e = idx
        if parents[m] != u or parents[e] != m:
            raise ValueError(f"plant: chain {c!r} is no chain: the parent of {c[1]!r} is joint {parents[m]}, the parent of {c[2]!r} is joint {parents[e]}")
        if taken & set(idx) or len(set(idx)) != 3:
            raise ValueError(f"plant: chain {c!r} shares a joint with an earlier chain")
        taken |= set(idx)
        out.append((u, m, e))
    pair = lambda k: tuple(float(x) for x in o[k]) if isinstance(o[k], (tuple, list)) and len(o[k]) == 2 else None  # noqa: E731
    speed, height = pair("speed"), pair("height")
    if speed is None or not 0.0 <= speed[0] <= speed[1] < float("inf"):
        raise ValueError(f"plant: speed {o['speed']!r} ((v_on, v_off) with 0 <= v_on <= v_off)")
    if height is None or not height[0] <= height[1] or not all(np.isfinite(height)):
        raise ValueError(f"plant: height {o['height']!r} ((h_on, h_off) with h_on <= h_off)")
    release = o["release"]
    if isinstance(release, bool) or not isinstance(release, (int, np.integer)) or not 0 <= int(release) <= 4096:
        raise ValueError(f"plant: release {release!r} (frames, 0..4096)")
    ground, slack, stretch = float(o["ground"]), float(o["slack"]), float(o["stretch"])
    if not np.isfinite(ground):
        raise ValueError(f"plant: ground {o['ground']!r}")
    if not 0.0 <= slack < float("inf"):
        raise ValueError(f"plant: slack {o['slack']!r} (>= 0)")
    if not 0.0 < stretch <= 1.0:
        raise ValueError(f"plant: stretch {o['stretch']!r} (0 < stretch <= 1)")
    return dict(chains=out, speed=speed, height=height, ground=ground, slack=slack, release=int(release), stretch=stretch)


class LivePlant:
    """The planting stage of `rows` live rows (include/zeggs_hip_plant.h): the dims record -- the thresholds of `conf`
    (plant_options) and the frame time `dt` -- and the state block: the skeleton's parents and the chain table, then per row the
    chains' contact states (zeroes: a row is reset when it opens)."""

    def __init__(self, rows, parents, max_frames, conf, dt, device="cuda"):
        self.parents, self.chains = [int(p) for p in parents], [tuple(c) for c in conf["chains"]]
        self.J, self.C = len(self.parents), len(self.chains)
        self.d = PlantDims(int(rows), self.J, int(max_frames), self.C, int(conf["release"]), 0, float(dt), conf["speed"][0], conf["speed"][1],
                           conf["height"][0], conf["height"][1], conf["ground"], conf["slack"], conf["stretch"])
        nbytes = api().zeggs_live_plant_state_bytes(self.d)
        if nbytes == 0:
            raise ValueError(f"LivePlant: {api().zeggs_last_error().decode()}")
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        flat = [j for c in self.chains for j in c]
        api().zeggs_live_plant_prepare(self.d, (C.c_int * self.J)(*self.parents), (C.c_int * len(flat))(*flat), self.state, self.state.numel(),
                                       _stream())
        self.pose_floats = 6 + 15 * self.J


def live_plant_reset(lp, row):
    """zeggs_live_plant_reset: every chain of the row FREE, its next frame the first of a stream"""
    api().zeggs_live_plant_reset(lp.d, lp.state, lp.state.numel(), int(row), _stream())


def live_plant(lp, recs, n, recs_dev=None):
    """zeggs_live_plant: recs[:n] a HOST array of PlantRow (device addresses inside), `recs_dev` the device address of a copy of the
    same records (None: one record, in the kernel arguments): ONE launch for all of them"""
    api().zeggs_live_plant(lp.d, recs, _records(PlantRow, recs_dev), int(n), lp.state, lp.state.numel(), _stream())


def live_plant_spans(lp, row):
    """zeggs_live_plant_spans: where row `row` lives in lp.state -> [(offset, bytes)]"""
    return _spans(api().zeggs_live_plant_spans, lp.d, int(row))


STYLE_MAX_TERMS, STYLE_MAX_SLOTS = 8, 4096         # ZEGGS_STYLE_MAX_TERMS / ZEGGS_STYLE_MAX_SLOTS


class LiveStyles:
    """The style bank of a live server (include/zeggs_hip_styles.h): the dims record, the bank [capacity, 2, ST] (a slot's mean
    row and its deviation row; zeroes) and the noise tensor [rows, STYLE_MAX_TERMS, ST] the sampling records of a mix read,
    slice r the noise of row r."""

    def __init__(self, rows, ST, capacity, device):
        self.d = StyleBankDims(int(rows), int(ST), int(capacity))
        nbytes = api().zeggs_live_style_bank_bytes(self.d)
        if nbytes == 0:
            raise ValueError(f"LiveStyles: {api().zeggs_last_error().decode()}")
        self.bank = torch.zeros(int(capacity), 2, int(ST), dtype=torch.float32, device=device)
        self.eps = torch.zeros(int(rows), STYLE_MAX_TERMS, int(ST), dtype=torch.float32, device=device)


def live_style_put(ls, slot, enc):
    """zeggs_live_style_put: slot `slot` of the bank from `enc`, a float32 row on the device of 2 ST floats (the style encoder's
    VAE output: mean | log-variance) or ST floats (a plain vector: deviation 0): ONE launch"""
    api().zeggs_live_style_put(ls.d, ls.bank, ls.bank.numel() * 4, int(slot), enc, int(enc.numel()), _stream())


def live_style_mix(ls, recs, n, sty_old, sty_new, recs_dev=None, eps=None):
    """zeggs_live_style_mix: recs[:n] a HOST array of StyleMix, `recs_dev` the device address of a copy of the same records (None:
    one record, in the kernel arguments); sty_old / sty_new [rows, ST] are rewritten in the rows the records name; `eps`: the
    noise tensor [., STYLE_MAX_TERMS, ST] the records' eps_row index (None: ls.eps): ONE launch for all of them"""
    eps = ls.eps if eps is None else eps
    api().zeggs_live_style_mix(ls.d, recs, _records(StyleMix, recs_dev), int(n), ls.bank, ls.bank.numel() * 4, eps, int(eps.shape[0]),
                               sty_old, sty_new, _stream())


def live_style_read(ls, slot=None, row=None, sty_old=None, sty_new=None):
    """zeggs_live_style_read (waits for the stream): slot= -> (mean, dev) of a bank slot; row= with the two style tensors ->
    (old, new) of a live row; float32 arrays of ST"""
    ST = ls.d.ST
    out = np.empty(2 * ST, np.float32)
    api().zeggs_live_style_read(ls.d, ls.bank, ls.bank.numel() * 4, -1 if slot is None else int(slot), sty_old, sty_new,
                                -1 if row is None else int(row), out.ctypes.data, _stream())
    return out[:ST].copy(), out[ST:].copy()


class LiveSpeech:
    """The speech encoder's weights in the layout of the incremental kernel (zeggs_speech_encoder_live_prepare, once) for `rows`
    rows with rings of `depth` frames; `feat_ld` / `out_ld`: rows per row block of the feature and output tensors of every call."""

    def __init__(self, speech_net, a_mean, a_std, rows, depth, feat_ld, out_ld):
        self.params = [_f32c(t) for t in (speech_net.layer0.weight, speech_net.layer0.bias, speech_net.layer1.weight,
                                          speech_net.layer1.bias, speech_net.layer2.weight, speech_net.layer2.bias)]
        H, F = self.params[0].shape[0], self.params[0].shape[1]
        O, KW = self.params[2].shape[0], self.params[2].shape[2]
        self.mean, self.std = _f32c(a_mean).reshape(-1), _f32c(a_std).reshape(-1)
        if self.mean.numel() not in (1, F) or self.std.numel() not in (1, F):
            raise ValueError("LiveSpeech: audio mean / std do not match the encoder's input size")
        self.mean, self.std = self.mean.expand(F).contiguous(), self.std.expand(F).contiguous()      # (scalars broadcast, as in torch)
        self.d = LiveDims(int(rows), F, H, O, KW, int(depth), int(feat_ld), int(out_ld))
        self.P = _ptrs(SpeechPtrs, SPEECH_FIELDS, self.params)
        L = api()
        self.ws = _ws(L.zeggs_speech_encoder_live_workspace_bytes(self.d), self.params[0].device)
        L.zeggs_speech_encoder_live_prepare(self.d, self.P, self.ws, self.ws.numel(), _stream())

    def dims(self, feat_ld=None, out_ld=None):
        d = self.d
        return LiveDims(d.R, d.F, d.H, d.O, d.KW, d.D, int(feat_ld or d.feat_ld), int(out_ld or d.out_ld))


def speech_encoder_live(ls, rows, feats, ring, out):
    """zeggs_speech_encoder_live: ONE launch for all rows.  rows: a sequence of R LiveRow; feats [R, feat_ld, F] un-normalised
    features (row r's new frames from row LiveRow.feat_off on), ring [R, D, H] the rows' layer-0 rings (updated in place),
    out [R, out_ld, O] (row r, index i: frame k0 + i; zero beyond n_out)."""
    d = ls.dims(feats.shape[1], out.shape[1])
    if len(rows) != d.R or tuple(feats.shape) != (d.R, d.feat_ld, d.F) or tuple(ring.shape) != (d.R, d.D, d.H) or \
            tuple(out.shape) != (d.R, d.out_ld, d.O):
        raise ValueError("speech_encoder_live: tensor shapes do not match the LiveSpeech")
    arr = (LiveRow * d.R)(*rows)
    api().zeggs_speech_encoder_live(d, ls.P, ls.mean, ls.std, arr, feats, ring, out, ls.ws, ls.ws.numel(), _stream())
    return out


# ----------------------------------------------------------------------------- free functions of the Networks layer
# (reference ZEGGS/modules.py:673-813; csrc/funcs.hip).  Differentiable: the reference's own training loop (INTEGRATION.md
# route 2) calls normalize / compute_KL_div inside its inline loss and back-propagates through them.
class _NormalizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        x = _f32c(x)
        W = x.shape[-1]
        y = torch.empty_like(x)
        api().zeggs_normalize_vec_fwd(x, y, x.numel() // max(W, 1), W, eps, _stream())
        ctx.save_for_backward(x)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        W = x.shape[-1]
        dx = torch.empty_like(x)
        api().zeggs_normalize_vec_bwd(x, _f32c(dy), dx, x.numel() // max(W, 1), W, ctx.eps, _stream())
        return dx, None


def normalize_vec(x, eps=1e-8):
    """x / (||x||_2 + eps) over the last dimension (reference modules.py:673-675)"""
    return _NormalizeFn.apply(x, float(eps))


class _VectorizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, root_pos, root_rot, root_vel, root_vrt, lpos, ltxy, lvel, lvrt, gaze_pos, in_mean, in_std):
        a = [_f32c(t) for t in (root_pos, root_rot, root_vel, root_vrt, lpos, ltxy, lvel, lvrt, gaze_pos)]
        in_mean, in_std = _f32c(in_mean), _f32c(in_std)
        B, J = a[4].shape[0], a[4].shape[1]
        out = torch.empty(B, 9 + 15 * J, device=a[0].device, dtype=torch.float32)
        api().zeggs_vectorize_input_fwd(B, J, *a, in_mean, in_std, out, _stream())
        ctx.save_for_backward(a[0], a[1], a[8], in_std)
        ctx.shapes = [t.shape for t in a]
        ctx.dims = (B, J)
        return out

    @staticmethod
    def backward(ctx, dout):
        root_pos, root_rot, gaze_pos, in_std = ctx.saved_tensors
        B, J = ctx.dims
        g = [torch.empty(sh, device=root_pos.device, dtype=torch.float32) for sh in ctx.shapes]
        api().zeggs_vectorize_input_bwd(B, J, root_pos, root_rot, gaze_pos, in_std, _f32c(dout), *g, _stream())
        return (*g, None, None)


def vectorize_input(root_pos, root_rot, root_vel, root_vrt, lpos, ltxy, lvel, lvrt, gaze_pos, in_mean, in_std):
    """-> [B, 9 + 15 J] normalised autoregressive input (reference modules.py:677-713)"""
    return _VectorizeFn.apply(root_pos, root_rot, root_vel, root_vrt, lpos, ltxy, lvel, lvrt, gaze_pos, in_mean, in_std)


class _DevectorizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, predicted, root_pos, root_rot, J, dt, out_mean, out_std):
        predicted, root_pos, root_rot, out_mean, out_std = (_f32c(t) for t in (predicted, root_pos, root_rot, out_mean,
                                                                                 out_std))
        B = predicted.shape[0]
        dev = predicted.device
        pose = torch.empty(B, 6 + 15 * J, device=dev, dtype=torch.float32)
        nrp = torch.empty(B, 3, device=dev, dtype=torch.float32)
        nrr = torch.empty(B, 4, device=dev, dtype=torch.float32)
        api().zeggs_devectorize_output_fwd(B, J, dt, predicted, root_pos, root_rot, out_mean, out_std, pose, nrp, nrr, _stream())
        ctx.save_for_backward(predicted, root_pos, root_rot, out_mean, out_std)
        ctx.dims = (B, J, dt)
        ctx.set_materialize_grads(False)
        return pose, nrp, nrr

    @staticmethod
    def backward(ctx, dpose, dnrp, dnrr):
        predicted, root_pos, root_rot, out_mean, out_std = ctx.saved_tensors
        B, J, dt = ctx.dims
        c = lambda g: _f32c(g) if g is not None else None  # noqa: E731
        dpred, drp, drr = torch.empty_like(predicted), torch.empty_like(root_pos), torch.empty_like(root_rot)
        api().zeggs_devectorize_output_bwd(B, J, dt, predicted, root_pos, root_rot, out_mean, out_std, c(dpose), c(dnrp), c(dnrr),
                                           dpred, drp, drr, _stream())
        return dpred, drp, drr, None, None, None, None


def devectorize_output(predicted, root_pos, root_rot, njoints, dt, out_mean, out_std):
    """-> pose [B, 6 + 15 J] (de-normalised output vector), new root_pos [B,3], new root_rot [B,4] (reference modules.py:716-742)"""
    return _DevectorizeFn.apply(predicted, root_pos, root_rot, int(njoints), float(dt), out_mean, out_std)


class _KLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, logvar):
        mu, logvar = _f32c(mu), _f32c(logvar)
        out = torch.empty((), device=mu.device, dtype=torch.float32)
        api().zeggs_kl_div_fwd(mu, logvar, mu.shape[0], mu.numel() // mu.shape[0], out, _stream())
        ctx.save_for_backward(mu, logvar)
        return out

    @staticmethod
    def backward(ctx, dout):
        mu, logvar = ctx.saved_tensors
        dmu, dlv = torch.empty_like(mu), torch.empty_like(logvar)
        api().zeggs_kl_div_bwd(mu, logvar, mu.shape[0], mu.numel() // mu.shape[0], _f32c(dout).reshape(1), dmu, dlv, _stream())
        return dmu, dlv


def kl_div(mu, logvar):
    """mean_b(-0.5 mean_s(1 + logvar - mu^2 - exp(logvar))) as a device scalar (reference modules.py:778-779)"""
    return _KLFn.apply(mu, logvar)


def mask_from_lengths(lengths):
    """bool [B, max(lengths)]: position < length (reference modules.py:802-813; like the reference's `torch.arange(0,
    max_len)` on a device scalar, sizing the result reads max(lengths) back to the host)"""
    lengths = lengths.to(torch.int64).contiguous()
    B = lengths.shape[0]
    max_len = int(lengths.max().item())
    mask = torch.empty(B, max_len, device=lengths.device, dtype=torch.uint8)
    api().zeggs_mask_from_lengths(lengths, B, max_len, mask, _stream())
    return mask.view(torch.bool)


# ----------------------------------------------------------------------------- loss
class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o_pose, o_rpos, o_rrot, mu, logvar, w_pose, w_rpos, w_rrot, gaze, parents, kl_weight, dt, gscale,
                unit_grad, truth_ws):
        o_pose, o_rpos, o_rrot, w_pose, w_rpos, w_rrot, gaze = (
            _f32c(t) for t in (o_pose, o_rpos, o_rrot, w_pose, w_rpos, w_rrot, gaze))
        B, T, PO = o_pose.shape
        J = (PO - 6) // 15
        has_kl = mu is not None and kl_weight > 0
        S = mu.shape[1] if mu is not None else 0
        d = LossDims(B, T, J, S, float(dt))
        L = api()
        dev = o_pose.device
        need = L.zeggs_loss_workspace_bytes(d)
        prepared = truth_ws is not None and truth_ws.numel() >= need       # (loss_prepare_truth filled its truth half)
        ws = truth_ws if prepared else _ws(need, dev)
        terms = torch.empty(19, device=dev, dtype=torch.float32)
        dpose, drpos, drrot = torch.empty_like(o_pose), torch.empty_like(o_rpos), torch.empty_like(o_rrot)
        dmu = torch.empty(B, S, device=dev) if mu is not None else None
        dlv = torch.empty(B, S, device=dev) if mu is not None else None
        L.zeggs_loss_fwd_bwd_ex(d, parents, o_pose, o_rpos, o_rrot, w_pose, w_rpos, w_rrot, gaze,
                                _f32c(mu) if mu is not None else None, _f32c(logvar) if mu is not None else None,
                                kl_weight if has_kl else 0.0, terms, dpose, drpos, drrot, dmu, dlv, gscale, ws, ws.numel(), _stream(),
                                int(prepared))
        ctx.save_for_backward(dpose, drpos, drrot, dmu, dlv)
        ctx.unit_grad = bool(unit_grad)
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)      # no zero-filled gradient for the (non-differentiable) terms vector
        loss = torch.empty((), device=dev, dtype=torch.float32)
        scale_copy(terms[18:19], out=loss)
        return loss, terms

    @staticmethod
    def backward(ctx, g, _gterms):
        dpose, drpos, drrot, dmu, dlv = ctx.saved_tensors
        if g is None:
            return (None,) * 15
        if not ctx.unit_grad:        # general case: scale by the upstream scalar (device side, no host sync)
            g = _f32c(g).reshape(1)
            dpose, drpos, drrot = scale_copy(dpose, g), scale_copy(drpos, g), scale_copy(drrot, g)
            if dmu is not None:
                dmu, dlv = scale_copy(dmu, g), scale_copy(dlv, g)
        return (dpose, drpos, drrot, dmu, dlv, None, None, None, None, None, None, None, None, None, None)


def loss_prepare_truth(w_pose, w_rpos, w_rrot, gaze, parents, dt, ws=None):
    """The ground-truth half of the loss's feature pass on the current stream (zeggs_loss_prepare_truth) -> the workspace to
    hand to training_loss(truth_ws=...) for the same batch.  `ws`: a workspace of an earlier call to use again when it fits."""
    w_pose, w_rpos, w_rrot, gaze = (_f32c(t) for t in (w_pose, w_rpos, w_rrot, gaze))
    B, T, PO = w_pose.shape
    d = LossDims(B, T, (PO - 6) // 15, 0, float(dt))
    L = api()
    need = int(L.zeggs_loss_workspace_bytes(d))
    if ws is None or ws.numel() != need or ws.device != w_pose.device:
        ws = _ws(need, w_pose.device)
    L.zeggs_loss_prepare_truth(d, parents, w_pose, w_rpos, w_rrot, gaze, ws, ws.numel(), _stream())
    return ws


def training_loss(o_pose, o_rpos, o_rrot, w_pose, w_rpos, w_rrot, gaze, parents, dt, mu=None, logvar=None,
                  kl_weight=0.0, gscale=1.0, unit_grad=False, truth_ws=None):
    """-> (loss scalar tensor, terms[19]); terms[0:18] are the reference's weighted loss terms.
    unit_grad=True: the caller promises to call backward() on the returned loss itself (upstream gradient 1), so
    the gradients computed in the fused forward+backward kernel are handed on without a scaling pass."""
    return _LossFn.apply(o_pose, o_rpos, o_rrot, mu, logvar, w_pose, w_rpos, w_rrot, gaze, parents,
                         float(kl_weight), float(dt), float(gscale), bool(unit_grad), truth_ws)


EVAL_COLS = 22                                     # ZEGGS_EVAL_COLS


def loss_eval(o_pose, o_rpos, o_rrot, w_pose, w_rpos, w_rrot, gaze, parents, dt, mu=None, logvar=None, rows=None, ws=None):
    """The loss section's forward alone, per window (zeggs_loss_eval) -> rows float64 [B, EVAL_COLS]: columns 0..16 the weighted
    L1 terms of each window, 17 its unweighted KL (0 without mu), 18 MPJPE, 19 root drift at the last frame, 20 / 21 mean joint
    speed of the prediction / the truth.  No gradient is built and nothing is differentiable.  `rows` / `ws`: the table of an
    earlier call / a workspace of loss_eval_workspace() to use again when they fit."""
    o_pose, o_rpos, o_rrot, w_pose, w_rpos, w_rrot, gaze = (_f32c(t) for t in (o_pose, o_rpos, o_rrot, w_pose, w_rpos, w_rrot, gaze))
    B, T, PO = o_pose.shape
    S = mu.shape[1] if mu is not None else 0
    d = LossDims(B, T, (PO - 6) // 15, S, float(dt))
    L = api()
    dev = o_pose.device
    need = int(L.zeggs_loss_eval_workspace_bytes(d))
    if ws is None or ws.numel() < need or ws.device != dev:
        ws = _ws(need, dev)
    if rows is None or tuple(rows.shape) != (B, EVAL_COLS) or rows.device != dev:
        rows = torch.empty(B, EVAL_COLS, device=dev, dtype=torch.float64)
    L.zeggs_loss_eval(d, parents, o_pose, o_rpos, o_rrot, w_pose, w_rpos, w_rrot, gaze, _f32c(mu) if mu is not None else None,
                      _f32c(logvar) if mu is not None else None, rows, ws, ws.numel(), _stream())
    return rows


class fixed_order_gemms:
    """`with ops.fixed_order_gemms():` -- the matrix products this thread launches inside the block never split their contraction
    over workgroups (zeggs_gemm_fixed_order): no fp32 atomics, so a forward pass is bitwise the same on every call."""

    def __enter__(self):
        self.prev = api().zeggs_gemm_fixed_order(1)

    def __exit__(self, *exc):
        api().zeggs_gemm_fixed_order(int(self.prev))
        return False


# route ids of zeggs_test_gemm_route_log (include/zeggs_hip.h: ZEGGS_GEMM_ROUTE_*), in the header's order
GEMM_ROUTES = ("none", "skinny", "m32-split", "m32", "mid-split", "streamk-direct", "streamk-bf16-split", "streamk-dma",
               "streamk-lds-128x128", "streamk-lds-256x128", "splitk", "half", "tile-128x128", "tile-64x64")
GEMM_SPLITTING_ROUTES = ("m32-split", "mid-split", "streamk-direct", "streamk-bf16-split", "streamk-dma", "streamk-lds-128x128",
                         "streamk-lds-256x128", "splitk")       # the routes that combine partial sums with fp32 atomics


def gemm_route_log(reset=False):
    """Test hook: the route log of the calling thread's matrix products (zeggs_test_gemm_route_log) with names instead of numbers ->
    {"route", "splitk" (1 unsplit, 0 stream-K), "tile": (BM, BN)} of the last product and "counts": {route: launches since the last
    reset} (routes never taken are left out).  reset: clear the log after reading it."""
    last, counts = (C.c_int * 4)(), (C.c_long * len(GEMM_ROUTES))()
    n = api().zeggs_test_gemm_route_log(int(bool(reset)), last, counts, len(GEMM_ROUTES))
    if n != len(GEMM_ROUTES):
        raise RuntimeError(f"zeggs.ops.GEMM_ROUTES names {len(GEMM_ROUTES)} routes, the library has {n}: rebuild it")
    return {"route": GEMM_ROUTES[last[0]], "splitk": int(last[1]), "tile": (int(last[2]), int(last[3])),
            "counts": {GEMM_ROUTES[i]: int(c) for i, c in enumerate(counts) if c}}


def loss_eval_workspace(B, T, J, S, dt, device):
    """a workspace for loss_eval calls of these dimensions (zeggs_loss_eval_workspace_bytes)"""
    d = LossDims(int(B), int(T), int(J), int(S), float(dt))
    return _ws(api().zeggs_loss_eval_workspace_bytes(d), device)


def eval_accumulate(rows, group, acc):
    """acc [groups, EVAL_COLS + 1] float64 += the rows of each group in ascending row order (zeggs_eval_accumulate); group: int32
    [B], a negative entry leaves its row out; the last column of acc counts the rows.  The caller zeroes acc once."""
    B, groups = rows.shape[0], acc.shape[0]
    assert rows.shape == (B, EVAL_COLS) and acc.shape == (groups, EVAL_COLS + 1) and group.shape == (B,)
    api().zeggs_eval_accumulate(rows, group, int(B), int(groups), acc, _stream())
    return acc


# ----------------------------------------------------------------------------- optimizer / data
def radam_step(p, g, m, v, beta1, beta2, eps, step_scale, rectified, status=None, gflag=None, count=True, decay=0.0):
    """status (int32[STATUS_WORDS], device): the guarded step -- a no-op on the device, counted in status[1], when a
    persistent sweep of the iteration gave up here (status[0]) or on another rank (gflag, a device float).  A step applied in
    pieces (slices of the flat buffers) counts its skip in ONE of them: count=False for the others.
    decay = weight_decay * lr (reference optimizers.py:88-95), 0 when the step is not applied."""
    # the complements in double, as the reference forms them: float(1 - 0.999) = 0.001f, while 1.f - 0.999f = 0.00099998713; the
    # kernel rounds them for the second moment and forms the first moment in double (zeggs_radam_step_d)
    api().zeggs_radam_step_d(p, g, m, v, p.numel(), beta1, beta2, 1 - beta1, 1 - beta2, eps, step_scale, int(rectified), decay, status,
                             gflag if status is not None else None, int(bool(count)), _stream())


def status_flag(status, dst):
    """dst[0] (device float) = 1.0 if status[0] has a give-up bit, else 0.0 -- the word that rides on the gradient all-reduce"""
    api().zeggs_status_flag(status, dst, _stream())


def gather_windows(frames, starts, T, out=None):
    """frames [N, W] device, starts int64 [B] device -> [B, T, W] (into `out` when it has that shape)"""
    B, W = starts.shape[0], frames.shape[1]
    if out is None or out.shape != (B, T, W) or not out.is_contiguous():
        out = torch.empty(B, T, W, device=frames.device, dtype=torch.float32)
    api().zeggs_gather_windows(frames, W, starts, B, T, out, _stream())
    return out


def gather_rows(frames, rows, out=None, out_ld=None):
    """frames [N, W], rows int64 [...]-> [..., W] (or into a strided `out`)"""
    W = frames.shape[1]
    n = rows.numel()
    if out is None:
        out = torch.empty(*rows.shape, W, device=frames.device, dtype=torch.float32)
        out_ld = W
    api().zeggs_gather_rows(frames, W, rows.contiguous(), n, out, int(out_ld), _stream())
    return out


def normalize_rows_(x, mean, std):
    """in place (x - mean) / std over the last dim; std is a [W] tensor or a python float"""
    W = x.shape[-1]
    rows = x.numel() // W
    vec = std if torch.is_tensor(std) and std.dim() > 0 else None
    sc = 1.0 if vec is not None else float(std)
    api().zeggs_normalize_rows(x, rows, W, W, mean, vec, sc, _stream())
    return x


_OPTIONS = capi.OPTIONS  # switches set through set_option / ZEGGS_OPTIONS (the library's defaults otherwise)
_PERSISTENT_OPTION = ("persistent", "train_persistent", "bwd_persistent")


def _persistent_live(which):
    """True if persistent kernel `which` (0 B=1 decode, 1 training rollout, 2 BPTT sweep) is switched on and validated on this
    process -- only then can a call have ended in an undetected give-up (an unvalidated kernel is checked, with a stream
    synchronisation, by the library itself)."""
    return _OPTIONS.get(_PERSISTENT_OPTION[which], 1) != 0 and api().zeggs_persistent_state(which) == 1


def set_option(name, value):
    """Runtime switches of the library (e.g. "decoder_fast": 1 packed stage kernels / 0 generic GEMM path)."""
    global _CHAIN_DIAGNOSTICS, _LAST_DECODER_WS
    api().zeggs_set_option(name.encode(), int(value))
    _OPTIONS[name] = int(value)
    if name == "chain":
        _CHAIN_DIAGNOSTICS = bool(value)
        if not value:
            _LAST_DECODER_WS = None
