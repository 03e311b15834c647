"""CPU tests of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/zeggs_hip.h declares, answers host-only queries, and the product path refuses to run
without a GPU (no CPU fallback)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from zeggs import modules, ops, synth

ROOT = Path(__file__).resolve().parent.parent


def test_library_exports_every_declared_symbol():
    header = (ROOT / "include" / "zeggs_hip.h").read_text()
    names = set(re.findall(r"\b(zeggs_[a-z0-9_]+)\s*\(", header))
    assert len(names) >= 18
    L = ops.lib()
    for n in sorted(names):
        assert hasattr(L, n), f"libzeggs_hip.so does not export {n}"
    assert L.zeggs_version() >= 100


def test_workspace_queries_run_on_host():
    L = ops.lib()
    d = ops.DecDims(32, 256, synth.POSE_IN, synth.POSE_OUT, 64, 64, 1024, synth.DT)
    train, infer = L.zeggs_decoder_workspace_bytes(ctypes.byref(d), 1), L.zeggs_decoder_workspace_bytes(ctypes.byref(d), 0)
    assert train > infer > 0
    s = ops.StyleDims(32, 512, synth.POSE_IN, 512, 128, 4, 1, 0)
    assert L.zeggs_style_encoder_workspace_bytes(ctypes.byref(s)) > 0
    sp = ops.SpeechDims(32, 256, 81, 64, 64, 31, 0.2, 1)
    assert L.zeggs_speech_encoder_workspace_bytes(ctypes.byref(sp)) > 0
    ld = ops.LossDims(32, 256, 75, 64, synth.DT)
    assert L.zeggs_loss_workspace_bytes(ctypes.byref(ld)) > 0


def test_gemm_routing_is_per_thread_not_per_process():
    """zeggs_gemm_route: a caller's routing of the TN products (what TrainEngine wants for its three-queue tail) is the calling
    THREAD's; the process-wide options stay what they were for every other thread, and -1 falls back to them (host-only check)."""
    import threading
    L = ops.lib()
    out = (ctypes.c_int * 4)()
    L.zeggs_gemm_route_get(out)
    base = list(out)
    L.zeggs_gemm_route(1, 1, 8, 32)
    L.zeggs_gemm_route_get(out)
    assert list(out) == [1, 1, 8, 32]
    seen = []

    def other():
        o = (ctypes.c_int * 4)()
        L.zeggs_gemm_route_get(o)
        seen.append(list(o))
    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == [base]                       # another thread: untouched
    L.zeggs_gemm_route(-1, -1, 6, -1)
    L.zeggs_gemm_route_get(out)
    assert list(out) == [base[0], base[1], 6, base[3]]
    L.zeggs_gemm_route(-1, -1, -1, -1)
    L.zeggs_gemm_route_get(out)
    assert list(out) == base
    # the Python side: a context's route becomes the thread's at the entry of its calls, the default context resets it
    ctx = ops.EngineContext()
    ctx.gemm_route = (1, 2, 4, 16)
    ops._route(ctx)
    L.zeggs_gemm_route_get(out)
    assert list(out) == [1, 2, 4, 16]
    ops._route(ops._DEFAULT_CTX)
    L.zeggs_gemm_route_get(out)
    assert list(out) == base
    # ... and a route leaves the thread with its context: a raw zeggs_gemm* call after the block gets the outer context's again
    with ops.use(ctx):
        ops._route(ctx)
        L.zeggs_gemm_route_get(out)
        assert list(out) == [1, 2, 4, 16]
    L.zeggs_gemm_route_get(out)
    assert list(out) == base


_SWEEP_STATE_CHILD = """
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
L.zeggs_last_error.restype = ctypes.c_char_p
out = {"fresh": [L.zeggs_persistent_state(w) for w in range(3)], "toggle": []}
for w, name in ((0, b"persistent"), (1, b"train_persistent"), (2, b"bwd_persistent")):
    out["toggle"].append([L.zeggs_set_option(name, 0), L.zeggs_set_option(name, 1), L.zeggs_persistent_state(w)])
out["unknown"] = [L.zeggs_set_option(b"no_such_option", 1), L.zeggs_last_error().decode()]
print(json.dumps(out))
"""


def test_persistent_sweep_state_before_any_launch():
    """The owner of the persistent kernels' option / first-use state, host only, in a process that has launched nothing: every
    kernel starts unused (-1); switching its option off and on again succeeds and leaves it unused (re-enabling re-arms only a
    kernel that FAILED its validation, state 0); an unknown option is still refused by name."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _SWEEP_STATE_CHILD, str(ops._LIB_PATH)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["fresh"] == [-1, -1, -1]
    assert out["toggle"] == [[0, 0, -1]] * 3
    assert out["unknown"][0] != 0 and "no_such_option" in out["unknown"][1]


# (B, T, SP = ST, H, film) at the synthetic skeleton's PI / PO -> zeggs_decoder_workspace_bytes(d, 0), (d, 1),
# zeggs_decoder_batch_workspace_bytes(d), recorded from the library before the decoder's host code was reorganised
_WORKSPACE_BYTES = {
    (1, 1801, 64, 1024, 0): (98534400, 3748302080, 982638592),
    (32, 256, 64, 1024, 0): (101411840, 1888559360, 448683008),
    (64, 256, 64, 1024, 0): (104864000, 3033404160, 665913600),
    (17, 4, 64, 1024, 0): (100260608, 425267200, 237296384),
    (19, 12, 64, 1024, 1): (123731200, 225796520, 123731200),
    (2, 5, 16, 64, 0): (2396416, 4514928, 2396416),
    (65, 4, 64, 1024, 0): (105438720, 220587192, 105438720),
    (4, 1, 64, 1024, 0): (98764544, 408307712, 232723200),
}


@pytest.mark.parametrize("dims", sorted(_WORKSPACE_BYTES))
def test_decoder_workspace_bytes_are_pinned(dims):
    """The carve of the decoder's workspace is an ABI of its own (a caller sizes its buffer by these queries, the prepare /
    forward / backward calls of one step must agree on every offset): the byte counts at the shapes that take each path --
    B = 1 decode, the persistent sweeps at 32 and 64 rows, an odd batch, FiLM, H = 64, the generic path at 65 rows, T = 1."""
    B, T, S, H, film = dims
    L = ops.lib()
    d = ops.DecDims(B, T, synth.POSE_IN, synth.POSE_OUT, S, S, H, synth.DT)
    d.film = film
    got = (L.zeggs_decoder_workspace_bytes(ctypes.byref(d), 0), L.zeggs_decoder_workspace_bytes(ctypes.byref(d), 1),
           L.zeggs_decoder_batch_workspace_bytes(ctypes.byref(d)))
    assert got == _WORKSPACE_BYTES[dims]


# every option name the library accepts, with its default
_OPTIONS = {
    "attn_bwd_one_launch": 1, "decoder_fast": 1, "stage_variant": 0, "gemm_wg_target": 6144, "timing": 0, "chain": 0,
    "sweep_graphs": 0, "launch_window": 8, "train_persistent": 1, "bwd_persistent": 1, "persistent": 1, "mel_mfma": 1,
    "mel_fft": 1, "gemm_streamk_wgs": 0, "gemm_mid_split": 1, "gemm_dma": 0, "gemm_direct": 1, "gemm_direct_wgs": 0,
    "gemm_direct_depth": 4, "gemm_direct_shield": 0, "gemm_direct_reserve": 0, "gemm_asum": 1, "gemm_skinny": 1,
    "gemm_streamk": 1, "fused_attention": 1, "bwd_chunks": 1, "tp_tiles4": 1, "tp_dual": 0, "tp_prologue": 1, "loss_lds": 1,
    "wgrad_order": 0, "gemm_split_bf16": 0, "poll_stagger": 0, "poll_sleep": 0, "persistent_spin": 1 << 21, "ln_bwd4": 1,
    "mel_exact_log": 2,
}

_OPTIONS_CHILD = """
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
L.zeggs_last_error.restype = ctypes.c_char_p
opts = json.loads(sys.argv[2])
out = {"set": {k: [L.zeggs_set_option(k.encode(), 0), L.zeggs_set_option(k.encode(), v)] for k, v in opts.items()}}
out["chain"] = [L.zeggs_set_option(b"chain", 1), L.zeggs_last_error().decode()]
out["unknown"] = [L.zeggs_set_option(b"no_such_option", 1), L.zeggs_last_error().decode()]
print(json.dumps(out))
"""


def test_every_option_is_still_accepted():
    """zeggs_set_option, host only, in a process of its own (the switches are process-wide): every name is accepted with 0 and
    with its default, `chain` is refused outside measurement builds with the build flag in the message, an unknown name is
    refused by name."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _OPTIONS_CHILD, str(ops._LIB_PATH), json.dumps(_OPTIONS)], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["set"] == {k: [0, 0] for k in _OPTIONS}
    assert out["chain"][0] != 0 and "ZEGGS_CHAIN" in out["chain"][1]
    assert out["unknown"][0] != 0 and "no_such_option" in out["unknown"][1]


def test_no_cpu_fallback():
    se = modules.SpeechEncoder(synth.N_AUDIO, 64, 64)
    with pytest.raises(RuntimeError, match="GPU"):
        se(torch.zeros(1, 4, synth.N_AUDIO))


def test_state_dict_keys_match_reference_layout():
    torch.manual_seed(0)
    de = modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, 64, 1024, 2)
    st = modules.StyleEncoder(synth.POSE_IN, 512, 64, type="attn", use_vae=True)
    keys = set(de.state_dict())
    for k in ("recurrent_decoder.layer0.weight", "recurrent_decoder.layer1.weight_ih_l0",
              "recurrent_decoder.layer1.bias_hh_l1", "recurrent_decoder.layer2.bias",
              "cell_state_encoder.layer2.weight"):
        assert k in keys
    skeys = set(st.state_dict())
    for k in ("encoder.convs.0.conv.weight", "encoder.convs.2.weight", "encoder.convs.6.bias",
              "encoder.blocks.0.attention.multi_head_attention.in_proj_weight",
              "encoder.blocks.0.attention.multi_head_attention.out_proj.bias",
              "encoder.blocks.0.attention.layer_norm.weight", "encoder.blocks.0.feed_forward.convs.2.conv.weight",
              "encoder.blocks.0.feed_forward.layer_norm.bias"):
        assert k in skeys
    assert sum(p.numel() for p in de.parameters()) == 23301227
    assert sum(p.numel() for p in st.parameters()) == 2105472


def test_streaming_frame_accounting_is_consistent_host_only():
    """zeggs_mel_frames_ready (host integer rule of the streaming front-end): monotone in the sample count, never
    promises a frame whose STFT support reaches past the received samples, and reaches the offline frame count's
    neighbourhood as the signal grows (the tail is flushed by the final call)."""
    import ctypes as C
    import math
    from zeggs import audio, ops
    L = ops.lib()
    L.zeggs_mel_frames_ready.restype = C.c_long
    for flags in (0, 1):        # centered (the shipped configuration) / uncentered frames (audio_conf.centered = false)
        _frame_accounting(L, audio.MelDims(800, 200, 80, 16000, 60.0, 1e-5, 0.0, flags), flags)


def _frame_accounting(L, d, flags):
    import ctypes as C
    import math
    from zeggs import audio
    prev = 0
    for n in list(range(0, 3000, 37)) + [16000, 16001, 48000, 480000]:
        k = int(L.zeggs_mel_frames_ready(C.byref(d), C.c_long(n)))
        assert k >= prev or n < 3000 and k >= 0
        prev = max(prev, k)
        for kk in (k - 1,):
            if kk >= 0:
                hi = max(math.ceil((80.0 / 60.0) * kk), 1)          # last STFT frame that animation frame kk interpolates
                assert 200 * hi + (800 if flags & 1 else 400) <= n, (n, kk, hi)      # its window ends inside the received samples
        assert k <= audio.n_anim_frames(n) + 1
    assert int(L.zeggs_mel_frames_ready(C.byref(d), C.c_long(480000))) >= audio.n_anim_frames(480000) - 3


# ----------------------------------------------------------------------------- the binding (zeggs/capi.py) against the header
_SCALARS = {"int": "int", "long": "long", "size_t": "size_t", "uint64_t": "uint64", "float": "float", "double": "double"}
_ELEMENTS = {"float": "f32*", "double": "f64*", "int": "i32*", "unsigned": "i32*", "int64_t": "i64*", "long": "i64*",
             "long long": "i64*", "uint8_t": "u8*", "unsigned char": "u8*", "char": "u8*", "void": "any*"}
_C_WORDS = {"int", "long", "unsigned", "char", "float", "double", "void", "size_t", "uint64_t", "int64_t", "uint8_t"}
_CTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
           "double": ctypes.c_double}


def _header_text():
    return re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "zeggs_hip.h").read_text(), flags=re.S)


def _declarator(text):
    """'const float* x' -> (base type, pointer depth, name or None, array length or None)"""
    m = re.search(r"\[(\d+)\]\s*$", text)
    text = text[:m.start()] if m else text
    depth = text.count("*")
    words = text.replace("*", " ").replace("const", " ").split()
    name = words.pop() if len(words) > 1 and words[-1] not in _C_WORDS and not words[-1].startswith("Zeggs") else None
    return " ".join(words), depth, name, int(m.group(1)) if m else None


def _header_prototypes():
    """{name: (return base type, return pointer depth, [(base type, pointer depth)])} of every zeggs_* function the header declares"""
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \*]*?)\b(zeggs_\w+)\s*\(([^()]*)\)\s*;", _header_text()):
        rbase, rdepth, _, _ = _declarator(ret + " f")
        plist = [] if params.strip() in ("", "void") else [_declarator(p)[:2] for p in params.split(",")]
        assert name not in out
        out[name] = (rbase, rdepth, plist)
    return out


def _header_structs():
    """{ZeggsX: [(field name, base type, pointer depth, array length or None)]} of every typedef struct of the header"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(Zeggs\w+)\s*;", _header_text(), flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = [p.strip() for p in decl.split(",")]
            base, depth, fname, n = _declarator(first)
            fields.append((fname, base, depth, n))
            for p in more:                       # `float *a, *b` / `int B, T`: every further declarator has its own stars
                m = re.fullmatch(r"(\**)\s*(\w+)(?:\[(\d+)\])?", p)
                fields.append((m.group(2), base, len(m.group(1)), int(m.group(3)) if m.group(3) else None))
        out[name] = fields
    return out


def test_prototype_table_is_the_header():
    """capi.PROTOTYPES against include/zeggs_hip.h: the same names; per function the return kind, the parameter count, every
    parameter's kind and every device pointer's element type.  A host pointer or a stream of the table is a pointer in the header."""
    from zeggs import capi
    header = _header_prototypes()
    assert len(header) == 122 and set(header) == set(capi.PROTOTYPES)
    assert {b for _, _, ps in header.values() for b, depth in ps if depth == 0} == set(_SCALARS)       # no struct by value
    for name, (rbase, rdepth, params) in header.items():
        ret, kinds = capi.signature(name)
        want = {("int", 0): ("status", "mask", "int"), ("long", 0): ("long",), ("size_t", 0): ("size_t",), ("char", 1): ("str",)}
        assert ret in want[(rbase, rdepth)], (name, ret)
        assert len(kinds) == len(params), name
        for i, (kind, (base, depth)) in enumerate(zip(kinds, params)):
            where = (name, i, kind, base, depth)
            assert kind in capi.KINDS, where
            if depth == 0:
                assert kind == _SCALARS[base], where
            elif kind == "str":
                assert (base, depth) == ("char", 1), where
            elif kind == "stream":
                assert (base, depth) == ("void", 1), where
            elif kind == "host*":
                assert depth >= 1, where
            elif base.startswith("Zeggs"):
                assert kind == base + "*" and depth == 1 and base in capi.STRUCTS, where
            else:
                assert depth == 1 and kind == _ELEMENTS[base], where


def test_struct_mirrors_are_the_header():
    """every typedef struct of the header has a mirror in capi.STRUCTS with the same field names, order and C types; the pointer
    records are all pointers, named by their *_FIELDS tuple in order"""
    from zeggs import capi
    structs = _header_structs()
    assert set(structs) == set(capi.STRUCTS) and len(structs) == 21
    records = {"ZeggsSpeechParams": capi.SPEECH_FIELDS, "ZeggsSpeechGrads": capi.SPEECH_FIELDS, "ZeggsStyleParams": capi.STYLE_FIELDS,
               "ZeggsStyleGrads": capi.STYLE_FIELDS, "ZeggsStyleGruParams": capi.STYLE_GRU_FIELDS,
               "ZeggsStyleGruGrads": capi.STYLE_GRU_FIELDS, "ZeggsDecParams": capi.DEC_FIELDS, "ZeggsDecGrads": capi.DEC_FIELDS,
               "ZeggsDecStats": capi.STATS_FIELDS, "ZeggsAnimOut": capi.ANIM_OUT_FIELDS}
    for name, fields in structs.items():
        mirror = capi.STRUCTS[name]._fields_
        assert [f for f, _ in mirror] == [f for f, _, _, _ in fields], name
        if name in records:
            assert tuple(f for f, _ in mirror) == records[name] and all(depth == 1 for _, _, depth, _ in fields), name
        for (f, ctype), (_, base, depth, n) in zip(mirror, fields):
            want = ctypes.c_void_p if depth else _CTYPES[base]
            assert ctype is (want * n if n else want), (name, f)
    assert all(depth == 0 or name in records or name == "ZeggsDecCall" for name, fs in structs.items() for _, _, depth, _ in fs)


def test_typed_handle_host_only_calls():
    """The typed handle (capi.api()) without a GPU: bare Python ints above 2^31 arrive as the `long` / `size_t` they are, a 3.7 GB
    size comes back whole, a refused call raises with the function's name and the library's text, a CPU tensor is refused before
    the library is entered; the raw handle (ops.lib()) is the same dlopen handle with no argument types."""
    from zeggs import audio, capi
    api, L = capi.api(), ops.lib()
    d = audio.MelDims(800, 200, 80, 16000, 60.0, 1e-5, 0.0, 0)
    for n in (2 ** 31 + 12345, 3 * 2 ** 32 + 7):
        assert api.zeggs_mel_frames_ready(d, n) == L.zeggs_mel_frames_ready(ctypes.byref(d), ctypes.c_long(n)) > 2 ** 31 // 400
        k = n // 300
        assert api.zeggs_mel_window_first_sample(d, k) == L.zeggs_mel_window_first_sample(ctypes.byref(d), ctypes.c_long(k)) > 2 ** 31 // 2
        assert api.zeggs_table_text_workspace_bytes(n, 7) == L.zeggs_table_text_workspace_bytes(ctypes.c_long(n), 7) > 2 ** 31
    dd = ops.DecDims(1, 1801, synth.POSE_IN, synth.POSE_OUT, 64, 64, 1024, synth.DT)
    assert api.zeggs_decoder_workspace_bytes(dd, 1) == _WORKSPACE_BYTES[(1, 1801, 64, 1024, 0)][1] == 3748302080
    with pytest.raises(RuntimeError, match=r"^zeggs_set_option: .*no_such_option"):
        api.zeggs_set_option(b"no_such_option", 1)
    assert L.zeggs_set_option(b"no_such_option", 1) != 0
    with pytest.raises(RuntimeError, match="zeggs_fill: .*not on a GPU"):
        api.zeggs_fill(torch.zeros(4), 4, 0.0, None)
    f32 = capi.KINDS["f32*"]
    with pytest.raises(RuntimeError, match="not on a GPU"):          # the GPU refusal comes before the dtype check
        f32.from_param(torch.zeros(4, dtype=torch.float64))
    assert f32.from_param(None) is None
    f32.from_param(ctypes.c_void_p(64)), f32.from_param(64)         # an address passes as it is
    with pytest.raises(TypeError):
        f32.from_param(1.5)
    assert L.zeggs_fill.argtypes is None and api.zeggs_fill.argtypes is not None
    assert L._handle == api._handle
    assert L.zeggs_decoder_workspace_bytes.restype is ctypes.c_size_t and L.zeggs_last_error.restype is ctypes.c_char_p
