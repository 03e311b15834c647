"""Live serving: many audio streams per GPU, constant cost per tick, bounded state.

The serving form of zeggs.stream.GestureStream (same computation: mel + energy -> speech encoder -> autoregressive decoder, any
chunking of the audio gives the frames of the offline path), for `rows` independent streams on one device:

  * push(sid, chunk) uploads ONLY the new samples into the row's device window (fixed capacity; the samples no later frame loads,
    zeggs_mel_window_first_sample, are dropped) and computes the mel rows that became ready (zeggs_mel_features_window);
  * push_many({sid: chunk}) is push() for all streams of a tick at once: the same bookkeeping and feature bits, but one upload, one
    or two zeggs_copy_segments launches and the two launches of zeggs_mel_features_batch whatever the number of rows;
  * step() advances every row that has `tick` decodable frames by exactly `tick` frames: ONE zeggs_speech_encoder_live launch
    (layer-0 activations live in a per-row ring, so nothing is re-encoded) and ONE decoder call for all rows --
    zeggs_decoder_fwd_batch at B = rows, T = tick + 1 (index 0 = the last frame already produced), the weight-stationary sweep where
    it takes the dimensions; a single-row server uses zeggs_decoder_fwd_state_ex as GestureStream does.  Rows that are idle or
    short of `tick` frames ride along on finite filler and their state is not committed;
  * set_style(sid, style, fade) changes the style while speech goes on (the decoder takes a style row per frame);
  * close(sid) flushes the row's remaining frames with the true right-edge rules (B = 1 entry point) and frees the row;
  * LiveServer(loudness="running") normalises every row's loudness as its audio arrives (the streaming counterpart of
    audio_conf.normalize_loudness): a running BS.1770 gated estimate per row on the device, the gain applied as the samples enter
    the window (zeggs_live_loudness_push: one more launch per push / push_many); loudness(sid) reads it, hold(sid) freezes the gain;
  * open(..., rate=48000, pcm="s16") takes a stream at a rate and sample format of its own: its raw samples are uploaded and a
    band-limited converter on the device (zeggs_resample_push: one more launch in a call where some row converts; per-row
    history carried from call to call) writes the server-rate samples in front of the loudness stage and the window, bitwise
    independent of the cuts, of push() against push_many() and of the other rows;
  * LiveServer(frames=dict(parents=...)) adds an output head: step() and close() also return, under "frames", what a renderer or
    a BVH recorder takes of the new frames -- the placed root, local and world-space joint transforms, BVH motion rows (and their
    text) -- converted for all rows by ONE launch (zeggs_live_frames) and brought down by ONE copy into pinned memory per step;
    open(..., start_position=, start_rotation=) says where a character stands, bvh_header(sid, n) gives the head of its file;
  * LiveServer(frames=..., retime=True) hands those frames out at each stream's own frame rate: open(..., frame_rate=30) (24, 25,
    50, 72, 90, 120, 30000/1001, ...) and "frames" holds the stream's new frames at ITS rate, possibly none in a step -- frames
    that fall on a model frame are the plain head's, frames between two are interpolated ahead of FK (positions on the line,
    rotations on the shortest arc) and go through the head's own Euler conversion, FK, sign rule and formatter; going down in
    rate is point sampling.  Still ONE launch (zeggs_live_frames_retimed, in place of zeggs_live_frames) and one download a step;
  * LiveServer(frames=..., retime=dict(filter=True)) band-limits that re-timing: a stream at another rate than the server's (or
    one opened with filtered=True) gets every frame as a windowed-sinc combination of the 2 H + 1 model frames around it, ahead
    of FK -- nothing above half the output rate folds down, no corner at every model frame going up -- H model frames later
    (frame_delay(sid)); the frames still owed at the end come with close().  Still ONE launch (zeggs_live_frames_refiltered),
    filtered and unfiltered rows together;
  * snapshot(sid) / snapshot_many() take everything that determines a stream's future outputs off the device as one numpy.uint8
    blob -- window, pending features, ring, decoder state, the row's spans of the loudness, converter and head state blocks
    (include/zeggs_hip_snapshot.h), the host counters -- and restore(blob) puts it into a free row of any server with the same
    configuration: a drain for a restart, a move to another GPU, a fork.  ONE upload, ONE launch (zeggs_live_pack) and ONE
    download whatever the number of rows; restore() is one upload and one launch (zeggs_live_unpack) after every field was
    checked on the host; snapshot_info(blob) reads a blob's header without a device;
  * LiveServer(gaze=True) lets the point a character looks at move while speech goes on: set_gaze(sid, target, fade, space, path)
    / set_gaze_many({sid: ...}) put a schedule of 64 bytes per row on the device (include/zeggs_hip_gaze.h) -- from where the
    gaze stands to the target over `fade` frames, on a line or on an arc about a pivot, a root-space target resolved on the
    device with the row's root state at the call -- and ONE launch per decoder call (zeggs_live_condition) writes the gaze rows
    AND the style rows of the step's frames, in place of the style fade's weight upload and torch.lerp; gaze(sid) reads it;
  * LiveServer(styles=True | dict(net=style_net, capacity=64, terms=8)) makes styles a resource of the server: add_style(name,
    source) fills a slot of a style bank on the device (include/zeggs_hip_styles.h) -- from an example clip through the style
    encoder, the encoder's row never leaving the device, or from a finished vector -- and set_style(sid, "name" | {name:
    weight}, fade, temperature) / set_style_many({sid: ...}) / open(first_pose, "name") mix bank entries into a row's style by
    ONE launch whatever the number of rows (zeggs_live_style_mix); style(sid) reads a row's pair back.

Everything runs on the caller's current stream; nothing is captured into a graph.  Latency as GestureStream: 15 frames of
look-ahead + one STFT window.  Not here: close() on the batched path, a network front door.
"""
import ctypes as C
import types
import weakref

import numpy as np
import torch

from . import anim, audio, ops

LOOKAHEAD = 15        # (31 - 1) / 2 frames of the speech encoder's second convolution


def ring_depth(kw, tick):
    """frames per layer-0 ring: a step reads frames k0 - 1 - (kw-1)/2 .. k0 + tick - 1 + (kw-1)/2"""
    return int(kw) + int(tick)


def style_weight(f, k, fade):
    """weight of the NEW style at frame f after set_style(..., fade) returned k: 0 before k, then `fade` intermediate frames on a
    straight line, 1 from frame k + fade on (fade = 0: a step at k)"""
    return float(min(max((f - k + 1) / (fade + 1.0), 0.0), 1.0))


GAZE_DEFAULTS = dict(ease="linear")
GAZE_REQUEST = dict(target=None, fade=0, space="world", path="line", pivot=None, ease=None)


def gaze_options(gaze):
    """LiveServer's `gaze` argument -> None (off) or dict(ease: the ease of a set_gaze that names none): True is the defaults, a
    dict overrides them.  ValueError for anything else and for an ease other than "linear" / "smooth"."""
    if gaze is None or gaze is False:
        return None
    if gaze is True:
        gaze = {}
    if not isinstance(gaze, dict) or set(gaze) - set(GAZE_DEFAULTS):
        raise ValueError(f"LiveServer: gaze is None, True or a dict with keys {sorted(GAZE_DEFAULTS)}")
    o = dict(GAZE_DEFAULTS, **gaze)
    if o["ease"] not in ops.GAZE_EASES:
        raise ValueError(f"LiveServer: gaze ease {o['ease']!r} (one of {sorted(ops.GAZE_EASES)})")
    return dict(ease=o["ease"])


def _point(x, what):
    try:
        p = np.asarray(x, np.float64).reshape(-1)
    except (TypeError, ValueError):
        p = np.zeros(0)
    if p.size != 3 or not np.isfinite(p).all() or np.abs(p).max() > np.finfo(np.float32).max:      # (the records carry float32)
        raise ValueError(f"set_gaze: {what} is three finite numbers, not {x!r}")
    return p


def gaze_request(req, default_ease="linear"):
    """one entry of set_gaze_many -- a target [3] or dict(target=, fade=, space=, path=, pivot=, ease=) -> the checked request,
    dict(target: float64 [3], fade: int, space, path, pivot: float64 [3] or None, ease).  ValueError for a negative fade, a target
    or pivot that is not three finite numbers, an unknown space, path or ease, and an arc in world space without a pivot."""
    if not isinstance(req, dict):
        req = dict(target=req)
    if set(req) - set(GAZE_REQUEST) or "target" not in req:
        raise ValueError(f"set_gaze: a target or a dict with `target` and keys of {sorted(GAZE_REQUEST)}")
    o = dict(GAZE_REQUEST, **req)
    fade = o["fade"]
    if isinstance(fade, bool) or not isinstance(fade, (int, np.integer)) or fade < 0:
        raise ValueError(f"set_gaze: fade {fade!r} (an integer >= 0)")
    ease = default_ease if o["ease"] is None else o["ease"]
    for name, value, table in (("space", o["space"], ops.GAZE_SPACES), ("path", o["path"], ops.GAZE_PATHS), ("ease", ease, ops.GAZE_EASES)):
        if not isinstance(value, str) or value not in table:
            raise ValueError(f"set_gaze: {name} {value!r} (one of {sorted(table)})")
    target = _point(o["target"], "the target")
    pivot = None if o["pivot"] is None else _point(o["pivot"], "the pivot")
    if o["path"] == "arc" and o["space"] == "world" and pivot is None:
        raise ValueError("set_gaze: path='arc' in space='world' needs a pivot (space='root' turns about the root by default)")
    return dict(target=target, fade=int(fade), space=o["space"], path=o["path"], pivot=pivot, ease=ease)


STYLES_DEFAULTS = dict(net=None, capacity=64, terms=8)
_F32_MAX = float(np.finfo(np.float32).max)          # (the records carry float32)
STYLE_REQUEST = dict(style=None, fade=0, temperature=None, seed=None)


def styles_options(styles):
    """LiveServer's `styles` argument -> None (off) or dict(net: the style encoder or None, capacity: slots of the bank, terms:
    the most bank entries one mix may name): True is the defaults, a dict overrides them.  ValueError for anything else, a
    capacity outside 1 .. 4096 and terms outside 1 .. 8."""
    if styles is None or styles is False:
        return None
    if styles is True:
        styles = {}
    if not isinstance(styles, dict) or set(styles) - set(STYLES_DEFAULTS):
        raise ValueError(f"LiveServer: styles is None, True or a dict with keys {sorted(STYLES_DEFAULTS)}")
    o = dict(STYLES_DEFAULTS, **styles)
    for key, top in (("capacity", ops.STYLE_MAX_SLOTS), ("terms", ops.STYLE_MAX_TERMS)):
        v = o[key]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= top:
            raise ValueError(f"LiveServer: styles {key} {v!r} (an integer in 1..{top})")
    return dict(net=o["net"], capacity=int(o["capacity"]), terms=int(o["terms"]))


def _is_number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)


def style_terms(style, names, max_terms=ops.STYLE_MAX_TERMS):
    """a named style -- "name", {name: weight} or [(name, weight), ...] -> [(slot, weight)] in the order given, with `names` the
    bank's {name: slot}.  A name alone has weight 1; the weights are taken as they are (not normalised: the offline "add" blend
    is a plain product) and a name may come twice in a list.  ValueError for an unknown name (naming it), no term or more
    than `max_terms`, and a weight that is not a finite number; TypeError for anything that is not one of the three forms."""
    if isinstance(style, str):
        pairs = [(style, 1.0)]
    elif isinstance(style, dict):
        pairs = list(style.items())
    elif isinstance(style, (list, tuple)):
        pairs = list(style)
        if not all(isinstance(p, (list, tuple)) and len(p) == 2 for p in pairs):
            raise TypeError(f"set_style: a list of (name, weight) pairs, not {style!r}")
    else:
        raise TypeError(f"set_style: a style is a tensor, a name, a {{name: weight}} dict or a list of (name, weight) pairs, not {type(style).__name__}")
    if not 1 <= len(pairs) <= max_terms:
        raise ValueError(f"set_style: {len(pairs)} terms (1..{max_terms}: LiveServer(styles=dict(terms=...)), at most {ops.STYLE_MAX_TERMS})")
    out = []
    for name, w in pairs:
        if not isinstance(name, str) or name not in names:
            raise ValueError(f"set_style: no style {name!r} in the bank (add_style(); it holds {sorted(names)})")
        if not _is_number(w) or not np.isfinite(w) or abs(float(w)) > _F32_MAX:
            raise ValueError(f"set_style: the weight of {name!r} is a finite number, not {w!r}")
        out.append((int(names[name]), float(w)))
    return out


def style_request(req, names, max_terms=ops.STYLE_MAX_TERMS):
    """one entry of set_style_many -- a named style (style_terms) or dict(style=, fade=, temperature=, seed=) -> the checked
    request, dict(terms: [(slot, weight)], fade: int, temperature: float (0.0: the means alone), seed: int or None).  A dict
    is the long form when it has the key "style" and that value is not a number ({"style": 0.5} mixes a style of that name).
    ValueError for a negative fade, a temperature that is not None or a finite number >= 0, and a seed without a temperature."""
    if not (isinstance(req, dict) and "style" in req and not _is_number(req["style"])):
        req = dict(style=req)
    if set(req) - set(STYLE_REQUEST):
        raise ValueError(f"set_style: a style or a dict with `style` and keys of {sorted(STYLE_REQUEST)}")
    o = dict(STYLE_REQUEST, **req)
    if isinstance(o["style"], torch.Tensor):
        raise TypeError("set_style_many: named styles only; a tensor goes through set_style(sid, tensor, fade)")
    terms = style_terms(o["style"], names, max_terms)
    fade, t, seed = o["fade"], o["temperature"], o["seed"]
    if isinstance(fade, bool) or not isinstance(fade, (int, np.integer)) or fade < 0:
        raise ValueError(f"set_style: fade {fade!r} (an integer >= 0)")
    if t is not None and (not _is_number(t) or not np.isfinite(t) or t < 0 or float(t) > _F32_MAX):
        raise ValueError(f"set_style: temperature {t!r} (None or a finite number >= 0)")
    t = 0.0 if t is None else float(t)
    if seed is not None and (t == 0.0 or isinstance(seed, bool) or not isinstance(seed, (int, np.integer))):
        raise ValueError(f"set_style: seed {seed!r} (an integer, with a temperature > 0: the means alone draw nothing)")
    return dict(terms=terms, fade=int(fade), temperature=t, seed=None if seed is None else int(seed))


def _quat_rotate(q, v):
    """csrc/quat_math.h's quat_mul_vec in float64: t = 2 (q_v x v); v + w t + q_v x t"""
    t = 2.0 * np.cross(q[1:], v)
    return v + q[0] * t + np.cross(q[1:], t)


def gaze_to_model(target, ref_pos, ref_rot, start_position, start_rotation):
    """a point of the client's placed space -- the space open(start_position=, start_rotation=) puts a stream's frames in -- as a
    point of the model's world, what set_gaze(space="world") takes: the inverse of open()'s re-basing
    x' = start_rot ref_rot^-1 (x - ref_pos) + start_pos, i.e. x = ref_rot start_rot^-1 (x' - start_pos) + ref_pos, with ref_pos /
    ref_rot the root of the stream's frame 0 (quaternions w first, taken as they are: unit length is the caller's).  float64, no
    state, no device."""
    x, rp, sp = (np.asarray(a, np.float64).reshape(3) for a in (target, ref_pos, start_position))
    rr, sr = (np.asarray(a, np.float64).reshape(4) for a in (ref_rot, start_rotation))
    inv = lambda q: q * np.array([1.0, -1.0, -1.0, -1.0])  # noqa: E731
    return _quat_rotate(rr, _quat_rotate(inv(sr), x - sp)) + rp


class _GazeRows(torch.Tensor):
    """LiveServer.gaze: the rows' gaze tensor [R, T, 3] that step() hands the decoder -- and, called with a stream id, the
    monitoring call gaze(sid) (LiveServer._gaze_read).  The tensor has carried the name since live serving began (tests and
    tools index it); the call takes the name the other stages' calls have (loudness(sid)).  Tensor operations see a plain
    tensor: no __torch_function__ dispatch, the same storage, nothing more enqueued."""
    __torch_function__ = torch._C._disabled_torch_function_impl

    def __call__(self, sid):
        return self._server()._gaze_read(sid)


class _Ring:
    """The staging of every stage of live serving, stated once: RING pinned host blocks of `nbytes` that take turns, one event a
    block, recorded behind the copy that last used it and waited for before the block is used again, and ONE device block
    (calls on a stream are ordered).  A subclass states what its block holds and which way its copies go."""
    RING, turn = 2, 0

    def _blocks(self, nbytes, dev, make=torch.empty):
        self.nbytes = int(nbytes)
        self.host = [make(self.nbytes, dtype=torch.uint8).pin_memory() for _ in range(self.RING)]
        self.dev = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.events = [None] * self.RING

    def _next(self):
        """the next block's index, once the copy that last used it is done"""
        self.turn = t = (self.turn + 1) % self.RING
        if self.events[t] is not None:
            self.events[t].synchronize()
        return t

    def _copy(self, lo, hi, up=True):
        """bytes lo .. hi of the turn's block to the same place of the device block (up) or back -> the event behind the copy"""
        host, dev = self.host[self.turn][lo:hi], self.dev[lo:hi]
        if up:
            dev.copy_(host, non_blocking=True)
        else:
            host.copy_(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[self.turn] = ev
        return ev

    def idle(self):
        for ev in self.events:
            if ev is not None:
                ev.synchronize()


class _RecStaging(_Ring):
    """The records of a gaze launch with more than one record, uploaded as ONE block."""
    RING = 4

    def __init__(self, record, rows, dev):
        self._blocks(rows * C.sizeof(record), dev, torch.zeros)
        self.recs = [(record * rows).from_buffer(h.numpy()) for h in self.host]
        self.size = C.sizeof(record)

    def take(self):
        return self.recs[self._next()]

    def upload(self, n):
        self._copy(0, n * self.size)
        return self.dev.data_ptr()


def plan_step(rows, tick, depth, lookahead=LOOKAHEAD):
    """The pure part of step(): which rows advance and what the encoder launch is told about them.  rows[r]: None (free row) or a
    dict with "n_feat" (feature rows computed: frames [0, n_feat)), "n_ring" (frames whose layer-0 activation is in the ring) and
    "kd" (first frame not yet decoded, >= 1).  A row is eligible when frames kd .. kd + tick - 1 all have their look-ahead:
    kd + tick + lookahead <= n_feat.  -> per row None or dict(k0, k1: frames decoded [k0, k1); enc_k0, n_out: the encoder's output
    range starts one frame earlier (index 0 of the decoder chunk); n_new: feature rows that enter the ring, frames n_ring ..;
    slots: their ring slots)."""
    plan = []
    for row in rows:
        if row is None or row["kd"] + tick + lookahead > row["n_feat"]:
            plan.append(None)
            continue
        kd, n_ring = row["kd"], row["n_ring"]
        n_new = kd + tick + lookahead - n_ring
        assert 0 <= n_new <= depth
        plan.append(dict(k0=kd, k1=kd + tick, enc_k0=kd - 1, n_out=tick + 1, n_new=n_new,
                         slots=[(n_ring + i) % depth for i in range(n_new)]))
    return plan


def plan_push(rows, caps, lens, FC, width, first_sample, frames_ready):
    """The pure part of push_many(): push()'s bookkeeping for several rows, in order, as ONE list of copies.  rows[i]: dict with
    n, base (samples received / absolute index of the window's first sample), n_feat, fbase, n_ring (feature rows computed / frame of
    the pending block's first row / frames in the ring); caps[i]: capacity of the row's window; lens[i]: samples of its chunk (0: the
    row takes no part, as push() returns at once); FC: rows of a pending-feature block, `width` floats each; first_sample(k):
    zeggs_mel_window_first_sample; frames_ready(n): feature rows computable from n samples while the signal goes on.
    -> dict(rows=[dict(n, base, n_feat, fbase: the new counters; cap: capacity the row's window needs; swap: the window was
    compacted INTO the row's alternate buffer, which is the current one from now on; k0, k1: feature rows to compute, into row
    k0 - fbase of the block)], segs, segs_back: the copies of the first and the second launch, FC: the (grown) block size,
    n_stage: samples in the staging area).  A copy is (src, src_off, dst, dst_off, count) in floats; src / dst are ("win", i) the
    row's current window BEFORE the call, ("alt", i) its alternate, ("stage", None) all chunks one after another, ("feats", i)
    the row's pending block, ("scratch", i) the row's block of the scratch area.  No copy is in place: a compaction goes to the
    other buffer, kept feature rows go to scratch and come back in the second launch (the block itself cannot move: the encoder
    reads it at a fixed stride)."""
    out, segs, back, soff = [], [], [], 0
    for i, (st, cap, m) in enumerate(zip(rows, caps, lens)):
        n, base, n_feat, fbase, n_ring = (int(st[k]) for k in ("n", "base", "n_feat", "fbase", "n_ring"))
        cap, m, swap, k0, k1 = int(cap), int(m), False, n_feat, n_feat
        if m > 0:
            if n - base + m > cap:
                # drop what no frame >= n_feat loads any more; grow only if this single chunk does not fit beside what must stay
                nb = max(base, min(first_sample(n_feat), n))
                keep = n - nb
                cap = max(cap, keep + m)
                if keep:
                    segs.append((("win", i), nb - base, ("alt", i), 0, keep))
                swap, base = True, nb
            segs.append((("stage", None), soff, ("alt" if swap else "win", i), n - base, m))
            soff += m
            n += m
            k1 = max(int(frames_ready(n)), k0)
            if k1 > k0:
                pend = k0 - n_ring                           # rows still waiting for the ring: frames n_ring .. k0 - 1
                if k0 - fbase + (k1 - k0) > FC:              # compact (and grow if this one chunk needs more than the block holds)
                    FC = max(FC, pend + (k1 - k0))
                    if pend:
                        segs.append((("feats", i), (n_ring - fbase) * width, ("scratch", i), 0, pend * width))
                        back.append((("scratch", i), 0, ("feats", i), 0, pend * width))
                    fbase = n_ring
                n_feat = k1
        out.append(dict(n=n, base=base, n_feat=n_feat, fbase=fbase, cap=cap, swap=swap, k0=k0, k1=k1))
    return dict(rows=out, segs=segs, segs_back=back, FC=FC, n_stage=soff)


class _Staging(_Ring):
    """What one push_many() uploads, as ONE block: [copy records | copy records of the second launch | mel records | loudness
    records (`loud_rows` of them: none on a server without running loudness) | samples], and in a call with converting rows,
    behind the samples the call stages (tail()): [converter records | the converting rows' raw input, 2 bytes a sample for s16].
    Two pinned host blocks take turns (_Ring), so a block is never rewritten while a copy from it may be in flight."""

    def __init__(self, rows, n_samples, dev, loud_rows=0, tail_bytes=0):
        a64 = lambda x: (x + 63) // 64 * 64  # noqa: E731
        self.rows, self.n_samples, self.loud_rows = rows, int(n_samples), int(loud_rows)
        self.o_back = a64(3 * rows * C.sizeof(ops.Seg))
        self.o_mel = self.o_back + a64(rows * C.sizeof(ops.Seg))
        self.o_loud = self.o_mel + a64(rows * C.sizeof(ops.MelRow))
        self.o_smp = self.o_loud + a64(self.loud_rows * C.sizeof(ops.LoudRow))
        self.tail_bytes = int(tail_bytes)               # room behind the samples for converter records and raw input
        self._blocks(self.o_smp + 4 * self.n_samples + self.tail_bytes, dev)
        self.view = []
        for h in self.host:
            b = h.numpy()
            self.view.append(dict(segs=(ops.Seg * (3 * rows)).from_buffer(b, 0), back=(ops.Seg * rows).from_buffer(b, self.o_back),
                                  mel=(ops.MelRow * rows).from_buffer(b, self.o_mel),
                                  smp=b[self.o_smp:self.o_smp + 4 * self.n_samples].view(np.float32), block=b,
                                  loud=(ops.LoudRow * self.loud_rows).from_buffer(b, self.o_loud)))

    def take(self):
        """the next host block, once the copy that last read it is done"""
        return self.view[self._next()]

    def tail(self, n_samples, n_records, raw_bytes):
        """where a call that stages n_samples floats puts its converter records and raw input, and where the block then ends"""
        a64 = lambda x: (x + 63) // 64 * 64  # noqa: E731
        o_rs = a64(self.o_smp + 4 * int(n_samples))
        o_raw = o_rs + a64(int(n_records) * C.sizeof(ops.ResampleRow))
        return o_rs, o_raw, o_raw + int(raw_bytes)

    def upload(self, n_samples, end=None):
        self._copy(0, self.o_smp + 4 * int(n_samples) if end is None else int(end))


LOUDNESS_DEFAULTS = dict(target=-20.0, horizon=60.0, warmup=1, gain_db=(-30.0, 30.0))


def loudness_options(loudness):
    """LiveServer's `loudness` argument -> None (off) or dict(target, horizon, warmup, gain_db, ring_blocks): "running" is the
    defaults, a dict overrides them.  `horizon`: seconds the estimate looks back over, a positive multiple of 0.1 s (one gating
    block per 0.1 s: ring_blocks = round(horizon * 10)); `warmup` >= 1 gated blocks before the first estimate; `gain_db` (lo, hi)
    bounds of the gain in dB.  Anything else raises ValueError."""
    if loudness is None:
        return None
    if loudness == "running":
        loudness = {}
    if not isinstance(loudness, dict) or set(loudness) - set(LOUDNESS_DEFAULTS):
        raise ValueError(f"LiveServer: loudness is None, 'running' or a dict with keys {sorted(LOUDNESS_DEFAULTS)}")
    o = dict(LOUDNESS_DEFAULTS, **loudness)
    try:
        target, horizon, warmup = float(o["target"]), float(o["horizon"]), int(o["warmup"])
        lo, hi = (float(x) for x in o["gain_db"])
    except (TypeError, ValueError):
        raise ValueError(f"LiveServer: loudness options {loudness!r}") from None
    blocks = round(horizon * 10) if np.isfinite(horizon) else 0
    if not (blocks >= 1 and abs(horizon * 10 - blocks) < 1e-6):
        raise ValueError(f"LiveServer: loudness horizon {horizon} s is not a positive multiple of 0.1 s")
    if warmup < 1 or warmup != o["warmup"]:
        raise ValueError(f"LiveServer: loudness warmup {o['warmup']} (an integer >= 1)")
    if not lo <= hi or not np.isfinite([lo, hi, target]).all():
        raise ValueError(f"LiveServer: loudness gain_db {o['gain_db']} (lo <= hi) / target {target}")
    return dict(target=target, horizon=horizon, warmup=warmup, gain_db=(lo, hi), ring_blocks=int(blocks))


def resample_row(rate, pcm, fs):
    """open()'s `rate` / `pcm` on a server at `fs` Hz -> None (today's row: float32 at the server's rate) or (input rate, format
    code).  ValueError for an unknown format and for a rate the converter does not take (naming both rates)."""
    if pcm not in ops.RS_FORMATS:
        raise ValueError(f"LiveServer.open: pcm {pcm!r} (one of {sorted(ops.RS_FORMATS)})")
    if rate is None or rate == fs:
        return None if pcm == "f32" else (int(fs), ops.RS_FORMATS[pcm])
    if isinstance(rate, bool) or not isinstance(rate, (int, float, np.integer, np.floating)):
        raise ValueError(f"LiveServer.open: rate {rate!r} Hz (the server runs at {fs} Hz)")
    audio.resample_ratio(rate, fs)
    return int(rate), ops.RS_FORMATS[pcm]


FRAMES_DEFAULTS = dict(parents=None, names=None, what=("local", "world", "bvh"), order="zyx", text=False)


def frames_options(frames):
    """LiveServer's `frames` argument -> None (off) or dict(parents, names, what: the names in the order local, world, bvh, mask:
    their bits, order, text, seq: the joint order of the BVH rows).  ValueError for anything but a dict with keys of
    FRAMES_DEFAULTS, for a dict without `parents` or with a skeleton the kernel refuses, an unknown `what`, a channel order
    quat.to_euler does not have, `names` of another length, and `text` without "bvh"."""
    if frames is None:
        return None
    if not isinstance(frames, dict) or set(frames) - set(FRAMES_DEFAULTS):
        raise ValueError(f"LiveServer: frames is None or a dict with keys {sorted(FRAMES_DEFAULTS)}")
    o = dict(FRAMES_DEFAULTS, **frames)
    if o["parents"] is None:
        raise ValueError("LiveServer: frames needs the skeleton: frames=dict(parents=...)")
    parents = [int(p) for p in o["parents"]]
    seq = ops.frames_seq(parents)
    mask = ops.frames_what(o["what"])
    if o["order"] not in ("zyx", "xzy"):
        raise ValueError(f"LiveServer: frames order {o['order']!r} ('zyx' or 'xzy': what quat.to_euler converts to)")
    names = None if o["names"] is None else [str(n) for n in o["names"]]
    if names is not None and len(names) != len(parents):
        raise ValueError(f"LiveServer: frames has {len(names)} names for {len(parents)} joints")
    if o["text"] and not mask & ops.FRAMES_WHAT["bvh"]:
        raise ValueError("LiveServer: frames text=True formats the BVH rows: what must hold 'bvh'")
    return dict(parents=parents, names=names, what=tuple(n for n in ("local", "world", "bvh") if mask & ops.FRAMES_WHAT[n]), mask=mask,
                order=o["order"], text=bool(o["text"]), seq=seq)


RETIME_DEFAULTS = dict(max_rate=None, min_rate=None, filter=None)
REFILTER_DEFAULT_HALF = 16        # the default min_rate is the lowest rate that keeps H_max at or below this


def retime_options(retime, frames_conf, fps):
    """LiveServer's `retime` argument -> None (off) or dict(max_rate: the highest frame rate a stream may ask for, a Fraction,
    ratio: max_rate / fps as (L, M)): True is the defaults, a dict overrides them; max_rate None is the server's own rate `fps`
    (re-timing downward only: the staging blocks are the plain head's).  ValueError for anything else, for `retime` without
    `frames`, and for a max_rate the kernel does not take (naming both rates).
    With filter=True | dict(zero_crossings, rolloff, beta) (ops.refilter_options) the dict also holds `filter` (the checked
    options), `min_rate` (a Fraction: the lowest rate a FILTERED stream may ask for; default the lowest that keeps H_max <= 16,
    never below fps / 4) and `half_max` = H_max = ceil(zero_crossings fps / min_rate), what the rows' rings are sized for.
    ValueError naming both rates for a min_rate below fps / 4 (the filter takes M <= 4 L) or above fps, and for a min_rate
    without `filter`."""
    if retime is None or retime is False:
        return None
    if retime is True:
        retime = {}
    if not isinstance(retime, dict) or set(retime) - set(RETIME_DEFAULTS):
        raise ValueError(f"LiveServer: retime is None, True or a dict with keys {sorted(RETIME_DEFAULTS)}")
    if frames_conf is None:
        raise ValueError("LiveServer: retime re-times the frames of the output head: it needs frames=dict(parents=...)")
    o = dict(RETIME_DEFAULTS, **retime)
    rate = fps if o["max_rate"] is None else o["max_rate"]
    try:
        L, M = ops.retime_ratio(rate, fps)
    except ValueError as e:
        raise ValueError(f"LiveServer: retime max_rate: {e}") from None
    if L < M:
        raise ValueError(f"LiveServer: retime max_rate {rate!r} is below the server's own {fps!r} frames per second")
    from fractions import Fraction
    conf = dict(max_rate=Fraction(L, M) * Fraction(str(float(fps))), ratio=(L, M))
    if o["filter"] is None or o["filter"] is False:
        if o["min_rate"] is not None:
            raise ValueError(f"LiveServer: retime min_rate {o['min_rate']!r} sizes the filter's history: it needs filter=True or a dict")
        return conf
    try:
        fopt = ops.refilter_options(o["filter"])
    except ValueError as e:
        raise ValueError(f"LiveServer: retime filter: {e}") from None
    Z, fr = fopt["zero_crossings"], Fraction(str(float(fps)))
    if o["min_rate"] is None:
        lo = max(fr * Z / REFILTER_DEFAULT_HALF, fr / ops.REFILTER_MAX_DOWN)
    else:
        try:
            l, m = ops.retime_ratio(o["min_rate"], fps)
        except ValueError as e:
            raise ValueError(f"LiveServer: retime min_rate: {e}") from None
        if m > ops.REFILTER_MAX_DOWN * l:
            raise ValueError(f"LiveServer: retime min_rate {o['min_rate']!r} on a server at {fps!r} frames per second is below a quarter of "
                             f"it, {float(fr / ops.REFILTER_MAX_DOWN)!r}: the filter takes M <= {ops.REFILTER_MAX_DOWN} L")
        if l > m:
            raise ValueError(f"LiveServer: retime min_rate {o['min_rate']!r} is above the server's own {fps!r} frames per second")
        lo = fr * l / m
    half_max = -(-(Z * fr) // lo)
    return dict(conf, filter=fopt, min_rate=lo, half_max=int(half_max))


def plant_options(plant, frames_conf):
    """LiveServer's `plant` argument -> None (off) or ops.plant_options' dict against the skeleton of `frames`: True is the
    defaults (NOT tuned on captured motion), a dict overrides them.  ValueError for `plant` without `frames` and for whatever
    ops.plant_options refuses, the chain named."""
    if plant is None or plant is False:
        return None
    if frames_conf is None:
        raise ValueError("LiveServer: plant corrects the rows the output head reads: it needs frames=dict(parents=...)")
    try:
        return ops.plant_options(plant, frames_conf["parents"], frames_conf["names"])
    except ValueError as e:
        raise ValueError(f"LiveServer: {e}") from None


def frames_placement(start_position, start_rotation):
    """open()'s placement -> None (neither given: the root is handed out as it is) or (position [3], rotation [4], float64);
    ValueError when only one of the two is given or a shape is wrong"""
    if start_position is None and start_rotation is None:
        return None
    if start_position is None or start_rotation is None:
        raise ValueError("LiveServer.open: start_position and start_rotation come together (both or neither)")
    pos, rot = np.asarray(start_position, np.float64).reshape(-1), np.asarray(start_rotation, np.float64).reshape(-1)
    if pos.size != 3 or rot.size != 4 or not (np.isfinite(pos).all() and np.isfinite(rot).all()):
        raise ValueError("LiveServer.open: start_position is [3], start_rotation a quaternion [4] (w first)")
    return pos, rot


def frames_layout(N, J, mask):
    """the packed block of N frames, the one place that states it: [BVH rows float64 [N][3 + 3J] | LOCAL float32 [N][7 + 7J] |
    WORLD float32 [N][7J]], an area whose bit is off in `mask` missing -> ((bvh, local, world), bytes of the block): an area is
    (its offset, its bytes a frame), or None where it is missing"""
    areas, total = [], 0
    for k, per in (("bvh", (3 + 3 * J) * 8), ("local", (7 + 7 * J) * 4), ("world", 7 * J * 4)):
        areas.append((total, per) if mask & ops.FRAMES_WHAT[k] else None)
        total += int(N) * per if areas[-1] else 0
    return tuple(areas), total


def frames_unpack(buf, counts, J, mask, copy=True):
    """the packed block of one zeggs_live_frames call on the host (uint8, frames_layout) -> per record the dict of arrays;
    N = sum(counts), record i owns rows sum(counts[:i]) .. of each area."""
    N = int(sum(counts))
    rows = lambda area, t: buf[area[0]:area[0] + N * area[1]].view(t).reshape(N, area[1] // np.dtype(t).itemsize) if area else None  # noqa: E731
    bvh, loc, wld = (rows(area, t) for area, t in zip(frames_layout(N, J, mask)[0], (np.float64, np.float32, np.float32)))
    out, a = [], 0
    own = (lambda x: np.array(x)) if copy else (lambda x: x)
    for c in counts:
        o = {}
        if loc is not None:
            x = loc[a:a + c]
            o.update(root_pos=own(x[:, 0:3]), root_rot=own(x[:, 3:7]), lrot=own(x[:, 7:7 + 4 * J]).reshape(c, J, 4),
                     lpos=own(x[:, 7 + 4 * J:]).reshape(c, J, 3))
        if wld is not None:
            x = wld[a:a + c]
            o.update(gpos=own(x[:, :3 * J]).reshape(c, J, 3), grot=own(x[:, 3 * J:]).reshape(c, J, 4))
        if bvh is not None:
            o["bvh"] = own(bvh[a:a + c])
        out.append(o)
        a += c
    return out


def frames_cat(parts):
    """the "frames" of consecutive steps of a stream as one: arrays concatenated along the frames, "text" joined, "frame0" (a
    re-timing server: the index of a part's first frame) the first part's"""
    return {k: b"".join(p[k] for p in parts) if k == "text" else parts[0][k] if k == "frame0" else np.concatenate([p[k] for p in parts])
            for k in parts[0]}


def frames_block_bytes(N, J, mask):
    """bytes of the packed block of N frames (frames_layout)"""
    return frames_layout(N, J, mask)[1]


class _FrameStaging(_Ring):
    """What the output head of a step needs beside the rows' state, allocated once: the device block the one launch writes
    (frames_unpack's layout, sized for every row at max_frames), a small ring of pinned host blocks the one download lands in
    (_Ring), and the records of the launch in pinned host memory -- page-locked
    memory is device accessible, so the kernel reads its records where the host wrote them and no upload is enqueued.  The
    records are rewritten only after the step that used them has waited for its download, which is ordered behind the launch."""
    RING = 3

    def __init__(self, rows, max_frames, J, mask, dev, record=None, tail_bytes=0, tail_record=None):
        record = record or ops.FramesRow              # (the re-timing head: ops.RetimeRow, max_frames OUTPUT frames a row)
        self.J, self.mask = J, mask
        # tail_bytes: room behind the three areas (a planting server: the contact flags of a step's model frames), and with
        # tail_record the records of the stage in front of the head, staged as the head's are
        self._blocks(frames_block_bytes(rows * max_frames, J, mask) + int(tail_bytes), dev)
        if tail_record is not None:
            self.tail_mem = torch.zeros(rows * C.sizeof(tail_record), dtype=torch.uint8).pin_memory()
            self.tail_recs = (tail_record * rows).from_buffer(self.tail_mem.numpy())
        self.rec_mem = torch.zeros(rows * C.sizeof(record), dtype=torch.uint8).pin_memory()
        self.recs = (record * rows).from_buffer(self.rec_mem.numpy())

    def download(self, nbytes):
        """one device-to-host copy of the block's first nbytes into the next pinned block -> that block's bytes, once they are
        there (a view: frames_unpack copies what it hands out)"""
        t = self._next()
        self._copy(0, nbytes, up=False).synchronize()
        return self.host[t].numpy()[:nbytes]


# ---------------------------------------------------------------------------------------------------------------- snapshots
# A blob, little-endian: [magic 8 | format u32 | zeggs_live_snapshot_version() u32 | sid i64 | fingerprint fields u32 |
# sections u32 | total bytes u64 | fingerprint float64[len(SNAP_FINGERPRINT)] | section table (kind u32, 0 u32, offset u64, bytes
# u64)[len(SNAP_SECTIONS)] | sections, each on a 16-byte boundary in the table's order, zero padded].  Every kind is in the table;
# one a stream does not have (no converter, a server without the head) has 0 bytes.
SNAP_MAGIC, SNAP_FORMAT = b"ZEGGSNAP", 1
# what sizes or interprets the state (LiveServer._fingerprint); NOT the weights and the statistics
SNAP_FINGERPRINT = ("tick", "fs", "fps", "mel_n_fft", "mel_hop", "mel_n_mels", "mel_fs", "mel_fps", "mel_min_clip", "mel_pre_emph", "mel_flags",
                    "FC", "ring_depth", "ring_width", "H", "ST", "PO", "speech_width", "KW",
                    "loudness", "loudness_target", "loudness_ring_blocks", "loudness_warmup", "loudness_gain_lo", "loudness_gain_hi",
                    "resample_zero_crossings", "resample_rolloff", "resample_beta",
                    "frames", "frames_joints", "frames_what", "frames_order", "frames_seq",
                    "retime", "retime_max_L", "retime_max_M", "filter", "filter_zero_crossings", "filter_rolloff", "filter_beta",
                    "filter_min_rate_num", "filter_min_rate_den", "filter_half_max")
# a planting server's blobs carry these behind SNAP_FINGERPRINT (the header's field count says which kind a blob is); the blobs of
# a server without `plant` are what they were
SNAP_FINGERPRINT_PLANT = ("plant_chains", "plant_v_on", "plant_v_off", "plant_h_on", "plant_h_off", "plant_ground", "plant_slack",
                          "plant_release", "plant_stretch")
SNAP_SECTIONS = ("row", "offsets", "window", "feats", "ring", "h", "pose", "rpos", "rrot", "gaze", "sty_old", "sty_new", "loudness",
                 "resample", "head")
# the `row` section, int64 each: the six counters, what _Row holds of the style fade, the converter and the output head, and how
# the `offsets` section is to be read (bytes per value, values)
SNAP_ROW = ("n", "base", "n_feat", "fbase", "n_ring", "kd", "sent0", "k_style", "fade", "rs", "rs_fi", "rs_fmt", "rs_n_in",
            "rt", "rt_L", "rt_M", "rt_n_in", "rt_n_out", "rt_half", "offsets_itemsize", "offsets_count")
_SNAP_HEAD = 8 + 4 + 4 + 8 + 4 + 4 + 8
_a16 = lambda x: (int(x) + 15) // 16 * 16  # noqa: E731


def _snap_fields(fingerprint):
    """the fingerprint fields a blob with this fingerprint carries: SNAP_FINGERPRINT, a planting server's also SNAP_FINGERPRINT_PLANT"""
    return SNAP_FINGERPRINT + SNAP_FINGERPRINT_PLANT if SNAP_FINGERPRINT_PLANT[0] in fingerprint else SNAP_FINGERPRINT


def snapshot_layout(sizes, n_fp=None):
    """bytes per section, in SNAP_SECTIONS' order -> (their offsets in the blob, the blob's length): the header, then every section
    on the next 16-byte boundary.  `n_fp`: the fingerprint fields of the header (None: len(SNAP_FINGERPRINT))"""
    assert len(sizes) == len(SNAP_SECTIONS)
    n_fp = len(SNAP_FINGERPRINT) if n_fp is None else int(n_fp)
    at, offs = _a16(_SNAP_HEAD + 8 * n_fp + 24 * len(SNAP_SECTIONS)), []
    for b in sizes:
        offs.append(at)
        at = _a16(at + int(b))
    return offs, at


def snapshot_header(sid, version, fingerprint, sizes):
    """the bytes in front of the first section: `fingerprint` a dict over SNAP_FINGERPRINT (a planting server's: also over
    SNAP_FINGERPRINT_PLANT), `sizes` as snapshot_layout takes them"""
    fields = _snap_fields(fingerprint)
    offs, total = snapshot_layout(sizes, len(fields))
    head = SNAP_MAGIC + np.array([SNAP_FORMAT, int(version)], "<u4").tobytes() + np.array([int(sid)], "<i8").tobytes()
    head += np.array([len(fields), len(SNAP_SECTIONS)], "<u4").tobytes() + np.array([total], "<u8").tobytes()
    head += np.array([float(fingerprint[k]) for k in fields], "<f8").tobytes()
    for kind, (o, b) in enumerate(zip(offs, sizes)):
        head += np.array([kind, 0], "<u4").tobytes() + np.array([o, int(b)], "<u8").tobytes()
    return head + bytes(offs[0] - len(head))


def snapshot_build(sid, version, fingerprint, sections):
    """a blob on the host from its parts: `sections` {name: bytes-like} over SNAP_SECTIONS (a missing one is empty) -> numpy.uint8.
    What snapshot_many() writes around the bytes it brings down; here for tools and tests, no device"""
    raw = lambda x: bytes(x) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x).tobytes()  # noqa: E731
    data = [raw(sections.get(k, b"")) for k in SNAP_SECTIONS]
    offs, total = snapshot_layout([len(d) for d in data], len(_snap_fields(fingerprint)))
    blob = np.zeros(total, np.uint8)
    head = snapshot_header(sid, version, fingerprint, [len(d) for d in data])
    blob[:len(head)] = np.frombuffer(head, np.uint8)
    for o, d in zip(offs, data):
        blob[o:o + len(d)] = np.frombuffer(d, np.uint8)
    return blob


def snapshot_info(blob):
    """the parsed header of a blob, without touching a device -> dict(format, version, sid, nbytes, fingerprint: {field: value},
    sections: {name: (offset, bytes)}, row: {field: value} of the `row` section).  ValueError naming the field or the section for
    anything but a whole blob of this format: a wrong magic or format version, other field or section counts, a length that is
    not the header's, a table that is not the layout of its own sizes (a section that is not on its 16-byte boundary, that
    overlaps the next or ends past the blob), a `row` section of another size or whose counts disagree with the `offsets`,
    `window` or `feats` sections."""
    b = np.frombuffer(bytes(blob) if isinstance(blob, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blob, np.uint8), np.uint8)
    if b.size < _SNAP_HEAD:
        raise ValueError(f"snapshot: {b.size} bytes are shorter than the header ({_SNAP_HEAD}): truncated")
    if b[:8].tobytes() != SNAP_MAGIC:
        raise ValueError(f"snapshot: magic {b[:8].tobytes()!r} is not {SNAP_MAGIC!r}")
    fmt, version = (int(x) for x in b[8:16].view("<u4"))
    if fmt != SNAP_FORMAT:
        raise ValueError(f"snapshot: format version {fmt} (this package reads {SNAP_FORMAT})")
    sid = int(b[16:24].view("<i8")[0])
    n_fp, n_sec = (int(x) for x in b[24:32].view("<u4"))
    total = int(b[32:40].view("<u8")[0])
    if n_fp not in (len(SNAP_FINGERPRINT), len(SNAP_FINGERPRINT) + len(SNAP_FINGERPRINT_PLANT)) or n_sec != len(SNAP_SECTIONS):
        raise ValueError(f"snapshot: {n_fp} fingerprint fields and {n_sec} sections (this package reads {len(SNAP_FINGERPRINT)} and {len(SNAP_SECTIONS)})")
    o_tab = _SNAP_HEAD + 8 * n_fp
    if b.size < o_tab + 24 * n_sec:
        raise ValueError(f"snapshot: {b.size} bytes end inside the header ({o_tab + 24 * n_sec}): truncated")
    fp = dict(zip(SNAP_FINGERPRINT + SNAP_FINGERPRINT_PLANT, (float(x) for x in b[_SNAP_HEAD:o_tab].view("<f8"))))
    sections, sizes = {}, []
    for i, name in enumerate(SNAP_SECTIONS):
        kind = int(b[o_tab + 24 * i:o_tab + 24 * i + 4].view("<u4")[0])
        off, nb = (int(x) for x in b[o_tab + 24 * i + 8:o_tab + 24 * i + 24].view("<u8"))
        if kind != i:
            raise ValueError(f"snapshot: section {i} is of kind {kind}, not {i} ({name})")
        sections[name] = (off, nb)
        sizes.append(nb)
    offs, want = snapshot_layout(sizes, n_fp)
    for name, o in zip(SNAP_SECTIONS, offs):
        if sections[name][0] != o:
            raise ValueError(f"snapshot: section {name!r} at offset {sections[name][0]} with {sections[name][1]} bytes: the table is not the layout "
                             f"of its own sizes (offset {o} expected)")
    for name in SNAP_SECTIONS:
        if sum(sections[name]) > b.size:
            raise ValueError(f"snapshot: section {name!r} ends at byte {sum(sections[name])}, the blob has {b.size}: truncated")
    if total != want or b.size != total:
        raise ValueError(f"snapshot: total length {b.size} bytes, the header says {total} and its sections make {want}")
    if sections["row"][1] != 8 * len(SNAP_ROW):
        raise ValueError(f"snapshot: section 'row' has {sections['row'][1]} bytes, {8 * len(SNAP_ROW)} expected")
    row = dict(zip(SNAP_ROW, (int(x) for x in b[sections["row"][0]:sum(sections["row"])].view("<i8"))))
    for name, nb in (("offsets", row["offsets_itemsize"] * row["offsets_count"]), ("window", 4 * (row["n"] - row["base"]))):
        if sections[name][1] != nb:
            raise ValueError(f"snapshot: section {name!r} has {sections[name][1]} bytes, its row counters ask for {nb}")
    return dict(format=fmt, version=version, sid=sid, nbytes=total, fingerprint=fp, sections=sections, row=row)


def snapshot_check_fingerprint(got, want):
    """restore()'s configuration check: ValueError naming the first field of SNAP_FINGERPRINT in which the blob's fingerprint
    `got` differs from the server's `want`, with both values; a blob of a planting server against a server without `plant`, and
    the other way round, is named as that"""
    if (SNAP_FINGERPRINT_PLANT[0] in got) != (SNAP_FINGERPRINT_PLANT[0] in want):
        raise ValueError("LiveServer.restore: the blob was taken from a server " + ("with plant, this one has none" if SNAP_FINGERPRINT_PLANT[0] in got
                         else "without plant, this one has it (LiveServer(plant=...))"))
    for k in _snap_fields(want):
        if float(got[k]) != float(want[k]):
            raise ValueError(f"LiveServer.restore: the blob was taken from a server with {k} = {got[k]!r}, this one has {k} = {float(want[k])!r}")


class _SnapStaging(_Ring):
    """What snapshot_many() and restore() need beside the rows' state, allocated at the first such call and grown when a call
    needs more (_Ring's blocks, made anew once the copies of the old ones are done).  A call's block is [segment records | 64-byte boundary | blobs, each on a 64-byte boundary]."""
    RING = 2

    def __init__(self, dev):
        self.device, self.nbytes, self.dev, self.host, self.events, self.turn = dev, 0, None, [], [], 0

    def take(self, nbytes):
        """the next pinned block with room for nbytes (uint8 array), once the copy that last used it is done"""
        if nbytes > self.nbytes:
            self.idle()
            self._blocks(max(2 * int(nbytes), 1 << 16), self.device)
        return self.host[self._next()].numpy()

    def upload(self, lo, hi):
        self._copy(lo, hi)

    def download(self, lo, hi):
        """bytes lo .. hi of the device block into the same place of the pinned block; returns once they are there"""
        self._copy(lo, hi, up=False).synchronize()


def _samples(chunk, rs):
    """a pushed chunk as the flat array that is uploaded: float32, or int16 for a row opened with pcm="s16"; an array whose dtype
    does not match the row's format is refused"""
    a = np.asarray(chunk)
    if rs is not None and rs["fmt"] == ops.RS_S16:
        if a.dtype != np.int16:
            raise TypeError(f"LiveServer: a row opened with pcm='s16' takes int16 samples, not {a.dtype}")
        return np.ascontiguousarray(a).reshape(-1)
    if hasattr(chunk, "dtype") and a.dtype.kind in "iub":
        raise TypeError(f"LiveServer: a float32 row takes float samples in [-1, 1), not {a.dtype} (open(..., pcm='s16') for 16-bit PCM)")
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


class _Row:
    __slots__ = ("sid", "n", "base", "n_feat", "fbase", "n_ring", "kd", "sent0", "k_style", "fade", "rs", "offsets", "rt")

    def __init__(self, sid):
        self.sid, self.n, self.base = sid, 0, 0          # samples received (absolute) / absolute index of window[0]
        self.n_feat, self.fbase, self.n_ring = 0, 0, 0   # feature rows computed / frame of feats[r, 0] / frames in the ring
        self.kd, self.sent0 = 1, False                   # first frame not yet decoded / frame 0 (the first pose) handed out
        self.k_style, self.fade = 0, 0                   # last set_style: from frame k_style on, over `fade` frames
        self.rs = None                                   # a converting row: dict(fi, fmt, table, L, M, WL, n_in: raw samples received)
        self.offsets = None                              # frames: the joint positions of frame 0 as placed (the OFFSETs of a BVH file)
        self.rt = None                                   # a re-timing server: dict(L, M, n_in: frames through the head, n_out: frames emitted; with the filter stage also half, table)


class LiveServer:
    """speech_net / decoder: zeggs.modules instances on the device (eval mode); `stats`: dict with audio_input_mean/std,
    anim_input_mean/std, anim_output_mean/std; `audio_conf`: data_pipeline_conf["audio_conf"]; `rows` streams at most at a time
    (<= 64), `tick` >= 3 frames per step (the batch sweep needs chunks of >= 4 frames).

    `loudness`: None, "running" or a dict (loudness_options) -- running loudness normalisation for every row, the streaming
    counterpart of audio_conf.normalize_loudness: each row keeps a BS.1770 gated estimate of what it has received over the last
    `horizon` seconds, and new samples enter its window times the gain that brings the estimate to `target` LUFS (one more
    launch per push / push_many: zeggs_live_loudness_push).  With None a conf that asks for loudness normalisation
    is refused, as before: there is no whole signal to measure.

    `resample`: None or dict(zero_crossings=64, rolloff=0.95, beta=10.0) -- the filter of the rows that open() takes at a rate
    or sample format of their own (audio.resample_options).  A server on which no such row was opened holds no
    converter state and enqueues what it always did.

    `frames`: None or dict(parents=..., names=None, what=("local", "world", "bvh"), order="zyx", text=False) -- the output head
    (frames_options): step() and close() also return, under "frames", what a renderer or a BVH recorder takes of the
    new frames, as host arrays: "root_pos" [n, 3], "root_rot" [n, 4], "lrot" [n, J, 4], "lpos" [n, J, 3] (local), "gpos"
    [n, J, 3], "grot" [n, J, 4] (world, the root folded into joint 0), "bvh" [n, 3 + 3J] float64 (the motion rows of a BVH file
    in the joint order of bvh_header()) and with text=True "text", those rows as the bytes of the file.  One more launch
    (zeggs_live_frames) and one download per step whatever the number of rows; quaternions keep their sign from frame to
    frame and from step to step.  With None the server holds no such state and enqueues what it always did.

    `retime`: None, True or dict(max_rate=...) (with `frames`; retime_options) -- every row's head runs through the
    re-timing kernel (zeggs_live_frames_retimed in place of zeggs_live_frames: the same number of launches), and
    open(..., frame_rate=) gives a stream a frame rate of its own, frame_rate / fps = L / M with 1 <= L, M <= 4096 and L / M <= 8,
    at most `max_rate` (default: the server's own rate, so that only lower rates are taken and the staging blocks stay the
    size they were).  out[sid]["frames"] then holds the stream's new frames at ITS rate (possibly none: empty arrays) and
    "frame0", the index of the first of them; "pose" / "rpos" / "rrot" stay the decoder's rows at `fps`.  Going down in rate is
    point sampling -- 30 from 60 is every second frame, and motion above half the output rate aliases, as decimating a BVH
    file would.  With None the server is the one it was.
    retime=dict(..., filter=True | dict(zero_crossings=4, rolloff=0.75, beta=5.0), min_rate=None) adds the filter stage (DESIGN
    3.7): every row's head runs through zeggs_live_frames_refiltered (the same number of launches), and a stream opened at
    another rate than the server's, or with open(filtered=True), gets each frame as the Kaiser-windowed-sinc combination of the
    2 H + 1 model frames around its position, ahead of FK: H = ceil(zero_crossings max(L, M) / L), 4 at or above the server's
    rate and 10 at 24 from 60 with the defaults.  Such a stream's frames leave H model frames later (frame_delay(sid)): a step's
    "frames" hold what became computable, "frame0" still counts the stream's own frames from 0, and close() hands out the
    rest, so that the stream ends with exactly the frames an unfiltered one has.  `min_rate`: the lowest rate a filtered stream
    may ask for; it sizes the rows' history, 2 ceil(zero_crossings fps / min_rate) raw frames a row; at least fps / 4, default
    the lowest rate that keeps 16 frames to either side.  Rows opened with filtered=False (and rows at the server's rate)
    run the unfiltered rules in the same launch, the same bits as without `filter`.

    `gaze`: None, True or dict(ease="linear" | "smooth") (gaze_options) -- every row keeps a gaze schedule on the
    device and set_gaze() / set_gaze_many() / gaze() work; step() and close() take the per-frame gaze rows and the style rows
    from ONE launch (zeggs_live_condition) in place of _style()'s upload and torch.lerp, so launches_per_step does not grow.
    `ease`: the ease of a set_gaze() that names none.  With None the three calls raise ValueError naming this option, and the
    server allocates and enqueues what it always did.  (The attribute `gaze` is the rows' gaze tensor [rows, tick + 1, 3] it
    has always been AND the call gaze(sid): _GazeRows.)

    `styles`: None, True or dict(net=None, capacity=64, terms=8) (styles_options) -- the server keeps a bank of
    `capacity` named styles on the device, each a mean row and a deviation row of ST floats (include/zeggs_hip_styles.h).
    add_style() / remove_style() / styles() manage it; `net` is the style encoder (zeggs.modules.StyleEncoder, eval mode) that
    add_style() sends example clips through -- without it the bank takes finished vectors only.  set_style(), set_style_many()
    and open() then also take a name, a {name: weight} dict or a list of (name, weight) pairs of at most `terms` entries, mixed
    on the device by ONE launch whatever the number of rows (zeggs_live_style_mix); style(sid) reads a row's style back.  The
    bank is the server's, not a row's: it is not part of a snapshot, and a row keeps the vectors it was given when a slot
    changes afterwards.  step() and close() enqueue what they always did.  With None those calls raise ValueError naming this
    option (set_style() with a tensor works as ever), and the server allocates and enqueues what it always did.

    `plant`: None, True or dict(chains="auto", speed=(v_on, v_off), height=(h_on, h_off), ground=0.0, slack=..., release=...,
    stretch=0.999) (with `frames`; plant_options) -- feet that stay planted.  A planting stage runs in front of the
    output head (zeggs_live_plant: ONE more launch per step whatever the number of rows): per stream and leg chain -- (upper leg,
    lower leg, foot) by name or index, "auto": the Right and Left UpLeg / Leg / Foot of `names` -- it detects ground contact with
    hysteresis (speed in model units a second and height above `ground`), holds the ankle of a foot in contact at a fixed world
    point by an analytic two-bone solve of hip and knee, releases it when the unconstrained ankle leaves by more than `slack`,
    and fades the correction out over `release` frames.  The head reads the corrected copy of the rows, in all three forms;
    "pose" / "rpos" / "rrot" and the decoder's feedback stay the raw rows.  out[sid]["contacts"] [n, chains] bool: the flags of the
    step's MODEL frames (also on a re-timing server), in the step's one download.  The defaults are NOT tuned on captured
    motion.  With None the server allocates and enqueues what it always did."""

    def __init__(self, speech_net, decoder, stats, audio_conf, dt, rows=8, tick=4, feature_type=("mel_spec", "energy"), fps=60.0,
                 device="cuda", window_capacity=16384, loudness=None, resample=None, frames=None, retime=None, gaze=None, styles=None, plant=None):
        g = audio_conf
        loud = loudness_options(loudness)
        self.gaze_conf = gaze_options(gaze)
        self.styles_conf = styles_options(styles)
        self.resample_conf = audio.resample_options(resample)
        self.frames_conf = frames_options(frames)
        self.retime_conf = retime_options(retime, self.frames_conf, fps)
        self.plant_conf = plant_options(plant, self.frames_conf)
        if loud is None and g.get("normalize_loudness"):
            raise ValueError("loudness normalisation needs the whole signal: apply audio.normalize_loudness() first")
        if tuple(feature_type) != ("mel_spec", "energy"):
            raise NotImplementedError("live serving supports the shipped feature set [mel_spec, energy]")
        if g.get("resample_method", "linear") == "cubic":
            raise ValueError("resample_method 'cubic' is a spline over the whole signal: not available while the signal is still arriving")
        if not 1 <= rows <= ops.LIVE_MAX_ROWS or tick < 3:
            raise ValueError(f"LiveServer: rows 1..{ops.LIVE_MAX_ROWS}, tick >= 3")
        self.dev = torch.device(device)
        self.rows, self.tick, self.T = int(rows), int(tick), int(tick) + 1
        self.speech_net, self.decoder = speech_net.eval(), decoder.eval()
        self.st = {k: v.to(self.dev, torch.float32).contiguous() for k, v in stats.items()}
        self.dt, self.fps, self.fs = float(dt), float(fps), int(g["sampling_rate"])
        self.fb, min_clip = audio.mel_tables(g["filter_length"], self.fs, g["n_mel_channels"], g["mel_fmin"], g["mel_fmax"],
                                             g["min_clipping"], g["normalize_mel_bins"], g.get("real_amplitude", True), self.dev)
        self.mel = audio.MelDims(g["filter_length"], g["hop_length"], g["n_mel_channels"], self.fs, self.fps, float(min_clip),
                                 float(g.get("pre_emph_coeff", 0.97)) if g.get("pre_emphasis") else 0.0,
                                 audio.mel_flags(g.get("centered", True), g.get("normalize_range", True), g.get("resample_method", "linear")))
        R, F = self.rows, self.mel.n_mels + 1
        KW = speech_net.layer1.weight.shape[2]
        if (KW - 1) // 2 != LOOKAHEAD:
            raise NotImplementedError("live serving assumes the reference's 31-tap speech encoder")
        self.D = ring_depth(KW, self.tick)
        self.tail = self.tick + LOOKAHEAD            # frames close() can flush in its last call (what the ring still holds)
        self.FC = max(4 * (self.tick + LOOKAHEAD + 1), 64)          # feature rows kept per row until their activation is in the ring
        SP = speech_net.layer2.weight.shape[0]
        ST = decoder.cell_state_encoder.layer0.weight.shape[1] - int(self.st["anim_input_mean"].numel())
        self.H = decoder.recurrent_decoder.layer1.hidden_size
        PO = int(self.st["anim_output_mean"].numel())
        with torch.no_grad():
            self.enc = ops.LiveSpeech(speech_net, self.st["audio_input_mean"], self.st["audio_input_std"], R, self.D, self.FC,
                                      self.tail + 1)
            self.bd = ops.BatchDecode(decoder, R, self.T, SP, ST, self.st["anim_input_mean"], self.st["anim_input_std"],
                                      self.st["anim_output_mean"], self.st["anim_output_std"], self.dt)
        z = lambda *s: torch.zeros(*s, device=self.dev, dtype=torch.float32)  # noqa: E731
        self.window = [z(int(window_capacity)) for _ in range(R)]   # per row: samples base .. n - 1 of its signal
        self.feats = z(R, self.FC, F)                # per row: feature rows of frames fbase .. n_feat - 1 (not yet in the ring)
        self.ring = z(R, self.D, self.enc.d.H)       # per row: layer-0 activations, frame f in slot f % D
        self.h = z(2, R, self.H)                     # GRU state after each row's last decoded frame
        self.pose, self.rpos, self.rrot = z(R, PO), z(R, 3), z(R, 4)       # each row's last decoded frame
        self.rrot[:, 0] = 1.0
        self.gaze = z(R, self.T, 3).as_subclass(_GazeRows)          # (also the call gaze(sid): _GazeRows)
        self.gaze._server = weakref.ref(self)
        self.sty_old, self.sty_new = z(R, ST), z(R, ST)             # style(f) = lerp(old, new, style_weight(f, k_style, fade))
        self.mel_ws = ops.mel_range_workspace(self.mel, self.FC + 2, self.dev)
        # push_many(): the window's alternate buffer (a compaction copies into it and the two swap), scratch for kept feature
        # rows, the batched front-end's tables and workspace, the staging blocks of the one upload per call
        self._alt = [z(int(window_capacity)) for _ in range(R)]
        self._scratch = torch.empty_like(self.feats)
        self._mb = ops.MelBatch(self.mel, self.fb, R, self.FC, self.dev)
        # running loudness: the rows' state, and push()'s staging area for one chunk (push_many's chunks ride in its staging block)
        self.loudness_conf = loud
        self._loud = None if loud is None else ops.LiveLoudness(self.fs, R, loud["ring_blocks"], loud["warmup"], loud["target"],
                                                                loud["gain_db"], audio._kweighting(self.fs), self.dev)
        self._chunk = z(2048) if loud else None
        self._stage = _Staging(R, R * 2048, self.dev, R if loud else 0)
        self._rs = None                              # ops.LiveResample, from the first open(..., rate= / pcm=) on
        self._snap = None                            # _SnapStaging, from the first snapshot*() / restore() on
        # a moving gaze: the rows' schedules (ops.LiveGaze), the style rows the condition launch writes beside self.gaze, and
        # the staging blocks of the records of a set_gaze_many() and of a step with more than one row
        self._gz = self._gz_style = self._gz_set = self._gz_cond = None
        if self.gaze_conf is not None:
            self._gz = ops.LiveGaze(R, ST, self.dev)
            self._gz_style = z(R, self.T, ST)
            self._gz_set = _RecStaging(ops.GazeSet, R, self.dev)
            self._gz_cond = _RecStaging(ops.GazeCond, R, self.dev)
        # named styles: the bank and the rows' noise (ops.LiveStyles), {name: slot}, and the staging blocks of the records of a
        # set_style_many() with more than one record
        self._sb = self._sb_set = None
        self._style_names = {}
        if self.styles_conf is not None:
            self._sb = ops.LiveStyles(R, ST, self.styles_conf["capacity"], self.dev)
            self._sb_set = _RecStaging(ops.StyleMix, R, self.dev)
        self._fr = self._fr_stage = None            # the output head: the rows' state (ops.LiveFrames) and its staging blocks
        self._pl = self._pl_pose = None
        if self.frames_conf is not None:
            fc = self.frames_conf
            if 6 + 15 * len(fc["parents"]) != PO:
                raise ValueError(f"LiveServer: frames has {len(fc['parents'])} joints, the decoder's pose rows hold {(PO - 6) // 15}")
            # a record: a step's tick frames (+ frame 0 once), or what close() flushes in one decoder call.  The head's form is
            # chosen here and nowhere else: its entry points and its record type are the head object's (ops.LiveFrames)
            rc, L, M = self.retime_conf, 1, 1
            if rc is None:
                self._fr = ops.LiveFrames(R, fc["parents"], self.tick + LOOKAHEAD + 1, fc["mask"], fc["order"], fc["seq"], self.dev)
            else:                                    # a row's share of the blocks: what max_rate makes of a record's input frames
                if "filter" in rc:                   # the filter stage: every row's head runs through its kernel, half = 0 without
                    self._fr = ops.LiveRefilter(R, fc["parents"], self.tick + LOOKAHEAD + 1, rc["half_max"], rc["filter"], fc["mask"],
                                                fc["order"], fc["seq"], self.dev)
                else:
                    self._fr = ops.LiveRetime(R, fc["parents"], self.tick + LOOKAHEAD + 1, fc["mask"], fc["order"], fc["seq"], self.dev)
                L, M = rc["ratio"]
            # (a step's record never emits more than its input frames make at max_rate, filtered or not: the filter only
            # delays; the tail record of close() has a block of its own, sized for it)
            # feet that stay planted: the chains' states (ops.LivePlant), the corrected copy of a step's rows, which the head
            # reads in place of the decoder's, and behind the head's three areas the contact flags of the step's model frames
            tail = {}
            if self.plant_conf is not None:
                self._pl = ops.LivePlant(R, fc["parents"], self._fr.d.max_frames, self.plant_conf, self.dt, self.dev)
                self._pl_pose = torch.empty(R, self._fr.d.max_frames, PO, device=self.dev, dtype=torch.float32)
                tail = dict(tail_bytes=R * self._fr.d.max_frames * self._pl.C, tail_record=ops.PlantRow)
            self._fr_stage = _FrameStaging(R, -(-self._fr.d.max_frames * L // M), self._fr.J, fc["mask"], self.dev, self._fr.record, **tail)
        self.status = ops.new_status(self.dev)       # give-up word of THIS server's decoder calls, looked at after every step
        self.redone_steps = 0
        self._rows = [None] * R
        self._sids, self._next_sid = {}, 0
        self._ops = 0
        self.stats = dict(uploaded_samples=0, window_capacity=[int(window_capacity)] * R, ring_bytes=self.ring.numel() * 4,
                          launches_per_step=0, steps=0, ops_last_push_many=0, uploaded_bytes=0, resampled_rows=0)
        if self._gz is not None:
            self.stats["ops_last_set_gaze"] = 0
        if self._sb is not None:
            self.stats["ops_last_set_style"] = 0
        if self._fr is not None:
            self.stats["frame_bytes"] = 0            # bytes the output head has downloaded so far

    # ------------------------------------------------------------------ rows
    def _row(self, sid):
        if sid not in self._sids:
            raise KeyError(f"LiveServer: no open stream {sid}")
        r = self._sids[sid]
        return r, self._rows[r]

    def _frame_rate(self, frame_rate):
        """open()'s `frame_rate` -> None (a server without re-timing) or the row's dict(L, M, n_in, n_out); ValueError naming both
        rates on a server without `retime`, for a ratio the kernel does not take and for a rate above max_rate"""
        conf = self.retime_conf
        if conf is None:
            if frame_rate is None:
                return None
            raise ValueError(f"LiveServer.open: frame_rate {frame_rate!r} on a server that hands out {self.fps!r} frames per second: "
                             "re-timing is off (LiveServer(frames=..., retime=True))")
        if frame_rate is None:
            L, M = 1, 1
        else:
            try:
                L, M = ops.retime_ratio(frame_rate, self.fps)
            except ValueError as e:
                raise ValueError(f"LiveServer.open: {e}") from None
        if L * conf["ratio"][1] > conf["ratio"][0] * M:
            raise ValueError(f"LiveServer.open: frame_rate {frame_rate!r} on a server at {self.fps!r} frames per second is above its "
                             f"max_rate {float(conf['max_rate'])!r} (LiveServer(retime=dict(max_rate=...)))")
        return LiveServer._retimed(None, L, M)

    @staticmethod
    def _retimed(fr, L, M, n_in=0, n_out=0, half=-1):
        """a row's re-timing dict, for open() from its arguments and for restore() from a blob's counters.  half < 0: a server
        without the filter stage; 0: an unfiltered stream of one that has it; > 0: a filtered stream -- the half and the table
        are those of the head `fr` at the ratio (built and uploaded here, the first time a row has the ratio)"""
        rt = dict(L=L, M=M, n_in=n_in, n_out=n_out)
        if half > 0:
            t = fr.table(L, M)
            rt.update(half=t["half"], table=t["table"])
        elif half == 0:
            rt.update(half=0, table=None)
        return rt

    def _converter(self, fi, fmt, n_in=0):
        """a converting row's dict, for open() and restore() alike; the server's converter is made at its first use"""
        if self._rs is None:
            self._rs = ops.LiveResample(self.fs, self.rows, self.resample_conf, self.dev)
        return dict(self._rs.table(fi), fi=fi, fmt=fmt, n_in=n_in)

    def _free_row(self, needed=True):
        """the first free row; with none the RuntimeError of open(), or None for a caller that only sizes"""
        for r, row in enumerate(self._rows):
            if row is None:
                return r
        if needed:
            raise RuntimeError(f"LiveServer: all {self.rows} rows are in use")
        return None

    def _filter_of(self, rt, frame_rate, filtered):
        """open()'s `filtered` -> the row's dict with the filter's half = H and table where the stream is filtered (the table is
        built and uploaded here, the first time a row opens at the ratio).  None: filtered if and only if the server has the
        filter stage and the stream's rate differs from the server's.  ValueError naming both rates for filtered=True on a
        server without `filter`, for a ratio the filter does not take and for a rate below the server's min_rate."""
        conf = self.retime_conf
        rate = self.fps if frame_rate is None else frame_rate
        if conf is None or "filter" not in conf:
            if filtered:
                raise ValueError(f"LiveServer.open: filtered=True at frame_rate {rate!r} on a server that hands out {self.fps!r} frames per "
                                 "second: the filter stage is off (LiveServer(frames=..., retime=dict(filter=True)))")
            return rt
        L, M = rt["L"], rt["M"]
        if not (L != M if filtered is None else filtered):
            return LiveServer._retimed(None, L, M, rt["n_in"], rt["n_out"], half=0)
        if L > ops.REFILTER_MAX_L or M > ops.REFILTER_MAX_DOWN * L:
            raise ValueError(f"LiveServer.open: frame_rate {rate!r} on a server at {self.fps!r} frames per second is the ratio {L} / {M}: a "
                             f"filtered stream takes L <= {ops.REFILTER_MAX_L} and M <= {ops.REFILTER_MAX_DOWN} L (filtered=False: point sampling)")
        from fractions import Fraction
        if Fraction(L, M) * Fraction(str(float(self.fps))) < conf["min_rate"]:
            raise ValueError(f"LiveServer.open: frame_rate {rate!r} on a server at {self.fps!r} frames per second is below its min_rate "
                             f"{float(conf['min_rate'])!r} (LiveServer(retime=dict(min_rate=...)) sizes the filter's history)")
        return LiveServer._retimed(self._fr, L, M, rt["n_in"], rt["n_out"], half=1)

    def frame_delay(self, sid):
        """what the filter stage adds to stream `sid`'s latency -> (input frames, seconds): H frames of the server's rate for a
        filtered stream (4 at or above the server's rate, 10 at 24 from 60 with the defaults), (0, 0.0) for any other"""
        rt = self._row(sid)[1].rt
        H = 0 if rt is None else int(rt.get("half", 0))
        return H, H / self.fps

    def open(self, first_pose, style, gain=1.0, rate=None, pcm="f32", start_position=None, start_rotation=None, frame_rate=None,
             filtered=None, temperature=None, seed=None):
        """a new stream on a free row: `first_pose` the 16-tuple of anim.preprocess_animation (frame 0 is used), `style` [1, S]
        -- or, on a server with `styles`, a name, a {name: weight} dict or a list of (name, weight) pairs of the bank, with
        `temperature` / `seed` as set_style() takes them: the mix launch writes the row's two style rows ahead of the
        CellStateEncoder, which reads the mixed row on the device.  -> stream id.  The GRU state comes from the CellStateEncoder (zeggs_decoder_state_init).  `gain` (running loudness only):
        what the row's samples are multiplied by until its first estimate; the row's loudness state starts from nothing.
        `rate` / `pcm`: what this stream delivers -- `rate` Hz (None: the server's rate) as "f32" (float32 in [-1, 1)) or "s16"
        (int16 PCM, x = s / 32768).  Anything but float32 at the server's rate is converted on the device as it arrives
        (zeggs_resample_push: band-limited, in front of the loudness stage and the window); a rate the converter does not
        take raises ValueError naming both rates.
        `start_position` [3] / `start_rotation` [4] (a server with `frames`; both or neither): where the character stands -- the
        root of the stream's frames is re-based on its frame 0, start_rot ref_rot^-1 (x - ref_pos) + start_pos, as write_bvh
        does for a clip; with neither the root is handed out as the decoder integrates it.
        `frame_rate` (a server with `retime`): the rate this stream's "frames" leave at -- an int, a fractions.Fraction, a
        (num, den) pair, or a float taken as Fraction(str(x)) (29.97 is 2997/100; the NTSC rate proper is (30000, 1001));
        None: the server's rate.  ValueError naming both rates on a server without `retime`, for a ratio outside 1 <= L, M
        <= 4096, L / M <= 8 and for a rate above the server's max_rate.
        `filtered` (a server with retime=dict(filter=...)): True -- the stream's frames are band-limited ahead of FK, a windowed-sinc
        combination of the 2 H + 1 model frames around each output frame, H = frame_delay(sid)[0] model frames later;
        False -- the two cheap rules (point sampling downward, the shortest arc upward); None: filtered if and only if the
        stream's rate differs from the server's.  filtered=True at the server's own rate is a jitter filter.  ValueError naming
        both rates for filtered=True on a server without `filter`, a ratio with L > 1024 or M > 4 L and a rate below min_rate."""
        rs = resample_row(rate, pcm, self.fs)
        place = frames_placement(start_position, start_rotation)
        if place is not None and self._fr is None:
            raise ValueError("LiveServer.open: a placement needs the output head (LiveServer(frames=...))")
        if self._loud is None and float(gain) != 1.0:
            raise ValueError("LiveServer.open: a gain needs running loudness (LiveServer(loudness=...))")
        rt = LiveServer._filter_of(self, self._frame_rate(frame_rate), frame_rate, filtered)
        named = None
        if not isinstance(style, torch.Tensor):
            self._styles_on("open")
            named = style_request(dict(style=style, temperature=temperature, seed=seed), self._style_names, self.styles_conf["terms"])
        elif temperature is not None or seed is not None:
            raise ValueError("LiveServer.open: temperature / seed sample a named style; a tensor is taken as it is")
        r, sid = self._free_row(), self._next_sid
        if self._loud is not None:
            ops.live_loudness_reset(self._loud, r, gain)
        self._next_sid += 1
        f32 = lambda a: a[0:1].to(self.dev, torch.float32).contiguous()  # noqa: E731
        root_pos, root_rot, root_vel, root_vrt, lpos, lrot, ltxy, lvel, lvrt = first_pose[:9]
        pose0 = torch.cat([f32(x).reshape(1, -1) for x in (root_vel, root_vrt, lpos, ltxy, lvel, lvrt)], dim=1)
        gaze0 = f32(first_pose[14])
        row = _Row(sid)
        if named is None:
            style0 = style.to(self.dev, torch.float32).reshape(1, -1).contiguous()
        else:                                            # the mix writes sty_old[r] = sty_new[r] (reset); the encoder reads that row
            with torch.no_grad():
                self._mix([(r, row, named)], reset=True)
            style0 = self.sty_new[r:r + 1]
        with torch.no_grad():
            self.h[:, r:r + 1] = ops.decoder_state_init(self.bd, pose0, f32(root_pos), f32(root_rot), gaze0, style0)
        self.pose[r], self.rpos[r], self.rrot[r] = pose0[0], f32(root_pos)[0], f32(root_rot)[0]
        self.gaze[r] = gaze0
        if self._gz is not None:                         # the row's schedule: it looks at the first pose's gaze until a set_gaze
            ops.live_gaze_reset(self._gz, r, gaze0.reshape(-1))
        if named is None:
            self.sty_old[r], self.sty_new[r] = style0[0], style0[0]
        if rs is not None:
            row.rs = self._converter(*rs)
            ops.live_resample_reset(self._rs, r)
        if self._fr is not None:
            J = self._fr.J
            p0, r0 = f32(root_pos).reshape(1, 3), f32(root_rot).reshape(1, 4)
            row.rt = rt
            if place is None:
                ops.live_head_reset(self._fr, r)
            else:
                ops.live_head_reset(self._fr, r, p0[0].cpu().numpy(), r0[0].cpu().numpy(), *place)
            if self._pl is not None:
                ops.live_plant_reset(self._pl, r)
            pos0, _ = anim.bvh_channels(p0, r0, pose0[:, 6:6 + 3 * J].reshape(1, J, 3), pose0[:, 6 + 3 * J:6 + 9 * J].reshape(1, J, 2, 3),
                                        *(place or (None, None)), order=self.frames_conf["order"])
            row.offsets = pos0[0].cpu().numpy()
        self._rows[r], self._sids[sid] = row, r
        return sid

    # ------------------------------------------------------------------ frames out
    def bvh_header(self, sid, nframes=0):
        """the head of a BVH file for stream `sid` (anim.bvh_header: HIERARCHY and the MOTION head for `nframes` frames at the
        server's dt, or the stream's own frame time dt M / L on a re-timing server) with the joint positions of the stream's frame
        0, as placed, as OFFSETs (the MODEL's frame 0, for a filtered stream too: its own frame 0 already leans on the frames behind it) -- what
        write_bvh and generate_gesture write.  `nframes` of a closed stream is the same with and without the filter.  Followed by the stream's "text" (or anim.format_rows of its "bvh" rows) it is a BVH file."""
        if self._fr is None:
            raise RuntimeError("LiveServer: the output head is off (LiveServer(frames=...))")
        fc, row = self.frames_conf, self._row(sid)[1]
        dt = self.dt if row.rt is None or row.rt["L"] == row.rt["M"] else self.dt * row.rt["M"] / row.rt["L"]
        head, seq = anim.bvh_header(row.offsets, fc["parents"], fc["names"], fc["order"], int(nframes), dt)
        assert seq == fc["seq"]
        return head

    def _frames_text(self, table, counts, outs):
        """outs[i]["text"]: the BVH rows of record i as the bytes of a file -- ONE table through the device formatter
        (zeggs_table_text_device), cut at the records' last row ends; a value outside its domain sends the table through the
        host formatter (anim._host_pieces, counted in anim.TEXT_FALLBACKS)"""
        cuts = np.cumsum(counts)[:-1].tolist()
        for o, piece in zip(outs, anim.format_rows_device(table, cuts)):
            o["text"] = bytes(piece)

    @staticmethod
    def _frames_records(recs, rows, rts, srcs, i, counts, outputs, final, base, areas, a=0):
        """fills the head records of ONE launch: record k brings counts[k] input frames of row rows[k] from frame i of its output
        tensors srcs[k] (float32 rows) and emits behind the records before it, the first behind output frame `a` of the packed
        block at the device address `base` (`areas`: frames_layout).  On a re-timing server -- rts[k] is the row's dict -- also the
        ratio, the input counter and outputs[k], which the caller has from _emitted; with the filter stage -- the dict carries
        half -- also the row's half and table, and `final`.  -> the output frame behind the last record"""
        bvh, loc, wld = areas
        for q, r, rt, o, count, outs in zip(recs, rows, rts, srcs, counts, outputs):
            pose, rpos, rrot = o["pose"], o["rpos"], o["rrot"]
            ld = q.pose_ld, q.rpos_ld, q.rrot_ld = pose.stride(0), rpos.stride(0), rrot.stride(0)
            q.pose, q.rpos, q.rrot = pose.data_ptr() + 4 * i * ld[0], rpos.data_ptr() + 4 * i * ld[1], rrot.data_ptr() + 4 * i * ld[2]
            q.bvh = base + bvh[0] + a * bvh[1] if bvh else None
            q.local = base + loc[0] + a * loc[1] if loc else None
            q.world = base + wld[0] + a * wld[1] if wld else None
            q.row, q.count = r, count
            if rt is None:
                a += count
                continue
            q.L, q.M, q.n_in, q.outputs = rt["L"], rt["M"], rt["n_in"] + i, outs
            if "half" in rt:
                half = q.half = rt["half"]
                q.final, q.table = final, rt["table"].data_ptr() if half else None
            a += outs
        return a

    def _plant_records(self, recs, rows, srcs, i, counts, dests, flags):
        """fills the planting records of ONE launch: record k takes counts[k] frames of row rows[k] from frame i of its output
        tensors srcs[k], writes the corrected rows to the same frames of dests[k] (float32 rows of PO) and the contact flags behind
        those of the records before it, the first at the device address `flags` -> what the head's records read in place of
        srcs: the same root tensors, the corrected rows as "pose"."""
        C_, planted = self._pl.C, []
        for q, r, o, count, dst in zip(recs, rows, srcs, counts, dests):
            pose, rpos, rrot = o["pose"], o["rpos"], o["rrot"]
            ld = q.pose_ld, q.rpos_ld, q.rrot_ld = pose.stride(0), rpos.stride(0), rrot.stride(0)
            q.pose, q.rpos, q.rrot = pose.data_ptr() + 4 * i * ld[0], rpos.data_ptr() + 4 * i * ld[1], rrot.data_ptr() + 4 * i * ld[2]
            q.out, q.out_ld, q.contacts = dst.data_ptr() + 4 * i * dst.stride(0), dst.stride(0), flags
            q.row, q.count = r, count
            flags += count * C_
            planted.append(dict(pose=dst, rpos=rpos, rrot=rrot))
        return planted

    def _frames_step(self, out, live):
        """the output head of a step: out[sid]["frames"] for the rows `live`, from the tensors out[sid] holds -- ONE launch and
        ONE download whatever their number"""
        fr, stg, fc = self._fr, self._fr_stage, self.frames_conf
        src = [out[self._rows[r].sid] for r in live]
        n_in = [int(o["pose"].shape[0]) for o in src]
        rts = [self._rows[r].rt for r in live] if self.retime_conf is not None else None
        # a re-timing server: a record emits what the counting rule gives its row for these input frames
        counts = n_in if rts is None else [self._emitted(t, t["n_in"] + c, False) - t["n_out"] for t, c in zip(rts, n_in)]
        N, J = sum(counts), fr.J
        areas, nbytes = frames_layout(N, J, fc["mask"])
        flags = 0                                        # bytes of the contact flags behind the three areas (a planting server)
        if self._pl is not None:                         # ONE more launch: the head's records then point at the planted copy
            flags = sum(n_in) * self._pl.C
            src = self._plant_records(stg.tail_recs, live, src, 0, n_in, [self._pl_pose[r] for r in live], stg.dev.data_ptr() + nbytes)
            ops.live_plant(self._pl, stg.tail_recs, len(live), stg.tail_mem.data_ptr() if len(live) > 1 else None)
            self._ops += 1
        self._frames_records(stg.recs, live, rts or [None] * len(live), src, 0, n_in, counts, 0, stg.dev.data_ptr(), areas)
        ops.live_head_launch(fr, stg.recs, len(live), stg.rec_mem.data_ptr() if len(live) > 1 else None)
        # (a step in which no row of a re-timing server emits a frame has nothing to bring down; it counts as if it had)
        buf = stg.download(nbytes + flags) if N or flags else np.zeros(0, np.uint8)
        got = frames_unpack(buf, counts, J, fc["mask"])
        self._ops += 2
        self.stats["frame_bytes"] += nbytes + flags
        if self._pl is not None:
            a = nbytes
            for r, c in zip(live, n_in):
                out[self._rows[r].sid]["contacts"] = np.array(buf[a:a + c * self._pl.C]).reshape(c, self._pl.C).astype(bool)
                a += c * self._pl.C
        if fc["text"]:
            self._frames_text(stg.dev[:N * areas[0][1]].view(torch.float64).view(N, fr.bvh_doubles), counts, got)
            self._ops += 3                               # (the formatter's call and its two downloads: row ends, then the text)
        for i, (r, g) in enumerate(zip(live, got)):
            if rts is not None:
                g["frame0"] = rts[i]["n_out"]
                rts[i]["n_in"] += n_in[i]
                rts[i]["n_out"] += counts[i]
            out[self._rows[r].sid]["frames"] = g

    @staticmethod
    def _emitted(rt, n, final):
        """output frames a re-timing row has emitted after n input frames: the filtered rule while a filtered stream runs"""
        if rt.get("half", 0) and not final:
            return ops.refilter_n_out(n, rt["L"], rt["M"], rt["half"])
        return ops.retime_n_out(n, rt["L"], rt["M"])

    def _frames_close(self, r, o):
        """the output head of close(): the tail `o` of row r through the same kernel and state, max_frames frames a call; on a
        re-timing server the output frames the counting rule gives the row for them -- there is no tail of its own, except for
        a filtered stream: its last record is marked final and emits everything up to retime_n_out of all its input frames"""
        fr, fc, rt = self._fr, self.frames_conf, self._rows[r].rt
        n_in, J, M = int(o["pose"].shape[0]), fr.J, fr.d.max_frames
        n = n_in if rt is None else self._emitted(rt, rt["n_in"] + n_in, True) - rt["n_out"]
        areas, nbytes = frames_layout(n, J, fc["mask"])
        pl = self._pl
        block = torch.empty(nbytes + (n_in * pl.C if pl is not None else 0), dtype=torch.uint8, device=self.dev)
        rec = (fr.record * 1)()
        base, a = block.data_ptr(), 0                    # a: output frames written so far
        if pl is not None:                               # the tail's corrected rows, and its contact flags behind the three areas
            prec, planted = (ops.PlantRow * 1)(), torch.empty(max(n_in, 1), o["pose"].shape[1], device=self.dev, dtype=torch.float32)
        for i in range(0, max(n_in, 1 if rt is not None and rt.get("half", 0) else 0), M):       # (a filtered stream: the final record, even an empty one)
            count, final, outputs = min(M, n_in - i), int(i + M >= n_in), None
            if rt is not None:
                outputs = self._emitted(rt, rt["n_in"] + i + count, final) - self._emitted(rt, rt["n_in"] + i, False)
            src = o
            if pl is not None and count > 0:
                src = self._plant_records(prec, (r,), (o,), i, (count,), (planted,), base + nbytes + i * pl.C)[0]
                ops.live_plant(pl, prec, 1)
            a = self._frames_records(rec, (r,), (rt,), (src,), i, (count,), (outputs,), final, base, areas, a)
            ops.live_head_launch(fr, rec, 1)
        buf = block.cpu().numpy()
        got = frames_unpack(buf, [n], J, fc["mask"])
        if pl is not None:
            got[0]["contacts"] = np.array(buf[nbytes:]).reshape(n_in, pl.C).astype(bool)
        self.stats["frame_bytes"] += int(block.numel())
        if fc["text"]:
            self._frames_text(block[:n * areas[0][1]].view(torch.float64).view(n, fr.bvh_doubles), [n], got)
        if rt is not None:
            got[0]["frame0"] = rt["n_out"]
            rt["n_in"], rt["n_out"] = rt["n_in"] + n_in, rt["n_out"] + n
        return got[0]

    # ------------------------------------------------------------------ audio
    def _grow_feats(self, FC):
        """more rows per pending-feature block (one push brought more frames than a block holds): every row's block is re-laid"""
        self.FC = FC
        grown = torch.zeros(self.rows, FC, self.feats.shape[2], device=self.dev)
        grown[:, :self.feats.shape[1]] = self.feats
        self.feats = grown
        self._scratch = torch.empty_like(grown)
        self.mel_ws = ops.mel_range_workspace(self.mel, FC + 2, self.dev)
        self._mb.resize(FC)

    def _features(self, r, row, k1, final):
        """feature rows [n_feat, k1) of row r from its window -> feats[r]"""
        k0 = row.n_feat
        if k1 <= k0:
            return
        pend = k0 - row.n_ring                           # rows still waiting for the ring: frames n_ring .. k0 - 1
        if k0 - row.fbase + (k1 - k0) > self.FC:         # compact (and grow if this one push needs more than the block holds)
            keep = self.feats[r, row.n_ring - row.fbase:k0 - row.fbase].clone()
            if pend + (k1 - k0) > self.FC:
                self._grow_feats(pend + (k1 - k0))
            self.feats[r, :pend] = keep
            row.fbase = row.n_ring
        out = self.feats[r, k0 - row.fbase:k1 - row.fbase]
        ops.mel_features_window(self.mel, self.window[r], row.base, row.n, final, self.fb, k0, k1, out, self.mel_ws)
        row.n_feat = k1

    def push(self, sid, wav_chunk):
        """append samples (float32 in [-1, 1)) to stream `sid`: only they are uploaded; the mel rows that became computable are
        computed.  Frames leave through step()."""
        r, row = self._row(sid)
        if row.rs is not None:                           # a converting row: the same launches as push_many(), one record each
            return self.push_many({sid: wav_chunk})
        chunk = torch.as_tensor(_samples(wav_chunk, None))
        m = int(chunk.numel())
        if m == 0:
            return
        w = self.window[r]
        if row.n - row.base + m > w.numel():
            # drop what no frame >= n_feat loads any more; grow only if this single push does not fit beside what must stay
            nb = max(row.base, min(ops.mel_window_first_sample(self.mel, row.n_feat), row.n))
            keep = w[nb - row.base:row.n - row.base].clone()
            if keep.numel() + m > w.numel():
                w = torch.zeros(keep.numel() + m, device=self.dev)
                self.window[r] = w
                self.stats["window_capacity"][r] = int(w.numel())
            w[:keep.numel()] = keep
            row.base = nb
        if self._loud is None:
            w[row.n - row.base:row.n - row.base + m].copy_(chunk)
        else:                                            # the same kernel as push_many(), one record (in the kernel arguments)
            if self._chunk.numel() < m:
                self._chunk = torch.empty(2 * m, device=self.dev)
            self._chunk[:m].copy_(chunk)
            rec = (ops.LoudRow * 1)()
            rec[0].src, rec[0].dst = self._chunk.data_ptr(), w.data_ptr() + 4 * (row.n - row.base)
            rec[0].count, rec[0].row = m, r
            ops.live_loudness_push(self._loud, rec, 1)
        row.n += m
        self.stats["uploaded_samples"] += m
        self.stats["uploaded_bytes"] += 4 * m
        ready = min(ops.mel_frames_ready(self.mel, row.n), audio.n_anim_frames(row.n, self.fs, self.fps) - 1)
        self._features(r, row, ready, final=False)       # (never ahead of the final frame count: it can only grow)

    def push_many(self, chunks):
        """push() for many streams at once: chunks = {sid: samples}.  Same bookkeeping per row (plan_push), same feature bits,
        but what the call enqueues does not depend on the number of rows: ONE upload (copy records, mel records and all new
        samples in a pinned block), ONE zeggs_copy_segments (window compactions into the alternate buffers, the new samples
        behind them, kept feature rows to scratch), a second one only when some row compacts its feature block, and the TWO
        launches of zeggs_mel_features_batch -- stats["ops_last_push_many"] <= 5.  Growth (a chunk that does not fit its window,
        more new frames than a feature block holds) reallocates first, as in push().  An unknown sid raises KeyError before
        anything changes.  With running loudness the new samples leave the copy list and are the records of ONE
        zeggs_live_loudness_push (uploaded in the same block): <= 6 operations; windows, features and loudness state are
        bitwise those of push(), however the signal is cut and whichever rows share a call.
        A row opened at a rate or format of its own takes its raw samples (int16 for pcm="s16"): they ride behind the float
        samples of the same one upload, the host plans with audio.resample_ready how many converted samples the row owes, and
        ONE zeggs_resample_push for all such rows writes them where the copy launch or the loudness launch finds its sources
        -- exactly one more operation, <= 6 (<= 7 with running loudness), and only in a call in which some row converts."""
        rows = [self._row(sid) for sid in chunks]
        items = [(r, row, _samples(c, row.rs)) for (r, row), c in zip(rows, chunks.values())]
        self._push_rows([(r, row, c) for r, row, c in items if c.size], False)

    def _push_rows(self, items, final):
        """push_many() behind its argument checks; `final` (close()): the converting rows' signals end here, their tails enter
        the windows against zero padding"""
        self.stats["ops_last_push_many"] = n_ops = 0
        conv = [i for i, (_, w, _) in enumerate(items) if w.rs is not None]
        lens = [c.size for _, _, c in items]
        for i in conv:
            q, n1 = items[i][1].rs, items[i][1].rs["n_in"] + lens[i]
            due = audio.resample_total(n1, q["L"], q["M"]) if final else audio.resample_ready(n1, q["L"], q["M"], q["WL"])
            lens[i] = due - items[i][1].n               # (a converting row's n: converted samples in its window = outputs so far)
        if not any(c.size or m for (_, _, c), m in zip(items, lens)):
            return
        F = self.feats.shape[2]
        plan = plan_push([dict(n=w.n, base=w.base, n_feat=w.n_feat, fbase=w.fbase, n_ring=w.n_ring) for _, w, _ in items],
                         [self.window[r].numel() for r, _, _ in items], lens, self.FC, F,
                         lambda k: ops.mel_window_first_sample(self.mel, k),
                         lambda n: min(ops.mel_frames_ready(self.mel, n), audio.n_anim_frames(n, self.fs, self.fps) - 1))
        # ---- growth, the one exception to "nothing is allocated"
        if plan["FC"] > self.FC:
            self._grow_feats(plan["FC"])
            n_ops += 3
        for (r, _, _), p in zip(items, plan["rows"]):
            if p["swap"] and self._alt[r].numel() < p["cap"]:
                self._alt[r] = torch.zeros(p["cap"], device=self.dev)
                n_ops += 1
        raw_bytes = sum((items[i][2].nbytes + 63) // 64 * 64 for i in conv)
        if plan["n_stage"] > self._stage.n_samples or (conv and self._stage.tail(plan["n_stage"], len(conv), raw_bytes)[2] > self._stage.nbytes):
            self._stage.idle()
            n_smp = 2 * plan["n_stage"] if plan["n_stage"] > self._stage.n_samples else self._stage.n_samples
            self._stage = _Staging(self.rows, n_smp, self.dev, self._stage.loud_rows,
                                   max(self._stage.tail_bytes, 2 * (raw_bytes + self.rows * C.sizeof(ops.ResampleRow) + 128)) if conv
                                   else self._stage.tail_bytes)
        # ---- the staging block: records with device addresses, then the samples (a converting row's share of the sample area
        # is written by the converter on the device), then the converter's records and raw input
        stg = self._stage
        blk = stg.take()
        pos, end = 0, None
        for (_, w, c), m in zip(items, lens):
            if w.rs is None:
                blk["smp"][pos:pos + m] = c
            pos += m
        if conv:
            o_rs, o_raw, end = stg.tail(plan["n_stage"], len(conv), raw_bytes)
            rs_recs = (ops.ResampleRow * len(conv)).from_buffer(blk["block"], o_rs)
            offs = np.concatenate([[0], np.cumsum(lens)])
            for q, i in zip(rs_recs, conv):
                (r, w, c), t = items[i], items[i][1].rs
                blk["block"][o_raw:o_raw + c.nbytes] = c.view(np.uint8)
                q.src, q.dst, q.table = stg.dev.data_ptr() + o_raw, stg.dev.data_ptr() + stg.o_smp + 4 * int(offs[i]), t["table"].data_ptr()
                q.count, q.n_in, q.n_out, q.outputs, q.WL = c.size, t["n_in"], w.n, lens[i], t["WL"]
                q.row, q.format, q.final, q.L, q.M = r, t["fmt"], int(final), t["L"], t["M"]
                o_raw += (c.nbytes + 63) // 64 * 64
        block_bytes = 4 * self.FC * F
        where = {"win": lambda i: self.window[items[i][0]].data_ptr(), "alt": lambda i: self._alt[items[i][0]].data_ptr(),
                 "stage": lambda i: stg.dev.data_ptr() + stg.o_smp, "feats": lambda i: self.feats.data_ptr() + items[i][0] * block_bytes,
                 "scratch": lambda i: self._scratch.data_ptr() + items[i][0] * block_bytes}
        segs, loud = plan["segs"], []
        if self._loud is not None:
            # the new samples do not go through the copy launch: they enter their windows through the loudness kernel, scaled
            loud = [s for s in segs if s[0][0] == "stage"]
            segs = [s for s in segs if s[0][0] != "stage"]
            for q, ((sk, si), so, (dk, di), do, cnt) in zip(blk["loud"], loud):
                q.src, q.dst, q.count, q.row = where[sk](si) + 4 * so, where[dk](di) + 4 * do, cnt, items[di][0]
        for name, copies in (("segs", segs), ("back", plan["segs_back"])):
            for j, ((sk, si), so, (dk, di), do, cnt) in enumerate(copies):
                g = blk[name][j]
                g.src, g.dst, g.count = where[sk](si) + 4 * so, where[dk](di) + 4 * do, cnt
        n_mel = 0
        for (r, _, _), p in zip(items, plan["rows"]):
            if p["k1"] > p["k0"]:
                q = blk["mel"][n_mel]
                q.wav = (self._alt[r] if p["swap"] else self.window[r]).data_ptr()
                q.out = self.feats.data_ptr() + r * block_bytes + 4 * (p["k0"] - p["fbase"]) * F
                q.base, q.n_samples, q.k0, q.k1, q.final = p["base"], p["n"], p["k0"], p["k1"], 0
                n_mel += 1
        # ---- at most five operations (six with running loudness), one more in a call with converting rows
        with torch.no_grad():
            stg.upload(plan["n_stage"], end)
            n_ops += 1
            if conv:
                ops.live_resample_push(self._rs, rs_recs, len(conv), stg.dev.data_ptr() + o_rs)
                n_ops += 1
            if segs:
                ops.copy_segments(blk["segs"], len(segs), stg.dev.data_ptr())
                n_ops += 1
            if loud:
                ops.live_loudness_push(self._loud, blk["loud"], len(loud), stg.dev.data_ptr() + stg.o_loud)
                n_ops += 1
            if plan["segs_back"]:
                ops.copy_segments(blk["back"], len(plan["segs_back"]), stg.dev.data_ptr() + stg.o_back)
                n_ops += 1
            if n_mel:
                n_ops += ops.mel_features_batch(self._mb, blk["mel"], n_mel, stg.dev.data_ptr() + stg.o_mel)
        for (r, row, c), p in zip(items, plan["rows"]):
            if p["swap"]:
                self.window[r], self._alt[r] = self._alt[r], self.window[r]
                self.stats["window_capacity"][r] = int(self.window[r].numel())
            row.n, row.base, row.n_feat, row.fbase = p["n"], p["base"], p["n_feat"], p["fbase"]
            if row.rs is None:
                self.stats["uploaded_samples"] += int(c.size)
            else:
                row.rs["n_in"] += int(c.size)
                self.stats["resampled_rows"] += 1
        self.stats["uploaded_bytes"] += stg.o_smp + 4 * plan["n_stage"] if end is None else end
        self.stats["ops_last_push_many"] = n_ops

    # ------------------------------------------------------------------ running loudness
    def _loud_row(self, sid):
        if self._loud is None:
            raise RuntimeError("LiveServer: running loudness is off (LiveServer(loudness=...))")
        return self._row(sid)[0]

    def loudness(self, sid):
        """-> dict(lufs: the row's last estimate (NaN before the first), gain: what new samples are multiplied by, blocks: gating
        blocks completed, gated: blocks past the relative gate at the last one, held: the last block left the gain as it was --
        no estimate, or hold()).  One small read-back that waits for the stream: monitoring, not for the tick path."""
        got = ops.live_loudness_read(self._loud, self._loud_row(sid))
        return {k: got[k] for k in ("lufs", "gain", "blocks", "gated", "held")}

    def hold(self, sid, on=True):
        """freeze the row's gain at what it is (it goes on metering), or release it: the next estimate moves it again"""
        ops.live_loudness_hold(self._loud, self._loud_row(sid), on)

    # ------------------------------------------------------------------ style
    def set_style(self, sid, style, fade=0, temperature=None, seed=None):
        """a new style for stream `sid` from frame k on, k = the first frame not yet decoded (returned); `fade` > 0: a linear
        cross-fade, frame f carries lerp(old, new, style_weight(f, k, fade)).
        `style`: a tensor [S] / [1, S] -- or, on a server with `styles`, a name, a {name: weight} dict or a list of (name,
        weight) pairs of the bank (style_terms): the row's new style is sum_i w_i (mean_i + (dev_i / temperature) eps_i) over the
        named slots, in float64, rounded once, and its old style is where an unfinished fade stands at frame k - 1,
        both written by ONE launch with the record in its arguments (zeggs_live_style_mix).
        `temperature` None (or 0): the means alone -- deterministic.  This is a default of the LIVE path only: the offline entry
        points sample at temperature 1.0 unless told otherwise.  With temperature t > 0 the noise is ops.randn((terms, S),
        seed=seed), one more launch into the row's slice of the server's noise tensor (`seed` None: ops.next_seed()); one term
        of weight 1 is then the offline style_net(example, t, eps).  Neither applies to a tensor.
        ValueError before anything is enqueued for a negative fade, an unknown name, too many terms, a weight or temperature
        that is not finite, and a named style on a server without `styles`; KeyError for a stream that is not open."""
        if not isinstance(style, torch.Tensor):
            self._styles_on("set_style")
            return self.set_style_many({sid: dict(style=style, fade=fade, temperature=temperature, seed=seed)})[sid]
        if temperature is not None or seed is not None:
            raise ValueError("set_style: temperature / seed sample a named style; a tensor is taken as it is")
        r, row = self._row(sid)
        if fade < 0:
            raise ValueError("set_style: fade >= 0")
        w = style_weight(row.kd - 1, row.k_style, row.fade)      # where an unfinished fade stands: the new fade starts there
        self.sty_old[r] = torch.lerp(self.sty_old[r], self.sty_new[r], w)
        self.sty_new[r] = style.to(self.dev, torch.float32).reshape(-1)
        row.k_style, row.fade = row.kd, int(fade)
        return row.kd

    # ------------------------------------------------------------------ named styles
    def _styles_on(self, what):
        if self._sb is None:
            raise ValueError(f"LiveServer.{what}: named styles are off (LiveServer(styles=True))")

    def styles(self):
        """-> {name: slot} of the bank"""
        self._styles_on("styles")
        return dict(self._style_names)

    def add_style(self, name, source, trim=None, mirror=False):
        """put a style into the bank under `name` -> its slot.  A name the bank already has keeps its slot and is overwritten;
        rows that were set from it keep the vectors they were given.  `source`:
          * a BVH path, a parsed clip (the dict of anim.bvh_load) or un-normalised exemplar rows [L, F] -- an EXAMPLE: it goes
            through the calls the offline front end makes (anim.preprocess_animation, the exemplar feature rows, (x -
            anim_input_mean) / anim_input_std, the style encoder) and the encoder's raw row -- mean | log-variance for a VAE
            encoder -- goes into the slot without leaving the device (zeggs_live_style_put).  The encoder's products run in a
            fixed summation order here (ops.fixed_order_gemms), so the same example gives the same slot, bit for bit, on every
            call and every server; the offline call gives these bits under the same switch and differs in the last place
            without it, from run to run.  Needs LiveServer(styles=dict(net=));
            `trim` = (a, b) keeps frames a .. b - 1 of the clip, as generate_gesture's (path, (a, b)) does; `mirror`: the clip's
            left/right reflection (anim.mirror_take after loading, before the features: a BVH path or a parsed clip only);
          * a 1-D tensor or array of S floats -- an embedding computed elsewhere, or a one-hot label of a label-conditioned
            model: the slot's mean, deviation 0 -- or of 2 S floats, an encoder row computed elsewhere (mean | log-variance).
            Needs no encoder.
        Set-up work, not for the tick path: a clip is parsed on the host and encoded by a call of its own.  ValueError for a
        name that is not a string, an example without `net`, a vector or encoder row of another length; RuntimeError naming the
        capacity when the bank is full."""
        self._styles_on("add_style")
        if not isinstance(name, str):
            raise ValueError(f"add_style: a name is a string, not {name!r}")
        ST, conf = int(self.sty_old.shape[1]), self.styles_conf
        vector = isinstance(source, (torch.Tensor, np.ndarray)) and source.ndim == 1
        if not vector and conf["net"] is None:
            raise ValueError("add_style: an example needs the style encoder (LiveServer(styles=dict(net=style_net))); without it the "
                             f"bank takes vectors of {ST} floats")
        if vector and int(source.shape[0]) not in (ST, 2 * ST):
            raise ValueError(f"add_style: a vector of {int(source.shape[0])} floats, the model's styles have {ST} (or {2 * ST}: mean | log-variance)")
        if trim is not None and (vector or len(trim) != 2):
            raise ValueError(f"add_style: trim {trim!r} is (first frame, end) of an example")
        if mirror and (vector or isinstance(source, (torch.Tensor, np.ndarray))):
            raise ValueError("add_style: mirror reflects an example's BVH channels: give a BVH path or a parsed clip")
        if name not in self._style_names and len(self._style_names) >= conf["capacity"]:
            raise RuntimeError(f"add_style: the bank is full, all {conf['capacity']} slots are in use (LiveServer(styles=dict(capacity=...)); "
                               "remove_style() frees one)")
        with torch.no_grad():
            if vector:
                enc = torch.as_tensor(source).to(self.dev, torch.float32).contiguous()
            else:
                enc = self._encode_example(source, trim, mirror)
                if int(enc.numel()) not in (ST, 2 * ST):
                    raise ValueError(f"add_style: the style encoder returns {int(enc.numel())} floats, the model's styles have {ST}")
            if name in self._style_names:
                slot = self._style_names[name]
            else:
                slot = min(set(range(conf["capacity"])) - set(self._style_names.values()))
            ops.live_style_put(self._sb, slot, enc)
        self._style_names[name] = slot
        return slot

    def _encode_example(self, source, trim, mirror=False):
        """the style encoder's raw output row [E] for an example (add_style), on the device"""
        import pathlib
        from . import modules
        from .generate import _example_features
        if isinstance(source, (torch.Tensor, np.ndarray)):
            rows = torch.as_tensor(source).to(self.dev, torch.float32)
            if rows.ndim != 2 or rows.shape[1] != self.st["anim_input_mean"].numel():
                raise ValueError(f"add_style: exemplar rows are [L, {self.st['anim_input_mean'].numel()}], not {list(rows.shape)}")
            if trim is not None:
                rows = rows[trim[0]:trim[1]]
        else:
            if isinstance(source, (pathlib.PurePath, str)):
                clip = anim.bvh_load(source)
            elif isinstance(source, dict):
                clip = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in source.items()}
            else:
                raise ValueError(f"add_style: a BVH path, a parsed clip, exemplar rows [L, F] or a vector, not {type(source).__name__}")
            if trim is not None:
                clip["rotations"] = clip["rotations"][trim[0]:trim[1]]
                clip["positions"] = clip["positions"][trim[0]:trim[1]]
            if mirror:
                clip = anim.mirror_take(clip)
            rows = _example_features(anim.preprocess_animation(clip, self.dev))
        if rows.shape[0] < 1:
            raise ValueError("add_style: the example has no frames")
        ex = ((rows - self.st["anim_input_mean"]) / self.st["anim_input_std"])[None].contiguous()
        net = self.styles_conf["net"]
        enc = net.encoder
        with ops.fixed_order_gemms():                    # no split-K atomics: the same example fills a slot with the same bits on every server
            out = ops.style_encoder_gru(ex, enc) if isinstance(enc, modules.StyleEncoderGRU) else ops.style_encoder_attn(ex, enc, net.training)
        return out.reshape(-1).contiguous()

    def remove_style(self, name):
        """take `name` out of the bank; its slot is free for the next add_style().  Rows keep the vectors they were given"""
        self._styles_on("remove_style")
        if name not in self._style_names:
            raise ValueError(f"remove_style: no style {name!r} in the bank (it holds {sorted(self._style_names)})")
        del self._style_names[name]

    def set_style_many(self, requests):
        """set_style() with named styles for many streams at once: requests = {sid: style | dict(style=, fade=, temperature=,
        seed=)} -> {sid: k}.  Whatever the number of streams: ONE upload of the records and ONE launch (zeggs_live_style_mix; a
        single record travels in the kernel arguments, without the upload), plus one noise launch per record that samples --
        what a director changing the mood of every character in a tick calls.  The rows' vectors and counters are bit for bit
        those of the same requests as single set_style() calls.  Every request is checked before anything is enqueued;
        stats["ops_last_set_style"] counts what the call enqueued."""
        self._styles_on("set_style_many")
        rows = [self._row(sid) for sid in requests]
        reqs = [style_request(q, self._style_names, self.styles_conf["terms"]) for q in requests.values()]
        self.stats["ops_last_set_style"] = 0
        if not reqs:
            return {}
        with torch.no_grad():
            self.stats["ops_last_set_style"] = self._mix([(r, row, o) for (r, row), o in zip(rows, reqs)], reset=False)
        for (_, row), o in zip(rows, reqs):
            row.k_style, row.fade = row.kd, o["fade"]
        return {sid: row.kd for sid, (_, row) in zip(requests, rows)}

    def _mix(self, jobs, reset):
        """ONE zeggs_live_style_mix launch for jobs = [(r, row, checked request)], in front of it the upload of the records where
        there are several and a noise launch per record that samples -> the number of operations enqueued"""
        n, sb = len(jobs), self._sb
        recs = (ops.StyleMix * 1)() if n == 1 else self._sb_set.take()
        count = 1 if n == 1 else 2
        for q, (r, row, o) in zip(recs, jobs):
            terms = o["terms"]
            q.slot[:] = [s for s, _ in terms] + [0] * (ops.STYLE_MAX_TERMS - len(terms))
            q.weight[:] = [w for _, w in terms] + [0.0] * (ops.STYLE_MAX_TERMS - len(terms))
            q.k, q.k_style, q.fade_style = row.kd, row.k_style, row.fade
            q.row, q.terms, q.reset, q.temperature, q.eps_row = r, len(terms), int(reset), o["temperature"], -1
            if o["temperature"] > 0.0:
                ops.randn_into(sb.eps[r, :len(terms)], o["seed"])
                q.eps_row = r
                count += 1
        dev = None if n == 1 else self._sb_set.upload(n)
        ops.live_style_mix(sb, recs, n, self.sty_old, self.sty_new, dev)
        return count

    def style(self, sid):
        """-> dict(old [S], new [S]: the row's two style vectors, k, fade: its fade, current [S]: the style of frame kd, the first
        frame not yet decoded, lerp(old, new, style_weight(kd, k, fade)) by torch.lerp's float32 formula with the multiply-add in
        one rounding, as the device evaluates it).  One small read-back that waits for the stream: monitoring, not for the tick
        path."""
        self._styles_on("style")
        r, row = self._row(sid)
        old, new = ops.live_style_read(self._sb, row=r, sty_old=self.sty_old, sty_new=self.sty_new)
        w = np.float32(style_weight(row.kd, row.k_style, row.fade))
        d = (new - old).astype(np.float64)              # (a product of two float32 values is exact in float64)
        current = (old + np.float64(w) * d if w < 0.5 else new - d * np.float64(np.float32(1.0) - w)).astype(np.float32)
        return dict(old=old, new=new, k=row.k_style, fade=row.fade, current=current)

    def _style(self, jobs):
        """style rows [R, n, ST] of the jobs' frames, jobs = [(row, -, first frame, frames)] as _condition() takes them (a row
        without a job: its current style)"""
        n = max(j[3] for j in jobs)
        wgt = np.ones((self.rows, n, 1), np.float32)
        for r, _, k0, cnt in jobs:
            row = self._rows[r]
            wgt[r, :cnt, 0] = [style_weight(x, row.k_style, row.fade) for x in range(k0, k0 + cnt)]
        self._ops += 2
        return torch.lerp(self.sty_old[:, None], self.sty_new[:, None], torch.as_tensor(wgt, device=self.dev)).contiguous()

    # ------------------------------------------------------------------ gaze
    def _gaze_on(self, what):
        if self._gz is None:
            raise ValueError(f"LiveServer.{what}: the moving gaze is off (LiveServer(gaze=True))")

    def set_gaze(self, sid, target, fade=0, space="world", path="line", pivot=None, ease=None):
        """a new gaze target for stream `sid` from frame k on, k = the first frame not yet decoded (returned): frame f looks at
        P(w(f)), w = style_weight(f, k, fade) -- with ease="smooth" w^2 (3 - 2 w) -- from P(0), where the row's gaze stands at
        frame k - 1 (an unfinished fade goes on from where it is), to P(1) = `target`.
        `space`: "world" -- target and pivot are points of the model's world, the space of "rpos" (gaze_to_model() brings a point
        of a placed character's space there); "root" -- they are given in the character's root frame and resolved ON THE DEVICE,
        once, with the row's root state after frame k - 1: world = rpos + rrot (x) p.  The call does not follow the root
        afterwards: a client that wants the gaze re-centred on a drifting character calls again.
        `path`: "line" -- P(w) = (1 - w) P(0) + w P(1); "arc" -- the direction turns about `pivot` on the great circle while the
        distance goes on a line, the line where a direction is undefined; the pivot defaults to the root position in
        root space and is required in world space.  `ease` None: the server's (LiveServer(gaze=dict(ease=...))).
        ValueError before anything is enqueued for a negative fade, a target or pivot that is not three finite numbers, an
        unknown space, path or ease; KeyError for a stream that is not open.  ONE launch, the record in its arguments."""
        self._gaze_on("set_gaze")
        return self.set_gaze_many({sid: dict(target=target, fade=fade, space=space, path=path, pivot=pivot, ease=ease)})[sid]

    def set_gaze_many(self, requests):
        """set_gaze() for many streams at once: requests = {sid: target | dict(target=, fade=, space=, path=, pivot=, ease=)} ->
        {sid: k}.  Whatever the number of streams: ONE upload of the records and ONE launch (zeggs_live_gaze_set; a single
        record travels in the kernel arguments, without the upload) -- the call a tracker makes every tick.  Every request is
        checked before anything is enqueued; stats["ops_last_set_gaze"] counts what the call enqueued."""
        self._gaze_on("set_gaze_many")
        rows = [self._row(sid) for sid in requests]
        reqs = [gaze_request(q, self.gaze_conf["ease"]) for q in requests.values()]
        self.stats["ops_last_set_gaze"] = 0
        if not reqs:
            return {}
        n = len(reqs)
        recs = (ops.GazeSet * 1)() if n == 1 else self._gz_set.take()
        for q, (r, row), o in zip(recs, rows, reqs):
            q.target[:] = [float(v) for v in o["target"]]
            q.pivot[:] = [0.0] * 3 if o["pivot"] is None else [float(v) for v in o["pivot"]]
            q.k, q.fade, q.row, q.has_pivot = row.kd, o["fade"], r, int(o["pivot"] is not None)
            q.space, q.path, q.ease = ops.GAZE_SPACES[o["space"]], ops.GAZE_PATHS[o["path"]], ops.GAZE_EASES[o["ease"]]
        with torch.no_grad():
            dev = None if n == 1 else self._gz_set.upload(n)
            ops.live_gaze_set(self._gz, recs, n, self.rpos, self.rrot, dev)
        self.stats["ops_last_set_gaze"] = 1 if n == 1 else 2
        return {sid: row.kd for sid, (_, row) in zip(requests, rows)}

    def _gaze_read(self, sid):
        """gaze(sid) (the attribute `gaze` is the rows' tensor and this call: _GazeRows) -> dict(target [3]: what frame kd, the
        first frame not yet decoded, will look at; k, fade, start [3], end [3], path, ease: the row's schedule, float32 points of
        the model's world).  One small read-back that waits for the stream: monitoring, not for the tick path."""
        self._gaze_on("gaze")
        r, row = self._row(sid)
        got = ops.live_gaze_read(self._gz, r, row.kd)
        return {k: got[k] for k in ("target", "k", "fade", "start", "end", "path", "ease")}

    def _conditioned(self, jobs, own=False):
        """the conditioning of ONE decoder call, jobs = [(row, output slice, first frame, frames)] -> (gaze rows or None, style
        rows).  A gaze server: both from ONE launch (_condition), into the step's tensors or, for `own` (close(): one job of up
        to tick + LOOKAHEAD + 1 frames), into tensors of the call's own length.  Any other server: no gaze rows, and style rows
        by _style() -- those of every row of the server, or for `own` the job's row alone."""
        if self._gz is None:
            style = self._style(jobs)
            return None, style[jobs[0][0]:jobs[0][0] + 1].contiguous() if own else style
        gaze, style = self.gaze, self._gz_style
        if own:
            n = jobs[0][3]
            gaze, style = torch.empty(1, n, 3, device=self.dev), torch.empty(1, n, self.sty_old.shape[1], device=self.dev)
        self._condition(jobs, gaze, style)
        return gaze, style

    def _condition(self, jobs, gaze_out, style_out):
        """the conditioning rows of one decoder call on a gaze server: jobs = [(row, out_row, first frame, frames)] -> the gaze
        rows [., n, 3] and the style rows [., n, ST] of those frames in slice out_row of the two tensors, by ONE launch
        (zeggs_live_condition) -- in place of _style()'s weight upload and torch.lerp.  Several records are uploaded first."""
        n = len(jobs)
        recs = (ops.GazeCond * 1)() if n == 1 else self._gz_cond.take()
        for q, (r, o, k0, cnt) in zip(recs, jobs):
            row = self._rows[r]
            q.row, q.out_row, q.k0, q.n, q.k_style, q.fade_style = r, o, k0, cnt, row.k_style, row.fade
        dev = None if n == 1 else self._gz_cond.upload(n)
        ops.live_condition(self._gz, recs, n, self.sty_old, self.sty_new, gaze_out, style_out, dev)
        self._ops += 1 if n == 1 else 2

    # ------------------------------------------------------------------ decode
    def _encode(self, jobs, out_ld):
        """one zeggs_speech_encoder_live launch; jobs[r] = None or (enc_k0, n_out, n_new, last) -> speech [R, out_ld, O]"""
        lr = []
        for r in range(self.rows):
            row = self._rows[r]
            if jobs[r] is None:
                lr.append(ops.LiveRow(0, 0, -1, 0, 0, 0, 0))
                continue
            k0, n_out, n_new, last = jobs[r]
            lr.append(ops.LiveRow(row.n_ring, k0, last, n_new, n_out, row.n_ring - row.fbase, 0))
        speech = torch.empty(self.rows, out_ld, self.enc.d.O, device=self.dev)
        ops.speech_encoder_live(self.enc, lr, self.feats, self.ring, speech)
        self._ops += 1
        for r in range(self.rows):
            if jobs[r] is not None:
                self._rows[r].n_ring += jobs[r][2]
        return speech

    def _decode_one(self, r, speech, style, n, gaze=None):
        """frames kd .. kd + n - 1 of row r alone on the B = 1 entry point (speech / style [1, n + 1, .], index 0 = frame kd - 1);
        the give-up word is looked at before the state is committed, a chunk that gave up is redone on the stage launches.
        `gaze` [1, n + 1, 3]: the per-frame rows of a gaze server (None: the row's fixed point in every frame)"""
        st = self.st
        if gaze is None:
            gaze = self.gaze[r:r + 1, :1].expand(1, n + 1, 3).contiguous()
        args = (self.decoder, self.pose[r:r + 1], self.rpos[r:r + 1], self.rrot[r:r + 1],
                gaze, speech, style, st["anim_input_mean"], st["anim_input_std"],
                st["anim_output_mean"], st["anim_output_std"], self.dt)
        h_in = self.h[:, r:r + 1].contiguous()
        pose, rpos, rrot, h = ops.decoder_chunk(*args, h_in=h_in, status=self.status)
        self._ops += 3
        if ops._persistent_live(0):
            bits = int(self.status[0].item())
            if bits:
                ops._warn_gave_up(bits, "the step")
                ops.set_option("persistent", 0)
                ops.fill_(self.status.view(torch.float32))
                self.redone_steps += 1
                pose, rpos, rrot, h = ops.decoder_chunk(*args, h_in=h_in, status=self.status)
        self.h[:, r:r + 1] = h
        self.pose[r], self.rpos[r], self.rrot[r] = pose[0, -1], rpos[0, -1], rrot[0, -1]
        self._ops += 4
        return pose[0], rpos[0], rrot[0]

    def _head(self, r):
        """frame 0 of row r (its first pose) if it has not been handed out yet, else None; taken BEFORE the row's state moves on"""
        if self._rows[r].sent0:
            return None
        self._rows[r].sent0 = True
        return self.pose[r:r + 1].clone(), self.rpos[r:r + 1].clone(), self.rrot[r:r + 1].clone()

    @staticmethod
    def _emit(head, pose, rpos, rrot):
        """frames 1.. of a decoded chunk (index 0 is the frame it started from), with frame 0 in front once per stream"""
        o = (pose[1:], rpos[1:], rrot[1:])
        if head is not None:
            o = tuple(torch.cat([a, b]) for a, b in zip(head, o))
        return dict(zip(("pose", "rpos", "rrot"), o))

    def step(self):
        """-> {sid: {"pose": [tick, PO], "rpos": [tick, 3], "rrot": [tick, 4]}} for every row that had `tick` decodable frames
        (the first step of a stream also carries frame 0, the first pose, in front).  With `frames` also "frames"; on a re-timing
        server those are the stream's new frames at ITS rate, possibly none, and "frame0" the index of the first of them."""
        rows = [None if x is None else dict(n_feat=x.n_feat, n_ring=x.n_ring, kd=x.kd) for x in self._rows]
        plan = plan_step(rows, self.tick, self.D)
        live = [r for r in range(self.rows) if plan[r] is not None]
        if not live:
            return {}
        self._ops = 0
        tick, T = self.tick, self.T
        with torch.no_grad():
            speech = self._encode([None if p is None else (p["enc_k0"], p["n_out"], p["n_new"], -1) for p in plan], T)
            gaze, style = self._conditioned([(r, r, plan[r]["enc_k0"], T) for r in live])
            out = {}
            heads = {r: self._head(r) for r in live}
            if self.rows == 1:
                row = self._rows[0]
                pose, rpos, rrot = self._decode_one(0, speech, style, tick, gaze)
                out[row.sid] = self._emit(heads[0], pose, rpos, rrot)
                row.kd += tick
            else:
                info = {}
                pose, rpos, rrot, h = ops.decoder_batch_chunk(self.bd, self.pose, self.rpos, self.rrot, self.gaze, speech, style,
                                                              self.h, status=self.status, info=info)
                if info["gave_up"]:                  # (the chunk was redone with mode 1 before anything is committed below)
                    self.redone_steps += 1
                mask = torch.zeros(self.rows, dtype=torch.bool)
                mask[live] = True
                mask = mask.to(self.dev)
                # masked commit: rows that did not take part keep their state (theirs was computed from filler)
                self.h = torch.where(mask[None, :, None], h, self.h)
                self.pose = torch.where(mask[:, None], pose[:, -1], self.pose)
                self.rpos = torch.where(mask[:, None], rpos[:, -1], self.rpos)
                self.rrot = torch.where(mask[:, None], rrot[:, -1], self.rrot)
                self._ops += 6
                for r in live:
                    row = self._rows[r]
                    out[row.sid] = self._emit(heads[r], pose[r], rpos[r], rrot[r])
                    row.kd += tick
            if self._fr is not None:
                self._frames_step(out, live)
        self.stats["launches_per_step"] = self._ops
        self.stats["steps"] += 1
        return out

    def drain(self):
        """step() until no row is eligible -> {sid: frames} concatenated over the steps"""
        acc = {}
        while True:
            out = self.step()
            if not out:
                break
            for sid, o in out.items():
                acc.setdefault(sid, []).append(o)
        out = {sid: {k: torch.cat([o[k] for o in v]) for k in v[0] if k not in ("frames", "contacts")} for sid, v in acc.items()}
        if self._pl is not None:
            for sid, v in acc.items():
                out[sid]["contacts"] = np.concatenate([o["contacts"] for o in v])
        if self._fr is not None:
            for sid, v in acc.items():
                out[sid]["frames"] = frames_cat([o["frames"] for o in v])
        return out

    def close(self, sid):
        """end of stream `sid`'s signal: its remaining frames with the right-edge rules of the offline path (reflect padding of the
        STFT, replicate padding of the speech encoder), decoded for that row alone; the row is free again"""
        r, row = self._row(sid)
        if row.rs is not None:                           # the converter's tail enters the window ahead of the final features
            self._push_rows([(r, row, np.zeros(0, np.int16 if row.rs["fmt"] == ops.RS_S16 else np.float32))], True)
        n_total = audio.n_anim_frames(row.n, self.fs, self.fps)
        outs = []
        with torch.no_grad():
            if row.n > 0:
                self._features(r, row, n_total, final=True)
            if n_total >= 1 and not row.sent0:
                outs.append(self._head(r))
            while row.kd < n_total:
                rem = n_total - row.kd
                n = rem if rem <= self.tail else self.tick       # the last call flushes what the ring still reaches
                final = n == rem
                top = n_total if final else row.kd + n + LOOKAHEAD
                jobs = [None] * self.rows
                jobs[r] = (row.kd - 1, n + 1, top - row.n_ring, n_total - 1 if final else -1)
                speech = self._encode(jobs, self.tail + 1)[r:r + 1, :n + 1].contiguous()
                gaze, style = self._conditioned([(r, 0, row.kd - 1, n + 1)], own=True)
                pose, rpos, rrot = self._decode_one(r, speech, style, n, gaze)
                outs.append((pose[1:], rpos[1:], rrot[1:]))
                row.kd += n
            out = {k: torch.cat([o[i] for o in outs]).contiguous() for i, k in enumerate(("pose", "rpos", "rrot"))} if outs else {}
            if not outs and self._fr is not None and row.rt is not None and row.rt.get("half", 0) and row.rt["n_in"] > 0:
                # a filtered stream whose frames all left through step(): the final record brings no frame and emits the tail
                out = dict(pose=self.pose[r:r], rpos=self.rpos[r:r], rrot=self.rrot[r:r])
            if out and self._fr is not None:
                out["frames"] = self._frames_close(r, out)
                if self._pl is not None:
                    out["contacts"] = out["frames"].pop("contacts")
        self._rows[r] = None
        del self._sids[sid]
        return out

    # ------------------------------------------------------------------ snapshot and restore
    def _fingerprint(self):
        """{field: number} over SNAP_FINGERPRINT: everything that sizes or interprets a row's state.  Not the weights, not the
        statistics."""
        import zlib
        m, lc, rc, fc, tc = self.mel, self.loudness_conf, self.resample_conf, self.frames_conf, self.retime_conf
        fl = (tc or {}).get("filter")
        fp = dict(tick=self.tick, fs=self.fs, fps=self.fps, mel_n_fft=m.n_fft, mel_hop=m.hop, mel_n_mels=m.n_mels, mel_fs=m.fs, mel_fps=m.fps,
                  mel_min_clip=m.min_clip, mel_pre_emph=m.pre_emph, mel_flags=m.flags, FC=self.FC, ring_depth=self.D,
                  ring_width=self.ring.shape[2], H=self.H, ST=self.sty_old.shape[1], PO=self.pose.shape[1], speech_width=self.enc.d.O,
                  KW=self.D - self.tick, loudness=int(lc is not None), loudness_target=lc["target"] if lc else 0.0,
                  loudness_ring_blocks=lc["ring_blocks"] if lc else 0, loudness_warmup=lc["warmup"] if lc else 0,
                  loudness_gain_lo=lc["gain_db"][0] if lc else 0.0, loudness_gain_hi=lc["gain_db"][1] if lc else 0.0,
                  resample_zero_crossings=rc["zero_crossings"], resample_rolloff=rc["rolloff"], resample_beta=rc["beta"],
                  frames=int(fc is not None), frames_joints=len(fc["parents"]) if fc else 0, frames_what=fc["mask"] if fc else 0,
                  frames_order=anim._to_euler_order(fc["order"]) if fc else 0,
                  frames_seq=zlib.crc32(np.asarray(fc["seq"], "<i4").tobytes()) if fc else 0,
                  retime=int(tc is not None), retime_max_L=tc["ratio"][0] if tc else 0, retime_max_M=tc["ratio"][1] if tc else 0,
                  filter=int(fl is not None), filter_zero_crossings=fl["zero_crossings"] if fl else 0, filter_rolloff=fl["rolloff"] if fl else 0.0,
                  filter_beta=fl["beta"] if fl else 0.0, filter_min_rate_num=tc["min_rate"].numerator if fl else 0,
                  filter_min_rate_den=tc["min_rate"].denominator if fl else 0, filter_half_max=tc["half_max"] if fl else 0)
        assert set(fp) == set(SNAP_FINGERPRINT)
        pc = self.plant_conf
        if pc is not None:                               # only a planting server's fingerprint has these
            fp.update(plant_chains=zlib.crc32(np.asarray(pc["chains"], "<i4").tobytes()), plant_v_on=pc["speed"][0], plant_v_off=pc["speed"][1],
                      plant_h_on=pc["height"][0], plant_h_off=pc["height"][1], plant_ground=pc["ground"], plant_slack=pc["slack"],
                      plant_release=pc["release"], plant_stretch=pc["stretch"])
            assert set(fp) == set(SNAP_FINGERPRINT + SNAP_FINGERPRINT_PLANT)
        return {k: float(v) for k, v in fp.items()}

    def _snap_pieces(self, r, n_window, n_pending, rs_on):
        """where the device side of row r's sections lives -> {section: [(device address, bytes)]}, for a row with n_window
        live samples and n_pending pending feature rows; `rs_on`: the row converts.  A section's pieces follow one another in
        the blob, each on a 16-byte boundary."""
        F4 = 4 * self.feats.shape[2]
        at = lambda t, i: t.data_ptr() + i * t.stride(0) * 4  # noqa: E731
        p = dict(window=[(self.window[r].data_ptr(), 4 * n_window)], feats=[(at(self.feats, r), F4 * n_pending)],
                 ring=[(at(self.ring, r), 4 * self.ring.shape[1] * self.ring.shape[2])],
                 h=[(self.h[i, r].data_ptr(), 4 * self.H) for i in range(2)],
                 pose=[(at(self.pose, r), 4 * self.pose.shape[1])], rpos=[(at(self.rpos, r), 12)], rrot=[(at(self.rrot, r), 16)],
                 gaze=[(at(self.gaze, r), 12 * self.T)], sty_old=[(at(self.sty_old, r), 4 * self.sty_old.shape[1])],
                 sty_new=[(at(self.sty_new, r), 4 * self.sty_new.shape[1])], loudness=[], resample=[], head=[])
        rs = self._rs if rs_on else None
        if rs_on and rs is None:                        # (restore()'s size check ahead of the converter's first use: sizes only)
            rs = types.SimpleNamespace(state=None, d=ops.ResampleDims(self.rows, 2 * self.resample_conf["zero_crossings"] * audio.RESAMPLE_MAX_DECIMATION))
        # (section, the stage or None, its span report, whether its pieces ride behind what the section has: a gaze server's
        # schedule behind the gaze rows, a planting server's chains behind the head's pieces)
        for name, obj, spans, behind in (("gaze", self._gz, ops.live_gaze_spans, True), ("loudness", self._loud, ops.live_loudness_spans, False),
                                         ("resample", rs, ops.live_resample_spans, False), ("head", self._fr, ops.live_frames_spans, False),
                                         ("head", self._pl, ops.live_plant_spans, True)):
            if obj is not None:
                base = 0 if obj.state is None else obj.state.data_ptr()
                p[name] = (p[name] if behind else []) + [(base + o, b) for o, b in spans(obj, r)]
        for t in (self.feats, self.ring, self.h, self.pose, self.rpos, self.rrot, self.gaze, self.sty_old, self.sty_new):
            assert t.is_contiguous()
        return p

    @staticmethod
    def _snap_sizes(pieces, host):
        """bytes per section in SNAP_SECTIONS' order: the host sections as they are, a device section's pieces on 16-byte boundaries"""
        return [len(host[k]) if k in host else (sum(_a16(b) for _, b in pieces[k][:-1]) + pieces[k][-1][1] if pieces[k] else 0) for k in SNAP_SECTIONS]

    def _snap_stage(self):
        if self._snap is None:
            self._snap = _SnapStaging(self.dev)          # (the first snapshot or restore: a server that never does allocates nothing)
        return self._snap

    def snapshot(self, sid):
        """snapshot_many([sid])[sid]"""
        return self.snapshot_many([sid])[sid]

    def snapshot_many(self, sids=None):
        """-> {sid: blob}: everything that determines the future outputs of each stream in `sids` (None: every open stream), as
        one numpy.uint8 array per stream that restore() of any server with the same configuration takes -- on this server (a
        fork), on another GPU, in another process.  The streams go on exactly as before.  A snapshot may be taken between any two
        calls: right after open(), after a push no step has consumed, in a style fade, while a filtered stream's last frames
        are held back, after hold(); not after close() (KeyError, before anything is enqueued).
        Whatever the number of streams: ONE upload (the segment records), ONE launch (zeggs_live_pack gathers a thousand pieces
        of 64 rows as it gathers the fifteen of one) and ONE download into a pinned block, which the call waits for; the blobs
        are copies of its slices.  stats["ops_last_snapshot"] counts the three.
        A blob holds the live part of the row's sample window and its pending feature rows, the layer-0 ring, the GRU state,
        the last pose and root, gaze and both styles, the row's spans of every state block the server has (running loudness,
        the rate converter, the output head: include/zeggs_hip_snapshot.h) and the host counters, behind a header with a
        fingerprint of the configuration (SNAP_FINGERPRINT; snapshot_info() reads it).  It does NOT cover the networks and the
        statistics: restoring into a server with other weights is the caller's business."""
        sids = list(self._sids) if sids is None else list(sids)
        rows = [self._row(sid) for sid in sids]
        if len(set(sids)) != len(sids):
            raise ValueError("LiveServer.snapshot_many: a stream is named twice")
        if not sids:
            return {}
        fp, version = self._fingerprint(), ops.lib().zeggs_live_snapshot_version()
        plans, n_seg, at = [], 0, 0
        for r, row in rows:
            rs, rt, off = row.rs, row.rt, row.offsets
            vals = dict(n=row.n, base=row.base, n_feat=row.n_feat, fbase=row.fbase, n_ring=row.n_ring, kd=row.kd, sent0=int(row.sent0),
                        k_style=row.k_style, fade=row.fade, rs=int(rs is not None), rs_fi=rs["fi"] if rs else 0, rs_fmt=rs["fmt"] if rs else 0,
                        rs_n_in=rs["n_in"] if rs else 0, rt=int(rt is not None), rt_L=rt["L"] if rt else 0, rt_M=rt["M"] if rt else 0,
                        rt_n_in=rt["n_in"] if rt else 0, rt_n_out=rt["n_out"] if rt else 0, rt_half=rt.get("half", -1) if rt else -1,
                        offsets_itemsize=off.dtype.itemsize if off is not None else 0, offsets_count=off.size if off is not None else 0)
            host = dict(row=np.array([vals[k] for k in SNAP_ROW], "<i8").tobytes(), offsets=b"" if off is None else np.ascontiguousarray(off).tobytes())
            pieces = self._snap_pieces(r, row.n - row.base, row.n_feat - row.fbase, rs is not None)
            sizes = self._snap_sizes(pieces, host)
            offs, total = snapshot_layout(sizes, len(_snap_fields(fp)))
            plans.append(dict(host=host, pieces=pieces, sizes=sizes, offs=offs, total=total, at=at))
            n_seg += sum(1 for v in pieces.values() for _, b in v if b)
            at += (total + 63) // 64 * 64
        o_blobs = (n_seg * C.sizeof(ops.SnapSeg) + 63) // 64 * 64
        stg = self._snap_stage()
        blk = stg.take(o_blobs + at)
        segs, j = (ops.SnapSeg * n_seg).from_buffer(blk, 0), 0
        for p in plans:
            for name, o in zip(SNAP_SECTIONS, p["offs"]):
                for addr, nb in p["pieces"].get(name, ()):
                    if nb:
                        segs[j].src, segs[j].dst_offset, segs[j].bytes = addr, p["at"] + o, nb
                        j += 1
                    o += _a16(nb)
        assert j == n_seg
        n_ops = 0
        with torch.no_grad():
            stg.upload(0, o_blobs)
            ops.live_pack(segs, n_seg, stg.dev.data_ptr(), stg.dev.data_ptr() + o_blobs, at)
            stg.download(o_blobs, o_blobs + at)
            n_ops += 3
        del segs
        out = {}
        for sid, p in zip(sids, plans):
            mine = blk[o_blobs + p["at"]:o_blobs + p["at"] + p["total"]]
            head = snapshot_header(sid, version, fp, p["sizes"])
            mine[:len(head)] = np.frombuffer(head, np.uint8)
            for name, o, nb in zip(SNAP_SECTIONS, p["offs"], p["sizes"]):
                if name in p["host"]:
                    mine[o:o + nb] = np.frombuffer(p["host"][name], np.uint8)
                    mine[o + nb:_a16(o + nb)] = 0
                    continue
                for _, b in p["pieces"][name]:               # what lies between the pieces is not the stream's: zeroes
                    mine[o + b:o + _a16(b)] = 0
                    o += _a16(b)
            out[sid] = np.array(mine)
        self.stats["ops_last_snapshot"] = n_ops
        self.stats["snapshot_bytes"] = self.stats.get("snapshot_bytes", 0) + at
        return out

    def restore(self, blob):
        """a stream from snapshot() / snapshot_many() on a free row of THIS server -> its new stream id.  The stream goes on as the
        one the blob was taken from would have: the same frames for the same further input, bit for bit where the stages are
        (the audio side and the output head; the decoder's sums are what they are between any two servers).  The source is
        not involved: restoring on the server the blob came from is a fork.
        Everything is checked on the host before anything is enqueued -- magic and versions, every field of the configuration
        fingerprint (ValueError naming the first that differs and both values), every section's size against this server's
        own span reports and tensor shapes, the total length: a blob that is refused leaves the server as it was, no row taken,
        no launch made.  With no free row: the RuntimeError of open().  Then ONE upload (the blob with its segment records) and
        ONE launch (zeggs_live_unpack); the row's host counters come from the blob, the converter's and the filter's tables are
        rebuilt from the recorded rate and ratio by the host functions open() uses (float64 host arithmetic: the same bits;
        uploaded only where this server has not seen the rate yet, as in open()).  The live samples go to the front of the
        row's window with `base` kept; a window too small for them grows first.  stats["ops_last_restore"] counts what the call
        enqueued.  The fingerprint does NOT cover the networks and the statistics: a blob from a server with other weights is
        taken, and what the stream then does is the caller's business."""
        info = snapshot_info(blob)
        version = ops.lib().zeggs_live_snapshot_version()
        if info["version"] != version:
            raise ValueError(f"LiveServer.restore: the blob was written by snapshot version {info['version']}, this library is version {version}")
        snapshot_check_fingerprint(info["fingerprint"], self._fingerprint())
        w, sec = info["row"], info["sections"]
        if not (0 <= w["base"] <= w["n"] and 0 <= w["fbase"] <= w["n_ring"] <= w["n_feat"] and w["kd"] >= 1 and w["n_feat"] - w["fbase"] <= self.FC
                and w["sent0"] in (0, 1) and w["rs"] in (0, 1) and w["rt"] in (0, 1) and w["fade"] >= 0):
            raise ValueError(f"LiveServer.restore: section 'row': counters {w} are not those of a stream of this server")
        if w["rt"] != int(self.retime_conf is not None) or (w["rt_half"] >= 0) != bool(self.retime_conf and "filter" in self.retime_conf):
            raise ValueError("LiveServer.restore: section 'row': its re-timing fields are not those of a stream of this server")
        r = self._free_row(needed=False) or 0            # (sizes do not depend on the row: a full server still checks them)
        pieces = self._snap_pieces(r, w["n"] - w["base"], w["n_feat"] - w["fbase"], bool(w["rs"]))
        J3 = 3 * len(self.frames_conf["parents"]) if self.frames_conf else 0
        if w["offsets_count"] != J3 or (J3 and w["offsets_itemsize"] not in (4, 8)):
            raise ValueError(f"LiveServer.restore: section 'offsets' holds {w['offsets_count']} values of {w['offsets_itemsize']} bytes, this server's "
                             f"skeleton asks for {J3}")
        host = dict(row=bytes(8 * len(SNAP_ROW)), offsets=bytes(J3 * w["offsets_itemsize"]))
        for name, nb in zip(SNAP_SECTIONS, self._snap_sizes(pieces, host)):
            if sec[name][1] != nb:
                raise ValueError(f"LiveServer.restore: section {name!r} has {sec[name][1]} bytes, this server's row takes {nb}")
        r = self._free_row()
        # ---- the host side of the row: tables by the functions open() uses (a refused rate or ratio raises before a row is taken)
        row = _Row(self._next_sid)
        row.n, row.base, row.n_feat, row.fbase, row.n_ring, row.kd = (w[k] for k in ("n", "base", "n_feat", "fbase", "n_ring", "kd"))
        row.sent0, row.k_style, row.fade = bool(w["sent0"]), w["k_style"], w["fade"]
        if w["rs"]:
            if w["rs_fmt"] not in ops.RS_FORMATS.values():
                raise ValueError(f"LiveServer.restore: section 'row': sample format {w['rs_fmt']}")
            if w["rs_fi"] != self.fs:
                audio.resample_ratio(w["rs_fi"], self.fs)
            row.rs = self._converter(w["rs_fi"], w["rs_fmt"], w["rs_n_in"])
        if w["rt"]:
            row.rt = self._retimed(self._fr, w["rt_L"], w["rt_M"], w["rt_n_in"], w["rt_n_out"], w["rt_half"])
            if w["rt_half"] > 0 and row.rt["half"] != w["rt_half"]:
                raise ValueError(f"LiveServer.restore: section 'row': half {w['rt_half']} at the ratio {w['rt_L']} / {w['rt_M']}, this server's filter has {row.rt['half']}")
        b = np.frombuffer(bytes(blob) if isinstance(blob, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blob, np.uint8), np.uint8)
        if J3:
            row.offsets = np.array(b[sec["offsets"][0]:sum(sec["offsets"])].view("<f8" if w["offsets_itemsize"] == 8 else "<f4")).reshape(-1, 3)
        n_ops = 0
        if w["n"] - w["base"] > self.window[r].numel():   # growth, the one exception, as in push()
            self.window[r] = torch.zeros(w["n"] - w["base"], device=self.dev)
            self.stats["window_capacity"][r] = int(self.window[r].numel())
            n_ops += 1
        pieces = self._snap_pieces(r, w["n"] - w["base"], w["n_feat"] - w["fbase"], bool(w["rs"]))
        n_seg = sum(1 for v in pieces.values() for _, nb in v if nb)
        o_blob = (n_seg * C.sizeof(ops.SnapSeg) + 63) // 64 * 64
        stg = self._snap_stage()
        blk = stg.take(o_blob + b.size)
        segs, j = (ops.SnapSeg * n_seg).from_buffer(blk, 0), 0
        for name in SNAP_SECTIONS:
            o = sec[name][0]
            for addr, nb in pieces.get(name, ()):
                if nb:
                    segs[j].src, segs[j].dst_offset, segs[j].bytes = addr, o, nb
                    j += 1
                o += _a16(nb)
        assert j == n_seg
        blk[o_blob:o_blob + b.size] = b
        with torch.no_grad():
            stg.upload(0, o_blob + b.size)
            ops.live_unpack(segs, n_seg, stg.dev.data_ptr(), stg.dev.data_ptr() + o_blob, b.size)
            n_ops += 2
        del segs
        sid = row.sid
        self._next_sid += 1
        self._rows[r], self._sids[sid] = row, r
        self.stats["ops_last_restore"] = n_ops
        return sid
