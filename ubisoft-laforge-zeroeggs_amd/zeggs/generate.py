"""generate_gesture(): the reference's inference entry point on the HIP engine.

Same signature, file layout and return value as ZEGGS/generate.py:22-411.  Host side: file I/O, style blending.
Device side (HIP kernels): exemplar feature extraction, BVH channel conversion, mel front-end, speech encoder, style encoder + VAE,
autoregressive decoder rollout (no-grad ring-buffer path).  `use_script` is accepted and ignored (TorchScript cannot
wrap the C-ABI calls; every shipped config sets it to false).
"""
import json
import pathlib
from pathlib import Path
from shutil import copyfile

import numpy as np
import torch
from scipy.io import wavfile

from . import anim, audio, compat

PROFILE = None      # bench.py sets this to a dict: generate_gesture() then adds the wall-clock ms of each stage to it (device
                    # stages bracketed by a synchronisation -- measurement only, the default path never synchronises for it)


class _stage:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if PROFILE is not None:
            import time
            torch.cuda.synchronize()
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if PROFILE is not None:
            import time
            torch.cuda.synchronize()
            PROFILE[self.name] = PROFILE.get(self.name, 0.0) + (time.perf_counter() - self.t0) * 1e3


def split_by_ratio(length, ratio):
    """integer frame splits of the "stitch" blend (reference helpers.py:26-37: truncation, last end = length)"""
    assert sum(ratio) == 1.0
    out, prev = [], 0
    for r in ratio:
        s, e = int(prev), int(prev + r * length)
        out.append([s, e])
        prev = e
    out[-1][-1] = length
    return out


def read_wav_mono16k(path):
    """16 kHz WAV -> float32 in [-1, 1) (the reference rescales int PCM the same way; other formats would need SoX)"""
    fs, x = wavfile.read(str(path))
    if fs != 16000:
        raise ValueError(f"{path}: expected a 16 kHz wav (got {fs} Hz); resample offline")
    if x.ndim > 1:
        x = x.mean(axis=1)
    if np.issubdtype(x.dtype, np.integer):
        scale = float(np.iinfo(x.dtype).max + 1)          # a power of two: multiplying by its reciprocal is the same division, exactly
        x = x.astype(np.float32)
        np.multiply(x, np.float32(1.0 / scale), out=x)    # (one pass over the 115 MB of a 30-minute clip instead of three)
    return fs, x if x.dtype == np.float32 else x.astype(np.float32)


def _example_features(p):
    """feature rows [F, 1134] of an exemplar clip (gaze slot zero), as in generate.py:229-248 (device tensors)"""
    root_pos, root_rot, root_vel, root_vrt, lpos, lrot, ltxy, lvel, lvrt = p[:9]
    n = len(root_vel)
    cols = [root_vel, root_vrt, lpos, ltxy, lvel, lvrt]
    return torch.cat([c.reshape(n, -1).to(torch.float32) for c in cols] +
                     [torch.zeros(n, 3, dtype=torch.float32, device=root_vel.device)], dim=1)


STREAM_MIN_FRAMES = 20000     # clips longer than this are decoded chunk by chunk with the BVH text written meanwhile
STREAM_CHUNK = 8192
STREAM_BLOCK = 512            # rows per formatting task (host threads; anim.TEXT = "host" only)


def _decode_to_bvh_streaming(decoder, pose0, rpos0, rrot0, gaze_row, speech, style, stats, dt, path, parents, names,
                             chunk=None, block=None, threads=None, plant=None):
    """Long clips (configs[4]: 108 000 frames): the B = 1 rollout runs as a sequence of persistent launches of `chunk` frames,
    each resumed from the state of the one before (zeggs_decoder_fwd_state_ex); behind every chunk its frames are converted to
    the rows of the BVH motion block ON THE DEVICE (zeggs_pose_to_bvh_table) and formatted there (zeggs_table_text_device: what
    comes down on the copy streams into pinned memory is the file content; anim.TEXT = "host": the float64 rows come down and
    host threads format them, zeggs_format_table_text) WHILE the next chunks are being decoded -- _TextStaging; this thread writes
    the text in order.  Same file as the one-launch path (decoder -> bvh_channels -> write_bvh_channels) up to the fp32
    re-association at the chunk boundaries (joint rotations a few hundredths of a degree apart after 700 free-running frames):
    tests/test_gpu_parity.py::test_generate_gesture_streaming_writer_equals_one_launch.  The decoder's frames are not kept
    (488 MB for 30 minutes).  Give-ups of the persistent kernel are collected in one status word that is looked at ONCE, after
    the last chunk: then everything is redone on the stage launches.
    `plant` (the options of anim.plant_feet): every chunk's rows go through the planting stage between the decoder and the
    conversion, the chains' contact state carried from chunk to chunk (anim.plant_stage); the decoder resumes from its raw rows."""
    import time as _t0
    from concurrent.futures import ThreadPoolExecutor
    from . import ops
    t_enter = _t0.perf_counter()
    chunk, block = chunk or STREAM_CHUNK, block or STREAM_BLOCK
    dev = speech.device
    T = speech.shape[1]
    J = len(parents)
    in_mean, in_std, out_mean, out_std = stats
    L = ops.api()
    cols = 3 + 3 * J
    # frame 0 is the given first pose: its joint positions are the OFFSETs of the file (utils.write_bvh: offsets = positions[0])
    sl = lambda a, b: pose0[:, a:b]  # noqa: E731
    pos0, _ = anim.bvh_channels(rpos0, rrot0, sl(6, 6 + 3 * J).reshape(1, J, 3), sl(6 + 3 * J, 6 + 9 * J).reshape(1, J, 2, 3),
                                np.array([0, 0, 0]), np.array([1, 0, 0, 0]))
    head, seq = anim.bvh_header(pos0[0].cpu().numpy(), parents, names, "zyx", T, dt)
    seq_dev = torch.as_tensor(np.asarray(seq, np.int32), device=dev)
    d = anim.BvhDims(0, J, 1)
    d.start_pos[:] = [0.0, 0.0, 0.0]
    d.start_rot[:] = [1.0, 0.0, 0.0, 0.0]
    ref_pos, ref_rot = rpos0.to(torch.float32).contiguous(), rrot0.to(torch.float32).contiguous()
    status = ops.new_status(dev)
    main = torch.cuda.current_stream()

    # the last chunk is what nothing hides: its rows are converted, downloaded, formatted (36 us of host time per row: 18 ms for
    # a 512-row task) and written AFTER the decode has ended -- so it is short and its formatting tasks are small
    # (with the device text a pool thread only waits for a chunk's row ends and issues its sized copy: two are plenty)
    workers = threads or (2 if anim.TEXT == "device" else min(16, (__import__("os").cpu_count() or 4)))
    tail_rows = max(1, min(chunk // 16, 512))
    RING = 4                                             # pinned staging buffers in flight (page-locking 15 MB costs ~5 ms: not per chunk)
    stage = _TextStaging(dev, RING, min(chunk, T) + 1, cols)

    marks = []

    def run(pool, fh):
        """decode chunk by chunk; chunk c's text is written while chunks c + 1 .. c + RING - 1 are queued on the device"""
        stage.pool = pool
        pending = []                                     # per chunk in flight: the getters of its text, in row order
        planting = None if plant is None else anim.plant_stage(parents, names, dt, dev, **plant)      # (a redo starts afresh)
        state = (pose0, rpos0, rrot0, None)
        k = 0                                            # last frame produced so far

        def drain(keep):
            while len(pending) > keep:
                for get in pending.pop(0):
                    fh.write(get())
        while True:
            n = min(chunk, T - 1 - k)                    # new frames of this chunk
            if n == T - 1 - k and n > tail_rows:         # the LAST chunk is short: what follows the end of the decode is only its
                n -= tail_rows                           # conversion, download and formatting (the pipeline's tail)
            sp, sty = speech[:, k:k + n + 1], style[:, k:k + n + 1]
            gz = gaze_row.expand(n + 1, 3)[None]
            if n > 0:
                pose, rpos, rrot, h = ops.decoder_chunk(decoder, state[0], state[1], state[2], gz, sp, sty, in_mean, in_std,
                                                        out_mean, out_std, dt, h_in=state[3], status=status)
                state = (pose[:, -1], rpos[:, -1], rrot[:, -1], h)
            else:                                        # a one-frame clip
                pose, rpos, rrot = pose0[:, None], rpos0[:, None], rrot0[:, None]
            lo = 0 if k == 0 else 1                      # (frame 0 of a later chunk was written with the chunk before)
            rows = n + 1 - lo
            table = torch.empty(rows, cols, dtype=torch.float64, device=dev)
            d.T = rows
            # (named, not temporaries: a tensor freed between two argument expressions hands its block to the next one)
            P = pose[0, lo:]
            a_rpos, a_rrot = rpos[0, lo:].contiguous(), rrot[0, lo:].contiguous()
            if planting is not None:                     # feet that stay planted: the conversion reads the corrected rows
                P = anim.plant_feet(P, a_rpos, a_rrot, parents, names, dt, stage=planting)[0]
            a_lpos, a_ltxy = P[:, 6:6 + 3 * J].contiguous(), P[:, 6 + 3 * J:6 + 9 * J].contiguous()
            L.zeggs_pose_to_bvh_table(d, a_rpos, a_rrot, a_lpos, a_ltxy, ref_pos, ref_rot, seq_dev, table, main.cuda_stream)
            del a_rpos, a_rrot, a_lpos, a_ltxy
            drain(RING - 1)                              # the staging buffer of chunk c - RING has been written
            last = n == 0 or k + n >= T - 1
            blk = block if not last else max(16, -(-rows // (2 * workers)))
            pending.append(stage.submit(table, [(0, rows)], blk)[0])
            k += n
            if n == 0 or k >= T - 1:
                break
        marks.append(_t0.perf_counter())                 # everything is enqueued
        drain(0)
        marks.append(_t0.perf_counter())                 # ... decoded, converted, downloaded, formatted and written

    try:      # (the ring goes back to the pool whatever happens in between: ADVICE r5)
        import time as _t
        t_setup = _t.perf_counter()
        with ThreadPoolExecutor(max_workers=workers) as pool:
            with open(path, "wb") as fh:
                fh.write(head.encode())
                run(pool, fh)
                t_run = _t.perf_counter()
            t_close = _t.perf_counter()
            if PROFILE is not None:
                PROFILE["  streaming_writer_breakdown_ms"] = {
                    "setup": round((t_setup - t_enter) * 1e3, 2), "enqueue_all_chunks": round((marks[0] - t_setup) * 1e3, 2),
                    "last_chunks_decoded_formatted_written": round((marks[1] - marks[0]) * 1e3, 2), "file_close": round((t_close - t_run) * 1e3, 2)}
            if ops._persistent_live(0) and int(status[0].item()):     # (every chunk has been downloaded by now: no extra wait)
                ops._warn_gave_up(int(status[0].item()), "the whole rollout")
                # redo on the stage launches -- for THIS call only: the process-wide switch is restored afterwards (a
                # give-up here used to turn the persistent decode off for every later caller without a word)
                was = ops._OPTIONS.get("persistent", 1)
                ops.set_option("persistent", 0)
                try:
                    ops.fill_(status.view(torch.float32))
                    with open(path, "wb") as fh:
                        fh.write(head.encode())
                        run(pool, fh)
                finally:
                    ops.set_option("persistent", was)
    finally:
        stage.release()


_PINNED = {}                      # (count, cols, dtype) -> list of free rings: a ring is CHECKED OUT for the duration of one call
_PINNED_LOCK = __import__("threading").Lock()


def _pinned_ring(count, rows, cols, dtype=torch.float64):
    """`count` page-locked staging buffers [rows, cols] (float64 table rows for the host formatter, uint8 text bytes and int64 row
    ends for the device one).  Page-locking is the expensive part (4 x 15 MB for the default chunk), so rings are pooled for the
    life of the process -- but a ring belongs to ONE call at a time (two generate_gesture() calls on two threads shared
    the buffers and corrupted each other's rows): take one with this function, give it back with _pinned_release()."""
    key = (count, cols, dtype)
    with _PINNED_LOCK:
        free = _PINNED.setdefault(key, [])
        for i, ring in enumerate(free):
            if min(b.shape[0] for b in ring) >= rows:
                return free.pop(i)
    return [torch.empty(rows, cols, dtype=dtype).pin_memory() for _ in range(count)]


def _pinned_release(ring):
    """Back to the pool -- which keeps ONE free ring per (count, cols, dtype), the largest: a smaller one can serve nobody the larger
    cannot, and page-locked memory that only accumulates with varying clip / chunk sizes is memory the system cannot page."""
    with _PINNED_LOCK:
        free = _PINNED.setdefault((len(ring), ring[0].shape[1], ring[0].dtype), [])
        free.append(ring)
        free.sort(key=lambda r: -min(b.shape[0] for b in r))
        del free[1:]


class _TextStaging:
    """What one writer call (streaming or batch) needs to turn device tables into text underneath the decode: the copy streams, the
    pinned rings (checked out for this call) and the two ways to the bytes.
      anim.TEXT = "device": the table is formatted on `main` behind the kernel that made it (anim.table_text_device); the row ends
        and the status word come down on the copy stream (8 bytes per row); ONE pool task per table waits for them, issues the copy
        of exactly row_end[-1] bytes into the pinned byte ring (grown when a table's text is longer than the slot) and hands out
        memoryviews cut at the spans.  The task holds the table until the status word has been read: a value outside the digit
        routine's domain sends the table through the host formatter (anim._host_pieces).
      anim.TEXT = "host": the table comes down as float64 and pool tasks format blocks of rows (anim.format_rows), as before.
    submit() -> per span a list of callables, each returning the next bytes of that span once they are there."""
    TEXT_ROW = 12            # bytes per number the byte ring starts with ("-123.456789 "); the bound is 24: slots grow on demand

    def __init__(self, dev, count, rows, cols):
        self.pool, self.count, self.used = None, count, 0      # (pool: the caller's thread pool, set before submit)
        self.device_text = anim.TEXT == "device"
        self.main = torch.cuda.current_stream()
        self.copy_stream = torch.cuda.Stream(device=dev)
        if self.device_text:
            self.text_stream = torch.cuda.Stream(device=dev)      # (the sized copies: never behind the next chunk's row ends)
            self.rings = [_pinned_ring(count, rows, cols * self.TEXT_ROW + 1, torch.uint8), _pinned_ring(count, rows + 1, 1, torch.int64)]
        else:
            self.rings = [_pinned_ring(count, rows, cols)]

    def release(self):
        for ring in self.rings:
            _pinned_release(ring)

    def submit(self, table, spans, block):
        """table [rows, cols] float64 made on `main`; spans [(first row, rows), ...] in row order, covering it.  The caller has
        drained the slot used `count` submissions ago."""
        rows = table.shape[0]
        slot = self.used % self.count
        self.used += 1
        if not self.device_text:
            done = torch.cuda.Event()
            done.record(self.main)
            host = self.rings[0][slot][:rows]
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(done)
                host.copy_(table, non_blocking=True)
                table.record_stream(self.copy_stream)
                ev = torch.cuda.Event()
                ev.record(self.copy_stream)

            def fmt(a, b):
                ev.synchronize()
                return anim.format_rows(host[a:b].numpy())
            return [[self.pool.submit(fmt, a, min(a + block, s0 + n)).result for a in range(s0, s0 + n, block)] for s0, n in spans]
        text, meta = anim.table_text_device(table)
        done = torch.cuda.Event()
        done.record(self.main)
        meta_h = self.rings[1][slot][:rows + 1, 0]
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(done)
            meta_h.copy_(meta, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        bounds = [s0 for s0, _ in spans] + [rows]

        def fetch(keep=(table, text, meta)):      # (the device buffers live until their bytes are on the host: the copies run on
            ev.synchronize()                      #  other streams than the one the allocator hands their blocks out on)
            m = meta_h.numpy()
            if int(m[rows]) & 0xFFFFFFFF:
                return anim._host_pieces(table, bounds)
            total = int(m[rows - 1])
            ring = self.rings[0]
            if ring[slot].numel() < total:
                width = ring[slot].shape[1]
                ring[slot] = torch.empty(-(-(total + total // 4) // width), width, dtype=torch.uint8).pin_memory()
            flat = ring[slot].view(-1)[:total]
            with torch.cuda.stream(self.text_stream):
                flat.copy_(text[:total], non_blocking=True)
                got = torch.cuda.Event()
                got.record(self.text_stream)
            got.synchronize()
            view = memoryview(flat.numpy())
            end = lambda r: int(m[r - 1]) if r else 0  # noqa: E731
            return [view[end(a):end(b)] for a, b in zip(bounds[:-1], bounds[1:])]
        fut = self.pool.submit(fetch)
        return [[lambda i=i: fut.result()[i]] for i in range(len(spans))]


class _Loaded:
    """what a call needs from disk besides the job itself: data definition, statistics and the networks, loaded ONCE"""

    def __init__(self, network_path, data_path, style_encoding_type, device):
        network_path, data_path = Path(network_path), Path(data_path)
        self.device = device
        with open(data_path / "data_pipeline_conf.json") as f:
            self.pipe_conf = json.load(f)
        with open(data_path / "data_definition.json") as f:
            details = json.load(f)
        self.nlabels, self.label_names, self.bone_names = len(details["label_names"]), details["label_names"], details["bone_names"]
        self.parents, self.dt = np.asarray(details["parents"]), details["dt"]
        stat = np.load(data_path / "stats.npz")
        tt = lambda k: torch.as_tensor(np.asarray(stat[k]), dtype=torch.float32, device=device)  # noqa: E731
        self.audio_mean, self.audio_std = tt("audio_input_mean"), tt("audio_input_std")
        self.stats = (tt("anim_input_mean"), tt("anim_input_std"), tt("anim_output_mean"), tt("anim_output_std"))
        if (network_path / "decoder.pt").exists():      # the reference's whole-module pickles
            self.speech_net = compat.load_module(network_path / "speech_encoder.pt", device).to(device).eval()
            self.decoder = compat.load_module(network_path / "decoder.pt", device).to(device).eval()
            self.style_net = None
            if style_encoding_type == "example":
                self.style_net = compat.load_module(network_path / "style_encoder.pt", device).to(device).eval()
        else:                                           # pickle-free twin written by zeggs.train (safetensors + arch.json)
            speech_net, decoder, style_net, _ = compat.load_state(network_path, device)
            self.speech_net, self.decoder = speech_net.eval(), decoder.eval()
            self.style_net = style_net.eval() if style_net is not None else None
            assert self.style_net is not None or style_encoding_type != "example", "checkpoint has no style encoder"
        self.film = hasattr(self.decoder.recurrent_decoder, "gammas_predictor")


def _style_mirrored(style):
    """a style entry (bvh, frames) or (bvh, frames, "mirror")"""
    if len(style) > 2 and style[2] not in (None, False):
        if style[2] not in ("mirror", True):
            raise ValueError(f"style entry {style!r}: the third field is 'mirror' (or absent)")
        return True
    return False


def _seed_all(seed):
    from . import ops
    np.random.seed(seed)
    torch.manual_seed(seed)
    ops.manual_seed(seed)       # the VAE noise comes from the library's counter-hash stream: the same seed gives the same clip,
                                # as `torch.manual_seed(seed)` does for the reference's randn_like (generate.py:86-87)


def _front_end(ld, audio_file, styles, style_encoding_type, blend_type, blend_ratio, file_name, first_pose, temperature,
               cache=None, mirror_style=False):
    """Everything of generate_gesture() in front of the decoder: WAV read, loudness + mel, speech encoder, exemplar parse, style
    encoder, blend.  -> dict(final, speech, feat, file_name).  `cache` (generate_gestures: a dict shared by the jobs of a list)
    keeps parsed BVH files and exemplar features across calls; without it files are parsed on a host thread beside the audio
    front-end, every distinct file once per call.  An exemplar entry (bvh, frames, "mirror"), or every exemplar with
    `mirror_style`, is reflected left/right after loading and before the features (anim.mirror_take)."""
    device = ld.device
    in_mean, in_std = ld.stats[0], ld.stats[1]
    # exemplar / first-pose BVH files are parsed on a host thread (the C parser releases the GIL) while this thread reads the WAV
    # and enqueues the audio front-end: every distinct file once
    from concurrent.futures import ThreadPoolExecutor
    bvh_paths = [str(Path(s_[0])) for s_ in styles
                 if style_encoding_type == "example" and isinstance(s_, (tuple, list)) and isinstance(s_[0], (pathlib.PurePath, str))]
    if audio_file is not None and isinstance(first_pose, (pathlib.PurePath, str)):
        bvh_paths.append(str(Path(first_pose)))
    clips = cache.setdefault("clips", {}) if cache is not None else None
    if clips is not None:
        bvh_paths = [p_ for p_ in bvh_paths if p_ not in clips]
    loader = ThreadPoolExecutor(max_workers=1) if (audio_file is not None and bvh_paths) else None
    loading = {}
    if loader is not None:
        for pth in dict.fromkeys(bvh_paths):
            loading[pth] = loader.submit(anim.bvh_load, pth)
        loader.shutdown(wait=False)

    def load_bvh(pth):
        """parsed clip of a BVH path (a private copy: callers trim / modify it)"""
        key = str(Path(pth))
        if clips is not None and key in clips:
            clip = clips[key]
        else:
            fut = loading.get(key)
            clip = fut.result() if fut is not None else anim.bvh_load(pth)
            if clips is not None:
                clips[key] = clip
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in clip.items()}

    speech, n_frames = None, None
    if audio_file is not None:
        with _stage("wav_read_host"):
            _, wav = read_wav_mono16k(audio_file)
        n_frames = audio.n_anim_frames(len(wav))
        with _stage("loudness+mel_device"):
            feats = audio.preprocess_audio_device(wav, 60, n_frames, ld.pipe_conf["audio_conf"],
                                                  ld.pipe_conf["audio_feature_type"], device)
        with _stage("speech_encoder_device"):
            speech = ld.speech_net(((feats[None] - ld.audio_mean) / ld.audio_std).contiguous())

    encodings, feat = [], None
    anim_name = "style"
    parsed = cache.setdefault("feats", {}) if cache is not None else {}   # exemplar files already parsed: (path, trim) -> feature arrays
    for style in styles:
        if style_encoding_type == "example":
            if isinstance(style[0], (pathlib.PurePath, str)):
                anim_name = Path(style[0]).stem
                mirrored = bool(mirror_style) or _style_mirrored(style)
                fkey = (str(Path(style[0]).resolve()), None if style[1] is None else tuple(style[1])) + (("mirror",) if mirrored else ())
                if cache is not None and fkey in parsed:
                    feat = parsed[fkey]
                else:
                    with _stage("exemplar_bvh_parse_host"):
                        clip = load_bvh(style[0])
                    if style[1] is not None:
                        clip["rotations"] = clip["rotations"][style[1][0]:style[1][1]]
                        clip["positions"] = clip["positions"][style[1][0]:style[1][1]]
                    assert int(np.ceil(1 / clip["frametime"])) == 60
                    if mirrored:
                        clip = anim.mirror_take(clip)
                    with _stage("exemplar_features_device"):
                        feat = anim.preprocess_animation(clip, device)
                        parsed[fkey] = feat
                with _stage("exemplar_features_device"):
                    ex = (_example_features(feat) - in_mean) / in_std
                with _stage("style_encoder_device"):
                    z, _, _ = ld.style_net(ex[None].contiguous(), temperature)
                encodings.append(z)
            elif isinstance(style[0], np.ndarray):
                if mirror_style or (len(style) > 2 and style[2] not in (None, False)):
                    raise ValueError("a style entry (embedding, name) cannot be mirrored: mirror reflects an exemplar's BVH channels, "
                                     "an embedding has none")
                anim_name = style[1]
                encodings.append(torch.as_tensor(style[0], dtype=torch.float32, device=device)[None])
        elif style_encoding_type == "label":
            onehot = torch.zeros((1, ld.nlabels), device=device)
            onehot[0, ld.label_names.index(style)] = 1.0
            encodings.append(onehot)
            anim_name = style
            assert first_pose is not None
        else:
            raise ValueError("Unknown style encoding type")

    if blend_type == "stitch" and len(encodings) > 1:
        if audio_file is None:
            final = encodings
        else:
            assert len(styles) == len(blend_ratio)
            se = split_by_ratio(n_frames, blend_ratio)
            final = torch.cat([z.unsqueeze(1).repeat(1, e - s, 1) for z, (s, e) in zip(encodings, se)], dim=1)
    elif blend_type == "add" and len(encodings) > 1:
        assert len(encodings) == len(blend_ratio)
        final = torch.matmul(torch.stack(encodings, dim=1).transpose(2, 1),
                             torch.tensor(blend_ratio, device=device, dtype=torch.float32))
    else:
        final = encodings[0]

    if audio_file is not None:
        if first_pose is not None:
            key = (str(Path(first_pose).resolve()), None) if isinstance(first_pose, (pathlib.PurePath, str)) else None
            if key in parsed:       # the first pose is an (untrimmed) style exemplar: parsed already
                feat = parsed[key]
            else:
                with _stage("first_pose_bvh_parse_host"):
                    clip = load_bvh(first_pose) if key is not None else dict(first_pose)
                with _stage("first_pose_features_device"):
                    feat = anim.preprocess_animation(clip, device)
                if cache is not None and key is not None:
                    parsed[key] = feat
        if final.dim() == 2:
            final = final.unsqueeze(1).repeat(1, speech.shape[1], 1)
        if file_name is None:
            file_name = f"audio_{Path(audio_file).stem}_label_{anim_name}"
    return dict(final=final, speech=speech, feat=feat, file_name=file_name)


def _first_frame(feat):
    """-> pose0 [1,PO], rpos0 [1,3], rrot0 [1,4], gaze [1,3] of the frame a clip starts from"""
    g = lambda a: a[0:1].to(torch.float32).contiguous()  # noqa: E731
    root_pos, root_rot, root_vel, root_vrt, lpos, lrot, ltxy, lvel, lvrt = feat[:9]
    pose0 = torch.cat([g(x).reshape(1, -1) for x in (root_vel, root_vrt, lpos, ltxy, lvel, lvrt)], dim=1)
    return pose0, g(root_pos), g(root_rot), g(feat[14])


def _decode_one(ld, fe, audio_file, results_path, return_poses=False, plant=None):
    """decoder rollout of ONE clip (B = 1) + BVH / WAV files: the tail of generate_gesture().  `plant`: the options of
    anim.plant_feet (None: off) -- the planting stage between the decoder and the BVH conversion, on both paths"""
    in_mean, in_std, out_mean, out_std = ld.stats
    decoder, dt, parents, bone_names = ld.decoder, ld.dt, ld.parents, ld.bone_names
    speech, final, feat, file_name = fe["speech"], fe["final"], fe["feat"], fe["file_name"]
    g = lambda a: a[0:1].to(torch.float32).contiguous()  # noqa: E731
    root_pos, root_rot, root_vel, root_vrt, lpos, lrot, ltxy, lvel, lvrt = feat[:9]
    gaze_pos = feat[14]
    T = speech.shape[1]
    if T > STREAM_MIN_FRAMES and not ld.film and not return_poses:
        # long clip: chunked persistent decode with the BVH text formatted and written underneath it
        pose0 = torch.cat([g(x).reshape(1, -1) for x in (root_vel, root_vrt, lpos, ltxy, lvel, lvrt)], dim=1)
        # the WAV copy runs beside the decode; its errors surface where the one-launch path's do (a bare Thread
        # sent a PermissionError to threading.excepthook instead of the `except` below)
        from concurrent.futures import ThreadPoolExecutor as _TPE
        with _TPE(max_workers=1) as copy_pool:
            try:
                copier = copy_pool.submit(copyfile, audio_file, str(results_path / (file_name + ".wav")))
                with _stage("decode+pose_to_bvh_device_with_bvh_text_write_host_underneath"):
                    _decode_to_bvh_streaming(decoder, pose0, g(root_pos), g(root_rot), g(gaze_pos), speech,
                                             final.contiguous(), (in_mean, in_std, out_mean, out_std), dt,
                                             str(results_path / (file_name + ".bvh")), parents, bone_names, plant=plant)
                copier.result()
            except (PermissionError, OSError) as e:
                print(e)
        return None
    gaze = g(gaze_pos).repeat(T, 1)[None]
    with _stage("decode_device"):
        out = decoder(g(root_pos), g(root_rot), g(root_vel), g(root_vrt), g(lpos), g(ltxy), g(lvel), g(lvrt),
                      gaze.contiguous(), speech, final.contiguous(), None, in_mean, in_std, out_mean, out_std, dt)
    V_root_pos, V_root_rot, _, _, V_lpos, V_ltxy = out[0], out[1], out[2], out[3], out[4], out[5]
    if plant is not None:                                # feet that stay planted: the decoded rows through the stage, whole
        with _stage("plant_feet_device"):
            J = V_lpos.shape[2]
            rows = torch.cat([o[0].reshape(T, -1) for o in out[2:8]], dim=1)
            rows = anim.plant_feet(rows, V_root_pos[0], V_root_rot[0], parents, bone_names, dt, **plant)[0]
            V_lpos, V_ltxy = rows[None, :, 6:6 + 3 * J].reshape(1, T, J, 3), rows[None, :, 6 + 3 * J:6 + 9 * J].reshape(1, T, J, 2, 3)
    try:
        with _stage("pose_to_bvh_device"):
            channels = anim.bvh_channels(V_root_pos[0], V_root_rot[0], V_lpos[0], V_ltxy[0], np.array([0, 0, 0]),
                                         np.array([1, 0, 0, 0]))
        with _stage("bvh_text_write_host"):
            anim.write_bvh_channels(str(results_path / (file_name + ".bvh")), *channels, parents=parents,
                                    names=bone_names, order="zyx", dt=dt)
        with _stage("wav_copy_host"):
            copyfile(audio_file, str(results_path / (file_name + ".wav")))
    except (PermissionError, OSError) as e:
        print(e)
    return (V_root_pos[0], V_root_rot[0], V_lpos[0], V_ltxy[0]) if return_poses else None


def generate_gesture(audio_file, styles, network_path, data_path, results_path, style_encoding_type="example",
                     blend_type="add", blend_ratio=[0.5, 0.5], file_name=None, first_pose=None, temperature=1.0,
                     seed=1234, use_gpu=True, use_script=False, plant=None, mirror_style=False):
    """the reference's generate_gesture.  A style entry (bvh, frames, "mirror") -- or every exemplar, with `mirror_style` (not the
    reference's) -- is used as its left/right reflection: the exemplar's channels are mirrored after loading, before the
    features; nothing else changes.  `plant` (not the reference's): None, True or dict(chains="auto", speed=(v_on, v_off),
    height=(h_on, h_off), ground, slack, release, stretch) -- feet that stay planted (anim.plant_feet): the decoded
    rows go through the contact lock and the leg IK on the device before they become the BVH file, on the one-launch path and
    on the chunked long-clip path (the contact state carried from chunk to chunk).  The defaults are NOT tuned on captured
    motion.  ValueError before anything is decoded for options or chains the skeleton does not have."""
    network_path, data_path = Path(network_path), Path(data_path)
    if results_path is not None:
        results_path = Path(results_path)
        results_path.mkdir(exist_ok=True)
    assert (audio_file is None) == (results_path is None)
    if not (use_gpu and torch.cuda.is_available()):
        raise RuntimeError("the ZeroEGGS MI355X engine has no CPU path (use_gpu=False / no GPU visible)")
    _seed_all(seed)
    ld = _Loaded(network_path, data_path, style_encoding_type, torch.device("cuda"))
    if plant is not None and plant is not False:
        from . import ops
        ops.plant_options(plant, ld.parents, ld.bone_names)          # (checked here, ahead of the front end)
        plant = {} if plant is True else dict(plant)
    else:
        plant = None
    with torch.no_grad():
        fe = _front_end(ld, audio_file, styles, style_encoding_type, blend_type, blend_ratio, file_name, first_pose, temperature,
                        mirror_style=mirror_style)
        if audio_file is not None:
            _decode_one(ld, fe, audio_file, results_path, plant=plant)
    return fe["final"]


# ----------------------------------------------------------------------------- many clips per decode
def plan_slots(lengths, batch, chunk):
    """Slot plan of the batch decode: clips of `lengths` frames (frame 0 = the given first pose, frames 1 .. L-1 are generated)
    on `batch` rows, decoded in chunks of at most `chunk` frames (frame 0 of a chunk = the last frame already produced, so a
    chunk yields at most chunk - 1 new frames per row).  -> one list per chunk of pieces (row, clip, start, count): row `row`
    starts from frame `start` of clip `clip` and produces frames start + 1 .. start + count (a piece with start == 0 also
    delivers the given frame 0).  Clips enter in job order as rows free up; a row whose clip ends inside a chunk idles until the
    next boundary; a one-frame clip is a piece with count == 0.  The launch length of a chunk is max(4, max count + 1): shorter
    rows are padded and their surplus frames discarded (the sweep needs 4 frames)."""
    batch, chunk = int(batch), int(chunk)
    if batch < 1 or chunk < 4:
        raise ValueError("plan_slots: batch >= 1 and chunk >= 4")
    lengths = [int(n) for n in lengths]
    if any(n < 1 for n in lengths):
        raise ValueError("plan_slots: every clip has at least its first frame")
    rows = [None] * batch            # per row: [clip, last frame produced]
    nxt, chunks = 0, []
    while True:
        pieces = []
        for r in range(batch):
            if rows[r] is None and nxt < len(lengths):
                rows[r] = [nxt, 0]
                nxt += 1
            if rows[r] is not None:
                clip, k = rows[r]
                n = min(chunk - 1, lengths[clip] - 1 - k)
                pieces.append((r, clip, k, n))
                rows[r] = [clip, k + n] if k + n < lengths[clip] - 1 else None
        if not pieces:
            return chunks
        chunks.append(pieces)


class Job:
    """one row of a job list: the arguments of generate_gesture() that vary per clip"""

    def __init__(self, audio_file, styles, file_name=None, first_pose=None, temperature=1.0, seed=1234, blend_type="add",
                 blend_ratio=(0.5, 0.5), mirror_style=False):
        self.audio_file, self.styles, self.file_name, self.first_pose = audio_file, list(styles), file_name, first_pose
        self.mirror_style = bool(mirror_style)
        self.temperature, self.seed, self.blend_type, self.blend_ratio = temperature, seed, blend_type, list(blend_ratio)


BATCH_RING = 4          # chunks whose rows are being downloaded / formatted while the next ones are decoded


def decode_plan(bd, firsts, speech, style, plan, status=None, fill=0.0, infos=None):
    """Run a slot plan (plan_slots) on the batch decode `bd` (ops.BatchDecode).  Per clip j: firsts[j] = (pose0 [1,PO], rpos0 [1,3],
    rrot0 [1,4], gaze target [1,3]) of its frame 0, speech[j] [L_j,SP], style[j] [L_j,ST].  A generator: per chunk it yields
    (pieces, pose [B,N,PO], rpos [B,N,3], rrot [B,N,4]); row r of a piece (r, j, start, count) holds frames start .. start + count
    of clip j at indices 0 .. count (index 0 = the frame the chunk started from).  Rows that begin a clip take their state from
    the CellStateEncoder (ops.decoder_state_init); `fill` is what idle rows and the frames past a row's last valid one hold
    (anything on the sweep: rows are independent and a row's frames past its last valid one do not reach it; a chunk that is
    redone on the stage launches is redone with non-finite inputs replaced by 0, see ops.decoder_batch_chunk).  `infos` (a list) receives one dict per decoded chunk (ops.decoder_batch_chunk's info)."""
    from . import ops
    dev = speech[0].device
    B, H = bd.B, bd.H
    SP, ST, PO = speech[0].shape[1], style[0].shape[1], firsts[0][0].shape[1]
    pose_l = torch.zeros(B, PO, device=dev)
    rpos_l = torch.zeros(B, 3, device=dev)
    rrot_l = torch.zeros(B, 4, device=dev)
    rrot_l[:, 0] = 1.0
    h = torch.zeros(2, B, H, device=dev)
    # a chunk's inputs are ONE gather each from the clips' rows laid end to end (+ a last row of `fill`), not three copies per row
    off = np.concatenate([[0], np.cumsum([int(x.shape[0]) for x in speech])]).astype(np.int64)
    sp_all = torch.cat(list(speech) + [torch.full((1, SP), fill, device=dev)])
    st_all = torch.cat(list(style) + [torch.full((1, ST), fill, device=dev)])
    gz_all = torch.cat([f[3] for f in firsts] + [torch.full((1, 3), fill, device=dev)])
    for pieces in plan:
        nmax = max(n for _, _, _, n in pieces)
        N = max(4, nmax + 1)
        new = [(r, j) for r, j, k, _ in pieces if k == 0]
        if new:              # rows that begin a clip: first pose and the CellStateEncoder's state
            idx = torch.as_tensor([r for r, _ in new], device=dev)
            p0 = torch.cat([firsts[j][0] for _, j in new])
            rp0 = torch.cat([firsts[j][1] for _, j in new])
            rr0 = torch.cat([firsts[j][2] for _, j in new])
            pose_l[idx], rpos_l[idx], rrot_l[idx] = p0, rp0, rr0
            if nmax > 0:
                gz0 = torch.cat([firsts[j][3] for _, j in new])
                st0 = torch.stack([style[j][0] for _, j in new])
                h[:, idx] = ops.decoder_state_init(bd, p0, rp0, rr0, gz0, st0)
        if nmax > 0:
            fidx = np.full((B, N), off[-1], np.int64)
            gidx = np.full((B, N), len(firsts), np.int64)
            for r, j, k, n in pieces:
                fidx[r, :n + 1] = off[j] + k + np.arange(n + 1)
                gidx[r, :n + 1] = j
            fidx, gidx = torch.as_tensor(fidx, device=dev), torch.as_tensor(gidx, device=dev)
            gz, sp, sty = gz_all[gidx], sp_all[fidx], st_all[fidx]
            info = {} if infos is not None else None
            pose, rpos, rrot, h = ops.decoder_batch_chunk(bd, pose_l, rpos_l, rrot_l, gz, sp, sty, h, status=status, info=info)
            if infos is not None:
                infos.append(info)
            # (a row that goes on fills its chunk: h is its state after frame start + count)
            ridx = torch.as_tensor([r for r, _, _, _ in pieces], device=dev)
            nidx = torch.as_tensor([n for _, _, _, n in pieces], device=dev)
            pose_l[ridx], rpos_l[ridx], rrot_l[ridx] = pose[ridx, nidx], rpos[ridx, nidx], rrot[ridx, nidx]
        else:                # only one-frame clips in this chunk
            pose, rpos, rrot = pose_l[:, None].clone(), rpos_l[:, None].clone(), rrot_l[:, None].clone()
        yield pieces, pose, rpos, rrot


def _decode_batch(ld, fes, paths, bd, batch, chunk, return_poses, threads=None, block=None):
    """The clips of `fes` on `batch` rows of the weight-stationary sweep (ops.decoder_batch_chunk), chunk by chunk through the slot
    plan; every (row, chunk) piece is converted to BVH motion rows on the device (zeggs_pose_to_bvh_table), a chunk's pieces share
    one table, which is formatted on the device and comes down as text cut at the pieces (anim.TEXT = "host": as float64 rows that
    host threads format) underneath the following chunks -- _TextStaging, the mechanism of _decode_to_bvh_streaming; this thread
    writes each clip's text in order.  `paths[j]` None: no file for clip j."""
    from concurrent.futures import ThreadPoolExecutor
    from . import ops
    dev = ld.device
    J, dt = len(ld.parents), ld.dt
    cols = 3 + 3 * J
    L = ops.api()
    firsts = [_first_frame(fe["feat"]) for fe in fes]
    speech = [fe["speech"][0] for fe in fes]
    style = [fe["final"].contiguous()[0] for fe in fes]
    lengths = [int(x.shape[0]) for x in speech]
    plan = plan_slots(lengths, batch, chunk)
    # per clip: header + channel order of its file (frame 0's joint positions are the OFFSETs: utils.write_bvh)
    heads, seqs = [], []
    for (pose0, rpos0, rrot0, _), n in zip(firsts, lengths):
        sl = lambda a, b: pose0[:, a:b]  # noqa: E731
        pos0, _r = anim.bvh_channels(rpos0, rrot0, sl(6, 6 + 3 * J).reshape(1, J, 3), sl(6 + 3 * J, 6 + 9 * J).reshape(1, J, 2, 3),
                                     np.array([0, 0, 0]), np.array([1, 0, 0, 0]))
        head, seq = anim.bvh_header(pos0[0].cpu().numpy(), ld.parents, ld.bone_names, "zyx", n, dt)
        heads.append(head)
        seqs.append(seq)
    seq_dev = torch.as_tensor(np.asarray(seqs[0], np.int32), device=dev)      # (the skeleton is the data definition's: one order)
    d = anim.BvhDims(0, J, 1)
    d.start_pos[:] = [0.0, 0.0, 0.0]
    d.start_rot[:] = [1.0, 0.0, 0.0, 0.0]
    main = torch.cuda.current_stream()
    status = ops.new_status(dev)
    workers = threads or (2 if anim.TEXT == "device" else min(16, (__import__("os").cpu_count() or 4)))
    block = block or STREAM_BLOCK
    stage = _TextStaging(dev, BATCH_RING, batch * chunk, cols)
    kept = [[] for _ in fes] if return_poses else None
    files = {}
    pending = []                     # per chunk in flight: [(clip, getter of the next bytes, clip ends here), ...] in row order

    dead = set()                     # clips whose file could not be opened or written: reported, the other clips go on

    def live(j):
        return paths[j] is not None and j not in dead

    def drain(keep):
        while len(pending) > keep:
            for j, get, last in pending.pop(0):
                txt = get()
                if live(j):
                    try:
                        files[j].write(txt)
                    except OSError as e:
                        print(e)
                        dead.add(j)
                if last and j in files:          # the clip's last rows: its file is complete (a long job list must not hold
                    files.pop(j).close()         # every file open until the end)

    try:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            stage.pool = pool
            for pieces, pose, rpos, rrot in decode_plan(bd, firsts, speech, style, plan, status=status):
                for r, j, k, n in pieces:
                    if k == 0 and paths[j] is not None:
                        try:
                            files[j] = open(paths[j], "wb")
                            files[j].write(heads[j].encode())
                        except OSError as e:     # (PermissionError included) this clip has no file; generate_gesture prints too
                            print(e)
                            dead.add(j)
                total = sum(n + (1 if k == 0 else 0) for _, _, k, n in pieces)
                table = torch.empty(total, cols, dtype=torch.float64, device=dev)
                spans, r0 = [], 0
                for r, j, k, n in pieces:
                    lo = 0 if k == 0 else 1          # (frame 0 of a later chunk was written with the chunk before)
                    rows = n + 1 - lo
                    if rows == 0:
                        continue
                    P = pose[r, lo:n + 1]
                    a_rpos, a_rrot = rpos[r, lo:n + 1].contiguous(), rrot[r, lo:n + 1].contiguous()
                    a_lpos, a_ltxy = P[:, 6:6 + 3 * J].contiguous(), P[:, 6 + 3 * J:6 + 9 * J].contiguous()
                    if kept is not None:
                        kept[j].append((a_rpos, a_rrot, a_lpos.reshape(rows, J, 3), a_ltxy.reshape(rows, J, 2, 3)))
                    if live(j):
                        d.T = rows
                        out = table[r0:r0 + rows]
                        ref_pos, ref_rot = firsts[j][1], firsts[j][2]
                        L.zeggs_pose_to_bvh_table(d, a_rpos, a_rrot, a_lpos, a_ltxy, ref_pos, ref_rot, seq_dev, out, main.cuda_stream)
                        spans.append((j, r0, rows, k + n == lengths[j] - 1))
                        r0 += rows
                    del a_rpos, a_rrot, a_lpos, a_ltxy
                if not spans:
                    continue
                drain(BATCH_RING - 1)            # the staging buffer used BATCH_RING chunks ago has been written
                getters = stage.submit(table[:r0], [(s0, rows) for _, s0, rows, _ in spans], block)
                pending.append([(j, get, end and i == len(gs) - 1) for (j, _, _, end), gs in zip(spans, getters)
                                for i, get in enumerate(gs)])
            drain(0)
    finally:
        for fh in files.values():
            fh.close()
        stage.release()
    if kept is None:
        return None
    return [tuple(torch.cat([p[i] for p in ps]) for i in range(4)) for ps in kept]


def generate_gestures(jobs, network_path, data_path, results_path, style_encoding_type="example", batch=32, chunk=256,
                      use_gpu=True, return_poses=False, threads=None):
    """A whole job list in one call: `jobs` are Job objects (or dicts of Job's arguments); N (audio, style) jobs in, N BVH / WAV
    pairs out.  Networks and statistics are loaded once, each job's front end runs exactly as generate_gesture() does (same
    seeding, so a job's style encoding equals what generate_gesture() returns for the same arguments; parsed exemplars are kept
    across jobs), and the clips are decoded together, `batch` rows at a time, on the weight-stationary sweep
    (ops.decoder_batch_chunk) in chunks of `chunk` frames: rows of clips that end are handed to the next job at the chunk
    boundary.  One job, a FiLM decoder or dimensions the sweep does not take: every job runs the per-clip path of
    generate_gesture(), still on the networks loaded once.  -> the list of style encodings; with return_poses also each clip's
    (root_pos [T,3], root_rot [T,4], lpos [T,J,3], ltxy [T,J,2,3]) device tensors."""
    from . import ops
    jobs = [j if isinstance(j, Job) else Job(**j) for j in jobs]
    results_path = Path(results_path)
    results_path.mkdir(exist_ok=True)
    if not (use_gpu and torch.cuda.is_available()):
        raise RuntimeError("the ZeroEGGS MI355X engine has no CPU path (use_gpu=False / no GPU visible)")
    device = torch.device("cuda")
    if not jobs:
        return ([], []) if return_poses else []
    _seed_all(jobs[0].seed)
    ld = _Loaded(network_path, data_path, style_encoding_type, device)
    cache, fes = {}, []
    with torch.no_grad():
        for j in jobs:
            _seed_all(j.seed)
            fes.append(_front_end(ld, j.audio_file, j.styles, style_encoding_type, j.blend_type, j.blend_ratio, j.file_name,
                                  j.first_pose, j.temperature, cache=cache, mirror_style=j.mirror_style))
        bd = None
        rows = min(int(batch), len(jobs))
        if rows >= 2 and not ld.film and int(chunk) >= 4:
            sp, st = fes[0]["speech"], fes[0]["final"]
            bd = ops.BatchDecode(ld.decoder, rows, min(int(chunk), max(4, max(fe["speech"].shape[1] for fe in fes))),
                                 sp.shape[2], st.shape[2], *ld.stats, ld.dt)
            if not bd.sweep:
                bd = None
        if bd is None:
            poses = [_decode_one(ld, fe, j.audio_file, results_path, return_poses) for j, fe in zip(jobs, fes)]
        else:
            # a file that cannot be opened, written or copied costs that job's file only (as in the loop over generate_gesture)
            with _stage("batch_decode+pose_to_bvh_device_with_bvh_text_write_host_underneath"):
                poses = _decode_batch(ld, fes, [str(results_path / (fe["file_name"] + ".bvh")) for fe in fes], bd, bd.B,
                                      bd.chunk, return_poses, threads=threads)
            with _stage("wav_copy_host"):
                for j, fe in zip(jobs, fes):
                    try:
                        copyfile(j.audio_file, str(results_path / (fe["file_name"] + ".wav")))
                    except (PermissionError, OSError) as e:
                        print(e)
    encodings = [fe["final"] for fe in fes]
    return (encodings, poses) if return_poses else encodings
