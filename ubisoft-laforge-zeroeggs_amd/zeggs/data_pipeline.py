"""Dataset preparation on the device: raw corpus (BVH + WAV takes, info CSV, speaker-timing CSVs) -> processed_data.npz,
stats.npz, data_definition.json -- the driver `data_pipeline(conf)` of the reference (ZEGGS/data_pipeline.py:234-736).

The host keeps the bookkeeping (CSV rows, timecodes, ranges, labels) and the text I/O (zeggs.anim.bvh_load / bvh_save); every
array stage runs on the device (csrc/prepare.hip, mel.hip, anim.hip): speaker silencing and trimming, the `len_ratios` time-stretch
(not-a-knot cubic splines over positions, unrolled quaternions and the raw audio), the trimmed-take centring, the audio and
animation features and the masked dataset statistics.  A take's features go from the kernels into the dataset's device buffers at
the take's row offset; the dataset comes down once at the end.

The reference's in-place writes are part of what it computes, and are reproduced as explicit data flow (tests/golden/prepare.npz
pins them): with `save_trimmed_animation` the centring is written into the take, so the saved file AND the features come from the
centred take; at len_ratio 1.0 the take is the trimmed original itself, which also receives the root-relative hips position that
preprocess_animation writes into its input.  Ratios listed after 1.0 are therefore stretched from that modified original: the order
of `len_ratios` matters.

Differences from the reference, on purpose:
  * `label_names` is in order of first appearance, train ranges before validation ranges (the reference's `list(set(...))` order
    changes with the process's hash seed: any order is one it can produce);
  * an info file without a validation take works (the reference writes its files and then dies in its summary table);
    `ranges_valid` is then an empty [0, 2] array;
  * `visualize_spectrogram`, `visualize_gaze` and `save_normalized_animations` raise NotImplementedError, and `data_info.html`
    is not written (cosmetics);
  * WAV files must already have `audio_conf.sampling_rate` (the reference shells out to SoX otherwise);
  * the conf key `mirror` (the reference has none: it expects `*_mirror.bvh` files, made outside its code base, in the corpus): every
    info row is followed by its left/right reflection, made on the device from the loaded take (zeggs.anim.mirror_take) and taken
    through the same stages as any take, with the capture's audio side computed once.  Without the key nothing changes.
"""
import csv
import ctypes as C
import json
import time
from pathlib import Path

import numpy as np

from .capi import api

NOT_IMPLEMENTED_KEYS = ("visualize_spectrogram", "visualize_gaze", "save_normalized_animations")
ANIM_FPS = 60


# ----------------------------------------------------------------------------- host bookkeeping (no GPU, no pandas)
def timecode_to_sixtieths(text, frame_units):
    """'HH:MM:SS:FF' -> sixtieths of a second; a frame is `frame_units` sixtieths (audio timecodes run at 30 fps: 2, animation and
    acting timecodes at 60 fps: 1).  data_pipeline.py:336-372"""
    h, m, s, f = (int(v) for v in str(text).rsplit(":"))
    return h * 216000 + m * 3600 + s * 60 + f * frame_units


def speaker_time_to_sample(text, fs):
    """'M:SS.mmm' of a speaker-timing row -> sample index (data_pipeline.py:314-327: the milliseconds are truncated)"""
    m, s, ms = (int(v) for v in str(text).replace(".", ":").rsplit(":"))
    return m * 60 * fs + s * fs + int(ms * (fs / 1000))


def speaker_intervals(rows, fs):
    """rows of a speaker-timing CSV (dicts with '#', 'Start', 'End') -> int64 [K, 2] sample intervals [start, end) of the rows whose
    '#' holds an "R": what is kept, everything else is silenced"""
    iv = [[speaker_time_to_sample(r["Start"], fs), speaker_time_to_sample(r["End"], fs)] for r in rows if "R" in str(r["#"])]
    return np.asarray(iv, dtype=np.int64).reshape(-1, 2)


def take_timing(row, audio_sr, anim_fps=ANIM_FPS):
    """info row -> (audio start, audio end, first frame, end frame) of the acting span in the take's own audio samples / animation
    frames (data_pipeline.py:345-400; numpy's round: halves to even)"""
    audio0 = timecode_to_sixtieths(row["audio_start_time"], 2)
    anim0 = timecode_to_sixtieths(row["anim_start_time"], 1)
    act0 = timecode_to_sixtieths(row["acting_start_time"], 1)
    act1 = timecode_to_sixtieths(row["acting_end_time"], 1)
    a0 = int(np.round((act0 - audio0) * (audio_sr / 60)))
    a1 = int(np.round((act1 - audio0) * (audio_sr / 60)))
    f0 = int(np.round((act0 - anim0) * (anim_fps / 60)))
    f1 = int(np.round((act1 - anim0) * (anim_fps / 60)))
    if a0 < 0 or f0 < 0 or a1 < 0 or f1 < 0:
        raise ValueError("The timings are incorrect!")
    return a0, a1, f0, f1


def is_validation(value):
    """the `validation` column as pandas reads it: TRUE / FALSE (any case), 1 / 0"""
    return str(value).strip().lower() in ("true", "1", "1.0", "yes")


def trimmed_name(anim_bvh, len_ratio):
    return str(anim_bvh).split(".")[0] + "_x_" + str(len_ratio).replace(".", "_")


def read_csv_rows(path):
    with open(path, newline="") as fh:
        return list(csv.DictReader(fh))


class Ranges:
    """The dataset's row bookkeeping: takes are appended in processing order, each as [first row, end row) with its style."""

    def __init__(self):
        self.row = 0
        self.train, self.valid, self.train_styles, self.valid_styles = [], [], [], []

    def add(self, nframes, style, validation):
        span = [self.row, self.row + nframes]
        (self.valid if validation else self.train).append(span)
        (self.valid_styles if validation else self.train_styles).append(style)
        self.row += nframes
        return span

    def finish(self):
        """-> (ranges_train, ranges_valid, ranges_train_labels, ranges_valid_labels, label_names): int32 arrays, the names in
        order of first appearance, train before valid"""
        names = list(dict.fromkeys(self.train_styles + self.valid_styles))
        idx = lambda styles: np.asarray([names.index(s) for s in styles], dtype=np.int32)  # noqa: E731
        arr = lambda r: np.asarray(r, dtype=np.int32).reshape(-1, 2)  # noqa: E731
        return arr(self.train), arr(self.valid), idx(self.train_styles), idx(self.valid_styles), names

    def stats_mask(self):
        """rows that enter the statistics: [s + 2, e - 2) of the TRAIN ranges (data_pipeline.py:564-566)"""
        mask = np.zeros(self.row, dtype=bool)
        for s, e in self.train:
            mask[s + 2:e - 2] = True
        return mask


def label_totals(ranges_train, ranges_valid, train_labels, valid_labels, label_names):
    """-> [(label, train frames, valid frames)]; frames are halved as in the reference's table (mirrored takes count once)"""
    out = []
    for i, name in enumerate(label_names):
        tr, va = ranges_train[train_labels == i], ranges_valid[valid_labels == i]
        out.append((name, float(np.sum(tr[:, 1] - tr[:, 0])) / 2, float(np.sum(va[:, 1] - va[:, 0])) / 2))
    return out


def check_conf(conf):
    for k in NOT_IMPLEMENTED_KEYS:
        if conf.get(k, False):
            raise NotImplementedError(f"data_pipeline: conf key {k!r} is not supported (plots and normalised BVH dumps are not ported)")
    mirror_options(conf)


MIRROR_SUFFIX = "_mirror"


def mirror_options(conf):
    """the conf key `mirror` (an addition: the reference expects the mirrored files to exist) -> None (absent or false: the pipeline
    as it is) or dict(suffix, pairs); true is {"suffix": "_mirror", "pairs": "auto"}.  ValueError for anything malformed."""
    m = conf.get("mirror", False)
    if m is False or m is None:
        return None
    if m is True:
        m = {}
    if not isinstance(m, dict) or set(m) - {"suffix", "pairs"}:
        raise ValueError(f"data_pipeline: conf key 'mirror' must be false, true or {{'suffix': ..., 'pairs': ...}}, not {m!r}")
    suffix, pairs = m.get("suffix", MIRROR_SUFFIX), m.get("pairs", "auto")
    if not isinstance(suffix, str) or not suffix or "." in suffix or "/" in suffix:
        raise ValueError(f"data_pipeline: mirror suffix {suffix!r} (a non-empty string without '.' or '/')")
    if not (pairs == "auto" or (isinstance(pairs, (list, tuple)) and all(isinstance(p, int) and not isinstance(p, bool) for p in pairs)) or
            (isinstance(pairs, dict) and all(isinstance(v, (str, int)) for kv in pairs.items() for v in kv))):
        raise ValueError(f"data_pipeline: mirror pairs {pairs!r} ('auto', a list of joint indices or a dict of partners)")
    return dict(suffix=suffix, pairs=pairs)


def mirrored_name(anim_bvh, suffix):
    """'take.bvh' -> 'take_mirror.bvh'.  The stem ends at the FIRST dot, as in trimmed_name (the reference's `split(".")[0]`), so that
    the trimmed files of a take and of its reflection get different names: 'take.v2.bvh' -> 'take_mirror.v2.bvh'"""
    stem, dot, ext = str(anim_bvh).partition(".")
    return stem + suffix + dot + ext


def mirror_plan_of_info(info, suffix):
    """-> per info row the `anim_bvh` its mirrored take gets, None for a row that gets none: its name already carries the suffix, or
    the mirrored name is listed itself"""
    listed = {str(r["anim_bvh"]) for r in info}
    out = []
    for r in info:
        name = mirrored_name(r["anim_bvh"], suffix)
        out.append(None if str(r["anim_bvh"]).partition(".")[0].endswith(suffix) or name in listed else name)
    return out


# ----------------------------------------------------------------------------- device kernels (csrc/prepare.hip)
def spline_chunk():
    """(rows per elimination chunk, halo rows, widest table on the thread-per-chunk kernel) of zeggs_spline_resample"""
    c, h, w = C.c_int(0), C.c_int(0), C.c_int(0)
    api().zeggs_spline_chunk(C.byref(c), C.byref(h), C.byref(w))
    return c.value, h.value, w.value


def spline_resample(y, m):
    """y: device float64 [N, W] (or [N]) -> [m, W] ([m]): the not-a-knot cubic spline over the integer grid at linspace(0, N-1, m)
    (scipy griddata(method="cubic") on 1-D points).  N < 4 raises ValueError, as scipy does."""
    import torch
    from . import ops
    if not (y.is_cuda and y.dtype == torch.float64):
        raise RuntimeError("spline_resample: a float64 tensor on the GPU is needed (the HIP engine has no CPU path)")
    flat = y.dim() == 1
    t = y.reshape(y.shape[0], -1).contiguous()
    n, w = t.shape
    if n < 4:
        raise ValueError(f"a cubic spline needs at least 4 rows, got {n}")
    L = api()
    out = torch.empty(int(m), w, dtype=torch.float64, device=y.device)
    ws = ops._ws(max(L.zeggs_spline_resample_workspace_bytes(n, int(w)), 256), y.device)
    L.zeggs_spline_resample(t, n, int(w), int(m), out, ws, ws.numel(), ops._stream())
    return out.reshape(-1) if flat else out.reshape((int(m),) + tuple(y.shape[1:]))


def rot_stretch(euler, m, order):
    """euler: device float64 [N, J, 3] degrees in channel order `order` -> [m, J, 3] (from_euler, unroll, spline, normalise, to_euler)"""
    import torch
    from . import anim, ops
    code = anim._to_euler_order(order)          # raises NotImplementedError for orders quat.to_euler does not have, as bvh_channels
    e = euler.contiguous()
    n, j = e.shape[0], e.shape[1]
    if n < 4:
        raise ValueError(f"a cubic spline needs 4 frames, got {n}")
    L = api()
    out = torch.empty(int(m), j, 3, dtype=torch.float64, device=e.device)
    ws = ops._ws(max(L.zeggs_rot_stretch_workspace_bytes(n, int(j), int(m)), 256), e.device)
    L.zeggs_rot_stretch(e, n, int(j), int(m), int(code), out, ws, ws.numel(), ops._stream())
    return out


def audio_prepare(wav, intervals, start, end, want_f64=False):
    """wav: device float32 [n]; intervals: int64 [K, 2] (host) -> (float32 [len], float64 [len] or None): the signal times the union of
    the intervals, cut to [start, end) (clipped at the signal's end like a numpy slice)"""
    import torch
    from . import ops
    n = wav.numel()
    length = max(min(int(end), n) - int(start), 0)
    iv = torch.as_tensor(np.ascontiguousarray(intervals, dtype=np.int64).reshape(-1, 2)).to(wav.device)
    o32 = torch.empty(length, dtype=torch.float32, device=wav.device)
    o64 = torch.empty(length, dtype=torch.float64, device=wav.device) if want_f64 else None
    api().zeggs_audio_prepare(wav, n, iv, int(iv.shape[0]), int(start), max(int(end), int(start)), o32, o64, ops._stream())
    return o32, o64


def center_take(pos, rot, order, round_f32):
    """the centring of data_pipeline.py:449-459 IN PLACE on device float64 [N, J, 3] positions / euler degrees"""
    from . import anim, ops
    code = anim._to_euler_order(order)
    assert pos.is_contiguous() and rot.is_contiguous()
    ws = ops._ws(256, pos.device)
    api().zeggs_center_take(pos, rot, pos.shape[0], int(pos.shape[1]), int(code), int(bool(round_f32)), ws, ws.numel(), ops._stream())


def masked_stats(x, mask):
    """x: device float32 [R, ...]; mask: device bool / uint8 [R] -> (mean [D], std [D], pooled std [1]) float64 device tensors over the
    masked rows (population std; pooled = the std of all masked elements).  Bitwise reproducible."""
    import torch
    from . import ops
    if not (x.is_cuda and x.dtype == torch.float32):
        raise RuntimeError("masked_stats: a float32 tensor on the GPU is needed (the HIP engine has no CPU path)")
    t = x.reshape(x.shape[0], -1).contiguous()
    r, d = t.shape
    mk = mask.to(torch.uint8).contiguous()
    L = api()
    out = torch.empty(2 * d + 1, dtype=torch.float64, device=x.device)
    ws = ops._ws(max(L.zeggs_masked_stats_workspace_bytes(r, int(d)), 256), x.device)
    L.zeggs_masked_stats(t, mk, r, int(d), out[:d], out[d:2 * d], out[2 * d:], ws, ws.numel(), ops._stream())
    return out[:d], out[d:2 * d], out[2 * d:]


class _Rows:
    """A dataset array on the device that grows by whole takes: `put` casts a take's rows into the buffer at the current row offset."""

    def __init__(self, device):
        self.device, self.buf, self.n = device, None, 0

    def put(self, t):
        import torch
        k = t.shape[0]
        if self.buf is None or self.n + k > self.buf.shape[0]:
            cap = max(2 * (self.buf.shape[0] if self.buf is not None else 0), self.n + k, 4096)
            new = torch.empty((cap,) + tuple(t.shape[1:]), dtype=torch.float32, device=self.device)
            if self.buf is not None:
                new[:self.n].copy_(self.buf[:self.n])
            self.buf = new
        self.buf[self.n:self.n + k].copy_(t)          # (float64 -> float32 on the way in)
        self.n += k

    def view(self):
        return self.buf[:self.n]


# dataset arrays in the order of preprocess_animation's tuple: (key, index)
_ANIM_KEYS = (("Y_root_pos", 0), ("Y_root_rot", 1), ("Y_root_vel", 2), ("Y_root_vrt", 3), ("Y_lpos", 4), ("Y_ltxy", 6), ("Y_lvel", 7),
              ("Y_lvrt", 8), ("Y_gaze_pos", 14), ("Y_gaze_dir", 15))
_IN_STATS = ("Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt", "Y_gaze_dir")
_OUT_STATS = _IN_STATS[:-1]


def read_wav(path, fs):
    """WAV -> float32 in [-1, 1) at the expected rate (audio_files.read_wavfile(rescale=True) without its SoX fall-back)"""
    from scipy.io import wavfile
    got, x = wavfile.read(str(path))
    if got != fs:
        raise ValueError(f"{path}: expected a {fs} Hz wav (got {got} Hz); resample offline")
    if x.ndim > 1:
        raise ValueError(f"{path}: expected a mono wav (got {x.shape[1]} channels)")
    if x.dtype == np.int16:
        return (x / 32768.0).astype(np.float32)
    if x.dtype == np.int32:
        return (x / 2147483648.0).astype(np.float32)
    if x.dtype == np.uint8:
        return (((x / 255.0) - 0.5) * 2).astype(np.float32)
    if x.dtype in (np.float32, np.float64):
        if np.max(np.abs(x)) > 1.0:
            raise ValueError(f"{path}: float wav contains samples outside [-1, 1]")
        return x.astype(np.float32)
    raise TypeError(f"could not normalize wav, unsupported sample type {x.dtype}")


def write_wav(path, samples, fs):
    """audio_files.write_wavefile: float samples * 2^15, truncated to int16"""
    from scipy.io import wavfile
    wavfile.write(str(path), fs, (np.asarray(samples) * 2 ** 15).astype("int16"))


def _device_statistics(arrays, mask):
    """arrays: key -> device float32 rows -> masked_stats of the audio rows and of every array of _IN_STATS (device tensors)"""
    return {k: masked_stats(arrays[k], mask) for k in ("X_audio_features",) + _IN_STATS}


def _normalisation(where):
    """the statistics of _device_statistics, downloaded -> the six normalisation entries of stats.npz in their order"""
    f32 = np.float32
    st = {k: tuple(t.cpu().numpy() for t in v) for k, v in where.items()}
    audio_mean, _, audio_pooled = st["X_audio_features"]
    in_mean = np.hstack([st[k][0] for k in _IN_STATS]).astype(f32)
    in_std = np.hstack([np.repeat(st[k][2] + 1e-10, len(st[k][0])) for k in _IN_STATS]).astype(f32)     # pooled scalars + eps
    out_mean = np.hstack([st[k][0] for k in _OUT_STATS]).astype(f32)
    out_std = np.hstack([st[k][1] for k in _OUT_STATS]).astype(f32)                                     # per column, no eps
    return dict(audio_input_mean=audio_mean.astype(f32), audio_input_std=f32(audio_pooled[0] + 1e-10), anim_input_mean=in_mean,
                anim_input_std=in_std, anim_output_mean=out_mean, anim_output_std=out_std)


_PROCESSED_KEYS = ("X_audio_features", "Y_root_pos", "Y_root_rot", "Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt",
                   "Y_gaze_pos")


def mirror_processed(processed, definition, pairs="auto", ranges_per_take=1, device="cuda"):
    """A processed dataset WITHOUT mirrored ranges (the dict of processed_data.npz) -> the dataset `data_pipeline` makes of the same
    corpus with `mirror`: for users who have a processed_data.npz and no raw takes.  The `Y_*` rows go through anim.mirror_rows
    (one launch per array), the audio rows are copied; every take's ranges are followed by the ranges of its reflection --
    `ranges_per_take` consecutive ranges are one take: the number of `len_ratios` the dataset was made with -- with the same
    labels, and the statistics are recomputed over the new train ranges with masked_stats.  The dataset does not store the gaze
    direction (only its statistics): it is restated here from the stored float32 root and gaze rows, so its four statistics
    agree with a pipeline run to float32 rounding, not bit for bit; every other number is the pipeline's.
    -> (processed, definition): new dicts, the inputs are not modified."""
    import torch
    from . import anim as zanim
    if not torch.cuda.is_available():
        raise RuntimeError("mirror_processed: no GPU (the HIP engine has no CPU path)")
    dev = torch.device(device)
    pair = zanim.resolve_pairs(pairs, definition["bone_names"], definition["parents"])
    k = int(ranges_per_take)
    tr, va = np.asarray(processed["ranges_train"]).reshape(-1, 2), np.asarray(processed["ranges_valid"]).reshape(-1, 2)
    spans = sorted([(int(s), int(e), False, int(l)) for (s, e), l in zip(tr, processed["ranges_train_labels"])] +
                   [(int(s), int(e), True, int(l)) for (s, e), l in zip(va, processed["ranges_valid_labels"])])
    if k < 1 or len(spans) % k:
        raise ValueError(f"mirror_processed: {len(spans)} ranges are not whole takes of {k} ranges each")
    up = {key: torch.as_tensor(np.ascontiguousarray(processed[key], dtype=np.float32)).to(dev) for key in _PROCESSED_KEYS}
    both = {key: (t, t if key == "X_audio_features" else zanim.mirror_rows(t, key, pair)) for key, t in up.items()}
    # rows: per take its ranges, then the same ranges of the reflection
    pieces, ranges, names = [], Ranges(), list(definition["label_names"])
    for g in range(0, len(spans), k):
        for side in (0, 1):
            for s, e, valid, label in spans[g:g + k]:
                pieces.append((side, s, e))
                ranges.add(e - s, names[label], valid)
    new = {key: torch.cat([both[key][side][s:e] for side, s, e in pieces]) for key in _PROCESSED_KEYS}
    ranges_train, ranges_valid, train_labels, valid_labels, new_names = ranges.finish()
    relabel = lambda idx: np.asarray([names.index(new_names[i]) for i in idx], dtype=np.int32)  # noqa: E731   (the definition keeps its order)
    # the gaze direction: inverse root rotation times (gaze - root), as preprocess_animation states it, from the stored rows
    q, v = new["Y_root_rot"].double(), new["Y_gaze_pos"].double() - new["Y_root_pos"].double()
    qv = -q[:, 1:]
    t = 2.0 * torch.linalg.cross(qv, v)
    arrays = dict(new, Y_gaze_dir=(v + q[:, :1] * t + torch.linalg.cross(qv, t)).float())
    norm = _normalisation(_device_statistics(arrays, torch.as_tensor(ranges.stats_mask()).to(dev)))
    out = {key: new[key].cpu().numpy() for key in _PROCESSED_KEYS}
    out.update(ranges_train=ranges_train, ranges_valid=ranges_valid, ranges_train_labels=relabel(train_labels),
               ranges_valid_labels=relabel(valid_labels), **norm)
    return out, dict(definition)


def data_pipeline(conf, device="cuda", log=None, timings=None):
    """Prepare audio and animation data for training (reference data_pipeline.data_pipeline, same conf keys, same return value
    (processed_data, data_definition) and the same files).  `log`: callable for the progress lines (one per take, totals per label);
    `timings`: dict that receives seconds per stage (the device is then synchronised after every stage)."""
    import torch
    from . import anim as zanim
    from . import audio as zaudio

    check_conf(conf)
    if not torch.cuda.is_available():
        raise RuntimeError("data_pipeline: no GPU (the HIP engine has no CPU path)")
    dev = torch.device(device)
    log = log or (lambda *_: None)
    clock = [time.perf_counter()]

    def lap(stage):
        if timings is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            timings[stage] = timings.get(stage, 0.0) + now - clock[0]
            clock[0] = now

    len_ratios = list(conf["len_ratios"])
    base = Path(conf["base_path"])
    out_dir = base / conf["processed_data_path"]
    out_dir.mkdir(exist_ok=True)
    with open(out_dir / "data_pipeline_conf.json", "w") as f:
        json.dump(conf, f, indent=4)
    info = read_csv_rows(base / conf["info_filename"])
    fs = int(conf["audio_conf"]["sampling_rate"])
    original = base / "original"

    rows = {k: _Rows(dev) for k in ("X_audio_features",) + tuple(k for k, _ in _ANIM_KEYS)}
    ranges = Ranges()
    last = None
    mirror = mirror_options(conf)
    mirror_names = mirror_plan_of_info(info, mirror["suffix"]) if mirror else [None] * len(info)
    n_row = 0
    for row in info:
        # ---- load
        take = zanim.bvh_load(str(original / row["anim_bvh"]))
        if int(np.ceil(1 / take["frametime"])) != ANIM_FPS:
            raise ValueError(f"{row['anim_bvh']}: {1 / take['frametime']:.3f} frames per second, the pipeline needs {ANIM_FPS}")
        audio_file = original / row["audio_filename"]
        wav = read_wav(audio_file, fs)
        intervals = speaker_intervals(read_csv_rows(audio_file.with_suffix(".csv")), fs)
        a0, a1, f0, f1 = take_timing(row, fs)
        lap("load")
        # ---- silence, trim (device)
        stretch = any(r != 1.0 for r in len_ratios)
        a32, a64 = audio_prepare(torch.as_tensor(wav).to(dev), intervals, a0, a1, want_f64=stretch)
        rot0 = torch.as_tensor(np.ascontiguousarray(take["rotations"][f0:f1])).to(dev).to(torch.float64)
        pos0 = torch.as_tensor(np.ascontiguousarray(take["positions"][f0:f1])).to(dev).to(torch.float64)
        n0, nj = rot0.shape[0], rot0.shape[1]
        valid = is_validation(row["validation"])
        folder = out_dir / "trimmed" / ("valid" if valid else "train")
        lap("trim")
        # the takes of this row: the capture and, with `mirror`, its left/right reflection directly after it -- an independent take
        # in every stage below (made from the LOADED channels, before the loop writes into them), with the capture's audio; both have
        # n0 frames of nj joints
        versions = [(row["anim_bvh"], take, rot0, pos0)]
        if mirror_names[n_row] is not None:
            mtake = zanim.mirror_take(dict(take, rotations=rot0, positions=pos0), mirror["pairs"])
            versions.append((mirror_names[n_row], mtake, mtake["rotations"], mtake["positions"]))
            lap("mirror")
        n_row += 1
        audio_side = {}          # len_ratio -> (float64 wave or None, float32 wave, audio features): computed for the first version
        for (v_bvh, v_take, v_rot0, v_pos0), ratio in ((v, r) for v in versions for r in len_ratios):
            # the take at 1.0 IS the trimmed original (float32 channels): what the centring does to it stays for the ratios after it
            if ratio != 1.0:
                m = int(ratio * n0)
                pos = spline_resample(v_pos0.reshape(n0, -1), m).reshape(m, nj, 3)
                rot = rot_stretch(v_rot0, m, v_take["order"])
            else:
                pos, rot = v_pos0, v_rot0
            if ratio in audio_side:
                wave64, wave, audio_feats = audio_side[ratio]
            elif ratio != 1.0:
                wave64 = spline_resample(a64, int(ratio * a64.numel()))
                wave, audio_feats = wave64.to(torch.float32), None
            else:
                wave64, wave, audio_feats = None, a32, None
            lap("stretch")
            name = trimmed_name(v_bvh, ratio)
            if conf["save_trimmed_audio"]:
                folder.mkdir(exist_ok=True, parents=True)
                write_wav(folder / (name + ".wav"), (wave64 if wave64 is not None else wave).cpu().numpy(), fs)
                lap("write_wav")
            if conf["save_trimmed_animation"]:
                folder.mkdir(exist_ok=True, parents=True)
                center_take(pos, rot, v_take["order"], round_f32=(ratio == 1.0))
                # (device float64 channels: the motion text is formatted where they are, anim.TEXT = "host" downloads them instead)
                zanim.bvh_save(folder / (name + ".bvh"), dict(v_take, positions=pos, rotations=rot))
                lap("write_bvh")
            # ---- features, straight into the dataset's buffers
            nframes = rot.shape[0]
            if audio_feats is None:
                audio_feats = zaudio.preprocess_audio_device(wave, ANIM_FPS, nframes, conf["audio_conf"], conf["audio_feature_type"], dev)
                if len(versions) > 1:
                    audio_side[ratio] = (wave64, wave, audio_feats)
            rows["X_audio_features"].put(audio_feats)
            lap("audio_features")
            feats = zanim.preprocess_animation_device(rot, pos, v_take["parents"], v_take["names"], v_take["frametime"], v_take["order"])
            for k, i in _ANIM_KEYS:
                rows[k].put(feats[i])
            if ratio == 1.0:
                # the reference's preprocess_animation writes the root-relative hips position into the take it was given
                # (data_pipeline.py:97, 147: `lpos` IS anim_data["positions"]); at 1.0 that is the trimmed original (float32)
                v_pos0[:, 0] = feats[4][:, 0].to(torch.float32)
            lap("anim_features")
            span = ranges.add(nframes, row["style"], valid)
            log(f"{name}: {nframes} frames -> rows [{span[0]}, {span[1]}) {'valid' if valid else 'train'} {row['style']}")
        last = take
    if last is None:
        raise ValueError(f"{base / conf['info_filename']}: no takes")

    ranges_train, ranges_valid, train_labels, valid_labels, label_names = ranges.finish()
    if bool(torch.isnan(rows["X_audio_features"].view()).any()):
        raise ValueError("data_pipeline: NaN in the audio features (a take's animation outlasts its audio)")
    # ---- statistics over rows [s + 2, e - 2) of the train ranges (device, float64 accumulation)
    mask = torch.as_tensor(ranges.stats_mask()).to(dev)
    where = _device_statistics({k: rows[k].view() for k in rows}, mask)
    lap("statistics")
    # ---- one download
    data = {k: rows[k].view().cpu().numpy() for k in rows}
    norm = _normalisation(where)
    lap("download")
    stats = dict(ranges_train=ranges_train, ranges_valid=ranges_valid, ranges_train_labels=train_labels,
                 ranges_valid_labels=valid_labels, **norm)
    processed = {k: data[k] for k in ("X_audio_features", "Y_root_pos", "Y_root_rot", "Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy",
                                      "Y_lvel", "Y_lvrt", "Y_gaze_pos")}
    processed.update(stats)
    definition = dict(dt=last["frametime"], label_names=label_names, parents=np.asarray(last["parents"]).tolist(),
                      bone_names=list(last["names"]))
    if conf["save_final_data"]:
        np.savez(out_dir / "processed_data.npz", **processed)
        np.savez(out_dir / "stats.npz", **stats)
        with open(out_dir / "data_definition.json", "w") as f:
            json.dump(definition, f, indent=4)
        lap("save")
    total = 0.0
    for name, tr, va in label_totals(ranges_train, ranges_valid, train_labels, valid_labels, label_names):
        log(f"{name}: train {tr} frames - {tr / 60:.1f} secs, validation {va} frames - {va / 60:.1f} secs, "
            f"total {tr + va} frames - {(tr + va) / 60:.1f} secs")
        total += tr + va
    log(f"Total length of dataset is {total} frames - {total / 60:.1f} seconds")
    return processed, definition
