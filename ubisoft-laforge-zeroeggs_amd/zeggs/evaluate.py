"""Held-out evaluation: the validation (or training) split scored on the device, per window.

The split is cut into non-overlapping windows of the training length (plan_windows), batches of them run through the networks in
eval mode under no_grad exactly as a training step runs them (speech encoder, style encoder with z = mu, decoder rollout at
B = batch), and the loss section's forward-only, per-window kernel (ops.loss_eval) scores every window on its own.  The rows
are added up per style label on the device (ops.eval_accumulate); the host sees ONE table, once, at the end.  The reference has
no counterpart: it only renders validation clips to look at.
"""
import numpy as np
import torch

from . import ops
from .modules import kl_div_weight

COLS = ops.EVAL_COLS
_NAMES = {18: "mpjpe", 19: "root_drift", 20: "speed_pred", 21: "speed_true"}


def plan_windows(ranges, window):
    """Non-overlapping windows of `window` frames: for every range [a, e) the starts a, a + window, ... while start < e - window
    -- the admissible starts of the training window table (engine.DeviceDataset, reference dataset.py:79-96) at stride `window`;
    a range's remainder is not scored.  Host integers only.  -> (starts int64 [n], range_index int64 [n])"""
    ranges = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    per = [np.arange(a, e - window, window, dtype=np.int64) for a, e in ranges]
    starts = np.concatenate(per) if per else np.zeros(0, np.int64)
    index = np.repeat(np.arange(len(ranges), dtype=np.int64), [len(p) for p in per]) if per else np.zeros(0, np.int64)
    return starts, index


def example_rows_for(starts, ranges, range_index, window, example_len, n_frames):
    """Source frame of every row of the style example of the windows at `starts` (reference dataset.py:176-204): the rule of
    engine.DeviceDataset.example_rows for windows of ANY ranges.  -> int64 [n, example_len]"""
    r0 = np.asarray(starts, dtype=np.int64)
    rng = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)[np.asarray(range_index, dtype=np.int64)]
    rs, re = rng[:, 0], rng[:, 1]
    r_last = r0 + window - 1
    ext = (example_len - window) // 2
    ws = np.minimum(ext, r0 - rs)
    we = np.minimum(ext, re - r_last)
    start = np.maximum(r0 - (ws + ext - we), rs)
    end = np.minimum(np.minimum(r_last + (we + ext - ws), re) + 1, n_frames)
    cur = end - start
    k = np.arange(example_len)[None, :]
    rows = np.where(k < cur[:, None], start[:, None] + k, end[:, None] - example_len + k)
    # an example longer than the frames in front of its window's range end would start before frame 0: the gather kernel reads the
    # rows it is given unchecked (an out-of-bounds read on the device), so it is refused here, on the host, ahead of any launch
    if rows.size and (rows.min() < 0 or rows.max() >= n_frames):
        raise ValueError(f"example_len {example_len} reaches outside the dataset's {n_frames} frames (source rows {int(rows.min())} .. "
                         f"{int(rows.max())}): shorten the style example")
    return rows.astype(np.int64)


def shard(n_batches, world, rank):
    """The batches of `rank`, dealt round-robin: rank, rank + world, ..."""
    return list(range(rank, n_batches, world))


def summarise(table, window, iteration=None):
    """[groups, COLS + 1] sums (last column: windows counted) -> the result dictionary of evaluate()"""
    from .train import LOSS_TAGS
    table = np.asarray(table, dtype=np.float64)
    klw = kl_div_weight(iteration) if iteration is not None else 0.0

    def one(row):
        n = row[COLS]
        m = row[:COLS] / n if n > 0 else np.full(COLS, np.nan)
        terms = dict(zip(LOSS_TAGS, [float(v) for v in m[:17]] + [float(klw * m[17])]))
        out = dict(loss=float((m[:17].sum() + klw * m[17]) / 18.0), terms=terms, kl=float(m[17]), windows=int(n),
                   frames_scored=int(n) * int(window))
        out.update({name: float(m[c]) for c, name in _NAMES.items()})
        return out
    res = one(table.sum(axis=0)) if len(table) else one(np.zeros(COLS + 1))
    res["per_label"] = {int(g): one(table[g]) for g in range(len(table)) if table[g, COLS] > 0}
    return res


def _split(dataset, split):
    if split == "valid":
        return dataset.ranges_valid, dataset.ranges_valid_labels
    if split == "train":
        return dataset.ranges_train, dataset.ranges_train_labels
    raise ValueError(f"evaluate: split {split!r} (valid or train)")


def evaluate(speech_encoder, decoder, style_encoder, dataset, parents, dt, split="valid", batch=32, example_len=None,
             iteration=None, max_windows=None, world=1, rank=0, group=None, reduce=True):
    """Score `split` of `dataset` (engine.DeviceDataset) -> dict(loss, terms {train.LOSS_TAGS}, kl, mpjpe, root_drift, speed_pred,
    speed_true, per_label {label: the same}, windows, frames_scored, frames_total, table).

    loss = (sum of the 17 term means + kl_div_weight(iteration) * kl) / 18, comparable with the logged training loss
    (iteration None: weight 0).  style_encoder None: label conditioning, the style is the one-hot of the range's label.
    example_len None: the window length.  world / rank / group: every rank scores its round-robin share of the batches and the
    table is summed with one all_reduce (`group`: the process group); reduce=False returns this rank's raw table
    [labels, 23] (float64 numpy: 22 column sums and the window count per label) instead of the dictionary.
    Eval mode and no_grad inside, the modules' training flags restored on exit.  The networks' matrix products run in a fixed
    summation order (ops.fixed_order_gemms: no split-K atomics), so the same window gives the same bits on every call.
    Batches are gathered into buffers of this call; no noise seed is drawn (eps = 0: z = mu); the last batch is filled up with
    copies of its first window, which are not counted.
    One device-to-host copy, of the table, at the end."""
    ds, T, B = dataset, int(dataset.window), int(batch)
    dev = ds.device
    ranges, labels = _split(ds, split)
    ranges = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    labels = np.asarray(labels, dtype=np.int64)
    frames_total = int((ranges[:, 1] - ranges[:, 0]).sum()) if len(ranges) else 0
    starts, ridx = plan_windows(ranges, T)
    if max_windows is not None:
        starts, ridx = starts[:int(max_windows)], ridx[:int(max_windows)]
    groups = int(labels.max()) + 1 if len(labels) else 0
    n = len(starts)
    if n == 0:      # nothing to score: no launch
        table = np.zeros((groups, COLS + 1))
        if not reduce:
            return table
        return dict(summarise(table, T, iteration), frames_total=frames_total, table=table)
    nb = (n + B - 1) // B
    mine = shard(nb, world, rank)
    mods = [m for m in (speech_encoder, decoder, style_encoder) if m is not None]
    was_training = [m.training for m in mods]
    acc = torch.zeros(groups, COLS + 1, device=dev, dtype=torch.float64)
    try:
        for m in mods:
            m.eval()
        # (fixed-order products: a window's numbers must not depend on the call -- two ranks' tables sum to one rank's table)
        with torch.no_grad(), ops.fixed_order_gemms():
            if mine:
                _score(speech_encoder, decoder, style_encoder, ds, parents, dt, starts, ridx, ranges, labels, mine, B, T,
                       example_len if example_len is not None else T, acc)
            if world > 1 and reduce:
                torch.distributed.all_reduce(acc, op=torch.distributed.ReduceOp.SUM, group=group)
    finally:
        for m, tr in zip(mods, was_training):
            m.train(tr)
    table = acc.cpu().numpy()                       # the one device-to-host copy
    if not reduce:
        return table
    return dict(summarise(table, T, iteration), frames_total=frames_total, table=table)


def _score(se, de, st, ds, parents, dt, starts, ridx, ranges, labels, batches, B, T, example_len, acc):
    """the batches `batches` of the plan, their rows added to `acc` (device); nothing is read back"""
    dev = ds.device
    n = len(starts)
    # the whole plan's index tables go up once, ahead of the first batch: per batch the host only enqueues
    pick = np.stack([np.where(np.arange(bi * B, bi * B + B) < n, np.arange(bi * B, bi * B + B), bi * B) for bi in batches])
    real = np.stack([np.arange(bi * B, bi * B + B) < n for bi in batches])
    up = lambda a, dt_: torch.as_tensor(np.ascontiguousarray(a), dtype=dt_).to(dev)  # noqa: E731
    d_starts = up(starts[pick], torch.int64)                                                       # [nb, B]
    d_group = up(np.where(real, labels[ridx[pick]], -1), torch.int32)                              # padded rows: -1
    parents_d = parents if torch.is_tensor(parents) else torch.as_tensor(np.asarray(parents), dtype=torch.int32)
    parents_d = parents_d.to(device=dev, dtype=torch.int32).contiguous()
    enc = getattr(st, "encoder", None)
    attn = type(enc).__name__ == "StyleEncoderAttn"
    if st is not None:
        d_rows = up(np.stack([example_rows_for(starts[p], ranges, ridx[p], T, example_len, ds.n_frames) for p in pick]), torch.int64)
        eps0 = ops.fill_(torch.empty(B, st.style_embedding_size, device=dev))                      # eps = 0: z = mu
    else:
        nstyle = de.cell_state_encoder.layer0.in_features - (ds.PO + 3)
        onehot = torch.as_tensor(np.eye(nstyle, dtype=np.float32)).to(dev)
        d_label = up(labels[ridx[pick]], torch.int64)
    J = (ds.PO - 6) // 15
    S = st.style_embedding_size if (st is not None and st.use_vae) else 0
    bufs = dict(loss_ws=ops.loss_eval_workspace(B, T, J, S, dt, dev), rows=torch.empty(B, COLS, device=dev, dtype=torch.float64))

    def gw(k, src, s):
        bufs[k] = ops.gather_windows(src, s, T, out=bufs.get(k))
        return bufs[k]

    def gr(k, src, s):
        if k not in bufs:
            bufs[k] = torch.empty(B, src.shape[1], device=dev, dtype=torch.float32)
        return ops.gather_rows(src, s, out=bufs[k], out_ld=src.shape[1])
    for k in range(len(batches)):
        s = d_starts[k]
        audio, pose, rpos, rrot, gaze = (gw(name, getattr(ds, name), s) for name in ("audio", "pose", "rpos", "rrot", "gaze"))
        pose0, rpos0, rrot0 = gr("pose0", ds.pose, s), gr("rpos0", ds.rpos, s), gr("rrot0", ds.rrot, s)
        ops.normalize_rows_(audio, ds.audio_mean, ds.audio_std)
        mu = logvar = None
        if st is not None:
            if attn:        # straight into the encoder's padded input (as engine.DeviceDataset.batch does)
                ws, xp = ops.style_input_buffer(enc, B, example_len, ds.PO + 3, False, dev, ws=bufs.get("style_ws"))
                ops.gather_example(ds.pose, d_rows[k], ds.in_mean, ds.in_std, xp)
                bufs["style_ws"] = ws
                example = ops.example_view(ws, xp)
            else:
                if "example" not in bufs:
                    bufs["example"] = torch.empty(B, example_len, ds.PO + 3, device=dev)
                example = ops.fill_(bufs["example"])                                               # gaze slot = 0
                ops.gather_rows(ds.pose, d_rows[k], out=example, out_ld=ds.PO + 3)
                ops.normalize_rows_(example, ds.in_mean, ds.in_std)
            z, mu, logvar = st(example, 1.0, eps=eps0)
        else:
            z = ops.gather_rows(onehot, d_label[k])
        speech = se(audio)
        style = ops.broadcast_time(z, T)
        o_pose, o_rpos, o_rrot = ops.decoder_core(de, pose0, rpos0, rrot0, gaze, speech, style, ds.in_mean, ds.in_std,
                                                  ds.out_mean, ds.out_std, dt)
        rows = ops.loss_eval(o_pose, o_rpos, o_rrot, pose, rpos, rrot, gaze, parents_d, dt, mu, logvar, rows=bufs["rows"],
                             ws=bufs["loss_ws"])
        ops.eval_accumulate(rows, d_group[k], acc)


def format_table(result, label_names=None):
    """the per-label table of a result dictionary as text lines"""
    head = f"{'label':<16}{'windows':>8}{'loss':>12}{'kl':>12}{'mpjpe':>12}{'root_drift':>12}{'speed_pred':>12}{'speed_true':>12}"
    lines = [head]

    def line(name, r):
        return (f"{name:<16}{r['windows']:>8}{r['loss']:>12.5f}{r['kl']:>12.5f}{r['mpjpe']:>12.5f}{r['root_drift']:>12.5f}"
                f"{r['speed_pred']:>12.5f}{r['speed_true']:>12.5f}")
    for g, r in sorted(result["per_label"].items()):
        lines.append(line(label_names[g] if label_names is not None and g < len(label_names) else str(g), r))
    lines.append(line("all", result))
    return lines
