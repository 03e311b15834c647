#!/usr/bin/env python
"""Live serving: wall time of one LiveServer.step() per row count and stream age, beside GestureStream.push of the same chunk.

  per rows in {1, 8, 32, 64} and stream age in {10 s, 600 s}: every row is fed a synthetic WAV up to that age (1 s pushes, drained),
  then `tick`-sized pushes (tick / 60 s of audio per row) each followed by ONE step(); the step's wall time (host call + device,
  synchronised before and after) over >= 200 steps: median, p95, min, max; what the server enqueues per step; the pushes' wall
  time beside it (mel stays per row: rows pushes per tick).
  baseline, same session: zeggs.stream.GestureStream.push of the same 4-frame chunk at the same two ages (one stream, B = 1).

  --leg push_many: the audio side of a tick, per rows in {1, 8, 32, 64}: two servers in ONE process are fed the same rows' signals
  up to 10 s, then tick by tick the same chunks -- one through push() per stream, the other through ONE push_many() -- each
  synchronised before and after the tick's pushes, taking turns, >= 200 ticks: median, p95, min, max of both, the step beside
  them, what push_many enqueued, and whether the two servers' pending features are bitwise equal at the end
  -> profiles/live_push_many.json.

  --leg loudness (or --loudness): what running loudness normalisation adds to push_many, per rows in {1, 8, 32, 64} and stream age
  in {10 s, 600 s}: two servers in ONE process, loudness=None and loudness="running", are fed the same rows' signals up to the age
  through push_many, then tick by tick the same chunks, each call synchronised before and after, taking turns, >= 200 ticks:
  median, p95, min, max of both, what each enqueued, and whether the cost with loudness on moves with the stream's age by more
  than the spread -> profiles/live_loudness.json.

  --leg resample: what a row at a rate and format of its own costs push_many, per rows in {1, 8, 32, 64} and stream age in
  {10 s, 600 s}: four servers in ONE process -- all rows native float32, or all rows opened at 48 kHz s16, each with loudness off
  and on -- are fed the same rows' signals (the 48 kHz ones three samples per native sample) up to the age through push_many, then
  tick by tick, each call synchronised before and after, taking turns, >= 200 ticks: median, p95, min, max of all four, what each
  enqueued and uploaded, and the converting server's median over the native one's in the same run -> profiles/live_resample.json.

  --leg frames: what the output head costs a step and what it saves a client, per rows in {1, 8, 32, 64} and stream age in
  {10 s, 600 s}: two servers in ONE process, frames=None and frames with all three outputs (local, world, bvh), are fed the same
  rows' signals up to the age through push_many, then tick by tick the same chunks; each step() synchronised before and after,
  taking turns at going first, >= 200 ticks: median, p95, min, max of both, what each enqueues per step (the head adds exactly
  two operations: asserted), the bytes it downloads per step -- and, timed in the same run on the plain server's output, what a
  client has to do today for the BVH part of the same result: per stream anim.bvh_channels on the returned tensors and the
  .cpu() of both -> profiles/live_frames.json.

  --leg retime: what handing the frames out at a stream's own rate costs a step, per rows in {1, 8, 32, 64}: servers in ONE process
  with all three outputs -- the plain head, and the re-timing head with every row at 1 / 1 (60), 1 / 2 (30) and 2 / 1 (120 frames
  a second, max_rate 120) -- are brought to 10 s through push_many, then fed the same chunks tick by tick; each step()
  synchronised before and after, the servers taking turns at going first, >= 200 ticks: median, p95, min, max of each, what each
  enqueues per step (the same number: asserted) and the bytes it downloads per step.  The yardstick is the plain-head column of
  the same run -> profiles/live_retime.json.

  --leg refilter: what the band-limiting filter of the re-timing head costs a step, per rows in {1, 8, 32, 64}: four servers in ONE
  process with all three outputs -- the re-timing head without the filter, every row at 30 and at 120 frames a second, and the
  same two with retime=dict(filter=True) (every row filtered, H = 8 and 4 model frames) -- are brought to 10 s through
  push_many, then fed the same chunks tick by tick; each step() synchronised before and after, the servers taking turns at going
  first, >= 200 ticks: median, p95, min, max of each, what each enqueues per step (the same number: asserted), the frames a row
  got.  The yardstick is the unfiltered column of the same run -> profiles/live_refilter.json.
  --leg snapshot: what LiveServer.snapshot_many() of all rows and restore() of one row cost, per rows in {1, 8, 32, 64}: a server with
  every stage on, medians over `--steps` repeats beside the median step() of the same process; the figure to look at is
  snapshot_many at 64 rows as a fraction of the 66.7 ms tick and beside that step() -> profiles/live_snapshot.json.
  --leg gaze: what the moving gaze costs a step, per rows in {1, 8, 32, 64}: a plain server and one with gaze=True in ONE process,
  brought to 10 s on the same signals, then fed the same chunks tick by tick, taking turns at going first; on the gaze server
  every row gets a new root-space target on an arc every tick (set_gaze_many of all rows, timed by itself).  Median and p95 of
  step() for both, the median of set_gaze_many, what each enqueues per step; the claim to check: the gaze server's median lies
  within the plain server's own spread of the same run (its p95 minus its median) -> profiles/live_gaze.json.
  --leg styles: what named styles cost, per rows in {1, 8, 32, 64}: a plain server and one with a style bank in ONE process,
  brought to 10 s on the same signals, then fed the same chunks tick by tick, taking turns at going first; every tick every row
  gets a new style -- ONE set_style_many of two-term named mixes on the bank server, a loop of tensor set_style calls on the
  plain one, each timed by itself.  Both columns and their ratio, median and p95 of step() for both (the claim to check: the bank
  server's median lies within the plain server's own spread), and at 1 row add_style() of a 600-frame and a 7 200-frame
  exemplar beside the tick -> profiles/live_styles.json.
  --leg plant: what feet that stay planted cost a step, per rows in {1, 8, 32, 64}: a server without the head, a plain-head server
  and a planting server (frames=..., plant=... with thresholds the test networks' motion meets, so that chains are held and
  solved) in ONE process, brought to 10 s on the same signals, then fed the same chunks tick by tick, taking turns at going
  first.  Median and p95 of step() for the three, the stage's added cost beside the head's own (head minus no head), the share
  of contact flags that were set, what each enqueues per step -> profiles/live_plant.json.

Every case is a child process under its own `timeout`; the first one that fails ends the run (as a chain of `&&` would).

    python tools/live_bench.py [--out profiles/live_stream.json] [--steps 200] [--rows 1,8,32,64] [--ages 10,600]
    python tools/live_bench.py --leg push_many [--out profiles/live_push_many.json] [--steps 200] [--rows 1,8,32,64]
    python tools/live_bench.py --leg loudness [--out profiles/live_loudness.json] [--steps 200] [--rows 1,8,32,64] [--ages 10,600]
    python tools/live_bench.py --leg resample [--out profiles/live_resample.json] [--steps 200] [--rows 1,8,32,64] [--ages 10,600]
    python tools/live_bench.py --leg frames [--out profiles/live_frames.json] [--steps 200] [--rows 1,8,32,64] [--ages 10,600]
    python tools/live_bench.py --leg retime [--out profiles/live_retime.json] [--steps 200] [--rows 1,8,32,64]
    python tools/live_bench.py --leg refilter [--out profiles/live_refilter.json] [--steps 200] [--rows 1,8,32,64]
    python tools/live_bench.py --leg snapshot [--out profiles/live_snapshot.json] [--steps 200] [--rows 1,8,32,64]
    python tools/live_bench.py --leg gaze [--out profiles/live_gaze.json] [--steps 200] [--rows 1,8,32,64]
    python tools/live_bench.py --leg styles [--out profiles/live_styles.json] [--steps 200] [--rows 1,8,32,64]
    python tools/live_bench.py --leg plant [--out profiles/live_plant.json] [--steps 200] [--rows 1,8,32,64]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ubisoft-laforge-zeroeggs_amd"), str(ROOT / "tests")]

TICK, FS, FPS = 4, 16000, 60.0
CONF = dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True, normalize_mel_bins=True,
            normalize_range=True, min_clipping=1e-5, sampling_rate=FS, mel_fmin=20, mel_fmax=7600, n_mel_channels=80,
            filter_length=800, hop_length=200, resample_method="linear", normalize_loudness=False)


def _summary(ts):
    ts = sorted(ts)
    ms = lambda x: round(1e3 * x, 4)  # noqa: E731
    return dict(n=len(ts), median_ms=ms(statistics.median(ts)), p95_ms=ms(ts[min(len(ts) - 1, int(0.95 * len(ts)))]),
                min_ms=ms(ts[0]), max_ms=ms(ts[-1]))


def _setup():
    import numpy as np
    import torch
    import helpers
    from zeggs import anim, synth
    se, de, _ = helpers.build_nets()
    dev = "cuda:0"
    stats = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32, device=dev) for k, v in synth.make_stats().items()}
    first = anim.preprocess_animation(synth.make_bvh_clip(8, seed=3), dev)
    base = [synth.synth_wav(4 * FS, seed=s).astype(np.float32) / 32768.0 for s in range(4)]      # 4 s of speech-like noise, looped
    return se.to(dev).eval(), de.to(dev).eval(), stats, first, base


def _samples(base, r, lo, hi):
    """samples [lo, hi) of row r's endless signal"""
    import numpy as np
    w = base[r % len(base)]
    idx = (np.arange(lo, hi) + 977 * r) % len(w)
    return w[idx]


def case_server(rows, age, steps):
    import torch
    from zeggs import live, synth
    se, de, stats, first, base = _setup()
    srv = live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK)
    gen = torch.Generator("cpu").manual_seed(0)
    sids = [srv.open(first, torch.randn(1, 64, generator=gen) * 0.5) for _ in range(rows)]
    pos = 0
    while pos < age * FS:                                  # bring every row to the age
        for r, sid in enumerate(sids):
            srv.push(sid, _samples(base, r, pos, pos + FS))
        pos += FS
        srv.drain()
    torch.cuda.synchronize()
    t_step, t_push, i = [], [], 0
    while len(t_step) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        t0 = time.perf_counter()
        for r, sid in enumerate(sids):
            srv.push(sid, _samples(base, r, pos, nxt))
        torch.cuda.synchronize()
        t_push.append(time.perf_counter() - t0)
        pos = nxt
        while True:
            t0 = time.perf_counter()
            out = srv.step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if not out:
                break
            assert len(out) == rows
            t_step.append(dt)
    from zeggs import ops
    return dict(kind="server", rows=rows, age_s=age, tick=TICK, step=_summary(t_step), pushes_per_tick=_summary(t_push),
                launches_per_step=srv.stats["launches_per_step"], decoder_path=ops.batch_last_path() if rows > 1 else "B=1",
                redone_steps=srv.redone_steps, window_capacity=srv.stats["window_capacity"][0], ring_bytes_per_row=srv.stats["ring_bytes"] // rows,
                uploaded_samples=srv.stats["uploaded_samples"])


def case_push_many(rows, steps, age=10):
    import torch
    from zeggs import live, synth
    se, de, stats, first, base = _setup()
    gen = torch.Generator("cpu").manual_seed(0)
    styles = [torch.randn(1, 64, generator=gen) * 0.5 for _ in range(rows)]
    srv = {k: live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK) for k in ("push", "push_many")}
    sids = {k: [s.open(first, st) for st in styles] for k, s in srv.items()}

    def feed(k, lo, hi):
        if k == "push":
            for r, sid in enumerate(sids[k]):
                srv[k].push(sid, _samples(base, r, lo, hi))
        else:
            srv[k].push_many({sid: _samples(base, r, lo, hi) for r, sid in enumerate(sids[k])})

    pos = 0
    while pos < age * FS:                                  # bring every row of both servers to the age
        for k in srv:
            feed(k, pos, pos + FS)
            srv[k].drain()
        pos += FS
    torch.cuda.synchronize()
    t = {k: dict(push=[], step=[]) for k in srv}
    ops_seen, i = set(), 0
    while len(t["push_many"]["step"]) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        for k in (("push", "push_many") if i % 2 else ("push_many", "push")):      # taking turns at going first
            chunks = [_samples(base, r, pos, nxt) for r in range(rows)]            # (the slicing is not what is timed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if k == "push":
                for sid, c in zip(sids[k], chunks):
                    srv[k].push(sid, c)
            else:
                srv[k].push_many(dict(zip(sids[k], chunks)))
            torch.cuda.synchronize()
            t[k]["push"].append(time.perf_counter() - t0)
            if k == "push_many":
                ops_seen.add(srv[k].stats["ops_last_push_many"])
            while True:
                t0 = time.perf_counter()
                out = srv[k].step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if not out:
                    break
                assert len(out) == rows
                t[k]["step"].append(dt)
        pos = nxt
    a, b = srv["push"], srv["push_many"]
    same = all((x.n, x.base, x.n_feat, x.fbase, x.n_ring, x.kd) == (y.n, y.base, y.n_feat, y.fbase, y.n_ring, y.kd)
               for x, y in zip(a._rows, b._rows))
    same = same and all(torch.equal(a.feats[r, w.n_ring - w.fbase:w.n_feat - w.fbase].view(torch.int32),
                                    b.feats[r, w.n_ring - w.fbase:w.n_feat - w.fbase].view(torch.int32)) for r, w in enumerate(a._rows))
    return dict(kind="push_many", rows=rows, age_s=age, tick=TICK, pushes_per_tick=_summary(t["push"]["push"]),
                push_many_per_tick=_summary(t["push_many"]["push"]), step_beside_push=_summary(t["push"]["step"]),
                step_beside_push_many=_summary(t["push_many"]["step"]), ops_per_push_many=sorted(ops_seen),
                pending_features_bitwise_equal=bool(same))


def case_loudness(rows, age, steps):
    """push_many with running loudness off and on: two servers in ONE process, the same rows' signals up to `age` (1 s
    push_many calls, drained), then tick by tick the same chunks, each call synchronised before and after, taking turns"""
    import torch
    from zeggs import live, synth
    se, de, stats, first, base = _setup()
    gen = torch.Generator("cpu").manual_seed(0)
    styles = [torch.randn(1, 64, generator=gen) * 0.5 for _ in range(rows)]
    srv = {k: live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK, loudness=v) for k, v in (("off", None), ("on", "running"))}
    sids = {k: [s.open(first, st) for st in styles] for k, s in srv.items()}
    pos = 0
    while pos < age * FS:
        for k in srv:
            srv[k].push_many({sid: _samples(base, r, pos, pos + FS) for r, sid in enumerate(sids[k])})
            srv[k].drain()
        pos += FS
    torch.cuda.synchronize()
    t = {k: dict(push=[], step=[]) for k in srv}
    ops_seen, i = {k: set() for k in srv}, 0
    while len(t["on"]["step"]) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        chunks = [_samples(base, r, pos, nxt) for r in range(rows)]                # (the slicing is not what is timed)
        for k in (("off", "on") if i % 2 else ("on", "off")):                      # taking turns at going first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            srv[k].push_many(dict(zip(sids[k], chunks)))
            torch.cuda.synchronize()
            t[k]["push"].append(time.perf_counter() - t0)
            ops_seen[k].add(srv[k].stats["ops_last_push_many"])
            while True:
                t0 = time.perf_counter()
                out = srv[k].step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if not out:
                    break
                assert len(out) == rows
                t[k]["step"].append(dt)
        pos = nxt
    state = srv["on"].loudness(sids["on"][0])
    return dict(kind="loudness", rows=rows, age_s=age, tick=TICK, samples_per_row_and_tick=round(TICK * FS / FPS, 1),
                push_many_off=_summary(t["off"]["push"]), push_many_on=_summary(t["on"]["push"]), step_off=_summary(t["off"]["step"]),
                step_on=_summary(t["on"]["step"]), ops_per_push_many_off=sorted(ops_seen["off"]), ops_per_push_many_on=sorted(ops_seen["on"]),
                row0_state=dict(lufs=round(state["lufs"], 4), gain=round(state["gain"], 6), blocks=state["blocks"], gated=state["gated"]))


def case_resample(rows, age, steps, fi=48000):
    """push_many on native float32 rows and on rows opened at 48 kHz s16, with running loudness off and on: four servers in ONE
    process, the same rows' signals up to `age` (1 s push_many calls, drained), then tick by tick, each call synchronised before
    and after, taking turns at going first"""
    import numpy as np
    import torch
    from zeggs import live, synth
    se, de, stats, first, base = _setup()
    up = fi // FS
    pcm = [np.round(w * 32767.0).astype(np.int16) for w in base]

    def chunk(kind, r, lo, hi):
        if kind == "native":
            return _samples(base, r, lo, hi)
        w = pcm[r % len(pcm)]                                                      # sample and hold: `up` raw samples per native one
        return w[(np.arange(up * lo, up * hi) // up + 977 * r) % len(w)]

    gen = torch.Generator("cpu").manual_seed(0)
    styles = [torch.randn(1, 64, generator=gen) * 0.5 for _ in range(rows)]
    kinds = [(k, l) for l in ("off", "on") for k in ("native", "s16")]
    srv = {kl: live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK, loudness="running" if kl[1] == "on" else None) for kl in kinds}
    sids = {kl: [s.open(first, st, **(dict(rate=fi, pcm="s16") if kl[0] == "s16" else {})) for st in styles] for kl, s in srv.items()}
    pos = 0
    while pos < age * FS:
        for kl in kinds:
            srv[kl].push_many({sid: chunk(kl[0], r, pos, pos + FS) for r, sid in enumerate(sids[kl])})
            srv[kl].drain()
        pos += FS
    torch.cuda.synchronize()
    t = {kl: dict(push=[], step=[]) for kl in kinds}
    ops_seen, i = {kl: set() for kl in kinds}, 0
    bytes0 = {kl: srv[kl].stats["uploaded_bytes"] for kl in kinds}
    while len(t[kinds[-1]]["push"]) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        chunks = {k: [chunk(k, r, pos, nxt) for r in range(rows)] for k in ("native", "s16")}      # (the slicing is not what is timed)
        for kl in kinds[i % 4:] + kinds[:i % 4]:                                   # taking turns at going first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            srv[kl].push_many(dict(zip(sids[kl], chunks[kl[0]])))
            torch.cuda.synchronize()
            t[kl]["push"].append(time.perf_counter() - t0)
            ops_seen[kl].add(srv[kl].stats["ops_last_push_many"])
            while True:
                t0 = time.perf_counter()
                out = srv[kl].step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if not out:
                    break
                assert len(out) == rows
                t[kl]["step"].append(dt)
        pos = nxt
    res = dict(kind="resample", rows=rows, age_s=age, tick=TICK, input_rate=fi, samples_per_row_and_tick=round(TICK * FS / FPS, 1),
               raw_samples_per_row_and_tick=round(TICK * fi / FPS, 1))
    for k, l in kinds:
        res[f"push_many_{k}_loudness_{l}"] = _summary(t[(k, l)]["push"])
        res[f"step_{k}_loudness_{l}"] = _summary(t[(k, l)]["step"])
        res[f"ops_per_push_many_{k}_loudness_{l}"] = sorted(ops_seen[(k, l)])
        res[f"uploaded_bytes_per_tick_{k}_loudness_{l}"] = round((srv[(k, l)].stats["uploaded_bytes"] - bytes0[(k, l)]) / len(t[(k, l)]["push"]))
    for l in ("off", "on"):
        res[f"s16_over_native_loudness_{l}"] = round(res[f"push_many_s16_loudness_{l}"]["median_ms"] / res[f"push_many_native_loudness_{l}"]["median_ms"], 3)
    return res


def case_frames(rows, age, steps):
    """step() with the output head off and on (local, world, bvh), and the client-side conversion of the plain server's output:
    two servers in ONE process, the same rows' signals up to `age` (1 s push_many calls, drained), then tick by tick"""
    import torch
    from zeggs import anim, live, synth
    se, de, stats, first, base = _setup()
    gen = torch.Generator("cpu").manual_seed(0)
    styles = [torch.randn(1, 64, generator=gen) * 0.5 for _ in range(rows)]
    head = dict(parents=synth.PARENTS, names=synth.BONE_NAMES, what=("local", "world", "bvh"), order="zyx", text=False)
    srv = {k: live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK, frames=v) for k, v in (("off", None), ("on", head))}
    sids = {k: [s.open(first, st, **(dict(start_position=[0.0, 0.0, 0.0], start_rotation=[1.0, 0.0, 0.0, 0.0]) if k == "on" else {}))
                for st in styles] for k, s in srv.items()}
    pos = 0
    while pos < age * FS:
        for k in srv:
            srv[k].push_many({sid: _samples(base, r, pos, pos + FS) for r, sid in enumerate(sids[k])})
            srv[k].drain()
        pos += FS
    torch.cuda.synchronize()
    J = len(synth.PARENTS)
    t = {k: [] for k in ("off", "on", "client")}
    ops_seen, i = {k: set() for k in srv}, 0
    bytes0 = srv["on"].stats["frame_bytes"]
    while len(t["on"]) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        chunks = [_samples(base, r, pos, nxt) for r in range(rows)]
        for k in (("off", "on") if i % 2 else ("on", "off")):                      # taking turns at going first
            srv[k].push_many(dict(zip(sids[k], chunks)))
            while True:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = srv[k].step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if not out:
                    break
                assert len(out) == rows and ("frames" in out[sids[k][0]]) == (k == "on")
                t[k].append(dt)
                ops_seen[k].add(srv[k].stats["launches_per_step"])
                if k == "off":                                                     # what a client does with it today, per stream
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for o in out.values():
                        n = o["pose"].shape[0]
                        p, e = anim.bvh_channels(o["rpos"], o["rrot"], o["pose"][:, 6:6 + 3 * J].reshape(n, J, 3),
                                                 o["pose"][:, 6 + 3 * J:6 + 9 * J].reshape(n, J, 2, 3), [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])
                        p, e = p.cpu(), e.cpu()
                    t["client"].append(time.perf_counter() - t0)
        pos = nxt
    assert ops_seen["on"] == {x + 2 for x in ops_seen["off"]} and len(ops_seen["on"]) == 1, (ops_seen)
    return dict(kind="frames", rows=rows, age_s=age, tick=TICK, step_off=_summary(t["off"]), step_on=_summary(t["on"]),
                client_bvh_channels_and_cpu=_summary(t["client"]), launches_per_step_off=sorted(ops_seen["off"]),
                launches_per_step_on=sorted(ops_seen["on"]), frame_bytes_per_step=round((srv["on"].stats["frame_bytes"] - bytes0) / len(t["on"])))


RETIME_LEGS = (("plain", None), ("1/1", 60), ("1/2", 30), ("2/1", 120))


def case_retime(rows, steps, age=10):
    """step() with the plain head and with the re-timing head, every row at 1 / 1, 1 / 2 and 2 / 1 (local, world, bvh): four servers
    in ONE process, the same rows' signals up to `age` (1 s push_many calls, drained), then tick by tick, taking turns"""
    import torch
    from zeggs import live, synth
    se, de, stats, first, base = _setup()
    gen = torch.Generator("cpu").manual_seed(0)
    styles = [torch.randn(1, 64, generator=gen) * 0.5 for _ in range(rows)]
    head = dict(parents=synth.PARENTS, names=synth.BONE_NAMES, what=("local", "world", "bvh"), order="zyx", text=False)
    place = dict(start_position=[0.0, 0.0, 0.0], start_rotation=[1.0, 0.0, 0.0, 0.0])
    srv = {k: live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK, frames=head, retime=None if rate is None else dict(max_rate=120))
           for k, rate in RETIME_LEGS}
    sids = {k: [srv[k].open(first, st, **place, **({} if rate is None else dict(frame_rate=rate))) for st in styles] for k, rate in RETIME_LEGS}
    pos = 0
    while pos < age * FS:
        for k in srv:
            srv[k].push_many({sid: _samples(base, r, pos, pos + FS) for r, sid in enumerate(sids[k])})
            srv[k].drain()
        pos += FS
    torch.cuda.synchronize()
    names = [k for k, _ in RETIME_LEGS]
    t, frames = {k: [] for k in names}, {k: 0 for k in names}
    ops_seen, i = {k: set() for k in names}, 0
    bytes0 = {k: srv[k].stats["frame_bytes"] for k in names}
    while len(t["plain"]) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        chunks = [_samples(base, r, pos, nxt) for r in range(rows)]
        for k in names[i % 4:] + names[:i % 4]:                                    # taking turns at going first
            srv[k].push_many(dict(zip(sids[k], chunks)))
            while True:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = srv[k].step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if not out:
                    break
                assert len(out) == rows
                t[k].append(dt)
                frames[k] += out[sids[k][0]]["frames"]["bvh"].shape[0]
                ops_seen[k].add(srv[k].stats["launches_per_step"])
        pos = nxt
    assert len({tuple(sorted(v)) for v in ops_seen.values()}) == 1 and len(ops_seen["plain"]) == 1, ops_seen
    n = len(t["plain"])
    assert frames["plain"] == frames["1/1"] == n * TICK and abs(frames["1/2"] * 2 - n * TICK) <= 2 and abs(frames["2/1"] - 2 * n * TICK) <= 2, frames
    return dict(kind="retime", rows=rows, age_s=age, tick=TICK, launches_per_step=sorted(ops_seen["plain"]),
                step={k: _summary(t[k]) for k in names}, frames_per_row={k: frames[k] for k in names},
                frame_bytes_per_step={k: round((srv[k].stats["frame_bytes"] - bytes0[k]) / len(t[k])) for k in names})


def case_gaze(rows, steps, age=10):
    """step() of a server with the moving gaze against step() of a plain one, and a set_gaze_many of all rows: two servers in ONE
    process, the same rows' signals up to `age` (1 s push_many calls, drained), then tick by tick, taking turns at going first.
    On the gaze server every row gets a new target every tick (a tracker's call: root space, an arc, a fade of 12), timed by
    itself in front of the step"""
    import torch
    from zeggs import live, synth
    se, de, stats, first, base = _setup()
    gen = torch.Generator("cpu").manual_seed(0)
    styles = [torch.randn(1, 64, generator=gen) * 0.5 for _ in range(rows)]
    srv = {"plain": live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK),
           "gaze": live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK, gaze=True)}
    sids = {k: [srv[k].open(first, st) for st in styles] for k in srv}
    pos = 0
    while pos < age * FS:
        for k in srv:
            srv[k].push_many({sid: _samples(base, r, pos, pos + FS) for r, sid in enumerate(sids[k])})
            srv[k].drain()
        pos += FS
    torch.cuda.synchronize()
    names = ["plain", "gaze"]
    t, t_set, ops_seen, i = {k: [] for k in names}, [], {k: set() for k in names}, 0
    while len(t["plain"]) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        chunks = [_samples(base, r, pos, nxt) for r in range(rows)]
        for k in names[i % 2:] + names[:i % 2]:
            srv[k].push_many(dict(zip(sids[k], chunks)))
            if k == "gaze":
                req = {sid: dict(target=[0.5 * ((i + r) % 5) - 1.0, 1.6, 2.0], fade=12, space="root", path="arc") for r, sid in enumerate(sids[k])}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                srv[k].set_gaze_many(req)
                torch.cuda.synchronize()
                t_set.append(time.perf_counter() - t0)
            while True:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = srv[k].step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if not out:
                    break
                assert len(out) == rows
                t[k].append(dt)
                ops_seen[k].add(srv[k].stats["launches_per_step"])
        pos = nxt
    assert len(ops_seen["plain"]) == len(ops_seen["gaze"]) == 1 and max(ops_seen["gaze"]) <= max(ops_seen["plain"]), ops_seen
    return dict(kind="gaze", rows=rows, age_s=age, tick=TICK, step={k: _summary(t[k]) for k in names}, set_gaze_many=_summary(t_set),
                launches_per_step={k: sorted(ops_seen[k]) for k in names}, ops_per_set_gaze_many=srv["gaze"].stats["ops_last_set_gaze"])


# thresholds the test networks' motion meets now and then (NOT a tuning for captured motion): chains are held, solved and released
PLANT_BENCH = dict(chains="auto", speed=(60.0, 120.0), height=(1e6, 2e6), ground=0.0, slack=3.0, release=5, stretch=0.999)


def case_plant(rows, steps, age=10):
    """step() of a server without the head, of a plain-head server and of a planting server: three servers in ONE process, the
    same rows' signals up to `age` (1 s push_many calls, drained), then tick by tick, taking turns at going first"""
    import torch
    from zeggs import live, synth
    se, de, stats, first, base = _setup()
    gen = torch.Generator("cpu").manual_seed(0)
    styles = [torch.randn(1, 64, generator=gen) * 0.5 for _ in range(rows)]
    head = dict(parents=synth.PARENTS, names=synth.BONE_NAMES, what=("local", "world", "bvh"), order="zyx", text=False)
    srv = {"no head": live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK),
           "head": live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK, frames=head),
           "plant": live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK, frames=head, plant=PLANT_BENCH)}
    sids = {k: [srv[k].open(first, st) for st in styles] for k in srv}
    pos = 0
    while pos < age * FS:
        for k in srv:
            srv[k].push_many({sid: _samples(base, r, pos, pos + FS) for r, sid in enumerate(sids[k])})
            srv[k].drain()
        pos += FS
    torch.cuda.synchronize()
    names = list(srv)
    t, ops_seen, i, flags, held = {k: [] for k in names}, {k: set() for k in names}, 0, 0, 0
    while len(t["head"]) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        chunks = [_samples(base, r, pos, nxt) for r in range(rows)]
        for k in names[i % 3:] + names[:i % 3]:
            srv[k].push_many(dict(zip(sids[k], chunks)))
            while True:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = srv[k].step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if not out:
                    break
                assert len(out) == rows
                t[k].append(dt)
                ops_seen[k].add(srv[k].stats["launches_per_step"])
                if k == "plant":
                    for o in out.values():
                        flags, held = flags + o["contacts"].size, held + int(o["contacts"].sum())
        pos = nxt
    assert all(len(v) == 1 for v in ops_seen.values()) and max(ops_seen["plant"]) == max(ops_seen["head"]) + 1, ops_seen
    return dict(kind="plant", rows=rows, age_s=age, tick=TICK, step={k: _summary(t[k]) for k in names}, contact_share=round(held / max(flags, 1), 4),
                launches_per_step={k: sorted(ops_seen[k]) for k in names})


def case_styles(rows, steps, age=10):
    """what named styles cost: a plain server and one with a style bank in ONE process, the same rows' signals up to `age` (1 s
    push_many calls, drained), then tick by tick, taking turns at going first.  Every tick every row gets a new style: on the
    bank server a two-term named mix by ONE set_style_many, on the plain server the same number of tensor set_style calls in a
    loop (vectors already on the device), each timed by itself in front of the step.  At rows == 1 also add_style() of a
    600-frame and a 7 200-frame exemplar through a style encoder of the flagship widths, beside the tick"""
    import numpy as np
    import torch
    from zeggs import live, modules, synth
    se, de, stats, first, base = _setup()
    gen = torch.Generator("cpu").manual_seed(0)
    styles = [torch.randn(1, 64, generator=gen) * 0.5 for _ in range(rows)]
    torch.manual_seed(1234)
    net = modules.StyleEncoder(synth.POSE_IN, 512, 64, type="attn", use_vae=True).to("cuda:0").eval()
    srv = {"plain": live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK),
           "bank": live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK, styles=dict(net=net, capacity=16))}
    vectors = [(torch.randn(128, generator=gen) * 0.5).to("cuda:0") for _ in range(8)]
    for j, v in enumerate(vectors):
        srv["bank"].add_style(f"s{j}", v)
    tensors = [v[:64].contiguous() for v in vectors]
    sids = {"plain": [srv["plain"].open(first, st) for st in styles], "bank": [srv["bank"].open(first, f"s{r % 8}") for r in range(rows)]}
    pos = 0
    while pos < age * FS:
        for k in srv:
            srv[k].push_many({sid: _samples(base, r, pos, pos + FS) for r, sid in enumerate(sids[k])})
            srv[k].drain()
        pos += FS
    torch.cuda.synchronize()
    names = ["plain", "bank"]
    t, t_set, ops_seen, i = {k: [] for k in names}, {k: [] for k in names}, {k: set() for k in names}, 0
    while len(t["plain"]) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        chunks = [_samples(base, r, pos, nxt) for r in range(rows)]
        for k in names[i % 2:] + names[:i % 2]:
            srv[k].push_many(dict(zip(sids[k], chunks)))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if k == "bank":
                srv[k].set_style_many({sid: dict(style={f"s{(i + r) % 8}": 0.7, f"s{(i + r + 3) % 8}": 0.3}, fade=12) for r, sid in enumerate(sids[k])})
            else:
                for r, sid in enumerate(sids[k]):
                    srv[k].set_style(sid, tensors[(i + r) % 8], fade=12)
            torch.cuda.synchronize()
            t_set[k].append(time.perf_counter() - t0)
            while True:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = srv[k].step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if not out:
                    break
                assert len(out) == rows
                t[k].append(dt)
                ops_seen[k].add(srv[k].stats["launches_per_step"])
        pos = nxt
    assert len(ops_seen["plain"]) == len(ops_seen["bank"]) == 1 and ops_seen["bank"] == ops_seen["plain"], ops_seen
    res = dict(kind="styles", rows=rows, age_s=age, tick=TICK, step={k: _summary(t[k]) for k in names},
               set_style={"tensor_loop": _summary(t_set["plain"]), "named_many": _summary(t_set["bank"])},
               launches_per_step={k: sorted(ops_seen[k]) for k in names}, ops_per_set_style_many=srv["bank"].stats["ops_last_set_style"])
    if rows == 1:
        st = synth.make_stats()
        add = {}
        for L in (600, 7200):
            c = synth.make_clip_stats(L, seed=L, stats=st)
            ex = np.concatenate([c["Y_root_vel"], c["Y_root_vrt"], c["Y_lpos"].reshape(L, -1), c["Y_ltxy"].reshape(L, -1),
                                 c["Y_lvel"].reshape(L, -1), c["Y_lvrt"].reshape(L, -1), np.zeros((L, 3), np.float32)], axis=1)
            ex = torch.as_tensor(ex, dtype=torch.float32, device="cuda:0")
            srv["bank"].add_style("example", ex)          # (the first call at a length builds what the encoder keeps per length)
            ts = []
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                srv["bank"].add_style("example", ex)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            add[f"{L} frames"] = _summary(ts)
        res["add_style_of_exemplar_rows_on_the_device"] = add
    return res


REFILTER_LEGS = (("30", 30, False), ("120", 120, False), ("30 filtered", 30, True), ("120 filtered", 120, True))


def case_refilter(rows, steps, age=10):
    """step() with the re-timing head without and with its filter stage, every row at 30 and at 120 frames a second (local, world,
    bvh): four servers in ONE process, the same rows' signals up to `age` (1 s push_many calls, drained), then tick by tick,
    taking turns"""
    import torch
    from zeggs import live, synth
    se, de, stats, first, base = _setup()
    gen = torch.Generator("cpu").manual_seed(0)
    styles = [torch.randn(1, 64, generator=gen) * 0.5 for _ in range(rows)]
    head = dict(parents=synth.PARENTS, names=synth.BONE_NAMES, what=("local", "world", "bvh"), order="zyx", text=False)
    place = dict(start_position=[0.0, 0.0, 0.0], start_rotation=[1.0, 0.0, 0.0, 0.0])
    srv = {k: live.LiveServer(se, de, stats, CONF, synth.DT, rows=rows, tick=TICK, frames=head,
                              retime=dict(max_rate=120, filter=True) if filt else dict(max_rate=120)) for k, _, filt in REFILTER_LEGS}
    sids = {k: [srv[k].open(first, st, **place, frame_rate=rate) for st in styles] for k, rate, _ in REFILTER_LEGS}
    delay = {k: srv[k].frame_delay(sids[k][0])[0] for k in srv}
    pos = 0
    while pos < age * FS:
        for k in srv:
            srv[k].push_many({sid: _samples(base, r, pos, pos + FS) for r, sid in enumerate(sids[k])})
            srv[k].drain()
        pos += FS
    torch.cuda.synchronize()
    names = [k for k, _, _ in REFILTER_LEGS]
    t, frames = {k: [] for k in names}, {k: 0 for k in names}
    ops_seen, i = {k: set() for k in names}, 0
    while len(t[names[0]]) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        chunks = [_samples(base, r, pos, nxt) for r in range(rows)]
        for k in names[i % 4:] + names[:i % 4]:                                    # taking turns at going first
            srv[k].push_many(dict(zip(sids[k], chunks)))
            while True:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = srv[k].step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if not out:
                    break
                assert len(out) == rows
                t[k].append(dt)
                frames[k] += out[sids[k][0]]["frames"]["bvh"].shape[0]
                ops_seen[k].add(srv[k].stats["launches_per_step"])
        pos = nxt
    assert len({tuple(sorted(v)) for v in ops_seen.values()}) == 1 and len(ops_seen[names[0]]) == 1, ops_seen
    n = len(t[names[0]])
    assert abs(frames["30"] * 2 - n * TICK) <= 2 and abs(frames["120"] - 2 * n * TICK) <= 2, frames
    assert abs(frames["30 filtered"] - frames["30"]) <= 1 and abs(frames["120 filtered"] - frames["120"]) <= 1, frames      # the filter only delays
    return dict(kind="refilter", rows=rows, age_s=age, tick=TICK, launches_per_step=sorted(ops_seen[names[0]]), delay_frames=delay,
                step={k: _summary(t[k]) for k in names}, frames_per_row={k: frames[k] for k in names})


def case_snapshot(rows, steps, age=10):
    """snapshot_many() of all rows and restore() of one row beside step(), in ONE process: a server with every stage on (running
    loudness, frames with all three outputs, the filtering re-timing head; every row at 24 frames a second, every fourth row
    48 kHz s16) aged `age` seconds; then `steps` ticks, each timed: the step, a snapshot of every row, and the restore of row 0's
    blob into a second server of the same configuration (its row is closed again outside the timing)"""
    import numpy as np
    import torch
    from zeggs import live, synth
    se, de, stats, first, base = _setup()
    gen = torch.Generator("cpu").manual_seed(0)
    styles = [torch.randn(1, 64, generator=gen) * 0.5 for _ in range(rows)]
    head = dict(parents=synth.PARENTS, names=synth.BONE_NAMES, what=("local", "world", "bvh"), order="zyx", text=False)
    kw = dict(rows=rows, tick=TICK, loudness="running", frames=head, retime=dict(max_rate=120, filter=True, min_rate=24))
    srv, dst = (live.LiveServer(se, de, stats, CONF, synth.DT, **kw) for _ in range(2))
    s16 = [r % 4 == 3 for r in range(rows)]
    sids = [srv.open(first, st, frame_rate=24, **(dict(rate=3 * FS, pcm="s16") if c else {})) for st, c in zip(styles, s16)]

    def chunks(lo, hi):
        """row r's samples [lo, hi) at the server's rate; a converting row delivers each of them three times, as int16"""
        out = {}
        for r, sid in enumerate(sids):
            x = _samples(base, r, lo, hi)
            out[sid] = np.repeat(np.round(x * 32767.0).astype(np.int16), 3) if s16[r] else x
        return out
    pos = 0
    while pos < age * FS:
        srv.push_many(chunks(pos, pos + FS))
        srv.drain()
        pos += FS
    torch.cuda.synchronize()
    t = dict(step=[], snapshot_many=[], restore=[])
    blob_bytes, i = 0, 0
    while len(t["step"]) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        srv.push_many(chunks(pos, nxt))
        pos = nxt
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = srv.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if not out:
            continue
        assert len(out) == rows
        t["step"].append(dt)
        t0 = time.perf_counter()
        blobs = srv.snapshot_many()                                 # (returns when the download is there)
        t["snapshot_many"].append(time.perf_counter() - t0)
        assert len(blobs) == rows and srv.stats["ops_last_snapshot"] == 3
        blob_bytes = sum(b.size for b in blobs.values())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        new = dst.restore(blobs[sids[0]])
        torch.cuda.synchronize()
        t["restore"].append(time.perf_counter() - t0)
        dst.close(new)
    return dict(kind="snapshot", rows=rows, age_s=age, tick=TICK, blob_bytes_all_rows=int(blob_bytes), blob_bytes_row_0=int(blobs[sids[0]].size),
                launches_per_step=srv.stats["launches_per_step"], **{k: _summary(v) for k, v in t.items()})


def case_baseline(age, steps):
    import torch
    from zeggs import stream, synth
    se, de, stats, first, base = _setup()
    gs = stream.GestureStream(se, de, first, torch.randn(1, 64, generator=torch.Generator("cpu").manual_seed(0)) * 0.5, stats, CONF,
                              synth.DT)
    pos = 0
    while pos < age * FS:
        gs.push(_samples(base, 0, pos, pos + FS))
        pos += FS
    torch.cuda.synchronize()
    ts, i = [], 0
    while len(ts) < steps:
        i += 1
        nxt = age * FS + int(round(i * TICK * FS / FPS))
        t0 = time.perf_counter()
        out = gs.push(_samples(base, 0, pos, nxt))
        torch.cuda.synchronize()
        if out:
            ts.append(time.perf_counter() - t0)
        pos = nxt
    return dict(kind="gesture_stream_push", rows=1, age_s=age, push=_summary(ts), redone_chunks=gs.redone_chunks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "live_stream.json"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rows", default="1,8,32,64")
    ap.add_argument("--ages", default="10,600")
    ap.add_argument("--limit", type=int, default=420, help="seconds per case")
    ap.add_argument("--leg", default="step", choices=("step", "push_many", "loudness", "resample", "frames", "retime", "refilter", "snapshot", "gaze", "styles", "plant"))
    ap.add_argument("--loudness", action="store_true", help="the same as --leg loudness")
    ap.add_argument("--case", default=None,
                    help="internal: one case in a child process, e.g. server:8:10, baseline:600, push_many:64, loudness:64:600, resample:64:600, frames:64:600, retime:64, refilter:64, snapshot:64, gaze:64, styles:64 or plant:64")
    a = ap.parse_args()
    if a.loudness:
        a.leg = "loudness"
    if a.case:
        kind, *rest = a.case.split(":")
        res = (case_server(int(rest[0]), int(rest[1]), a.steps) if kind == "server" else
               case_push_many(int(rest[0]), a.steps) if kind == "push_many" else
               case_loudness(int(rest[0]), int(rest[1]), a.steps) if kind == "loudness" else
               case_resample(int(rest[0]), int(rest[1]), a.steps) if kind == "resample" else
               case_frames(int(rest[0]), int(rest[1]), a.steps) if kind == "frames" else
               case_retime(int(rest[0]), a.steps) if kind == "retime" else
               case_refilter(int(rest[0]), a.steps) if kind == "refilter" else
               case_snapshot(int(rest[0]), a.steps) if kind == "snapshot" else
               case_gaze(int(rest[0]), a.steps) if kind == "gaze" else
               case_styles(int(rest[0]), a.steps) if kind == "styles" else
               case_plant(int(rest[0]), a.steps) if kind == "plant" else case_baseline(int(rest[0]), a.steps))
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    ages, rows = [int(x) for x in a.ages.split(",")], [int(x) for x in a.rows.split(",")]
    cases = [f"baseline:{g}" for g in ages] + [f"server:{r}:{g}" for r in rows for g in ages]
    if a.leg == "push_many":
        cases = [f"push_many:{r}" for r in rows]
        if a.out == ap.get_default("out"):
            a.out = str(ROOT / "profiles" / "live_push_many.json")
    if a.leg == "loudness":
        cases = [f"loudness:{r}:{g}" for r in rows for g in ages]
        if a.out == ap.get_default("out"):
            a.out = str(ROOT / "profiles" / "live_loudness.json")
    if a.leg == "resample":
        cases = [f"resample:{r}:{g}" for r in rows for g in ages]
        if a.out == ap.get_default("out"):
            a.out = str(ROOT / "profiles" / "live_resample.json")
    if a.leg == "frames":
        cases = [f"frames:{r}:{g}" for r in rows for g in ages]
        if a.out == ap.get_default("out"):
            a.out = str(ROOT / "profiles" / "live_frames.json")
    if a.leg == "retime":
        cases = [f"retime:{r}" for r in rows]
        if a.out == ap.get_default("out"):
            a.out = str(ROOT / "profiles" / "live_retime.json")
    if a.leg == "refilter":
        cases = [f"refilter:{r}" for r in rows]
        if a.out == ap.get_default("out"):
            a.out = str(ROOT / "profiles" / "live_refilter.json")
    if a.leg == "snapshot":
        cases = [f"snapshot:{r}" for r in rows]
        if a.out == ap.get_default("out"):
            a.out = str(ROOT / "profiles" / "live_snapshot.json")
    if a.leg == "gaze":
        cases = [f"gaze:{r}" for r in rows]
        if a.out == ap.get_default("out"):
            a.out = str(ROOT / "profiles" / "live_gaze.json")
    if a.leg == "styles":
        cases = [f"styles:{r}" for r in rows]
        if a.out == ap.get_default("out"):
            a.out = str(ROOT / "profiles" / "live_styles.json")
    if a.leg == "plant":
        cases = [f"plant:{r}" for r in rows]
        if a.out == ap.get_default("out"):
            a.out = str(ROOT / "profiles" / "live_plant.json")
    results = []
    for c in cases:                 # each GPU case under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--case", c, "--steps", str(a.steps)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(f"case {c} ended with status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return p.returncode
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        results.append(json.loads(line[7:]))
        print(c, line[7:], flush=True)
    import torch
    if a.leg == "push_many":
        pays = [r["rows"] for r in results if r["push_many_per_tick"]["median_ms"] < r["pushes_per_tick"]["median_ms"]]
        rec = dict(command="python tools/live_bench.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0),
                   tick_frames=TICK, ticks_per_case=a.steps, row_counts_at_which_push_many_is_faster=pays, results=results)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {a.out}")
        return 0
    if a.leg == "loudness":
        cost, age_effect = {}, {}
        for n in rows:
            mine = {r["age_s"]: r for r in results if r["rows"] == n}
            lo = mine[ages[0]]
            cost[str(n)] = dict(push_many_off_median_ms=lo["push_many_off"]["median_ms"], push_many_on_median_ms=lo["push_many_on"]["median_ms"],
                                added_ms=round(lo["push_many_on"]["median_ms"] - lo["push_many_off"]["median_ms"], 4))
            if len(ages) >= 2:
                hi = mine[ages[-1]]
                spread = max(x["push_many_on"]["p95_ms"] - x["push_many_on"]["min_ms"] for x in (lo, hi))
                age_effect[str(n)] = dict(median_ms_young=lo["push_many_on"]["median_ms"], median_ms_old=hi["push_many_on"]["median_ms"],
                                          spread_ms=round(spread, 4), differs_by_more_than_the_spread=abs(
                                              hi["push_many_on"]["median_ms"] - lo["push_many_on"]["median_ms"]) > spread)
        rec = dict(command="python tools/live_bench.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), tick_frames=TICK,
                   ticks_per_case=a.steps, cost_of_running_loudness_per_push_many=cost, age_effect_on_push_many_with_loudness=age_effect,
                   results=results)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {a.out}")
        return 0
    if a.leg == "resample":
        cost = {}
        for r in results:
            cost[f"{r['rows']} rows, {r['age_s']} s"] = {
                f"loudness_{l}": dict(native_median_ms=r[f"push_many_native_loudness_{l}"]["median_ms"],
                                      s16_48k_median_ms=r[f"push_many_s16_loudness_{l}"]["median_ms"],
                                      added_ms=round(r[f"push_many_s16_loudness_{l}"]["median_ms"] - r[f"push_many_native_loudness_{l}"]["median_ms"], 4),
                                      s16_over_native=r[f"s16_over_native_loudness_{l}"]) for l in ("off", "on")}
        rec = dict(command="python tools/live_bench.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), tick_frames=TICK,
                   ticks_per_case=a.steps, push_many_native_against_48k_s16=cost, results=results)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {a.out}")
        return 0
    if a.leg == "frames":
        table, age_effect = {}, {}
        for r in results:
            table[f"{r['rows']} rows, {r['age_s']} s"] = dict(
                step_off_median_ms=r["step_off"]["median_ms"], step_off_p95_ms=r["step_off"]["p95_ms"], step_on_median_ms=r["step_on"]["median_ms"],
                step_on_p95_ms=r["step_on"]["p95_ms"], client_median_ms=r["client_bvh_channels_and_cpu"]["median_ms"],
                client_p95_ms=r["client_bvh_channels_and_cpu"]["p95_ms"],
                head_added_ms=round(r["step_on"]["median_ms"] - r["step_off"]["median_ms"], 4), frame_bytes_per_step=r["frame_bytes_per_step"])
        if len(ages) >= 2:
            for n in rows:
                lo, hi = ([r for r in results if r["rows"] == n and r["age_s"] == g][0]["step_on"] for g in (ages[0], ages[-1]))
                spread = max(lo["p95_ms"] - lo["min_ms"], hi["p95_ms"] - hi["min_ms"])
                age_effect[str(n)] = dict(median_ms_young=lo["median_ms"], median_ms_old=hi["median_ms"], spread_ms=round(spread, 4),
                                          differs_by_more_than_the_spread=abs(hi["median_ms"] - lo["median_ms"]) > spread)
        rec = dict(command="python tools/live_bench.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), tick_frames=TICK,
                   ticks_per_case=a.steps, step_without_and_with_the_head_and_the_client_side_conversion=table,
                   age_effect_on_step_time_with_the_head=age_effect, results=results)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {a.out}")
        return 0
    if a.leg == "retime":
        table = {}
        for r in results:
            table[f"{r['rows']} rows"] = {k: dict(median_ms=v["median_ms"], p95_ms=v["p95_ms"],
                                                  over_plain_ms=round(v["median_ms"] - r["step"]["plain"]["median_ms"], 4),
                                                  frame_bytes_per_step=r["frame_bytes_per_step"][k]) for k, v in r["step"].items()}
        rec = dict(command="python tools/live_bench.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), tick_frames=TICK,
                   ticks_per_case=a.steps, step_with_the_plain_head_and_the_retiming_head=table, results=results)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {a.out}")
        return 0
    if a.leg == "refilter":
        table = {}
        for r in results:
            st = r["step"]
            table[f"{r['rows']} rows"] = {rate: dict(unfiltered_median_ms=st[rate]["median_ms"], unfiltered_p95_ms=st[rate]["p95_ms"],
                                                     filtered_median_ms=st[rate + " filtered"]["median_ms"], filtered_p95_ms=st[rate + " filtered"]["p95_ms"],
                                                     filtered_over_unfiltered=round(st[rate + " filtered"]["median_ms"] / st[rate]["median_ms"], 4),
                                                     delay_frames=r["delay_frames"][rate + " filtered"]) for rate in ("30", "120")}
        rec = dict(command="python tools/live_bench.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), tick_frames=TICK,
                   ticks_per_case=a.steps, step_without_and_with_the_filter=table, results=results)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {a.out}")
        return 0
    if a.leg == "snapshot":
        budget = 1e3 * TICK / FPS
        table = {f"{r['rows']} rows": dict(step_median_ms=r["step"]["median_ms"], snapshot_many_median_ms=r["snapshot_many"]["median_ms"],
                                           snapshot_many_p95_ms=r["snapshot_many"]["p95_ms"], restore_one_row_median_ms=r["restore"]["median_ms"],
                                           snapshot_many_over_the_tick=round(r["snapshot_many"]["median_ms"] / budget, 4),
                                           snapshot_many_over_step=round(r["snapshot_many"]["median_ms"] / r["step"]["median_ms"], 4),
                                           blob_bytes_all_rows=r["blob_bytes_all_rows"]) for r in results}
        rec = dict(command="python tools/live_bench.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), tick_frames=TICK,
                   tick_ms=round(budget, 2), repeats_per_case=a.steps, snapshot_of_all_rows_and_restore_of_one_beside_step=table, results=results)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {a.out}")
        return 0
    if a.leg == "gaze":
        table = {}
        for r in results:
            plain, gz = r["step"]["plain"], r["step"]["gaze"]
            spread = round(plain["p95_ms"] - plain["median_ms"], 4)
            table[f"{r['rows']} rows"] = dict(step_plain_median_ms=plain["median_ms"], step_plain_p95_ms=plain["p95_ms"],
                                              step_gaze_median_ms=gz["median_ms"], step_gaze_p95_ms=gz["p95_ms"],
                                              gaze_minus_plain_ms=round(gz["median_ms"] - plain["median_ms"], 4), plain_spread_ms=spread,
                                              gaze_median_within_the_plain_spread=abs(gz["median_ms"] - plain["median_ms"]) <= spread,
                                              gaze_median_below_the_plain_median=gz["median_ms"] < plain["median_ms"],
                                              set_gaze_many_all_rows_median_ms=r["set_gaze_many"]["median_ms"],
                                              launches_per_step=r["launches_per_step"])
        rec = dict(command="python tools/live_bench.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), tick_frames=TICK,
                   ticks_per_case=a.steps, step_without_and_with_the_moving_gaze=table, results=results)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {a.out}")
        return 0
    if a.leg == "plant":
        table = {}
        for r in results:
            off, head, pl = (r["step"][k] for k in ("no head", "head", "plant"))
            own, added = round(head["median_ms"] - off["median_ms"], 4), round(pl["median_ms"] - head["median_ms"], 4)
            table[f"{r['rows']} rows"] = dict(step_no_head_median_ms=off["median_ms"], step_head_median_ms=head["median_ms"], step_head_p95_ms=head["p95_ms"],
                                              step_plant_median_ms=pl["median_ms"], step_plant_p95_ms=pl["p95_ms"], head_own_ms=own, plant_added_ms=added,
                                              plant_added_exceeds_the_heads_own=added > own, contact_share=r["contact_share"],
                                              launches_per_step=r["launches_per_step"])
        rec = dict(command="python tools/live_bench.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), tick_frames=TICK,
                   ticks_per_case=a.steps, step_without_the_head_with_it_and_with_planted_feet=table, results=results)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {a.out}")
        return 0
    if a.leg == "styles":
        budget = 1e3 * TICK / FPS
        table, add = {}, None
        for r in results:
            plain, bank = r["step"]["plain"], r["step"]["bank"]
            loop, many = r["set_style"]["tensor_loop"], r["set_style"]["named_many"]
            spread = round(plain["p95_ms"] - plain["median_ms"], 4)
            table[f"{r['rows']} rows"] = dict(set_style_tensor_loop_median_ms=loop["median_ms"], set_style_many_named_median_ms=many["median_ms"],
                                              named_over_tensor_loop=round(many["median_ms"] / loop["median_ms"], 4),
                                              named_is_cheaper=many["median_ms"] < loop["median_ms"], ops_per_set_style_many=r["ops_per_set_style_many"],
                                              step_plain_median_ms=plain["median_ms"], step_plain_p95_ms=plain["p95_ms"],
                                              step_bank_median_ms=bank["median_ms"], step_bank_p95_ms=bank["p95_ms"],
                                              bank_minus_plain_ms=round(bank["median_ms"] - plain["median_ms"], 4), plain_spread_ms=spread,
                                              bank_median_within_the_plain_spread=abs(bank["median_ms"] - plain["median_ms"]) <= spread,
                                              launches_per_step=r["launches_per_step"])
            if "add_style_of_exemplar_rows_on_the_device" in r:
                add = {k: dict(median_ms=v["median_ms"], p95_ms=v["p95_ms"], ticks=round(v["median_ms"] / budget, 3))
                       for k, v in r["add_style_of_exemplar_rows_on_the_device"].items()}
        rec = dict(command="python tools/live_bench.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), tick_frames=TICK,
                   tick_ms=round(budget, 2), ticks_per_case=a.steps, a_new_style_for_every_row_every_tick_and_the_step_beside_it=table,
                   add_style_beside_the_tick=add, results=results)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {a.out}")
        return 0
    budget = 1e3 * TICK / FPS
    srv = [r for r in results if r["kind"] == "server"]
    live_rows = {g: max([r["rows"] for r in srv if r["age_s"] == g and r["step"]["p95_ms"] < budget], default=0) for g in ages}
    age_effect = {}
    if len(ages) >= 2:
        for n in rows:
            lo, hi = ([r for r in srv if r["rows"] == n and r["age_s"] == g][0]["step"] for g in (ages[0], ages[-1]))
            spread = max(lo["p95_ms"] - lo["min_ms"], hi["p95_ms"] - hi["min_ms"])
            age_effect[str(n)] = dict(median_ms_young=lo["median_ms"], median_ms_old=hi["median_ms"], spread_ms=round(spread, 4),
                                      differs_by_more_than_the_spread=abs(hi["median_ms"] - lo["median_ms"]) > spread)
    rec = dict(command="python tools/live_bench.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0),
               tick_frames=TICK, step_budget_ms=round(budget, 2), steps_per_case=a.steps,
               largest_row_count_with_p95_under_the_budget=live_rows, age_effect_on_step_time=age_effect, results=results)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
