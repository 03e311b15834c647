#!/usr/bin/env python
"""Live serving: wall time of one LiveServer.step() per row count and stream age, beside GestureStream.push of the same chunk.

  per rows in {1, 8, 32, 64} and stream age in {10 s, 600 s}: every row is fed a synthetic WAV up to that age (1 s pushes, drained),
  then `tick`-sized pushes (tick / 60 s of audio per row) each followed by ONE step(); the step's wall time (host call + device,
  synchronised before and after) over >= 200 steps: median, p95, min, max; what the server enqueues per step; the pushes' wall
  time beside it (mel stays per row: rows pushes per tick).
  baseline, same session: zeggs.stream.GestureStream.push of the same 4-frame chunk at the same two ages (one stream, B = 1).

Every case is a child process under its own `timeout`; the first one that fails ends the run (as a chain of `&&` would).

    python tools/live_bench.py [--out profiles/live_stream.json] [--steps 200] [--rows 1,8,32,64] [--ages 10,600]
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
    ap.add_argument("--case", default=None, help="internal: one case in a child process, e.g. server:8:10 or baseline:600")
    a = ap.parse_args()
    if a.case:
        kind, *rest = a.case.split(":")
        res = case_server(int(rest[0]), int(rest[1]), a.steps) if kind == "server" else case_baseline(int(rest[0]), a.steps)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    ages, rows = [int(x) for x in a.ages.split(",")], [int(x) for x in a.rows.split(",")]
    cases = [f"baseline:{g}" for g in ages] + [f"server:{r}:{g}" for r in rows for g in ages]
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
