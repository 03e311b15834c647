#!/usr/bin/env python
"""Dataset preparation on the MI355X, measured (recorded, no threshold) -> profiles/prepare.json:

  * the spline solve + evaluation alone at (N = 2 000 000, W = 1: a two-minute take's audio) and (N = 7 200, W = 300: its unrolled
    quaternions), M = 0.9 N: per kernel the median of the timed launches of ONE `rocprofv3 --kernel-trace --stats` pass over a child
    process (this file with --spline-probe), after warm launches of both shapes;
  * data_pipeline(conf) on eight synthetic two-minute 75-joint takes (seven train, one validation; len_ratios [0.9, 1.0], trimmed
    files written, loudness normalisation off): wall time with the profiler off, then a second run with a device synchronise after
    every stage for the per-stage split;
  * beside it the unmodified reference's data_pipeline(conf) on the same corpus on this box's CPUs, where the oracle/_ref snapshot
    (or the reference checkout) and its dependencies (pandas, rich) are present; "not measured" otherwise.

    python tools/prepare_bench.py [--out profiles/prepare.json] [--takes 8] [--frames 7200] [--no-reference]
"""
import argparse
import glob
import json
import os
import shutil
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ubisoft-laforge-zeroeggs_amd")]

SHAPES = ((2_000_000, 1), (7_200, 300))
WARM, TIMED = 5, 20


def spline_probe():
    """child under rocprofv3: WARM + TIMED launches of shape 0, then of shape 1"""
    import torch
    from zeggs import data_pipeline as dp
    for n, w in SHAPES:
        y = torch.randn(n, w, dtype=torch.float64, device="cuda:0")
        for _ in range(WARM + TIMED):
            dp.spline_resample(y, int(0.9 * n))
        torch.cuda.synchronize()


def spline_kernels(out_dir):
    """run the probe under one rocprofv3 pass and read the dispatches back (rocpd sqlite)"""
    prof = Path(out_dir) / "prepare_prof"
    shutil.rmtree(prof, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", str(prof), "-o", "spline", "--", sys.executable, str(Path(__file__).resolve()),
           "--spline-probe"]
    subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    db = sqlite3.connect(glob.glob(str(prof / "**" / "*.db"), recursive=True)[0])
    cols = [r[1] for r in db.execute("PRAGMA table_info(kernels)")]
    pick = lambda *c: next(x for x in c if x in cols)  # noqa: E731
    name, st, en = pick("name", "kernel_name"), pick("start", "start_timestamp"), pick("end", "end_timestamp")
    rows = [(n, e - s) for n, s, e in db.execute(f"select {name}, {st}, {en} from kernels order by {st}") if "spline_" in n]
    per = len(rows) // (len(SHAPES) * (WARM + TIMED))            # kernels per call: solve, ends, eval
    assert per * len(SHAPES) * (WARM + TIMED) == len(rows), (len(rows), per)
    out = []
    for i, (n, w) in enumerate(SHAPES):
        calls = [rows[(i * (WARM + TIMED) + c) * per:(i * (WARM + TIMED) + c + 1) * per] for c in range(WARM, WARM + TIMED)]
        kernels = {}
        for k in range(per):
            short = calls[0][k][0].replace("(anonymous namespace)::", "").split("(")[0]
            kernels[short] = round(statistics.median(c[k][1] for c in calls) / 1000.0, 2)
        total = [sum(d for _, d in c) / 1000.0 for c in calls]
        out.append(dict(N=n, W=w, M=int(0.9 * n), kernel_us_median=kernels, call_us_median=round(statistics.median(total), 2),
                        call_us_min=round(min(total), 2), call_us_max=round(max(total), 2), timed_launches=TIMED, warm_launches=WARM,
                        bytes_min=8 * (2 * n * w + int(0.9 * n) * w)))        # y read once, out written once, S written once (float64)
    shutil.rmtree(prof, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "prepare.json"))
    ap.add_argument("--takes", type=int, default=8)
    ap.add_argument("--frames", type=int, default=7200)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--spline-probe", action="store_true")
    a = ap.parse_args()
    if a.spline_probe:
        return spline_probe()
    import torch
    from zeggs import data_pipeline as dp
    from zeggs import synth
    assert torch.cuda.is_available(), "prepare_bench needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), cpus=len(os.sched_getaffinity(0)),
               spline=dict(source="rocprofv3 --kernel-trace --stats, one pass, per-dispatch durations", shapes=spline_kernels(Path(a.out).parent)))
    with tempfile.TemporaryDirectory() as tmp:
        base = Path(tmp)
        takes = [synth.make_raw_take(f"take{i}_{'Happy' if i % 2 else 'Sad'}", a.frames, seed=40 + i, style="Happy" if i % 2 else "Sad",
                                     validation=(i == a.takes - 1)) for i in range(a.takes)]
        synth.write_raw_corpus(base, takes)
        corpus = dict(takes=a.takes, frames_per_take=a.frames, joints=75, audio_seconds=round(len(takes[0]["wav"]) / 16000, 1),
                      len_ratios=[0.9, 1.0], trimmed_files=True, normalize_loudness=False,
                      bvh_bytes=sum(p.stat().st_size for p in (base / "original").glob("*.bvh")))
        warm = synth.pipeline_conf(base, processed_data_path="warm", info_filename="warm.csv")
        (base / "warm.csv").write_text("\n".join((base / "info.csv").read_text().splitlines()[:2]) + "\n")
        dp.data_pipeline(warm)                                      # code objects, filterbank cache, allocator: one take
        walls = []
        for r in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data, _ = dp.data_pipeline(synth.pipeline_conf(base, processed_data_path=f"run{r}"))
            walls.append(time.perf_counter() - t0)
        stages = {}
        dp.data_pipeline(synth.pipeline_conf(base, processed_data_path="staged"), timings=stages)
        res["builder"] = dict(corpus=corpus, rows=int(len(data["X_audio_features"])), wall_s=[round(w, 3) for w in walls],
                              wall_s_median=round(statistics.median(walls), 3),
                              stages_s={k: round(v, 3) for k, v in stages.items()}, stages_total_s=round(sum(stages.values()), 3),
                              note="stages: one more run with a device synchronise after every stage; load = BVH parse + WAV read + CSV, "
                                   "write_bvh / write_wav include the download of the take, save = the three output files")
        ref = dict(measured=False)
        if not a.no_reference:
            try:
                from oracle import ref_shims
                if not ref_shims.available():
                    raise RuntimeError("no reference checkout and no oracle/_ref snapshot on this box")
                mod = ref_shims.load()
                t0 = time.perf_counter()
                cwd = os.getcwd()
                try:
                    with open(os.devnull, "w") as null:
                        so, sys.stdout = sys.stdout, null
                        try:
                            mod.data_pipeline.data_pipeline(synth.pipeline_conf(base, processed_data_path="reference"))
                        finally:
                            sys.stdout = so
                finally:
                    os.chdir(cwd)
                    ref_shims.release()
                ref = dict(measured=True, wall_s=round(time.perf_counter() - t0, 3), source=ref_shims.source(), runs=1)
            except Exception as e:      # noqa: BLE001  (a missing dependency of the reference is a reason, not a failure of this tool)
                ref = dict(measured=False, reason=f"{type(e).__name__}: {e}")
        res["reference_cpu"] = ref
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
