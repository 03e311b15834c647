#!/usr/bin/env python
"""The BVH motion text on the device (csrc/text.hip) against the host formatter (snprintf, csrc/hostio.hip): one process, both
settings of anim.TEXT in the same session.

  kernel       a 4096 x 228 table: the measure, scan and emit passes between device events, both emit variants (LDS assembly with
               aligned 16-byte stores, and per-byte global stores), and the whole call
  crossover    bvh_save() of HOST tables of growing row counts under text = "host" and through the device (upload + format +
               download): the row count from which the device wins is anim.TEXT_UPLOAD_MIN_NUMBERS / 228
  end_to_end   tools/batch_decode_bench.py's end_to_end block (32 thirty-second jobs, generate_gestures and the generate_gesture
               loop with their stage profiles), unchanged, under both settings
  prepare      data_pipeline(conf) on the synthetic corpus of profiles/prepare.json: the write_bvh lap under both settings
  generate_30min   bench.py's generate_30min entry (what `bench.py --full` reports for the 30-minute clip) under both settings

    python tools/bvh_text_bench.py [--out profiles/bvh_text_device.json] [--regions 3] [--only kernel,crossover,...]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ubisoft-laforge-zeroeggs_amd"), str(ROOT / "tests"), str(ROOT / "tools")]
from zeggs import anim, ops, synth  # noqa: E402

DEV = torch.device("cuda:0")
ROWS, COLS = 4096, 228


def call(table, text, meta):
    rows, cols = table.shape
    return ops.lib().zeggs_table_text_device(C.c_void_p(table.data_ptr()), C.c_long(rows), int(cols), C.c_void_p(text.data_ptr()),
                                             C.c_size_t(text.numel()), C.c_void_p(meta.data_ptr()), C.c_void_p(meta[rows:].data_ptr()),
                                             C.c_void_p(_WS.data_ptr()), C.c_size_t(_WS.numel()),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))


def kernel(reps=30):
    rng = np.random.default_rng(0)
    table = torch.as_tensor((rng.random((ROWS, COLS)) - 0.5) * 360.0, device=DEV)
    want = anim.format_rows(table.cpu().numpy())
    out = dict(rows=ROWS, cols=COLS, text_bytes=len(want), table_bytes=ROWS * COLS * 8, reps=reps,
               note="median of device-event times per pass; every pass reads or writes HBM once: measure reads the table, emit reads "
                    "it again and writes the text; 7.5 + 7.5 + ~10.5 MB against 8 TB/s is ~3 us, so launch overhead and the "
                    "digit arithmetic are what is measured, not the memory system")
    for emit, name in ((1, "emit_lds_aligned_stores"), (0, "emit_per_byte_stores")):
        ops.set_option("text_emit", emit)
        ops.set_option("text_passes", 7)
        assert bytes(anim.format_rows_device(table)[0]) == want
        text, meta = anim.table_text_device(table)                    # (allocations of the timed calls come from the cache)
        res = {}
        for mask, label in ((1, "measure"), (2, "scan"), (4, "emit"), (7, "whole_call")):
            ts = []
            for _ in range(reps):
                # the passes one by one on the buffers of a full call: 1 refreshes the lengths, 2 scans them, 4 emits
                for m in ((1, 2, 4) if mask != 7 else (7,)):
                    ops.set_option("text_passes", m)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    if m == mask:
                        e0.record()
                    rc = call(table, text, meta)
                    assert rc == 0
                    if m == mask:
                        e1.record()
                        torch.cuda.synchronize()
                        ts.append(e0.elapsed_time(e1) * 1e3)
            res[label + "_us"] = dict(median=round(statistics.median(ts), 2), min=round(min(ts), 2), max=round(max(ts), 2))
        ops.set_option("text_passes", 7)
        torch.cuda.synchronize()
        assert bytes(text[:len(want)].cpu().numpy().tobytes()) == want
        out[name] = res
    ops.set_option("text_emit", 0)
    print(json.dumps(out, indent=1), flush=True)
    return out


def crossover(reps=7):
    """bvh_save of host channel arrays, `rows` frames of the 75-joint skeleton"""
    res = []
    tmp = Path(tempfile.mkdtemp(prefix="zeggs_text_bench_"))
    keep = anim.TEXT_UPLOAD_MIN_NUMBERS
    try:
        for rows in (1, 4, 16, 32, 64, 128, 256, 1024, 4096, 16384):
            clip = synth.make_bvh_clip(rows, seed=rows)
            t = {}
            for mode in ("host", "device"):
                anim.TEXT_UPLOAD_MIN_NUMBERS = 0
                ts = []
                for i in range(reps + 1):
                    t0 = time.perf_counter()
                    anim.bvh_save(tmp / f"{mode}.bvh", clip, text=mode)
                    ts.append(time.perf_counter() - t0)
                t[mode] = ts[1:]
            assert (tmp / "host.bvh").read_bytes() == (tmp / "device.bvh").read_bytes()
            res.append(dict(rows=rows, numbers=rows * COLS, host_ms_median=round(statistics.median(t["host"]) * 1e3, 3),
                            device_ms_median=round(statistics.median(t["device"]) * 1e3, 3),
                            host_ms_min=round(min(t["host"]) * 1e3, 3), device_ms_min=round(min(t["device"]) * 1e3, 3)))
            print(res[-1], flush=True)
    finally:
        anim.TEXT_UPLOAD_MIN_NUMBERS = keep
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)
    wins = [r["rows"] for r in res if r["device_ms_median"] < r["host_ms_median"]]
    return dict(table=res, device_wins_from_rows=min(wins) if wins else None, threshold_numbers_shipped=keep,
                note="host = zeggs_write_table_text (up to 16 threads from 2048 rows on); device = upload of the channels, table built "
                     "with torch.cat, zeggs_table_text_device, row ends + exact text downloaded into pinned memory, one write")


def both(fn):
    out = {}
    keep = anim.TEXT
    try:
        for mode in ("device", "host"):
            anim.TEXT = mode
            out[mode] = fn()
    finally:
        anim.TEXT = keep
    return out


def prepare(takes=4, frames=7200):
    from zeggs import data_pipeline as dp
    with tempfile.TemporaryDirectory() as tmp:
        base = Path(tmp)
        raw = [synth.make_raw_take(f"take{i}_{'Happy' if i % 2 else 'Sad'}", frames, seed=40 + i, style="Happy" if i % 2 else "Sad",
                                   validation=(i == takes - 1)) for i in range(takes)]
        synth.write_raw_corpus(base, raw)
        dp.data_pipeline(synth.pipeline_conf(base, processed_data_path="warm"))
        n = [0]

        def run():
            laps = []
            for _ in range(3):
                stages = {}
                n[0] += 1
                t0 = time.perf_counter()
                dp.data_pipeline(synth.pipeline_conf(base, processed_data_path=f"run{n[0]}"), timings=stages)
                laps.append(dict(wall_s=round(time.perf_counter() - t0, 3), write_bvh_s=round(stages.get("write_bvh", 0.0), 4),
                                 stages_total_s=round(sum(stages.values()), 3)))
            return dict(runs=laps, write_bvh_s_median=statistics.median(x["write_bvh_s"] for x in laps))
        out = both(run)
        out["corpus"] = dict(takes=takes, frames_per_take=frames, len_ratios=[0.9, 1.0])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bvh_text_device.json"))
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--only", default="kernel,crossover,end_to_end,prepare,generate_30min")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bvh_text_bench: needs the GPU (nothing is measured without one)")
    only = a.only.split(",")
    out_path = Path(a.out)
    res = json.loads(out_path.read_text()) if out_path.exists() else {}
    res.update(tool="tools/bvh_text_bench.py", device=torch.cuda.get_device_name(0))
    global _WS
    ops.lib().zeggs_table_text_workspace_bytes.restype = C.c_size_t
    _WS = torch.empty(int(ops.lib().zeggs_table_text_workspace_bytes(ROWS, COLS)), dtype=torch.uint8, device=DEV)
    if "kernel" in only:
        res["kernel"] = kernel()
    if "crossover" in only:
        res["crossover"] = crossover()
    if "end_to_end" in only:
        import batch_decode_bench
        res["end_to_end"] = both(lambda: batch_decode_bench.end_to_end(a.regions))
    if "prepare" in only:
        res["prepare"] = prepare()
    if "generate_30min" in only:
        import os
        import bench
        res["generate_30min"] = both(lambda: bench.generate_30min(DEV))
        res["generate_30min"]["host_threads"] = dict(device=2, host=min(16, os.cpu_count() or 4))
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
