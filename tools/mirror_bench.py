#!/usr/bin/env python
"""Left/right mirroring on the MI355X, measured (recorded, no threshold) -> profiles/mirror.json:

  * the signed column gather (zeggs_mirror_rows) against a device-to-device copy of the same bytes in the same process, at the
    shapes that matter -- [T, 225] float64 (BVH channels of 75 joints), [T, 1134] and [T, 1131] float32 (the decoder's rows) with
    T = 512, 7 200 and 100 000: device events around blocks of launches, kernel and copy blocks alternating, the median of the
    blocks; bytes = one read and one write of the table; the gather is timed twice, through anim.mirror_rows (what a caller pays:
    short tables are bound by the host side of that call) and through the C entry point with prepared arguments;
  * the device features of a mirrored take against the mirrored features of the take (three channel orders): the largest
    difference per array and whether it was zero;
  * data_pipeline(conf) on eight synthetic two-minute 75-joint takes with and without `mirror` (len_ratios [0.9, 1.0], trimmed files
    written): wall times, alternating, and their ratio.

    python tools/mirror_bench.py [--out profiles/mirror.json] [--takes 8] [--frames 7200] [--no-pipeline]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ubisoft-laforge-zeroeggs_amd")]

WARM, BLOCKS = 5, 7


def kernel_against_copy(torch, anim, synth):
    import ctypes as C
    from zeggs import capi, ops
    pairs = anim.mirror_pairs(synth.BONE_NAMES, synth.PARENTS)
    out = []
    for layout, dtype in (("rotations", torch.float64), ("decoder_in", torch.float32), ("decoder_out", torch.float32)):
        table = anim.mirror_table(layout, pairs)
        for T in (512, 7200, 100000):
            x = torch.randn(T, table.size, dtype=dtype, device="cuda:0")
            y = torch.empty_like(x)
            nbytes = 2 * x.numel() * x.element_size()
            per_block = max(10, min(2000, int(2e9 / nbytes)))          # ~ 2 GB of traffic a block
            plan, L = anim._mirror_plan(table, x.device), capi.raw()
            args = (plan.handle, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_long(T), x.element_size(), ops._stream())
            # mirror: the public call by layout name (table and plan look-ups, a fresh output tensor, the typed binding); raw: the C entry point alone
            work = dict(mirror=lambda: anim.mirror_rows(x, layout, pairs), raw=lambda: L.zeggs_mirror_rows(*args), copy=lambda: y.copy_(x))
            for f in work.values():
                for _ in range(WARM):
                    f()
            torch.cuda.synchronize()
            us = dict(mirror=[], raw=[], copy=[])
            for _ in range(BLOCKS):
                for name, f in work.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(per_block):
                        f()
                    b.record()
                    b.synchronize()
                    us[name].append(a.elapsed_time(b) * 1000.0 / per_block)
            m, c, r = statistics.median(us["mirror"]), statistics.median(us["copy"]), statistics.median(us["raw"])
            out.append(dict(layout=layout, rows=T, cols=int(table.size), dtype=str(dtype).replace("torch.", ""), bytes=nbytes,
                            launches_per_block=per_block, blocks=BLOCKS, mirror_us=round(m, 2), raw_us=round(r, 2), copy_us=round(c, 2),
                            mirror_us_min_max=[round(min(us["mirror"]), 2), round(max(us["mirror"]), 2)],
                            copy_us_min_max=[round(min(us["copy"]), 2), round(max(us["copy"]), 2)],
                            raw_us_min_max=[round(min(us["raw"]), 2), round(max(us["raw"]), 2)],
                            mirror_GBps=round(nbytes / m / 1e3, 1), raw_GBps=round(nbytes / r / 1e3, 1), copy_GBps=round(nbytes / c / 1e3, 1),
                            ratio=round(m / c, 3), raw_ratio=round(r / c, 3)))
    return out


def commute(torch, anim, synth):
    out = {}
    names = [n for n, _, _ in anim.ANIM_OUT]
    order_of_tuple = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "lrot", "ltxy", "lvel", "lvrt", "cpos", "crot", "ctxy", "cvel",
                      "cvrt", "gaze_pos", "gaze_dir")
    assert sorted(names) == sorted(order_of_tuple)
    for order in ("zyx", "xzy", "yzx"):
        clip = synth.make_bvh_clip(7200, seed=21)
        clip["order"] = order
        pairs = anim.mirror_pairs(clip["names"], clip["parents"])
        plain = anim.preprocess_animation(clip, "cuda:0")
        mirrored = anim.preprocess_animation(anim.mirror_take(clip), "cuda:0")
        diff = {n: float((anim.mirror_rows(a, n, pairs).double() - b.double()).abs().max()) for n, a, b in zip(order_of_tuple, plain, mirrored)}
        out[order] = dict(frames=7200, joints=75, max_abs_difference=diff, zero={n: d == 0.0 for n, d in diff.items()}, all_zero=all(d == 0.0 for d in diff.values()))
    return out


def pipeline(torch, synth, dp, takes_n, frames):
    with tempfile.TemporaryDirectory() as tmp:
        base = Path(tmp)
        takes = [synth.make_raw_take(f"take{i}_{'Happy' if i % 2 else 'Sad'}", frames, seed=40 + i, style="Happy" if i % 2 else "Sad",
                                     validation=(i == takes_n - 1)) for i in range(takes_n)]
        synth.write_raw_corpus(base, takes)
        (base / "warm.csv").write_text("\n".join((base / "info.csv").read_text().splitlines()[:2]) + "\n")
        dp.data_pipeline(synth.pipeline_conf(base, processed_data_path="warm", info_filename="warm.csv", mirror=True))
        walls = dict(plain=[], mirror=[])
        rows = {}
        for r in range(2):
            for name, extra in (("plain", {}), ("mirror", dict(mirror=True))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                data, _ = dp.data_pipeline(synth.pipeline_conf(base, processed_data_path=f"{name}{r}", **extra))
                walls[name].append(time.perf_counter() - t0)
                rows[name] = int(len(data["X_audio_features"]))
        stages = {}
        dp.data_pipeline(synth.pipeline_conf(base, processed_data_path="staged", mirror=True), timings=stages)
        p, m = statistics.median(walls["plain"]), statistics.median(walls["mirror"])
        return dict(corpus=dict(takes=takes_n, frames_per_take=frames, joints=75, len_ratios=[0.9, 1.0], trimmed_files=True),
                    rows=rows, wall_s={k: [round(w, 3) for w in v] for k, v in walls.items()}, plain_s=round(p, 3), mirror_s=round(m, 3),
                    ratio=round(m / p, 3), mirror_stages_s={k: round(v, 3) for k, v in stages.items()},
                    note="wall times with the profiler off, plain and mirrored runs alternating; stages: one more mirrored run with a "
                         "device synchronise after every stage")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mirror.json"))
    ap.add_argument("--takes", type=int, default=8)
    ap.add_argument("--frames", type=int, default=7200)
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args()
    import torch
    from zeggs import anim, synth
    from zeggs import data_pipeline as dp
    assert torch.cuda.is_available(), "mirror_bench needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), cpus=len(os.sched_getaffinity(0)),
               kernel=dict(source="device events around blocks of launches, medians of the blocks: mirror_* through anim.mirror_rows(x, layout name, pairs), "
                                  "raw_* through the C entry point zeggs_mirror_rows with prepared arguments, copy_* through Tensor.copy_",
                           shapes=kernel_against_copy(torch, anim, synth)),
               commute=commute(torch, anim, synth))
    res["pipeline"] = "not measured" if a.no_pipeline else pipeline(torch, synth, dp, a.takes, a.frames)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
