#!/usr/bin/env python
"""Batch decode against what a job list cost before it: one process, the same weights and inputs.

  per B in {2, 16, 32, 64}, T = 1800 frames per row (a 30 s clip), mean and spread of >= 3 timed regions after a warm-up:
    (a) B sequential B = 1 persistent rollouts            -- what a job list costs without the batch decode
    (b) the B-row inference rollout on the stage launches  -- ops.decoder_core under no_grad
    (c) the batch decode                                   -- generate.decode_plan on ops.BatchDecode, chunks of 256 frames, every
                                                              chunk's status word read back (as generate_gestures does)
    (c_chunk) one 256-frame chunk of (c) between device events: the sweep itself, per step
  end to end, 32 synthetic 30-second jobs: generate_gestures(batch=32) against 32 generate_gesture() calls, the whole call and
  the decode alone (generate.PROFILE, in runs of its own: the profile synchronises around every stage).

    python tools/batch_decode_bench.py [--out profiles/batch_decode.json] [--regions 3] [--skip-e2e]
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ubisoft-laforge-zeroeggs_amd"), str(ROOT / "tests")]
from zeggs import anim, generate, modules, ops, synth  # noqa: E402

DEV = torch.device("cuda:0")
T, CHUNK = 1800, 256


def timed(fn, regions):
    fn()                                            # warm-up: every shape of the timed regions
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def summary(ts, frames):
    m = statistics.mean(ts)
    return dict(regions_s=[round(t, 5) for t in ts], mean_s=round(m, 5), spread_s=round(max(ts) - min(ts), 5),
                frames_per_s=round(frames / m, 1))


def rollouts(regions):
    torch.manual_seed(0)
    de = modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, 64, 1024, 2).to(DEV).eval()
    s = {k: torch.as_tensor(v, dtype=torch.float32, device=DEV) for k, v in synth.make_stats().items() if k.startswith("anim")}
    st = (s["anim_input_mean"], s["anim_input_std"], s["anim_output_mean"], s["anim_output_std"])
    res = {}
    for B in (2, 16, 32, 64):
        g = torch.Generator(device="cpu").manual_seed(B)
        pose0 = (torch.randn(B, synth.POSE_OUT, generator=g) * 0.1).to(DEV)
        rpos0 = torch.zeros(B, 3, device=DEV)
        rrot0 = torch.tensor([[1.0, 0, 0, 0]], device=DEV).repeat(B, 1)
        gaze1 = (torch.randn(B, 1, 3, generator=g) + torch.tensor([0.0, 150.0, 100.0])).to(DEV)
        speech, style = (torch.randn(B, T, 64, generator=g) * 0.3).to(DEV), (torch.randn(B, T, 64, generator=g) * 0.3).to(DEV)
        gaze = gaze1.expand(B, T, 3).contiguous()

        def seq_b1():
            for b in range(B):
                ops.decoder_core(de, pose0[b:b + 1], rpos0[b:b + 1], rrot0[b:b + 1], gaze[b:b + 1], speech[b:b + 1],
                                 style[b:b + 1], *st, synth.DT)

        def stage():
            ops.decoder_core(de, pose0, rpos0, rrot0, gaze, speech, style, *st, synth.DT)

        bd = ops.BatchDecode(de, B, CHUNK, 64, 64, *st, synth.DT)
        firsts = [(pose0[b:b + 1], rpos0[b:b + 1], rrot0[b:b + 1], gaze1[b]) for b in range(B)]
        plan = generate.plan_slots([T] * B, B, CHUNK)
        status = ops.new_status(DEV)
        infos = []

        def batch():
            for _ in generate.decode_plan(bd, firsts, list(speech), list(style), plan, status=status, infos=infos):
                pass

        with torch.no_grad():
            r = dict(a_sequential_b1=summary(timed(seq_b1, regions), B * (T - 1)),
                     b_stage_launches=summary(timed(stage, regions), B * (T - 1)),
                     c_batch_decode=summary(timed(batch, regions), B * (T - 1)))
            r["c_paths"] = sorted({i["path"] for i in infos})
            r["c_chunks_redone"] = sum(1 for i in infos if i["gave_up"])
            # one chunk between device events: the sweep + its per-chunk prologue, no host in the window
            h = ops.decoder_state_init(bd, pose0, rpos0, rrot0, gaze1[:, 0], style[:, 0])
            args = (bd, pose0, rpos0, rrot0, gaze[:, :CHUNK].contiguous(), speech[:, :CHUNK].contiguous(),
                    style[:, :CHUNK].contiguous(), h)
            ops.decoder_batch_chunk(*args)
            ev = []
            for _ in range(max(regions, 3)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.decoder_batch_chunk(*args)
                e1.record()
                torch.cuda.synchronize()
                ev.append(e0.elapsed_time(e1) * 1e-3)
            r["c_chunk"] = dict(frames=CHUNK, regions_s=[round(t, 6) for t in ev],
                                us_per_step=round(statistics.mean(ev) * 1e6 / (CHUNK - 1), 2), path=ops.batch_last_path())
        for k in ("a_sequential_b1", "b_stage_launches", "c_batch_decode"):
            r[k]["us_per_step"] = round(r[k]["mean_s"] * 1e6 / (T - 1), 2)
        r["c_over_a"] = round(r["a_sequential_b1"]["mean_s"] / r["c_batch_decode"]["mean_s"], 2)
        r["c_over_b"] = round(r["b_stage_launches"]["mean_s"] / r["c_batch_decode"]["mean_s"], 2)
        res[f"B{B}"] = r
        print(f"B={B}: (a) {r['a_sequential_b1']['mean_s']:.4f} s  (b) {r['b_stage_launches']['mean_s']:.4f} s  "
              f"(c) {r['c_batch_decode']['mean_s']:.4f} s [{r['c_batch_decode']['us_per_step']} us/step, sweep alone "
              f"{r['c_chunk']['us_per_step']} us/step, {r['c_paths']}]  c/a x{r['c_over_a']}  c/b x{r['c_over_b']}", flush=True)
        del bd
    return res


def end_to_end(regions, njobs=32, seconds=30):
    import helpers
    import scipy.io.wavfile as wavfile
    tmp = Path(tempfile.mkdtemp(prefix="zeggs_batch_bench_"))
    net, data = tmp / "net", tmp / "data"
    net.mkdir(), data.mkdir()
    se, de, st = helpers.build_nets()
    torch.save(se, net / "speech_encoder.pt"), torch.save(de, net / "decoder.pt"), torch.save(st, net / "style_encoder.pt")
    np.savez(data / "stats.npz", **synth.make_stats())
    json.dump(synth.data_definition(), open(data / "data_definition.json", "w"))
    conf = dict(audio_conf=dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True,
                                normalize_mel_bins=True, normalize_range=True, min_clipping=1e-5, sampling_rate=16000,
                                mel_fmin=20, mel_fmax=7600, n_mel_channels=80, filter_length=800, hop_length=200,
                                resample_method="linear", normalize_loudness=False),
                audio_feature_type=["mel_spec", "energy"])
    json.dump(conf, open(data / "data_pipeline_conf.json", "w"))
    ex = tmp / "ex.bvh"
    anim.bvh_save(ex, synth.make_bvh_clip(256, seed=2))
    jobs = []
    for j in range(njobs):
        wavfile.write(tmp / f"a{j}.wav", 16000, synth.synth_wav(16000 * seconds, seed=100 + j))
        jobs.append(generate.Job(tmp / f"a{j}.wav", [(ex, None)], file_name=f"o{j}", first_pose=ex, temperature=1.0, seed=1000 + j,
                                 blend_ratio=[1.0]))

    def many(tag="many"):
        generate.generate_gestures(jobs, net, data, tmp / tag, batch=32, chunk=CHUNK)

    def loop(tag="loop"):
        (tmp / tag).mkdir(exist_ok=True)
        for j in jobs:
            generate.generate_gesture(j.audio_file, j.styles, net, data, tmp / tag, blend_ratio=[1.0], file_name=j.file_name,
                                      first_pose=j.first_pose, temperature=j.temperature, seed=j.seed)

    # alternating regions of the two (other people's work shares the host)
    many(), loop()
    torch.cuda.synchronize()
    tm, tl = [], []
    for _ in range(regions):
        for fn, acc in ((many, tm), (loop, tl)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append(time.perf_counter() - t0)
    frames = sum(len(anim.bvh_load(tmp / "many" / f"o{j}.bvh")["rotations"]) for j in range(njobs))
    out = dict(jobs=njobs, seconds_per_job=seconds, frames=frames, generate_gestures=summary(tm, frames),
               generate_gesture_loop=summary(tl, frames))
    out["whole_call_speedup"] = round(out["generate_gesture_loop"]["mean_s"] / out["generate_gestures"]["mean_s"], 2)
    # where the time goes: the stage profile (synchronises around every stage, so in runs of its own)
    for name, fn in (("generate_gestures", many), ("generate_gesture_loop", loop)):
        generate.PROFILE = {}
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        prof = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in generate.PROFILE.items()}
        generate.PROFILE = None
        out[name]["profiled_call_s"] = round(time.perf_counter() - t0, 4)
        out[name]["stages_ms"] = prof
    dm = out["generate_gestures"]["stages_ms"].get("batch_decode+pose_to_bvh_device_with_bvh_text_write_host_underneath")
    lp = out["generate_gesture_loop"]["stages_ms"]
    out["decode_alone"] = dict(
        generate_gestures_decode_convert_format_write_ms=dm,
        generate_gesture_loop_decode_ms=lp.get("decode_device"),
        generate_gesture_loop_pose_to_bvh_ms=lp.get("pose_to_bvh_device"),
        generate_gesture_loop_bvh_text_write_ms=lp.get("bvh_text_write_host"),
        bvh_rows_per_s_batch=round(frames / (dm * 1e-3), 1) if dm else None)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out, indent=1), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch_decode.json"))
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_decode_bench: needs the GPU (nothing is measured without one)")
    res = dict(tool="tools/batch_decode_bench.py", device=torch.cuda.get_device_name(0), frames_per_row=T, chunk=CHUNK,
               regions=a.regions, persistent_state_before=[int(ops.lib().zeggs_persistent_state(k)) for k in range(3)])
    res["rollouts"] = rollouts(a.regions)
    if not a.skip_e2e:
        res["end_to_end"] = end_to_end(a.regions)
    res["persistent_state_after"] = [int(ops.lib().zeggs_persistent_state(k)) for k in range(3)]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
