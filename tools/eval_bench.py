"""Held-out evaluation: what it costs (profiles/eval.json).

(a) zeggs_loss_eval against zeggs_loss_fwd_bwd, each alone on the chip, B = 32, T = 256, J = 75: HIP events around every launch
    of a call, 5 warm and 20 timed calls, alternating the two; median / min / max in microseconds, and their ratio.  The
    forward-only call does strictly less (no gradient table, no backward): it must not be slower.
(b) evaluate() on a synthetic validation split at the headline shape (batch 32, window 256, >= 20 batches): frames per second
    (host clock around the call, which ends in its one device-to-host copy), and the host synchronisations it makes, counted by
    wrapping torch.cuda.synchronize / Event.synchronize / Tensor.cpu / Tensor.item / Tensor.to for the length of the call.

    python tools/eval_bench.py [--out profiles/eval.json] [--batches 20]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "ubisoft-laforge-zeroeggs_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

from zeggs import engine, evaluate, modules, ops, synth  # noqa: E402

DEV = "cuda:0"
WARM, TIMED = 5, 20


def _loss_inputs(B, T):
    stats = synth.make_stats()
    keys = ("Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt")

    def side(seed):
        clips = [synth.make_clip(T, seed=seed + b, stats=stats) for b in range(B)]
        tt = lambda k: torch.as_tensor(np.stack([c[k] for c in clips]), dtype=torch.float32)  # noqa: E731
        pose = torch.cat([tt(k).reshape(B, T, -1) for k in keys], dim=-1)
        return pose.to(DEV), tt("Y_root_pos").to(DEV), tt("Y_root_rot").to(DEV), tt("Y_gaze_pos").to(DEV)
    wp, wrp, wrr, gaze = side(100)
    op, orp, orr, _ = side(500)
    op, orr = wp + 0.3 * (op - wp), wrr + 0.3 * (orr - wrr)
    g = torch.Generator().manual_seed(1)
    mu, lv = torch.randn(B, 64, generator=g).to(DEV), (0.3 * torch.randn(B, 64, generator=g)).to(DEV)
    return op, orp, orr, wp, wrp, wrr, gaze, torch.as_tensor(synth.PARENTS, dtype=torch.int32, device=DEV), mu, lv


def bench_kernel(B=32, T=256):
    op, orp, orr, wp, wrp, wrr, gaze, parents, mu, lv = _loss_inputs(B, T)
    rows = torch.empty(B, ops.EVAL_COLS, device=DEV, dtype=torch.float64)
    ws = ops.loss_eval_workspace(B, T, len(synth.PARENTS), 64, synth.DT, DEV)

    def forward_only():
        ops.loss_eval(op, orp, orr, wp, wrp, wrr, gaze, parents, synth.DT, mu, lv, rows=rows, ws=ws)

    def training():
        with torch.no_grad():        # (the call itself always builds the gradients: autograd only decides who keeps them)
            ops.training_loss(op, orp, orr, wp, wrp, wrr, gaze, parents, synth.DT, mu, lv, kl_weight=0.2)
    times = {"loss_eval": [], "loss_fwd_bwd": []}
    for k in range(WARM + TIMED):
        for name, fn in (("loss_eval", forward_only), ("loss_fwd_bwd", training)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= WARM:
                times[name].append(1000.0 * e0.elapsed_time(e1))
    out = {"shape": dict(B=B, T=T, J=len(synth.PARENTS)), "warm_launches": WARM, "timed_launches": TIMED}
    for name, t in times.items():
        out[name + "_us"] = dict(median=round(statistics.median(t), 2), min=round(min(t), 2), max=round(max(t), 2))
    out["ratio_eval_over_training"] = round(out["loss_eval_us"]["median"] / out["loss_fwd_bwd_us"]["median"], 4)
    L = ops.lib()
    import ctypes as C
    d = ops.LossDims(B, T, len(synth.PARENTS), 64, synth.DT)
    out["workspace_bytes"] = dict(loss_eval=int(L.zeggs_loss_eval_workspace_bytes(C.byref(d))),
                                  loss_fwd_bwd=int(L.zeggs_loss_workspace_bytes(C.byref(d))))
    return out


class _count_syncs:
    """host synchronisations made inside the block"""

    def __enter__(self):
        self.n = 0
        self.saved = [(torch.cuda, "synchronize"), (torch.cuda.Event, "synchronize"), (torch.Tensor, "cpu"), (torch.Tensor, "item")]
        self.orig = [getattr(o, n) for o, n in self.saved]
        for (o, n), f in zip(self.saved, self.orig):
            def wrap(*a, _f=f, **kw):
                self.n += 1
                return _f(*a, **kw)
            setattr(o, n, wrap)
        return self

    def __exit__(self, *exc):
        for (o, n), f in zip(self.saved, self.orig):
            setattr(o, n, f)
        return False


def bench_evaluate(batches=20, B=32, T=256, L=384):
    torch.manual_seed(1234)
    se = modules.SpeechEncoder(synth.N_AUDIO, 64, 64).to(DEV)
    de = modules.Decoder(synth.POSE_IN, synth.POSE_OUT, 64, 64, 1024, 2).to(DEV)
    st = modules.StyleEncoder(synth.POSE_IN, 512, 64, type="attn", use_vae=True).to(DEV)
    n_valid = 8
    per_range = (batches * B + n_valid - 1) // n_valid
    data = synth.make_processed(1, n_valid, per_range * T + 1, seed=5)
    ds = engine.DeviceDataset(data, T, torch.device(DEV))
    kw = dict(split="valid", batch=B, example_len=L, iteration=9000)
    evaluate.evaluate(se, de, st, ds, synth.PARENTS, synth.DT, max_windows=2 * B, **kw)      # warm: code objects, first-use checks
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        with _count_syncs() as c:
            t0 = time.perf_counter()
            res = evaluate.evaluate(se, de, st, ds, synth.PARENTS, synth.DT, **kw)
            dt = time.perf_counter() - t0
        nb = (res["windows"] + B - 1) // B
        runs.append(dict(seconds=round(dt, 4), frames_per_s=round(res["frames_scored"] / dt, 1), windows=res["windows"], batches=nb,
                         host_syncs_total=c.n, host_syncs_per_batch=round(c.n / nb, 3)))
    best = max(runs, key=lambda r: r["frames_per_s"])
    return dict(shape=dict(batch=B, window=T, example_len=L), runs=runs, frames_per_s=best["frames_per_s"],
                host_syncs_per_batch=best["host_syncs_per_batch"], loss=res["loss"], mpjpe=res["mpjpe"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "eval.json"))
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--training-frames-per-s", type=float, default=None,
                    help="bench.py's headline of the same session, recorded beside (b)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs a GPU (nothing is measured without one)")
    out = dict(device=torch.cuda.get_device_name(0), kernel=bench_kernel(), evaluate=bench_evaluate(a.batches))
    if a.training_frames_per_s is not None:
        out["training_frames_per_s_same_session"] = a.training_frames_per_s
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
