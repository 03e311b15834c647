"""Command line of the drop-in: the option surface of the reference's three scripts on the MI355X engine.

    python -m zeggs.cli prepare  -c data_pipeline_conf.json [--base-path DIR]  (ZEGGS/data_pipeline.py:739-744)
    python -m zeggs.cli train    -o options.json [-n NAME]                     (ZEGGS/main.py:10-74)
    python -m zeggs.cli generate -o options.json -s style.bvh -a speech.wav ... (ZEGGS/generate.py:414-525)
    python -m zeggs.cli generate -o options.json -c pairs.csv                   (batch mode, same CSV columns)
    python -m zeggs.cli generate -o options.json -c pairs.csv -b 32             (the job list decoded 32 clips at a time)
    python -m zeggs.cli evaluate -o options.json [--split valid|train]          (score the held-out split; no reference counterpart)

`options.json` is the reference's file (configs/configs_v*.json before training, <output_dir>/options.json after): keys
`train_opt`, `net_opt`, `paths` {base_path, path_processed_data, output_dir, models_dir}.  Differences from the reference's
scripts: there is no CPU path (`-g/--use_gpu` is accepted and implied), and the run's environment is not snapshotted
(`helpers.save_useful_info`: pip freeze / git state -- logging, out of scope)."""
import argparse
import csv
import datetime
import json
import sys
from pathlib import Path


def _paths(options):
    p = options["paths"]
    base = Path(p["base_path"])
    return p, base, base / p["path_processed_data"]


def cmd_train(a):
    from .train import train
    options = json.loads(Path(a.options).read_text())
    if a.name:
        options["name"] = a.name
    p, base, data = _paths(options)
    if p.get("output_dir") is None:      # a time-stamped run directory under <base>/outputs, as the reference does
        p["output_dir"] = str(base / "outputs" / datetime.datetime.now().strftime("%Y_%m_%d_%H_%M_%S"))
    out = Path(p["output_dir"])
    out.mkdir(parents=True, exist_ok=True)
    if p.get("models_dir") is None and not options["train_opt"]["resume"]:
        p["models_dir"] = str(out / "saved_models")
    models, logs = Path(p["models_dir"]), out / "logs"
    models.mkdir(parents=True, exist_ok=True)
    logs.mkdir(exist_ok=True)
    (out / "options.json").write_text(json.dumps(options, indent=4))      # what `generate -o` reads afterwards
    train(models_dir=models, logs_dir=logs, path_processed_data=data / "processed_data.npz",
          path_data_definition=data / "data_definition.json", train_options=options["train_opt"],
          network_options=options["net_opt"])
    return 0


def cmd_prepare(a):
    from .data_pipeline import data_pipeline
    conf = json.loads(Path(a.conf).read_text())
    if a.base_path:
        conf["base_path"] = a.base_path
    if a.mirror:
        conf["mirror"] = True
    data_pipeline(conf, log=lambda line: print(line, flush=True))
    return 0


def _truthy(v):
    return str(v).strip().lower() not in ("", "0", "false", "no", "nan", "none")


def cmd_generate(a):
    from .generate import generate_gesture
    options = json.loads(Path(a.options).read_text())
    p, _, data = _paths(options)
    network, results = Path(p["models_dir"]), Path(a.results_path) if a.results_path else Path(p["output_dir"]) / "results"
    results.mkdir(parents=True, exist_ok=True)
    kind = a.style_encoding_type
    jobs = []
    if a.csv:       # columns: base_path, audio, style, file_name, temperature, seed, use_gpu, frames, first_pose, generate
        with open(a.csv, newline="") as fh:
            for row in csv.DictReader(fh):
                if not _truthy(row.get("generate", "1")):
                    continue
                root = Path(row["base_path"])
                frames = [int(x) for x in row["frames"].split()] if _truthy(row.get("frames", "")) else None
                jobs.append(dict(audio=root / row["audio"], style=(root / row["style"], frames) if kind == "example" else row["style"],
                                 file_name=row.get("file_name") or None,
                                 first_pose=root / row["first_pose"] if _truthy(row.get("first_pose", "")) else None,
                                 temperature=float(row.get("temperature") or 1.0), seed=int(float(row.get("seed") or 1234))))
    else:
        if not (a.audio and a.style):
            raise SystemExit("generate: give -a AUDIO and -s STYLE (or -c CSV)")
        jobs.append(dict(audio=Path(a.audio), style=(Path(a.style), a.frames) if kind == "example" else a.style,
                         file_name=a.file_name, first_pose=Path(a.first_pose) if a.first_pose else None,
                         temperature=a.temperature, seed=a.seed))
    if a.batch:     # the whole list in one call: networks loaded once, the clips decoded a.batch rows at a time (zeggs.generate)
        from .generate import Job, generate_gestures
        print(f"{len(jobs)} jobs, {a.batch} clips per decode", flush=True)
        generate_gestures([Job(j["audio"], [j["style"]], file_name=j["file_name"], first_pose=j["first_pose"],
                               temperature=j["temperature"], seed=j["seed"], mirror_style=a.mirror_style) for j in jobs],
                          network_path=network, data_path=data, results_path=results, style_encoding_type=kind, batch=a.batch)
        return 0
    for k, j in enumerate(jobs):
        print(f"[{k + 1}/{len(jobs)}] {j['audio']}  style {j['style']}", flush=True)
        generate_gesture(audio_file=j["audio"], styles=[j["style"]], network_path=network, data_path=data, results_path=results,
                         style_encoding_type=kind, file_name=j["file_name"], first_pose=j["first_pose"],
                         temperature=j["temperature"], seed=j["seed"], use_gpu=True, mirror_style=a.mirror_style)
    return 0


def cmd_evaluate(a):
    """Score the validation (or training) split with the saved networks: the table by style label on stdout, the whole result as
    JSON (--json FILE, default <output_dir>/evaluation_<split>.json)."""
    import numpy as np
    import torch
    from . import compat, engine
    from .evaluate import evaluate, format_table
    options = json.loads(Path(a.options).read_text())
    p, _, data = _paths(options)
    topt, nopt = options["train_opt"], options["net_opt"]
    kind = topt.get("style_encoding_type", "example")
    device = torch.device("cuda", 0)
    if not torch.cuda.is_available():
        raise SystemExit("evaluate: the ZeroEGGS MI355X engine has no CPU path (no GPU visible)")
    torch.cuda.set_device(device)
    models = Path(p["models_dir"])
    if (models / "decoder.pt").exists():
        se = compat.load_module(models / "speech_encoder.pt", device).to(device)
        de = compat.load_module(models / "decoder.pt", device).to(device)
        st = compat.load_module(models / "style_encoder.pt", device).to(device) if kind == "example" else None
    else:
        se, de, st, _ = compat.load_state(models, device)
        st = st if kind == "example" else None
    with open(data / "data_definition.json") as f:
        details = json.load(f)
    ds = engine.DeviceDataset(np.load(data / "processed_data.npz"), topt["window"], device)
    iteration = None
    ck = models / "checkpoints.pt"
    if ck.exists():         # the KL weight the run had reached: the loss is then the one the training log shows
        iteration = int(torch.load(ck, map_location="cpu", weights_only=False)["iteration"])
    res = evaluate(se, de, st, ds, details["parents"], details["dt"], split=a.split, batch=a.batch or topt["batchsize"],
                   example_len=nopt["style_encoder"]["example_length"], iteration=iteration, max_windows=a.max_windows)
    print(f"{a.split}: {res['windows']} windows, {res['frames_scored']} of {res['frames_total']} frames scored"
          + (f", KL weight of iteration {iteration}" if iteration is not None else ""))
    for line in format_table(res, details["label_names"]):
        print(line)
    names = details["label_names"]
    out = dict(res, split=a.split, iteration=iteration, table=res["table"].tolist(),
               per_label={names[g] if g < len(names) else str(g): r for g, r in res["per_label"].items()})
    path = Path(a.json) if a.json else Path(p["output_dir"]) / f"evaluation_{a.split}.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=2))
    print(f"written {path}")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="zeggs", description="ZeroEGGS on the MI355X engine: prepare / train / generate / evaluate")
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("prepare", help="raw takes -> processed_data.npz, stats.npz, data_definition.json (reference: python data_pipeline.py)")
    d.add_argument("-c", "--conf", required=True, help="pipeline conf (configs/data_pipeline_conf_v*.json layout)")
    d.add_argument("--base-path", default=None, help="overrides the conf's base_path (the directory that holds original/ and the info CSV)")
    d.add_argument("--mirror", action="store_true", help="add every take's left/right reflection to the dataset (the conf key `mirror`: true)")
    d.set_defaults(fn=cmd_prepare)
    t = sub.add_parser("train", help="train the networks (reference: python main.py -o ... -n ...)")
    t.add_argument("-o", "--options", required=True, help="options file (configs_v*.json layout)")
    t.add_argument("-n", "--name", help="run name stored in the options")
    t.set_defaults(fn=cmd_train)
    g = sub.add_parser("generate", help="generate gesture BVHs (reference: python generate.py -o ... -s ... -a ...)")
    g.add_argument("-o", "--options", required=True, help="options.json written by training")
    g.add_argument("-p", "--results_path", nargs="?", default=None, help="where the BVH / WAV pairs go (default <output_dir>/results)")
    g.add_argument("-se", "--style_encoding_type", default="example", choices=("example", "label"))
    g.add_argument("-s", "--style", help="style exemplar BVH (or the label name with -se label)")
    g.add_argument("-a", "--audio", help="16 kHz speech WAV")
    g.add_argument("-n", "--file_name", help="output base name")
    g.add_argument("-fp", "--first_pose", default=None, help="BVH whose first frame starts the animation")
    g.add_argument("-t", "--temperature", type=float, nargs="?", default=1.0, help="VAE temperature")
    g.add_argument("-r", "--seed", type=int, nargs="?", default=1234)
    g.add_argument("-g", "--use_gpu", action="store_true", help="accepted for compatibility: the engine always runs on the GPU")
    g.add_argument("-f", "--frames", type=int, nargs=2, help="start and end frame of the exemplar")
    g.add_argument("--mirror-style", action="store_true", help="use the left/right reflection of every style exemplar")
    g.add_argument("-c", "--csv", help="CSV with one audio / style pair per row (evaluation_example_based.csv layout)")
    g.add_argument("-b", "--batch", type=int, default=0, metavar="N",
                   help="decode the jobs N clips at a time on the weight-stationary batch sweep (default: one clip per decode)")
    g.set_defaults(fn=cmd_generate)
    e = sub.add_parser("evaluate", help="score the held-out split with the saved networks (per-window loss, MPJPE, root drift by style label)")
    e.add_argument("-o", "--options", required=True, help="options.json written by training")
    e.add_argument("--split", default="valid", choices=("valid", "train"))
    e.add_argument("--batch", type=int, default=0, metavar="N", help="windows per decoder rollout (default: the training batch size)")
    e.add_argument("--max-windows", type=int, default=None, metavar="N", help="score only the first N windows of the split")
    e.add_argument("--json", default=None, metavar="FILE", help="where the result goes (default <output_dir>/evaluation_<split>.json)")
    e.set_defaults(fn=cmd_evaluate)
    a = ap.parse_args(argv)
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
