"""Record tests/golden/prepare.npz: what the UNMODIFIED reference's data_pipeline(conf) makes of a tiny raw corpus.

    python tools/make_golden_prepare.py            (build container only: needs the reference checkout, pandas, rich, scipy)

The corpus: three takes of a 9-joint skeleton (Hips .. Head, two arms, one leg), two styles, the last take marked as validation;
130 to 150 frames at 60 fps (acting spans of 61 to 70 frames) with Euler angles inside +-60 degrees (to_euler's arcsin stays far from its clip), 2.5 to 2.8 s of
16 kHz speech-like noise, speaker CSVs with "R" and non-"R" rows, a non-zero acting start.  Three confs (loudness normalisation
off: pyloudnorm is not installed, and that pre-pass is pinned elsewhere):
    c0: len_ratios [0.9, 1.0], save_trimmed_animation true     c1: the same, false     c2: [1.0, 1.1], true
The centring that save_trimmed_animation switches on writes into the take the features are computed from, and at ratio 1.0 into the
trimmed original itself, so the three datasets differ: the fixture pins that data flow.

Stored: the corpus files byte for byte (`file/<path>`), the conf JSONs, every returned array, label names, dt, the trimmed BVH channel
tables [frames, 3 + 3 J] (`c<i>/bvh/<split>/<name>`) and the trimmed WAV samples (`wav/<split>/<name>`, int16; the audio does not depend
on save_trimmed_animation, so one copy per take and ratio).  The three datasets share most of their numbers (the audio features of a take
at one ratio, every joint but the root), and a committed file must stay under 1 MiB, so equal blocks are stored once: a per-row array is
cut at the take boundaries (per-joint arrays also into joint 0 | the other joints), each distinct block goes into `pool/<id>`, and
`c<i>/<key>@pool` lists the ids ([blocks] or [blocks, 2]); BVH tables go through the same pool.  The statistics, ranges and labels are
stored as they are (`c<i>/<key>`).  tests/test_gpu_prepare.py puts the arrays together again.
"""
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "ubisoft-laforge-zeroeggs_amd"):
    sys.path.insert(0, str(p))

NAMES = ["Hips", "Spine", "Spine1", "Spine2", "Neck", "Head", "LeftArm", "RightArm", "LeftUpLeg"]
PARENTS = [-1, 0, 1, 2, 3, 4, 3, 3, 0]
#        name, frames, style, validation, frames after the acting, seconds of audio      (acting spans: 70, 65 and 61 frames)
TAKES = (("t0_Happy", 150, "Happy", False, 65, 2.8), ("t1_Sad", 140, "Sad", False, 59, 2.65), ("t2_Happy", 130, "Happy", True, 52, 2.5))
PER_ROW = ("X_audio_features", "Y_root_pos", "Y_root_rot", "Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt", "Y_gaze_pos")
PER_JOINT = ("Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt")
CONFS = (dict(len_ratios=[0.9, 1.0], save_trimmed_animation=True), dict(len_ratios=[0.9, 1.0], save_trimmed_animation=False),
         dict(len_ratios=[1.0, 1.1], save_trimmed_animation=True))


def small_clip(nframes, seed):
    from zeggs import synth
    rng = np.random.default_rng(seed)
    nj = len(NAMES)
    offsets = rng.normal(0, 6.0, (nj, 3)).astype(np.float32)
    offsets[:, 1] = np.abs(offsets[:, 1])
    offsets[0] = [0.0, 90.0, 0.0]
    rot = np.clip(synth._smooth(rng, nframes, nj * 3, 14.0), -60.0, 60.0).reshape(nframes, nj, 3).astype(np.float32)
    rot[:, 0, 1] += 35.0            # the character does not face +z: the centring has something to undo
    pos = np.repeat(offsets[None], nframes, axis=0)
    pos[:, 0] += (synth._smooth(rng, nframes, 3, 3.0) * np.array([1.0, 0.1, 1.0]) + np.array([25.0, 0.0, -40.0])).astype(np.float32)
    return dict(rotations=rot, positions=pos, offsets=offsets, parents=np.asarray(PARENTS, np.int32), names=list(NAMES),
                order="zyx", frametime=1.0 / 60.0)


def main():
    from oracle import ref_shims
    from zeggs import synth
    ref = ref_shims.load()
    out, seen = {}, {}

    def pool(block):
        block = np.ascontiguousarray(block)
        key = (block.dtype.str, block.shape, block.tobytes())
        if key not in seen:
            seen[key] = len(seen)
            out[f"pool/{seen[key]}"] = block
        return seen[key]

    with tempfile.TemporaryDirectory() as tmp:
        base = Path(tmp)
        takes = [synth.make_raw_take(n, f, seed=11 + i, style=s, validation=v, anim=small_clip(f, 11 + i), lead=(600 + 7 * i, 10 + i, 25 + 2 * i),
                                     tail=tail, audio_seconds=secs) for i, (n, f, s, v, tail, secs) in enumerate(TAKES)]
        synth.write_raw_corpus(base, takes)
        for path in sorted(base.rglob("*")):
            if path.is_file():
                out["file/" + str(path.relative_to(base))] = np.frombuffer(path.read_bytes(), dtype=np.uint8)
        confs = []
        for i, over in enumerate(CONFS):
            conf = synth.pipeline_conf(base, processed_data_path=f"processed_c{i}", **over)
            confs.append(dict(conf, base_path="."))
            cwd = os.getcwd()
            try:
                data, definition = ref.data_pipeline.data_pipeline(conf)
            finally:
                os.chdir(cwd)
            bounds = sorted(data["ranges_train"].tolist() + data["ranges_valid"].tolist())
            for k, v in data.items():
                v = np.asarray(v)
                if k not in PER_ROW:
                    out[f"c{i}/{k}"] = v
                elif k in PER_JOINT:
                    out[f"c{i}/{k}@pool"] = np.asarray([[pool(v[s:e, :1]), pool(v[s:e, 1:])] for s, e in bounds], np.int32)
                else:
                    out[f"c{i}/{k}@pool"] = np.asarray([pool(v[s:e]) for s, e in bounds], np.int32)
            out[f"c{i}/label_names"] = np.asarray(definition["label_names"])
            out[f"c{i}/dt"] = np.float64(definition["dt"])
            trimmed = base / f"processed_c{i}" / "trimmed"
            for path in sorted(trimmed.rglob("*.bvh")):
                b = ref.bvh.load(str(path))
                table = np.concatenate([b["positions"][:, 0], b["rotations"].reshape(len(b["rotations"]), -1)], axis=1)
                out[f"c{i}/bvh/{path.parent.name}/{path.stem}@pool"] = np.int32(pool(table.astype(np.float32)))
            from scipy.io import wavfile
            for path in sorted(trimmed.rglob("*.wav")):
                fs, x = wavfile.read(str(path))
                assert fs == 16000 and x.dtype == np.int16
                key = f"wav/{path.parent.name}/{path.stem}"
                if key in out:
                    assert np.array_equal(out[key], x), key      # (the audio does not depend on save_trimmed_animation)
                out[key] = x
        out["confs"] = np.asarray(json.dumps(confs))
    ref_shims.release()
    dst = ROOT / "tests" / "golden" / "prepare.npz"
    np.savez_compressed(dst, **out)
    print(f"{dst}: {dst.stat().st_size} bytes, {len(out)} arrays")
    for k in sorted(out):
        if k.startswith("c2/") or k.startswith("file/") or k.startswith("wav/"):
            print(f"  {k}: {out[k].dtype} {out[k].shape}")


if __name__ == "__main__":
    main()
