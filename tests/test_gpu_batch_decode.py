"""Batch decode: many clips per weight-stationary rollout (zeggs_decoder_fwd_batch, the inference form of the training
rollout's sweep; ops.decoder_batch_chunk, generate.decode_plan, generate.generate_gestures).  Yardsticks: the CPU oracle
(oracle.nets.decoder_rollout, pinned to the reference's fixtures) and the existing B = 1 persistent decode, never the new path
against itself."""
import json
import warnings

import numpy as np
import pytest
import torch

import helpers
from oracle import anim as oanim
from oracle import nets as onets
from zeggs import generate, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPIN = 1 << 21
KEYS = ("Y_root_pos", "Y_root_rot", "Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt")
OUT = ("pose", "root_pos", "root_rot")


def g(t):
    return t.to(DEV)


@pytest.fixture
def restore_options():
    yield
    for k, v in (("persistent_spin", SPIN), ("train_persistent", 1), ("bwd_persistent", 1), ("persistent", 1)):
        ops.set_option(k, v)


def _decoder():
    _, de, _ = helpers.build_nets()
    return de


def _clips(lengths, seed):
    """per clip: its first pose (a different one per clip, synth.make_clip), a gaze target, random speech / style rows"""
    stats = synth.make_stats()
    rng = np.random.default_rng(seed)
    out = []
    for j, n in enumerate(lengths):
        c = synth.make_clip(4, seed=seed + 17 * j, stats=stats)
        fp = [torch.as_tensor(c[k][:1]) for k in KEYS]
        out.append(dict(fp=fp, gaze=torch.as_tensor(c["Y_gaze_pos"][:1]), n=n,
                        speech=torch.as_tensor(rng.standard_normal((n, 64)).astype(np.float32) * 0.5),
                        style=torch.as_tensor(rng.standard_normal((n, 64)).astype(np.float32) * 0.5)))
    return out


def _firsts(clips):
    res = []
    for c in clips:
        rp, rr, vel, vrt, lpos, ltxy, lvel, lvrt = c["fp"]
        pose0 = torch.cat([x.reshape(1, -1) for x in (vel, vrt, lpos, ltxy, lvel, lvrt)], dim=1)
        res.append(tuple(g(t.to(torch.float32)).contiguous() for t in (pose0, rp, rr, c["gaze"])))
    return res


def _oracle(de, clips, dtype):
    """oracle rollout of the clips as ONE batch (equal lengths) -> (pose, root_pos, root_rot) [B,T,.] in `dtype`"""
    s = helpers.stats_tensors(dtype)
    fp = [torch.cat([c["fp"][i] for c in clips]).to(dtype) for i in range(8)]
    T = clips[0]["n"]
    gaze = torch.stack([c["gaze"].to(dtype).expand(T, 3) for c in clips])
    speech, style = torch.stack([c["speech"] for c in clips]).to(dtype), torch.stack([c["style"] for c in clips]).to(dtype)
    with torch.no_grad():
        o = onets.decoder_rollout(helpers.sd(de, dtype), *fp, gaze, speech, style, s["in_mean"], s["in_std"], s["out_mean"],
                                  s["out_std"], synth.DT)
    return helpers.pack_pose(*o[2:8]), o[0], o[1]


def _batch(de_dev, clips, batch, chunk, fill=0.0, infos=None, status=None):
    """the clips through generate.decode_plan -> per clip (pose, root_pos, root_rot) [L,.] on the host"""
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    lengths = [c["n"] for c in clips]
    bd = ops.BatchDecode(de_dev, batch, min(chunk, max(4, max(lengths))), 64, 64, s["in_mean"], s["in_std"], s["out_mean"],
                         s["out_std"], synth.DT)
    assert bd.sweep, "these dimensions must run on the sweep"
    plan = generate.plan_slots(lengths, batch, chunk)
    got = [[[], [], []] for _ in clips]
    with torch.no_grad():
        for pieces, pose, rpos, rrot in generate.decode_plan(bd, _firsts(clips), [g(c["speech"]) for c in clips],
                                                             [g(c["style"]) for c in clips], plan, status=status, fill=fill,
                                                             infos=infos):
            for r, j, k, n in pieces:
                lo = 0 if k == 0 else 1
                for acc, t in zip(got[j], (pose, rpos, rrot)):
                    acc.append(t[r, lo:n + 1].cpu())
    return [tuple(torch.cat(a) for a in accs) for accs in got]


def _b1(de_dev, clip):
    """the existing B = 1 persistent decode of one clip -> (pose, root_pos, root_rot) [L,.] on the host"""
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    (pose0, rp, rr, gz), = _firsts([clip])
    with torch.no_grad():
        o = ops.decoder_core(de_dev, pose0, rp, rr, gz.expand(clip["n"], 3)[None].contiguous(), g(clip["speech"])[None],
                             g(clip["style"])[None], s["in_mean"], s["in_std"], s["out_mean"], s["out_std"], synth.DT)
    return tuple(t[0].cpu() for t in o)


def _err(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("B", [2, 16, 17, 32, 48, 64])      # every instantiation: 1, 2 (4-row tiles), 3, 4 (4-row tiles) batch tiles
def test_single_chunk_vs_oracle(B):
    """one chunk of 37 frames, state from the CellStateEncoder entry point: every output within 1e-4 of the oracle rollout (the
    bound of test_gpu_parity._oracle_vs_hip_rollout), on the sweep and not on the fall-back"""
    de = _decoder()
    clips = _clips([37] * B, seed=900 + B)
    ref = _oracle(de, clips, torch.float32)
    infos = []
    got = _batch(de.to(DEV).eval(), clips, B, 64, infos=infos)
    assert [i["path"] for i in infos] == ["persistent"] and ops.batch_last_path() == "persistent"
    assert ops.lib().zeggs_persistent_state(1) == 1
    for i, name in enumerate(OUT):
        e = max(_err(got[b][i], ref[i][b]) for b in range(B))
        print(f"B={B} {name}: max |hip - oracle| = {e:.3e}")
        assert e < 1e-4, (name, e)


def test_chunked_resume_vs_float64_oracle():
    """B = 32, 600 frames as chunks of 256 / 256 / 90 frames, each row against the float64 oracle rollout of that row; the
    yardstick is the existing B = 1 persistent decode of the same rows against the same oracle: err_new <= max(2 err_B1, 1e-4)
    per output (2: the different fp32 summation order, MFMA tiles against granule products; 1e-4: the per-step parity figure).
    Measured on an MI355X (err_new / err_B1): pose 1.473e-05 / 1.544e-05, root_pos 2.832e-05 / 2.464e-05, root_rot 3.090e-06 / 3.180e-06"""
    de = _decoder()
    clips = _clips([600] * 32, seed=77)
    ref = _oracle(de, clips, torch.float64)
    de_dev = de.to(DEV).eval()
    infos = []
    got = _batch(de_dev, clips, 32, 256, infos=infos)
    assert [i["path"] for i in infos] == ["persistent"] * 3
    b1 = [_b1(de_dev, c) for c in clips]
    assert ops.lib().zeggs_persistent_state(0) == 1
    for i, name in enumerate(OUT):
        e_new = max(_err(got[b][i], ref[i][b]) for b in range(32))
        e_b1 = max(_err(b1[b][i], ref[i][b]) for b in range(32))
        print(f"{name}: err_new = {e_new:.3e}  err_B1 = {e_b1:.3e}")
        assert got[0][i].shape == ref[i][0].shape
        assert e_new <= max(2 * e_b1, 1e-4), (name, e_new, e_b1)


LENGTHS = [700, 130, 4, 300, 257]


def test_slot_refill_and_padding_never_leaks():
    """the planner drives clips of different lengths through 2 rows: each clip within 5e-5 of its own B = 1 rollout (the bound
    of test_persistent_decode_kernel_matches_stage_launches).  Then the same run with NaN in speech / style / gaze past each
    row's valid frames and in the idle row: live frames finite and within 2e-5 of the clean run (only the split-K atomics of the
    prologue products differ run to run)."""
    de_dev = _decoder().to(DEV).eval()
    clips = _clips(LENGTHS, seed=31)
    infos = []
    clean = _batch(de_dev, clips, 2, 256, infos=infos)
    assert infos and all(i["path"] == "persistent" for i in infos)
    for j, c in enumerate(clips):
        ref = _b1(de_dev, c)
        for i, name in enumerate(OUT):
            assert clean[j][i].shape == ref[i].shape, (j, name)
            e = _err(clean[j][i], ref[i])
            print(f"clip {j} ({c['n']} frames) {name}: max |batch - B1| = {e:.3e}")
            assert e < 5e-5, (j, name, e)
    dirty = _batch(de_dev, clips, 2, 256, fill=float("nan"))
    for j in range(len(clips)):
        for i, name in enumerate(OUT):
            assert torch.isfinite(dirty[j][i]).all(), (j, name)
            e = _err(dirty[j][i], clean[j][i])
            print(f"clip {j} {name}: max |NaN-padded - clean| = {e:.3e}")
            assert e < 2e-5, (j, name, e)


def test_giveup_redoes_the_chunk_on_the_stage_launches(restore_options):
    """a sweep that gives up after its validated first use (persistent_spin = 0 for ONE chunk: the existing bounded-wait hook, used
    once) sets its status bit, the chunk is redone on the stage launches, the clip equals the undisturbed run, and the next
    chunk is back on the sweep"""
    de_dev = _decoder().to(DEV).eval()
    clips = _clips([100, 100], seed=5)
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    good = _batch(de_dev, clips, 2, 64)                       # (validates the sweep on this process)
    assert ops.lib().zeggs_persistent_state(1) == 1
    bd = ops.BatchDecode(de_dev, 2, 64, 64, 64, s["in_mean"], s["in_std"], s["out_mean"], s["out_std"], synth.DT)
    plan = generate.plan_slots([100, 100], 2, 64)
    assert len(plan) == 2
    status = ops.new_status(DEV)
    infos, got = [], [[[], [], []] for _ in clips]
    before = ops.COUNTERS.get("batch_chunks_redone", 0)
    with torch.no_grad(), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        ops.set_option("persistent_spin", 0)
        for c, (pieces, pose, rpos, rrot) in enumerate(generate.decode_plan(bd, _firsts(clips), [g(x["speech"]) for x in clips],
                                                                            [g(x["style"]) for x in clips], plan, status=status,
                                                                            infos=infos)):
            ops.set_option("persistent_spin", SPIN)          # only the first chunk runs with the exhausted bound
            for r, j, k, n in pieces:
                for acc, t in zip(got[j], (pose, rpos, rrot)):
                    acc.append(t[r, (0 if k == 0 else 1):n + 1].cpu())
    assert infos[0]["gave_up"] & 8, infos                    # ZEGGS_GAVE_UP_BATCH_FWD was set by the kernel
    assert infos[0]["path"] == "stage" and any("gave up" in str(w.message) for w in rec)
    assert ops.COUNTERS.get("batch_chunks_redone", 0) == before + 1
    assert infos[1] == {"path": "persistent", "gave_up": 0}
    assert int(status[0].item()) == 0 and ops.lib().zeggs_persistent_state(1) == 1
    for j in range(2):
        for i, name in enumerate(OUT):
            a = torch.cat(got[j][i])
            assert torch.isfinite(a).all()
            e = _err(a, good[j][i])
            print(f"clip {j} {name}: max |redone - undisturbed| = {e:.3e}")
            assert e < 5e-5, (j, name, e)


def _bvh_angle_deg(rot_a, rot_b):
    """largest angle (degrees) between two sets of zyx Euler channels, compared as rotations (no +-180 wrap artefacts)"""
    qa = oanim.q_from_euler(np.radians(np.asarray(rot_a, np.float64)))
    qb = oanim.q_from_euler(np.radians(np.asarray(rot_b, np.float64)))
    return float((2 * np.degrees(np.arccos(np.clip(np.abs(np.sum(qa * qb, axis=-1)), 0, 1)))).max())


def test_generate_gestures_end_to_end(golden_dir, tmp_path):
    """three jobs (the fixture's WAV, its first 60 % and its first 35 %; seeds 1234 / 7 / 99) through
    generate_gestures(batch=2, chunk=64): each BVH against generate_gesture() of the same job, the full-WAV job also against the
    reference's own output, the WAV copies, and return_poses"""
    import scipy.io.wavfile as wavfile
    from zeggs import anim
    gd = np.load(golden_dir / "generate.npz")
    net, data, res, one = tmp_path / "net", tmp_path / "data", tmp_path / "res", tmp_path / "one"
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
    wav = gd["wav"]
    ex = tmp_path / "ex.bvh"
    ex.write_bytes(gd["exemplar_bvh"].tobytes())
    jobs = []
    for tag, frac, seed in (("full", 1.0, 1234), ("p60", 0.6, 7), ("p35", 0.35, 99)):
        wavfile.write(tmp_path / f"{tag}.wav", 16000, wav[:int(len(wav) * frac)])
        jobs.append(generate.Job(tmp_path / f"{tag}.wav", [(ex, None)], file_name=tag, first_pose=ex, temperature=1e8, seed=seed,
                                 blend_type="add", blend_ratio=[1.0]))
    before = ops.COUNTERS.get("batch_chunks_redone", 0)
    encs, poses = generate.generate_gestures(jobs, net, data, res, style_encoding_type="example", batch=2, chunk=64,
                                             return_poses=True)
    assert ops.batch_last_path() == "persistent" and ops.COUNTERS.get("batch_chunks_redone", 0) == before
    assert len(encs) == len(poses) == 3
    for j, (job, enc, P) in enumerate(zip(jobs, encs, poses)):
        tag = job.file_name
        enc1 = generate.generate_gesture(job.audio_file, job.styles, net, data, one, style_encoding_type="example",
                                         blend_type="add", blend_ratio=[1.0], file_name=tag, first_pose=ex, temperature=1e8,
                                         seed=job.seed)
        assert enc.shape == enc1.shape and float((enc - enc1).abs().max()) < 1e-5, tag
        a, b = anim.bvh_load(res / f"{tag}.bvh"), anim.bvh_load(one / f"{tag}.bvh")
        assert a["rotations"].shape == b["rotations"].shape and a["rotations"].shape[0] == enc.shape[1], tag
        ang = _bvh_angle_deg(a["rotations"], b["rotations"])
        print(f"{tag}: {a['rotations'].shape[0]} frames, max angle vs generate_gesture = {ang:.3e} deg")
        assert ang < 2e-2, (tag, ang)
        np.testing.assert_allclose(a["positions"][:, 0], b["positions"][:, 0], atol=2e-3, err_msg=tag)
        assert (res / f"{tag}.wav").read_bytes() == (tmp_path / f"{tag}.wav").read_bytes()
        assert open(res / f"{tag}.bvh").read().split("MOTION")[0] == open(one / f"{tag}.bvh").read().split("MOTION")[0]
        # return_poses: the arrays' BVH conversion gives the same file
        ch = anim.bvh_channels(*P, np.array([0, 0, 0]), np.array([1, 0, 0, 0]))
        anim.write_bvh_channels(str(tmp_path / f"{tag}_poses.bvh"), *ch, parents=synth.PARENTS, names=synth.BONE_NAMES,
                                order="zyx", dt=synth.DT)
        c = anim.bvh_load(tmp_path / f"{tag}_poses.bvh")
        assert c["rotations"].shape == a["rotations"].shape
        assert _bvh_angle_deg(c["rotations"], a["rotations"]) < 1e-3, tag
        np.testing.assert_allclose(c["positions"][:, 0], a["positions"][:, 0], atol=1e-4, err_msg=tag)
    out = anim.bvh_load(res / "full.bvh")
    assert out["rotations"].shape == gd["out_rotations"].shape
    assert float((encs[0].cpu() - torch.as_tensor(gd["encoding"])).abs().max()) < 1e-4
    ang = _bvh_angle_deg(out["rotations"], gd["out_rotations"])
    print(f"full: max angle vs the reference = {ang:.3e} deg")
    assert ang < 2e-2, ang
    np.testing.assert_allclose(out["positions"][:, 0], gd["out_positions"][:, 0], atol=2e-3)


def test_stage_fallback_of_the_batch_entry_point(restore_options):
    """zeggs_decoder_fwd_batch where the sweep does not run -- a chunk of fewer than 4 frames, and the sweep switched off --
    takes the stage launches inside the same call, says so, and is within 1e-4 of the oracle like every other rollout"""
    de, de_dev = _decoder(), _decoder().to(DEV).eval()      # (the same seeded weights: host copy for the oracle)
    s = {k: g(v) for k, v in helpers.stats_tensors().items()}
    for T, off in ((3, False), (9, True)):
        clips = _clips([T] * 3, seed=40 + T)
        ref = _oracle(de, clips, torch.float32)
        try:
            if off:
                ops.set_option("train_persistent", 0)
            bd = ops.BatchDecode(de_dev, 3, 16, 64, 64, s["in_mean"], s["in_std"], s["out_mean"], s["out_std"], synth.DT)
            assert bd.sweep == (not off)
            f = _firsts(clips)
            p0, rp, rr, gz = (torch.cat([x[i] for x in f]) for i in range(4))
            sp, st = g(torch.stack([c["speech"] for c in clips])), g(torch.stack([c["style"] for c in clips]))
            with torch.no_grad():
                h = ops.decoder_state_init(bd, p0, rp, rr, gz, st[:, 0])
                info = {}
                got = ops.decoder_batch_chunk(bd, p0, rp, rr, gz[:, None].expand(3, T, 3).contiguous(), sp, st, h, info=info)
        finally:
            ops.set_option("train_persistent", 1)
        assert info["path"] == "stage", (T, info)
        for i, name in enumerate(OUT):
            e = _err(got[i].cpu(), ref[i])
            print(f"T={T} sweep off={off} {name}: max |stage - oracle| = {e:.3e}")
            assert e < 1e-4, (T, name, e)


@pytest.mark.parametrize("case", ["one_job", "sweep_off"])
def test_jobs_the_sweep_does_not_take_run_the_per_clip_path(case, golden_dir, tmp_path, monkeypatch, restore_options):
    """one job, or a sweep that is not available (switched off here; a FiLM decoder and other dimensions take the same
    branch): the per-clip path of generate_gesture() for every job, networks still loaded once, nothing raises"""
    import scipy.io.wavfile as wavfile
    from zeggs import anim
    gd = np.load(golden_dir / "generate.npz")
    net, data, res = tmp_path / "net", tmp_path / "data", tmp_path / "res"
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
    wavfile.write(tmp_path / "a.wav", 16000, gd["wav"])
    ex = tmp_path / "ex.bvh"
    ex.write_bytes(gd["exemplar_bvh"].tobytes())
    called = []
    orig = generate._decode_one
    monkeypatch.setattr(generate, "_decode_one", lambda *a, **k: (called.append(1), orig(*a, **k))[1])
    job = dict(audio_file=tmp_path / "a.wav", styles=[(ex, None)], file_name="solo", first_pose=ex, temperature=1e8, seed=1234,
               blend_ratio=[1.0])
    njobs = 1 if case == "one_job" else 2
    if case == "sweep_off":
        ops.set_option("train_persistent", 0)
    loads = []
    orig_loaded = generate._Loaded
    monkeypatch.setattr(generate, "_Loaded", lambda *a, **k: (loads.append(1), orig_loaded(*a, **k))[1])
    encs = generate.generate_gestures([dict(job, file_name=f"solo{i}") for i in range(njobs)], net, data, res, batch=32)
    assert len(encs) == njobs and called == [1] * njobs and loads == [1]
    for i in range(njobs):
        out = anim.bvh_load(res / f"solo{i}.bvh")
        assert out["rotations"].shape == gd["out_rotations"].shape and (res / f"solo{i}.wav").exists()
        assert _bvh_angle_deg(out["rotations"], gd["out_rotations"]) < 2e-2
