"""Host side of the dataset builder (zeggs/data_pipeline.py), no GPU: timecode and speaker-interval parsing against hand-computed
sample indices, range / label bookkeeping, the conf keys that are refused, the raw-corpus writer the tests and tools share."""
import json

import numpy as np
import pytest

from zeggs import data_pipeline as dp
from zeggs import synth


def test_timecodes_to_sixtieths():
    # audio timecodes count 30 frames per second (a frame = 2 sixtieths), animation / acting timecodes 60
    assert dp.timecode_to_sixtieths("00:00:00:00", 1) == 0
    assert dp.timecode_to_sixtieths("09:28:00:01", 2) == 9 * 216000 + 28 * 3600 + 2
    assert dp.timecode_to_sixtieths("09:28:03:35", 1) == 9 * 216000 + 28 * 3600 + 3 * 60 + 35
    assert dp.timecode_to_sixtieths("01:00:00:29", 2) == 216000 + 58


def test_take_timing_against_hand_computed_indices():
    # first row of the reference's data/info.csv: audio 09:28:00:01 (30 fps), animation 09:28:03:35, acting 09:28:15:21 .. 09:30:16:47
    row = dict(audio_start_time="09:28:00:01", anim_start_time="09:28:03:35", acting_start_time="09:28:15:21", acting_end_time="09:30:16:47")
    # acting start - audio start = 15 s 21 f - 2 sixtieths = 919 sixtieths -> 919 * 16000 / 60 = 245066.67 -> 245067
    # acting end   - audio start = 136 s 47 f - 2 = 8205 sixtieths -> 2188000 exactly
    # frames: 919 + 2 - 215 = 706;  8205 + 2 - 215 = 7992
    assert dp.take_timing(row, 16000) == (245067, 2188000, 706, 7992)


def test_take_timing_rounds_halves_to_even_like_numpy():
    base = dict(audio_start_time="00:00:00:00", anim_start_time="00:00:00:00")
    # 22 050 Hz: 367.5 samples per sixtieth.  1 sixtieth -> 367.5 -> 368 (even), 3 -> 1102.5 -> 1102 (even), 5 -> 1837.5 -> 1838
    assert dp.take_timing(dict(base, acting_start_time="00:00:00:01", acting_end_time="00:00:00:03"), 22050)[:2] == (368, 1102)
    assert dp.take_timing(dict(base, acting_start_time="00:00:00:05", acting_end_time="00:00:01:00"), 22050)[:2] == (1838, 22050)
    # 16 kHz: 266.67 per sixtieth: 1 -> 267, 2 -> 533, 25 -> 6667
    assert dp.take_timing(dict(base, acting_start_time="00:00:00:01", acting_end_time="00:00:00:02"), 16000)[:2] == (267, 533)
    assert dp.take_timing(dict(base, acting_start_time="00:00:00:25", acting_end_time="00:00:01:00"), 16000) == (6667, 16000, 25, 60)


def test_take_timing_refuses_an_acting_span_before_the_recordings():
    row = dict(audio_start_time="00:00:10:00", anim_start_time="00:00:10:10", acting_start_time="00:00:10:05", acting_end_time="00:00:12:00")
    with pytest.raises(ValueError, match="The timings are incorrect!"):       # the animation starts after the acting
        dp.take_timing(row, 16000)
    row = dict(audio_start_time="00:00:10:10", anim_start_time="00:00:10:00", acting_start_time="00:00:10:05", acting_end_time="00:00:12:00")
    with pytest.raises(ValueError, match="The timings are incorrect!"):       # the audio starts after the acting (10:10 at 30 fps = 20 sixtieths)
        dp.take_timing(row, 16000)


def test_speaker_intervals():
    assert dp.speaker_time_to_sample("0:00.200", 16000) == 3200
    assert dp.speaker_time_to_sample("1:02.500", 16000) == 62 * 16000 + 8000
    assert dp.speaker_time_to_sample("0:01.275", 16000) == 16000 + 4400
    # the milliseconds are multiplied by fs / 1000 and truncated: 333 ms at 22 050 Hz = 7342.65 -> 7342
    assert dp.speaker_time_to_sample("0:00.333", 22050) == 7342
    # ... and are an integer of their own: ".5" is 5 ms, not half a second (the reference's int(), kept)
    assert dp.speaker_time_to_sample("0:01.5", 16000) == 16000 + 80
    rows = [{"#": "R1", "Start": "0:00.200", "End": "0:01.000"}, {"#": "L1", "Start": "0:01.000", "End": "0:02.000"},
            {"#": "M2", "Start": "0:02.000", "End": "0:02.100"}, {"#": "R2", "Start": "0:02.100", "End": "1:00.000"}]
    iv = dp.speaker_intervals(rows, 16000)
    assert iv.dtype == np.int64 and iv.tolist() == [[3200, 16000], [33600, 960000]]
    assert dp.speaker_intervals(rows[1:3], 16000).shape == (0, 2)              # nobody to keep: everything is silenced


def test_validation_flag_and_trimmed_names():
    assert [dp.is_validation(v) for v in ("TRUE", "True", "1", "FALSE", "false", "0", "")] == [True, True, True, False, False, False, False]
    assert dp.trimmed_name("001_Neutral_0.bvh", 0.9) == "001_Neutral_0_x_0_9"
    assert dp.trimmed_name("001_Neutral_0.bvh", 1.0) == "001_Neutral_0_x_1_0"


def test_ranges_and_labels_bookkeeping():
    r = dp.Ranges()
    assert r.add(117, "Sad", False) == [0, 117]
    assert r.add(130, "Sad", False) == [117, 247]
    assert r.add(90, "Old", True) == [247, 337]
    assert r.add(100, "Happy", False) == [337, 437]
    assert r.add(3, "Happy", False) == [437, 440]                 # e - s <= 4: contributes no row to the statistics
    tr, va, trl, val, names = r.finish()
    assert names == ["Sad", "Happy", "Old"]                       # first appearance, train before valid
    assert tr.dtype == va.dtype == trl.dtype == val.dtype == np.int32
    assert tr.tolist() == [[0, 117], [117, 247], [337, 437], [437, 440]] and va.tolist() == [[247, 337]]
    assert trl.tolist() == [0, 0, 1, 1] and val.tolist() == [2]
    mask = r.stats_mask()
    assert mask.shape == (440,) and mask.sum() == 113 + 126 + 96
    assert not mask[:2].any() and mask[2] and mask[114] and not mask[115:119].any() and mask[119]
    assert not mask[245:339].any() and not mask[435:].any()      # the validation take and the 3-row take stay out
    totals = dp.label_totals(tr, va, trl, val, names)
    assert totals == [("Sad", 123.5, 0.0), ("Happy", 51.5, 0.0), ("Old", 0.0, 45.0)]


def test_empty_validation_bookkeeping():
    r = dp.Ranges()
    r.add(50, "Sad", False)
    tr, va, trl, val, names = r.finish()
    assert va.shape == (0, 2) and va.dtype == np.int32 and val.shape == (0,) and val.dtype == np.int32
    assert dp.label_totals(tr, va, trl, val, names) == [("Sad", 25.0, 0.0)]      # (the reference's summary table dies here)


@pytest.mark.parametrize("key", ["visualize_spectrogram", "visualize_gaze", "save_normalized_animations"])
def test_cosmetic_conf_keys_are_refused_by_name(tmp_path, key):
    conf = synth.pipeline_conf(tmp_path, **{key: True})
    with pytest.raises(NotImplementedError, match=key):
        dp.data_pipeline(conf)
    assert not (tmp_path / "processed").exists()                  # refused before anything is written
    dp.check_conf(synth.pipeline_conf(tmp_path))


def test_raw_corpus_writer_round_trips_through_the_readers(tmp_path):
    from zeggs import anim
    takes = [synth.make_raw_take("a_Happy", 40, seed=3, style="Happy"), synth.make_raw_take("b_Sad", 30, seed=4, style="Sad", validation=True)]
    info = synth.write_raw_corpus(tmp_path, takes)
    rows = dp.read_csv_rows(info)
    assert [r["anim_bvh"] for r in rows] == ["a_Happy.bvh", "b_Sad.bvh"] and [dp.is_validation(r["validation"]) for r in rows] == [False, True]
    a0, a1, f0, f1 = dp.take_timing(rows[0], 16000)
    assert (f0, f1) == (15, 35) and a0 == 6667 and a1 == int(np.round(45 * 16000 / 60))
    wav = dp.read_wav(tmp_path / "original" / "a_Happy.wav", 16000)
    assert wav.dtype == np.float32 and len(wav) >= a1 and np.abs(wav).max() <= 1.0
    assert np.array_equal(wav, takes[0]["wav"].astype(np.float32) / 32768.0)
    with pytest.raises(ValueError, match="16000"):
        dp.read_wav(tmp_path / "original" / "a_Happy.wav", 22050)
    iv = dp.speaker_intervals(dp.read_csv_rows(tmp_path / "original" / "a_Happy.csv"), 16000)
    assert iv.shape == (2, 2) and iv[0, 0] == 3200 and iv[0, 1] < iv[1, 0] <= iv[1, 1]
    clip = anim.bvh_load(tmp_path / "original" / "a_Happy.bvh")
    assert clip["rotations"].shape == (40, 75, 3) and int(np.ceil(1 / clip["frametime"])) == 60
    json.dumps(synth.pipeline_conf(tmp_path))


def test_prepare_command_line(tmp_path, capsys):
    from zeggs import cli
    with pytest.raises(SystemExit):
        cli.main(["prepare"])                                     # -c is required
    conf = synth.pipeline_conf(tmp_path, visualize_gaze=True)
    (tmp_path / "conf.json").write_text(json.dumps(conf))
    with pytest.raises(NotImplementedError, match="visualize_gaze"):
        cli.main(["prepare", "-c", str(tmp_path / "conf.json"), "--base-path", str(tmp_path)])
