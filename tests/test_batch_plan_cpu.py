"""Host side of the batch decode (many clips per weight-stationary rollout): the slot planner that deals clips of different
lengths to the rows of the sweep, and the `generate -b/--batch` switch of the command line.  No GPU."""
import json

import pytest

from zeggs.generate import plan_slots


def _frames(piece):
    """the frames of its clip a piece delivers: the given frame 0 with the clip's first piece, then the new ones"""
    _, _, start, count = piece
    return ([0] if start == 0 else []) + list(range(start + 1, start + count + 1))


def _check_plan(lengths, batch, chunk):
    plan = plan_slots(lengths, batch, chunk)
    seen = {j: [] for j in range(len(lengths))}
    last = {}                       # clip -> (row, last frame produced) after the previous chunk
    started = []
    for pieces in plan:
        assert pieces, "a chunk without pieces"
        rows = [r for r, _, _, _ in pieces]
        assert len(set(rows)) == len(rows), "a row holds two clips in one chunk"
        assert all(0 <= r < batch for r in rows)
        clips = [j for _, j, _, _ in pieces]
        assert len(set(clips)) == len(clips), "a clip on two rows at once"
        for r, j, start, count in pieces:
            assert 0 <= count <= chunk - 1 and start + count <= lengths[j] - 1
            if j in last:           # resumed: same row, frame 0 of this chunk = the last frame of the chunk before
                assert last[j] == (r, start), (j, last[j], r, start)
            else:
                assert start == 0
                started.append(j)
            # a clip keeps its row until it ends, and fills the chunk unless it ends in it
            assert count == min(chunk - 1, lengths[j] - 1 - start)
            last[j] = (r, start + count)
            seen[j] += _frames((r, j, start, count))
    assert started == list(range(len(lengths))), "clips start in job order"
    for j, n in enumerate(lengths):
        assert seen[j] == list(range(n)), f"clip {j}: every frame exactly once, in order"
    return plan


def test_plan_mixed_lengths_on_two_rows():
    plan = _check_plan([700, 130, 4, 300, 257, 1], 2, 256)
    # chunk 0: the two first jobs; the 130-frame clip ends inside it and its row idles until the boundary
    assert plan[0] == [(0, 0, 0, 255), (1, 1, 0, 129)]
    # chunk 1: row 0 resumes clip 0 at its frame 255, row 1 takes the next job
    assert plan[1] == [(0, 0, 255, 255), (1, 2, 0, 3)]
    assert plan[2] == [(0, 0, 510, 189), (1, 3, 0, 255)]
    # the 257-frame clip needs a second chunk for ONE frame; the one-frame clip delivers its given frame only
    assert [p for pieces in plan for p in pieces if p[1] == 4] == [(0, 4, 0, 255), (0, 4, 255, 1)]
    assert [p for pieces in plan for p in pieces if p[1] == 5] == [(1, 5, 0, 0)]


def test_plan_more_clips_than_rows():
    plan = _check_plan([5] * 70, 32, 256)
    assert [len(p) for p in plan] == [32, 32, 6]
    assert all(count == 4 for pieces in plan for _, _, _, count in pieces)


@pytest.mark.parametrize("lengths,batch,chunk", [([1], 4, 8), ([1, 1, 1], 2, 4), ([2, 3, 4, 5, 9, 10, 11], 3, 5), ([600] * 32, 32, 256),
                                                 ([1800] * 5, 64, 256), ([7, 1, 300, 2], 1, 64)])
def test_plan_edge_cases(lengths, batch, chunk):
    _check_plan(lengths, batch, chunk)


def test_plan_rejects_what_the_sweep_cannot_run():
    with pytest.raises(ValueError):
        plan_slots([10], 2, 3)          # the sweep needs chunks of 4 frames
    with pytest.raises(ValueError):
        plan_slots([10, 0], 2, 16)      # a clip has at least its first frame
    assert plan_slots([], 2, 16) == []


def test_cli_batch_switch(tmp_path, monkeypatch):
    """`generate -b N -c csv` hands the rows with generate = true to ONE generate_gestures(batch=N) call; without -b the loop over
    generate_gesture() is what it was (both stubbed: no GPU)."""
    from zeggs import cli
    import zeggs.generate as zg
    calls = []
    monkeypatch.setattr(zg, "generate_gesture", lambda **k: calls.append(("one", k)))
    monkeypatch.setattr(zg, "generate_gestures", lambda jobs, **k: calls.append(("many", jobs, k)))
    opts = {"train_opt": {"resume": False}, "net_opt": {},
            "paths": {"base_path": str(tmp_path), "path_processed_data": "data/processed_v1", "output_dir": str(tmp_path / "out"),
                      "models_dir": str(tmp_path / "models")}}
    of = tmp_path / "o.json"
    of.write_text(json.dumps(opts))
    csvf = tmp_path / "p.csv"
    csvf.write_text("base_path,audio,style,file_name,temperature,seed,use_gpu,frames,first_pose,generate\n"
                    f"{tmp_path},a1.wav,s1.bvh,o1,1.0,1234,True,5 50,s1.bvh,True\n"
                    f"{tmp_path},a2.wav,s2.bvh,o2,0.8,99,True,,s2.bvh,False\n"
                    f"{tmp_path},a3.wav,s3.bvh,o3,0.8,99,True,,,True\n")
    assert cli.main(["generate", "-o", str(of), "-c", str(csvf), "--batch", "8"]) == 0
    assert len(calls) == 1 and calls[0][0] == "many"
    _, jobs, k = calls[0]
    assert k["batch"] == 8 and k["style_encoding_type"] == "example" and k["results_path"].name == "results"
    assert k["network_path"] == tmp_path / "models" and k["data_path"] == tmp_path / "data/processed_v1"
    assert [j.file_name for j in jobs] == ["o1", "o3"]
    assert jobs[0].styles == [(tmp_path / "s1.bvh", [5, 50])] and jobs[0].first_pose == tmp_path / "s1.bvh" and jobs[0].seed == 1234
    assert jobs[1].styles == [(tmp_path / "s3.bvh", None)] and jobs[1].first_pose is None
    assert jobs[1].temperature == 0.8 and jobs[1].seed == 99 and jobs[1].audio_file == tmp_path / "a3.wav"
    # the single job of -s / -a goes the same way with -b
    assert cli.main(["generate", "-o", str(of), "-s", "ex.bvh", "-a", "a.wav", "-b", "2", "-r", "7"]) == 0
    assert calls[-1][0] == "many" and len(calls[-1][1]) == 1 and calls[-1][1][0].seed == 7 and calls[-1][2]["batch"] == 2
    # without --batch: one generate_gesture() per row, as before
    n0 = len(calls)
    assert cli.main(["generate", "-o", str(of), "-c", str(csvf)]) == 0
    assert [c[0] for c in calls[n0:]] == ["one", "one"] and [c[1]["file_name"] for c in calls[n0:]] == ["o1", "o3"]
