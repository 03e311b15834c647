"""Host side of the held-out evaluation (zeggs/evaluate.py): the window plan, the style-example rule for arbitrary ranges, the
round-robin shards, and the per-window float64 oracle the GPU tests compare the kernel with (tests/eval_helpers.py)."""
import numpy as np
import pytest
import torch

import eval_helpers
import helpers
from oracle import loss as oloss
from zeggs import evaluate, synth

W = 8


def test_plan_windows_counts_and_admissible_starts():
    ranges = np.array([[0, W], [20, 20 + W + 1], [40, 40 + 2 * W], [70, 70 + 2 * W + 1]])
    starts, index = evaluate.plan_windows(ranges, W)
    assert np.bincount(index, minlength=4).tolist() == [0, 1, 1, 2]
    assert starts.tolist() == [20, 40, 70, 70 + W] and index.tolist() == [1, 2, 3, 3]
    assert starts.dtype == np.int64 and index.dtype == np.int64
    # every start is a window of the training table of a dataset with these ranges as its training ranges
    ds = eval_helpers.plan_dataset(ranges, W)
    assert set(starts.tolist()) <= set(ds.win_start.tolist())
    for s, i in zip(starts, index):
        assert ds.win_sample[ds.win_start.tolist().index(s)] == i


def test_plan_windows_empty():
    for ranges in ([], np.zeros((0, 2), np.int64)):
        starts, index = evaluate.plan_windows(ranges, W)
        assert starts.shape == (0,) and index.shape == (0,)


@pytest.mark.parametrize("example_len", [16, 33])
def test_example_rows_for_is_the_dataset_rule(example_len):
    """windows at a range's start, middle and end (stride 1: every admissible start), two ranges, one at the end of the data"""
    ranges = np.array([[3, 45], [50, 90]])
    ds = eval_helpers.plan_dataset(ranges, W)
    ds.n_frames = 90                                 # the last range ends with the data: the rule's clamp to n_frames
    idx = np.arange(len(ds))
    want = ds.example_rows(idx, example_len)
    got = evaluate.example_rows_for(ds.win_start[idx], ranges, ds.win_sample[idx].astype(np.int64), W, example_len, ds.n_frames)
    assert got.dtype == want.dtype and got.shape == (len(idx), example_len)
    np.testing.assert_array_equal(got, want)
    starts, index = evaluate.plan_windows(ranges, W)      # ... and the plan's own windows
    pos = [ds.win_start.tolist().index(s) for s in starts]
    np.testing.assert_array_equal(evaluate.example_rows_for(starts, ranges, index, W, example_len, ds.n_frames),
                                  ds.example_rows(np.asarray(pos), example_len))


def test_example_longer_than_the_data_in_front_of_it_is_refused():
    """the rule places an example that does not fit into [start, end) so that it ENDS at `end`: longer than `end` frames, it would
    start before frame 0 -- rows the device gather would read unchecked.  Refused on the host; the longest example that fits passes."""
    ranges = np.array([[42, 63], [63, 84]])
    starts, index = evaluate.plan_windows(ranges, W)
    assert evaluate.example_rows_for(starts, ranges, index, W, 86, 84).min() == 0
    with pytest.raises(ValueError, match="example_len 88"):
        evaluate.example_rows_for(starts, ranges, index, W, 88, 84)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_shards_partition_the_batches(world):
    for nb in (0, 1, 2, 7):
        parts = [evaluate.shard(nb, world, r) for r in range(world)]
        assert sorted(b for p in parts for b in p) == list(range(nb))
        assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1


def test_summarise_weights_the_kl_and_counts():
    table = np.zeros((3, 23))
    table[0, :17], table[0, 17], table[0, 22] = 2.0, 4.0, 2          # two windows of label 0
    table[2, :17], table[2, 17], table[2, 18], table[2, 22] = 3.0, 1.0, 5.0, 1
    r = evaluate.summarise(table, W, iteration=None)
    assert r["windows"] == 3 and r["frames_scored"] == 3 * W and sorted(r["per_label"]) == [0, 2]
    assert r["loss"] == pytest.approx(17 * (5.0 / 3) / 18) and r["kl"] == pytest.approx(5.0 / 3)
    assert r["per_label"][2]["mpjpe"] == 5.0 and r["per_label"][0]["windows"] == 2
    k = oloss.kl_weight(9000)
    r9 = evaluate.summarise(table, W, iteration=9000)
    assert r9["loss"] == pytest.approx((17 * (5.0 / 3) + k * 5.0 / 3) / 18)
    assert r9["terms"]["loss_kl_div"] == pytest.approx(k * 5.0 / 3) and list(r9["terms"]) == list(__import__("zeggs.train").train.LOSS_TAGS)
    empty = evaluate.summarise(np.zeros((3, 23)), W)
    assert empty["windows"] == 0 and np.isnan(empty["loss"]) and empty["per_label"] == {}


# ----------------------------------------------------------------------------- the per-window oracle
CASE = ("rig", 3, 7, "general")


def test_oracle_rows_average_to_the_training_terms():
    d = helpers.loss_case(CASE)
    rows = eval_helpers.rows_oracle(d)
    _, terms = oloss.training_loss([o.double() for o in d["O"]], [w.double() for w in d["W"]], d["gaze"].double(), d["parents"],
                                   synth.DT, d["mu"].double(), d["logvar"].double(), iteration=helpers.LOSS_KL_ITERATION)
    np.testing.assert_allclose(rows[:, :17].mean(0).numpy(), terms[:17].numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(oloss.kl_weight(helpers.LOSS_KL_ITERATION) * float(rows[:, 17].mean()), float(terms[17]), rtol=1e-12)
    assert float(rows.min()) > 0


def test_oracle_row_of_the_truth_is_zero():
    d = eval_helpers.with_row_as_truth(helpers.loss_case(CASE), 1)
    rows = eval_helpers.rows_oracle(d)
    assert float(rows[1, :20].abs().max()) == 0.0
    assert float(rows[1, 20]) == float(rows[1, 21]) > 0
    assert float(rows[0, :20].min()) > 0 and float(rows[2, :20].min()) > 0


def test_oracle_sees_differences_across_windows():
    d = helpers.loss_case(CASE)
    good, bad = eval_helpers.rows_oracle(d), eval_helpers.rows_oracle(d, bug="diff_across_windows")
    diff = list(oloss.DIFF_TERMS)
    assert (good[:-1][:, diff] != bad[:-1][:, diff]).all()
    rel = ((good[:-1][:, diff] - bad[:-1][:, diff]).abs() / good[:-1][:, diff]).min()
    assert float(rel) > 100 * helpers.LOSS_TERM_BOUND["rtol"], float(rel)      # far outside the bound of the GPU comparison
    assert torch.equal(good[-1], bad[-1])
    keep = [c for c in range(22) if c not in diff]
    assert torch.equal(good[:, keep], bad[:, keep])
