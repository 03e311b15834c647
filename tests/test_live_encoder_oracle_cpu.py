"""The yardstick of tests/test_gpu_live_dims.py, examined on the host: the incremental scheme of csrc/live.hip restated in float64
(oracle/live.py: rings with frame f in slot f % D, taps clamped to [0, top], the same per-row records), driven by the schedules of
helpers.live_schedule for every case of helpers.LIVE_KERNEL_CASES.

  * it equals the whole-row oracle (oracle.nets.speech_encoder, float64) to 1e-12: the schedules and records state the computation;
  * every record passes the argument checks of zeggs_speech_encoder_live restated in oracle/live.py (check_row), the dimensions
    pass live_dims_ok (check_dims), and the schedules between them contain what the device test relies on (listed in
    test_schedules_reach_what_they_claim);
  * the same restatement in float32 -- normalisation included -- stays within a quarter of helpers.SPEECH_OUT_BOUND (measured:
    1e-7 .. 6e-7 over the seven cases), so a correct float32 kernel has room;
  * each mistake of oracle.live.BUGS moves some frame by >= 10x the bound -- except where the mistake is the identity by
    construction, which is asserted too: "pack_h_o_swapped" at H == O, "taps_reversed" and "zero_padding" at KW = 1 (one tap, no
    padding)."""
import pytest
import torch

import helpers as H
from oracle import live as olive

CASES = H.LIVE_KERNEL_CASES
IDS = [c["id"] for c in CASES]


def _run(case, dtype=torch.float64, bug=None):
    d = H.live_case_data(case)
    s = d["sched"]
    with torch.no_grad():
        return olive.encoder_incremental(H.live_case_weights(d["net"]), d["mean"], d["std"], lambda c: H.live_feat_block(d, c),
                                         s["calls"], case["R"], s["D"], dtype=dtype, bug=bug)


def _worst(case, got):
    ref = H.live_case_data(case)["ref"]
    assert [tuple(g.shape) for g in got] == [tuple(r.shape) for r in ref]
    return max(H.relerr(g, r) for g, r in zip(got, ref))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_incremental_restatement_equals_the_whole_row_oracle(case):
    e = _worst(case, _run(case))
    print(f"{case['id']}: float64 incremental vs whole row {e:.2e}")
    assert e <= 1e-12, e


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_restatement_keeps_a_quarter_of_the_bound(case):
    e = _worst(case, _run(case, torch.float32))
    print(f"{case['id']}: float32 incremental vs float64 whole row {e:.2e}")
    assert e <= H.SPEECH_OUT_BOUND / 4, e


def _identity(case, bug):
    return (bug == "pack_h_o_swapped" and case["H"] == case["O"]) or (bug in ("taps_reversed", "zero_padding") and case["KW"] == 1)


@pytest.mark.parametrize("bug", olive.BUGS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_each_mistake_is_far_outside_the_bound(case, bug):
    e = _worst(case, _run(case, bug=bug))
    print(f"{case['id']} {bug}: {e:.2e}")
    if _identity(case, bug):
        assert e <= 1e-12, e
    else:
        assert e >= 10 * H.SPEECH_OUT_BOUND, e


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_record_passes_the_c_checks(case):
    s = H.live_schedule(case)
    assert olive.check_dims(case["R"], case["F"], case["H"], case["O"], case["KW"], s["D"], s["feat_ld"], s["out_ld"]) is None
    done, n_ring = [0] * case["R"], [0] * case["R"]
    for c, recs in enumerate(s["calls"]):
        assert len(recs) == case["R"]
        for r, rec in enumerate(recs):
            assert olive.check_row(rec, case["KW"], s["D"], s["feat_ld"], s["out_ld"]) is None, (c, r, rec)
            if rec[3] or rec[4]:
                assert rec[0] == n_ring[r] and rec[1] == done[r], (c, r, rec)       # frames arrive and leave in order, none twice
            n_ring[r] += rec[3]
            done[r] += rec[4]
    assert done == n_ring == s["lens"]


def test_the_lds_figures():
    assert olive.lds_bytes(81, 256, 16, 29) == 64144 <= olive.LDS_LIMIT < olive.lds_bytes(*H.LIVE_LDS_REFUSED) == 66192
    assert olive.check_dims(3, *H.LIVE_LDS_REFUSED, 80, 8, 8) == "bytes of LDS"
    assert all(olive.lds_bytes(c["F"], c["H"], c["O"], c["KW"]) <= olive.LDS_LIMIT for c in CASES)


def test_schedules_reach_what_they_claim():
    """per case: bursts of 1, FRP - 1, FRP, FRP + 1 and D; a ring-fill-only call and an output-only call; an output of several
    passes with a partial last one; feat_off non-zero and feat_ld far below the long row; the long rows wrap the ring at least
    twice and the ring is the least the schedule needs; rows finish at different calls and are skipped afterwards.  Between the
    cases: rows of 1, 2, half, half + 1, KW - 1 and KW frames delivered and ended in one call."""
    one_call = set()
    for case in CASES:
        s = H.live_schedule(case)
        KW, D, FRP, half = case["KW"], s["D"], 512 // case["O"], (case["KW"] - 1) // 2
        recs = [rec for call in s["calls"] for rec in call]
        bursts = {rec[3] for rec in recs}
        assert {1, FRP, FRP + 1, D} <= bursts and (FRP == 1 or FRP - 1 in bursts), (case["id"], sorted(bursts))
        assert any(rec[3] > 0 and rec[4] == 0 for rec in recs) and any(rec[3] == 0 and rec[4] > 0 for rec in recs)
        assert any(rec[4] > FRP and (FRP == 1 or rec[4] % FRP) for rec in recs), case["id"]      # (FRP = 1 has no partial pass)
        assert any(rec[5] > 0 and rec[3] > 0 for rec in recs) and s["feat_ld"] <= max(s["lens"]) // 2
        assert max(s["lens"]) == case["long"] > 2 * D
        need = max([KW] + [rec[3] for rec in recs] +
                   [rec[0] + rec[3] - max(rec[1] - half, 0) for rec in recs if rec[4] > 0 and rec[2] < 0])
        assert need == D, (case["id"], need, D)
        last_call = [max(c for c, call in enumerate(s["calls"]) if call[r][3] or call[r][4]) for r in range(case["R"])]
        assert len(set(last_call)) >= min(case["R"], 3) // 2 + 1 and min(last_call) < len(s["calls"]) - 1
        for r, n in enumerate(s["lens"]):
            if n <= KW:
                mine = [call[r] for call in s["calls"] if call[r][3] or call[r][4]]
                assert len(mine) == 1 and mine[0][2:5] == (n - 1, n, n), (case["id"], r, mine)
                one_call.add((n, KW))
    kw = 31
    assert {(n, kw) for n in (1, 2, 15, 16, 30, 31)} <= one_call, sorted(one_call)
    assert len(set(H.live_case_lens(CASES[0]))) == 64 and min(H.live_case_lens(CASES[0])) == 1
