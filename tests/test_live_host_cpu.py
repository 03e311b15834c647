"""The host contract every stage of live serving keeps (csrc/live_host.h), asked of every entry point that takes records and of
every span report: one table line a call, the same questions of each.  A later stage joins by adding a line.  No GPU needed --
every refusal comes before a launch, the addresses are never followed, and the library loads on the CPU for host-only calls."""
import ctypes

import pytest

from zeggs import audio, capi

ROWS, STATE = 4, ctypes.c_void_p(0x900000)
J5, MAX_HALF = 5, 16


def _loud_dims(rows=ROWS):
    coef = [c for b, a in audio._kweighting(16000) for c in (b[0], b[1], b[2], a[1], a[2])]
    return capi.LoudDims(16000, rows, 20, 1, -20.0, -30.0, 30.0, (ctypes.c_double * 10)(*coef))


def _plant_dims(rows=ROWS):
    return capi.PlantDims(rows, 9, 8, 2, 4, 0, 1 / 60.0, 1.0, 2.0, 1.0, 2.0, 0.0, 5.0, 0.999)


def _frames_dims(rows=ROWS):
    return capi.FramesDims(rows, J5, 20, 7, 0)


# a good record of each kind but for its row: one that has work, so that a call of good records gets as far as its device copy
_HEAD = dict(pose=0x10000, rpos=0x20000, rrot=0x30000, local=0x40000, world=0x50000, bvh=0x60000, pose_ld=6 + 15 * J5, rpos_ld=3, rrot_ld=4, count=4)
_RECORDS = {
    capi.LoudRow: dict(src=0x10000, dst=0x20000, count=96),
    # 48 kHz -> 16 kHz, Z = 4: `outputs` is what ready() asks for
    capi.ResampleRow: dict(src=0x10000, dst=0x20000, table=0x30000, count=96, n_in=0, n_out=0, outputs=audio.resample_ready(96, 1, 3, 12), WL=12,
                           format=0, final=0, L=1, M=3),
    capi.GazeSet: dict(target=(0.0, 1.5, 2.0), pivot=(0.0, 0.0, 0.0), k=5, fade=0, space=0, path=0, ease=0, has_pivot=0),
    capi.GazeCond: dict(k0=4, k_style=0, fade_style=0, n=5),
    capi.StyleMix: dict(k=5, k_style=0, fade_style=0, weight=(1.0,) + (0.0,) * 7, slot=(0,) * 8, temperature=0.0, terms=1, eps_row=-1, reset=0),
    capi.PlantRow: dict(pose=0x10000, rpos=0x20000, rrot=0x30000, out=0x40000, contacts=0x50000, pose_ld=141, rpos_ld=3, rrot_ld=4, out_ld=141, count=4),
    capi.FramesRow: _HEAD,
    capi.RetimeRow: dict(_HEAD, L=3, M=2, n_in=10, outputs=6),                                       # n_out(14) - n_out(10) at 3 / 2
    capi.RefilterRow: dict(_HEAD, L=2, M=5, n_in=20, outputs=2, table=0x80000, half=10, final=0),    # 24 from 60, H = 10
}


def _records(kind, rows):
    arr = (kind * len(rows))()
    for q, row in zip(arr, rows):
        for k, v in dict(_RECORDS[kind], row=row).items():
            setattr(q, k, v)
        if kind is capi.GazeCond:
            q.out_row = row                      # (an output slice a record: checked behind the row)
    return arr


# One line an entry point: its word in every message, its record, its word for the device copy, the size query of its block, what
# stands in front of the records (the dims record first) and what stands behind their count -- `block`: the state block and its
# size, p: a fake address, or NULL in the call without records.
CALLS = {
    "zeggs_live_loudness_push": ("live loudness push", capi.LoudRow, "rows_dev", "zeggs_live_loudness_state_bytes", lambda: (_loud_dims(),),
                                 lambda block, p: block),
    "zeggs_resample_push": ("resample push", capi.ResampleRow, "rows_dev", "zeggs_resample_state_bytes", lambda: (capi.ResampleDims(ROWS, 3072),),
                            lambda block, p: block),
    "zeggs_live_gaze_set": ("live gaze set", capi.GazeSet, "recs_dev", "zeggs_live_gaze_state_bytes", lambda: (capi.GazeDims(ROWS, 64),),
                            lambda block, p: (p(0x10000), 3, p(0x20000), 4, *block)),
    "zeggs_live_condition": ("live condition", capi.GazeCond, "recs_dev", "zeggs_live_gaze_state_bytes", lambda: (capi.GazeDims(ROWS, 64),),
                             lambda block, p: (*block, p(0x10000), p(0x20000), p(0x30000), p(0x40000), ROWS, 5)),
    "zeggs_live_style_mix": ("live style mix", capi.StyleMix, "recs_dev", "zeggs_live_style_bank_bytes", lambda: (capi.StyleBankDims(ROWS, 64, 6),),
                             lambda block, p: (*block, None, 0, p(0x10000), p(0x20000))),
    "zeggs_live_plant": ("plant", capi.PlantRow, "recs_dev", "zeggs_live_plant_state_bytes", lambda: (_plant_dims(),), lambda block, p: block),
    "zeggs_live_frames": ("frames", capi.FramesRow, "rows_dev", "zeggs_live_frames_state_bytes", lambda: (_frames_dims(),), lambda block, p: block),
    "zeggs_live_frames_retimed": ("retime", capi.RetimeRow, "rows_dev", "zeggs_live_retime_state_bytes", lambda: (_frames_dims(),),
                                  lambda block, p: block),
    "zeggs_live_frames_refiltered": ("refilter", capi.RefilterRow, "rows_dev", "zeggs_live_refilter_state_bytes", lambda: (_frames_dims(), MAX_HALF),
                                     lambda block, p: block),
}


def _launch(name, rows, dev=0x7000, records=True):
    """the call with a good record for each of `rows` (records=False: with none, and every tensor NULL) -> its return value, or
    the text of its refusal, which begins with the call's own word"""
    who, kind, _, size_query, front, behind = CALLS[name]
    api, front = capi.api(), front()
    nbytes = getattr(api, size_query)(*front)
    assert nbytes > 0
    recs = _records(kind, rows) if records else None
    dev_p = ctypes.cast(ctypes.c_void_p(dev), ctypes.POINTER(kind)) if dev else None
    try:
        return getattr(api, name)(*front, recs, dev_p, len(rows), *behind((STATE, nbytes), (lambda a: a) if records else (lambda a: None)), None)
    except RuntimeError as e:
        text = api.zeggs_last_error().decode()
        assert str(e) == f"{name}: {text}" and text.startswith(who + ": "), (str(e), text)
        return text


@pytest.mark.parametrize("name", list(CALLS))
def test_every_records_call_keeps_the_record_contract(name):
    who, _, word = CALLS[name][:3]
    # more records than rows
    assert f"{who}: 5 records for 4 rows" in _launch(name, [0, 1, 2, 3, 0])
    # no records: nothing to do, with every pointer NULL
    assert _launch(name, [], dev=None, records=False) == 0
    # records announced, none given
    assert _launch(name, [0, 1], records=False) == f"{who}: NULL records"
    # a row the state does not have, with the record named
    assert _launch(name, [4], dev=None) == f"{who}: record 0: row 4 of 4"
    assert _launch(name, [0, -1]) == f"{who}: record 1: row -1 of 4"
    # a row twice, with the second record named
    assert _launch(name, [2, 1, 2]) == f"{who}: record 2: row 2 twice in one call"
    assert _launch(name, [0, 0, 1]) == f"{who}: record 1: row 0 twice in one call"
    # good records without their device copy (so the table's records ARE good: nothing else stopped them), in the call's own words
    assert _launch(name, [0, 1], dev=None) == f"{who}: 2 records must also be in device memory ({word})"
    assert _launch(name, [3, 1, 0, 2], dev=None) == f"{who}: 4 records must also be in device memory ({word})"


# One line a span report: its word, the dims in front of the row, and the spans a row has (csrc/snapshot_math.h; the ninth and
# the eleventh header for the gaze schedule and the plant stage).
SPANS = {
    "zeggs_live_loudness_spans": ("live loudness spans", lambda rows: (_loud_dims(rows),), 2),
    "zeggs_resample_spans": ("resample spans", lambda rows: (capi.ResampleDims(rows, 3072),), 1),
    "zeggs_live_frames_spans": ("frames spans", lambda rows: (_frames_dims(rows),), 1),
    "zeggs_live_retime_spans": ("retime spans", lambda rows: (_frames_dims(rows),), 1),
    "zeggs_live_refilter_spans": ("refilter spans", lambda rows: (_frames_dims(rows), MAX_HALF), 1),
    "zeggs_live_gaze_spans": ("live gaze spans", lambda rows: (capi.GazeDims(rows, 64),), 1),
    "zeggs_live_plant_spans": ("plant spans", lambda rows: (_plant_dims(rows),), 1),
}


@pytest.mark.parametrize("name", list(SPANS))
def test_every_span_report_keeps_the_span_contract(name):
    who, dims, count = SPANS[name]
    call, room = getattr(capi.api(), name), (capi.SnapSpan * 4)()
    for row in (-1, 8):
        with pytest.raises(RuntimeError, match=f"^{name}: {who}: row {row} of 8$"):
            call(*dims(8), row, room, 4)
    for less in range(count):                    # max_spans = 0, and every other count that is too small
        with pytest.raises(RuntimeError, match=f"^{name}: {who}: room for {less} spans, the row has {count}$"):
            call(*dims(8), 0, room, less)
    with pytest.raises(RuntimeError, match=f"^{name}: {who}: room for 0 spans, the row has {count}$"):
        call(*dims(8), 0, None, 4)
    got = [[(room[i].offset, room[i].bytes) for i in range(call(*dims(8), row, room, 4))] for row in (0, 3, 7)]
    assert [len(g) for g in got] == [count] * 3
    flat = [s for g in got for s in g]
    assert all(b > 0 and o % 4 == 0 and b % 4 == 0 for o, b in flat)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(flat, flat[1:]))          # a row's spans in order, the rows one behind another
    assert call(*dims(8), 7, room, count) == count                            # room for exactly the row's spans is enough
