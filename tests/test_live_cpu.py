"""Host-only parts of live serving (zeggs/live.py, zeggs_mel_window_first_sample): no GPU needed -- the library loads on the CPU for
host-only calls, as in test_abi.py."""
import itertools
import math

import pytest

from zeggs import audio, live, ops

NF, HOP, FS, FPS = 800, 200, 16000, 60.0


def _loads(d, k, pe):
    """every sample index that animation frame k makes the STFT kernels load while the signal continues: the STFT frames of
    zeggs_mel_features_range (mel.hip: m0 = ceil(r k) - 1 clamped at 0, m1 = max(ceil(r k) + 1, 2)), the index rule of their load
    sites (p = m hop + j - n_fft / 2 when centred, src = -p left of the signal), and the sample before when pre-emphasis is on"""
    r = (float(d.fs) / float(d.hop)) / float(d.fps)
    m0, m1 = max(math.ceil(r * k) - 1, 0), max(math.ceil(r * k) + 1, 2)
    out = set()
    for m in range(m0, m1):
        for j in range(d.n_fft):
            p = m * d.hop + j - (0 if d.flags & 1 else d.n_fft // 2)
            src = -p if p < 0 else p
            out.add(src)
            if pe and src > 0:
                out.add(src - 1)
    return out


@pytest.mark.parametrize("centred,pe,k0", list(itertools.product((True, False), (False, True), (0, 1, 2, 7, 60, 10007))))
def test_window_first_sample_is_the_smallest_index_read(centred, pe, k0):
    d = audio.MelDims(NF, HOP, 80, FS, FPS, 1e-5, 0.97 if pe else 0.0, audio.mel_flags(centred, True, "linear"))
    first = ops.mel_window_first_sample(d, k0)
    read = set()
    for k in range(k0, k0 + 9):
        read |= _loads(d, k, pe)
    assert all(first <= i for i in read)
    assert first == min(read)


@pytest.mark.parametrize("tick,depth", [(4, 35), (3, 34), (4, 40), (5, 36), (4, 64)])      # 35 | 1400 frames and 4 | ...; 40, 64: no
def test_step_plan(tick, depth):
    L = live.LOOKAHEAD
    assert live.ring_depth(31, tick) <= depth
    rows = [None,                                                       # free row
            dict(kd=1, n_feat=tick + L + 1, n_ring=0),                  # fresh row, exactly enough features
            dict(kd=1, n_feat=tick + L, n_ring=0),                      # one feature row short
            dict(kd=1 + 7 * tick, n_feat=400, n_ring=7 * tick + L + 1), # running row with a backlog of features
            dict(kd=1401, n_feat=1401 + tick + L, n_ring=1401 + L)]     # far into the stream: the ring has wrapped many times
    plan = live.plan_step(rows, tick, depth)
    assert [p is not None for p in plan] == [False, True, False, True, True]
    for row, p in zip(rows, plan):
        if p is None:
            continue
        assert (p["k0"], p["k1"]) == (row["kd"], row["kd"] + tick)
        assert (p["enc_k0"], p["n_out"]) == (row["kd"] - 1, tick + 1)
        # the ring is fed exactly as far as the last produced frame's look-ahead reaches
        assert row["n_ring"] + p["n_new"] == p["k1"] + L and p["n_new"] <= depth
        assert p["slots"] == [f % depth for f in range(row["n_ring"], row["n_ring"] + p["n_new"])]
        # every frame the step reads is still in the ring afterwards, each in a slot of its own
        need = range(max(p["enc_k0"] - L, 0), p["k1"] + L)
        assert need[0] >= row["n_ring"] + p["n_new"] - depth
        assert len({f % depth for f in need}) == len(need)
    assert plan[1]["n_new"] == tick + L + 1 and plan[3]["n_new"] == tick and plan[4]["slots"][0] == (1401 + L) % depth


def test_style_weight_is_a_step_or_a_ramp():
    assert [live.style_weight(f, 10, 0) for f in (8, 9, 10, 11)] == [0.0, 0.0, 1.0, 1.0]
    w = [live.style_weight(f, 10, 3) for f in range(8, 16)]
    assert w == [0.0, 0.0, 0.25, 0.5, 0.75, 1.0, 1.0, 1.0]


def test_live_symbols_are_exported():
    L = ops.lib()
    for n in ("zeggs_mel_window_first_sample", "zeggs_mel_features_window", "zeggs_speech_encoder_live",
              "zeggs_speech_encoder_live_prepare", "zeggs_speech_encoder_live_workspace_bytes"):
        assert hasattr(L, n), n
    assert L.zeggs_version() >= 106
    d = ops.LiveDims(8, 81, 64, 64, 31, 35, 80, 5)
    assert L.zeggs_speech_encoder_live_workspace_bytes(__import__("ctypes").byref(d)) >= 4 * (81 * 64 + 31 * 64 * 64 + 64 * 64)
