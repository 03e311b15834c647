"""The mel front-end at STFT shapes other than the shipped 800 / 200 / 80 at 60 fps -- the CPU half: the case table, the fixture
tests/golden/mel_shapes.npz (recorded from the unmodified reference's preprocess_audio by `python -m oracle.make_golden mel_shapes`)
against the float64 restatement oracle/mel.py, three negative controls that show the GPU bound of tests/test_gpu_mel_shapes.py
discriminates at every shape, and the expectation that file asserts: which STFT form (zeggs_mel_last_form) each case reaches.

Cases, 16 kHz, fmin 20, fmax 7600: tag -> (n_fft, hop, n_mels, fps, samples, forms), forms = what zeggs_mel_last_form reports by
default | with mel_fft = 0 | with mel_fft = 0 and mel_mfma = 0 (1 FFT, 2 matrix-core DFT, 3 direct DFT); `dispatch` below restates
the rule of csrc/mel.hip: launch_stft and test_expected_forms_follow_the_dispatch_rule holds the table against it.

  r2     1024 256 80  60 6000   plan 4 4 4 4 2 (a radix-2 stage); 513 bins: the matrix-core form declines
  r2b     400 160 80  50 5000   plan 4 5 5 2; all three forms; r = (fs / hop) / fps = 2 exactly
  big    2048 512 80  30 9000   five radix-4 stages, 145 KB of LDS; direct form at 57 KB
  f3      600 150 80  60 5000   300 = 4 5 5 3: no plan -> matrix-core form by default
  f3d     900 225 80  60 5000   no plan, 451 bins -> direct form by default
  wide    892 223 80  60 5000   no plan, 447 bins fit the matrix-core table, but 31 hops + n_fft samples and 32 x 447 amplitudes
                                need 166 KB of LDS -> direct form by default (the rule's LDS clause, at its first refusal)
  widem   892 150 80  60 5000   the same window at a hop at which the matrix-core form fits (157 KB): its widest table, 447 of 448
                                bin slots, last column tile partly empty
  r5      250 100 40  60 3000   plan 5 5 5; n_fft % 4 != 0; 40 mel channels
  empty   160  80 80 100 3000   plan 4 4 5; all-zero filters; r = 2
  r4      128  64 64  60 3000   plan 4 4 4; all-zero filters
  odd     254  64 32  60 3000   127 is prime, n_fft % 4 = 2: direct form only
  lds    2400 600 80  60 9000   direct form only, 66 KB of LDS (past the 64 KB a kernel gets without the opt-in); 2 NaN rows at the end
  short   512 128 40  60  300   clip shorter than the window, 4 STFT frames, one animation frame
  hop    1024 300 80  60 6000   the hop does not divide n_fft
  gap     400 500 80  30 9000   hop > n_fft
  tiny     10   5  4  60  400   one-stage plan [5]
  many     64  16 80  60 2000   n_mels > n_fft: the FFT form declines; all-zero filters
  slow    640 320 80  60 5000   r = 5/6 < 1

Option cases on those signals: r2 with pre-emphasis, f3 uncentered with the raw dB range, r2b "cubic", r2 "nearest".
"""
import functools

import numpy as np
import pytest

from oracle import mel as omel
from zeggs import synth

FS, FMIN, FMAX, MIN_CLIP, PRE_EMPH = 16000, 20.0, 7600.0, 1e-5, 0.97
FFT, MFMA, DIRECT, FFT_BATCH = 1, 2, 3, 4      # zeggs_mel_last_form
CASES = {
    "r2": (1024, 256, 80, 60, 6000, (FFT, DIRECT, DIRECT)),
    "r2b": (400, 160, 80, 50, 5000, (FFT, MFMA, DIRECT)),
    "big": (2048, 512, 80, 30, 9000, (FFT, DIRECT, DIRECT)),
    "f3": (600, 150, 80, 60, 5000, (MFMA, MFMA, DIRECT)),
    "f3d": (900, 225, 80, 60, 5000, (DIRECT, DIRECT, DIRECT)),
    "wide": (892, 223, 80, 60, 5000, (DIRECT, DIRECT, DIRECT)),
    "widem": (892, 150, 80, 60, 5000, (MFMA, MFMA, DIRECT)),
    "r5": (250, 100, 40, 60, 3000, (FFT, DIRECT, DIRECT)),
    "empty": (160, 80, 80, 100, 3000, (FFT, MFMA, DIRECT)),
    "r4": (128, 64, 64, 60, 3000, (FFT, MFMA, DIRECT)),
    "odd": (254, 64, 32, 60, 3000, (DIRECT, DIRECT, DIRECT)),
    "lds": (2400, 600, 80, 60, 9000, (DIRECT, DIRECT, DIRECT)),
    "short": (512, 128, 40, 60, 300, (FFT, MFMA, DIRECT)),
    "hop": (1024, 300, 80, 60, 6000, (FFT, DIRECT, DIRECT)),
    "gap": (400, 500, 80, 30, 9000, (FFT, MFMA, DIRECT)),
    "tiny": (10, 5, 4, 60, 400, (FFT, DIRECT, DIRECT)),
    "many": (64, 16, 80, 60, 2000, (MFMA, MFMA, DIRECT)),
    "slow": (640, 320, 80, 60, 5000, (FFT, MFMA, DIRECT)),
}
# (tag, name in the fixture, audio_conf overrides, forms): the matrix-core form stages float32 samples and declines pre-emphasis
OPTIONS = (
    ("r2", "pre", {"pre_emphasis": True}, (FFT, DIRECT, DIRECT)),
    ("f3", "uncraw", {"centered": False, "normalize_range": False}, (MFMA, MFMA, DIRECT)),
    ("r2b", "cubic", {"resample_method": "cubic"}, (FFT, MFMA, DIRECT)),
    ("r2", "nearest", {"resample_method": "nearest"}, (FFT, DIRECT, DIRECT)),
)
PLANS = {"r2": [4, 4, 4, 4, 2], "r2b": [4, 5, 5, 2], "big": [4, 4, 4, 4, 4], "r5": [5, 5, 5], "empty": [4, 4, 5], "r4": [4, 4, 4],
         "short": [4, 4, 4, 4], "hop": [4, 4, 4, 4, 2], "gap": [4, 5, 5, 2], "tiny": [5], "many": [4, 4, 2], "slow": [4, 4, 4, 5]}
ZERO_FILTERS = {"empty": 8, "r4": 7, "many": 33, "tiny": 1}      # all-zero rows of the filterbank


# ----------------------------------------------------------------------------- shared with tests/test_gpu_mel_shapes.py
@functools.lru_cache(maxsize=None)
def fixture(golden_dir):
    g = np.load(golden_dir / "mel_shapes.npz")
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def signal(tag, golden_dir):
    """the case's signal, regenerated and held against what the fixture kept of the one the reference saw"""
    n_fft, hop, _, _, n, _ = CASES[tag]
    g = fixture(golden_dir)
    assert int(g[f"{tag}_seed"]) == n_fft + hop and list(g[f"{tag}_dims"]) == list(CASES[tag][:5])
    wav = synth.synth_wav(n, seed=n_fft + hop).astype(np.float32) / 32768.0
    w64 = wav.astype(np.float64)
    np.testing.assert_array_equal(np.concatenate([[w64.sum()], w64[:3], w64[-3:]]), g[f"{tag}_sig"])
    return wav


def n_frames(tag):
    """generate.py:170, what the fixture was recorded with (test_fixture_is_small_and_complete)"""
    return int(round(float(CASES[tag][3]) * (CASES[tag][4] / FS)))


def audio_conf(tag, **over):
    """the audio_conf block a user would write for the case"""
    n_fft, hop, n_mels = CASES[tag][:3]
    conf = dict(pre_emphasis=False, pre_emph_coeff=PRE_EMPH, centered=True, real_amplitude=True,
                normalize_mel_bins=True, normalize_range=True, min_clipping=MIN_CLIP, sampling_rate=FS, mel_fmin=FMIN, mel_fmax=FMAX,
                n_mel_channels=n_mels, filter_length=n_fft, hop_length=hop, resample_method="linear", normalize_loudness=False)
    conf.update(over)
    return conf


def gpu_bound(ref, option):
    """what tests/test_gpu_parity.py applies to this front-end: atol 2e-6 at the shipped options, atol = rtol = 3e-6 at the others"""
    return 3e-6 + 3e-6 * np.abs(ref) if option else np.full(ref.shape, 2e-6)


# ----------------------------------------------------------------------------- the dispatch rule (csrc/mel.hip: launch_stft)
LDS_MAX, MFB_CAP = 160 * 1024, 2048


def fft_plan(m):
    n = {4: 0, 5: 0, 2: 0}
    for r in (4, 5, 2):
        while m % r == 0:
            m //= r
            n[r] += 1
    stages = [4] * n[4] + [5] * n[5] + [2] * n[2]
    return stages if m == 1 and 0 < len(stages) <= 8 else []


def fft_lds(n_fft, n_mels):
    return 8 * 2 * (2 * 4 * (n_fft // 2)) + 8 * MFB_CAP + 4 * 3 * n_mels + 64


def mfma_lds(n_fft, hop, n_mels):
    xs = max(4 * (31 * hop + n_fft), 8 * 32 * n_mels)
    xs = (xs + 15) // 16 * 16
    return xs + 8 * (n_fft + 32 * (n_fft // 2 + 1) + MFB_CAP) + 4 * 3 * n_mels + 64


def direct_lds(n_fft, n_mels):
    return 8 * (3 * n_fft + n_fft // 2 + 1 + n_mels)


def dispatch(n_fft, hop, n_mels, pre_emphasis=False, mel_fft=1, mel_mfma=1):
    if mel_fft and fft_plan(n_fft // 2) and fft_lds(n_fft, n_mels) <= LDS_MAX and n_mels <= n_fft:
        return FFT
    if mel_mfma and not pre_emphasis and n_fft % 4 == 0 and 2 * (n_fft // 2 + 1) <= 896 and mfma_lds(n_fft, hop, n_mels) <= LDS_MAX:
        return MFMA
    assert direct_lds(n_fft, n_mels) <= LDS_MAX
    return DIRECT


def test_expected_forms_follow_the_dispatch_rule():
    for tag, (n_fft, hop, n_mels, _, _, forms) in CASES.items():
        got = tuple(dispatch(n_fft, hop, n_mels, False, f, m) for f, m in ((1, 1), (0, 1), (0, 0)))
        assert got == forms, tag
        assert fft_plan(n_fft // 2) == PLANS.get(tag, []), tag
    for tag, name, over, forms in OPTIONS:
        n_fft, hop, n_mels = CASES[tag][:3]
        got = tuple(dispatch(n_fft, hop, n_mels, over.get("pre_emphasis", False), f, m) for f, m in ((1, 1), (0, 1), (0, 0)))
        assert got == forms, (tag, name)
    # what the cases are for
    assert {f for c in CASES.values() for f in c[5]} == {FFT, MFMA, DIRECT}
    assert fft_lds(2048, 80) == 148480 and direct_lds(2048, 80) == 57992                          # big
    assert 64 * 1024 < direct_lds(2400, 80) == 67848 and direct_lds(2316, 80) <= 64 * 1024 < direct_lds(2318, 80)      # lds
    assert direct_lds(5828, 80) <= LDS_MAX < direct_lds(5830, 80) < direct_lds(8192, 80) == 230024
    assert 2 * (892 // 2 + 1) == 894 and 2 * (900 // 2 + 1) > 896                                # wide / widem, f3d
    assert mfma_lds(892, 223, 80) == 170208 > LDS_MAX >= mfma_lds(892, 150, 80) == 161152
    assert CASES["many"][2] > CASES["many"][0] and fft_plan(32) == [4, 4, 2]                     # the n_mels <= n_fft clause alone declines
    ratio = {tag: (FS / c[1]) / c[3] for tag, c in CASES.items()}
    assert ratio["r2b"] == ratio["empty"] == 2.0 and ratio["slow"] == 50.0 / 60.0 and ratio["gap"] > 1.0 > ratio["lds"]
    assert CASES["hop"][0] % CASES["hop"][1] != 0 and CASES["gap"][1] > CASES["gap"][0] and CASES["short"][4] < CASES["short"][0]


def test_fixture_is_small_and_complete(golden_dir):
    g = fixture(golden_dir)
    assert (golden_dir / "mel_shapes.npz").stat().st_size < 200 * 1024 and float(g["pre_emph_coeff"]) == PRE_EMPH
    assert list(g["tags"]) == list(CASES) and list(g["options"]) == [f"{t}:{o}" for t, o, _, _ in OPTIONS]
    assert not any(k.endswith("_wav") for k in g)
    for tag, (n_fft, hop, n_mels, fps, n, _) in CASES.items():
        assert n_frames(tag) == int(g[f"{tag}_nframes"])
        assert g[f"{tag}_feat"].dtype == np.float32 and g[f"{tag}_feat"].shape == (n_frames(tag), n_mels + 1)
        fb = omel.mel_filterbank(n_fft, FS, n_mels, FMIN, FMAX)
        assert int((~fb.any(axis=1)).sum()) == ZERO_FILTERS.get(tag, 0), tag
    assert n_frames("short") == 1 and int(g["short_M"]) == 4
    nan_rows = {tag: int(np.isnan(g[f"{tag}_feat"]).any(axis=1).sum()) for tag in CASES}
    assert nan_rows.pop("lds") == 2 and not any(nan_rows.values())
    assert np.isnan(g["lds_feat"][-2:, :-1]).all() and np.isfinite(g["lds_feat"][:, -1]).all()      # (the energy extrapolates)


# ----------------------------------------------------------------------------- oracle/mel.py == the reference, at every case
def _oracle(golden_dir, tag, **over):
    n_fft, hop, n_mels, fps, _, _ = CASES[tag]
    c = audio_conf(tag, **over)
    return omel.preprocess_audio(signal(tag, golden_dir), n_frames(tag), fs=FS, hop=hop, fps=float(fps), resample_method=c["resample_method"],
                                 n_fft=n_fft, n_mels=n_mels, fmin=FMIN, fmax=FMAX, min_clip=MIN_CLIP,
                                 pre_emph=c["pre_emph_coeff"] if c["pre_emphasis"] else 0.0, centered=c["centered"],
                                 normalize_range=c["normalize_range"])


ALL = [(tag, "", {}) for tag in CASES] + [(tag, name, over) for tag, name, over, _ in OPTIONS]


@pytest.mark.parametrize("tag,name,over", ALL, ids=[t + ("_" + n if n else "") for t, n, _ in ALL])
def test_oracle_equals_the_reference_fixture(tag, name, over, golden_dir):
    """NaN pattern equal, values within 1e-7 (measured: 0 everywhere but the cubic case, 1e-18 there), and the reference's STFT frame
    count is oracle.mel.stft_frame_count"""
    g = fixture(golden_dir)
    sfx = f"_{name}" if name else ""
    ref, got = g[f"{tag}_feat{sfx}"], _oracle(golden_dir, tag, **over)
    assert got.dtype == np.float32 and got.shape == ref.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    err = float(np.nanmax(np.abs(got.astype(np.float64) - ref)))
    print(f"{tag}{sfx}: max |oracle - reference| = {err:.3e}")
    assert err <= 1e-7
    n_fft, hop, _, _, n, _ = CASES[tag]
    assert int(g[f"{tag}_M{sfx}"]) == omel.stft_frame_count(n, n_fft, hop, over.get("centered", True))


# ----------------------------------------------------------------------------- the bound discriminates
def _periodic_hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def _control(monkeypatch, which):
    if which == "periodic_hann":
        monkeypatch.setattr(omel, "hann_symmetric", _periodic_hann)
    elif which == "filterbank_one_bin":
        fb = omel.mel_filterbank
        monkeypatch.setattr(omel, "mel_filterbank", lambda *a, **k: np.roll(fb(*a, **k), 1, axis=1))
    else:
        spec = omel.mel_spectrogram
        monkeypatch.setattr(omel, "mel_spectrogram", lambda wav, **k: spec(np.concatenate([wav[1:], wav[:1] * 0]), **k))


@pytest.mark.parametrize("which", ["periodic_hann", "filterbank_one_bin", "signal_one_sample"])
def test_deliberate_errors_are_ten_bounds_away_at_every_shape(monkeypatch, which, golden_dir):
    """three errors a kernel could make -- scipy's periodic window instead of the symmetric one, the filterbank one bin off, the
    signal one sample off -- put into the ORACLE (patched here, oracle/mel.py is as it is): each moves the features by at least ten
    times the GPU test's bound somewhere, at every shape"""
    _control(monkeypatch, which)
    g = fixture(golden_dir)
    shifts = {}
    for tag in CASES:
        ref, got = g[f"{tag}_feat"], _oracle(golden_dir, tag)
        excess = np.abs(got.astype(np.float64) - ref) / gpu_bound(ref, False)
        shifts[tag] = float(np.nanmax(excess)) * 2e-6
    print(which, {t: f"{s:.1e}" for t, s in shifts.items()})
    assert all(s >= 10 * 2e-6 for s in shifts.values()), shifts
