"""The mel front-end on the device at STFT shapes other than the shipped 800 / 200 / 80 at 60 fps, against the fixture recorded from
the unmodified reference (tests/golden/mel_shapes.npz).  The case table, what each case is for and which STFT form it is meant to
reach are in tests/test_mel_shapes_oracle_cpu.py, which also shows that the bounds used here discriminate (a periodic window, a
filterbank one bin off and a signal one sample off are each at least ten bounds away at every shape).

  a. offline: audio.preprocess_audio per case on every form that can take it (default, mel_fft = 0, mel_fft = mel_mfma = 0; a setting
     that would land on a form already run is skipped), the form that ran asserted through ops.mel_last_form(); NaN pattern equal,
     atol 2e-6 at the shipped options and atol = rtol = 3e-6 at the option cases (the bounds of tests/test_gpu_parity.py for this
     front-end; one float32 ulp of the largest value, an energy below 16, is 9.5e-7); the forms within 1e-6 of each other
  b. streaming: zeggs_mel_features_range over four growing prefixes == the offline table (1e-6), every prefix makes progress
  c. zeggs_mel_features_batch == zeggs_mel_features_window bit for bit, on the batched FFT kernel with a radix-2 stage and on the
     per-row fall-back of the other two forms
  d. n_fft = 2400 runs on the direct form past 64 KB of LDS (case `lds` of a.), n_fft = 8192 is refused ahead of any launch

Measured on an MI355X, worst |device - reference| per case and form (- = the form does not take the case; the same figure on every
form of a case: the float64 spectra differ in their last bits only, and a float32 feature then rounds the same way or one ulp off):

  case        fft       mfma      direct   | case        fft       mfma      direct
  r2          7.5e-9    -         7.5e-9   | lds         -         -         7.5e-9
  r2b         3.7e-9    3.7e-9    3.7e-9   | short       0         0         0
  big         7.5e-9    -         7.5e-9   | hop         7.5e-9    -         7.5e-9
  f3          -         3.7e-9    3.7e-9   | gap         3.7e-9    3.7e-9    3.7e-9
  f3d         -         -         3.7e-9   | tiny        0         -         0
  wide        -         -         3.7e-9   | many        -         3.7e-9    3.7e-9
  widem       -         9.5e-7    9.5e-7   | slow        7.5e-9    7.5e-9    7.5e-9
  r5          3.7e-9    -         3.7e-9   | r2_pre      7.5e-9    -         7.5e-9
  empty       3.7e-9    3.7e-9    3.7e-9   | f3_uncraw   -         0         0
  r4          3.7e-9    3.7e-9    3.7e-9   | r2b_cubic   3.7e-9    3.7e-9    3.7e-9
  odd         -         -         3.7e-9   | r2_nearest  7.5e-9    -         7.5e-9

3.7e-9 and 7.5e-9 are one float32 ulp of a log-mel value in [1/32, 1/8); widem's 9.5e-7 is one ulp of an energy in [8, 16), on both
forms alike.  `lds` ran on the direct form with 67 848 bytes of LDS, and every case reached the form of the table.  The streaming
ranges and the batched rows (b., c.) passed as stated; the 33 tests take 3 s.
"""
import numpy as np
import pytest
import torch

import test_mel_shapes_oracle_cpu as shapes
from zeggs import audio, capi, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SETTINGS = ((1, 1), (0, 1), (0, 0))      # (mel_fft, mel_mfma): the default first
FEATURES = ["mel_spec", "energy"]


@pytest.fixture
def restore_options():
    yield
    for k, v in (("mel_fft", 1), ("mel_mfma", 1)):
        ops.set_option(k, v)


def _dims(tag, **over):
    n_fft, hop, n_mels, fps = shapes.CASES[tag][:4]
    c = shapes.audio_conf(tag, **over)
    fb, min_clip = audio.mel_tables(n_fft, shapes.FS, n_mels, shapes.FMIN, shapes.FMAX, shapes.MIN_CLIP, True, True, DEV)
    d = audio.MelDims(n_fft, hop, n_mels, shapes.FS, float(fps), float(min_clip), c["pre_emph_coeff"] if c["pre_emphasis"] else 0.0,
                      audio.mel_flags(c["centered"], c["normalize_range"], c["resample_method"]))
    return d, fb


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- a. offline, every form
ALL = [(tag, "", {}, c[5]) for tag, c in shapes.CASES.items()] + list(shapes.OPTIONS)


@pytest.mark.parametrize("tag,name,over,forms", ALL, ids=[t + ("_" + n if n else "") for t, n, _, _ in ALL])
def test_offline_equals_the_reference_on_every_form(tag, name, over, forms, restore_options, golden_dir):
    n_fft, hop, n_mels, fps, n, _ = shapes.CASES[tag]
    g, wav, nfr = shapes.fixture(golden_dir), shapes.signal(tag, golden_dir), shapes.n_frames(tag)
    ref = g[f"{tag}_feat_{name}" if name else f"{tag}_feat"]
    conf = shapes.audio_conf(tag, **over)
    ran = {}
    for (fft, mfma), want in zip(SETTINGS, forms):
        if want in ran:
            continue
        ops.set_option("mel_fft", fft)
        ops.set_option("mel_mfma", mfma)
        got = audio.preprocess_audio(wav, fps, nfr, conf, FEATURES)
        assert ops.mel_last_form() == want, (tag, name, fft, mfma, ops.MEL_FORMS[ops.mel_last_form()])
        assert got.dtype == np.float32 and got.shape == ref.shape
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        err = float(np.nanmax(np.abs(got.astype(np.float64) - ref)))
        print(f"{tag}{'_' + name if name else ''} {ops.MEL_FORMS[want]}: max |device - reference| = {err:.3e}")
        if name:
            np.testing.assert_allclose(got, ref, atol=3e-6, rtol=3e-6, equal_nan=True, err_msg=f"{tag}_{name} {ops.MEL_FORMS[want]}")
        else:
            np.testing.assert_allclose(got, ref, atol=2e-6, rtol=0, equal_nan=True, err_msg=f"{tag} {ops.MEL_FORMS[want]}")
        ran[want] = got
    assert list(ran) == list(dict.fromkeys(forms))
    first, *others = ran.items()
    for form, got in others:
        np.testing.assert_allclose(got, first[1], atol=1e-6, rtol=0, equal_nan=True,
                                   err_msg=f"{tag} {ops.MEL_FORMS[form]} vs {ops.MEL_FORMS[first[0]]}")
    assert audio.stft_frame_count(n, n_fft, hop) == int(g[f"{tag}_M"])
    d, _ = _dims(tag, **over)
    assert capi.api().zeggs_mel_stft_frames(d, n) == int(g[f"{tag}_M_{name}" if name else f"{tag}_M"])


# ----------------------------------------------------------------------------- b. streaming == offline
@pytest.mark.parametrize("tag", ["r2", "r2b", "empty", "slow", "gap", "f3", "odd"])
def test_streaming_ranges_equal_offline(tag, golden_dir):
    """zeggs_mel_features_range over four growing prefixes (k1 from zeggs_mel_frames_ready, the last call final) against the offline
    table: a radix-2 plan, r = 2 exactly (every animation frame on an STFT frame), r < 1, hop > n_fft, and the two forms without a plan"""
    n_fft, hop, n_mels, fps, n, forms = shapes.CASES[tag]
    wav, nfr = shapes.signal(tag, golden_dir), shapes.n_frames(tag)
    full = audio.mel_features(wav, nfr, n_fft=n_fft, hop=hop, n_mels=n_mels, fs=shapes.FS, fps=float(fps), fmin=shapes.FMIN,
                              fmax=shapes.FMAX, min_clip=shapes.MIN_CLIP)
    d, fb = _dims(tag)
    w = torch.as_tensor(wav, device=DEV)
    rows, k0 = [], 0
    for got in (n * 3 // 10 + 1, n * 11 // 20, n * 4 // 5 + 3, n):
        final = got == n
        assert got >= hop + n_fft // 2                                     # STFT frames 0 and 1 are complete
        k1 = nfr if final else ops.mel_frames_ready(d, got)
        assert k0 < k1 <= nfr, (tag, got, k0, k1)                          # every prefix makes progress
        out = torch.empty(k1 - k0, n_mels + 1, device=DEV)
        ops.mel_features_range(d, w[:got].contiguous(), final, fb, k0, k1, out, ops.mel_range_workspace(d, k1 - k0, DEV, k0))
        assert ops.mel_last_form() == forms[0]
        rows.append(out)
        k0 = k1
    assert k0 == nfr
    st, fu = torch.cat(rows).cpu().numpy(), full.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(st), np.isnan(fu))
    np.testing.assert_allclose(st, fu, atol=1e-6, rtol=1e-6, equal_nan=True)


# ----------------------------------------------------------------------------- c. the batched call == the window call
@pytest.mark.parametrize("tag,batch_form", [("r2", shapes.FFT_BATCH), ("f3", shapes.MFMA), ("odd", shapes.DIRECT)])
def test_batch_equals_window_bit_for_bit(tag, batch_form, golden_dir):
    """three rows in one zeggs_mel_features_batch -- k0 = 0 while the signal continues, a window that starts exactly at
    zeggs_mel_window_first_sample(3), a final row up to the last animation frame -- each bit-identical to zeggs_mel_features_window
    with the same arguments, the guard row behind each output untouched"""
    n_mels, n = shapes.CASES[tag][2], shapes.CASES[tag][4]
    wav, nfr = torch.as_tensor(shapes.signal(tag, golden_dir), device=DEV), shapes.n_frames(tag)
    d, fb = _dims(tag)
    n_a = n * 3 // 5
    args = [(0, n_a, 0, 0, ops.mel_frames_ready(d, n_a)),                       # (base, samples, final, k0, k1)
            (ops.mel_window_first_sample(d, 3), n, 0, 3, ops.mel_frames_ready(d, n)),
            (ops.mel_window_first_sample(d, nfr // 2), n, 1, nfr // 2, nfr)]
    assert args[1][0] > 0 and args[2][0] > args[1][0] and all(a[4] > a[3] for a in args)
    recs, wins, outs, refs = (capi.MelRow * 3)(), [], [], []
    for q, (base, ns, final, k0, k1) in zip(recs, args):
        wins.append(wav[base:ns].clone())
        outs.append(torch.full((k1 - k0 + 1, n_mels + 1), 7.0, device=DEV))
        q.wav, q.out, q.base, q.n_samples, q.k0, q.k1, q.final = wins[-1].data_ptr(), outs[-1].data_ptr(), base, ns, k0, k1, final
        ref = torch.empty(k1 - k0, n_mels + 1, device=DEV)
        ops.mel_features_window(d, wins[-1], base, ns, final, fb, k0, k1, ref, ops.mel_range_workspace(d, k1 - k0, DEV, k0))
        refs.append(ref)
    assert ops.mel_last_form() == shapes.CASES[tag][5][0]
    mb = ops.MelBatch(d, fb, 3, max(a[4] - a[3] for a in args), DEV)
    ops.mel_features_batch(mb, recs, 3)
    torch.cuda.synchronize()
    assert ops.mel_last_form() == batch_form
    for i, (ref, out) in enumerate(zip(refs, outs)):
        assert float(out[-1].min()) == float(out[-1].max()) == 7.0, (tag, i, "guard row")
        assert torch.equal(_bits(out[:-1]), _bits(ref)), (tag, i)
    assert torch.isfinite(refs[0]).all() and torch.isfinite(refs[1]).all()


# ----------------------------------------------------------------------------- d. the window the LDS ends
def test_window_beyond_the_lds_is_refused_before_any_launch(golden_dir):
    """the direct form keeps its frame and tables in LDS: 160 KB end it at n_fft = 5828 (80 mel channels).  n_fft = 8192 has no other
    form (the FFT form would need 512 KB) and is refused by name, ahead of the launch: the form of the last call stays what it was"""
    wav = shapes.signal("lds", golden_dir)
    audio.mel_features(wav[:400], 2, n_fft=10, hop=5, n_mels=4)
    assert ops.mel_last_form() == shapes.FFT
    with pytest.raises(RuntimeError, match=r"n_fft = 8192 .*230024 bytes of LDS"):
        audio.mel_features(wav, 4, n_fft=8192, hop=2048)
    assert ops.mel_last_form() == shapes.FFT
    torch.cuda.synchronize()
