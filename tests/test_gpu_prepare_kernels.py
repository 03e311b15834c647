"""The dataset-preparation kernels one by one (csrc/prepare.hip, csrc/loudness.hip) on a real MI355X against the float64 restatements
of tests/prepare_oracle.py, at the smallest shapes that still take every path.  Run with -s for each case's worst error as a share
of its bound.  Every bound is an existing one of the project (named in prepare_oracle.py beside its value).

Which case reaches which path:
  audio_prepare   one launch of audio_prepare_k, 256 threads, the interval table in dynamic LDS (16 bytes an interval): k0 0 bytes,
                  the small cases 16 .. 48 bytes, k4096 65536 bytes (the default ceiling); k4097 is refused on the host.
                  start-eq-end / start-eq-n / start-past-n: no launch.  grid-stride: n_out = 3000010 > 8192 * 256, the only case whose
                  threads go round the grid-stride loop twice.
  center_take     center_offset_k (one thread) + center_apply_k, one thread a frame in blocks of 256: N = 1 and 256 one block,
                  257 and 600 two and three.  Orders zyx / xzy, round_f32 0 / 1.
  rot_stretch     the spline runs over 4 J columns: J = 1, 2 the thread-per-chunk kernel (4 J <= 8), J = 3 the first width of the
                  thread-per-column kernel (12 columns), J = 16 one full 64-column tile, J = 17 a second tile with 4 columns, J = 75
                  five tiles (the last with 44).  N = 4, 5, 6: only end conditions and up to two interior rows; C+3, C+4 one
                  elimination chunk (one row short, full), C+5 two, 2C+H+5 three.  M = 1 (step 0), 2, N (knots only), 2N-1, 0.9 N, 1.1 N.
  masked_stats    tcol = 1 (D = 1), 2 (D = 2), 8 (D = 5), 64 (D = 33 .. 130; D = 65 and 130 start a second and a third column tile);
                  slabs of 2048 rows: R = 1, 2047, 2048 one slab, 2049 and 4096 two, 6150 four; mid-slab-out, first-slab-out and
                  R2049-D1-one have a slab that counts nothing.
  loudness        rate-*: 2 s at 8 / 22.05 / 44.1 / 48 kHz, chunk 4096 (4 .. 24 chunks, 17 blocks); n-*: 8 kHz, 1 chunk (3200,
                  4095, 4096), 2 (4097, 8192), 3 (8193), 1 .. 7 blocks; chunk-*: 16000 samples in 250, 160, 16, 4 and 1 chunks;
                  blocks-1023 / 1024 / 1025 / 1100: gate_k's 1024 threads read one block each, and the first 1 / 76 of them a second.

Measured on the MI355X, worst error as a share of the bound per group (107 tests, 4 s):
  audio_prepare   16 cases + the refusal: no element differs in any output.  Found by start-eq-end / start-eq-n / start-past-n: the
                  entry point checked its output pointers before the length, and an empty tensor has no address, so an empty cut
                  raised "audio_prepare: no output"; the length is looked at first now.
  center_take     30 cases x round_f32 0 / 1: positions 2.8e-14, degrees 2.8e-14 = 2.8e-5 of the bound; with round_f32 every changed
                  value is the oracle's rounded value itself (0 ulp).
  rot_stretch     20 cases x 2 orders: 8.5e-14 degrees = 8.5e-5 of the bound (J75-N2C+H+5-M1.1N zyx).
  masked_stats    16 cases: 6.7e-7 of the bound (R6150-D65-all); constant channels exactly 0, two calls the same bits.
  loudness        19 cases x float64 / float32 input: 7.1e-15 LU = 7.1e-10 of the bound (float64), 3.8e-7 LU = 1.9e-2 of the bound
                  (float32, n-4096), samples 4.0e-2 of theirs; the sine reads -3.0517 LKFS (0.83 of the 0.05 LU the oracle is held
                  to), a tenth of it 20 LU less to 2.8e-10 LU.
"""
import warnings

import numpy as np
import pytest
import torch

import prepare_oracle as po
from oracle import loudness as olo
from zeggs import audio
from zeggs import data_pipeline as dp
from zeggs.capi import api

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def ids(table):
    return [c["id"] for c in table]


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ----------------------------------------------------------------------------- audio_prepare: bit-exact
@pytest.mark.parametrize("case", po.AUDIO_CASES, ids=ids(po.AUDIO_CASES))
def test_audio_prepare_vs_mask_and_slice(case):
    w = po.audio_wav(case)
    ref = po.silence_cut(w, case["intervals"], case["start"], case["end"])
    wd = g(w)
    o32, o64 = dp.audio_prepare(wd, case["intervals"], case["start"], case["end"], want_f64=True)
    only32, none = dp.audio_prepare(wd, case["intervals"], case["start"], case["end"], want_f64=False)
    torch.cuda.synchronize()
    got32, got64, got_only = o32.cpu().numpy(), o64.cpu().numpy(), only32.cpu().numpy()
    assert none is None and got32.dtype == np.float32 and got64.dtype == np.float64
    assert got32.shape == ref.shape == got64.shape == got_only.shape
    wrong = int((got32 != ref).sum())
    print(f"audio {case['id']}: K = {len(case['intervals'])}, {len(ref)} samples out, {int((ref != 0).sum())} kept, {wrong} differ (bound: none)")
    assert np.array_equal(got32, ref)                                          # by value: zeros of either sign compare equal
    assert np.array_equal(bits(got64), bits(got32.astype(np.float64)))         # the float64 twin: the same samples widened
    assert np.array_equal(bits(got_only), bits(got32))


def test_audio_prepare_refuses_4097_intervals_on_the_host():
    w = g(po.audio_wav(po.AUDIO_CASES[0]))
    iv = np.array([[100 + 2 * i, 101 + 2 * i] for i in range(po.AUDIO_MAX_INTERVALS + 1)], dtype=np.int64)
    with pytest.raises(RuntimeError, match=r"audio_prepare: 0 \.\. 4096 intervals, got 4097"):
        dp.audio_prepare(w, iv, 50, 9000, want_f64=True)
    # the C entry itself: nothing is launched, the output keeps what it held
    out = torch.full((8950,), 7.0, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="got 4097"):
        api().zeggs_audio_prepare(w, w.numel(), g(iv), len(iv), 50, 9000, out, None, None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ----------------------------------------------------------------------------- center_take
@pytest.mark.parametrize("case", po.CENTER_CASES, ids=ids(po.CENTER_CASES))
def test_center_take_vs_quaternion_helpers(case):
    pos, rot = po.center_inputs(case)
    order = case["order"]
    for round_f32 in (0, 1):
        ref_p, ref_r = po.center(pos, rot, order, round_f32)
        pd, rd = g(pos), g(rot)
        dp.center_take(pd, rd, order, round_f32)
        got_p, got_r = pd.cpu().numpy(), rd.cpu().numpy()
        # joints 1 .. J-1: the bits that went in
        assert np.array_equal(bits(got_p[:, 1:]), bits(pos[:, 1:])) and np.array_equal(bits(got_r[:, 1:]), bits(rot[:, 1:]))
        dp_, dr_ = np.abs(got_p[:, 0] - ref_p[:, 0]), po.angle_diff(got_r[:, 0], ref_r[:, 0])
        if round_f32 == 0:
            share = max(dp_.max() / po.POS_TOL, dr_.max() / po.DEG_TOL)
            print(f"center {case['id']}: positions {dp_.max():.3e} ({po.POS_TOL:.0e}), degrees {dr_.max():.3e} ({po.DEG_TOL:.0e}): "
                  f"{share:.3e} of the bound")
            assert dp_.max() <= po.POS_TOL and dr_.max() <= po.DEG_TOL
        else:
            for got in (got_p[:, 0], got_r[:, 0]):
                assert np.array_equal(got, got.astype(np.float32).astype(np.float64))      # rounded to float32, held in float64
            share = max(np.max(dp_ / po.ulp32(ref_p[:, 0])), np.max(dr_ / po.ulp32(ref_r[:, 0])))
            print(f"center {case['id']} round_f32: {share:.3e} float32 ulp of the oracle's rounded value at the most")
            assert np.all(dp_ <= po.ulp32(ref_p[:, 0])) and np.all(dr_ <= po.ulp32(ref_r[:, 0]))


@pytest.mark.parametrize("order", ["xyz", "yzx", "zxy"])
def test_center_take_other_orders_raise_before_the_data_is_touched(order):
    pos, rot = po.center_inputs(po.CENTER_CASES[2])
    pd, rd = g(pos), g(rot)
    with pytest.raises(NotImplementedError, match="Cannot convert to ordering"):
        dp.center_take(pd, rd, order, 0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(pd.cpu().numpy()), bits(pos)) and np.array_equal(bits(rd.cpu().numpy()), bits(rot))


# ----------------------------------------------------------------------------- rot_stretch
@pytest.mark.parametrize("case", po.ROT_CASES, ids=ids(po.ROT_CASES))
def test_rot_stretch_vs_quaternion_chain(case):
    c, h, nw = dp.spline_chunk()
    n, m = po.rot_sizes(case, c, h)
    j = case["j"]
    e = po.rot_inputs(case, n)
    ed = g(e)
    for order in ("zyx", "xzy"):
        ref, q = po.rot_stretch(e, m, order, with_quats=True)
        assert np.any(q[:, 0, 0] < -0.5) and np.any(q[:, j - 1, 0] < 0.0)      # the turning and the crossing joint went through w < 0
        got = dp.rot_stretch(ed, m, order).cpu().numpy()
        assert got.shape == (m, j, 3) and got.dtype == np.float64
        d = po.angle_diff(got, ref).max()
        print(f"rot_stretch {case['id']} {order}: N = {n}, M = {m}, {'narrow' if 4 * j <= nw else 'wide'} spline: {d:.3e} degrees, "
              f"{d / po.DEG_TOL:.3e} of the bound")
        assert d <= po.DEG_TOL


# ----------------------------------------------------------------------------- masked_stats
@pytest.mark.parametrize("case", po.STATS_CASES, ids=ids(po.STATS_CASES))
def test_masked_stats_vs_numpy(case):
    x, mask = po.stats_inputs(case)
    xd, md = g(x), g(mask)
    got = [t.cpu().numpy() for t in dp.masked_stats(xd, md)]
    ref = po.masked_stats(x, mask)
    worst = 0.0
    for name, a, r in zip(("mean", "std", "pooled"), got, ref):
        err, bound = np.abs(a - r), po.stats_bound(r)
        worst = max(worst, float(np.max(err / bound)))
        assert a.dtype == np.float64 and a.shape == r.shape and np.all(err <= bound), name
    print(f"stats {case['id']}: tcol = {po.stats_tcol(case['d'])}, {-(-case['r'] // po.STATS_SLAB)} slab(s), {int(mask.sum())} rows: "
          f"{worst:.3e} of the bound")
    if case["d"] > 1:
        assert got[1][1] == 0.0                       # the constant channel
    again = [t.cpu().numpy() for t in dp.masked_stats(xd, md)]
    for a, b in zip(got, again):
        assert np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- loudness
def check_loudness(name, x, rate, chunk):
    """float64 and float32 input (the same samples) against oracle.loudness -> worst share of a bound"""
    worst = 0.0
    for dt, tol in ((np.float64, po.LUFS_TOL64), (np.float32, po.LUFS_TOL32)):
        xin = x.astype(np.float32).astype(dt)
        ref_l = olo.Meter(rate).integrated_loudness(xin)
        y, lufs = audio.normalize_loudness_device(xin, rate, -20.0, chunk=chunk)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")               # (normalize.loudness warns when its output clips)
            ref_y = olo.normalize_loudness(xin, ref_l, -20.0).astype(np.float32)
        got_y = y.cpu().numpy()
        d_s = np.max(np.abs(got_y.astype(np.float64) - ref_y) / (po.SAMPLE_ATOL + po.SAMPLE_RTOL * np.abs(ref_y.astype(np.float64))))
        print(f"loudness {name} {np.dtype(dt).name}: {lufs:.6f} LUFS, off by {abs(lufs - ref_l):.3e} LU ({abs(lufs - ref_l) / tol:.3e} of the "
              f"bound), samples {d_s:.3e} of theirs")
        worst = max(worst, abs(lufs - ref_l) / tol, float(d_s))
        assert abs(lufs - ref_l) <= tol, (name, dt, lufs, ref_l)
        assert got_y.dtype == np.float32 and got_y.shape == ref_y.shape
        np.testing.assert_allclose(got_y, ref_y, rtol=po.SAMPLE_RTOL, atol=po.SAMPLE_ATOL, err_msg=name)
    return worst


@pytest.mark.parametrize("case", po.LOUD_CASES, ids=ids(po.LOUD_CASES))
def test_loudness_vs_meter_restatement(case):
    x = po.loud_signal(case)
    lo, _ = audio.gating_blocks(len(x), case["rate"])
    print(f"loudness {case['id']}: {-(-len(x) // case['chunk'])} chunk(s), {len(lo)} block(s)")
    check_loudness(case["id"], x, case["rate"], case["chunk"])


def test_loudness_refuses_a_chunk_under_64():
    case = po.LOUD_CHUNK_CASES[0]
    with pytest.raises(RuntimeError, match="loudness: bad sizes"):
        audio.normalize_loudness_device(po.loud_signal(case), case["rate"], -20.0, chunk=63)


def test_loudness_of_the_997_hz_sine():
    """BS.1770's known answer on the device: full scale at 48 kHz reads -3.01 LKFS, a tenth of it 20 LU less"""
    _, full = audio.normalize_loudness_device(po.sine(amplitude=1.0), 48000, -20.0)
    _, tenth = audio.normalize_loudness_device(po.sine(amplitude=0.1), 48000, -20.0)
    print(f"loudness sine: {full:.6f} LUFS ({abs(full + 3.01) / po.SINE_TOL:.3e} of the bound), a tenth of it {tenth:.6f} "
          f"({abs(tenth - (full - 20.0)) / po.LUFS_TOL64:.3e} of the bound)")
    assert abs(full + 3.01) <= po.SINE_TOL and abs(tenth - (full - 20.0)) <= po.LUFS_TOL64
