"""Dataset preparation on the device (csrc/prepare.hip, zeggs/data_pipeline.py) on a real MI355X:
  1. the spline kernel against a dense float64 solve of the not-a-knot system written here;
  2. the masked statistics kernel against numpy float64, and bitwise reproducibility;
  3. data_pipeline(conf) end to end against what the unmodified reference made of the same tiny corpus
     (tests/golden/prepare.npz, recorded by tools/make_golden_prepare.py), three confs;
  4. train() for two iterations on the files data_pipeline wrote.
"""
import json

import numpy as np
import pytest
import torch

from zeggs import data_pipeline as dp
from zeggs import synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------- 1. spline
def eval_spline(y, S, m):
    n = len(y)
    t = np.linspace(0, n - 1, m)
    lo = np.minimum(np.floor(t).astype(np.int64), n - 2)
    u = (t - lo)[:, None]
    v = 1.0 - u
    return y[lo] * v + y[lo + 1] * u + ((v ** 3 - v) * S[lo] + (u ** 3 - u) * S[lo + 1]) / 6.0


def dense_spline(y, m):
    """Not-a-knot cubic spline over the grid 0 .. n-1 in terms of its second derivatives S (unit spacing):
    S[i-1] + 4 S[i] + S[i+1] = 6 (y[i-1] - 2 y[i] + y[i+1]) inside, third derivative continuous across knots 1 and n-2
    (S[0] - 2 S[1] + S[2] = 0, S[n-3] - 2 S[n-2] + S[n-1] = 0); one dense solve, evaluated at linspace(0, n-1, m)."""
    n = len(y)
    A = np.zeros((n, n))
    rhs = np.zeros_like(y)
    A[0, :3] = [1.0, -2.0, 1.0]
    A[n - 1, n - 3:] = [1.0, -2.0, 1.0]
    for i in range(1, n - 1):
        A[i, i - 1:i + 2] = [1.0, 4.0, 1.0]
        rhs[i] = 6.0 * (y[i - 1] - 2.0 * y[i] + y[i + 1])
    return eval_spline(y, np.linalg.solve(A, rhs), m)


def windowed_spline(y, m, half=60):
    """The same spline for long tables without scipy: every output sample from a dense solve over the 2 * half rows around it (what a
    row feels of one k rows away decays like 0.268^k: 1e-34 at 60; the window's own end conditions are that far from the sample)."""
    n = len(y)
    t = np.linspace(0, n - 1, m)
    out = np.empty((m,) + y.shape[1:])
    span, key, S = 64, None, None
    for k, tk in enumerate(t):
        lo = min(int(np.floor(tk)), n - 2)
        a = max(min((lo // span) * span - half, n - (2 * half + span)), 0)      # the samples of `span` rows share a window
        b = min(a + 2 * half + span, n)
        if (a, b) != key:
            w = y[a:b]
            A = np.zeros((b - a, b - a))
            rhs = np.zeros_like(w)
            A[0, :3] = [1.0, -2.0, 1.0]
            A[-1, -3:] = [1.0, -2.0, 1.0]
            for i in range(1, b - a - 1):
                A[i, i - 1:i + 2] = [1.0, 4.0, 1.0]
                rhs[i] = 6.0 * (w[i - 1] - 2.0 * w[i] + w[i + 1])
            key, S = (a, b), np.linalg.solve(A, rhs)
        u = tk - lo
        v = 1.0 - u
        i = lo - a
        out[k] = y[lo] * v + y[lo + 1] * u + ((v ** 3 - v) * S[i] + (u ** 3 - u) * S[i + 1]) / 6.0
    return out


def long_reference(y, m):
    try:
        from scipy.interpolate import interp1d
    except ImportError:
        return windowed_spline(y, m)
    n = len(y)
    return interp1d(np.arange(n, dtype=np.float64), y, kind="cubic", axis=0)(np.linspace(0, n - 1, m))


def table(n, w, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.standard_normal((n, w)), axis=0) * 0.3 + rng.standard_normal((n, w)) + 3.0 * rng.standard_normal((1, w))


def check_spline(n, w, reference):
    y = table(n, w, seed=1000 * w + n)
    for ratio in (0.9, 1.1):
        m = int(ratio * n)
        got = dp.spline_resample(g(y), m).cpu().numpy()
        ref = reference(y, m)
        err, bound = float(np.abs(got - ref).max()), 1e-12 * float(np.abs(y).max())
        print(f"spline N={n} W={w} M={m}: max |device - reference| = {err:.3e} (bound {bound:.3e})")
        assert got.shape == (m, w) and err <= bound


C_, H_, NW_ = None, None, None


def chunking():
    global C_, H_, NW_
    if C_ is None:
        C_, H_, NW_ = dp.spline_chunk()
    return C_, H_, NW_


@pytest.mark.parametrize("w", [1, 3, 81, 300])      # 81: the audio feature table (two column tiles, the second partly filled)
@pytest.mark.parametrize("size", ["4", "5", "6", "C-1", "C", "C+1", "2C+H+3"])
def test_spline_vs_dense_solve(size, w):
    c, h, _ = chunking()
    n = {"4": 4, "5": 5, "6": 6, "C-1": c - 1, "C": c, "C+1": c + 1, "2C+H+3": 2 * c + h + 3}[size]
    assert n <= 400
    check_spline(n, w, dense_spline)


@pytest.mark.parametrize("case", ["narrow-width", "first-wide-width", "group-1", "group", "group+1", "group-w3", "group-w3+1", "chunks-w7"])
def test_spline_at_the_kernels_path_boundaries(case):
    """Sizes at which the code takes another path: the widest table of the thread-per-chunk kernel and the first of the thread-per-column
    kernel; the row count at which a thread-per-chunk workgroup (64 / W - 1 chunks) is exactly full, one short and one over, for W = 1 and
    W = 3; a width that does not divide the 64 lanes.  Reference: scipy's interp1d(kind="cubic") (the windowed dense solve without scipy)."""
    c, h, nw = chunking()
    full = lambda w: 4 + (64 // w - 1) * c  # noqa: E731   rows 2 .. N-3 in chunks of c: the workgroup's chunks exactly used
    n, w = {"narrow-width": (3 * c + 7, nw), "first-wide-width": (3 * c + 7, nw + 1), "group-1": (full(1) - 1, 1), "group": (full(1), 1),
            "group+1": (full(1) + 1, 1), "group-w3": (full(3), 3), "group-w3+1": (full(3) + 1, 3), "chunks-w7": (9 * c + 11, 7)}[case]
    check_spline(n, w, long_reference)


def test_spline_long_audio_table_and_short_table_error():
    check_spline(100000, 1, long_reference)
    with pytest.raises(ValueError):
        dp.spline_resample(g(table(3, 1, 0)), 5)
    from zeggs import ops
    L = ops.lib()                                    # the C entry refuses it too
    y, out, ws = g(table(3, 2, 0)), torch.empty(5, 2, dtype=torch.float64, device=DEV), torch.empty(4096, dtype=torch.uint8, device=DEV)
    import ctypes
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.zeggs_spline_resample(ptr(y), ctypes.c_long(3), 2, ctypes.c_long(5), ptr(out), ptr(ws), ctypes.c_size_t(4096), None) != 0
    assert b"4 rows" in L.zeggs_last_error()


def test_rot_stretch_vs_numpy_chain():
    """from_euler, unroll, spline on the four components, normalise, to_euler against the same chain in numpy float64 (the oracle's
    quaternion helpers and the dense spline above); orders without a to_euler raise as bvh_channels does."""
    from oracle import anim as oanim
    rng = np.random.default_rng(5)
    n, j = 150, 5
    e = np.clip(synth._smooth(rng, n, j * 3, 25.0), -70, 70).reshape(n, j, 3)
    e[:, 0, 0] += np.linspace(0, 400, n)            # a joint that turns more than once: the unrolling flips signs
    for order in ("zyx", "xzy"):
        q = oanim.q_unroll(oanim.q_from_euler(np.radians(e), order))
        assert np.any(q[:, 0, 0] < -0.5)             # (the unrolled quaternion of the turning joint did go through w < 0)
        for m in (135, 165):
            qs = dense_spline(q.reshape(n, -1), m).reshape(m, j, 4)
            qs = qs / np.linalg.norm(qs, axis=-1, keepdims=True)
            ref = np.degrees(oanim.q_to_euler(qs, order))
            got = dp.rot_stretch(g(e), m, order).cpu().numpy()
            d = np.abs((got - ref + 180.0) % 360.0 - 180.0).max()
            print(f"rot_stretch {order} M={m}: max angle difference {d:.3e} degrees")
            assert d < 1e-9
    with pytest.raises(NotImplementedError, match="Cannot convert to ordering"):
        dp.rot_stretch(g(e), 100, "xyz")


# ----------------------------------------------------------------------------- 2. statistics
def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("d", [1, 3, 81, 450])
def test_masked_stats_vs_numpy_float64(d):
    rng = np.random.default_rng(d)
    r = 5003                                          # no multiple of the slab (2048 rows) or of the workgroup
    x = (rng.standard_normal((r, d)) * rng.uniform(0.1, 30.0, (1, d)) + rng.uniform(-50.0, 50.0, (1, d))).astype(np.float32)
    if d > 2:
        x[:, 1] = np.float32(0.7251)                  # a constant channel: its std is exactly zero, as in the real statistics
    mask = np.zeros(r, dtype=bool)
    for s, e in ((0, 1200), (1200, 1204), (1204, 1207), (1207, 4100), (4400, r)):      # (1200, 1204) and (1204, 1207) are empty
        mask[s + 2:e - 2] = True
    assert mask[1198:1209].sum() == 0 and mask.sum() % 256 != 0
    xd, md = g(x), g(mask)
    mean, std, pooled = (t.cpu().numpy() for t in dp.masked_stats(xd, md))
    x64 = x[mask].astype(np.float64)
    std64 = x64.std(axis=0)
    if d > 2:
        std64[1] = 0.0                                # (numpy's mean of equal numbers can be one float64 ulp off; the true value is 0)
    for name, got, ref in (("mean", mean, x64.mean(axis=0)), ("std", std, std64), ("pooled", pooled, np.atleast_1d(x64.std()))):
        err = np.abs(got - ref)
        bound = ulp32(ref) + 1e-12 * np.abs(ref)
        print(f"stats D={d} {name}: max error {err.max():.3e}, in units of the bound {np.max(err / bound):.3e}")
        assert got.dtype == np.float64 and np.all(err <= bound), name
    if d > 2:
        assert std[1] == 0.0
    again = dp.masked_stats(xd, md)
    for a, b in zip((mean, std, pooled), again):
        assert np.array_equal(a.view(np.uint64), b.cpu().numpy().view(np.uint64))


# ----------------------------------------------------------------------------- 3. end to end on the fixture
PER_JOINT = ("Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt")
FEATURES = ("X_audio_features", "Y_root_pos", "Y_root_rot", "Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt", "Y_gaze_pos")
IN_STATS = ("Y_root_vel", "Y_root_vrt", "Y_lpos", "Y_ltxy", "Y_lvel", "Y_lvrt", "Y_gaze_dir")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(golden_dir / "prepare.npz")


def golden(z, i, key):
    """array `key` of conf i: stored as it is, or put together from the pool of distinct blocks (tools/make_golden_prepare.py)"""
    if f"c{i}/{key}" in z.files:
        return z[f"c{i}/{key}"]
    ids = z[f"c{i}/{key}@pool"]
    if ids.ndim == 0:
        return z[f"pool/{int(ids)}"]
    if ids.ndim == 2:
        return np.concatenate([np.concatenate([z[f"pool/{a}"], z[f"pool/{b}"]], axis=1) for a, b in ids], axis=0)
    return np.concatenate([z[f"pool/{a}"] for a in ids], axis=0)


def write_corpus(z, base):
    for k in z.files:
        if k.startswith("file/"):
            p = base / k[5:]
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_bytes(z[k].tobytes())


def reference_stats(data, gaze_dir=None):
    """the reference's statistics (data_pipeline.py:562-648) evaluated in float64 on float32 arrays -> dict of float64 vectors.
    Y_gaze_dir is not among the returned arrays: its three input-statistics entries are taken from `gaze_dir` (or left out)."""
    mask = np.zeros(len(data["X_audio_features"]), dtype=bool)
    for s, e in data["ranges_train"]:
        mask[s + 2:e - 2] = True
    sel = lambda k: np.asarray(data[k])[mask].astype(np.float64)  # noqa: E731
    keys = [k for k in IN_STATS if k != "Y_gaze_dir"]
    mean = {k: sel(k).mean(axis=0).ravel() for k in keys}
    out = dict(audio_input_mean=sel("X_audio_features").mean(axis=0), audio_input_std=np.atleast_1d(sel("X_audio_features").std() + 1e-10),
               anim_output_mean=np.hstack([mean[k] for k in keys]), anim_output_std=np.hstack([sel(k).std(axis=0).ravel() for k in keys]),
               anim_input_mean=np.hstack([mean[k] for k in keys]),
               anim_input_std=np.hstack([np.repeat(sel(k).std() + 1e-10, len(mean[k])) for k in keys]))
    return out


@pytest.mark.parametrize("i", [0, 1, 2])
def test_data_pipeline_vs_reference(fixture, tmp_path, i):
    """Every array of processed_data, the trimmed WAV samples and the trimmed BVH channels of conf i (c0: len_ratios [0.9, 1.0] with
    save_trimmed_animation, c1: the same without, c2: [1.0, 1.1] with) against the reference's.

    Bounds: integer arrays and label names (mapped by name) equal; features at the tolerances tests/test_gpu_parity.py applies to the
    same kernels against the reference (animation atol 2e-4 / rtol 1e-4, velocities atol 1e-3, audio 3e-6 / 3e-6); BVH degrees 2e-2,
    positions 2e-3; WAV samples: the device's float64 spline and scipy's agree to 1e-12, so a sample times 2^15 truncated to int16 can
    differ only where the value sits within that distance of an integer: one step at the most, and on well under 1 in 1000 samples.
    Statistics: the kernel on the FIXTURE's arrays is no further from their float64 numpy evaluation than the reference's own float32
    result, floored at one float32 ulp; the returned statistics are within one float32 ulp (+ 1e-12 relative) of the float64
    evaluation of the returned arrays."""
    z = fixture
    write_corpus(z, tmp_path)
    conf = json.loads(str(z["confs"]))[i]
    conf["base_path"] = str(tmp_path)
    lines = []
    data, definition = dp.data_pipeline(conf, log=lines.append)
    out = tmp_path / conf["processed_data_path"]
    # ---- bookkeeping
    names_ref = [str(s) for s in golden(z, i, "label_names")]
    assert sorted(definition["label_names"]) == sorted(names_ref) and definition["label_names"] == ["Happy", "Sad"]
    for k in ("ranges_train", "ranges_valid"):
        assert data[k].dtype == np.int32 and np.array_equal(data[k], golden(z, i, k)), k
    for k in ("ranges_train_labels", "ranges_valid_labels"):
        assert data[k].dtype == np.int32
        assert [definition["label_names"][c] for c in data[k]] == [names_ref[c] for c in golden(z, i, k)], k
    assert definition["dt"] == float(golden(z, i, "dt")) and definition["parents"] == [-1, 0, 1, 2, 3, 4, 3, 3, 0]
    assert definition["bone_names"][3] == "Spine2" and len(lines) == 6 + 2 + 1
    assert set(data) == {k[3:].split("@")[0] for k in z.files if k.startswith("c0/") and "/bvh/" not in k} - {"label_names", "dt"}
    # ---- features
    failures = []
    for k in FEATURES:
        ref = golden(z, i, k)
        assert data[k].dtype == np.float32 and data[k].shape == ref.shape, k
        if k == "X_audio_features":
            atol, rtol = 3e-6, 3e-6
        else:
            atol, rtol = (1e-3 if "v" in k[2:] else 2e-4), 1e-4
        err = np.abs(data[k].astype(np.float64) - ref)
        worst = float(np.max(err - rtol * np.abs(ref)))
        print(f"c{i} {k}: max |device - reference| = {err.max():.3e} (atol {atol:.0e}, rtol {rtol:.0e}; worst excess over rtol {worst:.3e})")
        if not np.all(err <= atol + rtol * np.abs(ref)):
            failures.append(k)
    assert not failures, failures
    # ---- trimmed files
    from scipy.io import wavfile
    from zeggs import anim
    wavs = sorted((out / "trimmed").rglob("*.wav"))
    assert len(wavs) == 6
    for p in wavs:
        fs, x = wavfile.read(str(p))
        ref = z[f"wav/{p.parent.name}/{p.stem}"]
        assert fs == 16000 and x.dtype == np.int16 and x.shape == ref.shape, p.name
        step = np.abs(x.astype(np.int32) - ref.astype(np.int32))
        print(f"c{i} {p.parent.name}/{p.name}: {int((step > 0).sum())} of {len(x)} samples differ, by {int(step.max())} at the most")
        assert step.max() <= 1 and (step > 0).sum() * 1000 <= len(x), p.name
        if p.stem.endswith("_x_1_0"):
            assert step.max() == 0, p.name               # silencing and trimming alone: exact
    bvhs = sorted((out / "trimmed").rglob("*.bvh"))
    assert len(bvhs) == (6 if conf["save_trimmed_animation"] else 0)
    for p in bvhs:
        b = anim.bvh_load(p)
        ref = golden(z, i, f"bvh/{p.parent.name}/{p.stem}")
        assert len(b["rotations"]) == len(ref) and b["order"] == "zyx" and b["names"][5] == "Head", p.name
        dpos = np.abs(b["positions"][:, 0] - ref[:, :3]).max()
        drot = np.abs((b["rotations"].reshape(len(ref), -1) - ref[:, 3:] + 180.0) % 360.0 - 180.0).max()
        print(f"c{i} {p.parent.name}/{p.name}: positions differ by {dpos:.3e} (2e-3), degrees by {drot:.3e} (2e-2)")
        assert dpos <= 2e-3 and drot <= 2e-2, p.name
    # ---- statistics: the kernel on the fixture's own arrays
    gold = {k: golden(z, i, k) for k in FEATURES + ("ranges_train",)}
    ref64 = reference_stats(gold)
    mask = np.zeros(len(gold["X_audio_features"]), dtype=bool)
    for s, e in gold["ranges_train"]:
        mask[s + 2:e - 2] = True
    st = {k: [t.cpu().numpy() for t in dp.masked_stats(g(gold[k]), g(mask))] for k in ("X_audio_features",) + IN_STATS[:-1]}
    keys = IN_STATS[:-1]
    dev = dict(audio_input_mean=st["X_audio_features"][0], audio_input_std=st["X_audio_features"][2] + 1e-10,
               anim_output_mean=np.hstack([st[k][0] for k in keys]), anim_output_std=np.hstack([st[k][1] for k in keys]),
               anim_input_mean=np.hstack([st[k][0] for k in keys]),
               anim_input_std=np.hstack([np.repeat(st[k][2] + 1e-10, len(st[k][0])) for k in keys]))
    for k, v in dev.items():
        theirs = np.atleast_1d(golden(z, i, k)).astype(np.float64)[:len(ref64[k])]      # (the input statistics end with gaze_dir: not returned)
        d_ref, d_dev = np.abs(theirs - ref64[k]), np.abs(v.astype(np.float32).astype(np.float64) - ref64[k])
        print(f"c{i} {k}: kernel on the fixture's arrays: distance {d_dev.max():.3e}, the reference's own {d_ref.max():.3e}")
        assert np.all(d_dev <= np.maximum(d_ref, ulp32(ref64[k]))), k
    # ---- statistics: what data_pipeline returned against the float64 evaluation of what it returned
    mine64 = reference_stats(data)
    for k, v in mine64.items():
        got = np.atleast_1d(data[k])
        assert got.dtype == np.float32 and got.shape == np.atleast_1d(golden(z, i, k)).shape, k
        err = np.abs(got.astype(np.float64)[:len(v)] - v)
        print(f"c{i} {k}: returned against float64 numpy on the returned arrays: {np.max(err / ulp32(v)):.3f} ulp")
        assert np.all(err <= ulp32(v) + 1e-12 * np.abs(v)), k
    # the gaze_dir tail of the input statistics (Y_gaze_dir is not returned): against the reference's at the feature tolerance
    for k, atol in (("anim_input_mean", 2e-4), ("anim_input_std", 2e-4)):
        np.testing.assert_allclose(data[k][-3:], golden(z, i, k)[-3:], atol=atol, rtol=1e-4, err_msg=k)
    # ---- files
    saved = np.load(out / "processed_data.npz")
    assert set(saved.files) == set(data) and all(np.array_equal(saved[k], data[k]) for k in data)
    stats = np.load(out / "stats.npz")
    assert set(stats.files) == {k for k in data if not k.startswith(("X_", "Y_"))}
    assert json.loads((out / "data_definition.json").read_text()) == definition
    assert json.loads((out / "data_pipeline_conf.json").read_text()) == conf


def test_centring_changes_the_dataset_as_in_the_reference(fixture):
    """The fixture itself: with save_trimmed_animation the features come from the centred take (c0 against c1), and the order of
    len_ratios matters (c2) -- what test_data_pipeline_vs_reference pins is not one dataset three times."""
    z = fixture
    assert np.abs(golden(z, 0, "Y_gaze_pos") - golden(z, 1, "Y_gaze_pos")).max() > 1.0
    assert np.abs(golden(z, 0, "Y_lpos") - golden(z, 1, "Y_lpos")).max() > 0.01
    assert np.array_equal(golden(z, 0, "X_audio_features"), golden(z, 1, "X_audio_features"))


# ----------------------------------------------------------------------------- 4. round trip
def test_prepare_then_train_round_trip(tmp_path):
    """`python -m zeggs.cli prepare` on a raw synthetic corpus (75 joints, one train take at two ratios, one validation take), then
    train() for two iterations on the files it wrote: finite losses, no exception."""
    from zeggs import cli
    from zeggs import train as train_mod
    takes = [synth.make_raw_take("a_Happy", 150, seed=1, style="Happy"), synth.make_raw_take("b_Sad", 120, seed=2, style="Sad", validation=True)]
    synth.write_raw_corpus(tmp_path, takes)
    conf = synth.pipeline_conf(tmp_path, save_trimmed_audio=False, save_trimmed_animation=False)
    (tmp_path / "conf.json").write_text(json.dumps(conf))
    assert cli.main(["prepare", "-c", str(tmp_path / "conf.json")]) == 0
    data = tmp_path / "processed"
    net_opt = {"decoder": {"nhidden": 1024, "num_rnn_layers": 2, "rnn_cond": "normal"},
               "speech_encoder": {"nhidden": 64, "speech_encoding_size": 64},
               "style_encoder": {"nhidden": 512, "style_encoding_size": 64, "example_length": 16, "type": "attn", "use_vae": True}}
    train_opt = dict(niterations=0.002, batchsize=4, window=8, change_pace=True, learning_rate=1e-4, learning_rate_decay=0.995,
                     eps=1e-5, resume=False, use_gpu=True, thread_count=1, seed=1234, use_tensorboard=False,
                     style_encoding_type="example", generate_samples_step=100, use_script=False)
    (tmp_path / "models").mkdir(), (tmp_path / "logs").mkdir()
    train_mod.train(tmp_path / "models", tmp_path / "logs", data / "processed_data.npz", data / "data_definition.json", train_opt, net_opt)
    eng = train_mod.last_engine
    assert eng.iteration >= 2 and torch.isfinite(eng.last_terms).all()


def test_data_pipeline_without_a_validation_take(fixture, tmp_path):
    """An info file whose takes are all training takes (the reference writes its files, then dies in its summary table): the dataset is
    built, ranges_valid is empty, and the train rows equal those of the full corpus (c1: the same conf with the validation take)."""
    z = fixture
    write_corpus(z, tmp_path)
    info = (tmp_path / "info.csv").read_text().splitlines()
    (tmp_path / "info.csv").write_text("\n".join(info[:3]) + "\n")
    conf = json.loads(str(z["confs"]))[1]
    conf["base_path"] = str(tmp_path)
    data, definition = dp.data_pipeline(conf)
    assert data["ranges_valid"].shape == (0, 2) and data["ranges_valid_labels"].shape == (0,)
    assert np.array_equal(data["ranges_train"], golden(z, 1, "ranges_train")) and definition["label_names"] == ["Happy", "Sad"]
    n = int(data["ranges_train"][-1, 1])
    assert len(data["Y_lpos"]) == n
    np.testing.assert_allclose(data["Y_lpos"], golden(z, 1, "Y_lpos")[:n], atol=2e-4, rtol=1e-4)
    assert (tmp_path / conf["processed_data_path"] / "processed_data.npz").exists()
