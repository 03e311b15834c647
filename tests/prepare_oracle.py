"""Float64 restatements of the dataset-preparation kernels (csrc/prepare.hip, csrc/loudness.hip), the case tables
their tests share, and PREPARE_BUGS: named mistakes a kernel could make, as mutations of the restatements.  TEST INFRASTRUCTURE
ONLY: tests/test_prepare_oracle_cpu.py checks the restatements against known answers and that a named case of the tables sees every
mutation at 10 bounds or more; tests/test_gpu_prepare_kernels.py compares the kernels with them.

numpy only, plus the pinned quaternion helpers of oracle/anim.py and the loudness restatement of oracle/loudness.py; the dense
not-a-knot spline and ulp32 are those of tests/test_gpu_prepare.py.  Written from what the operations mean:
  silence_cut   wav times the union of the [lo, hi) sample intervals (numpy slice rules), then the [start:end] slice;
  center        the root (joint 0) re-based on frame 0: position minus (x, 0, z) of frame 0, turned by the inverse of frame 0's
                root quaternion times (1, 0, 1, 0) -- NOT normalised, so with pitch or roll at frame 0 it is no rotation;
  rot_stretch   Euler degrees -> quaternions -> sign unrolling -> spline on the four components -> normalise -> Euler degrees;
  masked_stats  mean, population std per column and the std of all masked elements;
  loudness      BS.1770 as oracle.loudness.Meter computes it, cut open at the block energies so that the gates can be mutated.
"""
import warnings

import numpy as np

from oracle import anim as oanim
from oracle import loudness as olo
from test_gpu_prepare import dense_spline, ulp32  # noqa: F401  (unchanged there; ulp32 is handed on to the tests)
from zeggs import synth

# ----------------------------------------------------------------------------- bounds (each one an existing bound of the project)
POS_TOL = 1e-9            # position units: BVH_TOL of tests/test_gpu_anim_dims.py
DEG_TOL = 1e-9            # degrees modulo 360: the bound of test_gpu_prepare.py::test_rot_stretch_vs_numpy_chain
LUFS_TOL64, LUFS_TOL32 = 1e-5, 2e-5          # LU: test_gpu_full_shapes.py::test_device_loudness_normalisation_vs_pyloudnorm_restatement
SAMPLE_RTOL, SAMPLE_ATOL = 3e-6, 1e-9        # normalised samples: the same test
SINE_TOL = 0.05           # LU: what tests/test_loudness_cpu.py holds the oracle to on the 997 Hz sine


def stats_bound(ref):
    """test_gpu_prepare.py::test_masked_stats_vs_numpy_float64: one float32 ulp of the reference plus 1e-12 relative"""
    return ulp32(ref) + 1e-12 * np.abs(ref)


def angle_diff(a, b):
    return np.abs((np.asarray(a) - np.asarray(b) + 180.0) % 360.0 - 180.0)


# ----------------------------------------------------------------------------- 1. silence + cut
def silence_cut(wav, intervals, start, end, bug=None):
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
    if bug == "last_interval_only":
        iv = iv[-1:]
    if bug == "intervals_after_cut":
        cut = wav[start:end]
        mask = np.zeros(len(cut), dtype=np.float32)
        for lo, hi in iv:
            mask[lo:hi] = 1.0
        return cut * mask
    mask = np.zeros(len(wav), dtype=np.float32)
    for lo, hi in iv:
        mask[lo:(hi + 1 if bug == "interval_end_inclusive" else hi)] = 1.0
    return (wav * mask)[start:end]


AUDIO_N = 10007


def _audio_case(id, intervals, start, end, n=AUDIO_N):
    return dict(id=id, n=n, intervals=np.asarray(intervals, dtype=np.int64).reshape(-1, 2), start=start, end=end)


GRID_EDGE = 8192 * 256     # elements one sweep of the grid-stride loop covers (grid_for in csrc/prepare.hip)
AUDIO_CASES = (
    _audio_case("k0", [], 100, 9000),
    _audio_case("one", [[2000, 5000]], 1000, 8000),
    _audio_case("touching", [[1000, 2000], [2000, 3000]], 500, 9000),
    _audio_case("overlapping", [[1000, 2500], [2000, 3000]], 500, 9000),
    _audio_case("nested", [[1000, 6000], [2000, 3000]], 500, 9000),
    _audio_case("unsorted", [[7000, 8000], [1000, 2000], [4000, 4500]], 500, 9000),
    _audio_case("empty-and-inverted", [[1000, 2000], [3000, 3000], [6000, 5000]], 0, 9000),
    _audio_case("past-n", [[9000, 12000], [20000, 30000], [500, 600]], 100, AUDIO_N),
    _audio_case("whole", [[0, 10], [5000, AUDIO_N]], 0, AUDIO_N),
    _audio_case("end-past-n", [[9000, 20000]], 8000, AUDIO_N + 500),
    _audio_case("start-eq-end", [[1000, 9000]], 4000, 4000),
    _audio_case("start-eq-n", [[1000, 20000]], AUDIO_N, AUDIO_N + 20),
    _audio_case("start-past-n", [[1000, 20000]], AUDIO_N + 10, AUDIO_N + 20),
    _audio_case("cut-inside-interval", [[1000, 9000]], 3000, 5000),
    _audio_case("k4096", [[100 + 2 * i, 101 + 2 * i] for i in range(4096)], 50, 9000),        # 64 KB of dynamic LDS
    _audio_case("grid-stride", [[5, 1000], [GRID_EDGE - 300, GRID_EDGE + 300], [2999000, 4000000]], 7, 3000017, n=3000017),
)
AUDIO_MAX_INTERVALS = 4096


def audio_wav(case):
    """float32 samples in (-1, 1) with exact zeros of both signs among them"""
    rng = np.random.default_rng(case["n"])
    w = rng.uniform(-1.0, 1.0, case["n"]).astype(np.float32)
    w[::97] = np.float32(-0.0)
    w[5::101] = np.float32(0.0)
    return w


# ----------------------------------------------------------------------------- 2. centring
def axis_quat(deg, axis):
    return oanim.q_from_angle_axis(np.radians(np.asarray(deg, dtype=np.float64)), oanim._AXES[axis])


def euler_for(q, order):
    """unit quaternions -> Euler degrees e with q_from_euler(radians(e), order) == q.  "zyx": q_to_euler.  "xzy": q_to_euler("xzy")
    is, as the reference's, NOT the inverse of q_from_euler("xzy") = qx(a) qz(b) qy(c): it takes qy qz qx apart and returns the
    angles as (x, y, z).  inv(q) = qy(-c) qz(-b) qx(-a) is of that form, so (a, b, c) = -(x, z, y) of q_to_euler(inv(q))."""
    if order == "xzy":
        return -np.degrees(oanim.q_to_euler(oanim.q_inv(q), "xzy"))[..., [0, 2, 1]]
    return np.degrees(oanim.q_to_euler(q, order))


def middle_angle(e):
    """of Euler INPUT in channel order: the middle rotation (y for "zyx", z for "xzy"), where the gimbal lock sits"""
    return e[..., 1]


def asin_angle(e, order):
    """of q_to_euler OUTPUT: the angle it takes with asin (channel 1 for "zyx", channel 2 for "xzy")"""
    return e[..., 2 if order == "xzy" else 1]


def center(pos, rot_deg, order, round_f32, bug=None):
    """-> (positions, rotations): copies with joint 0 centred on frame 0"""
    pos, rot = np.array(pos, dtype=np.float64), np.array(rot_deg, dtype=np.float64)
    js = slice(None) if bug == "all_joints_moved" else slice(0, 1)
    q = oanim.q_from_euler(np.radians(rot[:, js]), order)
    off_p = pos[0, 0] * (np.ones(3) if bug == "offset_y_kept" else np.array([1.0, 0.0, 1.0]))
    off_q = q[0, 0] * np.array([1.0, 0.0, 1.0, 0.0])
    if bug == "offset_normalised":
        off_q = oanim.q_normalize(off_q)
    inv = off_q if bug == "offset_not_inverted" else oanim.q_inv(off_q)
    new_p = oanim.q_mul_vec(inv, pos[:, js] - off_p)
    new_r = np.degrees(oanim.q_to_euler(oanim.q_mul(inv, q), order))
    if round_f32:
        new_p, new_r = new_p.astype(np.float32).astype(np.float64), new_r.astype(np.float32).astype(np.float64)
    pos[:, js], rot[:, js] = new_p, new_r
    return pos, rot


def center_horizontal_factor(off_q):
    """What v -> q_mul_vec(inv(o), v) does to lengths when o = (w, 0, y, 0) has the squared length s = w^2 + y^2 < 1:
    v + 2 w (u x v) + 2 u x (u x v) with u = (0, -y, 0) leaves the y component alone and sends a horizontal v to
    (1 - 2 y^2) v - 2 w y (e_y x v), of length |v| sqrt((1 - 2 y^2)^2 + 4 w^2 y^2) = |v| sqrt(1 - 4 y^2 (1 - s)).
    (s itself is the factor of the sandwich o v conj(o); the helpers' mul_vec is not that product when |o| != 1.)"""
    w, y = off_q[0], off_q[2]
    return float(np.sqrt(1.0 - 4.0 * y * y * (1.0 - (w * w + y * y))))


CENTER_SHAPES = ((1, 1), (1, 5), (256, 3), (257, 3), (600, 75))
CENTER_ROOTS = {"upright": (30.0, 0.0, 0.0), "tilted": (60.0, 40.0, 25.0), "yaw": (125.0, 4.0, -3.0)}     # heading, pitch, roll at frame 0
CENTER_CASES = tuple(dict(id=f"N{n}-J{j}-{root}-{order}", n=n, j=j, root=root, order=order)
                     for (n, j) in CENTER_SHAPES for root in CENTER_ROOTS for order in ("zyx", "xzy"))


def center_inputs(case):
    """-> (positions [N, J, 3], rotations [N, J, 3] degrees in the case's channel order).  The root turns about y by the heading and
    carries the pitch and roll of the case at frame 0 exactly, with a few degrees of smooth wobble after it."""
    n, j, order = case["n"], case["j"], case["order"]
    rng = np.random.default_rng(1000 * n + 10 * j + len(case["root"]))
    heading, pitch, roll = CENTER_ROOTS[case["root"]]
    if case["root"] == "yaw" and n % 2:
        heading = -heading
    wob = synth._smooth(rng, n, 3, 3.0)
    wob -= wob[0]
    t = np.arange(n) / max(n - 1, 1)
    q = oanim.q_mul(axis_quat(heading * (1.0 + 0.06 * t) + wob[:, 0], "y"),
                    oanim.q_mul(axis_quat(pitch + wob[:, 1], "x"), axis_quat(roll + wob[:, 2], "z")))
    rot = np.clip(synth._smooth(rng, n, j * 3, 25.0), -70.0, 70.0).reshape(n, j, 3)
    rot[:, 0] = euler_for(q, order)
    pos = rng.normal(0.0, 20.0, (n, j, 3))
    pos[:, 0] = np.array([5.0, 90.0, -7.0]) + synth._smooth(rng, n, 3, 30.0)
    return pos, rot


# ----------------------------------------------------------------------------- 3. rotation stretch
def rot_stretch(e, m, order, bug=None, with_quats=False):
    n, j = e.shape[:2]
    q = oanim.q_unroll(oanim.q_from_euler(np.radians(e), order), bug="no_unroll" if bug == "no_unroll" else None)
    qs = dense_spline(q.reshape(n, -1), m).reshape(m, j, 4)
    if bug != "no_normalise":
        qs = qs / np.linalg.norm(qs, axis=-1, keepdims=True)
    out = np.degrees(oanim.q_to_euler(qs, order))
    return (out, q) if with_quats else out


ROT_CASES = tuple(dict(id=f"J{j}-N{n}-M{m}", j=j, n=n, m=m) for j, n, m in (
    (1, "4", "1"), (1, "C+5", "1.1N"), (1, "2C+H+5", "2N-1"), (1, "C+3", "0.9N"),
    (2, "5", "2"), (2, "C+5", "0.9N"), (2, "2C+H+5", "N"), (2, "C+4", "1.1N"),
    (3, "6", "2N-1"), (3, "C+5", "1.1N"), (3, "C+3", "N"),
    (16, "C+4", "0.9N"), (16, "2C+H+5", "1.1N"), (16, "4", "2N-1"),
    (17, "C+5", "2N-1"), (17, "5", "N"), (17, "2C+H+5", "0.9N"),
    (75, "2C+H+5", "1.1N"), (75, "6", "1"), (75, "C+3", "2")))
ROT_MULTI_CHUNK = ("C+5", "2C+H+5")       # rows 2 .. N-3 are eliminated in chunks of C rows: more than C of them


def rot_sizes(case, c, h):
    n = {"4": 4, "5": 5, "6": 6, "C+3": c + 3, "C+4": c + 4, "C+5": c + 5, "2C+H+5": 2 * c + h + 5}[case["n"]]
    m = {"1": 1, "2": 2, "N": n, "2N-1": 2 * n - 1, "0.9N": int(0.9 * n), "1.1N": int(1.1 * n)}[case["m"]]
    return n, m


def wrap180(a):
    return (a + 180.0) % 360.0 - 180.0


def rot_inputs(case, n):
    """Smooth angles clipped to +-70 degrees; the first angle of joint 0 climbs 400 degrees (more than one turn), the first angle of
    the last joint swings about 180 degrees and is wrapped into [-180, 180): it jumps by about 360 once downwards and once upwards.  With
    one joint, joint 0 is both: its climb is wrapped (one jump)."""
    j = case["j"]
    rng = np.random.default_rng(100 * j + n)
    e = np.clip(synth._smooth(rng, n, j * 3, 25.0), -70.0, 70.0).reshape(n, j, 3)
    e[:, 0, 0] += np.linspace(0.0, 400.0, n)
    if j == 1:
        e[:, 0, 0] = wrap180(e[:, 0, 0])
    else:
        t = np.arange(n) / (n - 1)
        e[:, j - 1] *= 0.2
        e[:, j - 1, 0] = wrap180(180.0 + 25.0 * np.cos(2.0 * np.pi * t + 0.3))
    return e


# ----------------------------------------------------------------------------- 4. masked statistics
def masked_stats(x, mask, bug=None):
    """-> (mean [D], std [D], pooled [1]) in float64.  A column whose masked values are all equal has the std 0 exactly."""
    sel = np.asarray(x)[np.asarray(mask, dtype=bool)].astype(np.float64)
    n = len(mask) if bug == "mask_ignored_in_count" else len(sel)
    mean = sel.sum(axis=0) / n
    ssq = ((sel - mean) ** 2).sum(axis=0)
    std = np.sqrt(ssq / (n - 1 if bug == "sample_std" else n))
    std[np.ptp(sel, axis=0) == 0.0] = 0.0
    if bug == "pooled_mean_of_stds":
        pooled = std.mean()
    else:
        g = sel.sum() / (n * sel.shape[1])
        pooled = np.sqrt(((sel - g) ** 2).sum() / ((n - 1 if bug == "sample_std" else n) * sel.shape[1]))
    return mean, std, np.atleast_1d(pooled)


STATS_SLAB = 2048
STATS_CASES = tuple(dict(id=f"R{r}-D{d}-{mask}", r=r, d=d, mask=mask) for r, d, mask in (
    (1, 1, "all"), (1, 5, "all"), (2047, 2, "all"), (2048, 64, "all"), (2049, 65, "all"), (6150, 65, "all"),
    (2049, 1, "one"), (2048, 33, "one"),
    (6150, 130, "mid-slab-out"), (6150, 1, "mid-slab-out"), (6150, 2, "mid-slab-out"),
    (6150, 5, "first-slab-out"), (4096, 130, "first-slab-out"),
    (4096, 33, "ranges"), (6150, 64, "ranges"), (2047, 130, "ranges")))


def stats_tcol(d):
    """columns per workgroup of stats_partial_k: the next power of two for D < 64, else 64"""
    return 64 if d >= 64 else 1 << max(d - 1, 0).bit_length()


def stats_inputs(case):
    """-> (x float32 [R, D], mask bool [R]).  Column 0 has the mean 1e4 and the spread 1e-2 (wherever there is more than one row);
    column 1, where there is one, is constant."""
    r, d = case["r"], case["d"]
    rng = np.random.default_rng(7 * r + d)
    x = (rng.standard_normal((r, d)) * rng.uniform(0.1, 30.0, (1, d)) + rng.uniform(-50.0, 50.0, (1, d))).astype(np.float32)
    if r > 1:
        x[:, 0] = (1e4 + 1e-2 * rng.standard_normal(r)).astype(np.float32)
    if d > 1:
        x[:, 1] = np.float32(0.7251)
    mask = np.zeros(r, dtype=bool)
    kind = case["mask"]
    if kind == "all":
        mask[:] = True
    elif kind == "one":
        mask[r - 1] = True                        # R = 2049: the second slab's only row, the first slab counts nothing
    elif kind == "mid-slab-out":
        mask[:STATS_SLAB] = True
        mask[2 * STATS_SLAB:] = True
    elif kind == "first-slab-out":
        mask[STATS_SLAB:] = True
    else:
        a, b = r // 4, (3 * r) // 4
        for s, e in ((0, a), (a, a + 4), (a + 4, a + 7), (a + 7, b), (b + 300, r)):       # the two short ranges are empty
            mask[s + 2:e - 2] = True
    return x, mask


# ----------------------------------------------------------------------------- 5. loudness
T_G, STEP = 0.4, 0.25
GATE_STRIDE = 1024         # threads of gate_k: block j is read by thread j % 1024


def block_energies(x, rate, bug=None, chunk=4096):
    """K-weighted mean squares of the 400 ms blocks, 75 % overlap -> z [nblocks] (mono).  Each filter stage is stored back in the
    signal's own type, and the squares are summed in it, as oracle.loudness.Meter does."""
    x = np.asarray(x)
    y = x.copy()
    for f in olo.Meter(rate)._filters.values():
        if bug == "chunk_state_dropped":
            y[:] = np.concatenate([f.apply_filter(y[i:i + chunk]) for i in range(0, len(y), chunk)])
        else:
            y[:] = f.apply_filter(y)
    nblocks = int(np.round((len(x) / rate - T_G) / (T_G * STEP)) + 1)
    z = np.zeros(nblocks)
    for j in range(nblocks):
        lo, hi = int(T_G * (j * STEP) * rate), int(T_G * (j * STEP + 1) * rate)
        z[j] = (1.0 / (T_G * rate)) * np.sum(np.square(y[lo:hi]))
    return z


def block_levels(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def relative_gate(z):
    """Gamma_r: the level of the mean energy of the blocks at or above -70, minus 10"""
    lv = block_levels(z)
    with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        return -0.691 + 10.0 * np.log10(np.mean(z[lv >= -70.0])) - 10.0


def gated_loudness(z, bug=None):
    z = np.asarray(z, dtype=np.float64)
    if bug == "blocks_past_1024_ignored":
        z = z[:GATE_STRIDE]
    lv, gamma = block_levels(z), relative_gate(z)
    keep = ((lv >= gamma) if bug == "relative_gate_inclusive" else (lv > gamma)) & (lv > -70.0)
    zavg = np.mean(z[keep]) if np.any(keep) else 0.0
    with np.errstate(divide="ignore"):
        return float(-0.691 + 10.0 * np.log10(zavg))


def loudness(x, rate, bug=None, chunk=4096):
    return gated_loudness(block_energies(x, rate, bug, chunk), bug)


def _speech(n, rate, seed):
    return synth.synth_wav(n, seed=seed, fs=rate).astype(np.float64) / 32768.0


def _loud_case(id, rate, n, chunk=4096, kind="speech"):
    return dict(id=id, rate=rate, n=n, chunk=chunk, kind=kind)


def gate_samples(nblocks, rate=8000):
    """the shortest signal of `nblocks` gating blocks"""
    return int(round(rate * (T_G + T_G * STEP * (nblocks - 1))))


LOUD_RATE_CASES = tuple(_loud_case(f"rate-{r}", r, 2 * r + 37) for r in (8000, 22050, 44100, 48000))
LOUD_EDGE_CASES = tuple(_loud_case(f"n-{n}", 8000, n) for n in (3200, 4095, 4096, 4097, 8192, 8193))
LOUD_CHUNK_CASES = tuple(_loud_case(f"chunk-{c}", 8000, 16000, chunk=c) for c in (64, 100, 1000, 4096, 1 << 20))
LOUD_GATE_CASES = tuple(_loud_case(f"blocks-{k}", 8000, gate_samples(k), kind="gate") for k in (1023, 1024, 1025, 1100))
LOUD_CASES = LOUD_RATE_CASES + LOUD_EDGE_CASES + LOUD_CHUNK_CASES + LOUD_GATE_CASES
GATE_TIE = np.array([1.9, 0.1])      # block energies whose mean is 1 exactly: the second block sits ON the relative gate


def loud_signal(case):
    """float64 samples that float32 holds exactly.  "speech": band-limited noise under a syllabic envelope, silent from 30 % to 55 %
    of its length and 30 dB down from 60 % to 85 %.  "gate": a loud stretch (0.5), one 30 dB below it and silence, each before
    block 1024 (which starts at 102.4 s) and again from it on where the signal goes on; from 102.4 s the loud stretch is at 1.0."""
    n, rate = case["n"], case["rate"]
    if case["kind"] == "speech":
        x = _speech(n, rate, seed=n % 1000 + 1)
        x[int(0.30 * n):int(0.55 * n)] = 0.0
        x[int(0.60 * n):int(0.85 * n)] *= 0.03
    else:
        x = np.tile(_speech(4 * rate, rate, seed=11), n // (4 * rate) + 1)[:n]
        t = np.arange(n) / rate
        edge = GATE_STRIDE * T_G * STEP                     # 102.4 s
        gain = np.zeros(n)
        gain[t < 3.0] = 0.5
        gain[(t >= 3.0) & (t < 6.0)] = 0.015
        gain[(t >= 99.0) & (t < 100.7)] = 0.015
        gain[(t >= 100.7) & (t < edge)] = 0.5
        if t[-1] < edge + 1.0:
            gain[t >= edge] = 1.0                           # 1023 .. 1025 blocks: what lies past the edge is loud
        else:
            gain[(t >= edge + 2.0) & (t < edge + 4.5)] = 0.03
            gain[t >= edge + 4.5] = 1.0                     # silence, quiet, loud again from block 1024 on
        x = x * gain
    return x.astype(np.float32).astype(np.float64)


def sine(rate=48000, seconds=2.0, amplitude=1.0, hz=997.0):
    return (amplitude * np.sin(2.0 * np.pi * hz * np.arange(int(seconds * rate)) / rate)).astype(np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- the mutations: name -> (group, the case that sees it)
PREPARE_BUGS = {
    "interval_end_inclusive": ("audio", "one"),
    "intervals_after_cut": ("audio", "one"),
    "last_interval_only": ("audio", "touching"),
    "offset_normalised": ("center", "N257-J3-tilted-zyx"),
    "offset_not_inverted": ("center", "N256-J3-upright-xzy"),
    "offset_y_kept": ("center", "N1-J1-upright-zyx"),
    "all_joints_moved": ("center", "N1-J5-yaw-zyx"),
    "no_unroll": ("rot", "J3-NC+5-M1.1N"),
    "no_normalise": ("rot", "J17-NC+5-M2N-1"),
    "sample_std": ("stats", "R2047-D2-all"),
    "pooled_mean_of_stds": ("stats", "R4096-D33-ranges"),
    "mask_ignored_in_count": ("stats", "R6150-D130-mid-slab-out"),
    "chunk_state_dropped": ("loudness", "chunk-64"),
    "relative_gate_inclusive": ("gate", "tie"),
    "blocks_past_1024_ignored": ("loudness", "blocks-1025"),
}
