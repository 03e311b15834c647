"""Float64 restatement of the running loudness estimate of live serving (include/zeggs_hip_loudness.h), on
oracle.loudness.IIRfilter and NumPy only -- nothing of the package under test.  TEST INFRASTRUCTURE.

  y = HP(HS(x)) over the whole float32 signal, each stage's output rounded to float32 (pyloudnorm on a float32 array);
  block j = samples [trunc(0.4 (j 0.25) fs), trunc(0.4 (j 0.25 + 1) fs)), taken when its last sample is there;
  z_j = sum(y[lo:hi]^2) / (0.4 fs) as 256 strided partial sums and a tree;
  after block j: the two gates over blocks max(0, j - NB + 1) .. j, NB = round(horizon * 10); with at least `warmup` blocks past
  the relative gate L_j = -0.691 + 10 log10(mean gated z) is a new estimate and -- unless the block is in `hold_blocks` -- the
  gain becomes float32(10^(clip(target - L_j, gain_db) / 20)) from sample hi_j on; otherwise estimate and gain stay.
"""
import numpy as np

from oracle.loudness import IIRfilter

ABS_GATE = -70.0


def block_bounds(j, fs):
    return int(0.4 * (j * 0.25) * fs), int(0.4 * (j * 0.25 + 1) * fs)


def kweighted(x, fs):
    """the filtered signal as float64 values that are float32 numbers"""
    y = np.asarray(x, np.float32)
    for f in (IIRfilter(4.0, 1 / np.sqrt(2), 1500.0, fs, "high_shelf"), IIRfilter(0.0, 0.5, 38.0, fs, "high_pass")):
        y = f.apply_filter(y.astype(np.float64)).astype(np.float32)
    return y.astype(np.float64)


def block_energy(y, lo, hi, fs):
    sq = np.zeros(-(-(hi - lo) // 256) * 256)
    sq[:hi - lo] = y[lo:hi] ** 2
    s = np.zeros(256)
    for row in sq.reshape(-1, 256):          # thread t: samples lo + t, lo + t + 256, ... in that order
        s += row
    o = 128
    while o:
        s[:o] += s[o:2 * o]
        o //= 2
    return s[0] * (1.0 / (0.4 * fs))


def _level(z):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def running_loudness(x, fs, target=-20.0, horizon=60.0, warmup=1, gain_db=(-30.0, 30.0), gain0=1.0, hold_blocks=()):
    """-> dict(gain: float32 [n], the gain of every sample; blocks: one dict per completed block j with hi, z, fresh (a new
    estimate), lufs (the last estimate so far, NaN before the first), gated (blocks past the relative gate), held (the gain was
    left as it was) and g (the float32 gain from sample hi on); d_abs / d_rel: per block, the distance in dB of every block in
    the ring to the absolute and to the relative gate (d_rel is empty where there is no relative gate: nothing passed the
    absolute one))"""
    x = np.asarray(x, np.float32)
    n, NB = x.size, int(round(horizon * 10))
    y = kweighted(x, fs)
    gain = np.full(n, np.float32(gain0), np.float32)
    g, lufs = np.float32(gain0), float("nan")
    zs, blocks, d_abs, d_rel = [], [], [], []
    j = 0
    while block_bounds(j, fs)[1] <= n:
        lo, hi = block_bounds(j, fs)
        zs.append(block_energy(y, lo, hi, fs))
        z = np.array(zs[max(0, j - NB + 1):])
        lev = _level(z)
        d_abs.append(np.abs(lev - ABS_GATE))
        a = lev >= ABS_GATE
        gamma_r = _level(z[a].sum() / a.sum()) - 10.0 if a.any() else float("nan")
        d_rel.append(np.abs(lev - gamma_r) if a.any() else np.zeros(0))
        with np.errstate(invalid="ignore"):
            r = (lev > gamma_r) & (lev > ABS_GATE)
        gated = int(r.sum())
        fresh = gated >= warmup
        if fresh:
            lufs = float(_level(z[r].sum() / gated))
        held = not fresh or j in hold_blocks
        if not held:
            g = np.float32(10.0 ** (np.clip(target - lufs, gain_db[0], gain_db[1]) / 20.0))
            gain[hi:] = g
        blocks.append(dict(hi=hi, z=zs[-1], fresh=fresh, lufs=lufs, gated=gated, held=held, g=g))
        j += 1
    return dict(gain=gain, blocks=blocks, d_abs=d_abs, d_rel=d_rel)


def state_after(trace, n):
    """what a row reports once n samples have arrived: dict(lufs, gain, blocks, gated, held) (before the first block: gain0)"""
    done = [b for b in trace["blocks"] if b["hi"] <= n]
    if not done:
        return dict(lufs=float("nan"), gain=float(trace["gain"][0]) if trace["gain"].size else 1.0, blocks=0, gated=0, held=False)
    b = done[-1]
    return dict(lufs=b["lufs"], gain=float(b["g"]), blocks=len(done), gated=b["gated"], held=b["held"])


def min_gate_distance(trace):
    return min([float(d.min()) for d in trace["d_abs"] + trace["d_rel"] if d.size] or [float("inf")])


def signals(fs=16000):
    """the four test signals (float32, whole hops beyond the first block): speech, gap, quiet, step"""
    from zeggs import synth
    s = (synth.synth_wav(6 * fs + 321, seed=8) / 32768).astype(np.float32)
    rng = np.random.default_rng(5)
    a = (0.05 * rng.standard_normal(2 * fs)).astype(np.float32)
    b = (1e-5 * rng.standard_normal(3 * fs)).astype(np.float32)
    zero = lambda k: np.zeros(k * fs, np.float32)  # noqa: E731
    cat = lambda *p: np.concatenate([np.asarray(q, np.float32) for q in p])  # noqa: E731
    hop, blk = fs // 10, int(0.4 * fs)
    return dict(speech=s[:blk + hop * 30],
                gap=cat(s[:2 * fs], zero(3), np.float32(0.3) * s[2 * fs:4 * fs], zero(2))[:blk + hop * 80],
                quiet=cat(a, b)[:blk + hop * 40],
                step=cat(np.float32(0.02) * s[:3 * fs], s[:3 * fs])[:blk + hop * 50])
