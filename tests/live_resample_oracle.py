"""Float64 restatement of the rate converter of live serving (include/zeggs_hip_resample.h), on NumPy and
fractions only -- nothing of the package under test, and not the library's coefficient table.  TEST INFRASTRUCTURE.

  g = gcd(fi, fo), L = fo / g, M = fi / g; output m sits at input position p_m = m M / L;
  s = min(1, L / M), c = rolloff s, W = Z / s;
  h(t) = c sinc(c t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta) for |t| < W, 0 elsewhere;
  y[m] = sum over the integers k with |p_m - k| < W of x[k] h(p_m - k), x[k] = 0 for k < 0 and, once the signal is closed,
  for k >= n_in.  While the signal is open output m is ready once p_m + W <= n_in; at close there are ceil(n_in L / M).
"""
from fractions import Fraction
from math import gcd

import numpy as np

DEFAULTS = dict(Z=64, rolloff=0.95, beta=10.0)


def ratio(fi, fo):
    g = gcd(int(fi), int(fo))
    return int(fo) // g, int(fi) // g


def width(L, M, Z):
    """W as an exact fraction of input samples"""
    return Fraction(Z) / min(Fraction(1), Fraction(L, M))


def h(t, L, M, Z=64, rolloff=0.95, beta=10.0):
    """the filter at t (float64 array, input samples), straight from the formula"""
    t = np.asarray(t, np.float64)
    s = min(1.0, L / M)
    c, W = rolloff * s, Z / s
    inside = np.abs(t) < W
    u = np.where(inside, t / W, 0.0)
    return np.where(inside, c * np.sinc(c * t) * np.i0(beta * np.sqrt(1.0 - u * u)) / np.i0(beta), 0.0)


def support(m, L, M, Z):
    """(first, last) integer k with |p_m - k| < W, by exact rational arithmetic"""
    p, W = Fraction(m * M, L), width(L, M, Z)
    lo, hi = p - W, p + W
    first = lo.numerator // lo.denominator + 1                    # smallest integer > p - W
    last = -((-hi.numerator) // hi.denominator) - 1               # largest integer < p + W
    return first, last


def ready_brute(n, L, M, Z):
    """outputs ready after n inputs: output m is ready once p_m + W <= n (all m before it are ready too: p_m grows)"""
    W, m = width(L, M, Z), 0
    while Fraction(m * M, L) + W <= n:
        m += 1
    return m


def total_brute(n, L, M):
    """outputs of a closed signal of n inputs: the m with p_m < n"""
    m = 0
    while Fraction(m * M, L) < n:
        m += 1
    return m


def output(m, x, L, M, Z=64, rolloff=0.95, beta=10.0):
    """y[m] from the samples x[0 : len(x)] (float64), zeros outside"""
    first, last = support(m, L, M, Z)
    k = np.arange(max(first, 0), min(last, len(x) - 1) + 1)
    if k.size == 0:
        return 0.0
    t = (m * M - k * L) / float(L)            # exact integers over L
    return float(np.sum(x[k] * h(t, L, M, Z, rolloff, beta)))


def whole(x, fi, fo, **kw):
    """the closed signal x at fi Hz -> float64 outputs at fo Hz"""
    x = np.asarray(x, np.float64)
    L, M = ratio(fi, fo)
    return np.array([output(m, x, L, M, **kw) for m in range(total_brute(len(x), L, M))])


class Stream:
    """the same signal arriving in pieces: push(chunk) -> the outputs that became ready, computed from the prefix alone;
    close() -> the tail against zero padding"""

    def __init__(self, fi, fo, **kw):
        (self.L, self.M), self.kw = ratio(fi, fo), kw
        self.Z = kw.get("Z", DEFAULTS["Z"])
        self.x, self.n_out = np.zeros(0), 0

    def _upto(self, count):
        out = np.array([output(m, self.x, self.L, self.M, **self.kw) for m in range(self.n_out, count)])
        self.n_out = max(self.n_out, count)
        return out

    def push(self, chunk):
        self.x = np.concatenate([self.x, np.asarray(chunk, np.float64)])
        return self._upto(ready_brute(len(self.x), self.L, self.M, self.Z))

    def close(self):
        return self._upto(total_brute(len(self.x), self.L, self.M))


def pcm16(x):
    """int16 PCM -> the float64 values s / 32768 (exact)"""
    return np.asarray(x, np.int16).astype(np.float64) / 32768.0


def cuts(n, seed, lo=1, hi=96):
    """random chunk lengths lo..hi that add up to n, from a fixed seed"""
    rng, out = np.random.default_rng(seed), []
    while sum(out) < n:
        out.append(int(min(rng.integers(lo, hi + 1), n - sum(out))))
    return out


def within_one_float32(dev, want):
    """every device float32 is the float32 nearest to the oracle's float64 or one of its two neighbours -> bool array"""
    dev, c = np.asarray(dev, np.float32), np.asarray(want, np.float64).astype(np.float32)
    return (dev == c) | (dev == np.nextafter(c, np.float32(-np.inf))) | (dev == np.nextafter(c, np.float32(np.inf)))
