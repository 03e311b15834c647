"""The float64 oracle of LiveServer's moving gaze: the definition of set_gaze() restated in numpy from its text (the README's and
DESIGN 3.7's), not from csrc/gaze_math.h.  A schedule is a dict(start, end, pivot: float32 [3]; k, fade: int; path, ease: str) --
the state is float32, every evaluation is float64, and a value becomes float32 once, where it is stored.

  weight(f, k, fade)            the weight of the new target at frame f (style_weight's rule)
  point(s, f)                   what frame f looks at under schedule s, float64 [3]
  resolve(rpos, rrot, p)        a root-space point in the model's world, float64 [3]
  reset(gaze0)                  the schedule of a stream that has just been opened
  apply(s, k, target, ...)      the schedule after set_gaze() returned k
  track(n, gaze0, sets)         the float64 per-frame gaze points of frames 0 .. n - 1 of a stream with a list of sets
  bound(want)                   the per-component tolerance of a float32 result against float32(want)"""
import numpy as np

EPS = 1e-6


def weight(f, k, fade):
    return min(max((f - k + 1) / (fade + 1.0), 0.0), 1.0)


def _eased(w, ease):
    assert ease in ("linear", "smooth")
    return w * w * (3.0 - 2.0 * w) if ease == "smooth" else w


def _line(p0, p1, w):
    return (1.0 - w) * p0 + w * p1


def path_point(p0, p1, pivot, path, w):
    """P(w) from P(0) = p0 to P(1) = p1 (float64 [3])"""
    assert path in ("line", "arc")
    if path == "line":
        return _line(p0, p1, w)
    a, b = p0 - pivot, p1 - pivot
    la, lb = np.sqrt(a @ a), np.sqrt(b @ b)
    if la < EPS or lb < EPS:
        return _line(p0, p1, w)
    u, v = a / la, b / lb
    x = np.cross(u, v)
    s = np.sqrt(x @ x)
    if s < EPS:
        return _line(p0, p1, w)
    theta = np.arctan2(s, u @ v)
    return pivot + ((1.0 - w) * la + w * lb) * (np.sin((1.0 - w) * theta) * u + np.sin(w * theta) * v) / s


def point(s, f):
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)  # noqa: E731
    return path_point(f64(s["start"]), f64(s["end"]), f64(s["pivot"]), s["path"], _eased(weight(f, s["k"], s["fade"]), s["ease"]))


def resolve(rpos, rrot, p):
    """rpos + rrot (x) p with the quaternion (w first) as it is stored: t = 2 (q_v x p); p + w t + q_v x t"""
    rpos, q, p = (np.asarray(x, np.float32).astype(np.float64) for x in (rpos, rrot, p))
    t = 2.0 * np.cross(q[1:], p)
    return rpos + (p + q[0] * t + np.cross(q[1:], t))


def reset(gaze0):
    g = np.asarray(gaze0, np.float32).reshape(3)
    return dict(start=g.copy(), end=g.copy(), pivot=np.zeros(3, np.float32), k=0, fade=0, path="line", ease="linear")


def apply(s, k, target, fade=0, space="world", path="line", pivot=None, ease="linear", rpos=None, rrot=None):
    """the schedule after a set at frame k: it starts where `s` stands at frame k - 1; root-space points are resolved with
    rpos / rrot (the root after frame k - 1), and without a pivot of its own a root-space arc turns about rpos"""
    assert space in ("world", "root") and fade >= 0
    f32 = lambda x: np.asarray(x, np.float64).astype(np.float32)  # noqa: E731
    target = f32(target)                                 # the record carries float32
    piv = None if pivot is None else f32(pivot)
    if space == "root":
        end = resolve(rpos, rrot, target)
        c = np.asarray(rpos, np.float32).astype(np.float64) if piv is None else resolve(rpos, rrot, piv)
    else:
        assert not (path == "arc" and piv is None)
        end, c = target.astype(np.float64), np.zeros(3) if piv is None else piv.astype(np.float64)
    return dict(start=f32(point(s, k - 1)), end=f32(end), pivot=f32(c), k=int(k), fade=int(fade), path=path, ease=ease)


def track(n, gaze0, sets):
    """float64 [n, 3]: what frames 0 .. n - 1 look at; sets = [dict(k=, target=, ...)] in the order of the calls (k ascending).
    Frame f is governed by the last set with k <= f."""
    s, out, sets = reset(gaze0), np.zeros((n, 3)), list(sets)
    for f in range(n):
        while sets and sets[0]["k"] <= f:
            s = apply(s, **sets.pop(0))
        out[f] = point(s, f)
    return out


def bound(want):
    """one float32 rounding that a last-bit difference of two libms can flip: 2^-23 max(1, |want|) per component"""
    return 2.0 ** -23 * np.maximum(1.0, np.abs(np.asarray(want, np.float64)))
