"""The float64 oracle of the style bank (include/zeggs_hip_styles.h), written from the definition alone: what a slot
holds of an encoder row, the mixed row of a record, the collapse of a row's old fade, and the bound of the mixed row.  numpy only;
shared by tests/test_live_styles_cpu.py and tests/test_gpu_live_styles.py."""
import numpy as np

MAX_TERMS = 8


def slot_of(enc, ST):
    """(mean, dev) in float64 of an encoder row: [mean | log-variance] of 2 ST floats, or a plain vector of ST (dev 0)"""
    enc = np.asarray(enc, np.float32).astype(np.float64)
    if enc.size == ST:
        return enc.copy(), np.zeros(ST)
    assert enc.size == 2 * ST
    return enc[:ST].copy(), np.exp(0.5 * enc[ST:])


def mix(bank, terms, temperature=0.0, eps=None):
    """bank [capacity, 2, ST] float32, terms [(slot, weight)] (weights as float32 values), eps [>= len(terms), ST] float32 or None
    -> (the sum in float64 [ST], sum_i |w_i v_i| [ST]): sum_i w_i (mean_i + (dev_i / temperature) eps_i) in the order of the terms"""
    bank = np.asarray(bank, np.float32).astype(np.float64)
    t = float(np.float32(temperature))
    acc, mag = np.zeros(bank.shape[2]), np.zeros(bank.shape[2])
    for i, (slot, w) in enumerate(terms):
        v = bank[slot, 0].copy()
        if eps is not None and t > 0.0:
            v = v + (bank[slot, 1] / t) * np.asarray(eps, np.float32).astype(np.float64)[i]
        w = float(np.float32(w))
        acc = acc + w * v
        mag = mag + np.abs(w * v)
    return acc, mag


def ulp32(x):
    """the spacing of float32 at |x| (the smallest subnormal at 0)"""
    x = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def bound(want, mag):
    """|got - want| <= 1/2 ulp32(want) + 2^-48 sum_i |w_i v_i|: the one rounding at the store, and at most 8 float64 roundings of
    the sum with room to spare (derived, not measured)"""
    return 0.5 * ulp32(want) + 2.0 ** -48 * np.asarray(mag, np.float64)


def weight(f, k, fade):
    """weight of the new style at frame f (zeggs.live.style_weight restated)"""
    return min(max((f - k + 1) / (fade + 1.0), 0.0), 1.0)


def lerp32(a, b, w):
    """torch.lerp's float32 formula, every operation rounded to float32: w < 0.5 ? a + w (b - a) : b - (b - a) (1 - w)"""
    a, b, w = np.asarray(a, np.float32), np.asarray(b, np.float32), np.float32(w)
    d = (b - a).astype(np.float32)
    if w < np.float32(0.5):
        return (a + (w * d).astype(np.float32)).astype(np.float32)
    return (b - (d * (np.float32(1.0) - w)).astype(np.float32)).astype(np.float32)


def lerp32_fused(a, b, w):
    """the same formula with the multiply-add of either branch contracted into one rounding, as a compiler may: fma(w, b - a, a) /
    fma(-(b - a), 1 - w, b).  (float64 holds the product of two float32 values exactly, and its sum with a third rounds to
    float32 as the fused operation does except in double-rounding ties, which the seeded inputs here do not hit.)"""
    a, b, w = np.asarray(a, np.float32), np.asarray(b, np.float32), np.float32(w)
    d = (b - a).astype(np.float32).astype(np.float64)
    if w < np.float32(0.5):
        return (a.astype(np.float64) + np.float64(w) * d).astype(np.float32)
    return (b.astype(np.float64) - d * np.float64(np.float32(1.0) - w)).astype(np.float32)


def collapse(old, new, k, k_style, fade_style):
    """the row's new old vector: where the fade (k_style, fade_style) stands at frame k - 1"""
    return lerp32(old, new, np.float32(weight(k - 1, k_style, fade_style)))
