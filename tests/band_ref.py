"""The band filter's definitions (include/thesia_amd.h, "Export what a spectrogram box holds") restated in numpy: the plan, the row,
every output as an f64 sum of the f32 coefficients times the samples with the sum of the magnitudes that the rounding-error bound
needs, and the magnitude response of a row.  Integer and f64 arithmetic only.  Nothing here calls the library: the tests compare it
with this."""
import math

import numpy as np

PASS, STOP = 0, 1
MAX_TAPS, DEFAULT_HALF_TAPS = 65536, 2048
BH = (0.35875, 0.48829, 0.14128, 0.01168)


def plan(sr, mode, f_lo_hz, f_hi_hz, trans_hz=0.0):
    """-> dict(K, mode, f_lo, f_hi, trans), or the name of the refusal: "invalid" / "unsupported"; K == 0 is the identity"""
    if sr == 0 or mode not in (PASS, STOP) or any(math.isnan(v) for v in (f_lo_hz, f_hi_hz, trans_hz)):
        return "invalid"
    nyq = sr / 2.0
    f_hi, f_lo = min(f_hi_hz, nyq), f_lo_hz
    if f_lo < 0 or f_lo >= f_hi or trans_hz < 0 or trans_hz > nyq:
        return "invalid"
    whole = f_lo == 0 and f_hi == nyq
    if whole:
        return "invalid" if mode == STOP else {"K": 0, "mode": mode, "f_lo": f_lo, "f_hi": f_hi, "trans": 0.0}
    K = DEFAULT_HALF_TAPS if trans_hz == 0 else math.ceil((16.0 * sr) / (5.0 * trans_hz))
    if 2 * K > MAX_TAPS:
        return "unsupported"
    return {"K": K, "mode": mode, "f_lo": f_lo, "f_hi": f_hi, "trans": (16.0 * sr) / (5.0 * K)}


def trans_for(sr, K):
    """a trans_hz that plans to K half taps: the width K has, nudged up while the division's rounding would ask for K + 1"""
    t = (16.0 * sr) / (5.0 * K)
    while plan(sr, PASS, 1.0, 2.0, t)["K"] > K:
        t = float(np.nextafter(t, np.inf))
    assert plan(sr, PASS, 1.0, 2.0, t)["K"] == K
    return t


def _sinc(x):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(np.pi * x) / (np.pi * x))


def window(u):
    b = BH[0] + BH[1] * np.cos(np.pi * u) + BH[2] * np.cos(2.0 * np.pi * u) + BH[3] * np.cos(3.0 * np.pi * u)
    return np.where(np.abs(u) < 1.0, b * b, 0.0)


def row(sr, p):
    """the 2K taps in f64"""
    K = p["K"]
    t = np.arange(2 * K, dtype=np.float64) - float(K) + 1.0
    a, c = 2.0 * p["f_hi"] / float(sr), 2.0 * p["f_lo"] / float(sr)
    delta = (t == 0.0).astype(np.float64)
    A = a * _sinc(a * t) if a < 1.0 else delta
    h = (A - c * _sinc(c * t)) * window(t / float(K))
    return delta - h if p["mode"] == STOP else h


def filt(x, c32, j0=0, n=None):
    """outputs [j0, j0 + n) of one channel x (f32, the whole channel) under the f32 row c32 -> (y in f64, sum over the taps of |c x| in
    f64): y[j] = sum over k of c32[k] x[j - K + 1 + k], multiplied and summed in f64"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    c = np.asarray(c32, dtype=np.float32).astype(np.float64)
    K = c.size // 2
    n = x.size - j0 if n is None else n
    assert j0 + n <= x.size
    y, mag = np.empty(n), np.empty(n)
    k = np.arange(2 * K, dtype=np.int64)
    for i in range(n):
        idx = j0 + i - K + 1 + k
        ok = (idx >= 0) & (idx < x.size)
        prod = c[ok] * x[idx[ok]]
        y[i] = math.fsum(prod)
        mag[i] = math.fsum(np.abs(prod))
    return y, mag


def bound(K, mag):
    """|y - y64| of the contract's f32 summation: a product passes its own fmaf, at most K / 2 more of its partial sum and the two
    additions of the fold, K / 2 + 3 roundings of relative size 2^-24 at most: within the resampler's (2K + 4) 2^-24 sum |c x| + 2^-149
    for every K up to 32768, second-order terms included"""
    return (2 * K + 4) * 2.0 ** -24 * mag + 2.0 ** -149


def response_db(c, sr, hz):
    """20 log10 |sum over k of c[k] e^(-i 2 pi hz (k - K + 1) / sr)| of a row c (f64 or f32), in f64"""
    c = np.asarray(c).astype(np.float64)
    K = c.size // 2
    t = np.arange(2 * K, dtype=np.float64) - float(K) + 1.0
    hz = np.asarray(hz, dtype=np.float64)
    out = np.empty(hz.size)
    for i, f in enumerate(hz):
        ph = (2.0 * np.pi * f / float(sr)) * t
        out[i] = 20.0 * np.log10(np.hypot(np.dot(c, np.cos(ph)), np.dot(c, np.sin(ph))))
    return out
