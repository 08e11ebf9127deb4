"""The polyphase sinc resampler's definitions (include/thesia_amd.h, "Export at a target sample rate") restated in numpy: the plan,
the output length, the prototype, the coefficient rows, and every output as an f64 sum of the f32 coefficients times the samples,
with the sum of the magnitudes that the rounding-error bound needs.  Integer and f64 arithmetic only.  Nothing here calls the
library: the tests compare it with this."""
import math

import numpy as np

Z, FC = 128, 0.95
MAX_TAPS, MAX_COEFS = 16384, 1 << 24
BH = (0.35875, 0.48829, 0.14128, 0.01168)


def plan(sr_in, sr_out):
    """-> dict(L, M, K, rho, cutoff), or the name of the refusal: "invalid" / "unsupported" """
    if sr_in == 0 or sr_out == 0:
        return "invalid"
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    K = Z if L >= M else -((-Z * M) // L)
    if 2 * K > MAX_TAPS or L * 2 * K > MAX_COEFS:
        return "unsupported"
    rho = 1.0 if L >= M else L / M
    return {"L": L, "M": M, "K": K, "rho": rho, "cutoff": rho * FC}


def n_out(n_in, p):
    return -((-n_in * p["L"]) // p["M"])


def proto(p, t):
    """h(t), t in input samples (f64 array)"""
    t = np.asarray(t, dtype=np.float64)
    x = p["cutoff"] * t
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(x == 0.0, 1.0, np.sin(np.pi * x) / (np.pi * x))
    u = p["rho"] * t / float(Z)
    b = BH[0] + BH[1] * np.cos(np.pi * u) + BH[2] * np.cos(2.0 * np.pi * u) + BH[3] * np.cos(3.0 * np.pi * u)
    return np.where(np.abs(u) < 1.0, p["cutoff"] * sinc * (b * b), 0.0)


def row(p, r):
    """the 2K taps of phase r in f64: h(k - K + 1 - r / L)"""
    k = np.arange(2 * p["K"], dtype=np.float64)
    return proto(p, (k - float(p["K"]) + 1.0) - float(r) / float(p["L"]))


def table32(p, rows=None):
    """{r: f32 row} for the given rows (all of them when None)"""
    return {int(r): row(p, int(r)).astype(np.float32) for r in (range(p["L"]) if rows is None else rows)}


def resample(x, sr_in, sr_out, j0=0, n=None):
    """outputs [j0, j0 + n) of one channel x (f32, the whole channel) -> (y in f64, sum over the taps of |c x| in f64): the f32
    coefficients and the f32 samples multiplied and summed in f64"""
    p = plan(sr_in, sr_out)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    no = n_out(x.size, p)
    n = no - j0 if n is None else n
    assert j0 + n <= no
    L, M, K = p["L"], p["M"], p["K"]
    j = np.arange(j0, j0 + n, dtype=object) if (j0 + n) * M >= 2 ** 62 else np.arange(j0, j0 + n, dtype=np.int64)
    q, r = (j * M) // L, (j * M) % L
    q, r = q.astype(np.int64), r.astype(np.int64)
    tab = table32(p, np.unique(r))
    y, mag = np.empty(n), np.empty(n)
    k = np.arange(2 * K, dtype=np.int64)
    for i in range(n):
        idx = q[i] - K + 1 + k
        ok = (idx >= 0) & (idx < x.size)
        c = tab[int(r[i])].astype(np.float64)[ok]
        prod = c * x[idx[ok]]
        y[i] = math.fsum(prod)
        mag[i] = math.fsum(np.abs(prod))
    return y, mag


def bound(p, mag):
    """|y - y64| of any f32 summation of the 2K products, with or without fma: (2K + 4) 2^-24 sum |c x| + 2^-149"""
    return (2 * p["K"] + 4) * 2.0 ** -24 * mag + 2.0 ** -149
