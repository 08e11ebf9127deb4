"""The alignment contract (include/thesia_amd.h "Align two tracks") restated in numpy f64, with the additions in the stated order:
block k div 4096, in it four partial sums by k mod 4 in ascending k from +0, (p0 + p1) + (p2 + p3), the blocks of a group of 32 in
ascending order from +0, the groups in ascending order from +0.  The lags are the vector axis; nothing is summed by numpy itself.
The product of two f32 is exact in f64, so the products are formed first and only the additions are ordered."""
import math

import numpy as np

BLOCK, GROUP_BLOCKS = 4096, 32
GROUP = BLOCK * GROUP_BLOCKS
SUMMARY = 10
ABS = 1
OUT_SUMMARY, OUT_CURVE = 0, 1


def n_groups(N):
    return -(-N // GROUP)


def _extent(x, first, count):
    """x[first : first + count] as f64, +0 where the track has no sample"""
    x = np.asarray(x, np.float32)
    out = np.zeros(max(count, 0), np.float64)
    lo, hi = max(first, 0), min(first + count, x.size)
    if hi > lo:
        out[lo - first: hi - first] = x[lo:hi].astype(np.float64)
    return out


def _ordered(prod):
    """prod: [lanes, N] exact terms -> [lanes] sums in the contract's order"""
    lanes, N = prod.shape
    total = np.zeros(lanes)
    for g0 in range(0, N, GROUP):
        group = np.zeros(lanes)
        for k0 in range(g0, min(g0 + GROUP, N), BLOCK):
            blk = prod[:, k0: min(k0 + BLOCK, N)]
            p = np.zeros((lanes, 4))
            rows = blk.shape[1] // 4
            quads = blk[:, :rows * 4].reshape(lanes, rows, 4)
            for m in range(rows):
                p += quads[:, m, :]
            for q in range(blk.shape[1] - rows * 4):
                p[:, q] += blk[:, rows * 4 + q]
            group = group + ((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3]))
        total = total + group
    return total


def xcorr(a, b, first, n_lags):
    """r[i] = sum_k a[k] b[first + i + k], i < n_lags"""
    a = np.asarray(a, np.float32).astype(np.float64)
    N = a.size
    if n_lags == 0:
        return np.zeros(0)
    if N == 0:
        return np.zeros(n_lags)
    ext = _extent(b, first, N + n_lags - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        win = np.lib.stride_tricks.sliding_window_view(ext, N)   # [n_lags, N]
        return _ordered(win * a[None, :])


def energy(x, first, N):
    v = _extent(x, first, N)
    with np.errstate(invalid="ignore", over="ignore"):
        return float(_ordered((v * v)[None, :])[0]) if N else 0.0


def exact_terms(a, b, first, lag_index):
    """the exact products of one lag as python floats (for math.fsum)"""
    a = np.asarray(a, np.float32).astype(np.float64)
    return (a * _extent(b, first + lag_index, a.size)).tolist()


def peak(r, flags, e_ref):
    """-> (status, index, delta, polarity)"""
    r = np.asarray(r, np.float64)
    if r.size == 0 or not math.isfinite(e_ref) or not e_ref > 0.0 or not np.isfinite(r).all():
        return 1, 0, 0.0, 1.0
    m = np.abs(r) if flags & ABS else r
    i = int(np.argmax(m))   # the first of the largest
    delta = 0.0
    if 0 < i < r.size - 1:
        mm, m0, mp = float(m[i - 1]), float(m[i]), float(m[i + 1])
        den = (mm - 2.0 * m0) + mp
        delta = (0.5 * (mm - mp)) / den if den < 0.0 else 0.0
    return 0, i, delta, (-1.0 if r[i] < 0.0 else 1.0)


def summary(r, D, flags, e_ref, e_probe_at):
    """the ten doubles; e_probe_at(index) -> E_probe at the peak's index"""
    st, i, delta, pol = peak(r, flags, e_ref)
    if st:
        return np.array([1.0] + [math.nan] * 9)
    f = np.float64
    with np.errstate(all="ignore"):
        rs, e_ref, e_probe = f(r[i]), f(e_ref), f(e_probe_at(i))
        gain = rs / e_ref
        resid = e_probe - rs * gain
        if resid < 0.0:
            resid = f(0.0)
        rho = rs / f(math.sqrt(e_ref * e_probe)) if e_ref * e_probe >= 0 else f(math.nan)
        q = resid / e_probe
        null = f(math.nan) if math.isnan(q) else f(-math.inf) if q == 0 else f(math.inf) if math.isinf(q) else f(10.0 * math.log10(q))
    return np.array([0.0, float(i - D), delta, rs, e_ref, e_probe, rho, gain, null, pol])


def align(ref, probe, s0, s1, D, kind=OUT_SUMMARY, flags=0):
    """a whole request on [s0, s1) of ref over the lags -D .. D"""
    ref, probe = np.asarray(ref, np.float32), np.asarray(probe, np.float32)
    N = s1 - s0
    n_lags = 2 * D + 1 if N else 0
    a = ref[s0:s1]
    r = xcorr(a, probe, s0 - D, n_lags)
    e_ref = energy(a, 0, N)
    out = summary(r, D, flags, e_ref, lambda i: energy(probe, s0 + i - D, N))
    return np.concatenate([out, r]) if kind == OUT_CURVE else out
