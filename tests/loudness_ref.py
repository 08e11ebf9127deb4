"""Restatement of the loudness arithmetic (StatCalculator::calc, dynamics/stats.rs:56-86: the ebur128 crate with Mode::all(), a port
of libebur128) for the tests: K-weighting design, the sequential f64 direct-form-II filter, 400 ms block energies, histogram gating.
Test infrastructure only: the product never imports it."""
import math

import numpy as np

MIN_SR, MAX_SR = 16, 2_822_400

# ITU-R BS.1770-4, Tables 1 and 2: the two stages of the K-weighting at 48 kHz
BS1770_STAGE1 = ([1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -1.69065929318241, 0.73248077421585])
BS1770_STAGE2 = ([1.0, -2.0, 1.0], [1.0, -1.99004745483398, 0.99007225036621])


def k_weighting(sr):
    """(b[5], a[5]) as libebur128's ebur128_init_filter designs them"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    pb = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    pa = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    rb = [1.0, -2.0, 1.0]
    ra = [1.0, 2.0 * (K * K - 1.0) / (1.0 + K / Q + K * K), (1.0 - K / Q + K * K) / (1.0 + K / Q + K * K)]
    b = [pb[0] * rb[0], pb[0] * rb[1] + pb[1] * rb[0], pb[0] * rb[2] + pb[1] * rb[1] + pb[2] * rb[0], pb[1] * rb[2] + pb[2] * rb[1],
         pb[2] * rb[2]]
    a = [pa[0] * ra[0], pa[0] * ra[1] + pa[1] * ra[0], pa[0] * ra[2] + pa[1] * ra[1] + pa[2] * ra[0], pa[1] * ra[2] + pa[2] * ra[1],
         pa[2] * ra[2]]
    return np.array(b), np.array(a)


def s100(sr):
    return (sr + 5) // 10


def n_blocks(n, sr):
    s = s100(sr)
    return 0 if n < 4 * s else (n - 4 * s) // s + 1


def channel_weight(c, n_ch):
    if n_ch == 4:
        return 1.0 if c < 2 else 1.41
    if n_ch == 5:
        return 1.0 if c < 3 else 1.41
    return 1.0 if c < 3 else 1.41 if c in (4, 5) else 0.0


def kfilter(x, sr, dtype=np.float64):
    """the sequential filter (v0 = x - a1 v1 - ... - a4 v4; y = b0 v0 + ... + b4 v4) from zero state, vectorised across channels.
    x: (C, N) f32 -> y: (C, N) f64.  dtype=np.longdouble: the same recurrence with the f64 coefficients in x87 extended precision.
    (The f64 filter's own rounding reaches 2e-10 (96 kHz) and 1.5e-9 (192 kHz) of a block energy on audio with a 0.4 DC offset,
    since the states grow with the high-pass's DC gain; the extended evaluation stays near 1e-13 there.)"""
    b, a = (c.astype(dtype) for c in k_weighting(sr))
    x = np.atleast_2d(np.asarray(x, np.float32)).astype(dtype)
    C, N = x.shape
    v1 = v2 = v3 = v4 = np.zeros(C, dtype)
    y = np.empty((C, N), dtype)
    for i in range(N):
        v0 = x[:, i] - a[1] * v1 - a[2] * v2 - a[3] * v3 - a[4] * v4
        y[:, i] = b[0] * v0 + b[1] * v1 + b[2] * v2 + b[3] * v3 + b[4] * v4
        v4, v3, v2, v1 = v3, v2, v1, v0
    return y.astype(np.float64)


def block_energies_of(y, sr, n_ch=None):
    """E_k = sum_c w_c sum_(block k) y_c^2 / L from the filtered channels y (C, N)"""
    C, N = y.shape
    s, nb = s100(sr), n_blocks(N, sr)
    n_ch = C if n_ch is None else n_ch
    out = np.zeros(nb)
    if not nb:
        return out
    nseg = nb + 3
    for c in range(C):
        w = channel_weight(c, n_ch)
        if w == 0.0:
            continue
        seg = (y[c, :nseg * s] ** 2).reshape(nseg, s).sum(1)
        out += w * np.array([seg[k:k + 4].sum() for k in range(nb)])
    return out / (4 * s)


def block_energies(x, sr, dtype=np.float64):
    return block_energies_of(kfilter(x, sr, dtype), sr)


BOUNDARIES = np.array([10.0 ** ((i / 10.0 - 70.0 + 0.691) / 10.0) for i in range(1001)])
ENERGIES = np.array([10.0 ** ((i / 10.0 - 69.95 + 0.691) / 10.0) for i in range(1000)])


def hist_index(e):
    """find_histogram_index: the largest j <= 999 with e >= BOUNDARIES[j]"""
    lo, hi = 0, 1000
    while hi - lo != 1:
        mid = (lo + hi) // 2
        if e >= BOUNDARIES[mid]:
            lo = mid
        else:
            hi = mid
    return lo


def gated_loudness(E):
    hist = [0] * 1000
    for e in E:
        if e >= BOUNDARIES[0]:
            hist[hist_index(e)] += 1
    rel, cnt = 0.0, 0
    for j in range(1000):
        rel += float(hist[j]) * ENERGIES[j]
        cnt += hist[j]
    if not cnt:
        return -math.inf
    rel /= float(cnt)
    rel *= 10.0 ** (-10.0 / 10.0)
    start = 0
    if not rel < BOUNDARIES[0]:
        start = hist_index(rel)
        if rel > ENERGIES[start]:
            start += 1
    s, cnt = 0.0, 0
    for j in range(start, 1000):
        s += float(hist[j]) * ENERGIES[j]
        cnt += hist[j]
    if not cnt:
        return -math.inf
    return 10.0 * math.log10(s / float(cnt)) - 0.691
