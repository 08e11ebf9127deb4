"""Restatement of the loudness meter's definitions (include/thesia_amd.h, "loudness meter of resident tracks") for the tests: the
true-peak interpolator's taps and its FIR in f64 with f32-rounded coefficients, the momentary / short-term energies from
loudness_ref.kfilter, LUFS, and the EBU Tech 3342 loudness range in libebur128's histogram mode.
Test infrastructure only: the product never imports it."""
import math

import numpy as np

from tests import loudness_ref as ref

# the largest sum of |c| over a phase's taps (f64 taps; checked in test_loudness_meter_host.py) and the taps of a phase
PHASE_GAIN = {4: 1.8642, 2: 2.3068}
PHASE_TAPS = {4: 12, 2: 24}


def factor(sr):
    return 4 if sr < 96000 else 2 if sr < 192000 else 1


def true_peak_filter(sr):
    """-> (F, coef f64, phase, delay): the kept taps in ascending j"""
    F = factor(sr)
    coef, phase, delay = [], [], []
    for j in range(49):
        m = float(j) - 24.0
        t = m * math.pi / float(F)
        sinc = 1.0 if m == 0.0 else math.sin(t) / t
        c = sinc * (0.5 * (1.0 - math.cos(2.0 * math.pi * float(j) / 48.0)))
        if not abs(c) > 1e-6:
            continue
        coef.append(c)
        phase.append(j % F)
        delay.append(j // F)
    return F, np.array(coef), np.array(phase, np.uint32), np.array(delay, np.uint32)


def phase_filters(sr):
    """-> [h_f]: per phase the f32-rounded taps as f64, indexed by delay"""
    F, coef, phase, delay = true_peak_filter(sr)
    out = []
    for f in range(F):
        h = np.zeros(int(delay[phase == f].max()) + 1)
        h[delay[phase == f]] = coef[phase == f].astype(np.float32).astype(np.float64)
        out.append(h)
    return out


def _nanmax0(a):
    return float(np.nanmax(a)) if a.size and not np.all(np.isnan(a)) else 0.0


def true_peaks(x, sr):
    """x (C, N) f32 -> per channel the largest |y_f[i]|, i in [0, N), of the causal polyphase FIR evaluated in f64 with the
    coefficients rounded to f32; NaN outputs are ignored (0 when there is nothing else).  F = 1: the largest |x|."""
    x = np.atleast_2d(np.asarray(x, np.float32))
    hs = phase_filters(sr)
    peaks = []
    for c in range(x.shape[0]):
        xc = x[c].astype(np.float64)
        if len(hs) == 1:
            peaks.append(_nanmax0(np.abs(xc)))
            continue
        with np.errstate(invalid="ignore"):
            peaks.append(max([_nanmax0(np.abs(_causal_fir(xc, h))) for h in hs] + [0.0]))
    return peaks


def true_peak(x, sr):
    """-> (peak, the lowest channel that attains it)"""
    peaks = true_peaks(x, sr)
    best = max(peaks) if peaks else 0.0
    return best, (peaks.index(best) if peaks else 0)


def _causal_fir(x, h):
    """y[i] = sum_d h[d] x[i - d], i < len(x), x[i < 0] = 0; a NaN sample makes NaN of the outputs it reaches only (np.convolve
    would too, but 0 * inf must not appear: the samples are finite or NaN here)"""
    n = x.size
    y = np.zeros(n)
    for d in np.flatnonzero(h):
        if d < n:
            y[d:] += h[d] * x[:n - d]
    return y


def true_peak_bar(x, sr):
    """(T + 1) 2^-24 S max|x|: the worst case of a T-term f32 fmaf chain (T roundings of at most 2^-24 of the partial sums, each at
    most S max|x|) plus the coefficients' rounding to f32 (2^-24 S max|x|)"""
    F = factor(sr)
    if F == 1:
        return 0.0
    a = np.abs(np.asarray(x, np.float64))
    mx = float(np.nanmax(a)) if a.size and not np.all(np.isnan(a)) else 0.0
    return (PHASE_TAPS[F] + 1) * 2.0 ** -24 * PHASE_GAIN[F] * mx


def n_short_term(n, sr):
    nseg = n // ref.s100(sr)
    return 0 if nseg < 30 else nseg - 29


def kfilter_fast(x, sr, dtype=np.float64, piece_sec=0.25):
    """loudness_ref.kfilter over pieces of piece_sec that run side by side, each from zero state piece_sec before its first sample
    (the first from the true zero state).  The K-weighting's slowest pole is the 38 Hz high-pass: what a piece misses of the true
    state has decayed by about exp(-2 pi 38 piece_sec) = 1e-26 of it, far below the rounding of either precision, so the result is the
    sequential filter's up to its own rounding noise (test_loudness_meter_host.py compares the two).  Finite samples only: a NaN
    stays in the sequential filter's state for good, and here it would end with its piece."""
    x = np.atleast_2d(np.asarray(x, np.float32))
    C, N = x.shape
    p = max(1, int(math.ceil(piece_sec * sr)))
    if N <= 2 * p:
        return ref.kfilter(x, sr, dtype)
    J = max(1, -(-N // p))
    pad = np.zeros((C, p + J * p), np.float32)
    pad[:, p:p + N] = x
    rows = np.stack([pad[c, j * p:(j + 2) * p] for c in range(C) for j in range(J)])
    y = ref.kfilter(rows, sr, dtype)[:, p:]
    return y.reshape(C, J * p)[:, :N]


def series_energies_of(y, sr, span, n_ch=None):
    """E_k = sum_c w_c (the energies of segments k .. k + span - 1) / (span s100) from the filtered channels y (C, N)"""
    C, N = y.shape
    s = ref.s100(sr)
    nseg = N // s
    nb = max(0, nseg - span + 1)
    n_ch = C if n_ch is None else n_ch
    out = np.zeros(nb)
    if not nb:
        return out
    for c in range(C):
        w = ref.channel_weight(c, n_ch)
        if w == 0.0:
            continue
        seg = (y[c, :nseg * s] ** 2).reshape(nseg, s).sum(1)
        out += w * np.array([seg[k:k + span].sum() for k in range(nb)])
    return out / (span * s)


def lufs(E):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(np.asarray(E, np.float64)) - 0.691


def energy(L):
    return 10.0 ** ((np.asarray(L, np.float64) + 0.691) / 10.0)


def series_max(L):
    L = np.asarray(L, np.float64)
    L = L[~np.isnan(L)]
    return float(L.max()) if L.size else -math.inf


def loudness_range(E):
    """the header's steps 1-8 on the short-term energies taken once per second"""
    hist = [0] * 1000
    for e in E:
        if e >= ref.BOUNDARIES[0]:
            hist[ref.hist_index(e)] += 1
    size, power = 0, 0.0
    for j in range(1000):
        size += hist[j]
        power += float(hist[j]) * ref.ENERGIES[j]
    if not size:
        return 0.0
    power /= float(size)
    integ = 0.01 * power
    idx = 0
    if not integ < ref.BOUNDARIES[0]:
        idx = ref.hist_index(integ)
        if integ > ref.ENERGIES[idx]:
            idx += 1
    size = sum(hist[idx:])
    if not size:
        return 0.0
    lo, hi = int(float(size - 1) * 0.1 + 0.5), int(float(size - 1) * 0.95 + 0.5)
    cnt, j = 0, idx
    while cnt <= lo:
        cnt += hist[j]
        j += 1
    l = ref.ENERGIES[j - 1]
    while cnt <= hi:
        cnt += hist[j]
        j += 1
    h = ref.ENERGIES[j - 1]
    return 10.0 * math.log10(h) - 10.0 * math.log10(l)


def meter(x, sr, dtype=np.float64, sequential=False):
    """the whole meter of one track x (C, N) f32 from the restatement: dict with the energies, LUFS series and summary numbers
    (sequential: loudness_ref.kfilter itself, for audio that holds a NaN)"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    if x.shape[1] < 4 * ref.s100(sr):
        y = np.zeros(x.shape)  # (no block: nothing reads it)
    else:
        y = ref.kfilter(x, sr, dtype) if sequential else kfilter_fast(x, sr, dtype)
    em, es = series_energies_of(y, sr, 4), series_energies_of(y, sr, 30)
    pk, ch = true_peak(x, sr)
    return {"e_momentary": em, "e_short_term": es, "momentary": lufs(em), "short_term": lufs(es), "loudness_range": loudness_range(es[::10]),
            "max_momentary_lufs": series_max(lufs(em)), "max_short_term_lufs": series_max(lufs(es)), "true_peak": pk,
            "true_peak_channel": ch, "oversampling": factor(sr)}
