"""The waveform envelope and the waveform lane restated in numpy (include/thesia_amd.h, "Waveform envelope"): the column edges in
Python floats (C doubles), min / max by np.fmin / np.fmax, both sums by math.fsum, the zero-order hold of empty columns, and the
integer pipeline of the lane, which takes envelope floats as its input."""
import math

import numpy as np

MAX_COLS = 65536
MAX_DIM = 16384
INF = float("inf")


def edges(sr, n, start_sec, end_sec, n_cols):
    """uint64[n_cols + 1], or None where th_envelope_edges refuses"""
    if math.isnan(start_sec) or math.isnan(end_sec) or start_sec < 0.0 or math.isinf(start_sec):
        return None
    if sr <= 0 or n <= 0 or n_cols <= 0 or n_cols > MAX_COLS:
        return None
    N = float(n)

    def clamp(v):
        return 0.0 if v < 0.0 else (N if v > N else v)

    A = clamp(start_sec * float(sr))
    B = N if end_sec == INF else clamp(end_sec * float(sr))
    if not B > A:
        return None
    W = n_cols
    last = int(math.ceil(B))
    e = [min(int(math.ceil(A + (B - A) * float(j) / float(W))), last) for j in range(W)]
    e.append(last)
    return np.array(e, np.uint64)


def envelope(x, e):
    """float32 [W, 4] (min, max, mean, rms) of the f32 samples x over the edges e, and per column the mean of |x| (f64; the
    tolerance of the mean is in its units)"""
    x = np.asarray(x, np.float32)
    W = len(e) - 1
    out = np.empty((W, 4), np.float32)
    mean_abs = np.zeros(W, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(W):
            a, b = int(e[j]), int(e[j + 1])
            c = b - a
            if c == 0:
                v = x[max(a, 1) - 1]
                out[j] = (v, v, v, np.abs(v))
                mean_abs[j] = abs(float(v))
                continue
            seg = x[a:b]
            d = seg.astype(np.float64)
            if np.isfinite(d).all():
                s, q = math.fsum(d), math.fsum(d * d)   # (d * d: the rounded f64 product, as the kernel adds it)
                mean_abs[j] = math.fsum(np.abs(d)) / c
            else:
                s, q = float(np.sum(d)), float(np.sum(d * d))
                mean_abs[j] = float(np.sum(np.abs(d))) / c
            out[j] = (np.fmin.reduce(seg, initial=np.float32(INF)), np.fmax.reduce(seg, initial=np.float32(-INF)),
                      np.float32(s / c), np.float32(math.sqrt(q / c) if q == q else float("nan")))
    return out, mean_abs


def spacing32(v):
    v = np.float32(abs(v))
    return float(np.spacing(v)) if np.isfinite(v) else 0.0


def tolerances(want, mean_abs, e):
    """(tol_mean[W], tol_rms[W]): the first-order bound of an f64 sum of c terms in any order plus the one f32 rounding, doubled for
    the division and the square root; 0 for held columns"""
    W = len(e) - 1
    tm, tr = np.zeros(W), np.zeros(W)
    for j in range(W):
        c = int(e[j + 1]) - int(e[j])
        if c == 0:
            continue
        m, r = float(want[j, 2]), float(want[j, 3])
        tm[j] = spacing32(m) / 2 + c * 2.0 ** -52 * mean_abs[j] if math.isfinite(m) else 0.0
        tr[j] = spacing32(r) / 2 + c * 2.0 ** -52 * r if math.isfinite(r) else 0.0
    return tm, tr


def _row(hi, lo, v, out_h):
    top = 256.0 * out_h
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.float64(hi) - np.float64(v)
        t = t / (np.float64(hi) - np.float64(lo))
        t = t * np.float64(out_h)
        t = t * np.float64(256.0)
        t = np.floor(t + np.float64(0.5))
    if not t > 0.0:
        t = 0.0
    if t > top:
        t = top
    return int(t)


def span(col, left, out_h, amp_lo, amp_hi, thickness):
    """(y_top, y_bot) of one column, or None where it draws nothing; col, left: four f32 each (left None for column 0)"""
    col = np.asarray(col, np.float32)
    mn, mx = col[0], col[1]
    if mx < mn or col[2] != col[2]:
        return None
    if left is not None:
        left = np.asarray(left, np.float32)
        if not left[1] < left[0]:
            if mx < left[0]:
                mx = left[0]
            if mn > left[1]:
                mn = left[1]
    hi, lo = np.float32(amp_hi), np.float32(amp_lo)
    top = 256 * out_h
    yt, yb = _row(hi, lo, mx, out_h), _row(hi, lo, mn, out_h)
    if yb - yt < thickness:
        yt = (yt + yb - thickness) // 2
        yb = yt + thickness
        yt = min(max(yt, 0), top)
        yb = min(max(yb, 0), top)
    return yt, yb


def lane(env, out_h, amp_lo, amp_hi, thickness, fill, background):
    """uint8 [out_h, W, 4] from envelope floats [W, 4]"""
    env = np.asarray(env, np.float32)
    W = env.shape[0]
    yt, yb = np.zeros(W, np.int64), np.zeros(W, np.int64)
    for j in range(W):
        s = span(env[j], env[j - 1] if j > 0 else None, out_h, amp_lo, amp_hi, thickness)
        if s is not None:
            yt[j], yb[j] = s
    r = np.arange(out_h, dtype=np.int64)[:, None] * 256
    cov = np.maximum(0, np.minimum(yb[None, :], r + 256) - np.maximum(yt[None, :], r))[:, :, None]
    f = np.asarray(fill, np.int64)[None, None, :]
    b = np.asarray(background, np.int64)[None, None, :]
    return ((f * cov + b * (256 - cov) + 128) >> 8).astype(np.uint8)
