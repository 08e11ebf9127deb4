"""A literal restatement of include/thesia_amd.h "Formant candidates", steps 1 - 6, in f64 with explicit loops in the stated order
(Python floats are C doubles; no operation here is fused).  alpha, the window and the start points come from the library's host
functions, so that libm does not enter steps 1 - 5; step 6 uses math.atan2 / math.log.  Not a test module."""
import math

import numpy as np

import thesia_amd as ta

LOADING = 1.0 + 2.0 ** -30
STOP = 2.0 ** -80
MAX_SWEEPS = 64
NAN = float("nan")


def analysis_signal(x, sr, plan):
    """the whole analysis signal u (float32[n_a]): the channel, or the resampler's output at sr_analysis"""
    x = np.ascontiguousarray(x, np.float32)
    if not plan["resampled"]:
        return x
    return ta.resample_f32(x, sr, plan["sr_analysis"], 0, plan["n_analysis"])


def windowed(u, alpha, g, W, H, f):
    n_a = len(u)
    b = f * H - W // 2
    s = [0.0] * W
    for k in range(W):
        n = b + k
        if 0 <= n < n_a:
            prev = float(u[n - 1]) if n > 0 else 0.0
            d = float(u[n]) - alpha * prev
        else:
            d = 0.0
        s[k] = d * float(g[k])
    return s


def autocorr(s, W, p):
    r = [0.0] * (p + 1)
    for m in range(p + 1):
        part = [0.0] * 64
        for q in range(64):
            acc = 0.0
            for k in range(q, W - m, 64):
                acc = acc + (s[k] * s[k + m])
            part[q] = acc
        h = 32
        while h:
            for q in range(h):
                part[q] = part[q] + part[q + h]
            h >>= 1
        r[m] = part[0]
    return r


def levinson(r, p):
    """-> (status, r0', E, a[0 .. p])"""
    a = [1.0] + [0.0] * p
    r0 = r[0]
    if not math.isfinite(r0) or not r0 > 0.0:
        return 1, 0.0, 0.0, a
    r0p = r0 * LOADING
    E = r0p
    for i in range(1, p + 1):
        acc = r[i]
        for j in range(1, i):
            acc = acc + a[j] * r[i - j]
        kappa = (-acc) / E
        new = [a[j] + kappa * a[i - j] for j in range(1, i)]
        a[1:i] = new
        a[i] = kappa
        E = E * (1.0 - kappa * kappa)
        if not E > 0.0:
            return 1, 0.0, 0.0, [1.0] + [0.0] * p
    return 0, r0p, E, a


def _mul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def _div(u, v):
    n = v[0] * v[0] + v[1] * v[1]
    try:
        return ((u[0] * v[0] + u[1] * v[1]) / n, (u[1] * v[0] - u[0] * v[1]) / n)
    except ZeroDivisionError:  # (IEEE: a quotient by zero is an infinity or a NaN)
        with np.errstate(all="ignore"):
            nn = np.float64(n)
            return (float(np.float64(u[0] * v[0] + u[1] * v[1]) / nn), float(np.float64(u[1] * v[0] - u[0] * v[1]) / nn))


def aberth(a, p, z0):
    """-> (roots as a list of (re, im), sweeps, stopped)"""
    z = [(float(c.real), float(c.imag)) for c in z0]
    sweeps, stopped = 0, False
    while sweeps < MAX_SWEEPS and not stopped:
        w = []
        for i in range(p):
            zi = z[i]
            P, D = (1.0, 0.0), (0.0, 0.0)
            for k in range(1, p + 1):
                t = _mul(D, zi)
                D = (t[0] + P[0], t[1] + P[1])
                t = _mul(P, zi)
                P = (t[0] + a[k], t[1])
            q = _div(P, D)
            sigma = (0.0, 0.0)
            for j in range(p):
                if j == i:
                    continue
                t = _div((1.0, 0.0), (zi[0] - z[j][0], zi[1] - z[j][1]))
                sigma = (sigma[0] + t[0], sigma[1] + t[1])
            t = _mul(q, sigma)
            w.append(_div(q, (1.0 - t[0], 0.0 - t[1])))
        z = [(z[i][0] - w[i][0], z[i][1] - w[i][1]) for i in range(p)]
        sweeps += 1
        stopped = all((wi[0] * wi[0] + wi[1] * wi[1]) <= STOP for wi in w)
    return z, sweeps, stopped


def frame(u, plan, g, z0, f, roots=True):
    """the raw fit of frame f -> dict(r, a, r0_loaded, E, roots, sweeps, status)"""
    p, W, H = plan["n_poles"], plan["win"], plan["hop"]
    s = windowed(u, plan["alpha"], g, W, H, f)
    r = autocorr(s, W, p)
    status, r0p, E, a = levinson(r, p)
    z, sweeps = [(0.0, 0.0)] * p, 0
    if status == 0 and roots:
        z, sweeps, stopped = aberth(a, p, z0)
        if not stopped:
            status = 2
    return {"r": np.array(r), "a": np.array(a), "r0_loaded": r0p, "E": E, "roots": np.array([complex(*c) for c in z]),
            "sweeps": sweeps, "status": status}


def pack(fit, plan):
    """step 6 and the output record of one frame (2 + p doubles)"""
    p, sr_a = plan["n_poles"], float(plan["sr_analysis"])
    if fit["status"] != 0:
        return [NAN] * (2 + p)
    if plan["kind"] == ta.FORMANT_OUT_LPC:
        return [fit["r0_loaded"], fit["E"]] + [float(v) for v in fit["a"][1:]]
    found = []
    for c in fit["roots"]:
        re, im = float(c.real), float(c.imag)
        if not im > 0.0:
            continue
        fr = math.atan2(im, re) * sr_a / (2.0 * math.pi)
        bw = -math.log(re * re + im * im) * sr_a / (2.0 * math.pi)
        if 50.0 <= fr <= sr_a / 2.0 - 50.0:
            found.append((fr, bw))
    found.sort()
    found = found[:p // 2]
    pad = [NAN] * (p // 2 - len(found))
    return [float(len(found)), fit["E"] / fit["r0_loaded"]] + [c[0] for c in found] + pad + [c[1] for c in found] + pad


def formants(x, sr, req, frame0=0, n_frames=None):
    """what th_formants_f64 gives: (float64 [n_frames, 2 + p], (n_invalid, n_unconverged))"""
    plan = ta.formant_plan(sr, len(x), req)
    u = analysis_signal(x, sr, plan)
    g, z0 = ta.formant_window(plan["window"], plan["win"]), ta.formant_start_points(plan["n_poles"])
    if n_frames is None:
        n_frames = plan["n_frames_total"] - frame0
    out = np.empty((n_frames, 2 + plan["n_poles"]))
    bad = unconv = 0
    for i in range(n_frames):
        fit = frame(u, plan, g, z0, frame0 + i, roots=plan["kind"] == ta.FORMANT_OUT_FORMANTS)
        bad += fit["status"] != 0
        unconv += fit["status"] == 2
        out[i] = pack(fit, plan)
    return out, (bad, unconv)
