"""The model of the decisions of the FLAC export's _ex entries (include/thesia_amd.h: TH_FLAC_LPC, TH_FLAC_STEREO), beside
tests/flac_ref.py, whose decoder and flags == 0 model it extends by import.  The LPC fit's f64 part (Levinson-Durbin, the coefficient
quantiser) is pure Python floats, which are the same IEEE doubles in the same order as flac_core.h, so the coefficients must be the
library's bit for bit; the integer parts (window, autocorrelation, residuals, Rice costs) are exact int64 numpy.  Test scaffolding."""
import math

import numpy as np

from tests import flac_ref as F

LPC, STEREO = 1, 2
MAX_ORDER = 8
ASSIGN = {1: (0, 1), 8: (0, 3), 9: (3, 1), 10: (2, 3)}  # the assignment code -> which of L R M S are the frame's two subframes


def decode(data):
    """flac_ref.decode, and: of every LPC subframe precision, shift and coefs; of every frame the channel assignment's four bits"""
    data = bytes(data)
    plain = F._subframe

    def subframe(br, bs, bps):
        start = br.p
        s, info = plain(br, bs, bps)
        if info["type"] == "lpc" and info["wasted"] == 0:
            b = F._Bits(br.b, 0)
            b.p = start + 8 + info["order"] * bps
            prec = b.u(4) + 1
            info.update(precision=prec, shift=b.s(5), coefs=[b.s(prec) for _ in range(info["order"])])
        return s, info

    F._subframe = subframe
    try:
        dec = F.decode(data)
    finally:
        F._subframe = plain
    at = dec["first_frame"]
    for f in dec["frames"]:
        f["assign"] = data[at + 3] >> 4
        at += f["size"]
    return dec


def part_order(n, order):
    least, p = max(5, order + 1), 0
    while p < 6 and n % (2 << p) == 0 and (n >> (p + 1)) >= least:
        p += 1
    return p


def quantize(a, P):
    """order m's coefficients -> (q, shift), or None where the order is no candidate"""
    if not all(math.isfinite(v) for v in a):
        return None
    cmax = max(abs(v) for v in a)
    if not cmax > 0.0:
        return None
    shift = min(P - math.frexp(cmax)[1] - 1, 15)
    if shift < 0:
        return None
    scale, hi, lo = float(1 << shift), (1 << (P - 1)) - 1, -(1 << (P - 1))
    fb, q = 0.0, []
    for v in a:
        fb = fb + v * scale
        t = max(lo, min(hi, math.floor(fb + 0.5)))
        q.append(t)
        fb = fb - t
    return q, shift


def lpc_fit(s, P):
    """a block's samples (int64 array) -> {order: (q, shift)}"""
    n = s.size
    i = np.arange(n, dtype=np.int64)
    w = (((2 * i + 1) * (2 * n - 2 * i - 1)) << 14) // (n * n)
    sh = max(0, int(np.abs(s).max()).bit_length() - 8)
    x = (s * w) >> sh
    assert int(np.abs(x).max()) < 1 << 22
    r = [int(np.dot(x[:n - m], x[m:])) for m in range(min(MAX_ORDER, n - 1) + 1)]
    if r[0] == 0:
        return {}
    E, a, out = float(r[0]), [], {}
    for m in range(1, len(r)):
        acc = float(r[m])
        for j in range(1, m):
            acc = acc - a[j - 1] * float(r[m - j])
        k = acc / E
        a = [a[j - 1] - k * a[m - j - 1] for j in range(1, m)] + [k]
        E = E * (1.0 - k * k)
        if not E > 0.0 or not math.isfinite(E):
            break
        qs = quantize(a, P)
        if qs is not None:
            out[m] = qs
    return out


def _rice(e, n, order, p, fbps):
    """the residuals' partitions -> (bits with the parameters', the parameters)"""
    kmax, pb = (14, 4) if fbps == 16 else (30, 5)
    ks = np.arange(kmax + 1, dtype=np.int64)
    u = (e << 1) ^ (e >> 63)
    bits, params, at = 0, [], 0
    for q in range(1 << p):
        m = (n >> p) - (order if q == 0 else 0)
        part = u[at:at + m]
        at += m
        c = (part[None, :] >> ks[:, None]).sum(axis=1) + m * (ks + 1)
        k = int(np.argmin(c))  # (the first of the smallest)
        params.append(k)
        bits += pb + int(c[k])
    return bits, params


def model_subframe(s, bps, fbps, lpc):
    """one coded channel of one block, samples of bps bits in a file of fbps bits -> the decision (bits: the whole subframe)"""
    s = np.asarray(s, np.int64)
    n = s.size
    if not lpc and bps == fbps:
        return F.model_subframe(s, bps)
    if np.all(s == s[0]):
        return {"type": "constant", "order": 0, "bits": 8 + bps}
    verbatim = {"type": "verbatim", "order": 0, "bits": 8 + n * bps}
    if n < 5:
        return verbatim
    best = None
    for o in range(5):
        p = part_order(n, o)
        bits, params = _rice(np.diff(s, o) if o else s, n, o, p, fbps)
        cost = o * bps + 6 + bits
        if best is None or cost < best[0]:
            best = (cost, {"type": "fixed", "order": o, "p": p, "params": params})
    if lpc:
        P = 12 if fbps == 16 else 14
        for m, (q, shift) in sorted(lpc_fit(s, P).items()):
            pred = np.zeros(n - m, np.int64)
            for j in range(1, m + 1):
                pred += q[j - 1] * s[m - j:n - j]
            e = s[m:] - (pred >> shift)
            if int(np.abs(e).max()) > (1 << 31) - 1:
                continue
            p = part_order(n, m)
            bits, params = _rice(e, n, m, p, fbps)
            cost = m * bps + 4 + 5 + m * P + 6 + bits
            if cost < best[0]:
                best = (cost, {"type": "lpc", "order": m, "p": p, "params": params, "precision": P, "shift": shift, "coefs": q})
    if best[0] >= n * bps:
        return verbatim
    return dict(best[1], bits=8 + best[0])


def model_frame(blk, bps, flags):
    """(n_ch, n) -> (the assignment code, the decisions of the frame's subframes in stream order)"""
    lpc = bool(flags & LPC)
    if blk.shape[0] == 2 and flags & STEREO:
        left, right = blk[0], blk[1]
        four = [model_subframe(left, bps, bps, lpc), model_subframe(right, bps, bps, lpc), model_subframe((left + right) >> 1, bps, bps, lpc),
                model_subframe(left - right, bps + 1, bps, lpc)]
        code = min(ASSIGN, key=lambda c: (sum(four[u]["bits"] for u in ASSIGN[c]), list(ASSIGN).index(c)))
        return code, [four[u] for u in ASSIGN[code]]
    return blk.shape[0] - 1, [model_subframe(blk[c], bps, bps, lpc) for c in range(blk.shape[0])]


def model_stream(chans, bps, sr, flags):
    """chans (n_ch, n) -> (file length, per frame (assignment, the subframes' decisions), the frames' sizes)"""
    chans = np.asarray(chans, np.int64).reshape(len(chans), -1)
    n = chans.shape[1]
    total, frames, sizes = 42, [], []
    for b in range((n + F.BLOCK - 1) // F.BLOCK):
        blk = chans[:, b * F.BLOCK:(b + 1) * F.BLOCK]
        code, subs = model_frame(blk, bps, flags)
        size = F.header_len(sr, b, blk.shape[1]) + (sum(x["bits"] for x in subs) + 7) // 8 + 2
        frames.append((code, subs))
        sizes.append(size)
        total += size
    return total, frames, sizes


def same_decisions(dec_sub, model_sub):
    """a decoded subframe's info (of this module's decode) against the model's"""
    if model_sub["type"] != "lpc":
        return F.same_decisions(dec_sub, model_sub)
    return all(dec_sub.get(key) == model_sub[key] for key in ("type", "order", "p", "params", "precision", "shift", "coefs")) and dec_sub["wasted"] == 0
