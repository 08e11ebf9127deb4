"""A strict pure-Python FLAC decoder (RFC 9639) and a numpy model of the export encoder's decisions (include/thesia_amd.h, "FLAC
export").  The decoder handles every subframe type, both Rice coding methods, escape partitions, wasted bits and all four channel
assignments; it checks the sync code, the reserved bits, CRC-8 and CRC-16, and returns each subframe's type, order, partition order
and parameters.  The model makes the decisions (type, order, p, k, bit counts), not the bit packing.  Test scaffolding only."""
import numpy as np


class FlacError(ValueError):
    pass


def _need(cond, what):
    if not cond:
        raise FlacError(what)


class _Bits:
    def __init__(self, data, pos):
        self.b, self.p = data, pos * 8

    def u(self, n):
        if n == 0:
            return 0
        p, e = self.p, self.p + n
        _need(e <= len(self.b) * 8, "the stream ends inside a frame")
        b1 = (e + 7) >> 3
        v = int.from_bytes(self.b[p >> 3:b1], "big")
        self.p = e
        return (v >> (b1 * 8 - e)) & ((1 << n) - 1)

    def s(self, n):
        v = self.u(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self):
        n = 0
        while True:
            left = len(self.b) * 8 - self.p
            _need(left > 0, "the stream ends inside a unary run")
            w = min(64, left)
            v = self.u(w)
            if v:
                lead = w - v.bit_length()
                self.p -= w - lead - 1
                return n + lead
            n += w


def crc8(d):
    c = 0
    for x in d:
        c ^= x
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_T16 = []
for _i in range(256):
    _c = _i << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _T16.append(_c)


def crc16(d):
    c = 0
    for x in d:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ x]
    return c


_FIXED = [[], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1]]
_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
_SIZES = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}


def _residual(br, bs, order, info):
    m = br.u(2)
    _need(m < 2, "reserved residual coding method")
    pb = 4 if m == 0 else 5
    po = br.u(4)
    _need(bs % (1 << po) == 0 and (bs >> po) >= order, "partition order %d does not fit a block of %d" % (po, bs))
    info.update(method=m, p=po, params=[])
    out = []
    for part in range(1 << po):
        n = (bs >> po) - (order if part == 0 else 0)
        k = br.u(pb)
        if k == (1 << pb) - 1:
            nb = br.u(5)
            info["params"].append(("escape", nb))
            out += [br.s(nb) if nb else 0 for _ in range(n)]
        else:
            info["params"].append(k)
            for _ in range(n):
                u = (br.unary() << k) | br.u(k)
                out.append((u >> 1) ^ -(u & 1))
    return out


def _subframe(br, bs, bps):
    _need(br.u(1) == 0, "subframe padding bit set")
    t = br.u(6)
    wasted = 0
    if br.u(1):
        wasted = br.unary() + 1
        bps -= wasted
        _need(bps > 0, "wasted bits leave no sample bits")
    info = {"wasted": wasted}
    if t == 0:
        info.update(type="constant", order=0)
        s = [br.s(bps)] * bs
    elif t == 1:
        info.update(type="verbatim", order=0)
        s = [br.s(bps) for _ in range(bs)]
    elif 8 <= t <= 12:
        o = t - 8
        _need(o <= bs, "predictor order above the block size")
        info.update(type="fixed", order=o)
        s = [br.s(bps) for _ in range(o)]
        c = _FIXED[o]
        for e in _residual(br, bs, o, info):
            s.append(e + sum(c[i] * s[-1 - i] for i in range(o)))
    elif t >= 32:
        o = t - 31
        _need(o <= bs, "predictor order above the block size")
        info.update(type="lpc", order=o)
        s = [br.s(bps) for _ in range(o)]
        prec = br.u(4)
        _need(prec != 15, "reserved coefficient precision")
        prec += 1
        shift = br.s(5)
        _need(shift >= 0, "negative predictor shift")
        c = [br.s(prec) for _ in range(o)]
        for e in _residual(br, bs, o, info):
            s.append(e + (sum(c[i] * s[-1 - i] for i in range(o)) >> shift))
    else:
        raise FlacError("reserved subframe type %d" % t)
    return ([x << wasted for x in s] if wasted else s), info


def decode(data, max_frames=None):
    """-> dict: the STREAMINFO fields, channels (n_ch lists of ints), frames (number, block, header_len, size, subframes)"""
    data = bytes(data)
    _need(data[:4] == b"fLaC", "no fLaC marker")
    pos, si = 4, None
    while True:
        _need(pos + 4 <= len(data), "the stream ends inside the metadata")
        h, ln = data[pos], int.from_bytes(data[pos + 1:pos + 4], "big")
        if h & 0x7F == 0:
            _need(ln == 34 and si is None, "bad STREAMINFO")
            si = data[pos + 4:pos + 4 + ln]
        _need((h & 0x7F) != 127, "reserved metadata block type")
        pos += 4 + ln
        if h & 0x80:
            break
    _need(si is not None, "no STREAMINFO")
    x = int.from_bytes(si[10:18], "big")
    out = {"min_block": int.from_bytes(si[0:2], "big"), "max_block": int.from_bytes(si[2:4], "big"),
           "min_frame": int.from_bytes(si[4:7], "big"), "max_frame": int.from_bytes(si[7:10], "big"),
           "sr": x >> 44, "n_ch": ((x >> 41) & 7) + 1, "bps": ((x >> 36) & 31) + 1, "total": x & ((1 << 36) - 1), "md5": si[18:34],
           "first_frame": pos, "frames": []}
    n_ch, bps_s = out["n_ch"], out["bps"]
    chans = [[] for _ in range(n_ch)]
    while pos < len(data) and (max_frames is None or len(out["frames"]) < max_frames):
        start, br = pos, _Bits(data, pos)
        _need(br.u(15) == 0x7FFC, "no sync code at byte %d" % pos)
        variable = br.u(1)
        bsc, src, ca, ssc = br.u(4), br.u(4), br.u(4), br.u(3)
        _need(br.u(1) == 0, "reserved header bit set")
        _need(bsc != 0 and src != 15 and ca <= 10 and ssc not in (3,), "reserved header code")
        first = br.u(8)
        nb = 0
        while first & (0x80 >> nb):
            nb += 1
        _need(nb != 1 and nb <= 7, "bad coded number")
        number = first & (0x7F >> nb) if nb else first
        for _ in range(max(nb - 1, 0)):
            c = br.u(8)
            _need(c >> 6 == 2, "bad continuation byte in the coded number")
            number = (number << 6) | (c & 0x3F)
        if bsc == 6:
            bs = br.u(8) + 1
        elif bsc == 7:
            bs = br.u(16) + 1
        elif bsc == 1:
            bs = 192
        elif 2 <= bsc <= 5:
            bs = 576 << (bsc - 2)
        else:
            bs = 256 << (bsc - 8)
        if src == 12:
            sr = br.u(8) * 1000
        elif src == 13:
            sr = br.u(16)
        elif src == 14:
            sr = br.u(16) * 10
        else:
            sr = _RATES.get(src, out["sr"])
        _need(sr == out["sr"], "frame rate %d against STREAMINFO's %d" % (sr, out["sr"]))
        bps = _SIZES.get(ssc, bps_s)
        _need(bps == bps_s, "frame sample size against STREAMINFO's")
        hl = (br.p >> 3) - start
        _need(br.u(8) == crc8(data[start:start + hl]), "CRC-8 of frame %d" % len(out["frames"]))
        nch = ca + 1 if ca < 8 else 2
        _need(nch == n_ch, "frame channels against STREAMINFO's")
        subs, sig = [], []
        for c in range(nch):
            side = (ca == 8 and c == 1) or (ca == 9 and c == 0) or (ca == 10 and c == 1)
            s, info = _subframe(br, bs, bps + (1 if side else 0))
            sig.append(s)
            subs.append(info)
        if ca == 8:
            sig[1] = [a - b for a, b in zip(sig[0], sig[1])]
        elif ca == 9:
            sig[0] = [a + b for a, b in zip(sig[0], sig[1])]
        elif ca == 10:
            mid = [(m << 1) | (s & 1) for m, s in zip(sig[0], sig[1])]
            sig = [[(m + s) >> 1 for m, s in zip(mid, sig[1])], [(m - s) >> 1 for m, s in zip(mid, sig[1])]]
        pad = (-br.p) % 8
        _need(br.u(pad) == 0, "padding bits set")
        end = br.p >> 3
        _need(br.u(16) == crc16(data[start:end]), "CRC-16 of frame %d" % len(out["frames"]))
        pos = end + 2
        for c in range(nch):
            chans[c] += sig[c]
        out["frames"].append({"number": number, "variable": variable, "block": bs, "header_len": hl + 1, "size": pos - start, "subframes": subs})
    out["channels"] = chans
    return out


def pcm_bytes(dec):
    """the decoded channels as interleaved little-endian PCM of the stream's sample size"""
    a = np.array(dec["channels"], np.int64).reshape(dec["n_ch"], -1).T.reshape(-1)
    nb = dec["bps"] // 8
    raw = (a & ((1 << dec["bps"]) - 1)).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :nb]
    return raw.tobytes()


# ------------------------------------------------------------------------------------------------ the encoder's decisions
BLOCK = 4096


def part_order(n):
    p = 0
    while p < 6 and n % (2 << p) == 0 and (n >> (p + 1)) >= 5:
        p += 1
    return p


def model_subframe(s, bps):
    """one channel of one block -> dict(type, order, p, params, bits): bits is the whole subframe, header included"""
    s = np.asarray(s, np.int64)
    n = s.size
    if np.all(s == s[0]):
        return {"type": "constant", "order": 0, "bits": 8 + bps}
    verbatim = {"type": "verbatim", "order": 0, "bits": 8 + n * bps}
    if n < 5:
        return verbatim
    p, kmax, pb = part_order(n), (14 if bps == 16 else 30), (4 if bps == 16 else 5)
    psz, ks = n >> p, np.arange(kmax + 1, dtype=np.int64)
    best = None
    for o in range(5):
        e = np.diff(s, o) if o else s
        u = (e << 1) ^ (e >> 63)
        cost, params, at = o * bps + 6, [], 0
        for q in range(1 << p):
            m = psz - (o if q == 0 else 0)
            part = u[at:at + m]
            at += m
            c = (part[None, :] >> ks[:, None]).sum(axis=1) + m * (ks + 1)
            k = int(np.argmin(c))  # (the first of the smallest)
            params.append(k)
            cost += pb + int(c[k])
        if best is None or cost < best[0]:
            best = (cost, o, params)
    if best[0] >= n * bps:
        return verbatim
    return {"type": "fixed", "order": best[1], "p": p, "params": best[2], "bits": 8 + best[0]}


_TABLE_RATES = {v: k for k, v in _RATES.items()}


def header_len(sr, number, n):
    nb = 1 if number < 0x80 else 2 if number < 0x800 else 3 if number < 0x10000 else 4 if number < 0x200000 else 5 if number < 0x4000000 else 6 if number < 0x80000000 else 7
    rate = 0 if sr in _TABLE_RATES else 2 if sr <= 65535 or (sr % 10 == 0 and sr // 10 <= 65535) else 0
    return 4 + nb + (0 if n == BLOCK else 1 if n <= 256 else 2) + rate + 1


def model_stream(chans, bps, sr):
    """chans (n_ch, n) -> (file length, per frame the list of the subframes' decisions, the frames' sizes)"""
    chans = np.asarray(chans, np.int64).reshape(len(chans), -1)
    n_ch, n = chans.shape
    total, frames, sizes = 42, [], []
    for b in range((n + BLOCK - 1) // BLOCK):
        blk = chans[:, b * BLOCK:(b + 1) * BLOCK]
        subs = [model_subframe(blk[c], bps) for c in range(n_ch)]
        size = header_len(sr, b, blk.shape[1]) + (sum(x["bits"] for x in subs) + 7) // 8 + 2
        frames.append(subs)
        sizes.append(size)
        total += size
    return total, frames, sizes


def bound(n, n_ch, bps):
    """th_flac_bound's formula"""
    full, rest = divmod(n, BLOCK)
    fb = lambda m: 16 + n_ch * (1 + m * (bps // 8)) + 1 + 2
    return 42 + full * fb(BLOCK) + (fb(rest) if rest else 0)


def same_decisions(dec_sub, model_sub):
    """a decoded subframe's info against the model's"""
    if dec_sub["type"] != model_sub["type"] or dec_sub["order"] != model_sub["order"] or dec_sub["wasted"] != 0:
        return False
    if model_sub["type"] != "fixed":
        return True
    return dec_sub["p"] == model_sub["p"] and dec_sub["params"] == model_sub["params"]
