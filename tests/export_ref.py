"""The PCM / WAV export's definitions (include/thesia_amd.h, "PCM / WAV export of resident tracks") restated in numpy: the sample
range, the counter-based dither generator, the quantiser, the interleave and the WAV header.  Integer and f64 arithmetic only.
Nothing here calls the library: the tests compare it with this."""
import math
import struct

import numpy as np

PCM_S16, PCM_S24, PCM_F32 = 0, 1, 2
DITHER_NONE, DITHER_TPDF = 0, 1
INF = float("inf")
SCALE = {PCM_S16: 32768, PCM_S24: 8388608}
BYTES = {PCM_S16: 2, PCM_S24: 3, PCM_F32: 4}
M32 = np.uint64(0xFFFFFFFF)


def sample_range(sr, n, start_sec=0.0, end_sec=INF):
    """[s0, s1): Python floats are C doubles"""
    clamp = lambda x: n if x >= n else int(x)  # noqa: E731  (x >= 0)
    s0 = clamp(math.ceil(start_sec * sr))
    s1 = n if end_sec == INF else max(s0, clamp(math.ceil(end_sec * sr)))
    return s0, s1


def fmix32(h):
    """h: uint64 array holding 32-bit values -> the same"""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & M32
    return h ^ (h >> np.uint64(16))


def dither(seed, ch, i):
    """-> (a, b), uint64 arrays of 24-bit values; seed, ch, i broadcast (i: ABSOLUTE sample indices)"""
    seed, ch, i = (np.asarray(v, dtype=np.uint64) for v in (seed, ch, i))
    k0 = fmix32((seed + np.uint64(0x9E3779B9) * ((ch + np.uint64(1)) & M32)) & M32)
    k1 = fmix32((i >> np.uint64(32)) ^ k0)
    k = fmix32((i & M32) ^ k1)
    return fmix32(k ^ np.uint64(0x68BC21EB)) >> np.uint64(8), fmix32(k ^ np.uint64(0x02E5BE93)) >> np.uint64(8)


def quantize(fmt, dith, seed, ch, first_index, x):
    """one channel -> (int64 q, n_clamped, n_nan)"""
    x = np.asarray(x, dtype=np.float32)
    S = SCALE[fmt]
    v = x.astype(np.float64) * float(S)  # exact
    if dith == DITHER_TPDF:
        a, b = dither(seed, ch, np.uint64(first_index) + np.arange(x.size, dtype=np.uint64))
        v += (a.astype(np.float64) - b.astype(np.float64)) * 2.0 ** -24
    nan = np.isnan(x)
    q = np.rint(v)  # ties to even; NaN stays NaN, and compares false below
    with np.errstate(invalid="ignore"):
        clamped = (q > S - 1) | (q < -S)
    q = np.clip(q, -S, S - 1)
    q[nan] = 0.0
    return q.astype(np.int64), int(clamped.sum()), int(nan.sum())


def pcm_bytes(fmt, dith, seed, chans, s0, s1):
    """chans: [n_ch][n] f32, the WHOLE track -> (uint8 bytes of frames [s0, s1) interleaved, n_clamped, n_nan)"""
    chans = np.asarray(chans, dtype=np.float32)
    n_ch, nf = chans.shape[0], s1 - s0
    if fmt == PCM_F32:
        out = np.ascontiguousarray(chans[:, s0:s1].T).view(np.uint8).reshape(-1)
        return out.copy(), 0, int(np.isnan(chans[:, s0:s1]).sum())
    bps = BYTES[fmt]
    out = np.empty((nf, n_ch, bps), np.uint8)
    n_clamped = n_nan = 0
    for c in range(n_ch):
        q, nc, nn = quantize(fmt, dith, seed, c, s0, chans[c, s0:s1])
        n_clamped += nc
        n_nan += nn
        out[:, c, :] = (q & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :bps]  # little-endian, the low bytes
    return out.reshape(-1), n_clamped, n_nan


def wav_header(fmt, sr, n_ch, n_frames):
    """-> (header bytes, pad_len), or the name of the refusal: "invalid" / "unsupported" """
    if n_ch == 0 or sr == 0 or fmt not in BYTES:
        return "invalid"
    bps = BYTES[fmt]
    block, rate = n_ch * bps, n_ch * bps * sr
    data = n_frames * block
    pad = data & 1
    hl = 58 if fmt == PCM_F32 else 44
    if n_ch > 65535 or block > 65535 or rate > 0xFFFFFFFF or hl - 8 + data + pad > 0xFFFFFFFF:
        return "unsupported"
    h = b"RIFF" + struct.pack("<I", hl - 8 + data + pad) + b"WAVEfmt "
    if fmt == PCM_F32:
        h += struct.pack("<IHHIIHHH", 18, 3, n_ch, sr, rate, block, 32, 0) + b"fact" + struct.pack("<II", 4, n_frames)
    else:
        h += struct.pack("<IHHIIHH", 16, 1, n_ch, sr, rate, block, 8 * bps)
    h += b"data" + struct.pack("<I", data)
    assert len(h) == hl
    return h, pad


def wav_file(fmt, dith, seed, sr, chans, s0, s1):
    """the complete file image: header + data + pad"""
    data, _, _ = pcm_bytes(fmt, dith, seed, chans, s0, s1)
    h, pad = wav_header(fmt, sr, np.asarray(chans).shape[0], s1 - s0)
    return h + data.tobytes() + b"\0" * pad
