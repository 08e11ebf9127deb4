"""The host side of the PCM / WAV export (th_audio_sample_range, th_export_dither, th_export_quantize, th_wav_header) against the
definitions restated in numpy (tests/export_ref.py), the interface of th_tm_export_pcm / th_tm_export_wav and their th_tmg twins,
and the known answers of the dither generator.  CPU only.

Dither statistics over i = 0 .. 2^20 - 1 of d = (a - b) 2^-24 for (seed, ch) = (0, 0), (0, 1), (12345, 0).  The definition itself
gives (numpy): |mean| <= 5.7e-4, variance within 0.18 % of 1 / 6, |lag-1 correlation| <= 1.8e-3, |corr(a, b)| <= 2.2e-3; the bounds
asserted are 2 - 3 times those: 2e-3, 1 %, 5e-3, 5e-3."""
import ctypes as C
import io
import os
import re
import struct
import wave

import numpy as np
import pytest

from tests import export_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
SYMS = ["th_audio_sample_range", "th_export_dither", "th_export_quantize", "th_wav_header", "th_tm_export_pcm", "th_tm_export_wav",
        "th_tmg_export_pcm", "th_tmg_export_wav"]


def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"TH_API\s+[\w\s\*]+?\b(th_\w+)\s*\(", txt))


def test_symbols_are_declared_exported_and_bound():
    import thesia_amd
    from thesia_amd import _ffi, api
    assert set(SYMS) <= _declared("thesia_amd.h")
    assert not set(SYMS) & _declared("thesia_amd_testing.h")
    lib = C.CDLL(thesia_amd.LIB_PATH)
    assert all(hasattr(lib, s) for s in SYMS), [s for s in SYMS if not hasattr(lib, s)]
    assert set(SYMS) <= set(_ffi._SIGS)
    assert (api.PCM_S16, api.PCM_S24, api.PCM_F32, api.DITHER_NONE, api.DITHER_TPDF) == (0, 1, 2, 0, 1)
    assert (R.PCM_S16, R.PCM_S24, R.PCM_F32, R.DITHER_NONE, R.DITHER_TPDF) == (0, 1, 2, 0, 1)
    for name in ("export_pcm", "export_wav"):
        assert _ffi._SIGS["th_tmg_" + name][1:] == _ffi._SIGS["th_tm_" + name][1:], name
        for cls in (thesia_amd.TrackManager, thesia_amd.MultiTrackManager):
            assert callable(getattr(cls, name))
    hdr = open(os.path.join(ROOT, "include", "thesia_amd.h")).read()
    assert re.search(r"#define TH_EXPORT_PIECE_BYTES \(32u << 20\)", hdr) and api.EXPORT_PIECE_BYTES == 32 << 20
    assert re.search(r"#define TH_WAV_HEADER_MAX 64\b", hdr) and api.WAV_HEADER_MAX == 64
    assert re.search(r"#define TH_EXPORT_MAX_CHANNELS 1024\b", hdr) and api.EXPORT_MAX_CHANNELS == 1024


def test_struct_layouts_match_the_header():
    from thesia_amd import _ffi
    assert C.sizeof(_ffi.ExportRequest) == 40 and _ffi.ExportRequest.start_sec.offset == 24
    assert C.sizeof(_ffi.ExportInfo) == 64 and _ffi.ExportInfo.n_clamped.offset == 40 and _ffi.ExportInfo.waveform_revision.offset == 56


def test_null_handles_and_pointers_are_invalid_arguments():
    from thesia_amd import _ffi
    req = (_ffi.ExportRequest * 1)(_ffi.ExportRequest(0, 0, 0, 0, 0, 0.0, INF))
    info = (_ffi.ExportInfo * 1)()
    n = C.c_size_t()
    out = (C.c_uint8 * 64)()
    for pfx in ("th_tm_", "th_tmg_"):
        assert getattr(_ffi.lib, pfx + "export_pcm")(None, req, 1, out, 64, info, C.byref(n)) == _ffi.ERR_INVALID_ARG
        assert getattr(_ffi.lib, pfx + "export_wav")(None, req, out, 64, info, C.byref(n)) == _ffi.ERR_INVALID_ARG
    a, b = C.c_uint32(), C.c_uint32()
    assert _ffi.lib.th_export_dither(0, 0, 0, None, C.byref(b)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_export_dither(0, 0, 0, C.byref(a), None) == _ffi.ERR_INVALID_ARG
    s0 = C.c_size_t()
    assert _ffi.lib.th_audio_sample_range(48000, 10, 0.0, INF, C.byref(s0), None) == _ffi.ERR_INVALID_ARG
    hl = C.c_size_t()
    assert _ffi.lib.th_wav_header(0, 48000, 1, 1, out, C.byref(hl), None) == _ffi.ERR_INVALID_ARG
    x, q, c = (C.c_float * 1)(), (C.c_int32 * 1)(), C.c_uint64()
    assert _ffi.lib.th_export_quantize(0, 0, 0, 0, 0, x, 1, q, None, C.byref(c)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_export_quantize(3, 0, 0, 0, 0, x, 1, q, C.byref(c), C.byref(c)) == _ffi.ERR_INVALID_ARG  # unknown format
    assert _ffi.lib.th_export_quantize(0, 2, 0, 0, 0, x, 1, q, C.byref(c), C.byref(c)) == _ffi.ERR_INVALID_ARG  # unknown dither


# ---------------------------------------------------------------- the dither generator
def test_dither_known_answers():
    import thesia_amd as ta
    idx = [0, 1, 2, 2 ** 32 + 5]
    want_a, want_b = [8220826, 1636180, 13041725, 15239218], [3630907, 8637162, 13696948, 15471473]
    assert [ta.export_dither(0, 0, i) for i in idx] == list(zip(want_a, want_b))
    a, b = R.dither(0, 0, np.array(idx, dtype=np.uint64))
    assert a.tolist() == want_a and b.tolist() == want_b
    idx = [0, 1, 2 ** 40]
    want_a, want_b = [8016142, 5584711, 11161591], [11962815, 15468606, 3483762]
    assert [ta.export_dither(7, 3, i) for i in idx] == list(zip(want_a, want_b))
    a, b = R.dither(7, 3, np.array(idx, dtype=np.uint64))
    assert a.tolist() == want_a and b.tolist() == want_b


def test_dither_matches_the_restatement_on_random_arguments():
    import thesia_amd as ta
    rng = np.random.default_rng(20261018)
    n = 10000
    seed = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    ch = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    ch[::3] = rng.integers(0, 8, ch[::3].size, dtype=np.uint64)
    i = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    i[::2] = rng.integers(0, 2 ** 32, i[::2].size, dtype=np.uint64)  # half below 2^32, half (almost all) at or above it
    i[:4] = [0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1]
    seed[:2], ch[:2] = 2 ** 32 - 1, 2 ** 32 - 1  # (ch + 1 wraps)
    assert (i >= 2 ** 32).sum() > 4000
    a, b = R.dither(seed, ch, i)
    got = [ta.export_dither(int(s), int(c), int(k)) for s, c, k in zip(seed, ch, i)]
    assert got == list(zip(a.tolist(), b.tolist()))
    assert int(a.max()) < 2 ** 24 and int(b.max()) < 2 ** 24


@pytest.mark.parametrize("seed, ch", [(0, 0), (0, 1), (12345, 0)])
def test_dither_statistics(seed, ch):
    """The statistics are taken on the restatement's d; that the library's generator gives these very values is checked on the
    whole run through th_export_quantize (x = 0 under TPDF gives q = rint(d)) and on 64 direct th_export_dither calls."""
    import thesia_amd as ta
    n = 1 << 20
    a, b = R.dither(seed, ch, np.arange(n, dtype=np.uint64))
    assert [ta.export_dither(seed, ch, i) for i in range(0, n, n // 64)] == list(zip(a[::n // 64].tolist(), b[::n // 64].tolist()))
    q, _, _ = ta.export_quantize(R.PCM_S24, R.DITHER_TPDF, seed, ch, 0, np.zeros(n, np.float32))
    af, bf = a.astype(np.float64), b.astype(np.float64)
    d = (af - bf) * 2.0 ** -24
    assert np.array_equal(q, np.rint(d).astype(np.int32))  # the library's whole run of 2^20 values is the restatement's
    mean, var = d.mean(), d.var()
    lag1 = np.corrcoef(d[:-1], d[1:])[0, 1]
    cab = np.corrcoef(af, bf)[0, 1]
    print("seed %d ch %d: mean %.3e  var/(1/6) - 1 %.3e  lag1 %.3e  corr(a, b) %.3e" % (seed, ch, mean, var * 6 - 1, lag1, cab))
    assert abs(mean) <= 2e-3
    assert abs(var * 6.0 - 1.0) <= 0.01
    assert abs(lag1) <= 5e-3
    assert abs(cab) <= 5e-3
    assert d.min() > -1.0 and d.max() < 1.0


# ---------------------------------------------------------------- the quantiser
@pytest.mark.parametrize("fmt", [R.PCM_S16, R.PCM_S24])
@pytest.mark.parametrize("dith", [R.DITHER_NONE, R.DITHER_TPDF])
def test_quantize_random_samples(fmt, dith):
    import thesia_amd as ta
    rng = np.random.default_rng(7 + fmt * 2 + dith)
    x = rng.uniform(-1.2, 1.2, 50000).astype(np.float32)
    for seed, ch, first in ((0, 0, 0), (99, 5, 123456789), (3, 1, 2 ** 32 - 20000)):
        q, nc, nn = ta.export_quantize(fmt, dith, seed, ch, first, x)
        wq, wnc, wnn = R.quantize(fmt, dith, seed, ch, first, x)
        assert np.array_equal(q, wq) and (nc, nn) == (wnc, wnn)
        assert nc > 1000 and nn == 0  # (a sixth of the samples lie beyond +-1)
        assert q.min() == -R.SCALE[fmt] and q.max() == R.SCALE[fmt] - 1


@pytest.mark.parametrize("fmt", [R.PCM_S16, R.PCM_S24])
def test_quantize_ties_and_edges(fmt):
    import thesia_amd as ta
    S = R.SCALE[fmt]
    f = np.float32
    ties = np.array([0.5 / S, 1.5 / S, -0.5 / S, 2.5 / S, -1.5 / S, -2.5 / S], f)
    q, nc, nn = ta.export_quantize(fmt, R.DITHER_NONE, 0, 0, 0, ties)
    assert q.tolist() == [0, 2, 0, 2, -2, -2] and (nc, nn) == (0, 0)
    tiny = np.array([1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38], f)  # f32 denormals
    assert np.all(tiny != 0) and np.all(np.abs(tiny) < np.finfo(f).tiny)
    edge = np.concatenate([np.array([1.0, -1.0, 1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24), INF, -INF, NAN, -0.0, 0.0,
                                     (S - 1) / S, (S - 0.5) / S, -(S + 0.5) / S, 3.0e38, -3.0e38], f), tiny])
    for dith in (R.DITHER_NONE, R.DITHER_TPDF):
        q, nc, nn = ta.export_quantize(fmt, dith, 11, 2, 1000, edge)
        wq, wnc, wnn = R.quantize(fmt, dith, 11, 2, 1000, edge)
        assert np.array_equal(q, wq) and (nc, nn) == (wnc, wnn), (dith, q, wq)
        assert nn == 1 and q[6] == 0
        assert q[4] == S - 1 and q[5] == -S and q[12] == S - 1 and q[13] == -S
    q, nc, nn = ta.export_quantize(fmt, R.DITHER_NONE, 0, 0, 0, edge)
    # +1.0 clamps to S - 1 and is counted; -1.0 is -S, in range; (S - 0.5) / S rounds to even = S: clamped
    assert q[0] == S - 1 and q[1] == -S and q[7] == 0 and q[8] == 0 and q[9] == S - 1
    assert q[10] == S - 1 and q[11] == -S
    assert nc == R.quantize(fmt, R.DITHER_NONE, 0, 0, 0, edge)[1]
    assert np.array_equal(q[-4:], [0, 0, 0, 0])


def test_quantize_f32_is_a_copy():
    import thesia_amd as ta
    x = np.array([0.25, -1.5, NAN, INF, -0.0, 1e-45], np.float32)
    x[2:3].view(np.uint32)[0] = 0x7FC12345  # a NaN with a payload
    q, nc, nn = ta.export_quantize(R.PCM_F32, R.DITHER_TPDF, 5, 1, 0, x)
    assert np.array_equal(q.view(np.uint32), x.view(np.uint32)) and (nc, nn) == (0, 1)
    data, wnc, wnn = R.pcm_bytes(R.PCM_F32, 0, 0, x[None], 0, x.size)
    assert data.tobytes() == x.tobytes() and (wnc, wnn) == (0, 1)


def test_restated_interleave_and_byte_order():
    ch = np.array([[0.5, -0.5], [0.25, -1.0]], np.float32)
    data, _, _ = R.pcm_bytes(R.PCM_S16, R.DITHER_NONE, 0, ch, 0, 2)
    assert data.tobytes() == struct.pack("<4h", 16384, 8192, -16384, -32768)
    data, _, _ = R.pcm_bytes(R.PCM_S24, R.DITHER_NONE, 0, ch, 1, 2)
    assert data.tobytes() == (-4194304).to_bytes(3, "little", signed=True) + (-8388608).to_bytes(3, "little", signed=True)


# ---------------------------------------------------------------- the WAV header
@pytest.mark.parametrize("fmt", [R.PCM_S16, R.PCM_S24, R.PCM_F32])
@pytest.mark.parametrize("sr, n_ch, n_frames", [(48000, 1, 0), (48000, 1, 1), (44100, 2, 12345), (8000, 3, 7), (192000, 6, 5),
                                                  (48000, 1, 1001), (96000, 1024, 3)])
def test_wav_header_equals_the_restatement(fmt, sr, n_ch, n_frames):
    import thesia_amd as ta
    want = R.wav_header(fmt, sr, n_ch, n_frames)
    assert ta.wav_header(fmt, sr, n_ch, n_frames) == want
    h, pad = want
    assert len(h) == (58 if fmt == R.PCM_F32 else 44)
    assert pad == (n_frames * n_ch * R.BYTES[fmt]) % 2


@pytest.mark.parametrize("fmt", [R.PCM_S16, R.PCM_S24])
@pytest.mark.parametrize("n_ch, n_frames", [(1, 1001), (2, 500), (3, 333), (1, 0)])
def test_wav_header_round_trips_through_the_wave_module(fmt, n_ch, n_frames):
    import thesia_amd as ta
    rng = np.random.default_rng(n_ch * 1000 + n_frames)
    ch = rng.uniform(-1, 1, (n_ch, n_frames)).astype(np.float32)
    data, _, _ = R.pcm_bytes(fmt, R.DITHER_NONE, 0, ch, 0, n_frames)
    h, pad = ta.wav_header(fmt, 44100, n_ch, n_frames)
    with wave.open(io.BytesIO(h + data.tobytes() + b"\0" * pad), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (n_ch, R.BYTES[fmt], 44100, n_frames)
        assert w.readframes(n_frames) == data.tobytes()


def test_wav_header_pad_byte_and_sizes():
    import thesia_amd as ta
    h, pad = ta.wav_header(R.PCM_S24, 48000, 1, 1001)  # 3003 data bytes: odd
    assert pad == 1
    assert struct.unpack_from("<I", h, 4)[0] == 36 + 3003 + 1   # the RIFF size counts the pad
    assert struct.unpack_from("<I", h, 40)[0] == 3003            # the data size does not
    assert ta.wav_header(R.PCM_S24, 48000, 1, 1000)[1] == 0 and ta.wav_header(R.PCM_S24, 48000, 2, 1001)[1] == 0
    assert ta.wav_header(R.PCM_S16, 48000, 1, 1001)[1] == 0


def test_wav_float_header_fields():
    import thesia_amd as ta
    h, pad = ta.wav_header(R.PCM_F32, 44100, 2, 777)
    assert pad == 0 and len(h) == 58
    riff, size, wave_, fmt_, fmt_len = struct.unpack_from("<4sI4s4sI", h, 0)
    assert (riff, wave_, fmt_, fmt_len) == (b"RIFF", b"WAVE", b"fmt ", 18)
    tag, n_ch, sr, rate, block, bits, cb = struct.unpack_from("<HHIIHHH", h, 20)
    assert (tag, n_ch, sr, rate, block, bits, cb) == (3, 2, 44100, 44100 * 8, 8, 32, 0)
    fact, fact_len, frames, data, data_len = struct.unpack_from("<4sII4sI", h, 38)
    assert (fact, fact_len, frames, data, data_len) == (b"fact", 4, 777, b"data", 777 * 8)
    assert size == 58 - 8 + 777 * 8


def test_wav_header_refusals():
    import thesia_amd as ta
    # the largest file RIFF can describe, and one frame more
    most = (2 ** 32 - 1 - 36) // 2
    h, pad = ta.wav_header(R.PCM_S16, 48000, 1, most)
    assert struct.unpack_from("<I", h, 4)[0] == 36 + 2 * most and R.wav_header(R.PCM_S16, 48000, 1, most) == (h, pad)
    cases = [(R.PCM_S16, 48000, 1, most + 1), (R.PCM_S24, 48000, 2, 2 ** 32 // 6), (R.PCM_F32, 48000, 2, 2 ** 29),
             (R.PCM_S16, 48000, 1, 2 ** 40), (R.PCM_S16, 48000, 65536, 1), (R.PCM_F32, 48000, 20000, 1), (R.PCM_S16, 2 ** 31, 2, 1)]
    for fmt, sr, n_ch, n_frames in cases:
        assert R.wav_header(fmt, sr, n_ch, n_frames) == "unsupported"
        with pytest.raises(ta.ThError) as e:
            ta.wav_header(fmt, sr, n_ch, n_frames)
        assert e.value.code == -2, (fmt, sr, n_ch, n_frames)
    for fmt, sr, n_ch in [(R.PCM_S16, 48000, 0), (R.PCM_S16, 0, 1), (3, 48000, 1)]:
        assert R.wav_header(fmt, sr, n_ch, 10) == "invalid"
        with pytest.raises(ta.ThError) as e:
            ta.wav_header(fmt, sr, n_ch, 10)
        assert e.value.code == -1


# ---------------------------------------------------------------- the sample range
@pytest.mark.parametrize("sr, n, a, b, want", [
    # the edges of th_spectrum_frame_range's own tests, at hop 1 (sample t is selected when t / sr lies in [a, b))
    (48000, 3001, 0.0, INF, (0, 3001)),
    (48000, 1440000, 0.01, 0.02, (480, 960)),
    (48000, 1440000, 29.99, 31.0, (1439520, 1440000)),
    (44100, 44100, 0.005, 0.0051, (221, 225)),
    (48000, 100, 0.0, 0.0, (0, 0)),
    (48000, 100, 1.0, 2.0, (100, 100)),
    (48000, 0, 0.0, INF, (0, 0)),
    (44100, 100, 1 / 44100, 3 / 44100, (1, 3)),
])
def test_sample_range_known_cases(sr, n, a, b, want):
    import thesia_amd as ta
    assert ta.audio_sample_range(sr, n, a, b) == want
    assert R.sample_range(sr, n, a, b) == want
    assert ta.spectrum_frame_range(sr, 1, n, a, b) == want


def test_sample_range_matches_the_restatement_on_random_ranges():
    import random
    import thesia_amd as ta
    rnd = random.Random(20261018)
    for _ in range(400):
        sr = rnd.choice([8000, 11025, 22050, 44100, 48000, 96000, 192000])
        n = rnd.choice([0, 1, 2, 51, 1200, 3001, 120000, 2 ** 33])
        dur = n / sr
        a = rnd.choice([0.0, rnd.uniform(0.0, 1.2 * dur + 0.01), rnd.randrange(0, min(n, 10 ** 6) + 2) / sr])
        b = rnd.choice([INF, a, a + rnd.uniform(0.0, dur + 0.01), a + rnd.randrange(0, min(n, 10 ** 6) + 2) / sr])
        got = ta.audio_sample_range(sr, n, a, b)
        assert got == R.sample_range(sr, n, a, b), (sr, n, a, b)
        assert 0 <= got[0] <= got[1] <= n
    assert ta.audio_sample_range(48000, 100) == (0, 100)  # the defaults: the whole track


@pytest.mark.parametrize("sr, a, b", [
    (48000, NAN, 1.0), (48000, -0.001, 1.0), (48000, INF, INF), (48000, -INF, 1.0),
    (48000, 0.0, NAN), (48000, 1.0, 0.999), (48000, 0.5, -INF), (0, 0.0, 1.0),
])
def test_sample_range_refusals(sr, a, b):
    import thesia_amd as ta
    with pytest.raises(ta.ThError) as e:
        ta.audio_sample_range(sr, 100, a, b)
    assert e.value.code == -1
