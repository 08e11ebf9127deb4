"""PCM / WAV export of resident tracks (th_tm_export_pcm / th_tm_export_wav and the th_tmg twins) on the GPU.

Reference: the definitions restated in numpy (tests/export_ref.py) applied to the samples th_tm_copy_audio returns for the same
(id, channel, which) - existing code, not the code under test.  Every comparison is byte-exact; the counts are exact.

Tracks (odd lengths, so that the last group of four samples of a channel is partial): ids 1, 2, 3, 6 hold 1, 2, 3 and 6 channels of
5003 samples with values up to +-1.1 (some clamp); 11 is 44.1 kHz stereo; a manager of its own holds a track with NaN, +-inf and
values beyond +-1.  The kernel
cuts a request on the track's absolute frame grid into chunks of export_chunk_frames(n_ch) frames (4096, 2048, 1364, 680 for 1, 2,
3, 6 channels): the frame counts include that length - 1, + 0 and + 1, from frame 0 (whole chunks) and from frame 1 (every chunk
boundary falls inside the range, the first and last chunk are partial)."""
import ctypes as C
import io
import wave

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api
from tests import export_ref as R
from tests.synth import synth_track

pytestmark = pytest.mark.gpu

INF = float("inf")
FORMATS = (R.PCM_S16, R.PCM_S24, R.PCM_F32)
DITHERS = (R.DITHER_NONE, R.DITHER_TPDF)
N = 5003
CANARY = 64


def _audio(seed, sr, n, channels, peak=1.1):
    x = np.stack([synth_track(seed + c, sr, n) for c in range(channels)])
    return (x * (peak / np.abs(x).max())).astype(np.float32)


def _tracks():
    t = {k: (48000, _audio(10 * k, 48000, N, k)) for k in (1, 2, 3, 6)}
    t[11] = (44100, _audio(200, 44100, 3001, 2, 0.9))
    return t


def _bad_track():
    bad = _audio(300, 48000, 1501, 2, 1.5)
    bad[0, 7] = np.nan
    bad[1, 8:10] = np.nan
    bad[0, 100] = np.inf
    bad[1, 101] = -np.inf
    bad[0, 1500] = np.nan  # the very last sample
    return bad


TRACKS = _tracks()


def sec_of(s, sr):
    """a time whose first sample at or after it is s"""
    t = s / sr
    while R.sample_range(sr, 10 ** 12, t, INF)[0] != s:
        t = np.nextafter(t, 0.0)
    return float(t)


@pytest.fixture(scope="module")
def ctx():
    c = ta.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tm(ctx):
    m = ta.TrackManager(ctx)
    m.add_tracks([(i, sr, x) for i, (sr, x) in sorted(TRACKS.items())])
    yield m
    m.close()


_AUDIO = {}


def audio_of(m, tid, which=0):
    """[n_ch][n] of the module's manager as th_tm_copy_audio returns it, read once per (id, which) and left unchanged"""
    if (tid, which) not in _AUDIO:
        a = np.stack([m.audio(tid, c, which) for c in range(TRACKS[tid][1].shape[0])])
        a.setflags(write=False)
        _AUDIO[(tid, which)] = a
    return _AUDIO[(tid, which)]


def expect(m, tid, fmt, dith, seed, s0, s1, which=0):
    return R.pcm_bytes(fmt, dith, seed, audio_of(m, tid, which), s0, s1)


def raw_export(handle, reqs, pfx="th_tm_", cap=None, fill=0xA5):
    """the C entry on a buffer with CANARY bytes of `fill` on each side -> (rc, whole buffer, infos, out_len)"""
    n = len(reqs)
    arr = (_ffi.ExportRequest * n)(*[api._export_request(r) for r in reqs])
    info = (_ffi.ExportInfo * n)()
    need = C.c_size_t()
    fn = getattr(_ffi.lib, pfx + "export_pcm")
    if cap is None:
        rc = fn(handle, arr, n, None, 0, info, C.byref(need))
        assert rc in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL), _ffi.last_error()
        cap = need.value
    buf = np.full(cap + 2 * CANARY, fill, np.uint8)
    rc = fn(handle, arr, n, buf.ctypes.data + CANARY, cap, info, C.byref(need))
    return rc, buf, [api._export_info_dict(o) for o in info], need.value


def check_image(buf, infos, wants, out_len):
    """request bytes, zero padding between requests, untouched canaries"""
    img = buf[CANARY: CANARY + out_len]
    assert np.all(buf[:CANARY] == 0xA5) and np.all(buf[CANARY + out_len:] == 0xA5)
    at = 0
    for i, (o, (data, n_clamped, n_nan)) in enumerate(zip(infos, wants)):
        assert o["offset"] % 16 == 0 and o["offset"] == at, (i, o)
        assert o["n_bytes"] == data.size, (i, o)
        assert np.array_equal(img[at: at + data.size], data), (i, o)
        assert (o["n_clamped"], o["n_nan"]) == (n_clamped, n_nan), (i, o)
        end = at + data.size
        at = (end + 15) // 16 * 16
        if i + 1 < len(infos):
            assert np.all(img[end: at] == 0), (i, o)  # the padding is written as zero
        else:
            assert end == out_len


def counts_for(n_ch):
    F = ta.export_chunk_frames(n_ch)
    return [0, 1, 3, 255, 256, 257, F - 1, F, F + 1, 5000]


def test_chunk_lengths():
    assert [ta.export_chunk_frames(c) for c in (1, 2, 3, 6, 1024)] == [4096, 2048, 1364, 680, 4]


@pytest.mark.parametrize("n_ch", [1, 2, 3, 6])
def test_formats_dithers_counts_and_odd_starts(tm, n_ch):
    """every format x dither x frame count, from frame 0 and from frame 1, as ONE batch (offsets, zero padding, canaries)"""
    sr = 48000
    reqs, wants = [], []
    for fmt in FORMATS:
        for dith in DITHERS:
            for cnt in counts_for(n_ch):
                for s0 in (0, 1):
                    seed = 1000 * fmt + 10 * dith + s0
                    reqs.append((n_ch, fmt, dith, seed, sec_of(s0, sr), sec_of(s0 + cnt, sr)))
                    wants.append(expect(tm, n_ch, fmt, dith, seed, s0, s0 + cnt))
    rc, buf, infos, out_len = raw_export(tm.handle, reqs)
    assert rc == _ffi.OK, _ffi.last_error()
    for o, r in zip(infos, reqs):
        assert (o["sr"], o["n_channels"]) == (sr, n_ch)
        assert (o["sample_start"], o["sample_end"]) == R.sample_range(sr, N, r[4], r[5])
    check_image(buf, infos, wants, out_len)
    assert sum(o["n_clamped"] for o in infos) > 0  # (the tracks peak at 1.1)


@pytest.mark.parametrize("n_ch", [1, 2, 3, 6])
def test_single_calls_whole_track_and_mid_chunk_ranges(tm, n_ch):
    """one request per call: the whole track (its last group of four samples is partial), and a range from an odd sample to the
    middle of a chunk"""
    F = ta.export_chunk_frames(n_ch)
    for fmt in FORMATS:
        for dith in DITHERS:
            for s0, s1 in ((0, N), (F - 3, min(N, 2 * F + F // 2 + 1)), (N - 1, N)):
                out, infos = tm.export_pcm([(n_ch, fmt, dith, 77, sec_of(s0, 48000), INF if s1 == N else sec_of(s1, 48000))])
                data, nc, nn = expect(tm, n_ch, fmt, dith, 77, s0, s1)
                assert np.array_equal(out, data), (fmt, dith, s0, s1)
                assert (infos[0]["offset"], infos[0]["n_bytes"], infos[0]["n_clamped"], infos[0]["n_nan"]) == (0, data.size, nc, nn)


@pytest.mark.parametrize("fmt", [R.PCM_S16, R.PCM_S24])
def test_a_range_is_a_slice_of_the_whole_export(tm, fmt):
    """TPDF: the dither index is the absolute sample index"""
    n_ch, bps = 3, R.BYTES[fmt]
    whole, _ = tm.export_pcm([(n_ch, fmt, R.DITHER_TPDF, 5)])
    assert whole.size == N * n_ch * bps
    for s0, s1 in ((1, 2), (1363, 1366), (777, 4097), (4999, N)):
        part, _ = tm.export_pcm([(n_ch, fmt, R.DITHER_TPDF, 5, sec_of(s0, 48000), sec_of(s1, 48000))])
        assert np.array_equal(part, whole[s0 * n_ch * bps: s1 * n_ch * bps]), (s0, s1)
    other, _ = tm.export_pcm([(n_ch, fmt, R.DITHER_TPDF, 6)])
    assert not np.array_equal(other, whole)  # the seed matters
    plain, _ = tm.export_pcm([(n_ch, fmt, R.DITHER_NONE, 5)])
    assert not np.array_equal(plain, whole)


def test_batched_mixed_requests_equal_the_single_calls(tm):
    reqs = [(2, R.PCM_S24, R.DITHER_TPDF, 1, sec_of(1, 48000), sec_of(2050, 48000)),
            (11, R.PCM_S16, R.DITHER_TPDF, 2),                                         # another rate
            (1, R.PCM_F32, R.DITHER_NONE, 0, 0.01, 0.05),
            (2, R.PCM_S16, R.DITHER_NONE, 3),                                          # an id again
            (6, R.PCM_S24, R.DITHER_NONE, 4, sec_of(3, 48000), sec_of(4, 48000)),     # 18 bytes
            (3, R.PCM_S16, R.DITHER_TPDF, 5, 0.02, 0.02),                              # empty
            (2, R.PCM_S24, R.DITHER_TPDF, 1, sec_of(1, 48000), sec_of(2050, 48000)),  # the first one again
            (6, R.PCM_S16, R.DITHER_TPDF, 9)]
    rc, buf, infos, out_len = raw_export(tm.handle, reqs)
    assert rc == _ffi.OK, _ffi.last_error()
    wants = []
    for r, o in zip(reqs, infos):
        single, si = tm.export_pcm([r])
        tid, fmt, dith, seed, a, b = tuple(r) + (0.0, INF)[len(r) - 4:]
        sr = TRACKS[tid][0]
        s0, s1 = R.sample_range(sr, TRACKS[tid][1].shape[1], a, b)
        want = expect(tm, tid, fmt, dith, seed, s0, s1)
        assert np.array_equal(single, want[0])
        assert {k: v for k, v in si[0].items() if k != "offset"} == {k: v for k, v in o.items() if k != "offset"}
        assert o["sr"] == sr
        wants.append(want)
    check_image(buf, infos, wants, out_len)
    assert infos[5]["n_bytes"] == 0 and infos[6]["offset"] == infos[5]["offset"]
    a, b = infos[0], infos[6]
    assert np.array_equal(buf[CANARY + a["offset"]: CANARY + a["offset"] + a["n_bytes"]],
                          buf[CANARY + b["offset"]: CANARY + b["offset"] + b["n_bytes"]])


@pytest.mark.parametrize("tid, fmt, dith, s0, s1", [
    (1, R.PCM_S24, R.DITHER_TPDF, 0, N),        # 24-bit mono, odd length: a pad byte; the data starts at byte 44
    (1, R.PCM_S24, R.DITHER_NONE, 2, 4100),     # even: no pad
    (2, R.PCM_F32, R.DITHER_NONE, 1, N),        # float stereo: the data starts at byte 58
    (2, R.PCM_S16, R.DITHER_TPDF, 0, N),
    (3, R.PCM_S16, R.DITHER_NONE, 10, 10),      # empty: a header-only file
])
def test_export_wav_is_header_data_pad(tm, tid, fmt, dith, s0, s1):
    sr, x = TRACKS[tid]
    a, b = sec_of(s0, sr), (INF if s1 == N else sec_of(s1, sr))
    blob, info = tm.export_wav(tid, fmt, dith, 42, a, b)
    pcm, _ = tm.export_pcm([(tid, fmt, dith, 42, a, b)])
    hdr, pad = ta.wav_header(fmt, sr, x.shape[0], s1 - s0)
    assert blob == hdr + pcm.tobytes() + b"\0" * pad
    assert blob == R.wav_file(fmt, dith, 42, sr, audio_of(tm, tid), s0, s1)
    data, nc, nn = expect(tm, tid, fmt, dith, 42, s0, s1)
    assert (info["offset"], info["n_bytes"], info["sample_start"], info["sample_end"]) == (len(hdr), data.size, s0, s1)
    assert (info["n_clamped"], info["n_nan"], info["sr"], info["n_channels"]) == (nc, nn, sr, x.shape[0])
    assert pad == (1 if (tid, fmt, s1 - s0) == (1, R.PCM_S24, N) else 0)
    if fmt != R.PCM_F32:
        with wave.open(io.BytesIO(blob), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (x.shape[0], R.BYTES[fmt], sr, s1 - s0)
            assert w.readframes(s1 - s0) == data.tobytes()


def test_export_wav_writes_inside_its_buffer_only(tm):
    """the data of a WAV image starts at byte 44: no 16-byte piece may spill over either end"""
    req = _ffi.ExportRequest(1, 0, R.PCM_S24, R.DITHER_TPDF, 1, 0.0, INF)
    info, need = _ffi.ExportInfo(), C.c_size_t()
    assert _ffi.lib.th_tm_export_wav(tm.handle, C.byref(req), None, 0, C.byref(info), C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert need.value == 44 + 3 * N + 1 and (info.offset, info.n_bytes) == (44, 3 * N)
    for shift in (0, 1, 7):  # the caller's buffer itself at an odd address
        buf = np.full(need.value + 2 * CANARY + 8, 0xA5, np.uint8)
        lo = CANARY + shift
        rc = _ffi.lib.th_tm_export_wav(tm.handle, C.byref(req), buf.ctypes.data + lo, need.value, C.byref(info), C.byref(need))
        assert rc == _ffi.OK, _ffi.last_error()
        assert buf[lo: lo + need.value].tobytes() == R.wav_file(R.PCM_S24, R.DITHER_TPDF, 1, 48000, audio_of(tm, 1), 0, N)
        assert np.all(buf[:lo] == 0xA5) and np.all(buf[lo + need.value:] == 0xA5)
        small = np.full(need.value + 2 * CANARY, 0xA5, np.uint8)
        rc = _ffi.lib.th_tm_export_wav(tm.handle, C.byref(req), small.ctypes.data + CANARY, need.value - 1, C.byref(info), C.byref(need))
        assert rc == _ffi.ERR_BUFFER_TOO_SMALL and np.all(small == 0xA5)


def test_nonfinite_and_loud_samples_and_the_counts(ctx):
    bad = _bad_track()
    n = bad.shape[1]
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(12, 48000, bad)])
        x = np.stack([m.audio(12, c) for c in range(2)])
        assert np.array_equal(x.view(np.uint32), bad.view(np.uint32))
        for fmt in FORMATS:
            for dith in DITHERS:
                out, infos = m.export_pcm([(12, fmt, dith, 3)])
                data, nc, nn = R.pcm_bytes(fmt, dith, 3, x, 0, n)
                assert np.array_equal(out, data)
                assert (infos[0]["n_clamped"], infos[0]["n_nan"]) == (nc, nn)
                assert nn == 4
                assert nc == 0 if fmt == R.PCM_F32 else nc > 2  # both infinities and samples beyond +-1
        # a range that holds none of the NaNs, and one that holds the last sample alone
        out, infos = m.export_pcm([(12, R.PCM_S16, R.DITHER_NONE, 0, sec_of(10, 48000), sec_of(20, 48000)),
                                   (12, R.PCM_F32, R.DITHER_NONE, 0, sec_of(1500, 48000), INF)])
        assert infos[0]["n_nan"] == 0 and infos[1]["n_nan"] == 1 and infos[1]["n_bytes"] == 8
        blob, info = m.export_wav(12, R.PCM_S24, R.DITHER_TPDF, 3)
        assert blob == R.wav_file(R.PCM_S24, R.DITHER_TPDF, 3, 48000, x, 0, n) and info["n_nan"] == 4
    finally:
        m.close()


def test_which_selects_audio_drawing_or_original(ctx):
    m = ta.TrackManager(ctx)
    try:
        sr, x = TRACKS[2]
        m.add_tracks([(2, sr, x)])
        m.set_common_guard_clipping(api.GUARD_CLIP)
        m.set_common_normalize(api.NORM_PEAK_DB, 6.0)  # a peak of +6 dB: the clip guard has work
        aud = [np.stack([m.audio(2, c, w) for c in range(2)]) for w in (0, 1, 2)]
        assert not np.array_equal(aud[0], aud[1]) and not np.array_equal(aud[1], aud[2]) and not np.array_equal(aud[0], aud[2])
        assert np.abs(aud[0]).max() == 1.0 and np.abs(aud[1]).max() > 1.9
        for which in (0, 1, 2):
            for fmt, dith in ((R.PCM_S16, R.DITHER_TPDF), (R.PCM_S24, R.DITHER_NONE), (R.PCM_F32, R.DITHER_NONE)):
                out, infos = m.export_pcm([(2, fmt, dith, 8, 0.0, INF, which)])
                data, nc, nn = R.pcm_bytes(fmt, dith, 8, aud[which], 0, N)
                assert np.array_equal(out, data), (which, fmt)
                assert (infos[0]["n_clamped"], infos[0]["n_nan"]) == (nc, nn)
        blob, _ = m.export_wav(2, R.PCM_S16, R.DITHER_TPDF, 8, which=1)
        assert blob == R.wav_file(R.PCM_S16, R.DITHER_TPDF, 8, sr, aud[1], 0, N)
    finally:
        m.close()


def test_waveform_revision_follows_set_common_normalize(ctx):
    m = ta.TrackManager(ctx)
    try:
        sr, x = TRACKS[1]
        m.add_tracks([(1, sr, x)])
        out0, i0 = m.export_pcm([(1, R.PCM_S16)])
        assert i0[0]["waveform_revision"] == m.revisions()[0]
        m.set_common_normalize(api.NORM_PEAK_DB, -12.0)
        out1, i1 = m.export_pcm([(1, R.PCM_S16)])
        assert i1[0]["waveform_revision"] == m.revisions()[0] > i0[0]["waveform_revision"]
        assert not np.array_equal(out0, out1)
        assert np.array_equal(out1, R.pcm_bytes(R.PCM_S16, 0, 0, m.audio(1, 0)[None], 0, N)[0])
        _, iw = m.export_wav(1, R.PCM_S16)
        assert iw["waveform_revision"] == i1[0]["waveform_revision"]
    finally:
        m.close()


def test_errors_write_nothing(tm):
    good = (1, R.PCM_S16, R.DITHER_NONE, 0, 0.0, 0.01)
    nan = float("nan")
    cases = [((99, R.PCM_S16), _ffi.ERR_NOT_FOUND),
             ((1, 3), _ffi.ERR_INVALID_ARG),                                  # unknown format
             ((1, R.PCM_S16, 2), _ffi.ERR_INVALID_ARG),                       # unknown dither
             ((1, R.PCM_S16, 0, 0, 0.0, INF, 3), _ffi.ERR_INVALID_ARG),       # unknown which
             ((1, R.PCM_S16, 0, 0, -0.5, INF), _ffi.ERR_INVALID_ARG),
             ((1, R.PCM_S16, 0, 0, nan, INF), _ffi.ERR_INVALID_ARG),
             ((1, R.PCM_S16, 0, 0, 0.0, nan), _ffi.ERR_INVALID_ARG),
             ((1, R.PCM_S16, 0, 0, INF, INF), _ffi.ERR_INVALID_ARG),
             ((1, R.PCM_S16, 0, 0, 0.02, 0.01), _ffi.ERR_INVALID_ARG)]
    for bad, code in cases:
        for reqs in ([bad], [good, bad], [good, bad, (98, R.PCM_S16)]):
            rc, buf, _, _ = raw_export(tm.handle, reqs, cap=4096)
            assert rc == code, (bad, rc, _ffi.last_error())
            assert np.all(buf == 0xA5), bad
    rc, buf, _, _ = raw_export(tm.handle, [good, (98, R.PCM_S16), (1, 3)], cap=4096)
    assert rc == _ffi.ERR_NOT_FOUND and np.all(buf == 0xA5)  # the first faulty request decides
    # export_wav: the same codes
    for bad, code in cases:
        req = api._export_request(bad)
        buf = np.full(4096, 0xA5, np.uint8)
        need = C.c_size_t()
        assert _ffi.lib.th_tm_export_wav(tm.handle, C.byref(req), buf.ctypes.data, buf.size, None, C.byref(need)) == code
        assert np.all(buf == 0xA5)


def test_size_query_and_small_buffers(tm):
    reqs = [(2, R.PCM_S24, R.DITHER_TPDF, 1, sec_of(1, 48000), sec_of(100, 48000)), (3, R.PCM_S16)]
    n = len(reqs)
    arr = (_ffi.ExportRequest * n)(*[api._export_request(r) for r in reqs])
    info = (_ffi.ExportInfo * n)()
    need = C.c_size_t()
    assert _ffi.lib.th_tm_export_pcm(tm.handle, arr, n, None, 0, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL  # out == NULL
    assert (info[0].offset, info[0].n_bytes, info[0].sample_start, info[0].sample_end) == (0, 99 * 6, 1, 100)
    assert (info[1].offset, info[1].n_bytes, info[1].sample_start, info[1].sample_end) == (608, N * 6, 0, N)
    assert need.value == 608 + N * 6
    assert (info[0].sr, info[0].n_channels, info[1].n_channels) == (48000, 2, 3)
    assert info[0].waveform_revision == tm.revisions()[0] and (info[0].n_clamped, info[0].n_nan) == (0, 0)
    assert _ffi.lib.th_tm_export_pcm(tm.handle, arr, n, None, 1 << 20, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    rc, buf, infos, out_len = raw_export(tm.handle, reqs, cap=need.value - 1)
    assert rc == _ffi.ERR_BUFFER_TOO_SMALL and np.all(buf == 0xA5) and out_len == need.value
    assert infos[1]["offset"] == 608
    # an empty batch is valid
    assert _ffi.lib.th_tm_export_pcm(tm.handle, None, 0, None, 0, None, C.byref(need)) == _ffi.OK and need.value == 0
    out, infos = tm.export_pcm([(3, R.PCM_S16, 0, 0, 0.05, 0.05)])  # an empty range alone: nothing to do
    assert out.size == 0 and infos[0]["n_bytes"] == 0
    assert (infos[0]["sample_start"], infos[0]["sample_end"]) == R.sample_range(48000, N, 0.05, 0.05)


def test_a_request_of_more_than_two_pieces(ctx):
    """two channels, 16 bit: the output just exceeds two pieces of TH_EXPORT_PIECE_BYTES, so the call runs three launches through the
    two staging buffers; the second call reuses them.  The undithered bytes are compared in full, the dithered ones on windows at
    the start, around both piece boundaries and at the end (a range's bytes are a slice of the whole export's)."""
    frames_per_piece = api.EXPORT_PIECE_BYTES // 4
    n = 2 * frames_per_piece + 1001
    rng = np.random.default_rng(5)
    x = (rng.integers(-40000, 40000, (2, n), dtype=np.int32).astype(np.float32) / np.float32(32768 * 1.25) + np.float32(1e-4))
    x[1, frames_per_piece - 1] = np.nan
    x[0, 2 * frames_per_piece] = 2.0
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(1, 48000, x)])
        aud = np.stack([m.audio(1, c) for c in range(2)])
        assert np.array_equal(aud.view(np.uint32), x.view(np.uint32))
        want, nc, nn = R.pcm_bytes(R.PCM_S16, R.DITHER_NONE, 0, aud, 0, n)
        assert want.size == 4 * n > 2 * api.EXPORT_PIECE_BYTES
        for _ in range(2):
            out, infos = m.export_pcm([(1, R.PCM_S16)])
            assert np.array_equal(out, want)
            assert (infos[0]["n_clamped"], infos[0]["n_nan"], infos[0]["n_bytes"]) == (nc, nn, want.size)
            assert nn == 1 and nc >= 1
        out, infos = m.export_pcm([(1, R.PCM_S16, R.DITHER_TPDF, 77)])
        for a, b in ((0, 9000), (frames_per_piece - 5000, frames_per_piece + 5000), (2 * frames_per_piece - 5000, 2 * frames_per_piece + 1001)):
            assert np.array_equal(out[4 * a: 4 * b], R.pcm_bytes(R.PCM_S16, R.DITHER_TPDF, 77, aud, a, b)[0]), (a, b)
        # a batch whose second request starts inside the first piece and ends in the second
        half = frames_per_piece + 4097
        out, infos = m.export_pcm([(1, R.PCM_S24, R.DITHER_NONE, 0, 0.0, sec_of(3, 48000)), (1, R.PCM_S16, R.DITHER_NONE, 0, sec_of(1, 48000), sec_of(half, 48000))])
        assert infos[1]["offset"] == 32 and np.all(out[18:32] == 0)
        assert np.array_equal(out[:18], R.pcm_bytes(R.PCM_S24, 0, 0, aud, 0, 3)[0])
        assert np.array_equal(out[32:], want[4: 4 * half])
    finally:
        m.close()


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_tmg_gives_the_bytes_and_infos_of_tm(tm, devices):
    reqs = [(2, R.PCM_S24, R.DITHER_TPDF, 1, sec_of(1, 48000), sec_of(2050, 48000)), (11, R.PCM_S16, R.DITHER_TPDF, 2),
            (1, R.PCM_F32), (6, R.PCM_S24, R.DITHER_NONE, 4, sec_of(3, 48000), sec_of(4, 48000)), (3, R.PCM_S16, R.DITHER_TPDF, 5),
            (6, R.PCM_S16, R.DITHER_NONE, 0), (2, R.PCM_S16)]
    g = ta.MultiTrackManager(devices)
    try:
        g.add_tracks([(i, sr, x) for i, (sr, x) in sorted(TRACKS.items())])
        if len(devices) > 1:
            assert len({g.device_of(i) for i in TRACKS}) == 2
        rc, buf, infos, out_len = raw_export(tm.handle, reqs)
        rcg, bufg, infosg, out_leng = raw_export(g.handle, reqs, pfx="th_tmg_")
        assert rc == rcg == _ffi.OK, _ffi.last_error()
        assert out_len == out_leng and np.array_equal(buf, bufg)
        strip = lambda d: {k: v for k, v in d.items() if k != "waveform_revision"}  # noqa: E731
        assert [strip(o) for o in infos] == [strip(o) for o in infosg]
        assert all(o["waveform_revision"] == g.revisions()[0] for o in infosg)
        for tid, fmt in ((1, R.PCM_S24), (2, R.PCM_F32)):
            assert g.export_wav(tid, fmt, R.DITHER_TPDF, 9)[0] == tm.export_wav(tid, fmt, R.DITHER_TPDF, 9)[0]
        with pytest.raises(ta.ThError) as e:
            g.export_pcm([(1, R.PCM_S16), (99, R.PCM_S16)])
        assert e.value.code == _ffi.ERR_NOT_FOUND
        with pytest.raises(ta.ThError) as e:
            g.export_wav(1, 3)
        assert e.value.code == _ffi.ERR_INVALID_ARG
    finally:
        g.close()
