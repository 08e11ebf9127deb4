"""Export at a target sample rate (th_tm_export_pcm_at / th_tm_export_wav_at and the th_tmg twins) on the GPU.

Reference: th_resample_f32 (the host restatement of the kernel's sum: tests/test_resample_host.py holds it against numpy f64)
applied to the samples th_tm_copy_audio returns, and for the integer formats tests/export_ref.py applied to those floats with the
absolute output index j as the dither index.  Every comparison is bit- or byte-exact; the counts are exact.

The kernel's tile (ta.resample_tile): R consecutive outputs x P periods Lp outputs (Mp input samples) apart; a period of Lp outputs
is S sub-tiles.  Track lengths lie around one and two tiles' input (P Mp +- 1) and output (P Lp +- 1, i.e. R P for the octave
ratios), around the filter length (2K - 1, 2K, 2K + 1), and at 1 and 100 samples; none is a multiple of 4 on purpose except 2K and
100.  Besides the seven rate pairs, three more take the remaining shapes of the tiling ({4, 2}, {4, 1}, {1, 2} waves x periods)."""
import ctypes as C
import io
import wave

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api
from tests import export_ref as E
from tests import resample_ref as R
from tests.synth import synth_track

pytestmark = pytest.mark.gpu

INF = float("inf")
CANARY = 64
PAIRS = [(44100, 48000), (48000, 44100), (48000, 96000), (96000, 48000), (8000, 48000), (48000, 16000), (8000, 8001)]
SHAPE_PAIRS = [(64000, 8000), (128000, 8000), (192000, 8000)]  # G x Pt = 4 x 2, 4 x 1, 1 x 2
FORMATS = (E.PCM_S16, E.PCM_S24, E.PCM_F32)
DITHERS = (E.DITHER_NONE, E.DITHER_TPDF)


def _audio(seed, sr, n, channels, peak=1.1):
    x = np.stack([synth_track(seed + c, sr, n) for c in range(channels)])
    return (x * (peak / max(np.abs(x).max(), 1e-9))).astype(np.float32)


def _noise(seed, n, channels, peak=0.9):
    return (np.random.default_rng(seed).uniform(-peak, peak, (channels, n))).astype(np.float32)


TRACKS = {1: (44100, _audio(10, 44100, 5003, 1)), 2: (48000, _audio(20, 48000, 5003, 2)), 3: (48000, _audio(30, 48000, 5003, 3)),
          6: (44100, _audio(60, 44100, 3001, 6)), 7: (96000, _audio(70, 96000, 9001, 2)), 8: (8000, _noise(80, 9000, 1))}


def sec_of(s, sr):
    """a time whose first sample at or after it is s"""
    t = s / sr
    while E.sample_range(sr, 10 ** 12, t, INF)[0] != s:
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


_WHOLE = {}


def whole(m, tid, sr_out):
    """[n_ch][n_out] f32: th_resample_f32 of the module manager's audio (th_tm_copy_audio), computed once and left unchanged"""
    if (tid, sr_out) not in _WHOLE:
        sr, x = TRACKS[tid]
        y = np.stack([ta.resample_f32(m.audio(tid, c), sr, sr_out) for c in range(x.shape[0])])
        y.setflags(write=False)
        _WHOLE[(tid, sr_out)] = y
    return _WHOLE[(tid, sr_out)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def planar(out, n_ch):
    """interleaved f32 bytes -> [n_ch][n]"""
    return np.ascontiguousarray(out.view(np.float32).reshape(-1, n_ch).T)


def raw_export_at(handle, reqs, pfx="th_tm_", cap=None, fill=0xA5):
    """the C entry on a buffer with CANARY bytes of `fill` on each side -> (rc, whole buffer, infos, out_len)"""
    n = len(reqs)
    arr = (_ffi.ExportAtRequest * n)(*[api._export_at_request(r) for r in reqs])
    info = (_ffi.ExportInfo * n)()
    need = C.c_size_t()
    fn = getattr(_ffi.lib, pfx + "export_pcm_at")
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
            assert np.all(img[end: at] == 0), (i, o)
        else:
            assert end == out_len


def lengths_for(pair):
    t = ta.resample_tile(*pair)
    p = R.plan(*pair)
    taps, PM, PL = t["taps"], t["P"] * t["Mp"], t["P"] * t["Lp"]
    in_for = lambda n_out: n_out * p["M"] // p["L"]  # noqa: E731  (an input length whose output length is n_out or n_out + 1)
    ls = {1, 100, taps - 1, taps, taps + 1, PM - 1, PM + 1, 2 * PM - 1, 2 * PM + 1, in_for(PL - 1), in_for(PL + 1), in_for(2 * PL + 1)}
    if pair == (8000, 8001):
        ls = {1, 100, taps - 1, taps, taps + 1, 9000}  # (a tile is one period here: 9000 samples wrap past phase L - 1)
    return sorted(n for n in ls if 0 < n <= 40000)


@pytest.mark.parametrize("pair", PAIRS + SHAPE_PAIRS)
def test_f32_is_bit_identical_to_the_host_function(ctx, pair):
    """every track length of the module docstring, mono, as ONE batch of float exports; each de-interleaves to th_resample_f32"""
    sr_in, sr_out = pair
    ls = lengths_for(pair)
    assert any(n % 4 for n in ls)
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(100 + i, sr_in, _noise(1000 + i, n, 1)) for i, n in enumerate(ls)])
        rc, buf, infos, out_len = raw_export_at(m.handle, [(100 + i, sr_out, E.PCM_F32) for i in range(len(ls))])
        assert rc == _ffi.OK, _ffi.last_error()
        wants = []
        for i, n in enumerate(ls):
            y = ta.resample_f32(m.audio(100 + i, 0), sr_in, sr_out)
            assert y.size == ta.resample_n_out(n, sr_in, sr_out) == R.n_out(n, R.plan(*pair))
            wants.append((y.view(np.uint8), 0, 0))
            assert (infos[i]["sr"], infos[i]["n_channels"], infos[i]["sample_start"], infos[i]["sample_end"]) == (sr_out, 1, 0, y.size)
        check_image(buf, infos, wants, out_len)
    finally:
        m.close()


@pytest.mark.parametrize("tid, sr_out", [(1, 48000), (2, 44100), (3, 96000), (6, 48000), (7, 48000), (2, 16000)])
def test_channels_formats_and_dithers(tm, tid, sr_out):
    """1, 2, 3 and 6 channels (5003 / 3001 / 9001 samples): float bit-identical, S16 / S24 with both dithers byte-identical to the
    export's restatement applied to the resampled floats with index j"""
    sr, x = TRACKS[tid]
    y = whole(tm, tid, sr_out)
    n_ch, no = y.shape
    reqs, wants = [], []
    for fmt in FORMATS:
        for dith in DITHERS:
            for j0, j1 in ((0, no), (1, no - 2), (no // 2 - 1, no // 2 + 2)):
                seed = 100 * fmt + 10 * dith + j0 % 7
                reqs.append((tid, sr_out, fmt, dith, seed, sec_of(j0, sr_out), sec_of(j1, sr_out)))
                wants.append(E.pcm_bytes(fmt, dith, seed, y, j0, j1))
    rc, buf, infos, out_len = raw_export_at(tm.handle, reqs)
    assert rc == _ffi.OK, _ffi.last_error()
    for o in infos:
        assert (o["sr"], o["n_channels"], o["waveform_revision"]) == (sr_out, n_ch, tm.revisions()[0])
    check_image(buf, infos, wants, out_len)
    if sr_out >= sr:  # (the tracks peak at 1.1; a reduction may filter the peaks away)
        assert sum(o["n_clamped"] for o in infos) > 0
    out, info = tm.export_pcm_at([(tid, sr_out, E.PCM_F32)])
    assert np.array_equal(bits(planar(out, n_ch)), bits(y))


@pytest.mark.parametrize("pair_tid", [((44100, 48000), 1), ((48000, 44100), 2), ((96000, 48000), 7), ((8000, 8001), 8), ((48000, 16000), 3)])
def test_a_range_is_a_slice_of_the_whole_export(tm, pair_tid):
    (sr_in, sr_out), tid = pair_tid
    t = ta.resample_tile(sr_in, sr_out)
    n_ch = TRACKS[tid][1].shape[0]
    tile, F = t["P"] * t["Lp"], ta.export_chunk_frames(n_ch)
    y = whole(tm, tid, sr_out)
    no = y.shape[1]
    full, _ = tm.export_pcm_at([(tid, sr_out, E.PCM_S24, E.DITHER_TPDF, 5)])
    assert full.size == no * n_ch * 3
    starts = sorted({0, 1, 2, 3, 5, t["R"] - 1, t["R"], t["R"] + 1, tile - 1, tile, tile + 1, F - 1, F + 1} & set(range(no - 1)))
    for j0 in starts:
        for j1 in sorted({j0 + 1, min(no, j0 + tile + 3), no}):
            part, infos = tm.export_pcm_at([(tid, sr_out, E.PCM_S24, E.DITHER_TPDF, 5, sec_of(j0, sr_out), INF if j1 == no else sec_of(j1, sr_out))])
            assert (infos[0]["sample_start"], infos[0]["sample_end"]) == (j0, j1)
            assert np.array_equal(part, full[j0 * n_ch * 3: j1 * n_ch * 3]), (j0, j1)
        f32, _ = tm.export_pcm_at([(tid, sr_out, E.PCM_F32, 0, 0, sec_of(j0, sr_out), sec_of(min(no, j0 + 9), sr_out))])
        assert np.array_equal(bits(planar(f32, n_ch)), bits(y[:, j0: j0 + 9])), j0


def test_batch_of_mixed_rates(tm):
    """one call, several tables: requests at different rates, at the track's own rate, an id twice, an empty range"""
    reqs = [(2, 44100, E.PCM_S24, E.DITHER_TPDF, 1, sec_of(1, 44100), sec_of(2050, 44100)),
            (1, 48000, E.PCM_S16, E.DITHER_TPDF, 2),
            (2, 0, E.PCM_S16, E.DITHER_NONE, 3),                                           # no resampling
            (7, 48000, E.PCM_F32, 0, 0, 0.01, 0.05),
            (2, 96000, E.PCM_S16, E.DITHER_NONE, 3, sec_of(3, 96000), sec_of(4, 96000)),  # 4 bytes
            (3, 16000, E.PCM_S16, E.DITHER_TPDF, 5, 0.02, 0.02),                           # empty
            (2, 44100, E.PCM_S24, E.DITHER_TPDF, 1, sec_of(1, 44100), sec_of(2050, 44100)),  # the first one again
            (8, 8001, E.PCM_S24, E.DITHER_NONE, 9),
            (2, 48000, E.PCM_F32)]                                                         # sr_out = the track's rate
    rc, buf, infos, out_len = raw_export_at(tm.handle, reqs)
    assert rc == _ffi.OK, _ffi.last_error()
    wants = []
    for r, o in zip(reqs, infos):
        tid, sr_out, fmt, dith, seed, a, b = tuple(r) + (0, 0, 0.0, INF)[len(r) - 3:]
        sr = TRACKS[tid][0]
        if sr_out in (0, sr):
            y, eff = np.stack([tm.audio(tid, c) for c in range(TRACKS[tid][1].shape[0])]), sr
        else:
            y, eff = whole(tm, tid, sr_out), sr_out
        j0, j1 = E.sample_range(eff, y.shape[1], a, b)
        assert (o["sr"], o["sample_start"], o["sample_end"]) == (eff, j0, j1)
        wants.append(E.pcm_bytes(fmt, dith, seed, y, j0, j1))
        single, si = tm.export_pcm_at([r])
        assert np.array_equal(single, wants[-1][0])
        assert {k: v for k, v in si[0].items() if k != "offset"} == {k: v for k, v in o.items() if k != "offset"}
    check_image(buf, infos, wants, out_len)
    assert infos[5]["n_bytes"] == 0 and infos[4]["n_bytes"] == 4


def test_same_rate_is_the_plain_export(tm):
    """sr_out = 0 and sr_out = the track's rate: bytes, counts and infos of th_tm_export_pcm / _wav"""
    plain_reqs = [(2, E.PCM_S24, E.DITHER_TPDF, 1, sec_of(1, 48000), sec_of(2050, 48000)), (6, E.PCM_S16, E.DITHER_TPDF, 2), (1, E.PCM_F32),
                  (3, E.PCM_S16, E.DITHER_NONE, 0, 0.02, 0.02)]
    want, want_infos = tm.export_pcm(plain_reqs)
    for own in (False, True):
        reqs = [(r[0], TRACKS[r[0]][0] if own else 0) + tuple(r[1:]) for r in plain_reqs]
        out, infos = tm.export_pcm_at(reqs)
        assert np.array_equal(out, want) and infos == want_infos
    for tid, fmt in ((1, E.PCM_S24), (2, E.PCM_F32)):
        blob, info = tm.export_wav(tid, fmt, E.DITHER_TPDF, 9, 0.01, 0.09)
        for sr_out in (0, TRACKS[tid][0]):
            assert tm.export_wav_at(tid, sr_out, fmt, E.DITHER_TPDF, 9, 0.01, 0.09) == (blob, info)


@pytest.mark.parametrize("tid, sr_out, fmt, dith, j0, j1", [
    (1, 48000, E.PCM_S24, E.DITHER_TPDF, 0, None),   # 24-bit mono, odd length: a pad byte
    (2, 44100, E.PCM_S16, E.DITHER_TPDF, 3, 4100),
    (7, 48000, E.PCM_F32, E.DITHER_NONE, 1, None),   # float stereo: the data starts at byte 58
    (3, 96000, E.PCM_S16, E.DITHER_NONE, 10, 10),    # empty: a header-only file
])
def test_wav_images(tm, tid, sr_out, fmt, dith, j0, j1):
    y = whole(tm, tid, sr_out)
    n_ch, no = y.shape
    j1 = no if j1 is None else j1
    a, b = sec_of(j0, sr_out), (INF if j1 == no else sec_of(j1, sr_out))
    blob, info = tm.export_wav_at(tid, sr_out, fmt, dith, 42, a, b)
    assert blob == E.wav_file(fmt, dith, 42, sr_out, y, j0, j1)
    data, nc, nn = E.pcm_bytes(fmt, dith, 42, y, j0, j1)
    hdr, pad = ta.wav_header(fmt, sr_out, n_ch, j1 - j0)
    assert (info["offset"], info["n_bytes"], info["sample_start"], info["sample_end"]) == (len(hdr), data.size, j0, j1)
    assert (info["n_clamped"], info["n_nan"], info["sr"], info["n_channels"]) == (nc, nn, sr_out, n_ch)
    if fmt != E.PCM_F32:
        with wave.open(io.BytesIO(blob), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (n_ch, E.BYTES[fmt], sr_out, j1 - j0)
            assert w.readframes(j1 - j0) == data.tobytes()
    # the caller's buffer at an odd address, canaries around it; one byte too small writes nothing
    req = _ffi.ExportAtRequest(_ffi.ExportRequest(tid, 0, fmt, dith, 42, a, b), sr_out)
    one, need = _ffi.ExportInfo(), C.c_size_t()
    for shift in (1, 7):
        buf = np.full(len(blob) + 2 * CANARY + 8, 0xA5, np.uint8)
        lo = CANARY + shift
        rc = _ffi.lib.th_tm_export_wav_at(tm.handle, C.byref(req), buf.ctypes.data + lo, len(blob), C.byref(one), C.byref(need))
        assert rc == _ffi.OK, _ffi.last_error()
        assert buf[lo: lo + len(blob)].tobytes() == blob and np.all(buf[:lo] == 0xA5) and np.all(buf[lo + len(blob):] == 0xA5)
    small = np.full(len(blob) + CANARY, 0xA5, np.uint8)
    rc = _ffi.lib.th_tm_export_wav_at(tm.handle, C.byref(req), small.ctypes.data, len(blob) - 1, C.byref(one), C.byref(need))
    assert rc == _ffi.ERR_BUFFER_TOO_SMALL and need.value == len(blob) and np.all(small == 0xA5)


def test_which_and_revisions(ctx):
    m = ta.TrackManager(ctx)
    try:
        sr, x = TRACKS[2]
        m.add_tracks([(2, sr, x)])
        _, i0 = m.export_pcm_at([(2, 44100, E.PCM_S16)])
        assert i0[0]["waveform_revision"] == m.revisions()[0]
        m.set_common_guard_clipping(api.GUARD_CLIP)
        m.set_common_normalize(api.NORM_PEAK_DB, 6.0)  # a peak of +6 dB: the clip guard has work
        aud = [np.stack([m.audio(2, c, w) for c in range(2)]) for w in (0, 1, 2)]
        assert not np.array_equal(aud[0], aud[1]) and not np.array_equal(aud[1], aud[2]) and not np.array_equal(aud[0], aud[2])
        for which in (0, 1, 2):
            y = np.stack([ta.resample_f32(aud[which][c], sr, 44100) for c in range(2)])
            out, infos = m.export_pcm_at([(2, 44100, E.PCM_F32, 0, 0, 0.0, INF, which)])
            assert np.array_equal(bits(planar(out, 2)), bits(y)), which
            out, infos = m.export_pcm_at([(2, 44100, E.PCM_S16, E.DITHER_TPDF, 8, 0.0, INF, which)])
            data, nc, nn = E.pcm_bytes(E.PCM_S16, E.DITHER_TPDF, 8, y, 0, y.shape[1])
            assert np.array_equal(out, data) and (infos[0]["n_clamped"], infos[0]["n_nan"]) == (nc, nn)
            assert infos[0]["waveform_revision"] == m.revisions()[0] > i0[0]["waveform_revision"]
        _, iw = m.export_wav_at(2, 44100, E.PCM_S16, which=1)
        assert iw["waveform_revision"] == m.revisions()[0]
    finally:
        m.close()


@pytest.mark.parametrize("pair", [(44100, 48000), (96000, 48000)])
def test_one_nan_touches_only_the_windows_that_hold_it(ctx, pair):
    sr_in, sr_out = pair
    p = R.plan(*pair)
    L, M, K = p["L"], p["M"], p["K"]
    x = _noise(7, 6001, 2)
    bad = x.copy()
    at = 3000
    bad[1, at] = np.nan
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(1, sr_in, x), (2, sr_in, bad)])
        out, infos = m.export_pcm_at([(1, sr_out, E.PCM_F32), (2, sr_out, E.PCM_F32), (2, sr_out, E.PCM_S16, E.DITHER_TPDF, 3)])
        n_out = infos[0]["sample_end"]
        clean = planar(out[:infos[0]["n_bytes"]], 2)
        dirty = planar(out[infos[1]["offset"]: infos[1]["offset"] + infos[1]["n_bytes"]], 2)
        q = (np.arange(n_out) * M) // L
        holds = (q - K + 1 <= at) & (at <= q + K)  # the 2K-tap window [q - K + 1, q + K] contains the NaN
        assert 0 < holds.sum() < n_out
        assert np.array_equal(bits(dirty[0]), bits(clean[0]))
        assert np.array_equal(bits(dirty[1][~holds]), bits(clean[1][~holds]))
        assert np.all(np.isnan(dirty[1][holds]))
        assert infos[0]["n_nan"] == 0 and infos[1]["n_nan"] == infos[2]["n_nan"] == int(holds.sum())
    finally:
        m.close()


def test_errors_write_nothing(ctx, tm):
    good = (1, 48000, E.PCM_S16, E.DITHER_NONE, 0, 0.0, 0.01)
    nan = float("nan")
    cases = [((99, 48000, E.PCM_S16), _ffi.ERR_NOT_FOUND),
             ((1, 48000, 3), _ffi.ERR_INVALID_ARG),                                  # unknown format
             ((1, 48000, E.PCM_S16, 2), _ffi.ERR_INVALID_ARG),                       # unknown dither
             ((1, 48000, E.PCM_S16, 0, 0, 0.0, INF, 3), _ffi.ERR_INVALID_ARG),       # unknown which
             ((1, 48000, E.PCM_S16, 0, 0, -0.5, INF), _ffi.ERR_INVALID_ARG),
             ((1, 48000, E.PCM_S16, 0, 0, nan, INF), _ffi.ERR_INVALID_ARG),
             ((1, 48000, E.PCM_S16, 0, 0, 0.0, nan), _ffi.ERR_INVALID_ARG),
             ((1, 48000, E.PCM_S16, 0, 0, INF, INF), _ffi.ERR_INVALID_ARG),
             ((1, 48000, E.PCM_S16, 0, 0, 0.02, 0.01), _ffi.ERR_INVALID_ARG),
             ((7, 95999, E.PCM_S16), _ffi.ERR_UNSUPPORTED),                          # L 2K beyond TH_RESAMPLE_MAX_COEFS
             ((7, 1000, E.PCM_F32), _ffi.ERR_UNSUPPORTED)]                           # reduction by 96: beyond TH_RESAMPLE_MAX_TAPS
    for bad, code in cases:
        for reqs in ([bad], [good, bad], [good, bad, (98, 48000, E.PCM_S16)]):
            rc, buf, _, _ = raw_export_at(tm.handle, reqs, cap=4096)
            assert rc == code, (bad, rc, _ffi.last_error())
            assert np.all(buf == 0xA5), bad
        req = api._export_at_request(bad)
        buf = np.full(4096, 0xA5, np.uint8)
        need = C.c_size_t()
        assert _ffi.lib.th_tm_export_wav_at(tm.handle, C.byref(req), buf.ctypes.data, buf.size, None, C.byref(need)) == code
        assert np.all(buf == 0xA5)
    rc, buf, _, _ = raw_export_at(tm.handle, [good, (7, 95999, E.PCM_S16), (98, 48000, E.PCM_S16)], cap=4096)
    assert rc == _ffi.ERR_UNSUPPORTED and np.all(buf == 0xA5)  # the first faulty request decides
    # 192000 -> 2000, the issue's second refused pair
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(1, 192000, _noise(1, 500, 1))])
        rc, buf, _, _ = raw_export_at(m.handle, [(1, 2000, E.PCM_S16)], cap=4096)
        assert rc == _ffi.ERR_UNSUPPORTED and np.all(buf == 0xA5)
        out, infos = m.export_pcm_at([(1, 3000, E.PCM_F32)])  # reduction by exactly 64: the limit itself
        assert np.array_equal(bits(out.view(np.float32)), bits(ta.resample_f32(m.audio(1, 0), 192000, 3000)))
    finally:
        m.close()
    # the size query, a buffer one byte short, an empty batch, an empty range
    reqs = [(2, 44100, E.PCM_S24, E.DITHER_TPDF, 1, sec_of(1, 44100), sec_of(100, 44100)), (3, 96000, E.PCM_S16)]
    n3 = ta.resample_n_out(5003, 48000, 96000)
    arr = (_ffi.ExportAtRequest * 2)(*[api._export_at_request(r) for r in reqs])
    info, need = (_ffi.ExportInfo * 2)(), C.c_size_t()
    assert _ffi.lib.th_tm_export_pcm_at(tm.handle, arr, 2, None, 0, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert (info[0].offset, info[0].n_bytes, info[0].sample_start, info[0].sample_end, info[0].sr) == (0, 99 * 6, 1, 100, 44100)
    assert (info[1].offset, info[1].n_bytes, info[1].sample_start, info[1].sample_end, info[1].sr) == (608, n3 * 6, 0, n3, 96000)
    assert need.value == 608 + n3 * 6 and (info[0].n_clamped, info[0].n_nan) == (0, 0)
    rc, buf, infos, out_len = raw_export_at(tm.handle, reqs, cap=need.value - 1)
    assert rc == _ffi.ERR_BUFFER_TOO_SMALL and np.all(buf == 0xA5) and out_len == need.value
    assert _ffi.lib.th_tm_export_pcm_at(tm.handle, None, 0, None, 0, None, C.byref(need)) == _ffi.OK and need.value == 0
    out, infos = tm.export_pcm_at([(3, 16000, E.PCM_S16, 0, 0, 0.05, 0.05)])
    assert out.size == 0 and infos[0]["n_bytes"] == 0 and infos[0]["sr"] == 16000
    assert (infos[0]["sample_start"], infos[0]["sample_end"]) == E.sample_range(16000, ta.resample_n_out(5003, 48000, 16000), 0.05, 0.05)


def test_a_request_of_more_than_two_pieces(ctx):
    """six channels, 16 bit, 8000 -> 48000 Hz: the output just exceeds two pieces of TH_EXPORT_PIECE_BYTES, so the call runs three
    pairs of launches through the slot's scratch and the two staging buffers; the second call reuses them.  Windows at the start,
    around both piece boundaries and at the end are compared with the host function (float) and the export's restatement
    (dithered 16 bit); the two calls are compared in full."""
    n_ch, sr_in, sr_out = 6, 8000, 48000
    frames_per_piece = api.EXPORT_PIECE_BYTES // (2 * n_ch)
    n_in = (2 * frames_per_piece + 5000) // 6 + 1
    x = _noise(11, n_in, n_ch, peak=1.05)
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(1, sr_in, x)])
        no = ta.resample_n_out(n_in, sr_in, sr_out)
        assert no * 2 * n_ch > 2 * api.EXPORT_PIECE_BYTES
        outs = [m.export_pcm_at([(1, sr_out, E.PCM_S16, E.DITHER_TPDF, 77)]) for _ in range(2)]
        assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
        out, infos = outs[0]
        assert infos[0]["n_bytes"] == out.size == no * 2 * n_ch and infos[0]["n_clamped"] > 0
        aud = np.stack([m.audio(1, c) for c in range(n_ch)])
        for a, b in ((0, 3000), (frames_per_piece - 3000, frames_per_piece + 1000), (2 * frames_per_piece - 3000, 2 * frames_per_piece + 1000), (no - 3000, no)):
            y = np.stack([ta.resample_f32(aud[c], sr_in, sr_out, a, b - a) for c in range(n_ch)])
            want = np.empty((b - a, n_ch, 2), np.uint8)
            for c in range(n_ch):
                q, _, _ = E.quantize(E.PCM_S16, E.DITHER_TPDF, 77, c, a, y[c])
                want[:, c, :] = (q & 0xFFFF).astype("<u2").view(np.uint8).reshape(-1, 2)
            assert np.array_equal(out[a * 2 * n_ch: b * 2 * n_ch], want.reshape(-1)), (a, b)
            f32, _ = m.export_pcm_at([(1, sr_out, E.PCM_F32, 0, 0, sec_of(a, sr_out), INF if b == no else sec_of(b, sr_out))])
            assert np.array_equal(bits(planar(f32, n_ch)), bits(y)), (a, b)
    finally:
        m.close()


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_tmg_gives_the_bytes_and_infos_of_tm(tm, devices):
    reqs = [(2, 44100, E.PCM_S24, E.DITHER_TPDF, 1, sec_of(1, 44100), sec_of(2050, 44100)), (1, 48000, E.PCM_S16, E.DITHER_TPDF, 2),
            (7, 48000, E.PCM_F32), (6, 48000, E.PCM_S24, E.DITHER_NONE, 4, sec_of(3, 48000), sec_of(400, 48000)), (3, 0, E.PCM_S16, E.DITHER_TPDF, 5),
            (8, 8001, E.PCM_S16, E.DITHER_NONE, 0), (2, 96000, E.PCM_S16), (3, 16000, E.PCM_F32)]
    g = ta.MultiTrackManager(devices)
    try:
        g.add_tracks([(i, sr, x) for i, (sr, x) in sorted(TRACKS.items())])
        if len(devices) > 1:
            assert len({g.device_of(i) for i in TRACKS}) == 2
        rc, buf, infos, out_len = raw_export_at(tm.handle, reqs)
        rcg, bufg, infosg, out_leng = raw_export_at(g.handle, reqs, pfx="th_tmg_")
        assert rc == rcg == _ffi.OK, _ffi.last_error()
        assert out_len == out_leng and np.array_equal(buf, bufg)
        strip = lambda d: {k: v for k, v in d.items() if k != "waveform_revision"}  # noqa: E731
        assert [strip(o) for o in infos] == [strip(o) for o in infosg]
        assert all(o["waveform_revision"] == g.revisions()[0] for o in infosg)
        for tid, sr_out, fmt in ((1, 48000, E.PCM_S24), (2, 44100, E.PCM_F32)):
            assert g.export_wav_at(tid, sr_out, fmt, E.DITHER_TPDF, 9)[0] == tm.export_wav_at(tid, sr_out, fmt, E.DITHER_TPDF, 9)[0]
        with pytest.raises(ta.ThError) as e:
            g.export_pcm_at([(1, 48000, E.PCM_S16), (99, 48000, E.PCM_S16)])
        assert e.value.code == _ffi.ERR_NOT_FOUND
        with pytest.raises(ta.ThError) as e:
            g.export_wav_at(7, 95999, E.PCM_S16)
        assert e.value.code == _ffi.ERR_UNSUPPORTED
    finally:
        g.close()
