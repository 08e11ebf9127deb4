"""Band-limited export (th_tm_export_pcm_band / th_tm_export_wav_band and the th_tmg twins) on the GPU.

Reference: th_band_f32 (the host restatement of the kernel's sum: tests/test_band_host.py holds it against numpy f64) applied to the
samples th_tm_copy_audio returns, and for the integer formats tests/export_ref.py applied to those floats with the absolute index j as
the dither index.  Every comparison is bit- or byte-exact; the counts are exact.

The kernel's tile is api.BAND_TILE = 2048 outputs of one channel, walked in blocks of api.BAND_TAP_BLOCK = 64 taps, so K = 31, 32, 33 are
a row shorter than one block (2K = 2 mod 4), exactly one and one block plus two taps; K = 64, 65, 66, 256, 1024 are several blocks with
and without the two-tap end.  Track lengths: 1, 100, around the filter length (2K - 1, 2K + 1), around one tile and just over two.
Tracks are at 8 kHz so that the transition widths, and with them the filters, stay small."""
import ctypes as C
import io
import wave

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api
from tests import band_ref as B
from tests import export_ref as E

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
CANARY = 64
SR = 8000
TILE, TAP_BLOCK = api.BAND_TILE, api.BAND_TAP_BLOCK
FORMATS = (E.PCM_S16, E.PCM_S24, E.PCM_F32)
DITHERS = (E.DITHER_NONE, E.DITHER_TPDF)
PASS, STOP = ta.BAND_PASS, ta.BAND_STOP
# (mode, f_lo, f_hi): a band and its complement, a low-pass and a high-pass
FILTERS = [(PASS, 1000.0, 2500.0), (STOP, 1000.0, 2500.0), (PASS, 0.0, 1500.0), (PASS, 1500.0, INF)]


def _noise(seed, n, channels, peak=0.9):
    return (np.random.default_rng(seed).uniform(-peak, peak, (channels, n))).astype(np.float32)


TRACKS = {1: _noise(10, 5003, 1, 1.1), 2: _noise(20, 5003, 2, 1.1), 3: _noise(30, 5003, 3, 1.1), 6: _noise(60, 3001, 6, 1.1)}


def sec_of(s, sr=SR):
    """a time whose first sample at or after it is s"""
    t = s / sr
    while E.sample_range(sr, 10 ** 12, t, INF)[0] != s:
        t = np.nextafter(t, 0.0)
    return float(t)


def band(K, mode=PASS, f_lo=1000.0, f_hi=2500.0, sr=SR):
    """(mode, f_lo_hz, f_hi_hz, trans_hz) of a request whose filter has K half taps"""
    return (mode, f_lo, f_hi, B.trans_for(sr, K))


def row_of(bd, sr=SR):
    """the f32 row of a request's band, or None for the identity"""
    p = ta.band_plan(sr, *bd)
    return ta.band_coefs(sr, p)[1] if p["half_taps"] else None


@pytest.fixture(scope="module")
def ctx():
    c = ta.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tm(ctx):
    m = ta.TrackManager(ctx)
    m.add_tracks([(i, SR, x) for i, x in sorted(TRACKS.items())])
    yield m
    m.close()


_WHOLE = {}


def whole(m, tid, bd):
    """[n_ch][n] f32: th_band_f32 of the module manager's audio (th_tm_copy_audio), computed once and left unchanged"""
    if (tid, bd) not in _WHOLE:
        row = row_of(bd)
        aud = [m.audio(tid, c) for c in range(TRACKS[tid].shape[0])]
        y = np.stack([a if row is None else ta.band_f32(a, row) for a in aud])
        y.setflags(write=False)
        _WHOLE[(tid, bd)] = y
    return _WHOLE[(tid, bd)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def planar(out, n_ch):
    """interleaved f32 bytes -> [n_ch][n]"""
    return np.ascontiguousarray(out.view(np.float32).reshape(-1, n_ch).T)


def raw_export_band(handle, reqs, pfx="th_tm_", cap=None, fill=0xA5):
    """the C entry on a buffer with CANARY bytes of `fill` on each side -> (rc, whole buffer, infos, out_len)"""
    n = len(reqs)
    arr = (_ffi.ExportBandRequest * n)(*[api._export_band_request(r) for r in reqs])
    info = (_ffi.ExportInfo * n)()
    need = C.c_size_t()
    fn = getattr(_ffi.lib, pfx + "export_pcm_band")
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


@pytest.mark.parametrize("K", [64, 65, 66, 256, 1024, TAP_BLOCK // 2 - 1, TAP_BLOCK // 2, TAP_BLOCK // 2 + 1])
def test_f32_is_bit_identical_to_the_host_function(ctx, K):
    """every track length of the module docstring, mono, under each of the four filters as ONE batch of float exports; each is
    th_band_f32 of the track"""
    ls = sorted({1, 100, 2 * K - 1, 2 * K + 1, TILE - 1, TILE + 1, 2 * TILE + 1})
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(100 + i, SR, _noise(1000 + i, n, 1)) for i, n in enumerate(ls)])
        aud = [m.audio(100 + i, 0) for i in range(len(ls))]
        for mode, f_lo, f_hi in FILTERS:
            bd = band(K, mode, f_lo, f_hi)
            p = ta.band_plan(SR, *bd)
            assert p["half_taps"] == K and p["f_hi_hz"] == min(f_hi, SR / 2)
            row = ta.band_coefs(SR, p)[1]
            rc, buf, infos, out_len = raw_export_band(m.handle, [(100 + i,) + bd + (E.PCM_F32,) for i in range(len(ls))])
            assert rc == _ffi.OK, _ffi.last_error()
            wants = []
            for i, n in enumerate(ls):
                y = ta.band_f32(aud[i], row)
                wants.append((y.view(np.uint8), 0, 0))
                assert (infos[i]["sr"], infos[i]["n_channels"], infos[i]["sample_start"], infos[i]["sample_end"]) == (SR, 1, 0, n)
            check_image(buf, infos, wants, out_len)
    finally:
        m.close()


def test_the_longest_row(ctx):
    """K = 32768 (a 4.6875 Hz transition at 48 kHz) on 70 000 samples: 2 000 outputs whose windows reach past the track's start"""
    sr, K, n = 48000, 32768, 70000
    bd = (PASS, 50.0, 100.0, 4.6875)
    p = ta.band_plan(sr, *bd)
    assert p["half_taps"] == K == api.BAND_MAX_TAPS // 2
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(1, sr, _noise(5, n, 1))])
        row = ta.band_coefs(sr, p)[1]
        for j0 in (1000, n - 2000):
            out, infos = m.export_pcm_band([(1,) + bd + (E.PCM_F32, 0, 0, sec_of(j0, sr), sec_of(j0 + 2000, sr) if j0 + 2000 < n else INF)])
            assert (infos[0]["sample_start"], infos[0]["sample_end"]) == (j0, j0 + 2000)
            assert np.array_equal(bits(out.view(np.float32)), bits(ta.band_f32(m.audio(1, 0), row, j0, 2000))), j0
    finally:
        m.close()


@pytest.mark.parametrize("tid, K", [(1, 64), (2, 65), (3, 66), (6, 33)])
def test_channels_formats_and_dithers(tm, tid, K):
    """1, 2, 3 and 6 channels (5003 / 3001 samples): float bit-identical, S16 / S24 with both dithers byte-identical to the export's
    restatement applied to the filtered floats with index j"""
    bd = band(K, STOP if tid == 2 else PASS)
    y = whole(tm, tid, bd)
    n_ch, n = y.shape
    reqs, wants = [], []
    for fmt in FORMATS:
        for dith in DITHERS:
            for j0, j1 in ((0, n), (1, n - 2), (n // 2 - 1, n // 2 + 2)):
                seed = 100 * fmt + 10 * dith + j0 % 7
                reqs.append((tid,) + bd + (fmt, dith, seed, sec_of(j0), sec_of(j1)))
                wants.append(E.pcm_bytes(fmt, dith, seed, y, j0, j1))
    rc, buf, infos, out_len = raw_export_band(tm.handle, reqs)
    assert rc == _ffi.OK, _ffi.last_error()
    for o in infos:
        assert (o["sr"], o["n_channels"], o["waveform_revision"]) == (SR, n_ch, tm.revisions()[0])
    check_image(buf, infos, wants, out_len)
    out, info = tm.export_pcm_band([(tid,) + bd + (E.PCM_F32,)])
    assert np.array_equal(bits(planar(out, n_ch)), bits(y))


@pytest.mark.parametrize("tid, K", [(1, 64), (2, 65), (6, 256)])
def test_a_range_is_a_slice_of_the_whole_export(tm, tid, K):
    bd = band(K)
    n_ch = TRACKS[tid].shape[0]
    F = ta.export_chunk_frames(n_ch)
    y = whole(tm, tid, bd)
    n = y.shape[1]
    full, _ = tm.export_pcm_band([(tid,) + bd + (E.PCM_S24, E.DITHER_TPDF, 5)])
    assert full.size == n * n_ch * 3
    R = TILE // 256
    starts = sorted({0, 1, 2, 3, 5, R - 1, R, R + 1, TILE - 1, TILE, TILE + 1, F - 1, F, F + 1} & set(range(n - 1)))
    for j0 in starts:
        for j1 in sorted({j0 + 1, min(n, j0 + TILE + 3), n}):
            part, infos = tm.export_pcm_band([(tid,) + bd + (E.PCM_S24, E.DITHER_TPDF, 5, sec_of(j0), INF if j1 == n else sec_of(j1))])
            assert (infos[0]["sample_start"], infos[0]["sample_end"]) == (j0, j1)
            assert np.array_equal(part, full[j0 * n_ch * 3: j1 * n_ch * 3]), (j0, j1)
        f32, _ = tm.export_pcm_band([(tid,) + bd + (E.PCM_F32, 0, 0, sec_of(j0), sec_of(min(n, j0 + 9)))])
        assert np.array_equal(bits(planar(f32, n_ch)), bits(y[:, j0: j0 + 9])), j0


def test_batch_of_mixed_filters(tm):
    """one call, several rows: requests under different filters and lengths, plain ones (the identity), an id twice, an empty range"""
    ident = (PASS, 0.0, INF, 0.0)
    reqs = [(2,) + band(64) + (E.PCM_S24, E.DITHER_TPDF, 1, sec_of(1), sec_of(2050)),
            (1,) + band(65, STOP) + (E.PCM_S16, E.DITHER_TPDF, 2),
            (2,) + ident + (E.PCM_S16, E.DITHER_NONE, 3),                      # no filter
            (6,) + band(256, PASS, 0.0, 1500.0) + (E.PCM_F32, 0, 0, 0.01, 0.05),
            (2,) + band(64) + (E.PCM_S16, E.DITHER_NONE, 3, sec_of(3), sec_of(4)),  # 4 bytes, the first filter again
            (3,) + band(66) + (E.PCM_S16, E.DITHER_TPDF, 5, 0.02, 0.02),       # empty
            (2,) + band(64) + (E.PCM_S24, E.DITHER_TPDF, 1, sec_of(1), sec_of(2050)),  # the first one again
            (3,) + band(64, PASS, 1500.0, INF) + (E.PCM_S24, E.DITHER_NONE, 9),  # K of the first, another row
            (2, PASS, 0.0, 4000.0, 400.0, E.PCM_F32)]                          # the identity with a width
    rc, buf, infos, out_len = raw_export_band(tm.handle, reqs)
    assert rc == _ffi.OK, _ffi.last_error()
    wants = []
    for r, o in zip(reqs, infos):
        tid, bd = r[0], tuple(r[1:5])
        fmt, dith, seed, a, b = tuple(r[5:]) + (0, 0, 0.0, INF)[len(r) - 6:]
        y = whole(tm, tid, bd)
        j0, j1 = E.sample_range(SR, y.shape[1], a, b)
        assert (o["sr"], o["sample_start"], o["sample_end"]) == (SR, j0, j1)
        wants.append(E.pcm_bytes(fmt, dith, seed, y, j0, j1))
        single, si = tm.export_pcm_band([r])
        assert np.array_equal(single, wants[-1][0])
        assert {k: v for k, v in si[0].items() if k != "offset"} == {k: v for k, v in o.items() if k != "offset"}
    check_image(buf, infos, wants, out_len)
    assert infos[5]["n_bytes"] == 0 and infos[4]["n_bytes"] == 4


def test_identity_is_the_plain_export(tm):
    """TH_BAND_PASS of [0, sr / 2]: bytes, counts and infos of th_tm_export_pcm / _wav"""
    plain_reqs = [(2, E.PCM_S24, E.DITHER_TPDF, 1, sec_of(1), sec_of(2050)), (6, E.PCM_S16, E.DITHER_TPDF, 2), (1, E.PCM_F32),
                  (3, E.PCM_S16, E.DITHER_NONE, 0, 0.02, 0.02)]
    want, want_infos = tm.export_pcm(plain_reqs)
    for ident in ((PASS, 0.0, INF, 0.0), (PASS, 0.0, SR / 2.0, 123.0), (PASS, 0.0, 1e9, 1e-9)):
        out, infos = tm.export_pcm_band([(r[0],) + ident + tuple(r[1:]) for r in plain_reqs])
        assert np.array_equal(out, want) and infos == want_infos
    for tid, fmt in ((1, E.PCM_S24), (2, E.PCM_F32)):
        blob, info = tm.export_wav(tid, fmt, E.DITHER_TPDF, 9, 0.01, 0.09)
        assert tm.export_wav_band(tid, PASS, 0.0, INF, 0.0, fmt, E.DITHER_TPDF, 9, 0.01, 0.09) == (blob, info)


@pytest.mark.parametrize("tid, K, fmt, dith, j0, j1", [
    (1, 64, E.PCM_S24, E.DITHER_TPDF, 0, None),   # 24-bit mono, odd length: a pad byte
    (2, 65, E.PCM_S16, E.DITHER_TPDF, 3, 4100),
    (2, 65, E.PCM_F32, E.DITHER_NONE, 1, None),   # float stereo: the data starts at byte 58
    (3, 66, E.PCM_S16, E.DITHER_NONE, 10, 10),    # empty: a header-only file
])
def test_wav_images(tm, tid, K, fmt, dith, j0, j1):
    bd = band(K, STOP if tid == 2 else PASS)
    y = whole(tm, tid, bd)
    n_ch, n = y.shape
    j1 = n if j1 is None else j1
    a, b = sec_of(j0), (INF if j1 == n else sec_of(j1))
    blob, info = tm.export_wav_band(tid, *bd, fmt, dith, 42, a, b)
    assert blob == E.wav_file(fmt, dith, 42, SR, y, j0, j1)
    data, nc, nn = E.pcm_bytes(fmt, dith, 42, y, j0, j1)
    hdr, pad = ta.wav_header(fmt, SR, n_ch, j1 - j0)
    assert (info["offset"], info["n_bytes"], info["sample_start"], info["sample_end"]) == (len(hdr), data.size, j0, j1)
    assert (info["n_clamped"], info["n_nan"], info["sr"], info["n_channels"]) == (nc, nn, SR, n_ch)
    if fmt != E.PCM_F32:
        with wave.open(io.BytesIO(blob), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (n_ch, E.BYTES[fmt], SR, j1 - j0)
            assert w.readframes(j1 - j0) == data.tobytes()
    # the caller's buffer at an odd address, canaries around it; one byte too small writes nothing
    req = _ffi.ExportBandRequest(_ffi.ExportRequest(tid, 0, fmt, dith, 42, a, b), *bd)
    one, need = _ffi.ExportInfo(), C.c_size_t()
    for shift in (1, 7):
        buf = np.full(len(blob) + 2 * CANARY + 8, 0xA5, np.uint8)
        lo = CANARY + shift
        rc = _ffi.lib.th_tm_export_wav_band(tm.handle, C.byref(req), buf.ctypes.data + lo, len(blob), C.byref(one), C.byref(need))
        assert rc == _ffi.OK, _ffi.last_error()
        assert buf[lo: lo + len(blob)].tobytes() == blob and np.all(buf[:lo] == 0xA5) and np.all(buf[lo + len(blob):] == 0xA5)
    small = np.full(len(blob) + CANARY, 0xA5, np.uint8)
    rc = _ffi.lib.th_tm_export_wav_band(tm.handle, C.byref(req), small.ctypes.data, len(blob) - 1, C.byref(one), C.byref(need))
    assert rc == _ffi.ERR_BUFFER_TOO_SMALL and need.value == len(blob) and np.all(small == 0xA5)


def test_which_and_revisions(ctx):
    m = ta.TrackManager(ctx)
    try:
        x = TRACKS[2]
        bd = band(64)
        row = row_of(bd)
        m.add_tracks([(2, SR, x)])
        _, i0 = m.export_pcm_band([(2,) + bd + (E.PCM_S16,)])
        assert i0[0]["waveform_revision"] == m.revisions()[0]
        m.set_common_guard_clipping(api.GUARD_CLIP)
        m.set_common_normalize(api.NORM_PEAK_DB, 6.0)  # a peak of +6 dB: the clip guard has work
        aud = [np.stack([m.audio(2, c, w) for c in range(2)]) for w in (0, 1, 2)]
        assert not np.array_equal(aud[0], aud[1]) and not np.array_equal(aud[1], aud[2]) and not np.array_equal(aud[0], aud[2])
        for which in (0, 1, 2):
            y = np.stack([ta.band_f32(aud[which][c], row) for c in range(2)])
            out, infos = m.export_pcm_band([(2,) + bd + (E.PCM_F32, 0, 0, 0.0, INF, which)])
            assert np.array_equal(bits(planar(out, 2)), bits(y)), which
            out, infos = m.export_pcm_band([(2,) + bd + (E.PCM_S16, E.DITHER_TPDF, 8, 0.0, INF, which)])
            data, nc, nn = E.pcm_bytes(E.PCM_S16, E.DITHER_TPDF, 8, y, 0, y.shape[1])
            assert np.array_equal(out, data) and (infos[0]["n_clamped"], infos[0]["n_nan"]) == (nc, nn)
            assert infos[0]["waveform_revision"] == m.revisions()[0] > i0[0]["waveform_revision"]
        _, iw = m.export_wav_band(2, *bd, E.PCM_S16, which=1)
        assert iw["waveform_revision"] == m.revisions()[0]
    finally:
        m.close()


@pytest.mark.parametrize("K", [64, 65])
def test_one_nan_makes_exactly_2k_outputs_nan(ctx, K):
    bd = band(K)
    x = _noise(7, 6001, 2)
    bad = x.copy()
    at = 3000
    bad[1, at] = np.nan
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(1, SR, x), (2, SR, bad)])
        out, infos = m.export_pcm_band([(1,) + bd + (E.PCM_F32,), (2,) + bd + (E.PCM_F32,), (2,) + bd + (E.PCM_S16, E.DITHER_TPDF, 3)])
        clean = planar(out[:infos[0]["n_bytes"]], 2)
        dirty = planar(out[infos[1]["offset"]: infos[1]["offset"] + infos[1]["n_bytes"]], 2)
        j = np.arange(6001)
        holds = (j >= at - K) & (j <= at + K - 1)  # the zero tap included
        assert holds.sum() == 2 * K
        assert np.array_equal(bits(dirty[0]), bits(clean[0]))
        assert np.array_equal(bits(dirty[1][~holds]), bits(clean[1][~holds]))
        assert np.all(np.isnan(dirty[1][holds]))
        assert infos[0]["n_nan"] == 0 and infos[1]["n_nan"] == infos[2]["n_nan"] == 2 * K
    finally:
        m.close()


def test_errors_write_nothing(tm):
    b64 = band(64)
    good = (1,) + b64 + (E.PCM_S16, E.DITHER_NONE, 0, 0.0, 0.01)
    cases = [((99,) + b64 + (E.PCM_S16,), _ffi.ERR_NOT_FOUND),
             ((1,) + b64 + (3,), _ffi.ERR_INVALID_ARG),                                   # unknown format
             ((1,) + b64 + (E.PCM_S16, 2), _ffi.ERR_INVALID_ARG),                         # unknown dither
             ((1,) + b64 + (E.PCM_S16, 0, 0, 0.0, INF, 3), _ffi.ERR_INVALID_ARG),         # unknown which
             ((1,) + b64 + (E.PCM_S16, 0, 0, -0.5, INF), _ffi.ERR_INVALID_ARG),
             ((1,) + b64 + (E.PCM_S16, 0, 0, NAN, INF), _ffi.ERR_INVALID_ARG),
             ((1,) + b64 + (E.PCM_S16, 0, 0, 0.02, 0.01), _ffi.ERR_INVALID_ARG),
             ((1, PASS, NAN, 1000.0, 0.0, E.PCM_S16), _ffi.ERR_INVALID_ARG),               # a NaN edge
             ((1, PASS, 100.0, NAN, 0.0, E.PCM_S16), _ffi.ERR_INVALID_ARG),
             ((1, PASS, -1.0, 1000.0, 0.0, E.PCM_S16), _ffi.ERR_INVALID_ARG),              # f_lo < 0
             ((1, PASS, 1000.0, 1000.0, 0.0, E.PCM_S16), _ffi.ERR_INVALID_ARG),            # f_lo >= f_hi
             ((1, PASS, 4000.0, INF, 0.0, E.PCM_S16), _ffi.ERR_INVALID_ARG),               # ... after the clamp
             ((1, 2, 100.0, 1000.0, 0.0, E.PCM_S16), _ffi.ERR_INVALID_ARG),                # unknown mode
             ((1, PASS, 100.0, 1000.0, NAN, E.PCM_S16), _ffi.ERR_INVALID_ARG),             # trans_hz
             ((1, PASS, 100.0, 1000.0, -1.0, E.PCM_S16), _ffi.ERR_INVALID_ARG),
             ((1, PASS, 100.0, 1000.0, 4000.5, E.PCM_S16), _ffi.ERR_INVALID_ARG),
             ((1, STOP, 0.0, INF, 0.0, E.PCM_S16), _ffi.ERR_INVALID_ARG),                  # TH_BAND_STOP of the whole band
             ((1, PASS, 100.0, 1000.0, 0.78, E.PCM_S16), _ffi.ERR_UNSUPPORTED)]            # narrower than 16 x 8000 / (5 x 32768) = 0.78125 Hz
    for bad, code in cases:
        for reqs in ([bad], [good, bad], [good, bad, (98,) + b64 + (E.PCM_S16,)]):
            rc, buf, _, _ = raw_export_band(tm.handle, reqs, cap=4096)
            assert rc == code, (bad, rc, _ffi.last_error())
            assert np.all(buf == 0xA5), bad
        req = api._export_band_request(bad)
        buf = np.full(4096, 0xA5, np.uint8)
        need = C.c_size_t()
        assert _ffi.lib.th_tm_export_wav_band(tm.handle, C.byref(req), buf.ctypes.data, buf.size, None, C.byref(need)) == code
        assert np.all(buf == 0xA5)
    rc, buf, _, _ = raw_export_band(tm.handle, [good, (1, PASS, 100.0, 1000.0, 0.78, E.PCM_S16), (98,) + b64 + (E.PCM_S16,)], cap=4096)
    assert rc == _ffi.ERR_UNSUPPORTED and np.all(buf == 0xA5)  # the first faulty request decides
    # the limit itself: 0.78125 Hz is K = 32768
    out, infos = tm.export_pcm_band([(1, PASS, 100.0, 1000.0, 0.78125, E.PCM_F32, 0, 0, 0.0, sec_of(8))])
    row = ta.band_coefs(SR, ta.band_plan(SR, PASS, 100.0, 1000.0, 0.78125))[1]
    assert row.size == api.BAND_MAX_TAPS and np.array_equal(bits(out.view(np.float32)), bits(ta.band_f32(tm.audio(1, 0), row, 0, 8)))
    # the size query, a buffer one byte short, an empty batch, an empty range
    reqs = [(2,) + b64 + (E.PCM_S24, E.DITHER_TPDF, 1, sec_of(1), sec_of(100)), (3,) + band(65) + (E.PCM_S16,)]
    arr = (_ffi.ExportBandRequest * 2)(*[api._export_band_request(r) for r in reqs])
    info, need = (_ffi.ExportInfo * 2)(), C.c_size_t()
    assert _ffi.lib.th_tm_export_pcm_band(tm.handle, arr, 2, None, 0, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert (info[0].offset, info[0].n_bytes, info[0].sample_start, info[0].sample_end, info[0].sr) == (0, 99 * 6, 1, 100, SR)
    assert (info[1].offset, info[1].n_bytes, info[1].sample_start, info[1].sample_end, info[1].sr) == (608, 5003 * 6, 0, 5003, SR)
    assert need.value == 608 + 5003 * 6 and (info[0].n_clamped, info[0].n_nan) == (0, 0)
    rc, buf, infos, out_len = raw_export_band(tm.handle, reqs, cap=need.value - 1)
    assert rc == _ffi.ERR_BUFFER_TOO_SMALL and np.all(buf == 0xA5) and out_len == need.value
    assert _ffi.lib.th_tm_export_pcm_band(tm.handle, None, 0, None, 0, None, C.byref(need)) == _ffi.OK and need.value == 0
    out, infos = tm.export_pcm_band([(3,) + b64 + (E.PCM_S16, 0, 0, 0.05, 0.05)])
    assert out.size == 0 and infos[0]["n_bytes"] == 0 and infos[0]["sr"] == SR
    assert (infos[0]["sample_start"], infos[0]["sample_end"]) == E.sample_range(SR, 5003, 0.05, 0.05)


def test_a_request_of_more_than_two_pieces(ctx):
    """six channels, 16 bit: the output just exceeds two pieces of TH_EXPORT_PIECE_BYTES, so the call runs three pairs of launches
    through the slot's scratch and the two staging buffers; the second call reuses them.  Windows at the start, around both piece
    boundaries and at the end are compared with the host function (float) and the export's restatement (dithered 16 bit); the two
    calls are compared in full."""
    n_ch, K = 6, 64
    bd = band(K)
    row = row_of(bd)
    frames_per_piece = api.EXPORT_PIECE_BYTES // (2 * n_ch)
    n = 2 * frames_per_piece + 5000
    x = _noise(11, n, n_ch, peak=1.3)
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(1, SR, x)])
        assert n * 2 * n_ch > 2 * api.EXPORT_PIECE_BYTES
        outs = [m.export_pcm_band([(1,) + bd + (E.PCM_S16, E.DITHER_TPDF, 77)]) for _ in range(2)]
        assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
        out, infos = outs[0]
        assert infos[0]["n_bytes"] == out.size == n * 2 * n_ch
        aud = np.stack([m.audio(1, c) for c in range(n_ch)])
        for a, b in ((0, 3000), (frames_per_piece - 3000, frames_per_piece + 1000), (2 * frames_per_piece - 3000, 2 * frames_per_piece + 1000), (n - 3000, n)):
            y = np.stack([ta.band_f32(aud[c], row, a, b - a) for c in range(n_ch)])
            want = np.empty((b - a, n_ch, 2), np.uint8)
            for c in range(n_ch):
                q, _, _ = E.quantize(E.PCM_S16, E.DITHER_TPDF, 77, c, a, y[c])
                want[:, c, :] = (q & 0xFFFF).astype("<u2").view(np.uint8).reshape(-1, 2)
            assert np.array_equal(out[a * 2 * n_ch: b * 2 * n_ch], want.reshape(-1)), (a, b)
            f32, _ = m.export_pcm_band([(1,) + bd + (E.PCM_F32, 0, 0, sec_of(a), INF if b == n else sec_of(b))])
            assert np.array_equal(bits(planar(f32, n_ch)), bits(y)), (a, b)
    finally:
        m.close()


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_tmg_gives_the_bytes_and_infos_of_tm(tm, devices):
    reqs = [(2,) + band(64) + (E.PCM_S24, E.DITHER_TPDF, 1, sec_of(1), sec_of(2050)), (1,) + band(65, STOP) + (E.PCM_S16, E.DITHER_TPDF, 2),
            (6,) + band(256, PASS, 0.0, 1500.0) + (E.PCM_F32,), (6,) + band(33) + (E.PCM_S24, E.DITHER_NONE, 4, sec_of(3), sec_of(400)),
            (3, PASS, 0.0, INF, 0.0, E.PCM_S16, E.DITHER_TPDF, 5), (1,) + band(64, PASS, 1500.0, INF) + (E.PCM_S16, E.DITHER_NONE, 0),
            (2,) + band(64) + (E.PCM_S16,), (3,) + band(1024) + (E.PCM_F32,)]
    g = ta.MultiTrackManager(devices)
    try:
        g.add_tracks([(i, SR, x) for i, x in sorted(TRACKS.items())])
        if len(devices) > 1:
            assert len({g.device_of(i) for i in TRACKS}) == 2
        rc, buf, infos, out_len = raw_export_band(tm.handle, reqs)
        rcg, bufg, infosg, out_leng = raw_export_band(g.handle, reqs, pfx="th_tmg_")
        assert rc == rcg == _ffi.OK, _ffi.last_error()
        assert out_len == out_leng and np.array_equal(buf, bufg)
        strip = lambda d: {k: v for k, v in d.items() if k != "waveform_revision"}  # noqa: E731
        assert [strip(o) for o in infos] == [strip(o) for o in infosg]
        assert all(o["waveform_revision"] == g.revisions()[0] for o in infosg)
        for tid, fmt in ((1, E.PCM_S24), (2, E.PCM_F32)):
            assert g.export_wav_band(tid, *band(65), fmt, E.DITHER_TPDF, 9)[0] == tm.export_wav_band(tid, *band(65), fmt, E.DITHER_TPDF, 9)[0]
        with pytest.raises(ta.ThError) as e:
            g.export_pcm_band([(1,) + band(64) + (E.PCM_S16,), (99,) + band(64) + (E.PCM_S16,)])
        assert e.value.code == _ffi.ERR_NOT_FOUND
        with pytest.raises(ta.ThError) as e:
            g.export_wav_band(1, PASS, 100.0, 1000.0, 0.78, E.PCM_S16)
        assert e.value.code == _ffi.ERR_UNSUPPORTED
    finally:
        g.close()
