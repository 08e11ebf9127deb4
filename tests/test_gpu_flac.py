"""FLAC export of resident tracks (th_tm_export_flac and the th_tmg twin) on the GPU.

FLAC is lossless, so the oracle is exact.  (1) The file, decoded by the strict decoder of tests/flac_ref.py, gives byte for byte what
th_tm_export_pcm returns for the same request - existing code, not the code under test.  (2) The file is byte for byte what
th_flac_encode_i32 makes on the host of th_export_quantize(th_tm_copy_audio(...)), which tests/test_flac_host.py checks against the
decoder and a numpy model of the decisions.  The counts are exact.

Shapes: a block is 4096 samples, so tracks of 1, 4, 5 (no predictor below 5), 4095, 4096, 4097 and 2 x 4096 + 1 samples; 1, 2, 3, 6
and 8 channels of 5003 samples (one whole block and a short one); a range from an odd sample in mid-track (the dither's index stays
absolute, the frame numbers start at 0 again); one track whose bound exceeds two pieces."""
import ctypes as C

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api
from tests import export_ref as R
from tests import flac_ref as F
from tests.synth import synth_track

pytestmark = pytest.mark.gpu

INF = float("inf")
FORMATS = (R.PCM_S16, R.PCM_S24)
DITHERS = (R.DITHER_NONE, R.DITHER_TPDF)
BPS = {R.PCM_S16: 16, R.PCM_S24: 24}
N = 5003
CANARY = 64
LENGTHS = {101: 1, 102: 4, 103: 5, 104: 4095, 105: 4096, 106: 4097, 107: 2 * 4096 + 1}


def _audio(seed, sr, n, channels, peak=0.9):
    x = np.stack([synth_track(seed + c, sr, max(n, 64))[:n] for c in range(channels)])
    return (x * (peak / max(np.abs(x).max(), 1e-9))).astype(np.float32)


def _tracks():
    t = {k: (48000, _audio(10 * k, 48000, N, k, 1.05 if k == 2 else 0.9)) for k in (1, 2, 3, 6, 8)}
    t[11] = (44100, _audio(200, 44100, 3001, 2))
    for tid, n in LENGTHS.items():
        t[tid] = (48000, _audio(tid, 48000, n, 2))
    rng = np.random.default_rng(3)
    t[20] = (48000, np.zeros((2, 4500), np.float32))                                   # silence: CONSTANT
    t[21] = (48000, rng.uniform(-1.0, 1.0, (2, 4500)).astype(np.float32))              # full-scale noise: VERBATIM
    return t


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


def host_file(audio, sr, fmt, dith, seed, s0, s1):
    """-> (file bytes, n_clamped, n_nan): the host's quantiser and the host's encoder on samples [s0, s1)"""
    q, nc, nn = [], 0, 0
    for c in range(audio.shape[0]):
        qc, a, b = ta.export_quantize(fmt, dith, seed, c, s0, audio[c, s0:s1])
        q.append(qc)
        nc, nn = nc + a, nn + b
    return ta.flac_encode_i32(np.stack(q) if s1 > s0 else np.zeros((audio.shape[0], 0), np.int32), fmt, sr), nc, nn


def raw_flac(handle, reqs, pfx="th_tm_", cap=None, fill=0xA5):
    """the C entry on a buffer with CANARY bytes of `fill` on each side -> (rc, whole buffer, infos, out_len, cap)"""
    n = len(reqs)
    arr = (_ffi.ExportRequest * n)(*[api._export_request(r) for r in reqs])
    info = (_ffi.ExportInfo * n)()
    need = C.c_size_t()
    fn = getattr(_ffi.lib, pfx + "export_flac")
    if cap is None:
        rc = fn(handle, arr, n, None, 0, info, C.byref(need))
        assert rc == _ffi.ERR_BUFFER_TOO_SMALL, _ffi.last_error()
        cap = need.value
    buf = np.full(cap + 2 * CANARY, fill, np.uint8)
    rc = fn(handle, arr, n, buf.ctypes.data + CANARY, cap, info, C.byref(need))
    return rc, buf, [api._export_info_dict(o) for o in info], need.value, cap


def check_decodes_to_pcm(m, blob, req, info):
    """the contract's core: the file decodes to the bytes th_tm_export_pcm returns for the same request"""
    pcm, pinfo = m.export_pcm([req])
    dec = F.decode(blob)
    assert F.pcm_bytes(dec) == pcm.tobytes()
    assert (dec["sr"], dec["n_ch"], dec["bps"]) == (info["sr"], info["n_channels"], BPS[req[1]])
    assert dec["total"] == info["sample_end"] - info["sample_start"] == pinfo[0]["sample_end"] - pinfo[0]["sample_start"]
    assert [f["number"] for f in dec["frames"]] == list(range(len(dec["frames"])))  # (the frame numbers start at 0 in every file)
    assert (info["n_clamped"], info["n_nan"]) == (pinfo[0]["n_clamped"], pinfo[0]["n_nan"])
    return dec


def test_decodes_to_the_pcm_export(tm):
    """the smallest statement of the feature (fails without it)"""
    req = (2, R.PCM_S16, R.DITHER_TPDF, 5)
    out, infos = tm.export_flac([req])
    assert out.size == infos[0]["n_bytes"] < tm.export_pcm([req])[1][0]["n_bytes"]  # (and it is smaller than the PCM)
    dec = check_decodes_to_pcm(tm, out.tobytes(), req, infos[0])
    assert infos[0]["n_clamped"] > 0  # (track 2 peaks at 1.05)
    assert all(s["type"] == "fixed" for f in dec["frames"] for s in f["subframes"])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dith", DITHERS)
@pytest.mark.parametrize("tid", [1, 2, 3, 6, 8])
def test_channels_formats_dithers(tm, tid, fmt, dith):
    sr, x = TRACKS[tid]
    req = (tid, fmt, dith, 7 + tid)
    out, infos = tm.export_flac([req])
    want, nc, nn = host_file(audio_of(tm, tid), sr, fmt, dith, 7 + tid, 0, N)
    assert out.tobytes() == want
    assert (infos[0]["n_bytes"], infos[0]["n_clamped"], infos[0]["n_nan"], infos[0]["n_channels"]) == (len(want), nc, nn, x.shape[0])
    check_decodes_to_pcm(tm, want, req, infos[0])


@pytest.mark.parametrize("tid", sorted(LENGTHS))
def test_track_lengths(tm, tid):
    n = LENGTHS[tid]
    for fmt, dith in ((R.PCM_S16, R.DITHER_TPDF), (R.PCM_S24, R.DITHER_NONE)):
        req = (tid, fmt, dith, 1)
        out, infos = tm.export_flac([req])
        assert out.tobytes() == host_file(audio_of(tm, tid), 48000, fmt, dith, 1, 0, n)[0]
        dec = check_decodes_to_pcm(tm, out.tobytes(), req, infos[0])
        assert [f["block"] for f in dec["frames"]] == [4096] * (n // 4096) + ([n % 4096] if n % 4096 else [])
        assert len(out) <= ta.flac_bound(n, 2, fmt)


def test_a_range_from_an_odd_sample_in_mid_track(tm):
    """the dither's index is the track's, the frame numbers are the file's"""
    s0, s1 = 2049, 8191
    req = (107, R.PCM_S16, R.DITHER_TPDF, 9, sec_of(s0, 48000), sec_of(s1, 48000))
    out, infos = tm.export_flac([req])
    assert (infos[0]["sample_start"], infos[0]["sample_end"]) == (s0, s1)
    assert out.tobytes() == host_file(audio_of(tm, 107), 48000, R.PCM_S16, R.DITHER_TPDF, 9, s0, s1)[0]
    check_decodes_to_pcm(tm, out.tobytes(), req, infos[0])
    whole = F.decode(tm.export_flac([(107, R.PCM_S16, R.DITHER_TPDF, 9)])[0].tobytes())
    part = F.decode(out.tobytes())
    assert [c[s0:s1] for c in whole["channels"]] == part["channels"]  # a range's samples are a slice of the whole file's


def test_mixed_batch_layout_and_canaries(tm):
    reqs = [(2, R.PCM_S24, R.DITHER_TPDF, 1, sec_of(1, 48000), sec_of(4100, 48000)), (11, R.PCM_S16, R.DITHER_TPDF, 2), (20, R.PCM_S16),
            (6, R.PCM_S24, R.DITHER_NONE, 4, sec_of(3, 48000), sec_of(4, 48000)), (3, R.PCM_S16, 0, 0, 0.05, 0.05), (21, R.PCM_S24),
            (107, R.PCM_S16, R.DITHER_TPDF, 3)]
    rc, buf, infos, out_len, cap = raw_flac(tm.handle, reqs)
    assert rc == _ffi.OK, _ffi.last_error()
    assert np.all(buf[:CANARY] == 0xA5) and np.all(buf[CANARY + cap:] == 0xA5)  # nothing at or beyond the last request's bound
    at = 0
    for i, (r, o) in enumerate(zip(reqs, infos)):
        sr, x = TRACKS[r[0]]
        s0, s1 = o["sample_start"], o["sample_end"]
        want, nc, nn = host_file(audio_of(tm, r[0]), sr, r[1], r[2] if len(r) > 2 else 0, r[3] if len(r) > 3 else 0, s0, s1)
        assert o["offset"] == at and at % 16 == 0, (i, o)
        assert buf[CANARY + at: CANARY + at + o["n_bytes"]].tobytes() == want, (i, o)
        assert (o["n_clamped"], o["n_nan"], o["waveform_revision"]) == (nc, nn, tm.revisions()[0])
        bound = ta.flac_bound(s1 - s0, x.shape[0], r[1])
        assert o["n_bytes"] <= bound
        at = (at + bound + 15) // 16 * 16
    assert out_len == infos[-1]["offset"] + infos[-1]["n_bytes"]
    assert cap == infos[-1]["offset"] + ta.flac_bound(LENGTHS[107], 2, R.PCM_S16)
    assert infos[4]["n_bytes"] == 42 and (infos[4]["sample_start"], infos[4]["sample_end"]) == R.sample_range(48000, N, 0.05, 0.05)
    # the same requests one by one give the same files: a file does not depend on the batch
    for r, o in zip(reqs, infos):
        one, _ = tm.export_flac([r])
        assert one.tobytes() == buf[CANARY + o["offset"]: CANARY + o["offset"] + o["n_bytes"]].tobytes()


def test_silence_and_noise(tm):
    for tid, kind, fmt in ((20, "constant", R.PCM_S16), (20, "constant", R.PCM_S24), (21, "verbatim", R.PCM_S16), (21, "verbatim", R.PCM_S24)):
        req = (tid, fmt)
        out, infos = tm.export_flac([req])
        dec = check_decodes_to_pcm(tm, out.tobytes(), req, infos[0])
        assert {s["type"] for f in dec["frames"] for s in f["subframes"]} == {kind}
        assert out.tobytes() == host_file(audio_of(tm, tid), 48000, fmt, 0, 0, 0, 4500)[0]
    # dithered silence is no longer constant
    out, infos = tm.export_flac([(20, R.PCM_S16, R.DITHER_TPDF, 1)])
    assert {s["type"] for f in F.decode(out.tobytes())["frames"] for s in f["subframes"]} == {"fixed"}


def test_nan_and_over_range_samples_are_counted(ctx):
    bad = _audio(300, 48000, 4200, 2, 0.8)
    bad[0, 7] = np.nan
    bad[1, 4100] = 1.5
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(12, 48000, bad)])
        x = np.stack([m.audio(12, c) for c in range(2)])
        for fmt in FORMATS:
            req = (12, fmt, R.DITHER_TPDF, 3)
            out, infos = m.export_flac([req])
            want, nc, nn = host_file(x, 48000, fmt, R.DITHER_TPDF, 3, 0, 4200)
            assert out.tobytes() == want and (infos[0]["n_clamped"], infos[0]["n_nan"]) == (nc, nn) == (1, 1)
            dec = check_decodes_to_pcm(m, want, req, infos[0])
            assert dec["channels"][0][7] == 0 and dec["channels"][1][4100] == (1 << (BPS[fmt] - 1)) - 1
    finally:
        m.close()


def test_which_and_the_revision(ctx):
    m = ta.TrackManager(ctx)
    try:
        sr, x = TRACKS[2]
        m.add_tracks([(2, sr, x)])
        _, i0 = m.export_flac([(2, R.PCM_S16)])
        assert i0[0]["waveform_revision"] == m.revisions()[0]
        m.set_common_guard_clipping(api.GUARD_CLIP)
        m.set_common_normalize(api.NORM_PEAK_DB, 6.0)
        aud = [np.stack([m.audio(2, c, w) for c in range(2)]) for w in (0, 1, 2)]
        assert not np.array_equal(aud[0], aud[1]) and not np.array_equal(aud[1], aud[2])
        files = []
        for which in (0, 1, 2):
            out, infos = m.export_flac([(2, R.PCM_S24, R.DITHER_TPDF, 8, 0.0, INF, which)])
            want, nc, nn = host_file(aud[which], sr, R.PCM_S24, R.DITHER_TPDF, 8, 0, N)
            assert out.tobytes() == want and (infos[0]["n_clamped"], infos[0]["n_nan"]) == (nc, nn), which
            assert infos[0]["waveform_revision"] == m.revisions()[0] > i0[0]["waveform_revision"]
            files.append(want)
        assert len(set(files)) == 3
    finally:
        m.close()


def test_errors_write_nothing(tm):
    good = (1, R.PCM_S16, R.DITHER_NONE, 0, 0.0, 0.01)
    nan = float("nan")
    cases = [((99, R.PCM_S16), _ffi.ERR_NOT_FOUND),
             ((1, R.PCM_F32), _ffi.ERR_INVALID_ARG),                          # FLAC has no float samples
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
            rc, buf, _, _, _ = raw_flac(tm.handle, reqs, cap=1 << 16)
            assert rc == code, (bad, rc, _ffi.last_error())
            assert np.all(buf == 0xA5), bad
    rc, buf, _, _, _ = raw_flac(tm.handle, [good, (98, R.PCM_S16), (1, R.PCM_F32)], cap=1 << 16)
    assert rc == _ffi.ERR_NOT_FOUND and np.all(buf == 0xA5)  # the first faulty request decides
    n = C.c_size_t()
    arr = (_ffi.ExportRequest * 1)(api._export_request(good))
    info = (_ffi.ExportInfo * 1)()
    assert _ffi.lib.th_tm_export_flac(None, arr, 1, None, 0, info, C.byref(n)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tm_export_flac(tm.handle, None, 1, None, 0, info, C.byref(n)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tm_export_flac(tm.handle, arr, 1, None, 0, None, C.byref(n)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tm_export_flac(tm.handle, arr, 1, None, 0, info, None) == _ffi.ERR_INVALID_ARG


def test_more_than_eight_channels_are_unsupported(ctx):
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(1, 48000, np.zeros((9, 64), np.float32))])
        rc, buf, _, _, _ = raw_flac(m.handle, [(1, R.PCM_S16)], cap=4096)
        assert rc == _ffi.ERR_UNSUPPORTED and np.all(buf == 0xA5)
        assert m.export_pcm([(1, R.PCM_S16)])[0].size == 9 * 64 * 2  # (the PCM export takes it)
    finally:
        m.close()


def test_size_query_and_small_buffers(tm):
    reqs = [(2, R.PCM_S24, R.DITHER_TPDF, 1, sec_of(1, 48000), sec_of(100, 48000)), (3, R.PCM_S16)]
    n = len(reqs)
    arr = (_ffi.ExportRequest * n)(*[api._export_request(r) for r in reqs])
    info = (_ffi.ExportInfo * n)()
    need = C.c_size_t()
    b0, b1 = F.bound(99, 2, 24), F.bound(N, 3, 16)
    off1 = (b0 + 15) // 16 * 16
    assert _ffi.lib.th_tm_export_flac(tm.handle, arr, n, None, 0, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL  # out == NULL
    assert (info[0].offset, info[0].n_bytes, info[0].sample_start, info[0].sample_end) == (0, b0, 1, 100)
    assert (info[1].offset, info[1].n_bytes, info[1].sample_start, info[1].sample_end) == (off1, b1, 0, N)
    assert need.value == off1 + b1 and (b0, b1) == (ta.flac_bound(99, 2, R.PCM_S24), ta.flac_bound(N, 3, R.PCM_S16))
    assert (info[0].sr, info[0].n_channels, info[1].n_channels) == (48000, 2, 3)
    assert info[0].waveform_revision == tm.revisions()[0] and (info[0].n_clamped, info[0].n_nan) == (0, 0)
    rc, buf, infos, out_len, _ = raw_flac(tm.handle, reqs, cap=need.value - 1)
    assert rc == _ffi.ERR_BUFFER_TOO_SMALL and np.all(buf == 0xA5) and out_len == need.value
    rc, buf, infos, out_len, _ = raw_flac(tm.handle, reqs, cap=need.value)
    assert rc == _ffi.OK and out_len == off1 + infos[1]["n_bytes"] < need.value
    assert _ffi.lib.th_tm_export_flac(tm.handle, None, 0, None, 0, None, C.byref(need)) == _ffi.OK and need.value == 0  # an empty batch


def test_a_track_of_more_than_two_pieces(ctx):
    """incompressible (full-scale noise, mono, 24 bit: every subframe VERBATIM), the smallest number of blocks whose bound exceeds
    two pieces of TH_EXPORT_PIECE_BYTES: three launches through the two staging buffers; the second call reuses them"""
    fb, two = 16 + 1 + 4096 * 3 + 3, 2 * api.EXPORT_PIECE_BYTES
    full = (two - 42) // fb                       # whole blocks inside two pieces
    m = (two - 42 - full * fb - 20) // 3 + 1      # and the samples of a short block that passes them
    n = full * 4096 + m
    assert 0 < m < 4096 and F.bound(n, 1, 24) > two >= F.bound(n - 1, 1, 24)
    x = np.random.default_rng(5).uniform(-1.0, 1.0, (1, n)).astype(np.float32)
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(1, 48000, x)])
        want, nc, nn = host_file(x, 48000, R.PCM_S24, R.DITHER_NONE, 0, 0, n)
        assert 3 * n < len(want) <= F.bound(n, 1, 24)  # (nothing gained: VERBATIM)
        for _ in range(2):
            out, infos = m.export_flac([(1, R.PCM_S24)])
            assert out.tobytes() == want and infos[0]["n_bytes"] == len(want) and (infos[0]["n_clamped"], infos[0]["n_nan"]) == (nc, nn)
        pcm, _ = m.export_pcm([(1, R.PCM_S24)])
        assert np.array_equal(np.frombuffer(want, np.uint8)[42 + 7: 42 + 7 + 3 * 4096].reshape(-1, 3)[:, ::-1], pcm[:3 * 4096].reshape(-1, 3))
    finally:
        m.close()


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_tmg_gives_the_files_and_infos_of_tm(tm, devices):
    reqs = [(2, R.PCM_S24, R.DITHER_TPDF, 1, sec_of(1, 48000), sec_of(4100, 48000)), (11, R.PCM_S16, R.DITHER_TPDF, 2), (1, R.PCM_S16),
            (6, R.PCM_S24, R.DITHER_NONE, 4, sec_of(3, 48000), sec_of(4, 48000)), (3, R.PCM_S16, R.DITHER_TPDF, 5), (8, R.PCM_S16), (107, R.PCM_S24)]
    g = ta.MultiTrackManager(devices)
    try:
        g.add_tracks([(i, sr, x) for i, (sr, x) in sorted(TRACKS.items())])
        if len(devices) > 1:
            assert len({g.device_of(i) for i in TRACKS}) == 2
        rc, buf, infos, out_len, cap = raw_flac(tm.handle, reqs)
        rcg, bufg, infosg, out_leng, capg = raw_flac(g.handle, reqs, pfx="th_tmg_")
        assert rc == rcg == _ffi.OK, _ffi.last_error()
        assert (out_len, cap) == (out_leng, capg)
        for o, og in zip(infos, infosg):
            assert {k: v for k, v in o.items() if k != "waveform_revision"} == {k: v for k, v in og.items() if k != "waveform_revision"}
            assert og["waveform_revision"] == g.revisions()[0]
            a, b = CANARY + o["offset"], CANARY + o["offset"] + o["n_bytes"]
            assert np.array_equal(buf[a:b], bufg[a:b])
        assert np.all(bufg[:CANARY] == 0xA5) and np.all(bufg[CANARY + capg:] == 0xA5)
        one, info1 = g.export_flac([reqs[0]])
        assert one.tobytes() == buf[CANARY: CANARY + infos[0]["n_bytes"]].tobytes()
    finally:
        g.close()
