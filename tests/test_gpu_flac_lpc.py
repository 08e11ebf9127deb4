"""FLAC export with LPC subframes and stereo decorrelation (th_tm_export_flac_ex and the th_tmg twin) on the GPU.

The oracle is exact, as in tests/test_gpu_flac.py.  For flags 1, 2, 3: (1) the file is byte for byte what th_flac_encode_i32_ex makes
on the host of th_export_quantize(th_tm_copy_audio(...)) with the same flags, which tests/test_flac_lpc_host.py checks against the
strict decoder and the model of the decisions; (2) the file, decoded, gives byte for byte what th_tm_export_pcm returns.

Shapes: a block is 4096 samples and no predictor is tried below 5, LPC order m needs m + 1 samples, so tracks of 1, 5, 9 (orders up to
8), 33, 4095, 4096, 4097 and 2 x 4096 + 17 samples; 1, 2 and 3 channels; a stereo track whose channels are nearly equal, so that the
side and mid channels are chosen; a compressible stereo track whose four units per block pass two pieces, for each flags value."""
import ctypes as C

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api
from tests import export_ref as R
from tests import flac_lpc_ref as M
from tests import flac_ref as F
from tests.synth import synth_track

pytestmark = pytest.mark.gpu

INF = float("inf")
FORMATS = (R.PCM_S16, R.PCM_S24)
DITHERS = (R.DITHER_NONE, R.DITHER_TPDF)
BPS = {R.PCM_S16: 16, R.PCM_S24: 24}
FLAGS = (1, 2, 3)
N = 5003
CANARY = 64
LENGTHS = {101: 1, 102: 5, 103: 9, 104: 33, 105: 4095, 106: 4096, 107: 4097, 108: 2 * 4096 + 17}


def _audio(seed, sr, n, channels, peak=0.9):
    x = np.stack([synth_track(seed + c, sr, max(n, 64))[:n] for c in range(channels)])
    return (x * (peak / max(np.abs(x).max(), 1e-9))).astype(np.float32)


def _near_stereo(seed, n):
    """two channels that are nearly equal: the side channel is small"""
    a = _audio(seed, 48000, n, 2, 0.7)
    return np.stack([a[0], (0.9 * a[0] + 0.004 * a[1]).astype(np.float32)])


def _tracks():
    t = {1: (48000, _audio(10, 48000, N, 1)), 2: (48000, _near_stereo(20, N)), 3: (48000, _audio(30, 48000, N, 3)),
         4: (44100, _audio(40, 44100, N, 2, 1.05))}
    for tid, n in LENGTHS.items():
        t[tid] = (48000, _near_stereo(tid, n))
    return t


TRACKS = _tracks()


def sec_of(s, sr):
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


def audio_of(m, tid):
    if tid not in _AUDIO:
        a = np.stack([m.audio(tid, c, 0) for c in range(TRACKS[tid][1].shape[0])])
        a.setflags(write=False)
        _AUDIO[tid] = a
    return _AUDIO[tid]


def host_file(audio, sr, fmt, dith, seed, s0, s1, flags):
    """-> (file bytes, n_clamped, n_nan): the host's quantiser and the host's encoder on samples [s0, s1)"""
    q, nc, nn = [], 0, 0
    for c in range(audio.shape[0]):
        qc, a, b = ta.export_quantize(fmt, dith, seed, c, s0, audio[c, s0:s1])
        q.append(qc)
        nc, nn = nc + a, nn + b
    return ta.flac_encode_i32(np.stack(q) if s1 > s0 else np.zeros((audio.shape[0], 0), np.int32), fmt, sr, flags=flags), nc, nn


def raw_flac(handle, reqs, flags, pfx="th_tm_", cap=None, fill=0xA5):
    """the C entry on a buffer with CANARY bytes of `fill` on each side -> (rc, whole buffer, infos, out_len, cap)"""
    n = len(reqs)
    arr = (_ffi.ExportRequest * n)(*[api._export_request(r) for r in reqs])
    info = (_ffi.ExportInfo * n)()
    need = C.c_size_t()
    fn = getattr(_ffi.lib, pfx + "export_flac_ex")
    if cap is None:
        rc = fn(handle, arr, n, flags, None, 0, info, C.byref(need))
        assert rc == _ffi.ERR_BUFFER_TOO_SMALL, _ffi.last_error()
        cap = need.value
    buf = np.full(cap + 2 * CANARY, fill, np.uint8)
    rc = fn(handle, arr, n, flags, buf.ctypes.data + CANARY, cap, info, C.byref(need))
    return rc, buf, [api._export_info_dict(o) for o in info], need.value, cap


def check_decodes_to_pcm(m, blob, req, info):
    pcm, pinfo = m.export_pcm([req])
    dec = M.decode(blob)
    assert F.pcm_bytes(dec) == pcm.tobytes()
    assert (dec["sr"], dec["n_ch"], dec["bps"]) == (info["sr"], info["n_channels"], BPS[req[1]])
    assert dec["total"] == info["sample_end"] - info["sample_start"]
    assert (info["n_clamped"], info["n_nan"]) == (pinfo[0]["n_clamped"], pinfo[0]["n_nan"])
    return dec


def test_smaller_files_that_decode_to_the_pcm_export(tm):
    """the smallest statement of the feature (fails without it): each tool makes the nearly-equal stereo track's file smaller"""
    req = (2, R.PCM_S16, R.DITHER_TPDF, 5)
    sizes = {}
    for flags in (0, 1, 2, 3):
        out, infos = tm.export_flac([req], flags=flags)
        dec = check_decodes_to_pcm(tm, out.tobytes(), req, infos[0])
        sizes[flags] = out.size
        if flags & 2:
            assert {f["assign"] for f in dec["frames"]} <= {8, 9, 10}
        if flags & 1:
            assert any(s["type"] == "lpc" for f in dec["frames"] for s in f["subframes"])
    assert sizes[3] < sizes[1] < sizes[0] and sizes[3] < sizes[2] < sizes[0]
    assert tm.export_flac([req], flags=0)[0].tobytes() == tm.export_flac([req])[0].tobytes()


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dith", DITHERS)
@pytest.mark.parametrize("tid", [1, 2, 3, 4])
def test_channels_formats_dithers(tm, tid, fmt, dith, flags):
    sr, x = TRACKS[tid]
    req = (tid, fmt, dith, 7 + tid)
    out, infos = tm.export_flac([req], flags=flags)
    want, nc, nn = host_file(audio_of(tm, tid), sr, fmt, dith, 7 + tid, 0, N, flags)
    assert out.tobytes() == want
    assert (infos[0]["n_bytes"], infos[0]["n_clamped"], infos[0]["n_nan"], infos[0]["n_channels"]) == (len(want), nc, nn, x.shape[0])
    check_decodes_to_pcm(tm, want, req, infos[0])
    assert len(want) <= tm.export_flac([req])[0].size  # never longer than th_tm_export_flac's


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("tid", sorted(LENGTHS))
def test_track_lengths(tm, tid, flags):
    n = LENGTHS[tid]
    for fmt, dith in ((R.PCM_S16, R.DITHER_TPDF), (R.PCM_S24, R.DITHER_NONE)):
        req = (tid, fmt, dith, 1)
        out, infos = tm.export_flac([req], flags=flags)
        assert out.tobytes() == host_file(audio_of(tm, tid), 48000, fmt, dith, 1, 0, n, flags)[0]
        dec = check_decodes_to_pcm(tm, out.tobytes(), req, infos[0])
        assert [f["block"] for f in dec["frames"]] == [4096] * (n // 4096) + ([n % 4096] if n % 4096 else [])
        assert len(out) <= ta.flac_bound(n, 2, fmt)


@pytest.mark.parametrize("flags", FLAGS)
def test_a_range_from_an_odd_sample_in_mid_track(tm, flags):
    s0, s1 = 2049, 8191
    req = (108, R.PCM_S16, R.DITHER_TPDF, 9, sec_of(s0, 48000), sec_of(s1, 48000))
    out, infos = tm.export_flac([req], flags=flags)
    assert (infos[0]["sample_start"], infos[0]["sample_end"]) == (s0, s1)
    assert out.tobytes() == host_file(audio_of(tm, 108), 48000, R.PCM_S16, R.DITHER_TPDF, 9, s0, s1, flags)[0]
    check_decodes_to_pcm(tm, out.tobytes(), req, infos[0])


@pytest.mark.parametrize("flags", FLAGS)
def test_mixed_batch_layout_and_canaries(tm, flags):
    reqs = [(1, R.PCM_S24, R.DITHER_TPDF, 1, sec_of(1, 48000), sec_of(4100, 48000)), (2, R.PCM_S16, R.DITHER_TPDF, 2), (3, R.PCM_S16),
            (2, R.PCM_S16, 0, 0, 0.05, 0.05), (108, R.PCM_S24, R.DITHER_NONE, 4), (3, R.PCM_S24, R.DITHER_TPDF, 3, sec_of(3, 48000), sec_of(4, 48000))]
    rc, buf, infos, out_len, cap = raw_flac(tm.handle, reqs, flags)
    assert rc == _ffi.OK, _ffi.last_error()
    assert np.all(buf[:CANARY] == 0xA5) and np.all(buf[CANARY + cap:] == 0xA5)  # nothing at or beyond the last request's bound
    at = 0
    for i, (r, o) in enumerate(zip(reqs, infos)):
        sr, x = TRACKS[r[0]]
        s0, s1 = o["sample_start"], o["sample_end"]
        want, nc, nn = host_file(audio_of(tm, r[0]), sr, r[1], r[2] if len(r) > 2 else 0, r[3] if len(r) > 3 else 0, s0, s1, flags)
        assert o["offset"] == at and at % 16 == 0, (i, o)
        assert buf[CANARY + at: CANARY + at + o["n_bytes"]].tobytes() == want, (i, o)
        assert (o["n_clamped"], o["n_nan"], o["waveform_revision"]) == (nc, nn, tm.revisions()[0])
        bound = ta.flac_bound(s1 - s0, x.shape[0], r[1])  # (the offsets are th_tm_export_flac's)
        assert o["n_bytes"] <= bound
        at = (at + bound + 15) // 16 * 16
    assert out_len == infos[-1]["offset"] + infos[-1]["n_bytes"]
    assert infos[3]["n_bytes"] == 42


def test_nan_and_over_range_samples_are_counted(ctx):
    bad = _near_stereo(300, 4200)
    bad[0, 7] = np.nan
    bad[1, 4100] = 1.5
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(12, 48000, bad)])
        x = np.stack([m.audio(12, c) for c in range(2)])
        for fmt in FORMATS:
            for flags in FLAGS:
                req = (12, fmt, R.DITHER_TPDF, 3)
                out, infos = m.export_flac([req], flags=flags)
                want, nc, nn = host_file(x, 48000, fmt, R.DITHER_TPDF, 3, 0, 4200, flags)
                assert out.tobytes() == want and (infos[0]["n_clamped"], infos[0]["n_nan"]) == (nc, nn) == (1, 1)  # (counted once: L and R)
                dec = check_decodes_to_pcm(m, want, req, infos[0])
                assert dec["channels"][0][7] == 0 and dec["channels"][1][4100] == (1 << (BPS[fmt] - 1)) - 1
    finally:
        m.close()


def test_flags_zero_is_the_plain_entry(tm):
    reqs = [(1, R.PCM_S16, R.DITHER_TPDF, 1), (2, R.PCM_S24), (3, R.PCM_S16, R.DITHER_TPDF, 2), (108, R.PCM_S16)]
    rc, buf, infos, out_len, cap = raw_flac(tm.handle, reqs, 0)
    out, plain = tm.export_flac(reqs)
    assert rc == _ffi.OK and out_len == out.size
    assert buf[CANARY:CANARY + out_len].tobytes()[:42] == out.tobytes()[:42]
    for o, p in zip(infos, plain):
        assert o == p
        assert buf[CANARY + o["offset"]:CANARY + o["offset"] + o["n_bytes"]].tobytes() == out[p["offset"]:p["offset"] + p["n_bytes"]].tobytes()


def test_errors_write_nothing(tm):
    good = (1, R.PCM_S16, R.DITHER_NONE, 0, 0.0, 0.01)
    for flags in (4, 8, 7, 0x80000000):
        for reqs in ([good], [good, (2, R.PCM_S24)]):
            rc, buf, _, _, _ = raw_flac(tm.handle, reqs, flags, cap=1 << 16)
            assert rc == _ffi.ERR_INVALID_ARG and np.all(buf == 0xA5), (flags, _ffi.last_error())
    # the flags are checked where the format is: a missing track or an unknown `which` comes first
    for bad, code in (((99, R.PCM_S16), _ffi.ERR_NOT_FOUND), ((1, R.PCM_S16, 0, 0, 0.0, INF, 3), _ffi.ERR_INVALID_ARG),
                      ((1, R.PCM_F32), _ffi.ERR_INVALID_ARG)):
        rc, buf, _, _, _ = raw_flac(tm.handle, [bad], 4, cap=1 << 16)
        assert rc == code and np.all(buf == 0xA5)
    rc, buf, _, _, _ = raw_flac(tm.handle, [(99, R.PCM_S16)], 4, cap=1 << 16)
    assert rc == _ffi.ERR_NOT_FOUND and "99" in _ffi.last_error()
    n = C.c_size_t()
    arr = (_ffi.ExportRequest * 1)(api._export_request(good))
    info = (_ffi.ExportInfo * 1)()
    fn = _ffi.lib.th_tm_export_flac_ex
    assert fn(None, arr, 1, 3, None, 0, info, C.byref(n)) == _ffi.ERR_INVALID_ARG
    assert fn(tm.handle, None, 1, 3, None, 0, info, C.byref(n)) == _ffi.ERR_INVALID_ARG
    assert fn(tm.handle, arr, 1, 3, None, 0, None, C.byref(n)) == _ffi.ERR_INVALID_ARG
    assert fn(tm.handle, arr, 1, 3, None, 0, info, None) == _ffi.ERR_INVALID_ARG
    assert fn(tm.handle, None, 0, 3, None, 0, None, C.byref(n)) == _ffi.OK and n.value == 0  # an empty batch


@pytest.mark.parametrize("flags", FLAGS)
def test_size_query_and_small_buffers(tm, flags):
    """the bounds, the offsets and the query are th_tm_export_flac's whatever the flags"""
    reqs = [(2, R.PCM_S24, R.DITHER_TPDF, 1, sec_of(1, 48000), sec_of(100, 48000)), (3, R.PCM_S16)]
    n = len(reqs)
    arr = (_ffi.ExportRequest * n)(*[api._export_request(r) for r in reqs])
    info = (_ffi.ExportInfo * n)()
    need = C.c_size_t()
    b0, b1 = F.bound(99, 2, 24), F.bound(N, 3, 16)
    off1 = (b0 + 15) // 16 * 16
    assert _ffi.lib.th_tm_export_flac_ex(tm.handle, arr, n, flags, None, 0, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert (info[0].offset, info[0].n_bytes, info[0].sample_start, info[0].sample_end) == (0, b0, 1, 100)
    assert (info[1].offset, info[1].n_bytes, info[1].sample_start, info[1].sample_end) == (off1, b1, 0, N)
    assert need.value == off1 + b1 and info[0].waveform_revision == tm.revisions()[0]
    rc, buf, infos, out_len, _ = raw_flac(tm.handle, reqs, flags, cap=need.value - 1)
    assert rc == _ffi.ERR_BUFFER_TOO_SMALL and np.all(buf == 0xA5) and out_len == need.value
    rc, buf, infos, out_len, _ = raw_flac(tm.handle, reqs, flags, cap=need.value)
    assert rc == _ffi.OK and out_len == off1 + infos[1]["n_bytes"] < need.value


def _long_stereo_len():
    """the smallest 2-channel 16-bit length whose bound exceeds two pieces of TH_EXPORT_PIECE_BYTES: whole blocks and a short one"""
    fb, two = 16 + 2 * (1 + 4096 * 2) + 3, 2 * api.EXPORT_PIECE_BYTES
    full = (two - 42) // fb
    rest = (two - 42 - full * fb - 21) // 4 + 1
    n = full * 4096 + rest
    assert 0 < rest < 4096 and F.bound(n, 2, 16) > two >= F.bound(n - 1, 2, 16)
    return n, full, rest


@pytest.fixture(scope="module")
def long_stereo(ctx):
    """a compressible near-stereo track just over two pieces (a 65 537-sample passage repeated: no two blocks alike), resident in a
    manager of its own, with the integers th_export_quantize makes of th_tm_copy_audio, computed once for the three flags values"""
    n, full, rest = _long_stereo_len()
    base = _near_stereo(77, 65537)
    x = np.ascontiguousarray(np.tile(base, (1, n // 65537 + 1))[:, :n])
    m = ta.TrackManager(ctx)
    m.add_tracks([(1, 48000, x)])
    audio = np.stack([m.audio(1, c) for c in range(2)])
    q = np.stack([ta.export_quantize(R.PCM_S16, R.DITHER_NONE, 0, c, 0, audio[c])[0] for c in range(2)])
    q.setflags(write=False)
    yield m, q, n, full, rest
    m.close()


def tail_frames(data, k):
    """the starts of a file's last k frames, found from the end: a sync code from which the CRC-16 of the frame holds"""
    end, starts = len(data), []
    for _ in range(k):
        at = end - 6
        while True:
            at = data.rfind(b"\xff\xf8", 42, at + 1)
            assert at >= 42
            if F.crc16(data[at:end - 2]) == int.from_bytes(data[end - 2:end], "big"):
                break
            at -= 1
        starts.append(at)
        end = at
    return starts[::-1]


@pytest.mark.parametrize("flags", FLAGS)
def test_a_stereo_track_of_more_than_two_pieces(long_stereo, flags):
    """Three pieces through the two staging buffers and the reused slot scratch, four units of 17-bit slots per block with
    TH_FLAC_STEREO: the file is byte for byte th_flac_encode_i32_ex's of the quantised audio.  The pure-Python decoder would take
    minutes on 33 M samples, so the whole file is compared with the host's, whose decode tests/test_flac_lpc_host.py covers, and only
    the last three frames are decoded here: the last two blocks of the second piece and the short block that is the third.  They
    give back the samples, and the tools are taken there: LPC subframes with TH_FLAC_LPC, a side channel with TH_FLAC_STEREO"""
    m, q, n, full, rest = long_stereo
    want = ta.flac_encode_i32(q, R.PCM_S16, 48000, flags=flags)
    plain = m.export_flac([(1, R.PCM_S16)])[1][0]["n_bytes"]
    for _ in range(2):  # (the second call reuses the slot's buffers)
        out, infos = m.export_flac([(1, R.PCM_S16)], flags=flags)
        assert infos[0]["n_bytes"] == out.size == len(want) and out.tobytes() == want
    assert len(want) < 0.97 * plain and plain < 4 * n  # (compressible, and each tool gains on it)
    starts = tail_frames(want, 3)
    dec = M.decode(want[:42] + want[starts[0]:])
    assert [f["number"] for f in dec["frames"]] == [full - 2, full - 1, full] and [f["block"] for f in dec["frames"]] == [4096, 4096, rest]
    assert np.array_equal(np.array(dec["channels"], np.int64), q[:, n - 8192 - rest:])
    for f in dec["frames"]:
        if flags & 1:
            assert all(s["type"] == "lpc" for s in f["subframes"]), f["subframes"]
        assert (f["assign"] in (8, 9, 10)) == bool(flags & 2), f["assign"]


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_tmg_gives_the_files_and_infos_of_tm(tm, devices):
    reqs = [(2, R.PCM_S24, R.DITHER_TPDF, 1, sec_of(1, 48000), sec_of(4100, 48000)), (4, R.PCM_S16, R.DITHER_TPDF, 2), (1, R.PCM_S16),
            (3, R.PCM_S16, R.DITHER_TPDF, 5), (108, R.PCM_S24)]
    g = ta.MultiTrackManager(devices)
    try:
        g.add_tracks([(i, sr, x) for i, (sr, x) in sorted(TRACKS.items())])
        if len(devices) > 1:
            assert len({g.device_of(i) for i in TRACKS}) == 2
        for flags in FLAGS:
            rc, buf, infos, out_len, cap = raw_flac(tm.handle, reqs, flags)
            rcg, bufg, infosg, out_leng, capg = raw_flac(g.handle, reqs, flags, pfx="th_tmg_")
            assert rc == rcg == _ffi.OK, _ffi.last_error()
            assert (out_len, cap) == (out_leng, capg)
            for o, og in zip(infos, infosg):
                assert {k: v for k, v in o.items() if k != "waveform_revision"} == {k: v for k, v in og.items() if k != "waveform_revision"}
                assert og["waveform_revision"] == g.revisions()[0]
                a, b = CANARY + o["offset"], CANARY + o["offset"] + o["n_bytes"]
                assert np.array_equal(buf[a:b], bufg[a:b])
            assert np.all(bufg[:CANARY] == 0xA5) and np.all(bufg[CANARY + capg:] == 0xA5)
        one, _ = g.export_flac([reqs[0]], flags=3)
        assert one.tobytes() == tm.export_flac([reqs[0]], flags=3)[0].tobytes()
        rcg, bufg, _, _, _ = raw_flac(g.handle, reqs, 4, pfx="th_tmg_", cap=1 << 16)
        assert rcg == _ffi.ERR_INVALID_ARG and np.all(bufg == 0xA5)
    finally:
        g.close()
