"""The waveform envelope and the waveform lane (th_tm_get_envelopes, th_tm_render_waveform_figures and the th_tmg twins) on the GPU.

Reference: the definition restated in numpy (tests/envelope_ref.py) applied to the samples th_tm_copy_audio returns.  min and max are
compared as values; mean and rms within the first-order bound of an f64 sum of c terms in any order plus the one f32 rounding
(envelope_ref.tolerances: derived, not measured); held columns, the bytes of a lane (computed from the envelope floats the reader
returned for the same request) and every comparison between two ways of asking are exact."""
import ctypes as C
import threading

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api
from tests import envelope_ref as R

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
SR, N = 48000, 70001
CHUNK = api.ENVELOPE_CHUNK
assert N % CHUNK != 0 and N > 4 * CHUNK   # several chunks, the last one partial


def _signal(seed, n, sr=SR):
    """a sine plus seeded noise, with isolated spikes so that extrema sit at known samples"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    x = 0.3 * np.sin(2 * np.pi * (180.0 + 40 * seed) * t) + 0.05 * rng.standard_normal(n)
    x = x.astype(np.float32)
    for k, s in enumerate(range(17, n, 4999)):
        x[s] = np.float32(0.9 if k & 1 else -0.95)
    return x


def _sec(sample, sr=SR):
    """a time whose product with sr rounds up to exactly `sample`"""
    t = sample / sr
    while np.ceil(t * float(sr)) > sample:
        t = np.nextafter(t, 0.0)
    assert np.ceil(t * float(sr)) == sample
    return float(t)


@pytest.fixture(scope="module")
def ctx():
    c = ta.Context(0)
    yield c
    c.close()


TRACKS = [(0, SR, np.stack([_signal(1, N), _signal(2, N)])), (1, SR, np.array([[-0.625]], np.float32))]


@pytest.fixture(scope="module")
def tm(ctx):
    m = ta.TrackManager(ctx)
    m.add_tracks(TRACKS)
    m.apply_track_list_changes()
    yield m
    m.close()


_AUDIO = {}


def audio(m, track, ch, which=1):
    """the samples on the device, fetched once per (manager, channel, which)"""
    key = (id(m), track, ch, which, m.revisions()[0])
    if key not in _AUDIO:
        _AUDIO[key] = m.audio(track, ch, which)
    return _AUDIO[key]


def assert_envelope(got, x, e, what):
    want, mean_abs = R.envelope(x, e)
    tol_m, tol_r = R.tolerances(want, mean_abs, e)
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert np.array_equal(got[:, :2], want[:, :2], equal_nan=True), (what, np.nonzero((got[:, :2] != want[:, :2]).any(1))[0][:5])
    for k, tol, name in ((2, tol_m, "mean"), (3, tol_r, "rms")):
        g, w = got[:, k].astype(np.float64), want[:, k].astype(np.float64)
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), (what, name)
        err = np.abs(g[fin] - w[fin])
        worst = int(np.argmax(err - tol[fin])) if err.size else 0
        print(f"{what}: {name} worst |err| - tol = {(err - tol[fin]).max() if err.size else 0:.3e} (column {np.nonzero(fin)[0][worst] if err.size else -1})")
        assert (err <= tol[fin]).all(), (what, name, np.nonzero(fin)[0][worst], err[worst], tol[fin][worst])
    held = np.diff(e.astype(np.int64)) == 0
    assert np.array_equal(got[held].view(np.uint32), want[held].view(np.uint32)), what   # bit for bit
    return want


# name, track, ch, start_sec, end_sec, n_cols
REQUESTS = [
    ("one_column_across_every_chunk", 0, 0, 0.0, INF, 1),
    ("w3", 0, 0, 0.0, INF, 3),
    ("w7", 0, 0, 0.0, INF, 7),
    ("w333", 0, 0, 0.0, INF, 333),
    ("w1093_dense_64_per_column", 0, 0, 0.0, INF, 1093),
    ("w1094_sparse_63_per_column", 0, 0, 0.0, INF, 1094),
    ("w4099", 0, 0, 0.0, INF, 4099),
    ("w16384", 0, 0, 0.0, INF, 16384),
    ("zoomed_in_700_empty_columns", 0, 0, 0.5, 0.50625, 1000),
    ("odd_start_to_the_end", 0, 0, _sec(1), INF, 5),
    ("odd_start_many_columns", 0, 1, _sec(4097), INF, 257),
    ("on_the_chunk_grid", 0, 0, _sec(CHUNK), _sec(3 * CHUNK), 2),
    ("on_the_chunk_grid_one_column", 0, 0, _sec(2 * CHUNK), _sec(3 * CHUNK), 1),
    ("inside_one_chunk_dense", 0, 0, _sec(CHUNK + 4), _sec(2 * CHUNK - 96), 9),
    ("inside_one_chunk_sparse", 0, 0, _sec(CHUNK + 4), _sec(2 * CHUNK - 96), 100),
    ("two_samples_across_a_chunk_boundary", 0, 0, _sec(CHUNK - 1), _sec(CHUNK + 1), 1),
    ("three_samples", 0, 0, 0.0, 2.5 / SR, 1),
    ("channel_1", 0, 1, 0.1234, 1.357, 333),
    ("end_beyond_the_track", 0, 1, 1.0, 1e9, 64),
    ("one_sample_track", 1, 0, 0.0, INF, 4),
    ("one_sample_track_one_column", 1, 0, 0.0, INF, 1),
    # B > A, but no sample index lies in [A, B): every column holds sample max(e[0], 1) - 1
    ("no_sample_in_the_range", 0, 0, 1000.25 / SR, 1000.75 / SR, 3),
    ("no_sample_before_sample_1", 0, 0, 0.2 / SR, 0.7 / SR, 5),
    ("no_sample_behind_the_last", 0, 1, (N - 0.5) / SR, INF, 300),
    ("no_sample_one_sample_track", 1, 0, 0.25 / SR, 0.5 / SR, 3),
]


@pytest.mark.parametrize("name,track,ch,a,b,W", REQUESTS, ids=[r[0] for r in REQUESTS])
def test_envelope_equals_the_definition(tm, name, track, ch, a, b, W):
    x = audio(tm, track, ch)
    e = ta.envelope_edges(SR, x.size, a, b, W)
    got, info = tm.get_envelope(track, ch, 1, a, b, W)
    assert (info["offset"], info["length"], info["sample_start"], info["sample_end"]) == (0, 4 * W, int(e[0]), int(e[-1]))
    assert info["waveform_revision"] == tm.revisions()[0]
    want = assert_envelope(got, x, e, name)
    d = np.diff(e.astype(np.int64))
    if name == "on_the_chunk_grid":
        assert e.tolist() == [CHUNK, 2 * CHUNK, 3 * CHUNK]
    if name == "zoomed_in_700_empty_columns":
        assert (d == 0).sum() == 700
    if name.startswith("w1093"):
        assert int(e[-1] - e[0]) >= api.ENVELOPE_DENSE_MIN * W
    if name.startswith("w1094"):
        assert int(e[-1] - e[0]) < api.ENVELOPE_DENSE_MIN * W
    if name == "one_column_across_every_chunk":   # the spikes are the extrema
        assert want[0, 0] == np.float32(-0.95) and want[0, 1] == np.float32(0.9)
    if track == 1:
        assert (got == np.float32([-0.625, -0.625, -0.625, 0.625])).all()
    if name.startswith("no_sample"):
        v = x[max(int(e[0]), 1) - 1]
        assert e[0] == e[-1] and (d == 0).all() and (got == np.float32([v, v, v, abs(v)])).all()
        assert int(e[0]) == {"no_sample_in_the_range": 1001, "no_sample_before_sample_1": 1, "no_sample_behind_the_last": N}.get(name, 1)


def test_which_selects_derived_or_original_audio(ctx):
    """after th_tm_set_common_normalize the audio (0), what is drawn (1) and the original (2) are three requests' three answers; the
    revision in the infos follows th_tm_revisions"""
    m = ta.TrackManager(ctx)
    try:
        m.add_tracks([(5, SR, np.stack([_signal(3, 20001), _signal(4, 20001)]))])
        m.apply_track_list_changes()
        rev0 = m.revisions()[0]
        _, info = m.get_envelope(5, 0, 2, 0.0, INF, 50)
        assert info["waveform_revision"] == rev0
        m.set_common_normalize(api.NORM_PEAK_DB, -9.0)
        rev1 = m.revisions()[0]
        assert rev1 != rev0
        orig, aud = m.audio(5, 1, 2), m.audio(5, 1, 0)
        assert not np.array_equal(orig, aud)
        assert np.array_equal(orig, _signal(4, 20001))
        for which in (0, 1, 2):
            x = m.audio(5, 1, which)
            e = ta.envelope_edges(SR, x.size, 0.01, INF, 77)
            got, info = m.get_envelope(5, 1, which, 0.01, INF, 77)
            assert info["waveform_revision"] == rev1
            assert_envelope(got, x, e, f"which {which}")
        e2, _ = m.get_envelope(5, 1, 2, 0.01, INF, 77)
        e0, _ = m.get_envelope(5, 1, 0, 0.01, INF, 77)
        assert not np.array_equal(e0, e2)
    finally:
        m.close()


def _nan_track():
    x = _signal(7, 12000)
    x[1500] = NAN                     # one NaN in a column
    x[3000:4000] = NAN                # a column of 12 that is all NaN
    x[4094:4100] = NAN                # NaN on both sides of a chunk boundary
    x[5500] = INF
    x[6500], x[6600] = -INF, INF
    x[8000:9000:2], x[8001:9000:2] = 0.0, -0.0
    x[11999] = NAN                    # the very last sample
    return x


@pytest.fixture(scope="module")
def tm_nan(ctx):
    m = ta.TrackManager(ctx)
    m.add_tracks([(9, SR, _nan_track()[None])])
    m.apply_track_list_changes()
    yield m
    m.close()


@pytest.mark.parametrize("W", [1, 2, 12, 400, 12000, 24000])
def test_nan_and_infinity(tm_nan, W):
    x = tm_nan.audio(9, 0, 1)
    assert np.array_equal(x.view(np.uint32), _nan_track().view(np.uint32))
    e = ta.envelope_edges(SR, x.size, 0.0, INF, W)
    got, _ = tm_nan.get_envelope(9, 0, 1, 0.0, INF, W)
    want = assert_envelope(got, x, e, f"nan W={W}")
    if W == 12:
        assert want[3].tolist()[:2] == [INF, -INF] and np.isnan(want[3, 2:]).all()          # all NaN
        assert np.isfinite(want[1, :2]).all() and np.isnan(want[1, 2:]).all()               # one NaN
        assert want[5, 1] == INF and want[5, 2] == INF and want[5, 3] == INF
        assert want[6, 0] == -INF and want[6, 1] == INF and np.isnan(want[6, 2]) and want[6, 3] == INF
        assert (want[8] == 0).all() and (got[8] == 0).all()                                 # +-0: either zero
    if W == 24000:   # every second column holds the sample to its left
        assert np.array_equal(got[1::2].view(np.uint32)[:, 0], x.view(np.uint32)) and np.isnan(got[-1]).all()


def _batch():
    return [(t, ch, 1, a, b, W) for _, t, ch, a, b, W in REQUESTS]


def _bits(arrs):
    return [np.ascontiguousarray(a).view(np.uint32).copy() for a in arrs]


def test_batch_equals_single_calls(tm):
    reqs = _batch()
    envs, infos = tm.get_envelopes(reqs)
    at = 0
    for r, env, info in zip(reqs, envs, infos):
        one, _ = tm.get_envelope(*r)
        assert np.array_equal(env.view(np.uint32), one.view(np.uint32)), r
        assert info["offset"] == at and info["length"] == 4 * r[5]
        at += 4 * r[5]
    again, _ = tm.get_envelopes(reqs)
    assert all(np.array_equal(a, b) for a, b in zip(_bits(envs), _bits(again)))   # a second call: the same bytes


def test_batch_across_a_piece_boundary(tm):
    per = api.ENVELOPE_PIECE_BYTES // (16384 * 16)
    reqs = [(0, k & 1, 1, 0.001 * k, INF, 16384) for k in range(per + 2)] + [(0, 0, 1, 0.0, INF, 7)]
    assert sum(16 * r[5] for r in reqs) > api.ENVELOPE_PIECE_BYTES
    envs, _ = tm.get_envelopes(reqs)
    for r, env in zip(reqs, envs):
        one, _ = tm.get_envelope(*r)
        assert np.array_equal(env.view(np.uint32), one.view(np.uint32)), r


@pytest.mark.parametrize("devices", [(0,), (0, 0)], ids=["one_slot", "two_slots"])
def test_tmg_equals_tm(tm, devices):
    reqs = _batch()
    want, winfo = tm.get_envelopes(reqs)
    lanes = [(0, 0, 1, 0.0, INF, 333, 64, -1.0, 1.0, 256, (255, 200, 0, 255), (0, 0, 0, 255)), (1, 0, 1, 0.0, INF, 4, 3, -1.0, 1.0, 0, (1, 2, 3, 4), (9, 9, 9, 9)),
             (0, 1, 1, 0.2, 0.9, 2048, 5, -0.2, 0.2, 100, (255, 255, 255, 255), (0, 0, 0, 0))]
    lwant, _ = tm.render_waveform_figures(lanes)
    with ta.MultiTrackManager(list(devices)) as g:
        g.add_tracks(TRACKS)
        g.apply_track_list_changes()
        got, ginfo = g.get_envelopes(reqs)
        assert all(np.array_equal(a, b) for a, b in zip(_bits(want), _bits(got)))
        rev = g.revisions()[0]
        for a, b in zip(winfo, ginfo):
            assert {k: v for k, v in a.items() if k != "waveform_revision"} == {k: v for k, v in b.items() if k != "waveform_revision"}
            assert b["waveform_revision"] == rev
        one, _ = g.get_envelope(*reqs[3])
        assert np.array_equal(one.view(np.uint32), want[3].view(np.uint32))
        lgot, linfo = g.render_waveform_figures(lanes)
        assert all(np.array_equal(a, b) for a, b in zip(lwant, lgot)) and all(i["waveform_revision"] == rev for i in linfo)
        fig, _ = g.render_waveform_figure(*lanes[0])
        assert np.array_equal(fig, lwant[0])


def test_eight_reader_threads(tm):
    reqs = _batch()
    want = _bits(tm.get_envelopes(reqs)[0])
    lane = (0, 0, 1, 0.0, INF, 333, 64, -1.0, 1.0, 256, (255, 200, 0, 255), (0, 0, 0, 255))
    lwant, _ = tm.render_waveform_figure(*lane)
    bad = []

    def work(k):
        try:
            for _ in range(3):
                got = _bits(tm.get_envelopes(reqs)[0])
                if not all(np.array_equal(a, b) for a, b in zip(want, got)):
                    bad.append((k, "envelopes"))
                if k & 1 and not np.array_equal(tm.render_waveform_figure(*lane)[0], lwant):
                    bad.append((k, "lane"))
        except Exception as ex:  # noqa: BLE001
            bad.append((k, repr(ex)))

    ths = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not bad, bad


def test_size_query_and_short_buffers(tm):
    reqs = [_ffi.EnvelopeRequest(0, 0, 1, 0.0, INF, 7, 0), _ffi.EnvelopeRequest(1, 0, 1, 0.0, INF, 4, 0)]
    arr = (_ffi.EnvelopeRequest * 2)(*reqs)
    info, need = (_ffi.EnvelopeInfo * 2)(), C.c_size_t()
    fn = _ffi.lib.th_tm_get_envelopes
    assert fn(tm.handle, arr, 2, None, 0, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert need.value == 44 and [(i.offset, i.length) for i in info] == [(0, 28), (28, 16)]
    assert (info[0].sample_start, info[0].sample_end, info[1].sample_start, info[1].sample_end) == (0, N, 0, 1)
    out = np.full(44, 7.5, np.float32)
    assert fn(tm.handle, arr, 2, out.ctypes.data_as(_ffi.c_f32p), 43, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert (out == 7.5).all() and need.value == 44
    assert fn(tm.handle, arr, 2, out.ctypes.data_as(_ffi.c_f32p), 44, info, C.byref(need)) == _ffi.OK and not (out == 7.5).any()
    assert fn(tm.handle, arr, 0, None, 0, None, C.byref(need)) == _ffi.OK and need.value == 0
    one = _ffi.EnvelopeInfo()
    assert _ffi.lib.th_tm_get_envelope(tm.handle, C.byref(reqs[0]), None, 0, C.byref(one)) == _ffi.ERR_BUFFER_TOO_SMALL and one.length == 28
    lreq = api._waveform_figure_request((0, 0, 1, 0.0, INF, 7, 5, -1.0, 1.0, 256, (1, 2, 3, 4), (0, 0, 0, 0)))
    lreq2 = api._waveform_figure_request((1, 0, 1, 0.0, INF, 3, 3, -1.0, 1.0, 256, (1, 2, 3, 4), (0, 0, 0, 0)))
    larr = (_ffi.WaveformFigureRequest * 2)(lreq, lreq2)
    linfo = (_ffi.WaveformFigureInfo * 2)()
    lfn = _ffi.lib.th_tm_render_waveform_figures
    assert lfn(tm.handle, larr, 2, None, 0, linfo, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert need.value == 192 + 36 and [(i.offset, i.bytes, i.out_w, i.out_h) for i in linfo] == [(0, 140, 7, 5), (192, 36, 3, 3)]
    buf = np.full(228, 0xAB, np.uint8)
    assert lfn(tm.handle, larr, 2, buf.ctypes.data, 227, linfo, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL and (buf == 0xAB).all()
    assert lfn(tm.handle, larr, 2, buf.ctypes.data, 228, linfo, C.byref(need)) == _ffi.OK
    assert (buf[140:192] == 0xAB).all() and not (buf[:140] == 0xAB).all()   # the bytes between two records are not written


def test_errors_write_nothing(tm):
    good = (0, 0, 1, 0.0, INF, 7)
    cases = [((99, 0, 1, 0.0, INF, 7), _ffi.ERR_NOT_FOUND), ((0, 2, 1, 0.0, INF, 7), _ffi.ERR_INVALID_ARG), ((0, 0, 3, 0.0, INF, 7), _ffi.ERR_INVALID_ARG),
             ((0, 0, 1, NAN, INF, 7), _ffi.ERR_INVALID_ARG), ((0, 0, 1, 0.0, NAN, 7), _ffi.ERR_INVALID_ARG), ((0, 0, 1, -1.0, INF, 7), _ffi.ERR_INVALID_ARG),
             ((0, 0, 1, INF, INF, 7), _ffi.ERR_INVALID_ARG), ((0, 0, 1, 1.0, 0.5, 7), _ffi.ERR_INVALID_ARG), ((0, 0, 1, 2.0, 3.0, 7), _ffi.ERR_INVALID_ARG),
             ((0, 0, 1, 0.0, INF, 0), _ffi.ERR_INVALID_ARG), ((0, 0, 1, 0.0, INF, 65537), _ffi.ERR_INVALID_ARG)]
    out = np.full(4 * (7 + 65537) + 8, 7.5, np.float32)
    for bad, code in cases:
        for reqs in ([bad], [good, bad]):
            with pytest.raises(ta.ThError) as ex:
                tm.get_envelopes(reqs, out=out)
            assert ex.value.code == code, bad
            assert (out == 7.5).all(), bad
    # the first faulty request in request order decides
    with pytest.raises(ta.ThError) as ex:
        tm.get_envelopes([good, cases[1][0], cases[0][0]], out=out)
    assert ex.value.code == _ffi.ERR_INVALID_ARG
    with pytest.raises(ta.ThError) as ex:
        tm.get_envelopes([cases[0][0], cases[1][0]], out=out)
    assert ex.value.code == _ffi.ERR_NOT_FOUND
    lgood = (0, 0, 1, 0.0, INF, 7, 5, -1.0, 1.0, 256, (1, 2, 3, 4), (0, 0, 0, 0))
    lcases = [((99,) + lgood[1:], _ffi.ERR_NOT_FOUND), (lgood[:1] + (2,) + lgood[2:], _ffi.ERR_INVALID_ARG), (lgood[:2] + (3,) + lgood[3:], _ffi.ERR_INVALID_ARG),
              (lgood[:3] + (1.0, 0.5) + lgood[5:], _ffi.ERR_INVALID_ARG), (lgood[:5] + (0,) + lgood[6:], _ffi.ERR_INVALID_ARG),
              (lgood[:5] + (16385,) + lgood[6:], _ffi.ERR_INVALID_ARG), (lgood[:6] + (0,) + lgood[7:], _ffi.ERR_INVALID_ARG),
              (lgood[:6] + (16385,) + lgood[7:], _ffi.ERR_INVALID_ARG), (lgood[:7] + (1.0, 1.0) + lgood[9:], _ffi.ERR_INVALID_ARG),
              (lgood[:7] + (1.0, -1.0) + lgood[9:], _ffi.ERR_INVALID_ARG), (lgood[:7] + (NAN, 1.0) + lgood[9:], _ffi.ERR_INVALID_ARG),
              (lgood[:7] + (-1.0, INF) + lgood[9:], _ffi.ERR_INVALID_ARG), (lgood[:9] + (5 * 256 + 1,) + lgood[10:], _ffi.ERR_INVALID_ARG)]
    buf = np.full(1 << 20, 0xAB, np.uint8)
    for bad, code in lcases:
        for reqs in ([bad], [lgood, bad]):
            with pytest.raises(ta.ThError) as ex:
                tm.render_waveform_figures(reqs, out=buf)
            assert ex.value.code == code, bad
            assert (buf == 0xAB).all(), bad


FILL, OPAQUE, CLEAR = (255, 180, 20, 255), (10, 20, 30, 255), (0, 0, 0, 0)
ROWS_OF_A_PIECE = api.FIGURE_PIECE_BYTES // (2048 * 4)
# name, track, ch, start, end, out_w, out_h, amp_lo, amp_hi, thickness, fill, background
LANES = [
    ("333x64", 0, 0, 0.0, INF, 333, 64, -1.0, 1.0, 256, FILL, OPAQUE),
    ("7x5", 0, 1, 0.0, INF, 7, 5, -1.0, 1.0, 256, FILL, CLEAR),
    ("1x1", 0, 0, 0.0, INF, 1, 1, -1.0, 1.0, 256, FILL, OPAQUE),
    ("one_row", 0, 0, 0.3, 1.1, 501, 1, -1.0, 1.0, 64, FILL, CLEAR),
    ("one_column_tall", 0, 1, 0.0, INF, 1, 333, -1.0, 1.0, 0, FILL, OPAQUE),
    ("across_a_lane_piece_boundary", 0, 0, 0.0, INF, 2048, ROWS_OF_A_PIECE + 1, -1.0, 1.0, 256, FILL, OPAQUE),
    ("narrow_amplitude_range_clamps", 0, 0, 0.0, INF, 333, 64, -0.1, 0.05, 256, FILL, CLEAR),
    ("thickness_0", 0, 0, 0.5, 0.50625, 1000, 37, -0.5, 0.5, 0, FILL, OPAQUE),
    ("zoomed_in_thickness_256", 0, 0, 0.5, 0.50625, 1000, 37, -0.5, 0.5, 256, (0, 0, 0, 255), (255, 255, 255, 255)),
    ("thick_line", 0, 1, 0.0, 0.2, 64, 16, -1.0, 1.0, 16 * 256, FILL, CLEAR),
    ("one_sample_track", 1, 0, 0.0, INF, 5, 9, -1.0, 1.0, 300, FILL, OPAQUE),
    ("no_sample_in_the_range", 0, 0, 1000.25 / SR, 1000.75 / SR, 9, 6, -1.0, 1.0, 256, FILL, OPAQUE),
    ("no_sample_one_sample_track", 1, 0, 0.25 / SR, 0.5 / SR, 3, 4, -1.0, 1.0, 128, FILL, CLEAR),
]


def _lane_want(m, r):
    _, track, ch, a, b, out_w, out_h, lo, hi, th, fill, bg = r
    env, _ = m.get_envelope(track, ch, 1, a, b, out_w)
    return R.lane(env, out_h, lo, hi, th, fill, bg), env


@pytest.mark.parametrize("r", LANES, ids=[r[0] for r in LANES])
def test_lane_equals_the_definition(tm, r):
    name, track, ch, a, b, out_w, out_h = r[:7]
    got, info = tm.render_waveform_figure(track, ch, 1, *r[3:])
    want, env = _lane_want(tm, r)
    assert got.shape == (out_h, out_w, 4) and np.array_equal(got, want), (name, int((got != want).any(2).sum()))
    e = ta.envelope_edges(SR, N if track == 0 else 1, a, b, out_w)
    assert (info["offset"], info["bytes"], info["out_w"], info["out_h"]) == (0, out_w * out_h * 4, out_w, out_h)
    assert (info["sample_start"], info["sample_end"], info["waveform_revision"]) == (int(e[0]), int(e[-1]), tm.revisions()[0])
    if name == "333x64":   # it draws: fill in the middle rows, the background at the top
        assert (got[32, :, :] == FILL).all() and (got[0] == OPAQUE).all()
    if name == "narrow_amplitude_range_clamps":
        assert (got[:, :, 3] == 255).all()   # every column reaches both clamps
    if name.startswith("no_sample"):   # one held sample: the same line in every column
        assert e[0] == e[-1] and (got == got[:, :1]).all() and (got[:, 0] != np.uint8(r[-1])).any()
    if name == "across_a_lane_piece_boundary":
        assert out_w * out_h * 4 > api.FIGURE_PIECE_BYTES


def test_lane_batch_equals_single_calls(tm):
    reqs = [r[1:3] + (1,) + r[3:] for r in LANES if r[0] != "across_a_lane_piece_boundary"]
    figs, infos = tm.render_waveform_figures(reqs)
    end = 0
    for r, fig, info in zip(reqs, figs, infos):
        one, _ = tm.render_waveform_figure(*r)
        assert np.array_equal(fig, one), r
        assert info["offset"] % 64 == 0 and info["offset"] == (end + 63) // 64 * 64
        end = info["offset"] + info["bytes"]


def test_lane_of_nan_columns_draws_nothing(tm_nan):
    r = ("nan", 9, 0, 0.0, INF, 12, 8, -1.0, 1.0, 256, FILL, OPAQUE)
    got, _ = tm_nan.render_waveform_figure(9, 0, 1, *r[3:])
    want, env = _lane_want(tm_nan, r)
    assert np.array_equal(got, want)
    assert (got[:, 3] == OPAQUE).all() and (got[:, 1] == OPAQUE).all() and (got[:, 6] == OPAQUE).all()   # all NaN; a NaN mean; inf - inf
    assert (got[:, 5, :3] != OPAQUE[:3]).any(1).sum() >= 4   # +inf: drawn up to the top clamp
    r = ("nan_zoomed", 9, 0, 0.0, INF, 16384, 4, -1.0, 1.0, 128, FILL, CLEAR)
    got, _ = tm_nan.render_waveform_figure(9, 0, 1, *r[3:])
    assert np.array_equal(got, _lane_want(tm_nan, r)[0])
