"""Alignment of two tracks on the GPU (th_tm_align_tracks and the th_tmg twin).

Reference: th_align_f64, the host function that runs the kernel's own arithmetic, applied to the samples th_tm_copy_audio returns.  The
contract is bit identity, for the summary and for the curve: every comparison here is of bits, a NaN being a NaN
(tests/test_align_host.py checks that host function against the numpy restatement, a derived error bound and known answers)."""
import ctypes as C

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
SR = 48000
SUMMARY, CURVE = ta.ALIGN_OUT_SUMMARY, ta.ALIGN_OUT_CURVE
TILE = 1024            # ALIGN_TILE: the lags of one workgroup
PIECE = 65536          # TH_ALIGN_PIECE_LAGS
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 131071, 131072, 131073, 2 * 131072 + 5]
N_LONG = 2 * 131072 + 5 + 10


def bits(a):
    a = np.ascontiguousarray(a, np.float64)
    return np.where(np.isnan(a), np.float64(NAN), a).view(np.uint64)


def noise(seed, n):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def sec(sample, sr=SR):
    """a time whose product with sr rounds up to exactly `sample`"""
    t = sample / sr
    while np.ceil(t * float(sr)) > sample:
        t = float(np.nextafter(t, 0.0))
    assert np.ceil(t * float(sr)) == sample
    return t


def _late(x, d, n, gain, seed):
    """x delayed by d samples, scaled, plus a little noise, n samples"""
    y = 0.01 * noise(seed, n)
    m = min(n - d, x.size)
    y[d:d + m] += gain * x[:m]
    return y.astype(np.float32)


_A = np.stack([noise(1, N_LONG), noise(2, N_LONG)])
# 1: the long reference; 2: a late, quieter copy of it (5 and 2 samples), a little longer; 3: another rate; 4, 5: short ones
TRACKS = [(1, SR, _A),
          (2, SR, np.stack([_late(_A[0], 5, N_LONG + 37, 0.5, 3), _late(_A[1], 2, N_LONG + 37, -0.25, 4)])),
          (3, 44100, noise(5, 3000)[None, :]),
          (4, SR, np.stack([noise(6, 5000), noise(7, 5000)])),
          (5, SR, _late(noise(6, 5000), 700, 4000, 0.75, 8)[None, :])]
RATE = {i: sr for i, sr, _ in TRACKS}


def request(ref_id, ref_ch, track_id, ch, s0=0, s1=None, D=8, kind=SUMMARY, flags=0, ref_which=0, which=0):
    sr = RATE.get(ref_id, SR)
    return ta.align_request(ref_id, ref_ch, track_id, ch, sec(s0, sr), INF if s1 is None else sec(s1, sr), D / RATE.get(track_id, SR), kind, flags,
                            ref_which, which)


@pytest.fixture(scope="module")
def ctx():
    c = ta.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tm(ctx):
    m = ta.TrackManager(ctx)
    m.add_tracks(TRACKS)
    m.apply_track_list_changes()
    yield m
    m.close()


_WANT = {}


def want_of(m, req):
    """the host's answer for a request on the manager's own samples, computed once per request and never written to"""
    key = bytes(req)
    if key not in _WANT:
        ref, probe = m.audio(req.ref_id, req.ref_ch, req.ref_which), m.audio(req.id, req.ch, req.which)
        out = ta.align_f64(ref, RATE.get(req.ref_id, SR), probe, RATE.get(req.id, SR), req)
        out.setflags(write=False)
        _WANT[key] = out
    return _WANT[key]


def check(m, reqs, owner=None):
    outs, infos = m.align_tracks(reqs)
    for req, got, info in zip(reqs, outs, infos):
        want = want_of(owner or m, req)
        assert got.size == want.size == info["length"]
        bad = np.nonzero(bits(got) != bits(want))[0]
        assert bad.size == 0, (bytes(req).hex(), bad[:5], got[bad[:5]], want[bad[:5]], got[:10], want[:10])
    return outs, infos


@pytest.mark.parametrize("N", SIZES)
def test_both_kinds_bit_identical_to_the_host(tm, N):
    s0 = 3      # an odd first sample
    reqs = [request(1, 0, 2, 0, s0, s0 + N, 8, kind) for kind in (SUMMARY, CURVE)]
    (summ, curve), (i0, i1) = check(tm, reqs)
    assert (i1["sample_start"], i1["sample_end"], i1["max_lag"], i1["sr"], i1["length"]) == (s0, s0 + N, 8, SR, 10 + 17)
    assert i0["length"] == 10 and i0["waveform_revision"] == tm.revisions()[0]
    assert np.array_equal(bits(summ), bits(curve[:10])) and summ[0] == 0.0
    if N >= 4095:   # the copy is 5 samples late, at half the level
        s = ta.align_summary(summ)
        assert s["lag"] == 5 and s["polarity"] == 1.0 and abs(s["gain"] - 0.5) < 0.01 and s["rho"] > 0.99 and s["null_dB"] < -25.0
        assert abs(s["delta"]) < 0.1


@pytest.mark.parametrize("D", [(TILE - 2) // 2, TILE // 2, (2 * TILE - 2) // 2, 2 * TILE // 2], ids=["tile_minus_1", "tile_plus_1", "two_tiles_minus_1", "two_tiles_plus_1"])
def test_lag_counts_around_the_tile(tm, D):
    """n_lags = 2 D + 1 is odd: one below and one above the tile, one below and one above twice the tile"""
    assert 2 * D + 1 in (TILE - 1, TILE + 1, 2 * TILE - 1, 2 * TILE + 1)
    outs, _ = check(tm, [request(4, 0, 5, 0, 100, 4197, D, CURVE), request(4, 0, 5, 0, 1001, 1300, D, SUMMARY)])
    if D >= 700:
        assert outs[0][1] == 700.0


def test_two_tracks_and_one_track_against_itself(tm):
    reqs = [request(1, 0, 2, 0, 1000, 9001, 40, CURVE), request(2, 0, 1, 0, 1000, 9001, 40, CURVE),      # the roles swapped: the lag's sign flips
            request(1, 0, 1, 0, 1000, 9001, 40, CURVE), request(1, 0, 1, 1, 1000, 9001, 40), request(4, 1, 4, 1, 0, None, 30, CURVE)]
    outs, _ = check(tm, reqs)
    assert outs[0][1] == 5.0 and outs[1][1] == -5.0
    own = ta.align_summary(outs[2])     # a channel against itself: lag 0, gain 1, a perfect null
    assert own["lag"] == 0.0 and own["gain"] == 1.0 and own["null_dB"] == -INF and own["e_ref"] == own["e_probe"] == own["r"]
    assert outs[4][1] == 0.0 and outs[4][7] == 1.0


def test_ranges_at_both_track_ends_and_a_probe_the_lags_leave(tm):
    n = 5000
    reqs = [request(4, 0, 4, 1, 0, 900, 300, CURVE), request(4, 0, 4, 1, n - 900, None, 300, CURVE), request(4, 0, 4, 1, n - 1, None, 5, CURVE),
            request(4, 0, 5, 0, 3500, None, 900, CURVE),        # the probe (4000 samples) ends inside the range
            request(4, 0, 4, 1, 0, None, 0, CURVE), request(4, 0, 4, 1, 77, 77, 9, CURVE)]     # lag 0 only; an empty range
    outs, infos = check(tm, reqs)
    assert outs[4].size == 11 and outs[5].size == 10 and outs[5][0] == 1.0 and np.isnan(outs[5][1:]).all()
    assert (infos[5]["sample_start"], infos[5]["sample_end"], infos[5]["length"]) == (77, 77, 10)


def test_the_inverted_copy_and_abs(tm):
    plain, absd = check(tm, [request(1, 1, 2, 1, 2001, 30000, 16), request(1, 1, 2, 1, 2001, 30000, 16, flags=ta.ALIGN_ABS)])[0]
    s = ta.align_summary(absd)
    assert s["lag"] == 2.0 and s["polarity"] == -1.0 and abs(s["gain"] + 0.25) < 0.01 and s["null_dB"] < -25.0
    assert ta.align_summary(plain)["null_dB"] > -1.0


def _mixed_batch():
    return [request(1, 0, 2, 0, 3, 4100, 8, CURVE), request(4, 0, 5, 0, 100, 4197, 600, SUMMARY), request(1, 1, 1, 0, 0, 131073, 2, CURVE),
            request(4, 1, 4, 1, 77, 77, 9, CURVE), request(2, 1, 1, 1, 500, 70000, 12, SUMMARY, ta.ALIGN_ABS), request(4, 0, 5, 0, 1001, 1300, TILE, CURVE)]


def test_mixed_batch_equals_single_calls_with_canaries(tm):
    reqs = _mixed_batch()
    single = [tm.align_tracks([r])[0][0] for r in reqs]
    need = sum(s.size for s in single)
    buf = np.full(need + 16, -77.25)
    outs, infos = tm.align_tracks(reqs, out=buf[8:8 + need])
    assert (buf[:8] == -77.25).all() and (buf[8 + need:] == -77.25).all()
    at = 0
    for req, got, s, info in zip(reqs, outs, single, infos):
        assert info["offset"] == at and info["length"] == s.size    # back to back: nothing between two records
        assert np.array_equal(bits(got), bits(s)) and np.array_equal(bits(s), bits(want_of(tm, req)))
        at += s.size
    rev = list(reversed(reqs))
    for got, s in zip(tm.align_tracks(rev)[0], reversed(single)):
        assert np.array_equal(bits(got), bits(s))
    one, info = tm.align_track(1, 0, 2, 0, start_sec=sec(3), end_sec=sec(4100), max_lag_sec=8 / SR, kind=CURVE)
    assert np.array_equal(bits(one), bits(single[0])) and info["length"] == one.size


def test_size_query_and_short_buffers(tm):
    reqs = [request(4, 0, 5, 0, 100, 900, 20, CURVE), request(4, 0, 5, 0, 100, 900, 20)]
    arr = (_ffi.AlignRequest * 2)(*reqs)
    info, need = (_ffi.AlignInfo * 2)(), C.c_size_t()
    f64p = C.POINTER(C.c_double)
    assert api.lib.th_tm_align_tracks(tm.handle, arr, 2, None, 0, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert need.value == 61 and (info[0].offset, info[0].length, info[1].offset, info[1].length) == (0, 51, 51, 10)
    assert (info[0].sample_start, info[0].sample_end, info[0].max_lag, info[0].sr) == (100, 900, 20, SR)
    buf = np.full(61, -3.5)
    assert api.lib.th_tm_align_tracks(tm.handle, arr, 2, buf.ctypes.data_as(f64p), 60, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert (buf == -3.5).all() and need.value == 61
    one = _ffi.AlignInfo()
    assert api.lib.th_tm_align_track(tm.handle, C.byref(reqs[0]), None, 0, C.byref(one)) == _ffi.ERR_BUFFER_TOO_SMALL and one.length == 51
    assert api.lib.th_tm_align_tracks(tm.handle, None, 0, None, 0, None, C.byref(need)) == _ffi.OK and need.value == 0
    assert api.lib.th_tm_align_tracks(tm.handle, arr, 2, buf.ctypes.data_as(f64p), 61, None, C.byref(need)) == _ffi.ERR_INVALID_ARG
    assert api.lib.th_tm_align_tracks(None, arr, 2, buf.ctypes.data_as(f64p), 61, info, C.byref(need)) == _ffi.ERR_INVALID_ARG
    assert (buf == -3.5).all()
    assert tm.align_tracks([]) == ([], [])


def test_errors_write_nothing(tm):
    good = dict(ref_id=4, ref_ch=0, track_id=5, ch=0, start_sec=0.01, end_sec=0.02, max_lag_sec=0.001)
    cases = [(dict(good, track_id=99), _ffi.ERR_NOT_FOUND), (dict(good, ref_id=99), _ffi.ERR_NOT_FOUND), (dict(good, ch=1), _ffi.ERR_INVALID_ARG),
             (dict(good, ref_ch=2), _ffi.ERR_INVALID_ARG), (dict(good, which=3), _ffi.ERR_INVALID_ARG), (dict(good, ref_which=3), _ffi.ERR_INVALID_ARG),
             (dict(good, kind=2), _ffi.ERR_INVALID_ARG), (dict(good, flags=2), _ffi.ERR_INVALID_ARG), (dict(good, start_sec=NAN), _ffi.ERR_INVALID_ARG),
             (dict(good, end_sec=NAN), _ffi.ERR_INVALID_ARG), (dict(good, max_lag_sec=NAN), _ffi.ERR_INVALID_ARG), (dict(good, max_lag_sec=-0.1), _ffi.ERR_INVALID_ARG),
             (dict(good, max_lag_sec=INF), _ffi.ERR_INVALID_ARG), (dict(good, start_sec=0.5, end_sec=0.1), _ffi.ERR_INVALID_ARG),
             (dict(good, start_sec=-1.0), _ffi.ERR_INVALID_ARG),
             (dict(good, ref_id=3), _ffi.ERR_UNSUPPORTED), (dict(good, track_id=3), _ffi.ERR_UNSUPPORTED),          # unequal rates, either way round
             (dict(good, max_lag_sec=((1 << 20) + 1) / SR), _ffi.ERR_UNSUPPORTED),
             (dict(good, ref_id=3, ch=7), _ffi.ERR_INVALID_ARG),          # a bad channel is reported before the rates
             (dict(good, track_id=98, ref_id=99), _ffi.ERR_NOT_FOUND)]
    for bad, code in cases:
        buf = np.full(4096, -9.5)
        with pytest.raises(ta.ThError) as ex:
            tm.align_tracks([good, bad, good], out=buf)
        assert ex.value.code == code, (bad, ex.value.code, str(ex.value))
        assert (buf == -9.5).all(), bad
    with pytest.raises(ta.ThError) as ex:   # the probe's id is looked at first
        tm.align_tracks([dict(good, track_id=98, ref_id=99)])
    assert "98" in str(ex.value)
    with pytest.raises(ta.ThError) as ex:   # the first faulty request decides
        tm.align_tracks([good, dict(good, kind=5), dict(good, track_id=99)], out=np.full(4096, -9.5))
    assert ex.value.code == _ffi.ERR_INVALID_ARG


def test_a_reference_above_the_limit_is_refused(ctx):
    m = ta.TrackManager(ctx)
    try:
        n = (1 << 22) + 1
        m.add_tracks([(1, SR, np.zeros((1, n), np.float32))])
        m.apply_track_list_changes()
        with pytest.raises(ta.ThError) as ex:
            m.align_tracks([dict(ref_id=1, track_id=1, max_lag_sec=0.0)])
        assert ex.value.code == _ffi.ERR_UNSUPPORTED
        with pytest.raises(ta.ThError) as ex:       # 2^22 samples x (2^18 + 1) lags: above 2^40
            m.align_tracks([dict(ref_id=1, track_id=1, end_sec=sec(1 << 22), max_lag_sec=(1 << 17) / SR)])
        assert ex.value.code == _ffi.ERR_UNSUPPORTED
        out, info = m.align_track(1, 0, 1, 0, end_sec=sec(1 << 22), max_lag_sec=0.0)     # the limit itself, all zeros: E_ref = 0 is invalid
        assert info["sample_end"] == 1 << 22 and out[0] == 1.0
    finally:
        m.close()


def test_which_and_revisions_under_a_set_normalisation(ctx):
    m = ta.TrackManager(ctx)
    try:
        n = 9000
        m.add_tracks([(5, SR, np.stack([noise(3, n), 0.3 * noise(4, n)])), (6, SR, _late(noise(3, n), 11, n, 0.9, 9)[None, :])])
        m.apply_track_list_changes()
        rev0 = m.revisions()[0]
        assert m.align_track(5, 0, 6, 0, max_lag_sec=20 / SR)[1]["waveform_revision"] == rev0
        m.set_common_normalize(api.NORM_PEAK_DB, -9.0)
        rev1 = m.revisions()[0]
        assert rev1 != rev0
        assert not np.array_equal(m.audio(5, 1, 0), m.audio(5, 1, 2))
        gains = []
        for ref_which in (0, 1, 2):
            for which in (0, 1, 2):
                reqs = [request(5, 0, 6, 0, 1001, 8000, 20, CURVE, 0, ref_which, which), request(5, 1, 5, 0, 1001, 8000, 20, SUMMARY, 0, ref_which, which)]
                outs, infos = check(m, reqs)
                assert infos[0]["waveform_revision"] == rev1 and outs[0][1] == 11.0
                gains.append(outs[0][7])
        assert len(set(gains)) > 1    # the normalisation moves the gain between audio and original
    finally:
        m.close()


def test_non_finite_samples(ctx):
    m = ta.TrackManager(ctx)
    try:
        a, b = noise(11, 3200), noise(12, 3500)
        a[1500], b[3010] = NAN, NAN
        m.add_tracks([(1, SR, a[None, :]), (2, SR, b[None, :])])
        m.apply_track_list_changes()
        if not (np.isnan(m.audio(1, 0, 2)[1500]) and np.isnan(m.audio(2, 0, 2)[3010])):
            pytest.fail("the manager did not keep the NaN samples")
        reqs = [request(1, 0, 2, 0, 1000, 2000, 5, CURVE, ref_which=2, which=2),       # the NaN in the reference: invalid, every lag NaN
                request(1, 0, 2, 0, 2000, 3000, 12, CURVE, ref_which=2, which=2),      # the NaN in the probe: exactly the lags that meet it
                request(1, 0, 2, 0, 1501, 2900, 12, CURVE, ref_which=2, which=2)]      # neither: valid
        outs, _ = check(m, reqs)
        assert outs[0][0] == 1.0 and np.isnan(outs[0][1:]).all()
        hit = np.array([2000 <= 3010 - l < 3000 for l in range(-12, 13)])
        assert np.array_equal(np.isnan(outs[1][10:]), hit) and hit.any() and not hit.all() and outs[1][0] == 1.0
        assert outs[2][0] == 0.0 and not np.isnan(outs[2]).any()
    finally:
        m.close()


def test_a_request_just_over_two_pieces_run_twice(tm):
    D = PIECE + 2       # 2 D + 1 = 2 pieces + 5 lags
    big = request(4, 0, 5, 0, 2000, 2300, D, CURVE)
    other = request(4, 1, 4, 0, 0, 500, 3, CURVE)
    want = want_of(tm, big)
    assert want.size == 10 + 2 * PIECE + 5
    for _ in range(2):
        (got, small), (info, _) = check(tm, [big, other])
        assert info["length"] == want.size and got[1] == 700.0
    summ = check(tm, [request(4, 0, 5, 0, 2000, 2300, D, SUMMARY)])[0][0]
    assert np.array_equal(bits(summ), bits(want[:10]))


@pytest.mark.parametrize("devices", [(0,), (0, 0)], ids=["one_slot", "two_slots"])
def test_tmg_equals_tm(tm, devices):
    # every ordered pair of tracks 1, 2, 4, 5 and each against itself: with two slots some pairs share a slot and some do not
    ids = (1, 2, 4, 5)
    reqs = [request(r, 0, p, 0, 3, 3900, 9, CURVE if (r + p) % 2 else SUMMARY) for r in ids for p in ids] + _mixed_batch()
    want, winfo = tm.align_tracks(reqs)
    with ta.MultiTrackManager(list(devices)) as g:
        g.add_tracks(TRACKS)
        g.apply_track_list_changes()
        for _ in range(2):
            got, ginfo = g.align_tracks(reqs)
            rev = g.revisions()[0]
            for a, b, wa, wb in zip(want, got, winfo, ginfo):
                assert np.array_equal(bits(a), bits(b))
                assert {k: v for k, v in wa.items() if k != "waveform_revision"} == {k: v for k, v in wb.items() if k != "waveform_revision"}
                assert wb["waveform_revision"] == rev
        buf = np.full(64, -9.5)
        one, info = g.align_track(1, 0, 2, 0, start_sec=sec(3), end_sec=sec(4100), max_lag_sec=8 / SR, kind=CURVE)
        assert np.array_equal(bits(one), bits(want_of(tm, request(1, 0, 2, 0, 3, 4100, 8, CURVE)))) and info["length"] == one.size
        for bad, code in ((dict(ref_id=1, track_id=99), _ffi.ERR_NOT_FOUND), (dict(ref_id=99, track_id=1), _ffi.ERR_NOT_FOUND),
                          (dict(ref_id=3, track_id=1), _ffi.ERR_UNSUPPORTED), (dict(ref_id=1, track_id=2, ref_ch=5), _ffi.ERR_INVALID_ARG),
                          (dict(ref_id=1, track_id=2, kind=3), _ffi.ERR_INVALID_ARG)):
            with pytest.raises(ta.ThError) as ex:
                g.align_tracks([dict(ref_id=4, track_id=5, end_sec=0.01), bad], out=buf)
            assert ex.value.code == code and (buf == -9.5).all(), bad
        need = C.c_size_t()
        arr = (_ffi.AlignRequest * 1)(request(1, 0, 2, 0, 3, 4100, 8, CURVE))
        info1 = (_ffi.AlignInfo * 1)()
        assert api.lib.th_tmg_align_tracks(g.handle, arr, 1, buf.ctypes.data_as(C.POINTER(C.c_double)), 26, info1, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
        assert need.value == 27 and info1[0].length == 27 and (buf == -9.5).all()
