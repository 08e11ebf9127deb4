"""th_tm_get_loudness_meters / th_tmg_get_loudness_meters (true peak, loudness range, maximum momentary / short-term loudness and the
two curves of resident tracks) against the restatement of tests/loudness_meter_ref.py, th_audio_stats_dev's block energies and the
EBU Tech 3341 true-peak signals.  Everything goes through the TrackManager at a cheap setting."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import thesia_amd as ta
from tests import loudness_meter_ref as mref
from tests import loudness_ref as ref
from thesia_amd import _ffi

pytestmark = pytest.mark.gpu

SETTING = (20.0, 2, 1, ta.LINEAR)
DB = 10.0 / math.log(10.0)  # d(10 log10 E) = DB dE / E


@pytest.fixture(scope="module")
def ctx():
    c = ta.Context(0)
    yield c
    c.close()


def _manager(ctx, tracks):
    tm = ta.TrackManager(ctx)
    tm.set_setting(*SETTING)
    tm.add_tracks(tracks)
    return tm


def _signal(rng, C_, n, kind):
    if kind == "noise":
        return rng.uniform(-0.5, 0.5, (C_, n)).astype(np.float32)
    if kind == "dc":
        return (0.4 + 0.3 * rng.uniform(-1, 1, (C_, n))).astype(np.float32)
    if kind == "clipped":
        return np.clip(rng.normal(0, 1.5, (C_, n)), -1, 1).astype(np.float32)
    if kind == "steps":  # noise whose level moves by the second: a loudness range
        g = 10.0 ** (np.repeat(rng.uniform(-30, -6, -(-n // 8000)), 8000)[:n] / 20.0)
        return (g * rng.uniform(-1, 1, (C_, n))).astype(np.float32)
    raise ValueError(kind)


def _ragged():
    """id -> (sr, x): rates 8 k .. 192 k (F = 4, 2, 1), 1 / 2 / 5 / 6 channels, lengths at the edges of the two series"""
    rng = np.random.default_rng(41)
    s = ref.s100
    specs = [(1, 8000, 1, 4 * s(8000) - 1, "noise"), (2, 8000, 2, 30 * s(8000) - 1, "dc"), (3, 11025, 5, 30 * s(11025), "clipped"),
             (4, 44100, 6, 31 * s(44100) - 1, "noise"), (5, 48000, 2, 3 * 48000 + 7, "dc"), (6, 96000, 2, 30 * s(96000), "dc"),
             (7, 192000, 1, 4 * s(192000) - 1, "clipped"), (8, 8000, 1, 13 * 8000, "steps"), (9, 48000, 1, 4 * s(48000) - 1, "noise"),
             (10, 96000, 1, 4 * s(96000) - 1, "clipped")]
    return {i: (sr, _signal(rng, C_, n, kind)) for i, sr, C_, n, kind in specs}


RAGGED = _ragged()


@pytest.fixture(scope="module")
def ragged(ctx):
    tm = _manager(ctx, [(i, sr, x) for i, (sr, x) in sorted(RAGGED.items())])
    yield tm
    tm.close()


@pytest.fixture(scope="module")
def ragged_want():
    """id -> (restatement in extended precision, restatement in f64): made once"""
    return {i: (mref.meter(x, sr, np.longdouble), mref.meter(x, sr)) for i, (sr, x) in RAGGED.items()}


def _check_series(got, want_ext, want64, what):
    """the bar of tests/test_gpu_loudness.py::_check_track on energies, max(1e-10, 2 x the f64 filter's own rounding), in LUFS"""
    for key in ("momentary", "short_term"):
        g, we, w64 = got[key], want_ext["e_" + key], want64["e_" + key]
        assert g.shape == we.shape, (what, key, g.shape, we.shape)
        nan = np.isnan(we)
        assert np.array_equal(np.isnan(g), nan), (what, key)
        zero = we == 0.0
        assert np.array_equal(np.isneginf(g), zero), (what, key)
        fin = ~nan & ~zero
        if not fin.any():
            continue
        noise = (np.abs(w64[fin] - we[fin]) / we[fin]).max()
        bar = max(1e-10, 2 * noise) * DB
        err = np.abs(g[fin] - mref.lufs(we[fin])).max()
        print(what, key, "err %.3g dB, bar %.3g dB" % (err, bar))
        assert err <= bar, (what, key, err, bar)


def _check_summary(got, x, sr, what):
    """loudness range and maxima from the RETURNED series; the true peak against the f64 restatement"""
    assert got["oversampling"] == mref.factor(sr), what
    assert got["max_momentary_lufs"] == mref.series_max(got["momentary"]), what
    assert got["max_short_term_lufs"] == mref.series_max(got["short_term"]), what
    # (the energies back from LUFS: the same histogram bin unless an energy lies within 1e-15 of a bin edge)
    want_lra = mref.loudness_range(mref.energy(got["short_term"][::10]))
    assert abs(got["loudness_range"] - want_lra) <= 1e-9, (what, got["loudness_range"], want_lra)
    _check_peak(got, x, sr, what)


def _check_peak(got, x, sr, what):
    peaks = mref.true_peaks(x, sr)
    want, bar = max(peaks), mref.true_peak_bar(x, sr)
    err = abs(float(got["true_peak"]) - want)
    assert err <= bar, (what, float(got["true_peak"]), want, bar)
    assert abs(peaks[got["true_peak_channel"]] - want) <= 2 * bar, what  # (the lowest channel at the device's own maximum)
    want_db = -math.inf if got["true_peak"] == 0 else np.float32(20.0 * math.log10(float(got["true_peak"])))
    assert got["true_peak_dB"] == want_db, what


def test_ragged_batch_against_restatement(ctx, ragged, ragged_want):
    ids = sorted(RAGGED)
    got = dict(zip(ids, ragged.loudness_meters(ids)))
    wrev = ragged.revisions()[0]
    # the momentary series is th_audio_stats_dev's block_energy of the same samples, converted
    bufs, args, outs = [], [], {}
    for i in ids:
        sr, x = RAGGED[i]
        chans = [ctx.to_device(np.ascontiguousarray(c)) for c in x]
        nb = ref.n_blocks(x.shape[1], sr)
        o = ctx.alloc(max(nb, 1) * 8)
        bufs += chans + [o]
        outs[i] = (o, nb)
        args.append(([b.ptr for b in chans], x.shape[1], sr, o.ptr))
    stats = dict(zip(ids, ctx.audio_stats_dev(args)))
    energies = {i: o.download((max(nb, 1),), np.float64)[:nb] for i, (o, nb) in outs.items()}
    for b in bufs:
        b.free()
    total = 0
    for i in ids:
        sr, x = RAGGED[i]
        g, (we, w64) = got[i], ragged_want[i]
        assert g["n_momentary"] == ref.n_blocks(x.shape[1], sr) == g["momentary"].size, i
        assert g["n_short_term"] == mref.n_short_term(x.shape[1], sr) == g["short_term"].size, i
        assert (g["momentary_offset"], g["short_term_offset"]) == (total, total + g["n_momentary"]), i
        total += g["n_momentary"] + g["n_short_term"]
        assert g["waveform_revision"] == wrev
        _check_series(g, we, w64, i)
        d = np.abs(g["momentary"] - mref.lufs(energies[i]))
        assert d.size == 0 or d.max() <= 1e-12, (i, d.max())
        _check_summary(g, x, sr, i)
        if g["oversampling"] == 1:
            assert g["true_peak"] == np.float32(stats[i]["max_peak"]) == np.float32(ragged.audio_stats(i)["max_peak"]), i
    assert got[8]["n_short_term"] == 101 and got[8]["loudness_range"] > 1.0  # 11 blocks, one per second
    assert got[1]["n_momentary"] == 0 and got[1]["max_momentary_lufs"] == -math.inf and got[1]["loudness_range"] == 0.0
    assert got[7]["oversampling"] == 1 and got[6]["oversampling"] == 2 and got[5]["oversampling"] == 4


def _tech_3341(sr):
    n = sr // 2
    t, k = np.arange(n), sr // 100
    fade = np.ones(n)
    fade[:k] = 0.5 * (1.0 - np.cos(np.pi * np.arange(k) / k))
    fade[-k:] = fade[:k][::-1]
    cases = [(0.5, 4, 0.0, -6.0), (0.5, 4, 45.0, -6.0), (0.5, 6, 60.0, -6.0), (0.5, 8, 67.5, -6.0), (1.41, 4, 45.0, 3.0)]
    return [((a * np.sin(2 * np.pi * t / per + np.deg2rad(ph)) * fade).astype(np.float32)[None], want) for a, per, ph, want in cases]


@pytest.mark.parametrize("sr", [48000, 44100])
def test_ebu_tech_3341_true_peak_cases_15_to_19(ctx, sr):
    cases = _tech_3341(sr)
    tm = _manager(ctx, [(15 + k, sr, x) for k, (x, _) in enumerate(cases)])
    got = tm.loudness_meters(range(15, 20), series=False)
    tm.close()
    for k, ((x, want), g) in enumerate(zip(cases, got)):
        print(15 + k, sr, float(g["true_peak_dB"]))
        assert want - 0.4 <= g["true_peak_dB"] <= want + 0.2, (15 + k, g["true_peak_dB"])
        _check_peak(g, x, sr, 15 + k)


SEAM_N = 3 * 16384 + 5


def _seam_positions():
    ps = {0, SEAM_N - 2}
    for B in (64, 256, 1024, 4096, 16384):
        for m in range(0, SEAM_N // B + 2):
            for o in (-24, -12, -11, -1, 0, 1, 11, 12, 23):
                if 0 <= m * B + o <= SEAM_N - 2:
                    ps.add(m * B + o)
    return sorted(ps)


def test_chunk_seams(ctx):
    """two adjacent samples of 0.5 at p, p + 1 in 0.01 noise: the inter-sample peak of about 0.64 lands 5 - 6 outputs later,
    whatever chunk and run lengths the kernel cuts the channel into (the pair at n - 2 is seen only partly, by definition)"""
    sr = 48000
    rng = np.random.default_rng(43)
    base = rng.uniform(-0.01, 0.01, SEAM_N).astype(np.float32)
    hs = mref.phase_filters(sr)
    reach = max(h.size for h in hs)
    # the restatement of every track from the noise's own outputs: prefix / suffix maxima of |y| plus the outputs the pair reaches,
    # recomputed with the same f64 operations in the same order
    ys = [mref._causal_fir(base.astype(np.float64), h) for h in hs]
    a = np.max(np.abs(np.stack(ys)), axis=0)
    pre = np.concatenate([[0.0], np.maximum.accumulate(a)])         # pre[i] = max a[:i]
    suf = np.concatenate([np.maximum.accumulate(a[::-1])[::-1], [0.0]])  # suf[i] = max a[i:]
    ps = _seam_positions()
    bar = mref.true_peak_bar(np.float32(0.5), sr)
    worst, seen = 0.0, 0
    for lo in range(0, len(ps), 2048):
        part = ps[lo:lo + 2048]
        xs = np.repeat(base[None], len(part), 0)
        for r, p in enumerate(part):
            xs[r, p:p + 2] = 0.5
        tm = _manager(ctx, [(r, sr, xs[r:r + 1]) for r in range(len(part))])
        got = tm.loudness_meters(range(len(part)), series=False)
        tm.close()
        for r, p in enumerate(part):
            w0, w1 = max(0, p - reach), min(SEAM_N, p + 2 + reach)
            seg = xs[r, w0:w1].astype(np.float64)
            hi = min(SEAM_N, p + 1 + reach)
            local = max(np.abs(mref._causal_fir(seg, h)[p - w0:hi - w0]).max() for h in hs)
            want = max(pre[p], local, suf[hi])
            err = abs(float(got[r]["true_peak"]) - want)
            worst = max(worst, err)
            seen += 1
            assert err <= bar, (p, float(got[r]["true_peak"]), want, bar)
            assert want > 0.6 or p > SEAM_N - 10, (p, want)
    print("seams: %d tracks, worst error %.3g, bar %.3g" % (seen, worst, bar))
    # the local restatement is the full one
    full = np.array(base)
    full[ps[len(ps) // 2]:ps[len(ps) // 2] + 2] = 0.5
    p = ps[len(ps) // 2]
    hi = min(SEAM_N, p + 1 + reach)
    w0 = max(0, p - reach)
    local = max(np.abs(mref._causal_fir(full[w0:min(SEAM_N, p + 2 + reach)].astype(np.float64), h)[p - w0:hi - w0]).max() for h in hs)
    assert max(pre[p], local, suf[hi]) == mref.true_peak(full[None], sr)[0]


def test_values_nan_zero_signed_zero(ctx):
    rng = np.random.default_rng(44)
    sr, n = 8000, 31 * 800
    nan = _signal(rng, 2, n, "noise")
    nan[1, n // 2] = np.nan
    zero = np.zeros((2, n), np.float32)
    mixed = np.zeros((1, n), np.float32)
    mixed[0, ::3] = -0.0
    tm = _manager(ctx, [(1, sr, nan), (2, sr, zero), (3, sr, mixed)])
    g_nan, g_zero, g_mixed = tm.loudness_meters([1, 2, 3])
    tm.close()
    # a NaN sample is ignored in the peak; the blocks that hold it stay NaN in the series and are ignored in the maxima
    _check_peak(g_nan, nan, sr, "nan")
    assert g_nan["true_peak"] > 0
    we, w64 = mref.meter(nan, sr, np.longdouble, sequential=True), mref.meter(nan, sr, sequential=True)
    assert np.isnan(we["e_momentary"]).any() and np.isnan(we["e_short_term"]).all()
    _check_series(g_nan, we, w64, "nan")
    assert g_nan["max_momentary_lufs"] == mref.series_max(g_nan["momentary"]) > -math.inf
    assert g_nan["max_short_term_lufs"] == -math.inf and g_nan["loudness_range"] == 0.0
    for g in (g_zero, g_mixed):
        assert g["true_peak"] == 0 and g["true_peak_dB"] == -math.inf and g["true_peak_channel"] == 0
        assert g["loudness_range"] == 0.0 and g["max_momentary_lufs"] == -math.inf == g["max_short_term_lufs"]
        assert g["momentary"].size == 28 and g["short_term"].size == 2
        assert np.isneginf(g["momentary"]).all() and np.isneginf(g["short_term"]).all()


def _same(a, b):
    """two meter dicts: the same bytes (NaN == NaN), series included; offsets relative to the track's own first double"""
    a = dict(a, momentary_offset=0, short_term_offset=a["short_term_offset"] - a["momentary_offset"])
    b = dict(b, momentary_offset=0, short_term_offset=b["short_term_offset"] - b["momentary_offset"])
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def test_derived_audio(ctx):
    """after a peak normalise with the limiter the meter measures the derived audio; back to Off it measures the original again"""
    rng = np.random.default_rng(45)
    sr = 8000
    tracks = [(1, sr, _signal(rng, 2, 31 * 800 + 9, "noise")), (2, sr, _signal(rng, 1, 33 * 800, "steps"))]
    tm = _manager(ctx, tracks)
    first = tm.loudness_meters([1, 2])
    tm.set_common_guard_clipping(ta.api.GUARD_LIMITER)
    tm.set_common_normalize(ta.api.NORM_PEAK_DB, 3.0)
    got = tm.loudness_meters([1, 2])
    for (i, _, x), g in zip(tracks, got):
        y = np.stack([tm.audio(i, c) for c in range(x.shape[0])])
        assert not np.array_equal(y, x)
        assert g["waveform_revision"] == tm.revisions()[0] != first[0]["waveform_revision"]
        _check_series(g, mref.meter(y, sr, np.longdouble), mref.meter(y, sr), ("derived", i))
        _check_summary(g, y, sr, ("derived", i))
    tm.set_common_normalize(ta.api.NORM_OFF, 0.0)
    again = tm.loudness_meters([1, 2])
    for a, b in zip(first, again):
        assert b["waveform_revision"] == tm.revisions()[0]
        b = dict(b, waveform_revision=a["waveform_revision"])
        assert _same(a, b)
    tm.close()


def _raw(mgr, ids, cap=None, want_series=True):
    """through the raw ABI into a sentinel-filled buffer -> (rc, meters as bytes, series array, out_len)"""
    fn = getattr(_ffi.lib, mgr._PFX + "get_loudness_meters")
    n = len(ids)
    arr = (C.c_size_t * n)(*ids)
    ms = (_ffi.LoudnessMeter * n)()
    C.memset(ms, 0xA5, C.sizeof(ms))
    need = C.c_size_t(12345)
    buf = np.full(1 << 12, -777.0) if want_series else None
    rc = fn(mgr.handle, arr, n, ms, buf.ctypes.data_as(C.POINTER(C.c_double)) if want_series else None,
            (buf.size if cap is None else cap) if want_series else 0, C.byref(need))
    return rc, bytes(ms), buf, need.value


def test_independence_and_refusals(ctx, ragged):
    ids = sorted(RAGGED)
    rc, mbytes, series, total = _raw(ragged, ids)
    assert rc == 0 and total < series.size and np.all(series[total:] == -777.0)
    every = ragged.loudness_meters(ids)
    by_id = dict(zip(ids, every))
    # alone, twice in one batch, from four threads at once
    for i in (2, 4, 6):
        assert _same(ragged.loudness_meter(i), by_id[i]), i
    twice = ragged.loudness_meters([5, 3, 5])
    assert _same(twice[0], twice[2]) and _same(twice[0], by_id[5]) and _same(twice[1], by_id[3])
    assert twice[2]["momentary_offset"] == twice[1]["short_term_offset"] + twice[1]["n_short_term"]
    results, errors = [None] * 4, []

    def work(k):
        try:
            results[k] = _raw(ragged, ids)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for r in results:
        assert r[0] == 0 and r[1] == mbytes and r[3] == total and r[2][:total].tobytes() == series[:total].tobytes()
    # series == NULL: the same meters
    rc, mb2, _, t2 = _raw(ragged, ids, want_series=False)
    assert rc == 0 and mb2 == mbytes and t2 == total
    # a short buffer: the size, the counts, nothing written
    rc, mb3, s3, t3 = _raw(ragged, ids, cap=total - 1)
    assert rc == _ffi.ERR_BUFFER_TOO_SMALL and t3 == total and np.all(s3 == -777.0)
    short = (_ffi.LoudnessMeter * len(ids)).from_buffer_copy(mb3)
    for m, g in zip(short, every):
        assert (m.n_momentary, m.n_short_term, m.momentary_offset, m.short_term_offset) == \
            (g["n_momentary"], g["n_short_term"], g["momentary_offset"], g["short_term_offset"])
    # an unknown id second in the batch: nothing is written
    rc, mb4, s4, _ = _raw(ragged, [ids[0], 999, ids[1]])
    assert rc == _ffi.ERR_NOT_FOUND and set(mb4) == {0xA5} and np.all(s4 == -777.0)
    # NULL meters, NULL ids
    fn = _ffi.lib.th_tm_get_loudness_meters
    need = C.c_size_t()
    assert fn(ragged.handle, (C.c_size_t * 1)(1), 1, None, None, 0, C.byref(need)) == _ffi.ERR_INVALID_ARG
    assert fn(ragged.handle, None, 1, (_ffi.LoudnessMeter * 1)(), None, 0, C.byref(need)) == _ffi.ERR_INVALID_ARG
    # the manager over devices: the same bytes on one slot and on two
    for devices in ([0], [0, 0]):
        with ta.MultiTrackManager(devices) as mg:
            mg.set_setting(*SETTING)
            mg.add_tracks([(i, sr, x) for i, (sr, x) in sorted(RAGGED.items())])
            rc, mbg, sg, tg = _raw(mg, ids)
            assert rc == 0 and tg == total and sg[:total].tobytes() == series[:total].tobytes(), devices
            assert np.all(sg[total:] == -777.0)
            a = (_ffi.LoudnessMeter * len(ids)).from_buffer_copy(mbg)
            b = (_ffi.LoudnessMeter * len(ids)).from_buffer_copy(mbytes)
            wrev = mg.revisions()[0]
            for x, y in zip(a, b):
                assert x.waveform_revision == wrev
                x.waveform_revision = y.waveform_revision
            assert bytes(a) == bytes(b), devices
            rc, _, s5, _ = _raw(mg, [ids[0], 999])
            assert rc == _ffi.ERR_NOT_FOUND and np.all(s5 == -777.0)
            if len(devices) == 1:
                continue
            # both slots own tracks and take turns in the id list: each writes its tracks' values between the other's.  The list
            # reversed: every track's meter and values again, at other places
            owners = [mg.device_of(i) for i in ids]
            assert set(owners) == {0, 1} and any(p != q for p, q in zip(owners, owners[1:]))
            rc, mbr, sr_, tr_ = _raw(mg, ids[::-1])
            assert rc == 0 and tr_ == total and np.all(sr_[total:] == -777.0)
            r = (_ffi.LoudnessMeter * len(ids)).from_buffer_copy(mbr)[::-1]
            a = (_ffi.LoudnessMeter * len(ids)).from_buffer_copy(mbg)
            for x, y in zip(a, r):
                k = x.n_momentary + x.n_short_term
                assert y.short_term_offset == y.momentary_offset + y.n_momentary
                assert sr_[y.momentary_offset: y.momentary_offset + k].tobytes() == sg[x.momentary_offset: x.momentary_offset + k].tobytes()
                y.momentary_offset, y.short_term_offset = x.momentary_offset, x.short_term_offset
                assert bytes(y) == bytes(x)
