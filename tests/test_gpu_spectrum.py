"""Spectrum of a time range (th_tm_get_spectra / th_tm_get_spectrum and the th_tmg twins) on resident specs.

Reference: numpy f64 on the rows th_tm_copy_spec returns for the same (id, ch) — existing code, not the code under test:
  mean amplitude 20 log10((1 / n) sum 10^(s / 20)), mean power 10 log10((1 / n) sum 10^(s / 10)), maximum max s; -inf rows count
  in n, an all -inf column gives -inf, a NaN in the column's range gives NaN, n = 0 gives NaN.
Tolerance of the two means: max(2e-5 dB, 2 f32 ulps of the value) — an f32-accurate exp2 contributes at most 2.4e-7 relative
(2e-6 dB), the f32 rounding of the result at most 7.6e-6 dB at 100 dB, the f64 sums nothing visible.  The non-finite pattern must
match exactly; the maximum must equal numpy's bit for bit.  Every case also checks mean_amp <= mean_power <= max per column.

Every manager holds the same tracks (mixed rates and lengths), under one of four settings:
  mel    48 kHz default (Mel, n_fft 2048, hop 480): track 1 is 0.5 s, T = 51, H = the Mel count (no multiple of 4 or 64)
  lin    the same, linear: H = 1025; track 1 is stereo with different channels
  tall   win_ms 10: the 8 kHz track 2 has n_fft 128, H 65, hop 20, 3 s: T = 1201 (many slices)
  wide   win_ms 1000: the 48 kHz track 3 has n_fft 65536, H 32769, 2 s: T = 9; a batch of it exceeds the readers' pinned staging
Track 4 has 100 samples (T = 1).  Track 9 is 75 s at 8 kHz: under `tall` T = 30001, H = 65, which the kernel cuts into slices of
192 frames with 32 frames side by side, so every thread adds 6 frames per slice: the unrolled four-loads body once and the tail loop
twice (under `lin`, T = 7501, H = 257: the body once, the tail once).  cut() restates the kernel's cut so that the tests can say
which path a case takes."""
import ctypes as C
import functools
import itertools
import math
import threading

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi
from tests.synth import synth_track

pytestmark = pytest.mark.gpu

INF = float("inf")
KINDS = (ta.SPECTRUM_MEAN_AMP, ta.SPECTRUM_MEAN_POWER, ta.SPECTRUM_MAX)
SETTINGS = {"mel": (40.0, 4, 1, ta.MEL), "lin": (40.0, 4, 1, ta.LINEAR), "tall": (10.0, 4, 1, ta.LINEAR),
            "wide": (1000.0, 4, 1, ta.LINEAR)}


def _audio(seed, sr, n, channels=1):
    x = np.stack([synth_track(seed + c, sr, n) for c in range(channels)])
    return (x * (0.5 / np.abs(x).max())).astype(np.float32)


def _tracks():
    t = {1: (48000, _audio(1, 48000, 24000, 2)), 2: (8000, _audio(3, 8000, 24000)), 3: (48000, _audio(4, 48000, 96000)),
         4: (48000, _audio(5, 48000, 100))}
    gap = _audio(6, 48000, 48000)
    gap[0, 16800:31200] = 0.0  # 0.3 s of exact zeros: frames whose whole window lies inside are -inf rows
    t[5] = (48000, gap)
    half = _audio(7, 48000, 24000, 2)
    half[1] = 0.0  # an all-zero channel
    t[6] = (48000, half)
    bad = _audio(9, 48000, 48000)
    bad[0, 24000] = np.nan  # one NaN sample: the frames whose window holds it are NaN
    t[7] = (48000, bad)
    k = 100  # a sine on the centre of bin k of n_fft 2048
    t[8] = (48000, (0.25 * np.sin(2 * np.pi * k * np.arange(48000) / 2048.0)).astype(np.float32)[None])
    t[9] = (8000, _audio(11, 8000, 600000))  # long: several frames per thread and slice
    return t


TRACKS = _tracks()
CHANNELS = [(i, c) for i, (_, x) in sorted(TRACKS.items()) for c in range(x.shape[0])]


@pytest.fixture(scope="module")
def ctx():
    c = ta.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def managers(ctx):
    """setting name -> TrackManager holding TRACKS (made on first use)"""
    made = {}

    def get(name):
        if name not in made:
            tm = ta.TrackManager(ctx)
            tm.set_setting(*SETTINGS[name])
            tm.add_tracks([(i, sr, x) for i, (sr, x) in sorted(TRACKS.items())])
            made[name] = tm
        return made[name]

    yield get
    for tm in made.values():
        tm.close()


@functools.lru_cache(maxsize=None)
def _hop(name, sr):
    return ta.calc_framing_params(*SETTINGS[name][:3], sr)[0]


_SPECS = {}


def spec_of(managers, name, tid, ch):
    """the rows th_tm_copy_spec returns, read once per (setting, id, ch) and left unchanged"""
    key = (name, tid, ch)
    if key not in _SPECS:
        s = managers(name).spec(tid, ch)
        s.setflags(write=False)
        _SPECS[key] = s
    return _SPECS[key]


def frames_of(sr, hop, T, a, b):
    f0 = min(T, math.ceil(a * sr / hop))
    return f0, (T if b == INF else max(f0, min(T, math.ceil(b * sr / hop))))


def cut(H, n):
    """spectrum_shape (kernels_spectrum.hip) restated: (frames side by side in a block, slice length, slices) of an H-column,
    n-frame job; a thread adds slice_len / rows frames of a full slice"""
    quads = (H + 3) // 4
    best, best_pad = 3, None
    for l in (6, 5, 4, 3):
        pad = -quads % (1 << l)
        if pad <= quads // 8:
            best = l
            break
        if best_pad is None or pad < best_pad:
            best, best_pad = l, pad
    ct = 1 << best
    rows, tiles = 256 // ct, -(-quads // ct)
    if n == 0:
        return rows, rows, 0
    wanted = -(-512 // tiles)
    slice_len = -(-(-(-n // wanted)) // rows) * rows
    return rows, slice_len, -(-n // slice_len)


def reference(spec, f0, f1, kind):
    H = spec.shape[1]
    if f1 == f0:
        return np.full(H, np.nan, np.float32 if kind == ta.SPECTRUM_MAX else np.float64)
    if kind == ta.SPECTRUM_MAX:
        return np.max(spec[f0:f1], axis=0)
    rows = spec[f0:f1].astype(np.float64)
    c = 20.0 if kind == ta.SPECTRUM_MEAN_AMP else 10.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return c * np.log10(np.sum(10.0 ** (rows / c), axis=0) / (f1 - f0))


def same_nonfinite(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isinf(got), np.isinf(want))
    inf = np.isinf(want)
    assert np.array_equal(np.signbit(got[inf]), np.signbit(want[inf]))
    return np.isfinite(want)


def same_bits(got, want):
    """equal bit for bit, any NaN standing for any other (numpy does not say which payload its maximum returns)"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def mean_tol(want):
    return np.maximum(2e-5, 2.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))


def check_request(managers, name, tid, ch, a, b, expect_frames=None):
    """all three kinds of one (channel, range) against the reference; returns {kind: row}"""
    tm, spec = managers(name), spec_of(managers, name, tid, ch)
    sr = TRACKS[tid][0]
    f0, f1 = frames_of(sr, _hop(name, sr), spec.shape[0], a, b)
    if expect_frames is not None:
        assert (f0, f1) == expect_frames
    rev = tm.revisions()[1]
    rows = {}
    for kind in KINDS:
        got, info = tm.spectrum(tid, ch, kind, a, b)
        assert got.dtype == np.float32 and got.shape == (spec.shape[1],)
        assert info == {"offset": 0, "height": spec.shape[1], "frame_start": f0, "frame_end": f1, "spectrogram_revision": rev}
        want = reference(spec, f0, f1, kind)
        if kind == ta.SPECTRUM_MAX:
            assert want.dtype == np.float32 and same_bits(got, want)
        else:
            fin = same_nonfinite(got, want)
            err = np.abs(got[fin].astype(np.float64) - want[fin])
            print(f"{name} {tid}_{ch} [{a}, {b}) kind {kind}: frames [{f0}, {f1}) max err {err.max() if err.size else 0.0:.3e} dB")
            assert np.all(err <= mean_tol(want[fin]))
        rows[kind] = got
    amp, pw, mx = (rows[k].astype(np.float64) for k in KINDS)
    ok = ~np.isnan(mx)
    assert np.array_equal(np.isnan(amp), np.isnan(mx)) and np.array_equal(np.isnan(pw), np.isnan(mx))
    with np.errstate(invalid="ignore"):  # (-inf - -inf where a column is silent)
        tol = np.where(np.isfinite(pw), mean_tol(np.where(np.isfinite(pw), pw, 0.0)), 0.0)
        assert np.all((amp[ok] <= pw[ok] + tol[ok]) & (pw[ok] <= mx[ok] + tol[ok]))
    return rows


# (setting, id, ch, hop, T): the shapes of the issue; the ranges are given in frames f and turned into seconds f hop / sr
SHAPES = {"mel_T51": ("mel", 1, 0, 480, 51), "lin_ch0": ("lin", 1, 0, 480, 51), "lin_ch1": ("lin", 1, 1, 480, 51),
          "tall": ("tall", 2, 0, 20, 1201), "wide": ("wide", 3, 0, 12000, 9), "T1": ("lin", 4, 0, 480, 1),
          "deep": ("tall", 9, 0, 20, 30001), "deep_lin": ("lin", 9, 0, 80, 7501)}


def ranges_for(T):
    """(name, first frame, end frame or inf) in (fractional) frames: the whole track; inside one slice; two ends inside different
    slices, neither on a slice boundary; one frame; empty; reaching past the end"""
    if T > 5000:  # (the long track: "across" and "past_end" leave ragged last slices of several frames per thread)
        return [("whole", 0, INF), ("one_slice", 100.5, 120.5), ("across", 37.5, T - 777.3), ("one_frame", 9.5, 10.5),
                ("empty", 10.1, 10.9), ("past_end", 0.2 * T + 3.5, 5 * T)]
    if T > 1000:
        return [("whole", 0, INF), ("one_slice", 100.5, 120.5), ("across", 37.5, 1110.2), ("one_frame", 9.5, 10.5),
                ("empty", 10.1, 10.9), ("past_end", 0.7 * T, 5 * T)]
    return [("whole", 0, INF), ("one_slice", 3.5, 7.5), ("across", 2.5, 15.7), ("one_frame", 9.5, 10.5), ("empty", 10.1, 10.9),
            ("past_end", 0.7 * T, 5 * T)]


def test_shapes_are_the_ones_described(managers):
    for key, (name, tid, ch, hop, T) in SHAPES.items():
        s = spec_of(managers, name, tid, ch)
        assert s.shape[0] == T and _hop(name, TRACKS[tid][0]) == hop, (key, s.shape)
    assert spec_of(managers, "lin", 1, 0).shape[1] == 1025 and spec_of(managers, "tall", 2, 0).shape[1] == 65
    assert spec_of(managers, "wide", 3, 0).shape[1] == 32769
    h = spec_of(managers, "mel", 1, 0).shape[1]
    assert h % 4 != 0 and h % 64 != 0, h
    assert not np.array_equal(spec_of(managers, "lin", 1, 0), spec_of(managers, "lin", 1, 1))


@pytest.mark.parametrize("rng", range(6))
@pytest.mark.parametrize("shape", ["mel_T51", "lin_ch0", "lin_ch1", "tall", "deep", "deep_lin"])
def test_ranges_against_numpy(managers, shape, rng):
    name, tid, ch, hop, T = SHAPES[shape]
    rname, fa, fb = ranges_for(T)[rng]
    if shape.startswith("deep") and rname in ("whole", "across", "past_end"):
        # the accumulation loop proper: several frames per thread in a full slice — five or six (the unrolled four-loads body and
        # then the tail loop) for every such range of the 65-column spec and for the whole 257-column one, three or four (the tail
        # loop alone, or the body alone) otherwise — several slices, and a last slice that is shorter than the others and no
        # multiple of the rows side by side
        f0, f1 = frames_of(TRACKS[tid][0], hop, T, fa * hop / TRACKS[tid][0], fb * hop / TRACKS[tid][0])
        rows, slice_len, n_slices = cut(spec_of(managers, name, tid, ch).shape[1], f1 - f0)
        assert slice_len >= (5 if shape == "deep" or rname == "whole" else 3) * rows and n_slices > 8 and (f1 - f0) % slice_len % rows != 0, (rows, slice_len, n_slices)
    sr = TRACKS[tid][0]
    rows = check_request(managers, name, tid, ch, fa * hop / sr, fb * hop / sr)
    _, info = managers(name).spectrum(tid, ch, ta.SPECTRUM_MAX, fa * hop / sr, fb * hop / sr)
    n = info["frame_end"] - info["frame_start"]
    if rname == "empty":
        assert n == 0 and all(np.isnan(r).all() for r in rows.values())
    elif rname == "one_frame":
        assert (info["frame_start"], info["frame_end"]) == (10, 11)
    elif rname == "whole":
        assert (info["frame_start"], info["frame_end"]) == (0, T)
    elif rname == "past_end":
        assert info["frame_end"] == T and 0 < n < T
    else:
        assert 1 < n < T


@pytest.mark.parametrize("shape", ["wide", "T1"])
def test_wide_and_single_frame_specs(managers, shape):
    name, tid, ch, hop, T = SHAPES[shape]
    check_request(managers, name, tid, ch, 0.0, INF, expect_frames=(0, T))
    if T > 1:
        sr = TRACKS[tid][0]
        check_request(managers, name, tid, ch, 1.5 * hop / sr, 6.2 * hop / sr, expect_frames=(2, 7))


@pytest.mark.parametrize("name", ["mel", "lin"])
def test_silence_inside_a_finite_mean(managers, name):
    spec = spec_of(managers, name, 5, 0)
    silent = np.isneginf(spec).all(axis=1)
    assert silent.any() and not silent.all()
    rows = check_request(managers, name, 5, 0, 0.0, INF)
    assert all(np.isfinite(r).all() for r in rows.values())
    f = np.flatnonzero(silent)
    rows = check_request(managers, name, 5, 0, (f[0] - 0.5) * 480 / 48000, (f[-1] + 0.5) * 480 / 48000, expect_frames=(f[0], f[-1] + 1))
    assert all(np.isneginf(r).all() for r in rows.values())


@pytest.mark.parametrize("name", ["mel", "lin"])
def test_all_zero_channel_is_minus_infinity(managers, name):
    assert np.isneginf(spec_of(managers, name, 6, 1)).all()
    for a, b in ((0.0, INF), (0.1, 0.3)):
        rows = check_request(managers, name, 6, 1, a, b)
        assert all(np.isneginf(r).all() for r in rows.values())
    check_request(managers, name, 6, 0, 0.0, INF)


@pytest.mark.parametrize("name", ["mel", "lin"])
def test_one_nan_sample(managers, name):
    spec = spec_of(managers, name, 7, 0)
    hit = np.flatnonzero(np.isnan(spec).any(axis=1))
    assert hit.size and np.isnan(spec[hit]).all() and 0 < hit[0] and hit[-1] + 1 < spec.shape[0]
    sec = lambda f: (f - 0.5) * 480 / 48000  # noqa: E731  (the first frame at or after it is f)
    for a, b in ((0.0, INF), (sec(hit[0]), sec(hit[0] + 1)), (sec(hit[-1]), INF), (sec(2), sec(hit[0] + 1))):
        rows = check_request(managers, name, 7, 0, a, b)
        assert all(np.isnan(r).all() for r in rows.values())
    for a, b in ((0.0, sec(hit[0])), (sec(hit[-1] + 1), INF)):
        rows = check_request(managers, name, 7, 0, a, b)
        assert all(np.isfinite(r).all() for r in rows.values())


def test_sine_on_a_bin_centre_peaks_there(managers):
    tm = managers("lin")
    for kind in KINDS:
        row, info = tm.spectrum(8, 0, kind, 0.2, 0.8)
        assert (info["frame_start"], info["frame_end"]) == frames_of(48000, 480, 101, 0.2, 0.8) and row.shape == (1025,)
        assert info["frame_end"] - info["frame_start"] == 60
        assert int(np.argmax(row)) == 100


def every_request(name):
    """every channel x every range of its own frame count; range j of channel number c has kind (j + c) mod 3, so that every
    (range, kind) pair is in the batch"""
    reqs = []
    for c, (tid, ch) in enumerate(CHANNELS):
        sr = TRACKS[tid][0]
        hop = _hop(name, sr)
        T = ta.stft_n_frames(TRACKS[tid][1].shape[1], ta.calc_framing_params(*SETTINGS[name][:3], sr)[1], hop)
        for j, (_, fa, fb) in enumerate(ranges_for(T)):
            reqs.append((tid, ch, KINDS[(j + c) % 3], fa * hop / sr, fb * hop / sr))
    assert {(j % 6, r[2]) for j, r in enumerate(reqs)} == {(j, k) for j in range(6) for k in KINDS}
    return reqs


def packed(mgr, reqs):
    """th_*_get_spectra through the raw ABI into a sentinel-filled buffer a few floats longer than the result, which stay as they
    were -> (floats as bytes, infos as tuples)"""
    fn = getattr(_ffi.lib, mgr._PFX + "get_spectra")
    n = len(reqs)
    arr = (_ffi.SpectrumRequest * n)(*[_ffi.SpectrumRequest(*r) for r in reqs])
    info = (_ffi.SpectrumInfo * n)()
    need = C.c_size_t()
    assert fn(mgr.handle, arr, n, None, 0, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    out = np.full(need.value + 5, 12345.0, np.float32)
    _ffi.check(fn(mgr.handle, arr, n, out.ctypes.data_as(_ffi.c_f32p), out.size, info, C.byref(need)))
    assert need.value == out.size - 5 and (out[need.value:] == 12345.0).all()
    return out[: need.value], [tuple(getattr(o, k) for k, _ in o._fields_) for o in info]


@pytest.mark.parametrize("name", ["mel", "lin", "tall", "wide"])
def test_batch_equals_single_calls_bit_for_bit(managers, name):
    tm = managers(name)
    reqs = every_request(name)
    out, infos = packed(tm, reqs)
    at = 0
    for r, inf in zip(reqs, infos):
        assert inf[0] == at
        single, si = tm.spectrum(*r)
        assert si["height"] == inf[1] and (si["frame_start"], si["frame_end"]) == inf[2:4]
        assert np.array_equal(out[at: at + inf[1]].view(np.uint32), single.view(np.uint32)), r
        at += inf[1]
    assert at == out.size
    again, infos2 = packed(tm, reqs)
    assert np.array_equal(again.view(np.uint32), out.view(np.uint32)) and infos2 == infos
    rev, rinfos = packed(tm, reqs[::-1])
    for (r, inf), k in zip(zip(reqs, infos), range(len(reqs))):
        o2 = rinfos[len(reqs) - 1 - k][0]
        assert np.array_equal(rev[o2: o2 + inf[1]].view(np.uint32), out[inf[0]: inf[0] + inf[1]].view(np.uint32)), r
    if name == "wide":
        assert out.size * 4 > 520 * 520 * 4  # (this batch took the route for results above the readers' pinned staging)


def taking_turns(reqs, owner):
    """the same requests, the two slots' by turns while both have some left: every slot's rows go to places that are not adjacent"""
    mine = [[r for r in reqs if owner(r[0]) == s] for s in (0, 1)]
    return [r for pair in itertools.zip_longest(*mine) for r in pair if r is not None]


@pytest.mark.parametrize("name", ["lin", "tall", "wide"])
def test_multi_manager_returns_the_same_bytes_and_infos(managers, name):
    reqs = every_request(name)
    with ta.MultiTrackManager([0, 0]) as mg:
        mg.set_setting(*SETTINGS[name])
        mg.add_tracks([(i, sr, x) for i, (sr, x) in sorted(TRACKS.items())])
        assert len({mg.device_of(i) for i in TRACKS}) == 2
        if name == "wide":  # one slot's share alone is above the readers' pinned staging: copies out of its device result buffer
            reqs = taking_turns(reqs, mg.device_of)
            share = [sum(spec_of(managers, name, r[0], r[1]).shape[1] for r in reqs if mg.device_of(r[0]) == s) for s in (0, 1)]
            assert max(share) * 4 > 520 * 520 * 4
        owners = [mg.device_of(r[0]) for r in reqs]
        assert any(a != b for a, b in zip(owners, owners[1:]))
        want, winfos = packed(managers(name), reqs)  # (made by the same calls as the two-slot manager: the revisions agree too)
        got, ginfos = packed(mg, reqs)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and ginfos == winfos
        assert ginfos[0][4] == mg.revisions()[1]
        own = [r for r in reqs if mg.device_of(r[0]) == 0]  # a batch one slot owns whole
        g1, i1 = packed(mg, own)
        at = {(r, inf[1]): inf[0] for r, inf in zip(reqs, winfos)}
        for r, inf in zip(own, i1):
            o = at[(r, inf[1])]
            assert np.array_equal(g1[inf[0]: inf[0] + inf[1]].view(np.uint32), want[o: o + inf[1]].view(np.uint32))
        row, info = mg.spectrum(1, 1, ta.SPECTRUM_MEAN_POWER, 0.1, 0.3)
        ref, rinfo = managers(name).spectrum(1, 1, ta.SPECTRUM_MEAN_POWER, 0.1, 0.3)
        assert np.array_equal(row.view(np.uint32), ref.view(np.uint32))
        assert {k: v for k, v in info.items() if k != "spectrogram_revision"} == \
            {k: v for k, v in rinfo.items() if k != "spectrogram_revision"}
        with pytest.raises(ta.ThError) as e:
            mg.spectrum(99, 0, 0)
        assert e.value.code == _ffi.ERR_NOT_FOUND
        # the first faulty request in request order decides, whichever slots own the requests: one th_tm's codes
        for bad in ([(1, 0, 0), (2, 5, 0)], [(1, 5, 0), (99, 0, 0)], [(99, 0, 0), (1, 5, 0)], [(2, 0, 7), (99, 0, 0), (1, 5, 0)],
                    [(1, 0, 0, 0.2, 0.1), (99, 0, 0)]):
            codes = []
            for m in (managers(name), mg):
                with pytest.raises(ta.ThError) as e:
                    m.spectra(bad)
                codes.append(e.value.code)
            assert codes[0] == codes[1], (bad, codes)


def test_results_follow_the_manager(ctx):
    tm = ta.TrackManager(ctx)
    try:
        sr, x = TRACKS[1]
        tm.add_tracks([(1, sr, x), (3,) + TRACKS[3]])

        def check():
            spec = tm.spec(1, 1)
            f0, f1 = frames_of(sr, ta.calc_framing_params(*setting[:3], sr)[0], spec.shape[0], 0.05, 0.4)
            for kind in KINDS:
                got, info = tm.spectrum(1, 1, kind, 0.05, 0.4)
                assert (info["frame_start"], info["frame_end"], info["height"]) == (f0, f1, spec.shape[1])
                assert info["spectrogram_revision"] == tm.revisions()[1]
                want = reference(spec, f0, f1, kind)
                if kind == ta.SPECTRUM_MAX:
                    assert same_bits(got, want)
                else:
                    assert np.all(np.abs(got - want) <= mean_tol(want))
            return tm.spectrum(1, 1, ta.SPECTRUM_MEAN_AMP, 0.05, 0.4)[0]

        setting = SETTINGS["mel"]
        first = check()
        setting = SETTINGS["tall"]
        tm.set_setting(*setting)
        second = check()
        assert second.shape != first.shape
        rev = tm.revisions()[1]
        tm.set_dB_range(60.0)
        assert tm.revisions()[1] != rev
        assert np.array_equal(check(), second)  # (the rows are unclamped: the range moves the images, not the spectra)
        tm.set_common_normalize(ta.api.NORM_PEAK_DB, -6.0)
        third = check()
        assert not np.array_equal(third, second)
        tm.remove_track(1)
        with pytest.raises(ta.ThError) as e:
            tm.spectrum(1, 1, ta.SPECTRUM_MAX)
        assert e.value.code == _ffi.ERR_NOT_FOUND
        assert tm.spectrum(3, 0, ta.SPECTRUM_MAX)[0].shape == (tm.spec(3, 0).shape[1],)
    finally:
        tm.close()


def test_refusals_and_sizes(managers):
    tm = managers("lin")
    lib = _ffi.lib
    h1, h2 = spec_of(managers, "lin", 1, 0).shape[1], spec_of(managers, "lin", 2, 0).shape[1]
    out = np.full(h1 + h2, 777.0, np.float32)
    p = out.ctypes.data_as(_ffi.c_f32p)
    info = (_ffi.SpectrumInfo * 2)()
    need = C.c_size_t()

    def call(reqs, ptr=p, cap=out.size):
        arr = (_ffi.SpectrumRequest * len(reqs))(*[_ffi.SpectrumRequest(*r) for r in reqs])
        return lib.th_tm_get_spectra(tm.handle, arr, len(reqs), ptr, cap, info, C.byref(need))

    good = (1, 0, 0, 0.0, INF)
    nan = float("nan")
    for bad, code in [((99, 0, 0, 0.0, INF), _ffi.ERR_NOT_FOUND), ((1, 2, 0, 0.0, INF), _ffi.ERR_INVALID_ARG),
                      ((1, 0, 3, 0.0, INF), _ffi.ERR_INVALID_ARG), ((1, 0, 0, nan, INF), _ffi.ERR_INVALID_ARG),
                      ((1, 0, 0, -0.1, INF), _ffi.ERR_INVALID_ARG), ((1, 0, 0, INF, INF), _ffi.ERR_INVALID_ARG),
                      ((1, 0, 0, 0.0, nan), _ffi.ERR_INVALID_ARG), ((1, 0, 0, 0.2, 0.1), _ffi.ERR_INVALID_ARG)]:
        assert call([good, bad]) == code, bad
        assert call([bad]) == code, bad
        assert lib.th_tm_get_spectrum(tm.handle, bad[0], bad[1], bad[2], bad[3], bad[4], p, out.size, None) == code, bad
        assert (out == 777.0).all()  # on any error nothing is written
    assert lib.th_tm_get_spectrum(tm.handle, 1, 0, -1, 0.0, INF, p, out.size, None) == _ffi.ERR_INVALID_ARG
    reqs = [good, (2, 0, 2, 0.5, 1.0)]
    # the size query: out = NULL; infos and the length are filled
    assert call(reqs, None, 0) == _ffi.ERR_BUFFER_TOO_SMALL
    assert need.value == h1 + h2 and (info[0].offset, info[0].height, info[1].offset, info[1].height) == (0, h1, h1, h2)
    f0, f1 = frames_of(8000, _hop("lin", 8000), spec_of(managers, "lin", 2, 0).shape[0], 0.5, 1.0)
    assert (info[1].frame_start, info[1].frame_end) == (f0, f1) and f0 < f1
    assert info[1].spectrogram_revision == tm.revisions()[1]
    # one float short
    need.value = 0
    assert call(reqs, p, out.size - 1) == _ffi.ERR_BUFFER_TOO_SMALL and need.value == h1 + h2
    assert (out == 777.0).all()
    one = _ffi.SpectrumInfo()
    assert lib.th_tm_get_spectrum(tm.handle, 1, 0, 0, 0.0, INF, p, h1 - 1, C.byref(one)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert one.height == h1 and (out == 777.0).all()
    assert call(reqs) == _ffi.OK and need.value == h1 + h2 and not (out == 777.0).any()
    assert call([]) == _ffi.OK and need.value == 0
    assert tm.spectra([]) == []
    rows = tm.spectra([(1, 0, 0), (2, 0, 2, 0.5, 1.0)])
    assert np.array_equal(np.concatenate([r for r, _ in rows]).view(np.uint32), out.view(np.uint32))


def test_readers_run_beside_tile_readers(ctx, golden_dir):
    tm = ta.TrackManager(ctx)
    try:
        tm.set_colormap(open(f"{golden_dir}/colormap_inferno_rgba258.bin", "rb").read())
        tm.add_tracks([(i, TRACKS[i][0], TRACKS[i][1]) for i in (1, 2, 3)])
        tm.apply_track_list_changes()
        reqs = [(i, c, k, a, b) for (i, c) in ((1, 0), (1, 1), (2, 0), (3, 0)) for k in KINDS for (a, b) in ((0.0, INF), (0.1, 0.35))]
        want = [tm.spectrum(*r)[0] for r in reqs]
        tiles = {(i, c): tm.get_spectrogram_tile(i, c, 0, 0, 0, 0) for (i, c) in ((1, 0), (2, 0), (3, 0))}
        errors = []

        def spectra(k):
            try:
                for j in range(20):
                    r = (k * 7 + j) % len(reqs)
                    if j % 5 == 4:
                        rows = tm.spectra(reqs[r:] + reqs[:r])
                        got = rows[0][0]
                    else:
                        got = tm.spectrum(*reqs[r])[0]
                    assert np.array_equal(got.view(np.uint32), want[r].view(np.uint32)), reqs[r]
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        def tile_reader(k):
            try:
                for j in range(20):
                    key = list(tiles)[(k + j) % len(tiles)]
                    assert tm.get_spectrogram_tile(*key, 0, 0, 0, 0) == tiles[key]
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=spectra, args=(k,)) for k in range(4)]
        threads += [threading.Thread(target=tile_reader, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
    finally:
        tm.close()
