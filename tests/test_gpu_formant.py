"""Formant candidates on the GPU (th_tm_get_formants and the th_tmg twin).

Reference: th_formants_f64, the host function that runs the kernel's own source, applied to the samples th_tm_copy_audio returns.  The
contract is bit identity, for both kinds of output: every comparison here is of bits (tests/test_formant_host.py checks that host
function against the numpy restatement and against independent formulations)."""
import ctypes as C

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
GAUSS, RECT = ta.FORMANT_WIN_GAUSS, ta.FORMANT_WIN_RECT
PIECE_FRAMES = 16384   # TH_FORMANT_PIECE_FRAMES


def _signal(seed, n, sr):
    """a pulse-train vowel plus seeded noise (an LPC fit of a few resonances, never silent)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    x = 0.02 * rng.standard_normal(n)
    for k, fr in enumerate((300.0 + 37 * seed, 1150.0, 2450.0, 3300.0)):
        x += 0.2 / (k + 1) * np.sin(2 * np.pi * fr * t + seed) * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t))
    return x.astype(np.float32)


def _sec(sample, sr):
    """a time whose product with sr rounds up to exactly `sample`"""
    t = sample / sr
    while np.ceil(t * float(sr)) > sample:
        t = float(np.nextafter(t, 0.0))
    assert np.ceil(t * float(sr)) == sample
    return t


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# the shapes: name -> (sr, sr_analysis, n samples, p, W, H, window, preemph_hz).  W = p + 2, 63, 64, 65, 129, 550, 4096; H = 1, 7, W,
# 2 W; lengths 1, W - 1, W, W + 1 (a workgroup is one frame, so its span is the window) and a few hundred frames; both windows;
# alpha = 0 and alpha > 0; 8 kHz native and two resampled rates; the 4096-sample window on a handful of frames
SHAPES = {
    "p2_w4_h1_300_frames": (8000, 0, 300, 2, 4, 1, GAUSS, 50.0),
    "one_sample": (8000, 0, 1, 2, 4, 7, RECT, INF),
    "w63_len_w_minus_1": (8000, 0, 62, 10, 63, 7, GAUSS, 50.0),
    "w63_len_w_h_w": (8000, 0, 63, 10, 63, 63, RECT, 50.0),
    "w63_len_w_plus_1_h_2w": (8000, 0, 64, 10, 63, 126, GAUSS, INF),
    "p16_w64_h7": (8000, 0, 900, 16, 64, 7, GAUSS, 50.0),
    "p16_w65_h_w_rect": (8000, 0, 900, 16, 65, 65, RECT, INF),
    "p32_w129_h7_286_frames": (8000, 0, 2000, 32, 129, 7, GAUSS, 50.0),
    "p32_w34_h_2w": (8000, 0, 3000, 32, 34, 68, GAUSS, 50.0),
    "p10_w4096_h_w": (8000, 0, 9000, 10, 4096, 4096, GAUSS, 50.0),
    "p32_w4096_h_2w_rect": (8000, 0, 4097, 32, 4096, 8192, RECT, INF),
    "defaults_44100": (44100, 11000, 22050, 10, 550, 138, GAUSS, 50.0),
    "h1_48000_1100_frames": (48000, 11000, 4800, 10, 550, 1, GAUSS, 50.0),
    "p16_w129_h_2w_48000": (48000, 11000, 24000, 16, 129, 258, RECT, INF),
    "p2_w63_h_w_44100": (44100, 11000, 5000, 2, 63, 63, RECT, 50.0),
}
IDS = {name: i for i, name in enumerate(SHAPES)}
TRACKS = [(IDS[name], s[0], np.stack([_signal(IDS[name], s[2], s[0]), _signal(100 + IDS[name], s[2], s[0])])) for name, s in SHAPES.items()]


def request(name, ch=0, which=0, start_sec=0.0, end_sec=INF, kind=ta.FORMANT_OUT_FORMANTS):
    sr, sr_a, n, p, W, H, window, pre = SHAPES[name]
    rate = sr_a or sr
    return ta.formant_request(IDS[name], ch, which, start_sec, end_sec, sr_analysis=sr_a, n_poles=p, win_sec=W / rate, step_sec=H / rate,
                              preemph_hz=pre, window=window, kind=kind)


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


def want_whole(m, name, ch, kind):
    """the host's whole-track answer for a shape, computed once and never written to"""
    key = (name, ch, kind)
    if key not in _WANT:
        x = m.audio(IDS[name], ch, 0)
        assert np.array_equal(x, TRACKS[IDS[name]][2][ch])
        out, counts = ta.formants_f64(x, SHAPES[name][0], request(name, ch, kind=kind))
        out.setflags(write=False)
        _WANT[key] = (out, counts)
    return _WANT[key]


@pytest.mark.parametrize("kind", [ta.FORMANT_OUT_FORMANTS, ta.FORMANT_OUT_LPC], ids=["formants", "lpc"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_bit_identical_to_the_host(tm, name, kind):
    sr, sr_a, n, p, W, H, window, pre = SHAPES[name]
    want, counts = want_whole(tm, name, 1, kind)
    plan = ta.formant_plan(sr, n, request(name, 1, kind=kind))
    assert (plan["win"], plan["hop"], plan["n_poles"]) == (W, H, p)
    got, info = tm.get_formant_track(IDS[name], 1, 0, sr_analysis=sr_a, n_poles=p, win_sec=W / (sr_a or sr), step_sec=H / (sr_a or sr),
                                     preemph_hz=pre, window=window, kind=kind)
    assert got.shape == want.shape == (plan["n_frames_total"], 2 + p)
    assert (info["frame_first"], info["frame_end"], info["sr_analysis"], info["win"], info["hop"]) == (0, plan["n_frames_total"], sr_a or sr, W, H)
    assert info["length"] == got.size and info["waveform_revision"] == tm.revisions()[0]
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    print(f"{name}: {got.shape[0]} frames, {bad.size} differ, invalid {info['n_invalid']}, unconverged {info['n_unconverged']}")
    assert bad.size == 0, (name, bad[:5], got[bad[:1]], want[bad[:1]])
    assert (info["n_invalid"], info["n_unconverged"]) == counts
    if n >= W:   # a real signal: every frame fits
        assert counts == (0, 0) and not np.isnan(got[:, :2]).any()


@pytest.mark.parametrize("name", ["defaults_44100", "p16_w64_h7"])
def test_a_range_is_a_slice_of_the_whole_track(tm, name):
    sr, sr_a, n, p, W, H, window, pre = SHAPES[name]
    rate = sr_a or sr
    whole, _ = want_whole(tm, name, 0, ta.FORMANT_OUT_FORMANTS)
    total = whole.shape[0]
    reqs, spans = [], []
    for s0 in (0, 1, H - 1, H, H + 1, 9 * H - 1, 9 * H, 9 * H + 1):
        for s1 in (s0, 11 * H - 1, 11 * H, 11 * H + 1, None):
            if s1 is not None and s1 < s0:
                continue
            reqs.append(request(name, 0, 0, _sec(s0, rate), INF if s1 is None else _sec(s1, rate)))
            spans.append((-(-s0 // H), total if s1 is None else -(-s1 // H)))
    outs, infos = tm.get_formants(reqs)
    for (f0, f1), got, info in zip(spans, outs, infos):
        assert (info["frame_first"], info["frame_end"]) == (f0, f1) and got.shape[0] == f1 - f0
        assert np.array_equal(bits(got), bits(whole[f0:f1])), (f0, f1)
    assert any(f0 == f1 for f0, f1 in spans)   # an empty range is valid


def _mixed_batch():
    return [request("defaults_44100", 0), request("p16_w64_h7", 1, kind=ta.FORMANT_OUT_LPC), request("h1_48000_1100_frames", 0, end_sec=0.01),
            request("p32_w129_h7_286_frames", 0), request("one_sample", 1), request("p2_w63_h_w_44100", 0, kind=ta.FORMANT_OUT_LPC),
            request("p16_w129_h_2w_48000", 1), request("p10_w4096_h_w", 0), request("defaults_44100", 1, start_sec=0.1, end_sec=0.3)]


def _singles(m, reqs):
    return [m.get_formants([r])[0][0] for r in reqs]


def test_mixed_batch_equals_single_calls_with_canaries(tm):
    reqs = _mixed_batch()
    single = _singles(tm, reqs)
    need = sum(s.size for s in single)
    buf = np.full(need + 16, -77.25)
    outs, infos = tm.get_formants(reqs, out=buf[8:8 + need])
    assert (buf[:8] == -77.25).all() and (buf[8 + need:] == -77.25).all()
    at = 0
    for got, s, info in zip(outs, single, infos):
        assert info["offset"] == at and info["length"] == s.size    # back to back: nothing between two records
        assert np.array_equal(bits(got), bits(s))
        at += s.size
    assert not (buf[8:8 + need] == -77.25).any()
    rev = list(reversed(reqs))
    for got, s in zip(tm.get_formants(rev)[0], reversed(single)):
        assert np.array_equal(bits(got), bits(s))


def test_size_query_and_short_buffers(tm):
    reqs = [request("p16_w64_h7", 0), request("one_sample", 0)]
    arr = (_ffi.FormantRequest * 2)(*reqs)
    info, need = (_ffi.FormantInfo * 2)(), C.c_size_t()
    assert api.lib.th_tm_get_formants(tm.handle, arr, 2, None, 0, info, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    n0 = ta.formant_plan(8000, 900, reqs[0])["n_frames_total"] * 18
    assert need.value == n0 + 4 and (info[0].offset, info[0].length, info[1].offset, info[1].length) == (0, n0, n0, 4)
    buf = np.full(need.value, -3.5)
    assert api.lib.th_tm_get_formants(tm.handle, arr, 2, buf.ctypes.data_as(C.POINTER(C.c_double)), need.value - 1, info,
                                      C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert (buf == -3.5).all() and need.value == n0 + 4
    one = _ffi.FormantInfo()
    assert api.lib.th_tm_get_formant_track(tm.handle, C.byref(reqs[0]), None, 0, C.byref(one)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert one.length == n0
    assert tm.get_formants([]) == ([], [])


def test_which_and_revisions_under_a_set_normalisation(ctx):
    m = ta.TrackManager(ctx)
    try:
        sr, n = 44100, 9000
        m.add_tracks([(5, sr, np.stack([_signal(3, n, sr), _signal(4, n, sr)]))])
        m.apply_track_list_changes()
        rev0 = m.revisions()[0]
        assert m.get_formant_track(5, 0, 2)[1]["waveform_revision"] == rev0
        m.set_common_normalize(api.NORM_PEAK_DB, -9.0)
        rev1 = m.revisions()[0]
        assert rev1 != rev0
        outs = []
        for which in (0, 1, 2):
            x = m.audio(5, 1, which)
            want, counts = ta.formants_f64(x, sr, ta.formant_request(5, 1, which))
            got, info = m.get_formant_track(5, 1, which)
            assert info["waveform_revision"] == rev1 and (info["n_invalid"], info["n_unconverged"]) == counts
            assert np.array_equal(bits(got), bits(want)), which
            outs.append(got)
        assert not np.array_equal(m.audio(5, 1, 0), m.audio(5, 1, 2))
        lpc0 = m.get_formant_track(5, 1, 0, kind=ta.FORMANT_OUT_LPC)[0]
        lpc2 = m.get_formant_track(5, 1, 2, kind=ta.FORMANT_OUT_LPC)[0]
        assert not np.array_equal(lpc0[:, 0], lpc2[:, 0])    # the gain moves r0'
    finally:
        m.close()


def test_invalid_frames_one_nan_and_an_all_zero_channel(ctx):
    m = ta.TrackManager(ctx)
    try:
        sr, n = 8000, 1500
        x = _signal(8, n, sr)
        x[700] = NAN
        m.add_tracks([(9, sr, np.stack([x, np.zeros(n, np.float32)]))])
        m.apply_track_list_changes()
        kw = dict(sr_analysis=0, n_poles=6, win_sec=65 / sr, step_sec=20 / sr)
        for kind in (ta.FORMANT_OUT_FORMANTS, ta.FORMANT_OUT_LPC):
            for ch in (0, 1):
                want, counts = ta.formants_f64(m.audio(9, ch, 0), sr, ta.formant_request(9, ch, 0, kind=kind, **kw))
                got, info = m.get_formant_track(9, ch, 0, kind=kind, **kw)
                assert np.array_equal(bits(got), bits(want)) and (info["n_invalid"], info["n_unconverged"]) == counts
                if ch == 1:
                    assert np.isnan(got).all() and counts == (got.shape[0], 0)
                else:   # exactly the frames whose window meets sample 700 or 701
                    touched = [any(f * 20 - 32 <= s < f * 20 - 32 + 65 for s in (700, 701)) for f in range(got.shape[0])]
                    assert np.array_equal(np.isnan(got).all(axis=1), touched) and counts == (sum(touched), 0) and sum(touched) in (3, 4)
    finally:
        m.close()


def test_errors_write_nothing(tm):
    good = dict(track_id=IDS["p16_w64_h7"], ch=0, sr_analysis=0, n_poles=16, win_sec=0.008, step_sec=0.001)
    cases = [(dict(good, track_id=99), _ffi.ERR_NOT_FOUND), (dict(good, ch=2), _ffi.ERR_INVALID_ARG), (dict(good, which=3), _ffi.ERR_INVALID_ARG),
             (dict(good, n_poles=15), _ffi.ERR_INVALID_ARG), (dict(good, n_poles=34), _ffi.ERR_INVALID_ARG), (dict(good, win_sec=0.002), _ffi.ERR_INVALID_ARG),
             (dict(good, win_sec=0.6), _ffi.ERR_INVALID_ARG), (dict(good, step_sec=9.0), _ffi.ERR_INVALID_ARG), (dict(good, step_sec=NAN), _ffi.ERR_INVALID_ARG),
             (dict(good, preemph_hz=-1.0), _ffi.ERR_INVALID_ARG), (dict(good, window=2), _ffi.ERR_INVALID_ARG), (dict(good, kind=2), _ffi.ERR_INVALID_ARG),
             (dict(good, start_sec=NAN), _ffi.ERR_INVALID_ARG), (dict(good, start_sec=1.0, end_sec=0.5), _ffi.ERR_INVALID_ARG),
             (dict(good, sr_analysis=100, win_sec=0.3), _ffi.ERR_UNSUPPORTED)]   # a reduction by 80: beyond the resampler's taps
    for bad, code in cases:
        buf = np.full(1 << 16, -9.5)
        with pytest.raises(ta.ThError) as ex:
            tm.get_formants([good, bad, good], out=buf)
        assert ex.value.code == code, (bad, ex.value.code, str(ex.value))
        assert (buf == -9.5).all(), bad
    with pytest.raises(ta.ThError) as ex:   # the first faulty request decides
        tm.get_formants([good, dict(good, n_poles=3), dict(good, track_id=99)], out=np.full(1 << 16, -9.5))
    assert ex.value.code == _ffi.ERR_INVALID_ARG


def test_a_request_just_over_two_pieces_run_twice(ctx):
    m = ta.TrackManager(ctx)
    try:
        sr, n = 8000, 2 * PIECE_FRAMES + 5     # H = 1: a frame per sample, two full pieces and five frames
        x = _signal(11, n, sr)
        m.add_tracks([(3, sr, x[None, :])])
        m.apply_track_list_changes()
        kw = dict(sr_analysis=0, n_poles=2, win_sec=4 / sr, step_sec=1 / sr)
        want, counts = ta.formants_f64(m.audio(3, 0, 0), sr, ta.formant_request(3, 0, 0, **kw))
        assert want.shape == (n, 4)
        other = ta.formant_request(3, 0, 0, kind=ta.FORMANT_OUT_LPC, end_sec=0.01, **kw)
        for _ in range(2):
            (got, lpc), (info, _) = m.get_formants([ta.formant_request(3, 0, 0, **kw), other])
            assert np.array_equal(bits(got), bits(want)) and (info["n_invalid"], info["n_unconverged"]) == counts
            assert lpc.shape == (80, 4) and not np.isnan(lpc).any()
    finally:
        m.close()


@pytest.mark.parametrize("devices", [(0,), (0, 0)], ids=["one_slot", "two_slots"])
def test_tmg_equals_tm(tm, devices):
    reqs = _mixed_batch()
    want, winfo = tm.get_formants(reqs)
    with ta.MultiTrackManager(list(devices)) as g:
        g.add_tracks(TRACKS)
        g.apply_track_list_changes()
        got, ginfo = g.get_formants(reqs)
        rev = g.revisions()[0]
        for a, b, wa, wb in zip(want, got, winfo, ginfo):
            assert np.array_equal(bits(a), bits(b))
            assert {k: v for k, v in wa.items() if k != "waveform_revision"} == {k: v for k, v in wb.items() if k != "waveform_revision"}
            assert wb["waveform_revision"] == rev
        one, info = g.get_formant_track(IDS["defaults_44100"], 0)
        assert np.array_equal(bits(one), bits(want[0])) and info["length"] == one.size
        with pytest.raises(ta.ThError) as ex:
            g.get_formants([reqs[0], ta.formant_request(99, 0)])
        assert ex.value.code == _ffi.ERR_NOT_FOUND
