"""set_common_normalize / set_common_guard_clipping on the TrackManager's resident audio (th_tm_* and th_tmg_*) against the
sequential restatement of tests/dynamics_ref.py.

Clip, ReduceGlobalLevel and a gain of 1 (or a gain that is not finite) are bit-identical to the restatement.  The limiter's gains
lie within tol(sr) = 4 * 2^-53 * (release_samples + 1) of the restatement's f64 gains: each release step rounds by at most 2^-54 and
the recurrence contracts by (1 - slew) per step, so two evaluations that round differently differ by at most 2^-53 (release_samples
+ 1); the box layers average and add nothing of that order; the factor 4 is margin.  Everything downstream of the audio (specs, dB
state, images, tiles, waveform tiles, AudioStats) is bit-identical to a fresh manager that is handed the copied-out audio."""
import math

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi
from tests import dynamics_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
MODES = (ref.GUARD_CLIP, ref.GUARD_REDUCE_GLOBAL_LEVEL, ref.GUARD_LIMITER)
# (peak +6 dB: every track that is not silent peaks at 2 — the one target under which the limiter runs on a track of ONE sample,
# whose rms is its peak and whose loudness is -inf)
TARGETS = ((ref.NORM_RMS_DB, -6.0), (ref.NORM_LUFS, -14.0), (ref.NORM_PEAK_DB, -1.0), (ref.NORM_PEAK_DB, 6.0))
CASES = [(k, t, m) for k, t in TARGETS for m in MODES]
CASE_IDS = ["%s%g-%s" % ({1: "lufs", 2: "rms", 3: "peak"}[k], t, ("clip", "global", "limiter")[m]) for k, t, m in CASES]
ZERO_ID, EXACT_ID, ABOVE_ID, QUIET_ID = 13, 11, 12, 8


def tol_of(sr):
    return 4.0 * 2.0 ** -53 * (ref.limiter_params(sr)["release_samples"] + 1.0)


@pytest.fixture(scope="module")
def ctx():
    c = ta.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cmap(golden_dir):
    return open(f"{golden_dir}/colormap_inferno_rgba258.bin", "rb").read()


def noise(seed, chans, n, amp=0.3, bursts=()):
    x = np.random.default_rng(seed).uniform(-amp, amp, (chans, n)).astype(F32)
    for k, (c, i) in enumerate(bursts):
        x[c, i] = F32(6 * amp) * (-1 if k & 1 else 1)
    return x


def _peak_pair(ctx):
    """Two 48 kHz mono tracks for the target RMS -6 dB: the peak of gain x is exactly 1.0 in the first, nextafter(1, 2) in the second
    (their one loud sample differs by an ulp).  The gain depends on the track's own rms, so the sample is found with the manager."""
    kind, target = TARGETS[0]
    x = noise(48, 1, 20000, amp=0.72)
    x[0, 777] = F32(0.9)
    tm = ta.TrackManager(ctx)
    try:
        for _ in range(4):
            tm.add_tracks([(1, 48000, x)])
            g = ta.normalize_gain(kind, target, tm.audio_stats(1))
            assert 1.05 < g < 1.35, g
            p = F32(1) / g
            while F32(g * np.nextafter(p, F32(2))) <= 1:  # the largest sample the gain takes to 1.0 or less
                p = np.nextafter(p, F32(2))
            while F32(g * p) > 1:
                p = np.nextafter(p, F32(0))
            if x[0, 777] == p:
                break
            x[0, 777] = p
        above = x.copy()
        above[0, 777] = np.nextafter(p, F32(2))
        tm.add_tracks([(1, 48000, x), (2, 48000, above)])
        ga, gb = (ta.normalize_gain(kind, target, tm.audio_stats(i)) for i in (1, 2))
        assert F32(ga * x[0, 777]) == 1 and np.abs(F32(ga) * x).max() == 1, "no sample with gain x == 1.0 found"
        assert F32(gb * above[0, 777]) == np.nextafter(F32(1), F32(2))
    finally:
        tm.close()
    return x, above


@pytest.fixture(scope="module")
def tracks(ctx):
    """id -> (sr, planar f32): one ragged batch"""
    t = {}
    for i, n in enumerate((1, 39, 40, 41, 160, 161)):  # 8 kHz: attack 40, hold 160
        t[1 + i] = (8000, noise(i, 1, n, bursts=[(0, n // 2)]))
    t[7] = (8000, noise(7, 1, 4801, bursts=[(0, 0), (0, 4800)]))  # the zero flush of the look-ahead
    # quiet (sigma 0.06 within +-0.3: about -21 LUFS) with three x6 bursts 2.5 s apart on alternating channels: LUFS -14 lifts it by a
    # gain > 1 that keeps everything but the bursts below 1, so the limiter's gain is exactly 1 again between them
    q = np.clip(np.random.default_rng(8).normal(0, 0.06, (2, 50000)), -0.3, 0.3).astype(F32)
    for k, (c, i) in enumerate([(0, 5000), (1, 25000), (0, 45000)]):
        q[c, i] = F32(1.8) * (-1 if k & 1 else 1)
    t[QUIET_ID] = (8000, q)
    t[9] = (44100, (np.random.default_rng(9).normal(0, 0.5, (1, 30011)) * 8).astype(F32))  # dense limiting, attack 221
    t[10] = (192000, noise(10, 3, 60000, bursts=[(1, 31000)]))
    t[EXACT_ID], t[ABOVE_ID] = [(48000, x) for x in _peak_pair(ctx)]
    t[ZERO_ID] = (8000, np.zeros((1, 3000), F32))
    return t


def _add(mgr, tracks, cmap):
    mgr.set_colormap(cmap)
    mgr.add_tracks([(i, sr, x) for i, (sr, x) in tracks.items()])
    mgr.apply_track_list_changes()


@pytest.fixture(scope="module")
def main(ctx, tracks, cmap):
    """The manager the cases run on and the AudioStats of the originals (read while it is Off)"""
    tm = ta.TrackManager(ctx)
    _add(tm, tracks, cmap)
    orig_stats = {i: tm.audio_stats(i) for i in tracks}
    yield tm, orig_stats
    tm.close()


_REF = {}


def reference(case, tracks, orig_stats):
    """id -> restatement of the track under the case, fed the library's own gain; computed once per case"""
    if case not in _REF:
        kind, target, mode = case
        _REF[case] = {i: ref.apply_gain(x, sr, ta.normalize_gain(kind, target, orig_stats[i]), mode) for i, (sr, x) in tracks.items()}
    return _REF[case]


def set_case(mgr, case):
    kind, target, mode = case
    if mgr.common_dynamics() != (kind, target, mode):
        mgr.set_common_normalize(kind, target)
        mgr.set_common_guard_clipping(mode)
    assert mgr.common_dynamics() == (kind, target, mode)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def full_gain(mgr, i, n):
    """the track's n f32 gains as the library holds them (the query gives [1.0] when none is below 1)"""
    q = mgr.limiter_gain(i)
    assert q is not None and q.size in (1, n)
    return q if q.size == n else np.ones(n, F32)


def check_track(mgr, i, sr, x, want, mode):
    """one track of `mgr` against its restatement `want`"""
    n_ch, n = x.shape
    dyn = mgr.track_dynamics(i)
    got = {w: np.stack([mgr.audio(i, c, w) for c in range(n_ch)]) for w in (0, 1, 2)}
    assert same_bits(got[2], x), (i, "original")
    assert dyn["guard_result"] == want["result"] and dyn["draws_before_clip"] == (want["result"] == ref.RESULT_BEFORE_CLIP), (i, dyn)
    assert bits(dyn["normalize_gain"]) == bits(want["gain"]) and bits(dyn["global_gain"]) == bits(want["global_gain"]), (i, dyn)
    assert mgr.render_metadata(i, 0, 1.0, False)["is_clipped"] == (want["result"] == ref.RESULT_BEFORE_CLIP)
    assert mgr.render_metadata(i, 0, 1.0, True)["is_clipped"] == 1
    gstats = mgr.guard_clip_stats(i)
    wstats = ref.select_guard_stats(want["guard_stats"], mode)
    assert len(gstats) == len(wstats), (i, gstats, wstats)
    if want["gain64"] is None:  # clip, global level, gain 1 / not finite, a limiter with nothing to do: bit for bit
        assert same_bits(got[0], want["audio"]), (i, "audio", np.abs(got[0] - want["audio"]).max())
        assert same_bits(got[1], want["drawn"]), (i, "drawn")
        assert [(bits(d), c) for d, c in gstats] == [(bits(d), c) for d, c in wstats], (i, gstats, wstats)
        q, wq = mgr.limiter_gain(i), ref.limiter_gain_query(want)
        assert (q is None) == (wq is None) and (q is None or same_bits(q, wq)), (i, q, wq)
        return None
    # the limiter ran
    tol, g = tol_of(sr), want["gain64"]
    lo, hi = np.minimum(g - tol, 1.0).astype(F32), np.minimum(g + tol, 1.0).astype(F32)
    glib = full_gain(mgr, i, n)
    assert np.all((lo <= glib) & (glib <= hi)), (i, "gain", np.abs(glib.astype(np.float64) - g).max())
    y = (want["gain"] * x).astype(np.float64)
    ya = np.clip(y * (g - tol)[None, :], -1.0, 1.0).astype(F32)
    yb = np.clip(y * (g + tol)[None, :], -1.0, 1.0).astype(F32)
    assert np.all((np.minimum(ya, yb) <= got[0]) & (got[0] <= np.maximum(ya, yb))), (i, "audio")
    assert same_bits(got[1], got[0]), (i, "drawn")
    (dB, cnt), = gstats
    assert int((hi != 1).sum()) <= cnt <= int((lo != 1).sum()), (i, cnt)
    assert ref.db_from_amp(lo.min()) <= dB <= ref.db_from_amp(hi.min()), (i, dB)
    assert cnt == int((glib != 1).sum()) and bits(dB) == bits(ref.db_from_amp(glib.min()))  # ... and are those of its own gains
    # the f64 gain each f32 gain stands for is not visible; what can be inferred: the distance of the f32 gains from the rounded reference
    return float(np.abs(glib.astype(np.float64) - g.astype(F32).astype(np.float64)).max())


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_track_against_the_restatement(main, tracks, case):
    tm, orig_stats = main
    set_case(tm, case)
    kind, target, mode = case
    want = reference(case, tracks, orig_stats)
    ran = []
    for i, (sr, x) in tracks.items():
        g_lib, g_ref = ta.normalize_gain(kind, target, orig_stats[i]), ref.normalize_gain(kind, target, orig_stats[i])
        assert (not np.isfinite(g_ref) and not np.isfinite(g_lib)) or abs(float(g_lib) - float(g_ref)) <= float(np.spacing(g_ref)), (i, g_lib, g_ref)
        dev = check_track(tm, i, sr, x, want[i], mode)
        if dev is not None:
            ran.append((i, dev))
    print("case", case, "limiter ran on", ran)
    # what each target is there for
    if (kind, mode) == (ref.NORM_RMS_DB, ref.GUARD_LIMITER):
        assert [i for i, _ in ran] == [i for i in tracks if i not in (1, ZERO_ID, EXACT_ID)], ran  # (one sample at -6 dB rms peaks at 0.5)
    if (kind, target, mode) == (ref.NORM_PEAK_DB, 6.0, ref.GUARD_LIMITER):
        assert [i for i, _ in ran] == [i for i in tracks if i != ZERO_ID], ran
    if kind == ref.NORM_LUFS:
        assert want[QUIET_ID]["gain"] > 1 and np.abs(want[QUIET_ID]["gain"] * tracks[QUIET_ID][1]).max() > 1  # the guard acts in every mode
        assert want[1]["gain"] == 1 and tm.track_dynamics(1)["guard_result"] == ref.RESULT_GLOBAL_GAIN  # shorter than a gating block: -inf LUFS
        if mode == ref.GUARD_LIMITER:  # only the bursts are limited: the gain is exactly 1 between them, so the count means something
            q, g = tm.limiter_gain(QUIET_ID), want[QUIET_ID]["gain"]
            assert 1 < g and g * F32(0.3) < 1 and q.size == 50000
            assert q[15000] == 1 and q[35000] == 1 and q[4990] < 1 and q[24990] < 1 and 0 < tm.guard_clip_stats(QUIET_ID)[0][1] < q.size // 2
    if (kind, target) == (ref.NORM_PEAK_DB, -1.0):  # the guard has nothing to do: 0 dB, empty stats
        for i in tracks:
            if i != ZERO_ID:
                assert all(ref.format_stats(s) == "" for s in tm.guard_clip_stats(i)), i
                assert mode != ref.GUARD_LIMITER or same_bits(tm.limiter_gain(i), np.ones(1, F32))
    z = tm.track_dynamics(ZERO_ID)  # a silent track: the gain is not finite, the audio is the original
    assert z["normalize_gain"] == 1 and z["guard_result"] == ref.RESULT_GLOBAL_GAIN and tm.limiter_gain(ZERO_ID) is None
    assert tm.guard_clip_stats(ZERO_ID) == [(0, 0)]


def test_peak_of_exactly_one_is_not_limited(main, tracks):
    tm, orig_stats = main
    set_case(tm, (ref.NORM_RMS_DB, -6.0, ref.GUARD_LIMITER))
    g = ta.normalize_gain(ref.NORM_RMS_DB, -6.0, orig_stats[EXACT_ID])
    x = tracks[EXACT_ID][1]
    assert np.abs(g * x).max() == 1 and same_bits(tm.audio(EXACT_ID, 0), (g * x)[0])  # untouched bit for bit
    assert same_bits(tm.limiter_gain(EXACT_ID), np.ones(1, F32)) and tm.guard_clip_stats(EXACT_ID) == [(0, 0)]
    assert tm.track_dynamics(EXACT_ID)["guard_result"] == ref.RESULT_GAIN_SEQUENCE
    above = tm.limiter_gain(ABOVE_ID)  # one ulp more: the limiter runs
    assert above.size == x.shape[1] and above.min() < 1 and tm.guard_clip_stats(ABOVE_ID)[0][1] > 0


def wave_levels(n):
    top = max(1, math.ceil(math.log2(max(n, 1))) + 1)
    return (0, 1, 2, top)


def downstream(mgr, tracks, which_wave=False):
    """what a host reads back that is made from the audio"""
    s = {"db": mgr.db_state()} if not which_wave else {}
    for i, (sr, x) in tracks.items():
        for c in range(x.shape[0]):
            if which_wave:
                for lv in wave_levels(x.shape[1]):
                    for t in (0, (x.shape[1] - 1) >> (lv + 10)):
                        s[("wave", i, c, lv, t)] = mgr.get_waveform_tile(i, c, lv, t)[8:]  # (behind the revision)
                continue
            s[("spec", i, c)] = mgr.spec(i, c)
            s[("img", i, c)] = mgr.img(i, c)
            s[("tile", i, c)] = mgr.get_spectrogram_tile(i, c, 0, 0, 0, 0)[8:]
            s[("lod", i, c)] = mgr.get_spectrogram_tile(i, c, 1, 1, 0, 0)[8:]
        if not which_wave:
            s[("stats", i)] = mgr.audio_stats(i)
    return s


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        elif isinstance(a[k], dict):
            assert {n: np.float64(v).tobytes() for n, v in a[k].items()} == {n: np.float64(v).tobytes() for n, v in b[k].items()}, (k, a[k], b[k])
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_downstream_equals_a_fresh_manager_fed_the_audio(ctx, main, tracks, cmap, case):
    tm, _ = main
    set_case(tm, case)
    for which in (0, 1):
        fed = {i: (sr, np.stack([tm.audio(i, c, which) for c in range(x.shape[0])])) for i, (sr, x) in tracks.items()}
        fresh = ta.TrackManager(ctx)
        try:
            _add(fresh, fed, cmap)
            assert fresh.common_dynamics() == (ref.NORM_OFF, 0.0, ref.GUARD_REDUCE_GLOBAL_LEVEL)
            assert_same(downstream(tm, tracks, which_wave=bool(which)), downstream(fresh, fed, which_wave=bool(which)))
        finally:
            fresh.close()


def test_new_tracks_are_normalised_with_the_common_settings(ctx, main, tracks, cmap):
    tm, _ = main
    for case in ((ref.NORM_RMS_DB, -6.0, ref.GUARD_LIMITER), (ref.NORM_RMS_DB, -6.0, ref.GUARD_CLIP)):
        set_case(tm, case)
        late = ta.TrackManager(ctx)
        try:
            late.set_colormap(cmap)
            set_case(late, case)  # no track yet
            late.add_tracks([(i, sr, x) for i, (sr, x) in tracks.items()])
            late.apply_track_list_changes()
            for i, (sr, x) in tracks.items():
                for w in (0, 1, 2):
                    assert all(same_bits(late.audio(i, c, w), tm.audio(i, c, w)) for c in range(x.shape[0])), (i, w)
                assert late.track_dynamics(i) == tm.track_dynamics(i) and late.guard_clip_stats(i) == tm.guard_clip_stats(i)
                a, b = late.limiter_gain(i), tm.limiter_gain(i)
                assert (a is None) == (b is None) and (a is None or same_bits(a, b))
            assert_same(downstream(late, tracks), downstream(tm, tracks))
            assert_same(downstream(late, tracks, True), downstream(tm, tracks, True))
        finally:
            late.close()


def full_state(mgr, tracks):
    s = downstream(mgr, tracks)
    s.update(downstream(mgr, tracks, True))
    for i, (sr, x) in tracks.items():
        s[("dyn", i)] = str(mgr.track_dynamics(i))
        s[("gstats", i)] = mgr.guard_clip_stats(i)
        s[("gain", i)] = mgr.limiter_gain(i)
        for c in range(x.shape[0]):
            for w in (0, 1, 2):
                s[("audio", i, c, w)] = mgr.audio(i, c, w)
    return s


def test_defaults_round_trip(ctx, tracks, cmap):
    tm = ta.TrackManager(ctx)
    try:
        _add(tm, tracks, cmap)
        assert tm.common_dynamics() == (ref.NORM_OFF, 0.0, ref.GUARD_REDUCE_GLOBAL_LEVEL)
        first, rev = full_state(tm, tracks), tm.revisions()
        for i, (sr, x) in tracks.items():
            assert same_bits(first[("audio", i, 0, 0)], x[0]) and first[("gain", i)] is None and first[("gstats", i)] == [(0, 0)]
        tm.set_common_normalize(ref.NORM_LUFS, -14.0)
        assert tm.revisions() == (rev[0] + 1, rev[1] + 1)
        assert not same_bits(tm.audio(QUIET_ID, 0), tracks[QUIET_ID][1][0])
        tm.set_common_normalize(ref.NORM_OFF, 0.0)
        assert tm.revisions() == (rev[0] + 2, rev[1] + 2)
        assert_same(first, full_state(tm, tracks))
        tm.set_common_guard_clipping(ref.GUARD_LIMITER)
        assert tm.common_dynamics() == (ref.NORM_OFF, 0.0, ref.GUARD_LIMITER)
        tm.set_common_guard_clipping(ref.GUARD_REDUCE_GLOBAL_LEVEL)
        assert tm.revisions() == (rev[0] + 4, rev[1] + 4)
        assert_same(first, full_state(tm, tracks))
    finally:
        tm.close()


def _limiter_refusal_after_staging(mgr, cmap):
    """A limiter refusal AFTER another track has staged its derived audio: track 1 (8 kHz) is derived first; track 2 runs at 99 Hz,
    where the limiter's attack would be 0 samples.  (40 ms at 99 Hz: hop 1, win 4, n_fft 4.)  Under a two-slot manager track 2's
    slot refuses while the other slot stages completely and is then discarded."""
    two = {1: (8000, noise(101, 1, 5000)), 2: (99, noise(102, 2, 300))}
    mgr.set_setting(40.0, 4, 1, ta.LINEAR)
    _add(mgr, two, cmap)
    mgr.set_common_normalize(ref.NORM_PEAK_DB, 6.0)  # every peak at 2: the limiter would have to run on both
    assert all(mgr.track_dynamics(i)["global_gain"] < 1 for i in two)
    before, dyn, rev = full_state(mgr, two), mgr.common_dynamics(), mgr.revisions()
    assert dyn == (ref.NORM_PEAK_DB, 6.0, ref.GUARD_REDUCE_GLOBAL_LEVEL)
    with pytest.raises(ta.ThError) as e:
        mgr.set_common_guard_clipping(ref.GUARD_LIMITER)
    assert e.value.code == _ffi.ERR_UNSUPPORTED
    assert mgr.common_dynamics() == dyn and mgr.revisions() == rev
    assert_same(before, full_state(mgr, two))
    mgr.set_common_guard_clipping(ref.GUARD_CLIP)  # later calls still work
    assert mgr.common_dynamics() == (ref.NORM_PEAK_DB, 6.0, ref.GUARD_CLIP) and mgr.revisions() == (rev[0] + 1, rev[1] + 1)
    for i, (sr, x) in two.items():
        assert mgr.track_dynamics(i)["guard_result"] == ref.RESULT_BEFORE_CLIP and np.abs(mgr.audio(i, 0)).max() == 1


def test_refusals_change_nothing(ctx, main, tracks, cmap):
    for mgr in (ta.TrackManager(ctx), ta.MultiTrackManager([0, 0])):
        try:
            _limiter_refusal_after_staging(mgr, cmap)
        finally:
            mgr.close()
    tm, _ = main
    set_case(tm, (ref.NORM_RMS_DB, -6.0, ref.GUARD_CLIP))
    before = (tm.common_dynamics(), tm.revisions(), tm.spec(QUIET_ID, 1), tm.audio(QUIET_ID, 1), tm.guard_clip_stats(QUIET_ID))
    for call in (lambda: tm.set_common_normalize(4, -6.0), lambda: tm.set_common_normalize(-1, -6.0),
                 lambda: tm.set_common_guard_clipping(3), lambda: tm.set_common_guard_clipping(-1)):
        with pytest.raises(ta.ThError) as e:
            call()
        assert e.value.code == _ffi.ERR_INVALID_ARG
    after = (tm.common_dynamics(), tm.revisions(), tm.spec(QUIET_ID, 1), tm.audio(QUIET_ID, 1), tm.guard_clip_stats(QUIET_ID))
    assert before[:2] == after[:2] and same_bits(before[2], after[2]) and same_bits(before[3], after[3]) and before[4] == after[4]
    for call in (lambda: tm.track_dynamics(99), lambda: tm.guard_clip_stats(99), lambda: tm.limiter_gain(99)):
        with pytest.raises(ta.ThError) as e:
            call()
        assert e.value.code == _ffi.ERR_NOT_FOUND
    out = np.empty(8, F32)
    assert _ffi.lib.th_tm_copy_audio(tm.handle, 99, 0, 0, out.ctypes.data_as(_ffi.c_f32p), 8) == _ffi.ERR_NOT_FOUND
    assert _ffi.lib.th_tm_copy_audio(tm.handle, QUIET_ID, 2, 0, out.ctypes.data_as(_ffi.c_f32p), 8) == _ffi.ERR_NOT_FOUND
    assert _ffi.lib.th_tm_copy_audio(tm.handle, QUIET_ID, 0, 3, out.ctypes.data_as(_ffi.c_f32p), 8) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tm_copy_audio(tm.handle, QUIET_ID, 0, 0, out.ctypes.data_as(_ffi.c_f32p), 8) == _ffi.ERR_BUFFER_TOO_SMALL


def test_nan_samples_do_not_fault(ctx, cmap):
    x = noise(3, 2, 5000, amp=0.8)
    x[0, 100:110] = np.nan
    x[1, 4999] = np.nan
    tm = ta.TrackManager(ctx)
    try:
        _add(tm, {1: (8000, x)}, cmap)
        assert np.isfinite(tm.audio_stats(1)["max_peak_dB"])  # abs_max ignores NaN: the peak target gives a finite gain
        tm.set_common_normalize(ref.NORM_PEAK_DB, 6.0)
        for mode in MODES:
            tm.set_common_guard_clipping(mode)
            assert tm.track_dynamics(1)["normalize_gain"] > 1.5 and tm.audio(1, 1).shape == (5000,)
    finally:
        tm.close()


@pytest.mark.parametrize("devices", [[0], [0, 0]], ids=["0", "0-0"])
def test_multi_manager_equals_one_manager(ctx, tracks, cmap, devices):
    one, multi = ta.TrackManager(ctx), ta.MultiTrackManager(devices)
    try:
        for m in (one, multi):
            _add(m, tracks, cmap)
            m.set_common_normalize(ref.NORM_RMS_DB, -6.0)
        for mode in MODES:
            for m in (one, multi):
                m.set_common_guard_clipping(mode)
            assert one.common_dynamics() == multi.common_dynamics() == (ref.NORM_RMS_DB, -6.0, mode)
            assert one.revisions() == multi.revisions()
            assert_same(full_state(one, tracks), full_state(multi, tracks))
        with pytest.raises(ta.ThError) as e:
            multi.set_common_guard_clipping(7)
        assert e.value.code == _ffi.ERR_INVALID_ARG and one.revisions() == multi.revisions()
        with pytest.raises(ta.ThError) as e:
            multi.track_dynamics(99)
        assert e.value.code == _ffi.ERR_NOT_FOUND
    finally:
        multi.close()
        one.close()
