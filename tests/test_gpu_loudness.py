"""th_audio_stats_dev and the TrackManager's per-track AudioStats (StatCalculator::calc, dynamics/stats.rs:56-86) against the
sequential restatement of tests/loudness_ref.py, the EBU Tech 3341 signals and the oracle's sum_squares / abs_max."""
import math

import numpy as np
import pytest
import torch

import thesia_amd as ta
from oracle import oracle as orc
from tests import loudness_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = ta.Context(0)
    yield c
    c.close()


def _run(ctx, tracks):
    """tracks: [(x (C, N) f32, sr)] -> (stats dicts, block energies per track)"""
    bufs, args, outs = [], [], []
    for x, sr in tracks:
        chans = [ctx.to_device(np.ascontiguousarray(c)) if c.size else ctx.alloc(16) for c in x]
        bufs += chans
        nb = ref.n_blocks(x.shape[1], sr)
        o = ctx.alloc(max(nb, 1) * 8)
        outs.append((o, nb))
        args.append(([b.ptr for b in chans], x.shape[1], sr, o.ptr))
    stats = ctx.audio_stats_dev(args)
    energies = [o.download((max(nb, 1),), np.float64)[:nb] for o, nb in outs]
    for b in bufs + [o for o, _ in outs]:
        b.free()
    return stats, energies


def _rms_peak(x):
    ss = np.float32(0)
    for c in x:
        ss = np.float32(ss + np.float32(orc.sum_squares(c)))
    ms = np.float32(ss / np.float32(x.size)) if x.size else np.float32("nan")
    pk = np.float32(max([orc.abs_max(c) for c in x] + [0.0]))
    with np.errstate(divide="ignore", invalid="ignore"):  # (f32 results of the exact logarithms)
        return (float(np.float32(10 * np.log10(np.float64(ms)))), float(pk), float(np.float32(20 * np.log10(np.float64(pk)))))


def _check_track(x, sr, st, e, what):
    # Against the restatement in extended precision.  The sequential f64 filter's own rounding exceeds 1e-10 of a block energy on
    # DC-heavy audio at 96 and 192 kHz (loudness_ref.kfilter); where it does, the bar is twice that rounding (the kernels run the same
    # f64 recurrence in their lanes).  The f64 restatement itself must agree within 5e-9.
    want_e = ref.block_energies(x, sr, np.longdouble)
    want64 = ref.block_energies(x, sr)
    fin64 = np.isfinite(want64)
    assert np.array_equal(fin64, np.isfinite(want_e)), what
    noise = (np.abs(want64[fin64] - want_e[fin64]) / want_e[fin64]).max() if fin64.any() else 0.0
    bar = max(1e-10, 2 * noise)
    assert not fin64.any() or (np.abs(e[fin64] - want64[fin64]) / want64[fin64]).max() <= 5e-9, what
    assert e.shape == want_e.shape, what
    nan = np.isnan(want_e)
    assert np.array_equal(np.isnan(e), nan), what
    fin = ~nan
    rel = np.abs(e[fin] - want_e[fin]) / np.maximum(np.abs(want_e[fin]), 1e-300)
    assert rel.size == 0 or rel.max() <= bar, (what, rel.max(), noise)
    # the same histogram bin for every block, and none within 1e-9 of a boundary
    near = [k for k in np.flatnonzero(fin) if np.min(np.abs(ref.BOUNDARIES - want_e[k]) / ref.BOUNDARIES) <= 1e-9]
    assert not near, (what, near)
    for k in np.flatnonzero(fin & (want_e >= ref.BOUNDARIES[0])):
        assert ref.hist_index(e[k]) == ref.hist_index(want_e[k]), (what, k)
    want_lufs = ref.gated_loudness(want_e)
    if math.isinf(want_lufs):
        assert st["global_lufs"] == want_lufs, what
    else:
        assert abs(st["global_lufs"] - want_lufs) <= 1e-9, (what, st["global_lufs"], want_lufs)
    rms, pk, pk_db = _rms_peak(x)
    if math.isnan(rms):
        assert math.isnan(st["rms_dB"]), what
    elif math.isinf(rms):
        assert st["rms_dB"] == rms, what
    else:
        assert abs(st["rms_dB"] - rms) <= 1e-5, (what, st["rms_dB"], rms)
    assert st["max_peak"] == pk, what
    if math.isinf(pk_db):
        assert st["max_peak_dB"] == pk_db
    else:
        assert abs(np.float32(st["max_peak_dB"]) - np.float32(pk_db)) <= np.spacing(np.float32(abs(pk_db))), (what, st["max_peak_dB"], pk_db)


def _signal(rng, C, n, kind):
    if kind == "noise":
        return rng.uniform(-0.5, 0.5, (C, n)).astype(np.float32)
    if kind == "dc":
        return (0.4 + 0.3 * rng.uniform(-1, 1, (C, n))).astype(np.float32)
    if kind == "clipped":
        return np.clip(rng.normal(0, 1.5, (C, n)), -1, 1).astype(np.float32)
    if kind == "nan":
        x = rng.uniform(-0.5, 0.5, (C, n)).astype(np.float32)
        x[0, n // 2] = np.nan
        return x
    raise ValueError(kind)


def test_block_energies_match_restatement_ragged_batch(ctx):
    """one call over ragged tracks: C = 1 .. 8, rates 8 k .. 192 k, lengths at the block edges, DC, clipped noise, a NaN sample"""
    rng = np.random.default_rng(5)
    specs = []  # (C, sr, n, kind)
    for sr in (8000, 11025, 16000, 44100, 48000, 96000, 192000):
        s, L = ref.s100(sr), 4 * ref.s100(sr)
        specs += [(1, sr, L - 1, "noise"), (2, sr, L, "dc"), (3, sr, L + s - 1, "clipped"), (4, sr, L + s, "noise")]
    specs += [(5, 48000, 3 * 48000 + 7, "dc"), (6, 44100, 2 * 44100, "clipped"), (7, 16000, 3 * 16000, "noise"),
              (8, 11025, 2 * 11025 + 3, "dc"), (2, 48000, 2 * 48000, "nan"), (1, 192000, 192000 + 5, "dc"), (1, 22050, 0, "noise")]
    tracks = [(_signal(rng, C, n, kind), sr) for C, sr, n, kind in specs]
    stats, energies = _run(ctx, tracks)
    for (C, sr, n, kind), (x, _), st, e in zip(specs, tracks, stats, energies):
        _check_track(x, sr, st, e, (C, sr, n, kind))
    assert math.isnan(stats[-1]["rms_dB"]) and stats[-1]["max_peak_dB"] == -math.inf and stats[-1]["global_lufs"] == -math.inf


def _sine(db, seconds, sr=48000):
    t = np.arange(int(round(seconds * sr))) / sr
    return (10.0 ** (db / 20.0) * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)


def test_ebu_tech_3341_signals(ctx):
    """Tech 3341 cases 1-5 and the 5.0 case; a sixth channel at index 3 (unused in the default map) changes nothing"""
    seq = lambda parts: np.concatenate([_sine(db, s) for db, s in parts])  # noqa: E731
    cases = {
        "stereo -23": (np.stack([_sine(-23, 20)] * 2), -22.95, True),
        "stereo -33": (np.stack([_sine(-33, 20)] * 2), -32.95, True),
        "-36/-23/-36": (np.stack([seq([(-36, 10), (-23, 60), (-36, 10)])] * 2), -22.971, False),
        "-72/-36/-23/-36/-72": (np.stack([seq([(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)])] * 2), -22.971, False),
        "-26/-20/-26": (np.stack([seq([(-26, 20), (-20, 20.1), (-26, 20)])] * 2), -22.936, False),
        "5.0": (np.stack([_sine(-28, 20), _sine(-28, 20), _sine(-24, 20), _sine(-30, 20), _sine(-30, 20)]), -23.05, True),
    }
    five = cases["5.0"][0]
    six = np.stack([five[0], five[1], five[2], _sine(-3, 20), five[3], five[4]])
    cases["5.0 as 6 ch"] = (six, -23.05, True)
    names = list(cases)
    stats, _ = _run(ctx, [(cases[k][0], 48000) for k in names])
    for k, st in zip(names, stats):
        x, want, steady = cases[k]
        target = -33.0 if k == "stereo -33" else -23.0
        assert abs(st["global_lufs"] - target) <= 0.1, (k, st)
        assert abs(st["global_lufs"] - want) <= (1e-9 if steady else 5e-4), (k, st["global_lufs"], want)
    assert stats[names.index("5.0 as 6 ch")]["global_lufs"] == stats[names.index("5.0")]["global_lufs"]


def test_long_track_late_window(ctx):
    """20 min at 48 kHz (offsets past 2^25): a late window of blocks against the restatement started one second earlier"""
    sr, n = 48000, 20 * 60 * 48000
    rng = np.random.default_rng(9)
    x = (0.1 + rng.uniform(-0.4, 0.4, n)).astype(np.float32)[None]
    _, (e,) = _run(ctx, [(x, sr)])
    s = ref.s100(sr)
    k0 = ref.n_blocks(n, sr) - 20
    start = k0 * s - sr  # zero state one second before the window
    y = ref.kfilter(x[:, start:k0 * s + 23 * s], sr)[:, sr:]
    want = ref.block_energies_of(y, sr)[:20]
    rel = np.abs(e[k0:k0 + 20] - want) / want
    assert k0 * s > 2 ** 25 and rel.max() <= 1e-10, rel.max()


def _same_stats(a, b):
    return all((math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k] for k in a)


def _tm_tracks(rng, big=False):
    out = [(1, 48000, _signal(rng, 2, 3 * 48000 + 11, "noise")), (2, 44100, _signal(rng, 1, 2 * 44100, "dc")),
           (3, 96000, _signal(rng, 6, 96000 + 5, "clipped")), (4, 3_000_000, _signal(rng, 1, 600_000, "noise"))]
    if big:  # several 96 MB groups
        out += [(10 + i, 48000, _signal(rng, 2, 150 * 48000, "noise")) for i in range(3)]
    return out


def _add(tm, tracks):
    tm.add_tracks([(i, sr, x) for i, sr, x in tracks])


def test_track_manager_audio_stats(ctx):
    rng = np.random.default_rng(21)
    tracks = _tm_tracks(rng, big=True)
    tm = ta.TrackManager(ctx)
    _add(tm, tracks)
    ok = [t for t in tracks if ref.MIN_SR <= t[1] <= ref.MAX_SR]
    direct, _ = _run(ctx, [(t[2], t[1]) for t in ok])
    for t, want in zip(ok, direct):
        assert _same_stats(tm.audio_stats(t[0]), want), t[0]
    bad = tm.audio_stats(4)  # a rate the crate refuses: the sums still count
    assert math.isnan(bad["global_lufs"]) and bad["max_peak"] == float(np.abs(tracks[3][2]).max())
    # not resident
    with pytest.raises(ta.ThError) as e:
        tm.audio_stats(99)
    assert e.value.code == -7
    # set_setting leaves the stats; a failed add leaves every earlier stat; re-add replaces; remove drops
    before = {t[0]: tm.audio_stats(t[0]) for t in tracks}
    tm.set_setting(20.0, 2, 1, ta.LINEAR)
    with pytest.raises(ta.ThError):
        tm.add_tracks([(1, 48000, np.zeros(100, np.float32)), (5, 48000, np.zeros(0, np.float32))])
    for t in tracks:
        assert _same_stats(tm.audio_stats(t[0]), before[t[0]]), t[0]
    y = _signal(rng, 1, 48000 * 2, "clipped")
    tm.add_tracks([(1, 48000, y)])
    ctx_stats, _ = _run(ctx, [(y, 48000)])
    assert _same_stats(tm.audio_stats(1), ctx_stats[0])
    tm.remove_track(2)
    with pytest.raises(ta.ThError):
        tm.audio_stats(2)
    tm.close()


@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]])
def test_multi_track_manager_audio_stats(ctx, devices):
    rng = np.random.default_rng(22)
    tracks = _tm_tracks(rng)
    one = ta.TrackManager(ctx)
    _add(one, tracks)
    g = ta.MultiTrackManager(devices)
    _add(g, tracks)
    for t in tracks:
        assert _same_stats(g.audio_stats(t[0]), one.audio_stats(t[0])), (devices, t[0])
    with pytest.raises(ta.ThError) as e:
        g.audio_stats(77)
    assert e.value.code == -7
    g.close()
    one.close()


def test_audio_stats_dev_on_caller_stream():
    """on a non-blocking side stream: the producer's copy is delayed, the block energies are read behind the call on the stream"""
    dev = "cuda:0"
    S = torch.cuda.Stream(dev)
    c = ta.Context(0, S.cuda_stream)
    rng = np.random.default_rng(3)
    x = _signal(rng, 2, 2 * 48000 + 17, "dc")
    nb = ref.n_blocks(x.shape[1], 48000)
    src = torch.from_numpy(x).to(dev)
    buf = torch.full_like(src, float("nan"))
    be = torch.full((nb,), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(1 << 26)
        buf.copy_(src)
        st = c.audio_stats_dev([([buf[0].data_ptr(), buf[1].data_ptr()], x.shape[1], 48000, be.data_ptr())])
        got = be.clone()
        be.fill_(-1.0)
    torch.cuda.synchronize()
    want = ref.block_energies(x, 48000)
    assert np.abs(got.cpu().numpy() - want).max() / want.max() <= 1e-10
    assert abs(st[0]["global_lufs"] - ref.gated_loudness(want)) <= 1e-9
    c.close()
