"""The host half of the export at a target sample rate (th_resample_plan_for, th_resample_n_out, th_resample_coefs, th_resample_f32)
against the contract restated in numpy f64 (tests/resample_ref.py).  CPU only.

The error bound of th_resample_f32 is derived, not measured: an f32 sum of 2K products, in any order, with or without fma, differs
from the exact sum by at most (2K + 4) 2^-24 sum |c x| (first order: at most 2K + 1 roundings of relative size 2^-24 act on any one
product; the + 4 covers the second-order terms for 2K <= 16384) plus one subnormal step.  A phase that is off by 1 / L exceeds it."""
import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi
from tests import resample_ref as R

PAIRS = [(44100, 48000), (48000, 44100), (48000, 96000), (96000, 48000), (8000, 48000), (48000, 16000), (8000, 8001)]
# (L, M, K): written out, not computed by either side
PLANS = {(44100, 48000): (160, 147, 128), (48000, 44100): (147, 160, 140), (48000, 96000): (2, 1, 128), (96000, 48000): (1, 2, 256),
         (8000, 48000): (6, 1, 128), (48000, 16000): (1, 3, 384), (8000, 8001): (8001, 8000, 128)}


@pytest.mark.parametrize("pair", PAIRS)
def test_plan_and_n_out(pair):
    p, want = ta.resample_plan(*pair), R.plan(*pair)
    assert (p["L"], p["M"], p["half_taps"]) == PLANS[pair] == (want["L"], want["M"], want["K"])
    assert p["rho"] == want["rho"] == min(1.0, p["L"] / p["M"]) and p["cutoff"] == want["cutoff"] == p["rho"] * 0.95
    for n_in in (0, 1, 2, 100, 3000, 44100, 10 ** 9 + 7):
        n = ta.resample_n_out(n_in, *pair)
        assert n == R.n_out(n_in, want) == (n_in * p["L"] + p["M"] - 1) // p["M"]
    assert 2 * p["half_taps"] <= ta.api.RESAMPLE_MAX_TAPS and p["L"] * 2 * p["half_taps"] <= ta.api.RESAMPLE_MAX_COEFS


def test_plan_limits_and_bad_rates():
    for pair in ((96000, 95999), (192000, 2000)):
        assert R.plan(*pair) == "unsupported"
        for fn in (lambda: ta.resample_plan(*pair), lambda: ta.resample_n_out(10, *pair), lambda: ta.resample_coefs(*pair, 0),
                   lambda: ta.resample_f32(np.zeros(4, np.float32), *pair, 0, 1)):
            with pytest.raises(ta.ThError) as e:
                fn()
            assert e.value.code == _ffi.ERR_UNSUPPORTED
    for pair in ((0, 48000), (48000, 0), (0, 0)):
        assert R.plan(*pair) == "invalid"
        with pytest.raises(ta.ThError) as e:
            ta.resample_plan(*pair)
        assert e.value.code == _ffi.ERR_INVALID_ARG
    # just inside: reduction by exactly 64, and the worst pair of standard rates
    assert ta.resample_plan(128000, 2000)["half_taps"] == 8192
    assert ta.resample_plan(11025, 192000)["L"] == 2560
    with pytest.raises(ta.ThError) as e:  # a phase the table does not have
        ta.resample_coefs(44100, 48000, 160)
    assert e.value.code == _ffi.ERR_INVALID_ARG
    with pytest.raises(ta.ThError) as e:  # outputs the track does not have
        ta.resample_f32(np.zeros(10, np.float32), 44100, 48000, 5, 7)
    assert e.value.code == _ffi.ERR_INVALID_ARG
    # j M beyond 64 bits
    with pytest.raises(ta.ThError) as e:
        ta.resample_n_out(2 ** 62, 8000, 8001)
    assert e.value.code == _ffi.ERR_UNSUPPORTED


@pytest.mark.parametrize("pair", PAIRS)
def test_coefficients(pair):
    p = R.plan(*pair)
    rows = sorted({0, 1, p["L"] // 2, p["L"] - 1} & set(range(p["L"])))
    for r in rows:
        h64, c32 = ta.resample_coefs(*pair, r)
        want = R.row(p, r)
        assert h64.shape == want.shape == (2 * p["K"],)
        assert np.abs(h64 - want).max() <= 1e-14, (pair, r)
        assert np.array_equal(c32.view(np.uint32), h64.astype(np.float32).view(np.uint32))  # the f64 row, rounded
        assert abs(h64.sum() - 1.0) <= 1e-11  # every phase has DC gain 1
    h64, _ = ta.resample_coefs(*pair, 0)
    assert abs(h64[p["K"] - 1] - p["cutoff"]) <= 1e-15  # t = 0: sinc(0) = 1, w(0) = 1


def test_filter_properties():
    """1000 -> 64000 Hz: the 64 rows interleaved are the prototype on a 64x grid.  Levels in dB relative to DC, frequencies relative
    to the lower rate's Nyquist (500 Hz)."""
    sr_in, sr_out = 1000, 64000
    p = R.plan(sr_in, sr_out)
    assert (p["L"], p["M"], p["K"]) == (64, 1, 128)
    rows = np.stack([ta.resample_coefs(sr_in, sr_out, r)[0] for r in range(64)])  # rows[r][k] = h(k - K + 1 - r / 64)
    # ascending t: for each k, r descends
    h = rows[::-1].T.reshape(-1)
    n_fft = 1 << 20
    H = np.abs(np.fft.rfft(h, n_fft)) / 64.0  # bin b = b * 64000 / n_fft Hz; / 64: the grid's density
    f = np.arange(H.size) * (sr_out / n_fft) / (sr_in / 2)  # in units of the Nyquist
    dB = 20.0 * np.log10(np.maximum(H / H[0], 1e-300))
    assert abs(H[0] - 1.0) <= 1e-11
    assert np.abs(dB[f <= 0.9]).max() <= 1e-4
    # exactly at 0.95 of the Nyquist (475 Hz; no bin lies there, and the edge is steep): the sum itself.  -6.02 to its two decimals
    t = np.arange(h.size) / 64.0  # input samples, up to a shift that the magnitude does not see
    at95 = abs(np.sum(h * np.exp(-2j * np.pi * (0.95 * 0.5) * t))) / 64.0 / H[0]
    assert abs(20.0 * np.log10(at95) + 6.02) <= 0.005
    assert dB[f >= 1.0].max() <= -119.0
    assert dB[f > 1.05].max() <= -180.0


def _noise(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def _check(x, pair, j0, n):
    p = R.plan(*pair)
    y = ta.resample_f32(x, *pair, j0, n)
    y64, mag = R.resample(x, *pair, j0, n)
    err, bnd = np.abs(y.astype(np.float64) - y64), R.bound(p, mag)
    assert y.dtype == np.float32 and y.shape == y64.shape
    assert np.all(err <= bnd), (pair, x.size, j0, float((err / bnd).max()))
    return y, y64, bnd


@pytest.mark.parametrize("pair", PAIRS)
def test_resample_f32_against_the_f64_restatement(pair):
    p = R.plan(*pair)
    x = _noise(3000, 1)
    no = R.n_out(3000, p)
    assert ta.resample_f32(x, *pair).size == no
    step = max(1, no // 1500)  # (at most ~1500 outputs per case through the per-output numpy sum: the head, the tail, a stride)
    _check(x, pair, 0, min(no, 400))
    _check(x, pair, no - min(no, 400), min(no, 400))
    mid = no // 3
    y_mid, _, _ = _check(x, pair, mid, min(300, no - mid))  # a range that starts and ends mid-track
    whole = ta.resample_f32(x, *pair)
    assert np.array_equal(whole[mid: mid + y_mid.size].view(np.uint32), y_mid.view(np.uint32))  # a range is a slice of the whole
    for j in range(0, no, step * 37):
        _check(x, pair, j, 1)
    # a track of 1 sample and one of 100 (shorter than the filter)
    for n_in in (1, 100):
        xs = _noise(n_in, 2 + n_in)
        y, _, _ = _check(xs, pair, 0, R.n_out(n_in, p))
        assert y.size == R.n_out(n_in, p) and np.any(y != 0)
    assert ta.resample_f32(np.zeros(0, np.float32), *pair).size == 0


def test_a_phase_off_by_one_exceeds_the_bound():
    """the bound is tight enough to tell phase r from r + 1 even at L = 8001: on noise, the wrong row is outside it for most outputs
    (this checks the yardstick, not the library: both sums are the restatement's)"""
    pair = (8000, 8001)
    p = R.plan(*pair)
    x = _noise(3000, 3)
    j0, n = 1500, 200
    y64, mag = R.resample(x, *pair, j0, n)
    L, M, K = p["L"], p["M"], p["K"]
    wrong = np.empty(n)
    for i in range(n):
        q, r = divmod((j0 + i) * M, L)
        c = R.row(p, (r + 1) % L).astype(np.float32).astype(np.float64)
        idx = q - K + 1 + np.arange(2 * K)
        ok = (idx >= 0) & (idx < x.size)
        wrong[i] = np.sum(c[ok] * x[idx[ok]].astype(np.float64))
    assert np.mean(np.abs(wrong - y64) > R.bound(p, mag)) > 0.5


@pytest.mark.parametrize("pair", PAIRS)
def test_sine_anchor(pair):
    """a 1 kHz sine, rounded to f32, comes out as the 1 kHz sine on the output grid (no delay) away from the ends"""
    sr_in, sr_out = pair
    p = R.plan(*pair)
    n_in = 2 * (p["K"] + 2) + 1200
    x = np.sin(2.0 * np.pi * 1000.0 * np.arange(n_in) / sr_in).astype(np.float32)
    no = R.n_out(n_in, p)
    j = np.arange(no)
    t_in = j * p["M"] / p["L"]  # the output's time in input samples
    inner = np.nonzero((t_in >= p["K"] + 2) & (t_in <= n_in - 1 - (p["K"] + 2)))[0]
    assert inner.size > 300
    j0, n = int(inner[0]), min(int(inner.size), 600)
    y, y64, bnd = _check(x, pair, j0, n)
    want = np.sin(2.0 * np.pi * 1000.0 * np.arange(j0, j0 + n) / sr_out)
    assert np.abs(y64 - want).max() <= 1e-7   # the restatement itself (<= 4e-8 from rounding the input to f32)
    assert np.all(np.abs(y - want) <= bnd + 1e-7)


def test_stopband_anchor():
    """96000 -> 48000: a tone at 1.1 x the output Nyquist (26.4 kHz) comes out below -119 dB of its amplitude in the interior"""
    pair = (96000, 48000)
    p = R.plan(*pair)
    n_in = 2 * (p["K"] + 2) + 1600
    x = np.sin(2.0 * np.pi * 26400.0 * np.arange(n_in) / 96000 + 0.3).astype(np.float32)
    j0 = (p["K"] + 2 + 1) // 2 + 1
    n = (n_in - 2 * (p["K"] + 2)) // 2 - 2
    y, y64, bnd = _check(x, pair, j0, n)
    floor = 10.0 ** (-119.0 / 20.0)
    assert np.abs(y64).max() <= floor
    assert np.all(np.abs(y) <= floor + bnd)
