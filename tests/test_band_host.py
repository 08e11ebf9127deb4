"""The host half of the band-limited export (th_band_plan_for, th_band_coefs, th_band_response, th_band_f32) against the contract
restated in numpy f64 (tests/band_ref.py).  CPU only.

The response bounds are those of the window, checked in f64 for exactly the six cases below (8.8e-6 dB of passband ripple, -119.89 dB
of stopband); the f32 row the library answers for has to stay inside them.  The error bound of th_band_f32 is the resampler's, derived
in tests/band_ref.py bound()."""
import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi
from tests import band_ref as B

INF = float("inf")
NAN = float("nan")
# (sr, trans_hz) -> K, written out: ceil(16 sr / (5 trans_hz))
PLANS = [(8000, 400.0, 64), (8000, 394.0, 65), (8000, 390.0, 66), (48000, 0.0, 2048), (48000, 4.6875, 32768)]
# (sr, K, f_lo, f_hi): the edges at least D = 16 sr / (5 K) from 0 and from sr / 2 and at least 2 D apart
RESPONSES = [(48000, 1024, 1000.0, 4000.0), (48000, 2048, 200.0, 8000.0), (8000, 64, 1000.0, 2500.0), (48000, 32768, 50.0, 100.0),
             (8000, 64, 0.0, 1500.0), (8000, 64, 1500.0, 4000.0)]


trans_for = B.trans_for


def test_python_constants_are_the_kernels():
    """api.BAND_TILE / BAND_TAP_BLOCK / BAND_* (tests/test_gpu_band.py takes its tile and tap-block boundary cases from them) against
    reader_plan.h and the public header"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    plan_h = open(os.path.join(root, "thesia_amd", "csrc", "reader_plan.h")).read()
    const = lambda name: int(re.search(r"constexpr uint32_t %s = (\d+);" % name, plan_h).group(1))  # noqa: E731
    assert re.search(r"constexpr uint32_t BAND_TILE = BAND_THREADS \* BAND_R;", plan_h)
    assert ta.api.BAND_TILE == const("BAND_THREADS") * const("BAND_R") and ta.api.BAND_TAP_BLOCK == const("BAND_TAP_BLOCK")
    pub_h = open(os.path.join(root, "include", "thesia_amd.h")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)u?\s" % name, pub_h).group(1))  # noqa: E731
    assert (ta.BAND_PASS, ta.BAND_STOP) == (define("TH_BAND_PASS"), define("TH_BAND_STOP")) == (B.PASS, B.STOP)
    assert ta.api.BAND_MAX_TAPS == define("TH_BAND_MAX_TAPS") == B.MAX_TAPS
    assert ta.api.BAND_DEFAULT_HALF_TAPS == define("TH_BAND_DEFAULT_HALF_TAPS") == B.DEFAULT_HALF_TAPS


def raises(code, fn):
    with pytest.raises(ta.ThError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))


@pytest.mark.parametrize("sr, trans, K", PLANS)
def test_plans(sr, trans, K):
    for mode in (ta.BAND_PASS, ta.BAND_STOP):
        p, want = ta.band_plan(sr, mode, 500.0, 1500.0, trans), B.plan(sr, mode, 500.0, 1500.0, trans)
        assert p["half_taps"] == K == want["K"] and p["mode"] == mode
        assert (p["f_lo_hz"], p["f_hi_hz"]) == (500.0, 1500.0)
        assert p["trans_hz"] == want["trans"] == (16.0 * sr) / (5.0 * K)
        assert 2 * K <= ta.api.BAND_MAX_TAPS
    assert (2 * K) % 4 == (2 if K == 65 else 0)


def test_plan_limits_and_arguments():
    assert B.plan(48000, B.PASS, 50.0, 100.0, 4.6) == "unsupported"
    raises(_ffi.ERR_UNSUPPORTED, lambda: ta.band_plan(48000, ta.BAND_PASS, 50.0, 100.0, 4.6))
    raises(_ffi.ERR_UNSUPPORTED, lambda: ta.band_plan(48000, ta.BAND_STOP, 50.0, 100.0, 1e-300))
    bad = [(8000, 0, NAN, 1000.0, 0.0), (8000, 0, 100.0, NAN, 0.0), (8000, 0, 100.0, 1000.0, NAN),  # a NaN
           (8000, 0, -1.0, 1000.0, 0.0),                                                            # f_lo < 0
           (8000, 0, 1000.0, 1000.0, 0.0), (8000, 0, 2000.0, 1000.0, 0.0),                          # f_lo >= f_hi
           (8000, 0, 4000.0, INF, 0.0), (8000, 0, 4500.0, 5000.0, 0.0),                             # ... after the clamp
           (8000, 2, 100.0, 1000.0, 0.0),                                                           # an unknown mode
           (8000, 0, 100.0, 1000.0, -1.0), (8000, 0, 100.0, 1000.0, 4000.5), (8000, 0, 100.0, 1000.0, INF),  # trans_hz
           (0, 0, 100.0, 1000.0, 0.0),                                                              # sr == 0
           (8000, 1, 0.0, 4000.0, 0.0), (8000, 1, 0.0, INF, 0.0), (8001, 1, 0.0, 4000.5, 400.0)]     # TH_BAND_STOP of the whole band
    for args in bad:
        assert B.plan(*args) == "invalid", args
        raises(_ffi.ERR_INVALID_ARG, lambda: ta.band_plan(*args))
    # f_hi = +inf and anything above sr / 2 clamp; trans_hz = sr / 2 is the widest
    for f_hi in (INF, 4000.0, 4000.5, 1e30):
        p = ta.band_plan(8000, ta.BAND_PASS, 1500.0, f_hi, 400.0)
        assert (p["half_taps"], p["f_lo_hz"], p["f_hi_hz"]) == (64, 1500.0, 4000.0)
    assert ta.band_plan(8001, ta.BAND_STOP, 100.0, INF, 0.0)["f_hi_hz"] == 4000.5
    assert ta.band_plan(8000, ta.BAND_PASS, 100.0, 1000.0, 4000.0)["half_taps"] == 7
    # the identity: no filter, whatever the width
    for trans in (0.0, 400.0, 1e-9):
        p = ta.band_plan(8000, ta.BAND_PASS, 0.0, INF, trans)
        assert (p["half_taps"], p["f_lo_hz"], p["f_hi_hz"], p["trans_hz"]) == (0, 0.0, 4000.0, 0.0) and B.plan(8000, B.PASS, 0.0, INF, trans)["K"] == 0
        raises(_ffi.ERR_INVALID_ARG, lambda: ta.band_coefs(8000, p))
        raises(_ffi.ERR_INVALID_ARG, lambda: ta.band_response(8000, p, [100.0]))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.band_f32(np.zeros(10, np.float32), np.zeros(8, np.float32), 5, 7))  # outputs the track does not have
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.band_f32(np.zeros(10, np.float32), np.zeros(0, np.float32)))


@pytest.mark.parametrize("sr, K, f_lo, f_hi", RESPONSES + [(8000, 65, 500.0, 3000.0), (8000, 66, 0.0, 3999.0)])
def test_rows(sr, K, f_lo, f_hi):
    trans = trans_for(sr, K)
    rows = {}
    for mode in (ta.BAND_PASS, ta.BAND_STOP):
        p, want = ta.band_plan(sr, mode, f_lo, f_hi, trans), B.plan(sr, mode, f_lo, f_hi, trans)
        assert p["half_taps"] == K == want["K"]
        h64, c32 = ta.band_coefs(sr, p)
        ref = B.row(sr, want)
        assert h64.shape == ref.shape == c32.shape == (2 * K,)
        assert np.abs(h64 - ref).max() <= 1e-14, mode
        assert np.array_equal(c32.view(np.uint32), h64.astype(np.float32).view(np.uint32))  # the f64 row, rounded
        assert h64[2 * K - 1] == 0.0 and c32[2 * K - 1] == 0.0                              # t = K: w(1) = 0; the tap is kept
        rows[mode] = h64
    delta = np.zeros(2 * K)
    delta[K - 1] = 1.0
    assert np.array_equal(rows[ta.BAND_PASS] + rows[ta.BAND_STOP], delta)  # exactly
    if f_hi == sr / 2:  # a == 1: the first term is the exact delta, so the row is delta - the low-pass at f_lo
        c = 2.0 * f_lo / sr
        t = np.arange(2 * K) - K + 1.0
        low = c * np.sinc(c * t) * B.window(t / K)
        assert np.abs(rows[ta.BAND_PASS] - (delta - low)).max() <= 1e-14
        assert rows[ta.BAND_PASS][K - 1] == 1.0 - c
        assert abs(rows[ta.BAND_PASS].sum()) <= 1e-9                   # a high-pass has no DC


@pytest.mark.parametrize("sr, K, f_lo, f_hi", RESPONSES)
def test_response(sr, K, f_lo, f_hi):
    nyq = sr / 2.0
    D = (16.0 * sr) / (5.0 * K)
    assert (f_lo == 0.0 or f_lo >= D) and (f_hi == nyq or f_hi <= nyq - D) and f_hi - f_lo >= 2 * D
    trans = trans_for(sr, K)
    p = ta.band_plan(sr, ta.BAND_PASS, f_lo, f_hi, trans)
    s = ta.band_plan(sr, ta.BAND_STOP, f_lo, f_hi, trans)
    assert p["half_taps"] == s["half_taps"] == K and p["trans_hz"] == D
    edges = [f for f in (f_lo, f_hi) if 0.0 < f < nyq]
    # the side lobes are sr / (2 K) = D / 6.4 wide: 8 points per lobe over the 4 D next to each transition, where ripple and lobes are
    # highest, and a sweep of 257 points over the whole of every interval the issue names
    near = lambda lo, hi: np.linspace(lo, hi, 257) if hi > lo else np.array([lo])  # noqa: E731
    inside = np.unique(np.concatenate([near(f_lo + D, min(f_hi - D, f_lo + 5 * D)), near(max(f_lo + D, f_hi - 5 * D), f_hi - D),
                                       np.linspace(f_lo + D, f_hi - D, 257)]))
    below = np.concatenate([near(max(0.0, f_lo - 5 * D), f_lo - D), np.linspace(0.0, f_lo - D, 257)]) if f_lo > 0.0 else np.empty(0)
    above = np.concatenate([near(f_hi + D, min(nyq, f_hi + 5 * D)), np.linspace(f_hi + D, nyq, 257)]) if f_hi < nyq else np.empty(0)
    NI = inside.size
    hz = np.concatenate([edges, inside, below, above])
    db = ta.band_response(sr, p, hz)
    # th_band_response is the f32 row's magnitude, summed in f64
    c32 = ta.band_coefs(sr, p)[1]
    some = slice(0, hz.size, 7)
    assert np.abs(db[some] - B.response_db(c32, sr, hz[some])).max() <= 1e-3
    ne = len(edges)
    print("edges", db[:ne], "ripple", np.abs(db[ne: ne + NI]).max(), "stopband", db[ne + NI:].max() if hz.size > ne + NI else None)
    assert np.all(np.abs(db[:ne] + 6.02) <= 0.01), db[:ne]
    assert np.abs(db[ne: ne + NI]).max() <= 1e-4
    assert np.all(db[ne + NI:] <= -119.0), db[ne + NI:].max()
    stop = ta.band_response(sr, s, np.concatenate([inside, edges]))
    print("stop mode inside", stop[:NI].max(), "edges", stop[NI:])
    assert np.all(stop[:NI] <= -119.0), stop[:NI].max()
    assert np.all(np.abs(stop[NI:] + 6.02) <= 0.01)  # (1 - H at an edge, where H is real and one half)


def _noise(seed, n, peak=0.9):
    return np.random.default_rng(seed).uniform(-peak, peak, n).astype(np.float32)


def _row(sr, K, mode, f_lo, f_hi):
    return ta.band_coefs(sr, ta.band_plan(sr, mode, f_lo, f_hi, trans_for(sr, K)))[1]


@pytest.mark.parametrize("K, mode, f_lo, f_hi", [(64, 0, 1000.0, 2500.0), (65, 1, 1000.0, 2500.0), (66, 0, 0.0, 1500.0), (256, 0, 1500.0, INF),
                                                 (7, 1, 0.0, 2000.0)])
def test_band_f32_is_the_sum_within_the_bound(K, mode, f_lo, f_hi):
    c32 = _row(8000, K, mode, f_lo, f_hi)
    for n in (1, 100, 2 * K - 1, 2 * K + 1, 1500):
        x = _noise(100 + n, n)
        y = ta.band_f32(x, c32)
        want, mag = B.filt(x, c32)
        assert y.shape == want.shape == (n,)
        err = np.abs(y.astype(np.float64) - want)
        assert np.all(err <= B.bound(K, mag)), (n, (err / B.bound(K, mag)).max())
        # mid-track ranges are slices, bit for bit
        for j0, m in ((0, 0), (0, 1), (n - 1, 1), (n // 2, n - n // 2), (n // 3, min(5, n - n // 3)), (n, 0)):
            assert np.array_equal(ta.band_f32(x, c32, j0, m).view(np.uint32), y[j0: j0 + m].view(np.uint32)), (n, j0, m)
    # an output that is off by one sample is outside the bound: the bound is not slack enough to hide a wrong index
    x = _noise(7, 1500)
    want, mag = B.filt(x, c32)
    y = ta.band_f32(x, c32)
    assert np.mean(np.abs(y[1:].astype(np.float64) - want[:-1]) > B.bound(K, mag[:-1])) > 0.9


def test_band_f32_summation_order():
    """tap k into partial sum k mod 4 by one fmaf, all four from +0, (a0 + a1) + (a2 + a3): restated with exact f64 products (an f32
    product is exact in f64, and rounding the f64 sum of an f32 and such a product to f32 is the fmaf unless the double rounding bites,
    which the comparison would show)"""
    import math
    K = 65
    c32 = _row(8000, K, 0, 1000.0, 2500.0)
    x = _noise(3, 400)
    y = ta.band_f32(x, c32)
    pad = np.concatenate([np.zeros(K - 1, np.float32), x, np.zeros(K, np.float32)])
    n_diff = 0
    for j in range(x.size):
        a = [np.float32(0.0)] * 4
        for k in range(2 * K):
            exact = math.fsum([float(a[k % 4]), float(c32[k]) * float(pad[j + k])])  # correctly rounded sum of two doubles
            a[k % 4] = np.float32(exact)
        n_diff += np.float32(np.float32(a[0] + a[1]) + np.float32(a[2] + a[3])).view(np.uint32) != y[j].view(np.uint32)
    assert n_diff == 0


def test_sines_and_delay():
    sr, K, n = 8000, 64, 4000
    t = np.arange(n) / sr
    x = (0.5 * np.sin(2 * np.pi * 1000.0 * t + 0.3)).astype(np.float32)
    mid = slice(K, n - K)
    # inside the band (the edges 400 Hz = D away at least): the same samples at the same indices, within the passband's 1e-4 dB
    y = ta.band_f32(x, _row(sr, K, ta.BAND_PASS, 500.0, 2000.0))
    tol = 0.5 * (10.0 ** (1e-4 / 20.0) - 1.0) + 0.5 * (2 * K + 4) * 2.0 ** -24
    print("in band: max |y - x|", np.abs(y[mid] - x[mid]).max(), "tol", tol)
    assert np.abs(y[mid] - x[mid]).max() <= tol
    assert np.abs(y[mid][1:] - x[mid][:-1]).max() > 0.1  # (a delay of one sample would show)
    # outside the band: below -119 dB of the input
    for mode, f_lo, f_hi in ((ta.BAND_PASS, 2000.0, 3000.0), (ta.BAND_STOP, 500.0, 2000.0), (ta.BAND_PASS, 1500.0, INF), (ta.BAND_PASS, 0.0, 500.0)):
        y = ta.band_f32(x, _row(sr, K, mode, f_lo, f_hi))
        db = 20.0 * np.log10(np.sqrt(np.mean(y[mid].astype(np.float64) ** 2)) / np.sqrt(np.mean(x[mid].astype(np.float64) ** 2)))
        print("out of band", mode, f_lo, f_hi, db)
        assert db <= -119.0, (mode, f_lo, f_hi, db)
    # stop + pass of the same band = the input (the rows add up to the delta), within the two roundings' bound
    yp, ys = ta.band_f32(x, _row(sr, K, ta.BAND_PASS, 500.0, 2000.0)), ta.band_f32(x, _row(sr, K, ta.BAND_STOP, 500.0, 2000.0))
    assert np.abs((yp.astype(np.float64) + ys) - x).max() <= 2 * (2 * K + 4) * 2.0 ** -24


@pytest.mark.parametrize("K", [64, 65])
def test_one_nan_makes_exactly_2k_outputs_nan(K):
    c32 = _row(8000, K, ta.BAND_PASS, 1000.0, 2500.0)
    assert c32[2 * K - 1] == 0.0
    x = _noise(5, 1000)
    clean = ta.band_f32(x, c32)
    for at in (0, 3, K - 1, K, 500, 999 - K, 999):
        bad = x.copy()
        bad[at] = np.nan
        y = ta.band_f32(bad, c32)
        j = np.arange(x.size)
        holds = (j >= at - K) & (j <= at + K - 1)  # the zero tap included
        assert holds.sum() == min(999, at + K - 1) - max(0, at - K) + 1
        assert np.all(np.isnan(y[holds])) and np.array_equal(y[~holds].view(np.uint32), clean[~holds].view(np.uint32)), at
