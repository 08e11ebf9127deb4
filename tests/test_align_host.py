"""The host side of the alignment reader (include/thesia_amd.h "Align two tracks"): th_align_plan_for's table and every argument rule,
th_xcorr_f64 / th_align_energy_f64 / th_align_peak / th_align_f64 bit for bit against the numpy restatement (tests/align_ref.py), a
derived error bound against math.fsum of the exact products, known answers, and the planner's pieces.  CPU only: the planner is reached
through tests/emu/emu_align_plan.cpp, compiled here with g++ beside align_plan.cpp and host_math.cpp (once; the library is kept under
tests/emu/_build and rebuilt when a source is newer)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api
from tests import align_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thesia_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "emu", "emu_align_plan.cpp"), os.path.join(CSRC, "align_plan.cpp"), os.path.join(CSRC, "host_math.cpp")]
DEPS = SRC + [os.path.join(CSRC, h) for h in ("align_plan.h", "align_core.h", "host_math.h", "stft_core.h")] + [os.path.join(ROOT, "include", "thesia_amd.h")]
LIB = os.path.join(ROOT, "tests", "emu", "_build", "libemu_align_plan.so")

INF, NAN = float("inf"), float("nan")
SR = 48000
SUMMARY, CURVE = ta.ALIGN_OUT_SUMMARY, ta.ALIGN_OUT_CURVE
# reference lengths: below, at and above the four partial sums, a block, a group, and two groups and a bit
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 131071, 131072, 131073, 2 * 131072 + 5]


def bits(a):
    """the doubles' bits; a NaN is a NaN (its sign and payload are the machine's, not the contract's)"""
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


def request(s0, s1, D, kind=SUMMARY, flags=0, sr=SR):
    return ta.align_request(start_sec=sec(s0, sr), end_sec=sec(s1, sr), max_lag_sec=D / sr, kind=kind, flags=flags)


# ------------------------------------------------------------------------------------------------ the plan and the argument rules
def test_plan_table():
    pl = ta.align_plan(SR, 100000, SR, 77, ta.align_request(start_sec=0.5, end_sec=1.0, max_lag_sec=0.01, kind=CURVE, flags=ta.ALIGN_ABS))
    assert pl == dict(sr=SR, max_lag=480, kind=CURVE, flags=1, sample_start=24000, sample_end=48000, n_lags=961, length=10 + 961)
    assert (pl["sample_start"], pl["sample_end"]) == ta.audio_sample_range(SR, 100000, 0.5, 1.0)
    # D = rint(max_lag_sec sr), ties to even; the whole track by default; a range past the end is clamped
    assert ta.align_plan(5, 100, 5, 100, ta.align_request(max_lag_sec=0.5))["max_lag"] == 2
    assert ta.align_plan(5, 100, 5, 100, ta.align_request(max_lag_sec=0.7))["max_lag"] == 4
    pl = ta.align_plan(SR, 1000, SR, 5, ta.align_request(max_lag_sec=0.0))
    assert (pl["sample_start"], pl["sample_end"], pl["max_lag"], pl["n_lags"], pl["length"]) == (0, 1000, 0, 1, 10)
    pl = ta.align_plan(SR, 1000, SR, 5, ta.align_request(start_sec=0.01, end_sec=9.0, max_lag_sec=1 / SR))
    assert (pl["sample_start"], pl["sample_end"], pl["n_lags"]) == (480, 1000, 3)
    # an empty range: no lags, the summary alone (also with the curve asked for)
    for kw in (dict(start_sec=0.01, end_sec=0.01), dict(start_sec=5.0)):
        pl = ta.align_plan(SR, 1000, SR, 1000, ta.align_request(max_lag_sec=0.1, kind=CURVE, **kw))
        assert pl["sample_start"] == pl["sample_end"] and (pl["n_lags"], pl["length"]) == (0, 10)
    # the limits themselves are served
    pl = ta.align_plan(SR, 1 << 22, SR, 9, ta.align_request(max_lag_sec=((1 << 17) - 1) / SR))
    assert pl["sample_end"] == 1 << 22 and pl["n_lags"] == (1 << 18) - 1
    assert ta.align_plan(SR, 1000, SR, 9, ta.align_request(max_lag_sec=(1 << 20) / SR))["max_lag"] == 1 << 20


@pytest.mark.parametrize("kw, code", [
    (dict(start_sec=NAN), _ffi.ERR_INVALID_ARG), (dict(end_sec=NAN), _ffi.ERR_INVALID_ARG), (dict(max_lag_sec=NAN), _ffi.ERR_INVALID_ARG),
    (dict(max_lag_sec=-1e-9), _ffi.ERR_INVALID_ARG), (dict(max_lag_sec=INF), _ffi.ERR_INVALID_ARG), (dict(start_sec=-0.1), _ffi.ERR_INVALID_ARG),
    (dict(start_sec=INF), _ffi.ERR_INVALID_ARG), (dict(start_sec=0.2, end_sec=0.1), _ffi.ERR_INVALID_ARG), (dict(kind=2), _ffi.ERR_INVALID_ARG),
    (dict(which=3), _ffi.ERR_INVALID_ARG), (dict(ref_which=3), _ffi.ERR_INVALID_ARG), (dict(flags=2), _ffi.ERR_INVALID_ARG),
    (dict(flags=3), _ffi.ERR_INVALID_ARG), (dict(sr=0), _ffi.ERR_INVALID_ARG), (dict(sr_ref=0), _ffi.ERR_INVALID_ARG),
    (dict(sr=44100), _ffi.ERR_UNSUPPORTED), (dict(sr=44100, start_sec=NAN), _ffi.ERR_INVALID_ARG), (dict(sr=44100, kind=7), _ffi.ERR_INVALID_ARG),
    (dict(n_ref=(1 << 22) + 1), _ffi.ERR_UNSUPPORTED), (dict(max_lag_sec=((1 << 20) + 1) / SR), _ffi.ERR_UNSUPPORTED),
    (dict(max_lag_sec=1e300), _ffi.ERR_UNSUPPORTED), (dict(n_ref=1 << 22, max_lag_sec=(1 << 17) / SR), _ffi.ERR_UNSUPPORTED)])
def test_argument_rules(kw, code):
    kw = dict(kw)
    sr_ref, sr, n_ref = kw.pop("sr_ref", SR), kw.pop("sr", SR), kw.pop("n_ref", 1000)
    with pytest.raises(ta.ThError) as ex:
        ta.align_plan(sr_ref, n_ref, sr, 1000, ta.align_request(**dict(dict(max_lag_sec=0.001), **kw)))
    assert ex.value.code == code, (kw, str(ex.value))
    if n_ref <= 4096:   # th_align_f64 refuses what the plan refuses, and writes nothing
        out, need = np.full(64, -5.5), C.c_size_t(77)
        x = noise(1, n_ref)
        req = ta.align_request(**dict(dict(max_lag_sec=0.001), **kw))
        f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
        rc = api.lib.th_align_f64(x.ctypes.data_as(f32p), x.size, sr_ref, x.ctypes.data_as(f32p), x.size, sr, C.byref(req), out.ctypes.data_as(f64p),
                                  out.size, C.byref(need))
        assert rc == code and (out == -5.5).all() and need.value == 0


def test_align_f64_size_query():
    x = noise(2, 500)
    req = request(0, 500, 4, CURVE)
    need = C.c_size_t()
    f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
    args = (x.ctypes.data_as(f32p), x.size, SR, x.ctypes.data_as(f32p), x.size, SR, C.byref(req))
    assert api.lib.th_align_f64(*args, None, 0, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL and need.value == 19
    out = np.full(32, -5.5)
    assert api.lib.th_align_f64(*args, out.ctypes.data_as(f64p), 18, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL and (out == -5.5).all()
    assert api.lib.th_align_f64(*args, out.ctypes.data_as(f64p), 19, C.byref(need)) == _ffi.OK and (out[19:] == -5.5).all()


# ------------------------------------------------------------------------------------------------ bit identity with the restatement
_CASES = {}


def case(N, D, probe_len=None, s0=3):
    """ref: s0 + N + 2 samples, the range [s0, s0 + N); the probe of its own length (default: the reference's)"""
    key = (N, D, probe_len, s0)
    if key not in _CASES:
        ref = noise(1000 + N, s0 + N + 2)
        probe = noise(2000 + N + D, ref.size if probe_len is None else probe_len)
        want = R.align(ref, probe, s0, s0 + N, D, CURVE)
        want.setflags(write=False)
        _CASES[key] = (ref, probe, want)
    return _CASES[key]


@pytest.mark.parametrize("N", SIZES)
def test_xcorr_and_align_bit_identical_to_the_restatement(N):
    D, s0 = (8 if N < 100000 else 3), 3
    ref, probe, want = case(N, D)    # the probe as long as the reference: the lags leave it at both ends
    r = ta.xcorr_f64(ref[s0:s0 + N], probe, s0 - D, 2 * D + 1)
    assert np.array_equal(bits(r), bits(want[10:]))
    assert bits(np.array([ta.align_energy_f64(ref, s0, N)]))[0] == bits(want[4:5])[0]
    got = ta.align_f64(ref, SR, probe, SR, request(s0, s0 + N, D, CURVE))
    assert got.size == 10 + 2 * D + 1 and np.array_equal(bits(got), bits(want)), (got[:10], want[:10])
    assert np.array_equal(bits(ta.align_f64(ref, SR, probe, SR, request(s0, s0 + N, D, SUMMARY))), bits(want[:10]))
    assert got[0] == 0.0 and -D <= got[1] <= D
    lag = int(got[1])
    assert got[5] == ta.align_energy_f64(probe, s0 + lag, N)


@pytest.mark.parametrize("probe_len, s0", [(1, 3), (400, 3), (1003, 0), (1500, 7), (5000, 501), (0, 3)],
                         ids=["one_sample", "shorter", "as_long", "longer", "much_longer_odd_s0", "empty"])
def test_n_1000_at_d_70_probes_shorter_and_longer(probe_len, s0):
    N, D = 1000, 70
    ref, probe, want = case(N, D, probe_len, s0)
    got = ta.align_f64(ref, SR, probe, SR, request(s0, s0 + N, D, CURVE))
    assert np.array_equal(bits(got), bits(want))
    if probe_len == 0:   # nothing to correlate with: every r is +0, the peak is the first lag, E_probe = 0
        assert (bits(got[10:]) == 0).all() and got[0] == 0.0 and got[1] == -D and got[5] == 0.0 and np.isnan(got[6]) and np.isnan(got[8])


def test_abs_flag_is_part_of_the_restatement():
    ref, probe, _ = case(1000, 70, 1500, 7)
    for flags in (0, ta.ALIGN_ABS):
        got = ta.align_f64(ref, SR, -probe, SR, request(7, 1007, 70, CURVE, flags))
        assert np.array_equal(bits(got), bits(R.align(ref, -probe, 7, 1007, 70, CURVE, flags)))


# ------------------------------------------------------------------------------------------------ the derived error bound
@pytest.mark.parametrize("N", [5, 4097, 131073, 2 * 131072 + 5])
def test_error_bound_against_fsum(N):
    """A term passes through at most d additions: 1024 in its partial sum, 2 in the block's value, 32 in its group, n_groups in r.
    Each rounds with relative error at most u = 2^-53, so |r - exact| <= ((1 + u)^d - 1) sum|a b| <= d u / (1 - d u) sum|a b|."""
    D, s0 = 2, 3
    ref, probe, want = case(N, 8 if N < 100000 else 3)
    u, d = 2.0 ** -53, 1024 + 2 + 32 + R.n_groups(N)
    r = ta.xcorr_f64(ref[s0:s0 + N], probe, s0 - D, 2 * D + 1)
    for i in range(2 * D + 1):
        terms = R.exact_terms(ref[s0:s0 + N], probe, s0 - D, i)
        exact, mass = math.fsum(terms), math.fsum(abs(t) for t in terms)
        bound = d * u * mass / (1.0 - d * u)
        print(f"N {N} lag {i - D}: |r - fsum| = {abs(r[i] - exact):.3e}, bound {bound:.3e}")
        assert abs(r[i] - exact) <= bound


# ------------------------------------------------------------------------------------------------ known answers
def delayed_copy(n, d, scale, seed=5):
    """probe[k + d] = scale ref[k] wherever the probe has that sample (scale a power of two: exact)"""
    ref = noise(seed, n)
    probe = np.zeros(n + abs(d) + 64, np.float32)
    j = np.arange(n) + d
    probe[j[j >= 0]] = ref[j >= 0] * np.float32(scale)
    return ref, probe


@pytest.mark.parametrize("d", [0, 1, 37, -37, 300])
def test_a_delayed_scaled_copy_nulls_exactly(d):
    ref, probe = delayed_copy(9000, d, 2.0 ** -3)
    s0, s1, D = 1001, 7001, 320          # the window [s0 + d, s1 + d) lies inside the probe
    got = ta.align_summary(ta.align_f64(ref, SR, probe, SR, request(s0, s1, D)))
    assert got["status"] == 0.0 and got["lag"] == d and got["polarity"] == 1.0
    assert got["gain"] == 0.125 and got["e_probe"] == got["e_ref"] / 64 and got["r"] == got["e_ref"] / 8
    assert got["null_dB"] == -INF and abs(got["rho"] - 1.0) <= 2.0 ** -52
    assert abs(got["delta"]) < 0.5


def test_an_inverted_copy_aligns_only_under_abs():
    ref, probe = delayed_copy(9000, 41, -(2.0 ** -3))
    plain = ta.align_summary(ta.align_f64(ref, SR, probe, SR, request(1001, 7001, 320)))
    assert plain["status"] == 0.0 and plain["lag"] != 41 and plain["null_dB"] > -3.0
    got = ta.align_summary(ta.align_f64(ref, SR, probe, SR, request(1001, 7001, 320, flags=ta.ALIGN_ABS)))
    assert got["lag"] == 41 and got["polarity"] == -1.0 and got["gain"] == -0.125 and got["null_dB"] == -INF
    assert abs(got["rho"] + 1.0) <= 2.0 ** -52 and got["r"] == -got["e_ref"] / 8


def test_a_plateau_returns_the_smallest_lag():
    ref, probe = np.ones(600, np.float32), np.ones(1000, np.float32)
    got = ta.align_f64(ref, SR, probe, SR, request(300, 400, 8, CURVE))
    assert (got[10:] == 100.0).all()
    s = ta.align_summary(got)
    assert s["status"] == 0.0 and s["lag"] == -8 and s["delta"] == 0.0 and s["gain"] == 1.0 and s["null_dB"] == -INF
    # ... and a peak of two equal neighbours inside the searched lags takes the first, with no vertex shift beyond half a lag
    pk = ta.align_peak([1.0, 3.0, 3.0, 1.0], 0, 1.0)
    assert (pk["status"], pk["peak"]) == (0, 1) and pk["delta"] == 0.5 * (1.0 - 3.0) / ((1.0 - 6.0) + 3.0)


def test_peak_rules():
    r = np.array([0.5, -4.0, 1.0, 2.0, 1.5])
    assert ta.align_peak(r, 0, 1.0) == dict(status=0, peak=3, delta=(0.5 * (1.0 - 1.5)) / ((1.0 - 4.0) + 1.5), polarity=1.0)
    pk = ta.align_peak(r, ta.ALIGN_ABS, 1.0)
    assert (pk["status"], pk["peak"], pk["polarity"]) == (0, 1, -1.0) and pk["delta"] == (0.5 * (0.5 - 1.0)) / ((0.5 - 8.0) + 1.0)
    assert ta.align_peak([1.0, 2.0, 3.0], 0, 1.0) == dict(status=0, peak=2, delta=0.0, polarity=1.0)    # an edge
    assert ta.align_peak([1.0, 2.0, 3.0], 0, 1.0)["peak"] == R.peak([1.0, 2.0, 3.0], 0, 1.0)[1]
    for bad_r, e in (([1.0, NAN, 2.0], 1.0), ([1.0, INF], 1.0), ([1.0, 2.0], 0.0), ([1.0, 2.0], -1.0), ([1.0, 2.0], NAN), ([1.0, 2.0], INF), ([], 1.0)):
        assert ta.align_peak(bad_r, 0, e)["status"] == 1
    with pytest.raises(ta.ThError):
        ta.align_peak(r, 2, 1.0)


def test_a_nan_in_the_reference_invalidates_the_request():
    ref, probe = noise(7, 3000), noise(8, 3000)
    ref[1500] = NAN
    got = ta.align_f64(ref, SR, probe, SR, request(1000, 2000, 5, CURVE))
    assert got[0] == 1.0 and np.isnan(got[1:]).all()
    assert np.array_equal(bits(got[10:]), bits(R.align(ref, probe, 1000, 2000, 5, CURVE)[10:]))
    ok = ta.align_f64(ref, SR, probe, SR, request(1501, 2000, 5))       # the NaN is outside the range: valid
    assert ok[0] == 0.0 and not np.isnan(ok).any()
    # an empty range is invalid too (no lags, E_ref = 0)
    empty = ta.align_f64(ref, SR, probe, SR, ta.align_request(start_sec=0.01, end_sec=0.01, max_lag_sec=0.001, kind=CURVE))
    assert empty.size == 10 and empty[0] == 1.0 and np.isnan(empty[1:]).all()


@pytest.mark.parametrize("i", [0, 1990, 2004, 2500, 3010, 3011, 3499])
def test_a_nan_in_the_probe_hits_exactly_the_lags_that_meet_it(i):
    s0, s1, D = 2000, 3000, 12
    ref, probe = noise(9, 3200), noise(10, 3500)
    probe[i] = NAN
    got = ta.align_f64(ref, SR, probe, SR, request(s0, s1, D, CURVE))
    hit = np.array([s0 <= i - l < s1 for l in range(-D, D + 1)])
    assert np.array_equal(np.isnan(got[10:]), hit)
    assert got[0] == (1.0 if hit.any() else 0.0)


# ------------------------------------------------------------------------------------------------ the planner
@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-ffp-contract=off", "-o", LIB] + SRC)
    so = C.CDLL(LIB)
    so.emu_align_plan.restype = C.c_int64
    return so


@pytest.mark.parametrize("N, n_lags", [(1, 1), (1000, 141), (131072, 65535), (131073, 65536), (131073, 65537), (1 << 22, 2 * 65536 + 5),
                                       (300000, (1 << 21) + 1), (1 << 22, (1 << 18) - 1), (5, 0), (0, 0)])
def test_pieces_cover_every_lag_once_and_in_order(emu, N, n_lags):
    out = np.zeros(4096, np.uint64)
    n = emu.emu_align_plan(C.c_uint64(N), C.c_uint64(n_lags), out.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_uint64(out.size))
    assert n >= 5
    v = [int(x) for x in out[:n]]
    n_pieces, scratch, rec, tile, group = v[:5]
    assert group == R.GROUP and n_pieces == -(-n_lags // api.ALIGN_PIECE_LAGS) and n == 5 + 5 * n_pieces
    at, groups = 0, -(-N // group)
    for p in range(n_pieces):
        lag0, cnt, n_tiles, n_groups, n_blocks = v[5 + 5 * p: 10 + 5 * p]
        assert lag0 == at and 1 <= cnt <= api.ALIGN_PIECE_LAGS
        assert cnt == api.ALIGN_PIECE_LAGS or p == n_pieces - 1            # only the last piece is short
        assert n_tiles == -(-cnt // tile) and n_groups == groups and n_blocks == n_tiles * n_groups
        assert n_groups * cnt <= scratch and cnt <= rec
        at += cnt
    assert at == n_lags
    # the bounds of the device memory: 16 MiB of group values, a record buffer of one piece
    assert scratch * 8 <= 16 << 20 and rec <= api.ALIGN_PIECE_LAGS
    assert scratch == (groups * min(n_lags, api.ALIGN_PIECE_LAGS) if n_lags else 0)
