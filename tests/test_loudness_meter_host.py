"""The loudness meter's interface and host arithmetic (th_true_peak_filter, th_loudness_range, th_loudness_n_short_term) against the
restatement of tests/loudness_meter_ref.py and the EBU Tech 3342 signals.  CPU only."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import thesia_amd as ta
from tests import loudness_meter_ref as mref
from tests import loudness_ref as ref
from thesia_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("get_loudness_meters", "get_loudness_meter")
HOST = ("th_true_peak_filter", "th_loudness_n_short_term", "th_loudness_range")


def _header():
    return open(os.path.join(ROOT, "include", "thesia_amd.h")).read()


def _decl_args(txt, name):
    m = re.search(r"TH_API\s+int\s+" + name + r"\s*\((.*?)\);", txt, flags=re.S)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def test_symbols_declared_exported_bound():
    txt = _header()
    lib = C.CDLL(ta.LIB_PATH)
    for name in [p + n for p in ("th_tm_", "th_tmg_") for n in NAMES] + list(HOST):
        _decl_args(txt, name)
        assert hasattr(lib, name), name
        assert name in _ffi._SIGS, name
    for n in NAMES:  # the twins take the same arguments after the handle
        a = [re.sub(r"\s+", " ", t).strip() for t in _decl_args(txt, "th_tm_" + n).split(",")][1:]
        b = [re.sub(r"\s+", " ", t).strip() for t in _decl_args(txt, "th_tmg_" + n).split(",")][1:]
        assert a == b, n
        assert _ffi._SIGS["th_tm_" + n] == _ffi._SIGS["th_tmg_" + n], n
    for cls in (ta.TrackManager, ta.MultiTrackManager):
        assert callable(cls.loudness_meters) and callable(cls.loudness_meter)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    binding = "\n".join(re.findall(r"```rust(.*?)```", integ, flags=re.S))
    for name in ("th_tm_get_loudness_meters", "th_tm_get_loudness_meter", "th_loudness_meter") + HOST:
        assert name in binding, name


def test_struct_layout_matches_header():
    """th_loudness_meter as a C compiler lays it out (all members naturally aligned, no padding: 3 f64, 2 f32, 2 u32, 5 u64)"""
    m = re.search(r"typedef struct \{([^}]*)\}\s*th_loudness_meter;", _header())
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    size = {"double": 8, "float": 4, "uint32_t": 4, "uint64_t": 8}
    off, want = 0, []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        for nm in names.split(","):
            off = (off + size[ty] - 1) // size[ty] * size[ty]
            want.append((nm.strip(), off, size[ty]))
            off += size[ty]
    got = [(n, getattr(_ffi.LoudnessMeter, n).offset, getattr(_ffi.LoudnessMeter, n).size) for n, _ in _ffi.LoudnessMeter._fields_]
    assert got == want
    assert C.sizeof(_ffi.LoudnessMeter) == (off + 7) // 8 * 8 == 80


def test_null_handles_are_invalid_arg():
    lib = _ffi.lib
    ids = (C.c_size_t * 1)(1)
    ms = (_ffi.LoudnessMeter * 1)()
    need = C.c_size_t()
    for pfx in ("th_tm_", "th_tmg_"):
        assert getattr(lib, pfx + "get_loudness_meters")(None, ids, 1, ms, None, 0, C.byref(need)) == -1
        assert getattr(lib, pfx + "get_loudness_meter")(None, 1, ms, None, 0) == -1
    assert lib.th_loudness_range(None, 3, C.byref(C.c_double())) == -1
    assert lib.th_loudness_n_short_term(10, 48000, None) == -1
    assert lib.th_loudness_n_short_term(10, 8, C.byref(need)) == -2


@pytest.mark.parametrize("sr", [8000, 44100, 48000, 95999, 96000, 191999, 192000])
def test_true_peak_filter_matches_restatement(sr):
    F, coef, phase, delay = ta.true_peak_filter(sr)
    wF, wcoef, wphase, wdelay = mref.true_peak_filter(sr)
    assert F == wF == (4 if sr < 96000 else 2 if sr < 192000 else 1)
    assert np.array_equal(phase, wphase) and np.array_equal(delay, wdelay)
    assert coef.shape == wcoef.shape and np.abs(coef - wcoef).max() <= 1e-15
    counts = [int((phase == f).sum()) for f in range(F)]
    assert counts == {4: [1, 12, 12, 12], 2: [1, 24], 1: [1]}[F]
    if F > 1:
        # phase 0 is the sample itself, delayed; the other phases' delays are 0 .. T - 1; the largest sum of |c| of a phase
        assert coef[phase == 0][0] == 1.0 and delay[phase == 0][0] == 24 // F
        for f in range(1, F):
            assert np.array_equal(delay[phase == f], np.arange(mref.PHASE_TAPS[F]))
        gain = max(np.abs(coef[phase == f]).sum() for f in range(F))
        assert abs(gain - mref.PHASE_GAIN[F]) <= 5e-5 and gain <= mref.PHASE_GAIN[F] + 5e-5


def test_loudness_range_matches_restatement_exactly():
    rng = np.random.default_rng(31)
    for trial in range(40):
        n = int(rng.integers(1, 200))
        lo = rng.uniform(-80, -20)
        e = 10.0 ** (rng.uniform(lo, lo + rng.uniform(1, 50), n) / 10.0)
        if trial % 4 == 0:
            e[rng.integers(0, n, max(1, n // 5))] = np.nan
        if trial % 5 == 0:
            e[rng.integers(0, n, max(1, n // 7))] = 0.0
        assert ta.loudness_range(e) == mref.loudness_range(e), trial
    assert ta.loudness_range([]) == 0.0 == mref.loudness_range([])
    below = np.full(20, ref.BOUNDARIES[0] * 0.999)
    assert ta.loudness_range(below) == 0.0 == mref.loudness_range(below)
    assert ta.loudness_range([1e-3]) == 0.0 == mref.loudness_range([1e-3])
    e = np.array([1e-3, np.nan, 1e-2, np.nan, 1e-3, 1e-2, np.nan])
    assert ta.loudness_range(e) == ta.loudness_range(e[~np.isnan(e)]) == mref.loudness_range(e)
    assert ta.loudness_range(np.full(5, np.nan)) == 0.0


def test_fast_filter_is_the_sequential_one():
    """kfilter_fast (pieces side by side) against loudness_ref.kfilter on DC-heavy audio: equal up to the f64 filter's own rounding"""
    rng = np.random.default_rng(32)
    x = (0.4 + 0.3 * rng.uniform(-1, 1, (2, 3 * 8000 + 7))).astype(np.float32)
    a, b = ref.kfilter(x, 8000), mref.kfilter_fast(x, 8000)
    ea, eb = mref.series_energies_of(a, 8000, 4), mref.series_energies_of(b, 8000, 4)
    assert np.abs(ea - eb).max() / ea.max() <= 1e-13
    ea, eb = mref.series_energies_of(a, 8000, 30), mref.series_energies_of(b, 8000, 30)
    assert ea.size == 1 and np.abs(ea - eb).max() / ea.max() <= 1e-13


def _sine_steps(levels_db, sr=8000, seconds=20):
    t = np.arange(seconds * sr * len(levels_db)) / sr
    g = np.repeat([10.0 ** (db / 20.0) for db in levels_db], seconds * sr)
    return (g * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)[None]


TECH_3342 = [((-20, -30), 10.0), ((-20, -15), 5.0), ((-40, -20), 20.0), ((-50, -35, -20, -35, -50), 15.0)]


@pytest.mark.parametrize("levels,want", TECH_3342)
def test_ebu_tech_3342_cases(levels, want):
    """Tech 3342 cases 1-4: 1 kHz mono sine, 20 s per level"""
    sr = 8000
    x = _sine_steps(levels, sr)
    es = mref.series_energies_of(mref.kfilter_fast(x, sr), sr, 30)
    assert es.size == ta.loudness_n_short_term(x.shape[1], sr) == mref.n_short_term(x.shape[1], sr)
    got = ta.loudness_range(es[::10])
    assert got == mref.loudness_range(es[::10])
    assert abs(got - want) <= 1.0
    assert abs(got - want) <= 1e-9, got  # (the restatement gives the nominal values exactly on these signals)


@pytest.mark.parametrize("sr", [8000, 44100, 48000])
def test_n_short_term_edges(sr):
    s = ref.s100(sr)
    for n, want in ((30 * s - 1, 0), (30 * s, 1), (30 * s + s - 1, 1), (31 * s, 2), (0, 0)):
        assert ta.loudness_n_short_term(n, sr) == want == mref.n_short_term(n, sr)
