"""The spectrum-of-a-time-range entries (th_spectrum_frame_range, th_tm_get_spectra / th_tm_get_spectrum and their th_tmg twins):
the interface, the NULL-handle checks, and the host-only frame-range helper against its definition restated in Python (Python
floats are C doubles).  CPU only."""
import ctypes as C
import math
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMS = ["th_spectrum_frame_range", "th_tm_get_spectra", "th_tm_get_spectrum", "th_tmg_get_spectra", "th_tmg_get_spectrum"]
INF = float("inf")
NAN = float("nan")


def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"TH_API\s+[\w\s\*]+?\b(th_\w+)\s*\(", txt))


def test_symbols_are_declared_exported_and_bound():
    import thesia_amd
    from thesia_amd import _ffi
    assert set(SYMS) <= _declared("thesia_amd.h")
    assert not set(SYMS) & _declared("thesia_amd_testing.h")
    lib = C.CDLL(thesia_amd.LIB_PATH)
    assert all(hasattr(lib, s) for s in SYMS), [s for s in SYMS if not hasattr(lib, s)]
    assert set(SYMS) <= set(_ffi._SIGS)
    assert (thesia_amd.SPECTRUM_MEAN_AMP, thesia_amd.SPECTRUM_MEAN_POWER, thesia_amd.SPECTRUM_MAX) == (0, 1, 2)
    for cls in (thesia_amd.TrackManager, thesia_amd.MultiTrackManager):
        assert callable(cls.spectrum) and callable(cls.spectra)


def test_tmg_twins_have_the_same_arguments_after_the_handle():
    from thesia_amd import _ffi
    for name in ("get_spectra", "get_spectrum"):
        assert _ffi._SIGS["th_tmg_" + name][1:] == _ffi._SIGS["th_tm_" + name][1:], name


def test_struct_layouts_match_the_header():
    from thesia_amd import _ffi
    assert C.sizeof(_ffi.SpectrumRequest) == 32 and _ffi.SpectrumRequest.start_sec.offset == 16
    assert C.sizeof(_ffi.SpectrumInfo) == 40 and _ffi.SpectrumInfo.spectrogram_revision.offset == 32


def test_null_handles_are_invalid_arguments():
    from thesia_amd import _ffi
    req = (_ffi.SpectrumRequest * 1)(_ffi.SpectrumRequest(0, 0, 0, 0.0, INF))
    info = (_ffi.SpectrumInfo * 1)()
    n = C.c_size_t()
    out = (C.c_float * 4)()
    for pfx in ("th_tm_", "th_tmg_"):
        assert getattr(_ffi.lib, pfx + "get_spectra")(None, req, 1, out, 4, info, C.byref(n)) == _ffi.ERR_INVALID_ARG
        assert getattr(_ffi.lib, pfx + "get_spectrum")(None, 0, 0, 0, 0.0, INF, out, 4, info) == _ffi.ERR_INVALID_ARG
    f0, f1 = C.c_size_t(), C.c_size_t()
    assert _ffi.lib.th_spectrum_frame_range(48000, 480, 10, 0.0, INF, None, C.byref(f1)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_spectrum_frame_range(48000, 480, 10, 0.0, INF, C.byref(f0), None) == _ffi.ERR_INVALID_ARG


def restated(sr, hop, T, a, b):
    clamp = lambda x: T if x >= T else int(x)  # noqa: E731  (x >= 0)
    f0 = clamp(math.ceil(a * sr / hop))
    f1 = T if b == INF else max(f0, clamp(math.ceil(b * sr / hop)))
    return f0, f1


@pytest.mark.parametrize("sr, hop, T, a, b, want", [
    (48000, 480, 3001, 0.0, INF, (0, 3001)),
    (48000, 480, 3001, 0.01, 0.02, (1, 2)),
    (48000, 480, 3001, 29.99, 31.0, (2999, 3001)),
    (44100, 441, 100, 0.005, 0.0051, (1, 1)),
])
def test_frame_range_known_cases(sr, hop, T, a, b, want):
    import thesia_amd as ta
    assert ta.spectrum_frame_range(sr, hop, T, a, b) == want
    assert restated(sr, hop, T, a, b) == want


def test_frame_range_matches_the_restatement_on_random_ranges():
    import thesia_amd as ta
    rnd = random.Random(20251017)
    for _ in range(400):
        sr = rnd.choice([8000, 11025, 22050, 44100, 48000, 96000, 192000])
        hop = rnd.choice([1, 20, 128, 441, 480, 512, 1000, 4096])
        T = rnd.choice([0, 1, 2, 51, 1200, 3001, 120000])
        dur = T * hop / sr
        a = rnd.choice([0.0, rnd.uniform(0.0, 1.2 * dur + 0.01), rnd.randrange(0, T + 2) * hop / sr])
        b = rnd.choice([INF, a, a + rnd.uniform(0.0, dur + 0.01), a + rnd.randrange(0, T + 2) * hop / sr])
        f0, f1 = ta.spectrum_frame_range(sr, hop, T, a, b)
        assert (f0, f1) == restated(sr, hop, T, a, b), (sr, hop, T, a, b)
        assert 0 <= f0 <= f1 <= T
    assert ta.spectrum_frame_range(48000, 480, 100) == (0, 100)  # the defaults: the whole track


@pytest.mark.parametrize("sr, hop, a, b", [
    (48000, 480, NAN, 1.0), (48000, 480, -0.001, 1.0), (48000, 480, INF, INF), (48000, 480, -INF, 1.0),
    (48000, 480, 0.0, NAN), (48000, 480, 1.0, 0.999), (48000, 480, 0.5, -INF),
    (0, 480, 0.0, 1.0), (48000, 0, 0.0, 1.0),
])
def test_frame_range_refusals(sr, hop, a, b):
    import thesia_amd as ta
    with pytest.raises(ta.ThError) as e:
        ta.spectrum_frame_range(sr, hop, 100, a, b)
    assert e.value.code == -1
