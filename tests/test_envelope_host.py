"""The waveform envelope, the host side (no GPU): th_envelope_edges and th_waveform_figure_span against the numpy restatement
(tests/envelope_ref.py), every refusal, the interface, and the planners under AddressSanitizer and UBSan in a stand-alone program
(scripts/san_envelope_plan.cpp), which also checks the pieces' bounds and repeats the kernels' index walk."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api
from tests import envelope_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")

EDGE_CASES = [(48000, 100000, 0.0, INF, 7), (48000, 100000, 0.5, 0.50625, 1000), (8000, 40000, 0.0123, 4.2, 333), (48000, 70001, 0.0, INF, 16384),
              (48000, 1, 0.0, INF, 4), (48000, 70001, 0.0, INF, 1), (48000, 70001, 1 / 48000, INF, 5), (44100, 86400000, 12.4, 47.9, 1800),
              (48000, 70001, 0.0, 1e9, 65536), (1, 5, 0.5, 3.5, 3), (192000, 1 << 40, 0.3, 1e6, 4099),
              # B > A without a sample index between them: ceil(A) == ceil(B), every column is empty (a hold)
              (48000, 70001, 0.2 / 48000, 0.7 / 48000, 5), (48000, 70001, 1000.25 / 48000, 1000.75 / 48000, 1),
              (48000, 70001, 70000.5 / 48000, INF, 9), (48000, 1, 0.25 / 48000, 0.5 / 48000, 3)]


@pytest.mark.parametrize("sr,n,a,b,W", EDGE_CASES)
def test_edges_equal_the_restatement(sr, n, a, b, W):
    e = ta.envelope_edges(sr, n, a, b, W)
    want = R.edges(sr, n, a, b, W)
    assert e.dtype == np.uint64 and e.shape == (W + 1,) and np.array_equal(e, want)
    d = np.diff(e.astype(np.int64))
    assert (d >= 0).all() and int(e[-1]) <= n
    if (sr, n, a, b, W) in EDGE_CASES[-4:]:
        assert e[0] == e[-1] and max(int(e[0]), 1) - 1 < n     # no sample in the range; the held sample exists
    if (sr, n, W) == (48000, 100000, 7):
        assert e[0] == 0 and e[-1] == n and set(d.tolist()) == {14285, 14286}
    if (sr, n, W) == (48000, 100000, 1000):
        assert (d == 0).sum() == 700 and set(d.tolist()) == {0, 1}
    if (sr, n, W) == (48000, 70001, 16384):
        assert set(d.tolist()) == {4, 5}
    if (sr, n, W) == (48000, 1, 4):
        assert (d == 0).sum() == 3 and d.sum() == 1
    assert ta.edges is ta.envelope_edges


def test_edges_refusals():
    ok = dict(sr=48000, n_samples=100000, start_sec=0.5, end_sec=1.5, n_cols=7)
    assert ta.envelope_edges(**ok).size == 8
    bad = [dict(start_sec=NAN), dict(end_sec=NAN), dict(start_sec=-0.1), dict(start_sec=INF), dict(end_sec=0.5), dict(end_sec=0.25),
           dict(start_sec=3.0, end_sec=4.0), dict(end_sec=-INF), dict(sr=0), dict(n_samples=0), dict(n_cols=0), dict(n_cols=65537)]
    for b in bad:
        a = dict(ok, **b)
        with pytest.raises(ta.ThError) as e:
            ta.envelope_edges(**a)
        assert e.value.code == _ffi.ERR_INVALID_ARG, b
        assert R.edges(a["sr"], a["n_samples"], a["start_sec"], a["end_sec"], a["n_cols"]) is None, b
    assert ta.envelope_edges(48000, 100000, 0.0, INF, 65536).size == 65537
    assert _ffi.lib.th_envelope_edges(48000, 100000, 0.0, INF, 7, None) == _ffi.ERR_INVALID_ARG


def _spans(cols, out_h, lo, hi, th):
    """both implementations over a run of columns; returns the list"""
    cols = np.asarray(cols, np.float32)
    got = []
    for j in range(len(cols)):
        left = cols[j - 1] if j > 0 else None
        g = ta.waveform_figure_span(cols[j], left, out_h, lo, hi, th)
        assert g == R.span(cols[j], left, out_h, lo, hi, th), (j, cols[j], left, out_h, lo, hi, th)
        got.append(g)
    return got


def test_span_equals_the_restatement():
    c = lambda mn, mx: (mn, mx, (mn + mx) / 2, abs(mx))  # noqa: E731
    # joins in both directions: a column wholly below, then wholly above its left neighbour
    g = _spans([c(0.5, 0.75), c(-0.5, -0.25), c(0.25, 0.5), c(0.3, 0.4)], 100, -1.0, 1.0, 0)
    assert g[1][0] == g[0][1]                                          # raised to the neighbour's minimum
    assert g[2][1] == R._row(1.0, -1.0, np.float32(-0.25), 100) < g[1][1]   # lowered to the neighbour's UN-joined maximum
    assert g[3] == (R._row(1.0, -1.0, np.float32(0.4), 100), R._row(1.0, -1.0, np.float32(0.3), 100))
    # the thickness rule in the middle, at the top clamp and at the bottom clamp; thickness 0
    assert _spans([c(0.0, 0.0)], 10, -1.0, 1.0, 256) == [(1152, 1408)]
    assert _spans([c(1.0, 1.0)], 10, -1.0, 1.0, 256) == [(0, 128)]
    assert _spans([c(-1.0, -1.0)], 10, -1.0, 1.0, 256) == [(2432, 2560)]
    assert _spans([c(3.0, 5.0)], 10, -1.0, 1.0, 300) == [(0, 150)]
    assert _spans([c(0.0, 0.0)], 10, -1.0, 1.0, 0) == [(1280, 1280)]
    assert _spans([c(0.0, 0.0)], 10, -1.0, 1.0, 2560) == [(0, 2560)]
    assert _spans([c(0.0, 0.0)], 10, -1.0, 1.0, 255) == [(1152, 1407)]     # floor of an odd difference
    assert _spans([c(0.0, 0.0)], 1, -1.0, 1.0, 0) == [(128, 128)]
    # all-NaN columns draw nothing and are not joined to; a NaN mean draws nothing; +-inf clamp
    g = _spans([c(0.5, 0.75), (INF, -INF, NAN, NAN), c(-0.5, -0.25), (-0.5, 0.5, NAN, NAN), (NAN, NAN, NAN, NAN), c(0.1, 0.2)], 64, -1.0, 1.0, 256)
    assert g[1] is None and g[3] is None and g[4] is None
    assert g[2] == R.span(c(-0.5, -0.25), None, 64, -1.0, 1.0, 256)   # its left neighbour is all NaN: no join
    g = _spans([(-INF, INF, NAN, INF), (-INF, INF, 0.0, INF), (INF, INF, INF, INF), (-INF, -INF, -INF, INF), (-1e30, 1e30, 0.0, 1e30)], 7, -0.5, 0.25, 100)
    assert g[0] is None and g[1] == (0, 7 * 256) and g[4] == (0, 7 * 256)
    assert g[2] == (0, 50) and g[3] == (0, 7 * 256)   # a point at the top clamp; -inf joined up to the neighbour's +inf
    # random columns, odd ranges
    rng = np.random.default_rng(5)
    cols = rng.normal(0, 0.6, (400, 2)).astype(np.float32)
    cols = np.stack([cols.min(1), cols.max(1), cols.mean(1), np.abs(cols).max(1)], 1)
    for out_h, lo, hi, th in [(64, -1.0, 1.0, 256), (5, -0.3, 0.9, 0), (333, -2.0, 0.1, 700), (16384, -1.0, 1.0, 16384 * 256), (1, 0.0, 0.5, 13)]:
        _spans(cols, out_h, lo, hi, th)


def test_span_refusals():
    col = np.zeros(4, np.float32)
    for a in [(0, -1.0, 1.0, 0), (16385, -1.0, 1.0, 0), (4, 1.0, 1.0, 0), (4, 1.0, -1.0, 0), (4, NAN, 1.0, 0), (4, -1.0, INF, 0), (4, -INF, 1.0, 0),
              (4, -1.0, 1.0, 4 * 256 + 1)]:
        with pytest.raises(ta.ThError) as e:
            ta.waveform_figure_span(col, None, *a)
        assert e.value.code == _ffi.ERR_INVALID_ARG, a
    yt, yb, dr = C.c_int32(), C.c_int32(), C.c_int()
    assert _ffi.lib.th_waveform_figure_span(None, None, 4, -1.0, 1.0, 0, C.byref(yt), C.byref(yb), C.byref(dr)) == _ffi.ERR_INVALID_ARG


def test_restatement_on_a_known_signal():
    """the restatement itself: columns of a ramp, a hold, a NaN, an all-NaN column, infinities, +-0"""
    x = np.arange(10, dtype=np.float32)
    env, _ = R.envelope(x, np.array([0, 5, 5, 10], np.uint64))
    assert env[0].tolist() == [0.0, 4.0, 2.0, np.float32(np.sqrt(6.0))] and env[1].tolist() == [4.0, 4.0, 4.0, 4.0]
    assert env[2].tolist() == [5.0, 9.0, 7.0, np.float32(np.sqrt(51.0))]
    env, _ = R.envelope(np.array([-3.0], np.float32), np.array([0, 0, 1], np.uint64))
    assert env[0].tolist() == [-3.0, -3.0, -3.0, 3.0]          # sample max(0, 1) - 1
    x = np.array([1.0, NAN, 3.0, NAN, NAN, INF, 1.0, -INF, INF], np.float32)
    env, _ = R.envelope(x, np.array([0, 3, 5, 7, 9], np.uint64))
    assert env[0, 0] == 1.0 and env[0, 1] == 3.0 and np.isnan(env[0, 2:]).all()
    assert env[1, 0] == INF and env[1, 1] == -INF and np.isnan(env[1, 2:]).all()
    assert env[2].tolist() == [1.0, INF, INF, INF]
    assert env[3, 0] == -INF and env[3, 1] == INF and np.isnan(env[3, 2]) and env[3, 3] == INF
    img = R.lane(np.array([[-0.5, 0.5, 0.0, 0.1]], np.float32), 4, -1.0, 1.0, 0, (255, 0, 10, 255), (0, 0, 0, 0))
    assert img.shape == (4, 1, 4) and img[:, 0, 0].tolist() == [0, 255, 255, 0] and img[:, 0, 2].tolist() == [0, 10, 10, 0]


NEW = ["th_envelope_edges", "th_waveform_figure_span", "th_tm_get_envelopes", "th_tm_get_envelope", "th_tm_render_waveform_figures",
       "th_tm_render_waveform_figure", "th_tmg_get_envelopes", "th_tmg_get_envelope", "th_tmg_render_waveform_figures",
       "th_tmg_render_waveform_figure"]


def test_interface_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "thesia_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(ta.LIB_PATH)
    for s in NEW:
        assert re.search(r"TH_API\s+int\s+%s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _ffi._SIGS, s
    testing = open(os.path.join(ROOT, "include", "thesia_amd_testing.h")).read()
    assert "envelope" not in testing
    assert re.search(r"#define\s+TH_ENVELOPE_MAX_COLS\s+65536u\b", code) and api.ENVELOPE_MAX_COLS == 65536
    assert re.search(r"#define\s+TH_ENVELOPE_PIECE_BYTES\s+\(4u << 20\)", code) and api.ENVELOPE_PIECE_BYTES == 4 << 20
    assert re.search(r"#define\s+TH_ENVELOPE_PART_BYTES\s+\(32u << 20\)", code) and api.ENVELOPE_PART_BYTES == 32 << 20
    plan = open(os.path.join(ROOT, "thesia_amd", "csrc", "envelope_plan.h")).read()
    assert re.search(r"ENV_CHUNK = %d;" % api.ENVELOPE_CHUNK, plan) and re.search(r"ENV_DENSE_MIN = %d;" % api.ENVELOPE_DENSE_MIN, plan)
    assert "hip/hip_runtime.h" not in plan and "hip/hip_runtime.h" not in open(os.path.join(ROOT, "thesia_amd", "csrc", "envelope_plan.cpp")).read()
    assert C.sizeof(_ffi.EnvelopeRequest) == 40 and C.sizeof(_ffi.EnvelopeInfo) == 40
    assert C.sizeof(_ffi.WaveformFigureRequest) == 64 and C.sizeof(_ffi.WaveformFigureInfo) == 48
    for cls in (ta.TrackManager, ta.MultiTrackManager):
        assert all(hasattr(cls, m) for m in ("get_envelopes", "get_envelope", "render_waveform_figures", "render_waveform_figure"))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    binding = "\n".join(re.findall(r"```rust(.*?)```", integ, flags=re.S))
    assert "th_tm_get_envelopes" in binding and "th_tm_render_waveform_figures" in binding and "th_envelope_edges" in binding


def test_reader_entries_refuse_null_handles():
    req = _ffi.EnvelopeRequest(0, 0, 0, 0.0, 1.0, 4, 0)
    info, need = _ffi.EnvelopeInfo(), C.c_size_t()
    assert _ffi.lib.th_tm_get_envelopes(None, C.byref(req), 1, None, 0, C.byref(info), C.byref(need)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tmg_get_envelopes(None, C.byref(req), 1, None, 0, C.byref(info), C.byref(need)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tm_get_envelope(None, C.byref(req), None, 0, C.byref(info)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tmg_get_envelope(None, C.byref(req), None, 0, C.byref(info)) == _ffi.ERR_INVALID_ARG
    lreq, linfo = _ffi.WaveformFigureRequest(), _ffi.WaveformFigureInfo()
    assert _ffi.lib.th_tm_render_waveform_figures(None, C.byref(lreq), 1, None, 0, C.byref(linfo), C.byref(need)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tmg_render_waveform_figures(None, C.byref(lreq), 1, None, 0, C.byref(linfo), C.byref(need)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tm_render_waveform_figure(None, C.byref(lreq), None, 0, C.byref(linfo)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tmg_render_waveform_figure(None, C.byref(lreq), None, 0, C.byref(linfo)) == _ffi.ERR_INVALID_ARG


def test_plans_under_sanitizers(tmp_path):
    """scripts/san_envelope_plan.cpp, a stand-alone program with its own main, built with g++ -fsanitize=address,undefined: pieces
    within TH_ENVELOPE_PIECE_BYTES, TH_ENVELOPE_PART_BYTES and TH_FIGURE_PIECE_BYTES, regions disjoint and aligned, every sample read once
    and every column written once by the kernels' index walk"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the planner's sanitizer run"
    exe = str(tmp_path / "san_envelope_plan")
    src = [os.path.join(ROOT, "scripts", "san_envelope_plan.cpp"), os.path.join(ROOT, "thesia_amd", "csrc", "envelope_plan.cpp"),
           os.path.join(ROOT, "thesia_amd", "csrc", "host_math.cpp")]
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"san_envelope_plan: \d+ plans .* nothing reported", r.stdout), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
