"""Export as figures, the host side (no GPU): the definition's numpy restatement (tests/figure_ref.py) against Pillow's committed
answers, th_figure_axis and th_figure_box against the restatement, the interface, and plan_figures under AddressSanitizer and UBSan
in a stand-alone program (scripts/san_figure_plan.cpp)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi
from tests import figure_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def test_restatement_equals_pillow(golden_dir):
    """tests/golden/figure_pillow_cases.npz (scripts/make_golden_figure.py, Pillow 12.2): boxes exact in float32, reductions and
    enlargements, boxes at the image's edges, less than a pixel, both images"""
    z = np.load(os.path.join(golden_dir, "figure_pillow_cases.npz"))
    assert len(z.files) == len(R.PILLOW_CASES) + 1
    for k, (name, box, out_w, out_h) in enumerate(R.PILLOW_CASES):
        want = z[f"case{k}"]
        got = R.resample(R.pillow_image(name), box, out_w, out_h)
        assert got.shape == want.shape == (out_h, out_w) and np.array_equal(got, want), (k, int((got != want).sum()))
    img = R.pillow_image("hash")
    assert np.array_equal(z["case0"], img)   # the whole image at its own size is a copy
    assert np.array_equal(R.figure(img, (0.0, 0.0, 83.0, 61.0), 83, 61, R.GREY16), img[::-1])


AXES = [(0.0, 83.0, 83, 83), (0.0, 83.0, 20, 83), (10.3, 390.6, 57, 401), (70.5, 12.5, 47, 83), (30.125, 0.75, 16, 83),
        (0.0, 6000.0, 3, 6000), (0.0, 1.0, 5, 1), (999.9, 0.1, 3, 1000), (0.0, 180000.0, 7, 180000)]


@pytest.mark.parametrize("origin,extent,n_out,n_in", AXES)
def test_figure_axis_equals_the_restatement(origin, extent, n_out, n_in):
    start, count, w = ta.figure_axis(origin, extent, n_out, n_in)
    s, c, ws = R.axis(origin, extent, n_out, n_in)
    assert np.array_equal(start, s) and np.array_equal(count, c) and w.shape == (n_out, max(int(c.max()), 1))
    for o in range(n_out):
        assert np.array_equal(w[o, :c[o]], ws[o]), o         # bit for bit
        assert not w[o, c[o]:].any()
    assert (start >= 0).all() and (start + count <= n_in).all()


def test_figure_axis_arguments():
    i32p = C.POINTER(C.c_int32)
    s, c, mt = np.zeros(4, np.int32), np.zeros(4, np.int32), C.c_uint32()
    fn = _ffi.lib.th_figure_axis
    assert fn(0.0, 8.0, 4, 8, s.ctypes.data_as(i32p), c.ctypes.data_as(i32p), None, 0, C.byref(mt)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert mt.value == int(c.max()) and c.min() > 0
    for a in ((0.0, 0.0, 4, 8), (0.0, -1.0, 4, 8), (NAN, 8.0, 4, 8), (0.0, INF, 4, 8), (0.0, 8.0, 0, 8), (0.0, 8.0, 4, 0)):
        assert fn(*a, s.ctypes.data_as(i32p), c.ctypes.data_as(i32p), None, 0, C.byref(mt)) == _ffi.ERR_INVALID_ARG, a
    assert fn(0.0, 8.0, 4, 8, None, c.ctypes.data_as(i32p), None, 0, C.byref(mt)) == _ffi.ERR_INVALID_ARG


BOX_TRACKS = [  # sr, n_samples, img_w, spec_h, img_h
    (48000, 48000 * 30, 3001, 1025, 1025),
    (44100, 44100 * 7 + 13, 2573, 1025, 1116),    # a track below max_sr: the image is higher than the spectrogram
    (22050, 1000, 3, 86, 187),
]
BOX_RANGES = [(0.0, INF, 0.0, INF), (0.4, 2.1, 200.0, 8000.0), (12.4, 47.9, 200.0, 8000.0), (0.0, 1e9, 0.0, 1e9), (5.0, INF, 3000.0, INF),
              (0.001, 0.002, 10.0, 10.5), (0.0, 0.5, 21000.0, 30000.0)]


@pytest.mark.parametrize("mel", [False, True], ids=["linear", "mel"])
def test_figure_box_equals_the_restatement(mel):
    scale = ta.MEL if mel else ta.LINEAR
    n = 0
    for tr in BOX_TRACKS:
        for rg in BOX_RANGES:
            want = R.box(*rg, *tr, mel)
            if want is None:
                with pytest.raises(ta.ThError) as e:
                    ta.figure_box(*rg, *tr, scale)
                assert e.value.code == _ffi.ERR_INVALID_ARG
                continue
            got = ta.figure_box(*rg, *tr, scale)
            assert got == want, (tr, rg)          # the same doubles
            left, top, width, height = got
            assert left >= 0 and top >= 0 and width > 0 and height > 0 and left + width <= tr[2] * (1 + 1e-12) and top + height <= tr[4] * (1 + 1e-12)
            n += 1
    assert n >= 15
    # +inf ends and clamping
    sr, ns, w, hs, hi = BOX_TRACKS[1]
    assert ta.figure_box(0.0, INF, 0.0, INF, sr, ns, w, hs, hi, scale) == (0.0, 0.0, float(w), float(hi))
    assert ta.figure_box(0.0, 1e9, 0.0, 1e9, sr, ns, w, hs, hi, scale) == (0.0, 0.0, float(w), float(hi))
    half = ta.figure_box(0.0, INF, 0.0, sr / 2, sr, ns, w, hs, hi, scale)
    assert half[1] == 0.0 and half[3] == float(hs)   # the track's own Nyquist is the spectrogram's top row, below the image's


def test_figure_box_refusals():
    ok = dict(start_sec=0.5, end_sec=2.0, hz_min=100.0, hz_max=5000.0, sr=48000, n_samples=480000, img_width=1000, spec_height=513,
              img_height=513, freq_scale=ta.LINEAR)
    assert ta.figure_box(**ok)
    bad = [dict(start_sec=NAN), dict(end_sec=NAN), dict(hz_min=NAN), dict(hz_max=NAN), dict(start_sec=-0.1), dict(start_sec=INF),
           dict(hz_min=-1.0), dict(hz_min=INF), dict(end_sec=0.5), dict(end_sec=0.25), dict(hz_max=100.0), dict(hz_max=50.0),
           dict(start_sec=11.0, end_sec=12.0),             # both clamp to the track's end
           dict(hz_min=30000.0, hz_max=40000.0),           # both clamp to the image's top
           dict(end_sec=-INF), dict(hz_max=-INF),
           dict(sr=0), dict(n_samples=0), dict(img_width=0), dict(spec_height=0), dict(img_height=0)]
    for b in bad:
        a = dict(ok, **b)
        with pytest.raises(ta.ThError) as e:
            ta.figure_box(**a)
        assert e.value.code == _ffi.ERR_INVALID_ARG, b
        assert R.box(a["start_sec"], a["end_sec"], a["hz_min"], a["hz_max"], a["sr"], a["n_samples"], a["img_width"], a["spec_height"],
                     a["img_height"], False) is None, b


@pytest.mark.parametrize("mel", [False, True], ids=["linear", "mel"])
def test_integral_boxes_reproduce_hz_range_to_idx(mel):
    """y(hz) is the continuous form of hz_range_to_idx: where the rows come out integral, floor / ceil give its crop"""
    scale = ta.MEL if mel else ta.LINEAR
    sr, n = 48000, 1024
    n_hit = 0
    for k0, k1 in [(0, 1024), (1, 1023), (10, 600), (128, 129), (333, 777), (512, 1000)]:
        if mel:   # hz of row k: the inverse of the mel ratio, then the nearest doubles that land on the row exactly, if any
            m_top = R.mel_f64(sr / 2)
            inv = lambda m: m * (200.0 / 3.0) if m < 15.0 else 1000.0 * math.exp(0.06875177742094912 * (m - 15.0))  # noqa: E731
            hz0, hz1 = inv(k0 / n * m_top), inv(k1 / n * m_top)
        else:
            hz0, hz1 = k0 * (sr / 2) / n, k1 * (sr / 2) / n
        left, top, width, height = ta.figure_box(0.0, INF, hz0, hz1, sr, 48000, 100, n, n, scale)
        i0, i1 = ta.hz_range_to_idx(scale, (np.float32(hz0), np.float32(hz1)), sr, n)
        if top == k0 and top + height == k1:
            assert (i0, i1) == (k0, k1), (k0, k1)
            n_hit += 1
        assert abs(top - k0) < 1e-9 and abs(top + height - k1) < 1e-9
        assert i0 in (math.floor(top), math.floor(top) - 1, math.floor(top) + 1)   # (f32 against f64 next to an integer)
    assert n_hit >= (6 if not mel else 1)


NEW = ["th_figure_axis", "th_figure_box", "th_tm_figure_box", "th_tm_render_figures", "th_tm_render_figure", "th_tmg_figure_box",
       "th_tmg_render_figures", "th_tmg_render_figure"]


def test_interface_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "thesia_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(ta.LIB_PATH)
    for s in NEW:
        assert re.search(r"TH_API\s+int\s+%s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _ffi._SIGS, s
        assert "_dev" not in s
    testing = open(os.path.join(ROOT, "include", "thesia_amd_testing.h")).read()
    assert "figure" not in testing
    for name, val in (("TH_FIGURE_RGBA", 0), ("TH_FIGURE_GREY16", 1), ("TH_FIGURE_MAX_DIM", 16384)):
        assert re.search(r"#define\s+%s\s+%du?\b" % (name, val), code), name
    assert re.search(r"#define\s+TH_FIGURE_PIECE_BYTES\s+\(8u << 20\)", code) and ta.api.FIGURE_PIECE_BYTES == 8 << 20
    assert re.search(r"#define\s+TH_FIGURE_TMP_BYTES\s+\(16u << 20\)", code) and ta.api.FIGURE_TMP_BYTES == 16 << 20
    assert C.sizeof(_ffi.FigureRequest) == 56 and C.sizeof(_ffi.FigureInfo) == 32
    for cls in (ta.TrackManager, ta.MultiTrackManager):
        assert all(hasattr(cls, m) for m in ("render_figures", "render_figure", "figure_box"))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    binding = "\n".join(re.findall(r"```rust(.*?)```", integ, flags=re.S))
    assert "th_tm_render_figures" in binding and "th_figure_box" in binding


def test_render_entries_refuse_null_handles():
    req = _ffi.FigureRequest(0, 0, 0, 4, 4, 0.0, 0.0, 1.0, 1.0)
    info, need = _ffi.FigureInfo(), C.c_size_t()
    assert _ffi.lib.th_tm_render_figures(None, C.byref(req), 1, None, 0, C.byref(info), C.byref(need)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tmg_render_figures(None, C.byref(req), 1, None, 0, C.byref(info), C.byref(need)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tm_render_figure(None, C.byref(req), None, 0, C.byref(info)) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tmg_render_figure(None, C.byref(req), None, 0, C.byref(info)) == _ffi.ERR_INVALID_ARG
    d = [C.c_double() for _ in range(4)]
    assert _ffi.lib.th_tm_figure_box(None, 0, 0, 0.0, 1.0, 0.0, 1.0, *[C.byref(v) for v in d]) == _ffi.ERR_INVALID_ARG
    assert _ffi.lib.th_tmg_figure_box(None, 0, 0, 0.0, 1.0, 0.0, 1.0, *[C.byref(v) for v in d]) == _ffi.ERR_INVALID_ARG


def test_plan_figures_under_sanitizers(tmp_path):
    """scripts/san_figure_plan.cpp, a stand-alone program with its own main, built with g++ -fsanitize=address,undefined: every output
    row in exactly one piece, no piece above its bounds, scratch and staging regions disjoint, tap tables deduplicated"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the planner's sanitizer run"
    exe = str(tmp_path / "san_figure_plan")
    src = [os.path.join(ROOT, "scripts", "san_figure_plan.cpp"), os.path.join(ROOT, "thesia_amd", "csrc", "figure_plan.cpp"),
           os.path.join(ROOT, "thesia_amd", "csrc", "host_math.cpp")]
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"san_figure_plan: \d+ plans .* nothing reported", r.stdout), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
