"""The definition of a figure (include/thesia_amd.h, "Export as figures") restated in numpy: the taps of one axis, the two passes,
the flip and the colour index.  Shares nothing with the library; bit-identical to Pillow 12.2's Image.resize(LANCZOS, box=...) on
I;16 images for boxes whose ends and extents are exact in float32 (tests/golden/figure_pillow_cases.npz)."""
from __future__ import annotations

import math

import numpy as np

RGBA, GREY16 = 0, 1


def _lanczos(x: float) -> float:
    if -3.0 <= x < 3.0:
        if x == 0.0:
            return 1.0
        a, b = x * math.pi, (x / 3) * math.pi
        return (math.sin(a) / a) * (math.sin(b) / b) if b != 0.0 else math.sin(a) / a
    return 0.0


def axis(origin: float, extent: float, n_out: int, n_in: int):
    """-> (start[n_out], count[n_out], list of weight arrays): window [(int)(c - s + .5), (int)(c + s + .5)) clipped to [0, n_in)"""
    sc = extent / float(n_out)
    f = 1.0 if sc < 1.0 else sc
    sup, ss = 3.0 * f, 1.0 / f
    start, count, ws = np.empty(n_out, np.int32), np.empty(n_out, np.int32), []
    for o in range(n_out):
        center = origin + (float(o) + 0.5) * sc
        i0, i1 = int(center - sup + 0.5), int(center + sup + 0.5)  # (truncation toward zero, as the C casts)
        i0, i1 = max(i0, 0), min(i1, n_in)
        i1 = max(i1, i0)
        w = np.array([_lanczos((float(t + i0) - center + 0.5) * ss) for t in range(i1 - i0)], np.float64)
        ww = 0.0
        for v in w:
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        start[o], count[o] = i0, i1 - i0
        ws.append(w)
    return start, count, ws


def _pass_rows(src: np.ndarray, start, count, ws) -> np.ndarray:
    """resample axis 1 of src (u16, [rows, n_in]) -> u16 [rows, n_out]: taps added in ascending order from 0.0, mul then add"""
    out = np.empty((src.shape[0], len(ws)), np.uint16)
    s64 = src.astype(np.float64)
    for o, w in enumerate(ws):
        acc = np.zeros(src.shape[0], np.float64)
        for t in range(int(count[o])):
            acc = acc + float(w[t]) * s64[:, int(start[o]) + t]
        out[:, o] = np.clip(np.floor(acc + 0.5), 0.0, 65535.0).astype(np.uint16)
    return out


def resample(img: np.ndarray, box, out_w: int, out_h: int) -> np.ndarray:
    """the u16 result in IMAGE row order (row 0 = the box's lowest rows): horizontal pass over the rows the vertical windows
    reach (every row would give the same pixels), then the vertical pass"""
    left, top, width, height = (float(v) for v in box)
    h, w = img.shape
    sx, cx, wx = axis(left, width, out_w, w)
    sy, cy, wy = axis(top, height, out_h, h)
    y_lo, y_hi = int(sy.min()), int((sy + cy).max())
    tmp = np.zeros((h, out_w), np.uint16)
    tmp[y_lo:y_hi] = _pass_rows(img[y_lo:y_hi], sx, cx, wx)
    return np.ascontiguousarray(_pass_rows(np.ascontiguousarray(tmp.T), sy, cy, wy).T)


def colour_index(v: np.ndarray, n_colors: int) -> np.ndarray:
    return (v.astype(np.uint64) * np.uint64(max(n_colors - 1, 0)) + np.uint64(32767)) // np.uint64(65535)


def figure(img: np.ndarray, box, out_w: int, out_h: int, kind: int, colormap: np.ndarray | None = None) -> np.ndarray:
    """what th_tm_render_figure returns: rows flipped (top = highest frequency); RGBA [out_h, out_w, 4] u8 through
    colormap [n_colors, 4] u8, or GREY16 [out_h, out_w] u16"""
    g = resample(img, box, out_w, out_h)[::-1]
    if kind == GREY16:
        return np.ascontiguousarray(g)
    return np.ascontiguousarray(colormap[colour_index(g, colormap.shape[0])])


def mel_f64(hz: float) -> float:
    return hz / (200.0 / 3.0) if hz < 1000.0 else 15.0 + math.log(hz / 1000.0) / 0.06875177742094912


def box(start_sec, end_sec, hz_min, hz_max, sr, n_samples, img_w, spec_h, img_h, mel: bool):
    """th_figure_box restated; None where it refuses"""
    a = (start_sec, end_sec, hz_min, hz_max)
    if any(math.isnan(v) for v in a) or start_sec < 0 or math.isinf(start_sec) or hz_min < 0 or math.isinf(hz_min):
        return None
    if 0 in (sr, n_samples, img_w, spec_h, img_h):
        return None
    W, Hs, Hi, half = float(img_w), float(spec_h), float(img_h), float(sr) / 2.0

    def x_of(sec):
        return sec * float(sr) / float(n_samples) * W

    def y_of(hz):
        return (mel_f64(hz) / mel_f64(half) if mel else hz / half) * Hs

    def clamp(v, hi):
        return 0.0 if v < 0.0 else (hi if v > hi else v)

    x0, x1 = clamp(x_of(start_sec), W), (W if end_sec == math.inf else clamp(x_of(end_sec), W))
    y0, y1 = clamp(y_of(hz_min), Hi), (Hi if hz_max == math.inf else clamp(y_of(hz_max), Hi))
    if not x1 > x0 or not y1 > y0:
        return None
    return x0, y0, x1 - x0, y1 - y0


# The Pillow pin (tests/golden/figure_pillow_cases.npz, scripts/make_golden_figure.py): (image, (left, top, width, height), out_w,
# out_h).  Box ends and extents are multiples of 1/8, exact in float32: Pillow holds the box, and forms in1 - in0, in float32, and
# differs from the definition (double) by one step in a few pixels otherwise.  Images: lod_images formulas, values inside
# [16384, 49152) or spectrogram-like, so that Pillow's 16-bit overflow artefact is never reached.
PILLOW_CASES = [
    ("hash", (0.0, 0.0, 83.0, 61.0), 83, 61),          # the whole image at its own size: a copy
    ("hash", (0.0, 0.0, 83.0, 61.0), 20, 15),          # the whole image reduced
    ("hash", (10.25, 5.5, 40.625, 33.125), 33, 21),    # fractional box, reduced
    ("hash", (70.5, 50.25, 12.5, 10.75), 47, 39),      # a corner, enlarged: the filter is clipped at the image
    ("hash", (0.0, 0.0, 9.375, 7.125), 40, 30),        # the other corner, enlarged
    ("hash", (30.125, 20.375, 0.75, 0.5), 16, 3),      # less than a pixel
    ("hash", (3.0, 0.0, 77.0, 61.0), 7, 61),           # pure horizontal reduction
    ("hash", (0.0, 2.5, 83.0, 55.25), 83, 9),          # pure vertical reduction
    ("spec", (12.375, 8.5, 150.25, 100.875), 61, 37),
    ("spec", (0.0, 0.0, 200.0, 120.0), 1, 1),
    ("spec", (100.5, 60.25, 20.0, 10.0), 90, 45),
]


def pillow_image(name: str) -> np.ndarray:
    from tests.lod_images import _hash_image, _spec_like
    return _hash_image(61, 83, 7) if name == "hash" else _spec_like(120, 200)
