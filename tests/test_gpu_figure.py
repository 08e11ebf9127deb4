"""Export as figures (th_tm_render_figures and the th_tmg twins) on the GPU: any region of a resident u16 image at any pixel size.

Reference: the definition restated in numpy (tests/figure_ref.py, pinned to Pillow by tests/test_figure_host.py) applied to the
image th_tm_copy_img returns, or to the image th_tm_put_img placed.  Every comparison is bit-exact, both kinds.

A resident image of any shape h x w: the linear setting with win 2, hop 1 and f_overlap h - 1 has n_fft = 2 (h - 1), so h rows, and
a track of w - 1 samples has w frames; th_tm_put_img then replaces the pixels."""
import ctypes as C
import threading

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api
from tests import figure_ref as R
from tests import lod_images as li
from tests.synth import synth_track

pytestmark = pytest.mark.gpu

RGBA, GREY16 = ta.FIGURE_RGBA, ta.FIGURE_GREY16
INF = float("inf")


def _cmap(n):
    """n distinct opaque colours: the index can be read back from the bytes"""
    i = np.arange(n, dtype=np.uint32)
    return np.stack([i & 255, (i >> 8) & 255, (i * 7 + 3) & 255, np.full(n, 255)], 1).astype(np.uint8)


CMAP = _cmap(258)


@pytest.fixture(scope="module")
def ctx():
    c = ta.Context(0)
    yield c
    c.close()


def tm_with_images(ctx, imgs, cmap=CMAP):
    """a manager that holds image k of imgs as channel 0 of track k (all of one height)"""
    h = imgs[0].shape[0]
    assert all(im.shape[0] == h for im in imgs)
    assert ta.calc_framing_params(2000 / 48000, 2, h - 1, 48000) == (1, 2, 2 * (h - 1))
    tm = ta.TrackManager(ctx)
    tm.set_setting(2000 / 48000, 2, h - 1, ta.LINEAR)
    tm.set_colormap(cmap.tobytes())
    tm.add_tracks([(k, 48000, synth_track(k, 48000, im.shape[1] - 1)[None]) for k, im in enumerate(imgs)])
    tm.apply_track_list_changes()
    for k, im in enumerate(imgs):
        assert tm.img(k, 0).shape == im.shape, (tm.img(k, 0).shape, im.shape)
        tm.put_img(k, 0, im)
    return tm


def check(tm, img, track, box, out_w, out_h, cmap=CMAP):
    want = R.resample(img, box, out_w, out_h)[::-1]
    grey, _ = tm.render_figure(track, 0, GREY16, out_w, out_h, box)
    assert grey.dtype == np.uint16 and np.array_equal(grey, want), (box, out_w, out_h, int((grey != want).sum()))
    rgba, info = tm.render_figure(track, 0, RGBA, out_w, out_h, box)
    assert np.array_equal(rgba, cmap[R.colour_index(want, cmap.shape[0])]), (box, out_w, out_h)
    assert (info["out_w"], info["out_h"], info["bytes"], info["offset"]) == (out_w, out_h, out_w * out_h * 4, 0)
    return grey


@pytest.fixture(scope="module")
def small(ctx):
    """129 x 300 noise (row pitch 320, not the width) and the 129 x 1025 image of the identity case (pitch 1088)"""
    imgs = [li._hash_image(129, 300, 11), li._hash_image(129, 1025, 12), li._spec_like(129, 77)]
    tm = tm_with_images(ctx, imgs)
    yield tm, imgs
    tm.close()


SHAPES = [
    ("one_pixel", 0, (0.0, 0.0, 300.0, 129.0), 1, 1),
    ("one_pixel_of_a_corner", 0, (297.5, 127.25, 2.5, 1.75), 1, 1),
    ("sub_pixel_box", 0, (150.25, 64.5, 0.75, 0.5), 64, 3),
    ("left_bottom_edge", 0, (0.0, 0.0, 40.5, 33.25), 17, 19),
    ("right_top_edge", 0, (251.5, 100.75, 48.5, 28.25), 31, 9),
    ("pure_horizontal", 0, (10.5, 20.0, 200.25, 64.0), 37, 64),
    ("pure_vertical", 0, (16.0, 3.5, 128.0, 120.25), 128, 23),
    ("whole_at_own_size", 0, (0.0, 0.0, 300.0, 129.0), 300, 129),
    ("identity_vertical_integral_box", 1, (0.0, 0.0, 1025.0, 129.0), 512, 129),
    ("upscale_10x10", 0, (100.0, 50.0, 10.0, 10.0), 333, 257),
    ("downscale_runs_of_64", 1, (3.0, 2.0, 1000.5, 125.0), 300, 40),   # span of 128 outputs > FIG_SPAN: oc 64
    ("narrow_image", 2, (0.5, 0.5, 76.0, 128.0), 131, 67),
]


@pytest.mark.parametrize("name,track,box,out_w,out_h", SHAPES, ids=[s[0] for s in SHAPES])
def test_figure_shapes_equal_the_definition(small, name, track, box, out_w, out_h):
    tm, imgs = small
    got = check(tm, imgs[track], track, box, out_w, out_h)
    if name == "whole_at_own_size":
        assert np.array_equal(got, tm.img(0, 0)[::-1])
    if name == "identity_vertical_integral_box":
        assert np.array_equal(got, R._pass_rows(imgs[1], *R.axis(0.0, 1025.0, 512, 1025))[::-1])


def test_overview_walks_its_taps_in_steps(ctx):
    """33 x 6000 to 3 x 33: 12 000 taps per output column, far beyond one staged step; and a second figure of the same image whose
    runs of 16 outputs each need several steps"""
    img = li._hash_image(33, 6000, 21)
    tm = tm_with_images(ctx, [img])
    check(tm, img, 0, (0.0, 0.0, 6000.0, 33.0), 3, 33)
    check(tm, img, 0, (100.5, 1.0, 5800.25, 31.5), 41, 7)
    tm.close()


def test_tie_image_rounds_half_up(ctx):
    img = li.lod_image("tie")
    tm = tm_with_images(ctx, [img])
    h, w = img.shape
    g = check(tm, img, 0, (0.0, 0.0, float(w), float(h)), w // 2, h // 2)
    assert ((g != 16384) & (g != 49151)).any()
    check(tm, img, 0, (8.5, 4.5, w - 17.0, h - 9.0), (w - 17) // 2, (h - 9) // 2)
    tm.close()


@pytest.fixture(scope="module")
def big(ctx):
    img = li.lod_image(li.TILE_IMAGE)
    tm = tm_with_images(ctx, [img])
    yield tm, img
    tm.close()


def test_tile_boxes_equal_the_per_request_lod_tiles(big):
    """every LOD tile of the big image: a figure with the tile's crop box (plan_lod_tile's arithmetic) and size == the RGBA payload of
    th_tm_get_spectrogram_tile on the per-request route; all tiles of a level in one call"""
    tm, img = big
    Hh, W = img.shape
    tm.set_lod_source(True)
    n = 0
    for lx, ly in li.TILE_LEVELS:
        lod_w, lod_h = -(-W // (1 << lx)), -(-Hh // (1 << ly))
        reqs, want = [], []
        for ty in range(-(-lod_h // 512)):
            for tx in range(-(-lod_w // 512)):
                g = li.tile_geometry(W, Hh, lx, ly, tx, ty)
                left = float(g["origin_x"]) * float(W) / float(lod_w)
                top = float(g["origin_y"]) * float(Hh) / float(lod_h)
                cw = float(g["origin_x"] + g["width"]) * float(W) / float(lod_w) - left
                chh = float(g["origin_y"] + g["height"]) * float(Hh) / float(lod_h) - top
                reqs.append((0, 0, RGBA, g["width"], g["height"], (left, top, cw, chh)))
                t = tm.get_spectrogram_tile(0, 0, lx, ly, tx, ty)
                want.append(np.frombuffer(t[40:], np.uint8).reshape(g["height"], g["width"], 4))
        figs, _ = tm.render_figures(reqs)
        for r, f, w_ in zip(reqs, figs, want):
            assert np.array_equal(f, w_), (lx, ly, r)
            n += 1
    tm.set_lod_source(False)
    assert n >= 30


def test_figure_across_the_piece_boundary(small):
    """the smallest RGBA figure of width 2048 above TH_FIGURE_PIECE_BYTES (1025 rows: one row into the second piece), and the widest
    figure there is, cut after 256 of its 300 rows"""
    tm, imgs = small
    assert 2048 * 1024 * 4 == api.FIGURE_PIECE_BYTES
    box = (20.25, 30.5, 40.0, 20.0)
    want = R.resample(imgs[0], box, 2048, 1025)[::-1]
    rgba, _ = tm.render_figure(0, 0, RGBA, 2048, 1025, box)
    assert np.array_equal(rgba, CMAP[R.colour_index(want, 258)])
    grey, _ = tm.render_figure(0, 0, GREY16, 2048, 1025, box)
    assert np.array_equal(grey, want)
    # 16384 x 300 GREY16 = 9.4 MiB of output
    box = (0.0, 0.0, 300.0, 129.0)
    grey, _ = tm.render_figure(0, 0, GREY16, 16384, 300, box)
    assert np.array_equal(grey, R.resample(imgs[0], box, 16384, 300)[::-1])


def test_band_cut_by_the_intermediate_bound(big):
    """1300 source rows x 8192 columns x 2 bytes = 20.3 MiB of intermediate for all rows at once: beyond TH_FIGURE_TMP_BYTES, so the
    40 output rows (640 KiB) are cut into bands that recompute the source rows they share"""
    tm, img = big
    assert 1300 * 8192 * 2 > api.FIGURE_TMP_BYTES
    box = (100.0, 0.0, 2048.0, 1300.0)
    grey, _ = tm.render_figure(0, 0, GREY16, 8192, 40, box)
    assert np.array_equal(grey, R.resample(img, box, 8192, 40)[::-1])


def _batch(imgs):
    return [
        (0, 0, RGBA, 64, 48, (10.0, 5.0, 128.0, 96.0)),
        (1, 0, GREY16, 64, 7, (10.0, 2.5, 128.0, 100.0)),      # shares its x axis with nobody (another image width)
        (0, 0, GREY16, 64, 31, (10.0, 7.0, 128.0, 31.0)),      # shares its x axis with request 0
        (2, 0, RGBA, 3, 5, (0.0, 0.0, 77.0, 129.0)),           # a 12-byte row: records and rows off the 16-byte grid
        (0, 0, RGBA, 1, 1, (1.0, 1.0, 2.0, 2.0)),
        (1, 0, RGBA, 257, 129, (0.0, 0.0, 1025.0, 129.0)),
    ]


def test_batch_equals_single_calls(ctx, small):
    tm, imgs = small
    reqs = _batch(imgs)
    singles = [tm.render_figure(*r)[0] for r in reqs]
    for r, s in zip(reqs, singles):
        assert np.array_equal(s, R.figure(imgs[r[0]], r[5], r[3], r[4], r[2], CMAP)), r
    figs, infos = tm.render_figures(reqs)
    at = 0
    for r, f, s, o in zip(reqs, figs, singles, infos):
        assert np.array_equal(f, s), r
        assert o["offset"] == at and o["offset"] % 64 == 0 and o["bytes"] == s.nbytes
        at = (at + s.nbytes + 63) // 64 * 64
    assert len({o["spectrogram_revision"] for o in infos}) == 1 and infos[0]["spectrogram_revision"] == tm.revisions()[1]
    # pinned memory, and the bytes between the records are left alone in either kind of buffer
    total = infos[-1]["offset"] + infos[-1]["bytes"]
    pin = C.c_void_p()
    _ffi.check(_ffi.lib.th_host_alloc(ctx.handle, total + 64, C.byref(pin)))
    try:
        raw = np.frombuffer((C.c_uint8 * (total + 64)).from_address(pin.value), np.uint8)
        page = np.empty(total + 64, np.uint8)
        for buf, where in ((raw, pin), (page, page)):
            buf[:] = 0xA5
            figs2, _ = tm.render_figures(reqs, out=where, cap=total + 64)
            for f, s in zip(figs2, singles):
                assert np.array_equal(f, s)
            used = np.zeros(total + 64, bool)
            for o in infos:
                used[o["offset"]: o["offset"] + o["bytes"]] = True
            assert (buf[~used] == 0xA5).all()
    finally:
        _ffi.check(_ffi.lib.th_host_free(ctx.handle, pin))


def _raw_call(tm, reqs, out, cap):
    arr = (_ffi.FigureRequest * len(reqs))(*[api._figure_request(r) for r in reqs])
    info = (_ffi.FigureInfo * len(reqs))()
    need = C.c_size_t(12345)
    rc = _ffi.lib.th_tm_render_figures(tm.handle, arr, len(reqs), out, cap, info, C.byref(need))
    return rc, need.value, info


def test_size_query_and_error_codes(small):
    tm, imgs = small
    ok = (0, 0, RGBA, 8, 4, (0.0, 0.0, 16.0, 8.0))
    rc, need, info = _raw_call(tm, [ok, ok], None, 0)
    assert rc == _ffi.ERR_BUFFER_TOO_SMALL and need == 256 and (info[1].offset, info[1].bytes) == (128, 128)
    buf = np.full(1024, 0x5A, np.uint8)
    rc, need, _ = _raw_call(tm, [ok, ok], buf.ctypes.data, 255)
    assert rc == _ffi.ERR_BUFFER_TOO_SMALL and need == 256 and (buf == 0x5A).all()
    bad = [
        ((99, 0, RGBA, 8, 4, ok[5]), _ffi.ERR_NOT_FOUND),
        ((0, 1, RGBA, 8, 4, ok[5]), _ffi.ERR_INVALID_ARG),
        ((0, 0, 2, 8, 4, ok[5]), _ffi.ERR_INVALID_ARG),
        ((0, 0, RGBA, 0, 4, ok[5]), _ffi.ERR_INVALID_ARG),
        ((0, 0, RGBA, 8, 16385, ok[5]), _ffi.ERR_INVALID_ARG),
        ((0, 0, RGBA, 8, 4, (0.0, 0.0, 0.0, 8.0)), _ffi.ERR_INVALID_ARG),
        ((0, 0, RGBA, 8, 4, (0.0, 0.0, -1.0, 8.0)), _ffi.ERR_INVALID_ARG),
        ((0, 0, RGBA, 8, 4, (0.0, 0.0, INF, 8.0)), _ffi.ERR_INVALID_ARG),
        ((0, 0, RGBA, 8, 4, (float("nan"), 0.0, 4.0, 8.0)), _ffi.ERR_INVALID_ARG),
        ((0, 0, RGBA, 8, 4, (-0.5, 0.0, 4.0, 8.0)), _ffi.ERR_INVALID_ARG),
        ((0, 0, RGBA, 8, 4, (0.0, 0.0, 300.5, 8.0)), _ffi.ERR_INVALID_ARG),
        ((0, 0, RGBA, 8, 4, (0.0, 100.0, 4.0, 29.5)), _ffi.ERR_INVALID_ARG),
    ]
    for r, code in bad:
        for reqs in ([r], [ok, r, (98, 0, RGBA, 8, 4, ok[5])]):   # (the first faulty request decides)
            rc, _, _ = _raw_call(tm, reqs, buf.ctypes.data, buf.size)
            assert rc == code, (r, rc)
            assert (buf == 0x5A).all(), r
    # the whole 1025-pixel axis on one output column of 16384 rows: (6 x 1025 + 4) taps x 8 bytes x 16384 > 256 MB by plan_lod_tile's rule
    rc, _, _ = _raw_call(tm, [ok, (1, 0, GREY16, 1, 16384, (0.0, 0.0, 1025.0, 129.0))], buf.ctypes.data, buf.size)
    assert rc == _ffi.ERR_UNSUPPORTED and (buf == 0x5A).all()


@pytest.mark.parametrize("n_colors", [2, 256, 1025])
def test_colormap_sizes(ctx, n_colors):
    """(a manager of its own: th_tm_set_colormap re-makes the images, so the colormap is set before the pixels are placed)"""
    cm = _cmap(n_colors)
    img = li._hash_image(65, 200, 30 + n_colors, full_range=True)
    tm = tm_with_images(ctx, [img], cmap=cm)
    box = (5.5, 3.0, 150.0, 60.0)
    rgba, _ = tm.render_figure(0, 0, RGBA, 97, 33, box)
    assert np.array_equal(rgba, R.figure(img, box, 97, 33, R.RGBA, cm))
    assert len(np.unique(rgba.reshape(-1, 4), axis=0)) >= min(n_colors, 200) // 2 + 1
    tm.close()


@pytest.mark.parametrize("devices", [(0,), (0, 0)], ids=["tmg0", "tmg00"])
def test_multi_manager_returns_the_same_bytes(ctx, devices):
    """th_tmg over one slot and over two slots on one card == th_tm: bytes and infos (the tracks land on different slots)"""
    tracks = [(3, 48000, np.stack([synth_track(41, 48000, 30000), synth_track(42, 48000, 30000)])),
              (5, 44100, synth_track(43, 44100, 21000)[None]), (8, 48000, synth_track(44, 48000, 12345)[None])]
    tm, g = ta.TrackManager(ctx), ta.MultiTrackManager(list(devices))
    try:
        for m in (tm, g):
            m.set_setting(1024 / 48, 4, 1, ta.MEL)
            m.set_colormap(CMAP.tobytes())
            m.add_tracks(tracks)
            m.apply_track_list_changes()
        if len(devices) > 1:
            assert len({g.device_of(t[0]) for t in tracks}) == 2
        reqs = []
        for k, (tid, ch) in enumerate([(3, 1), (5, 0), (8, 0), (3, 0), (5, 0)]):
            box = tm.figure_box(tid, ch, 0.05 * k, 0.2 + 0.05 * k, 100.0 * k, 6000.0 + 1000.0 * k)
            assert g.figure_box(tid, ch, 0.05 * k, 0.2 + 0.05 * k, 100.0 * k, 6000.0 + 1000.0 * k) == box
            reqs.append((tid, ch, (RGBA, GREY16)[k & 1], 50 + 13 * k, 40 - 7 * k, box))
        want, winfos = tm.render_figures(reqs)
        for r, w_ in zip(reqs, want):
            assert np.array_equal(w_, R.figure(tm.img(r[0], r[1]), r[5], r[3], r[4], r[2], CMAP)), r
        got, infos = g.render_figures(reqs)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        strip = lambda o: {k: v for k, v in o.items() if k != "spectrogram_revision"}  # noqa: E731
        assert [strip(o) for o in infos] == [strip(o) for o in winfos]
        assert all(o["spectrogram_revision"] == g.revisions()[1] for o in infos)
        one, _ = g.render_figure(*reqs[1])
        assert np.array_equal(one, want[1])
        with pytest.raises(ta.ThError) as e:
            g.render_figures(reqs + [(77, 0, RGBA, 4, 4, (0.0, 0.0, 1.0, 1.0))])
        assert e.value.code == _ffi.ERR_NOT_FOUND
    finally:
        g.close()
        tm.close()


def test_eight_reader_threads(small):
    tm, imgs = small
    reqs = _batch(imgs)
    want, _ = tm.render_figures(reqs)
    errs = []

    def work(k):
        try:
            for it in range(3):
                sub = reqs[k % 3:] + reqs[:k % 3]
                got, _ = tm.render_figures(sub)
                ref = want[k % 3:] + want[:k % 3]
                assert all(np.array_equal(a, b) for a, b in zip(got, ref))
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs


@pytest.mark.parametrize("scale", [ta.LINEAR, ta.MEL], ids=["linear", "mel"])
def test_real_audio_box_and_revisions(ctx, scale):
    """th_tm_figure_box + render on the image of real audio == the definition on copy_img; the dB range moves the figure and the
    revision; a removed track is NOT_FOUND"""
    tm = ta.TrackManager(ctx)
    tm.set_setting(40.0, 4, 1, scale)
    tm.set_colormap(CMAP.tobytes())
    sr, n = 44100, 44100 * 3 + 17
    tm.add_tracks([(4, sr, np.stack([synth_track(31, sr, n), synth_track(32, sr, n)])), (9, 48000, synth_track(33, 48000, 48000)[None])])
    tm.apply_track_list_changes()
    img = tm.img(4, 1)
    spec_h = tm.spec(4, 1).shape[1]
    assert img.shape[0] > spec_h   # (below max_sr: the image is higher than the spectrogram)
    box = tm.figure_box(4, 1, 0.4, 2.1, 200.0, 8000.0)
    assert box == R.box(0.4, 2.1, 200.0, 8000.0, sr, n, img.shape[1], spec_h, img.shape[0], scale == ta.MEL)
    assert box == ta.figure_box(0.4, 2.1, 200.0, 8000.0, sr, n, img.shape[1], spec_h, img.shape[0], scale)
    fig, info = tm.render_figure(4, 1, RGBA, 301, 120, box)
    assert np.array_equal(fig, R.figure(img, box, 301, 120, R.RGBA, CMAP))
    whole = tm.figure_box(4, 1)
    assert whole == (0.0, 0.0, float(img.shape[1]), float(img.shape[0]))
    grey, _ = tm.render_figure(4, 1, GREY16, 200, 90, whole)
    assert np.array_equal(grey, R.figure(img, whole, 200, 90, R.GREY16))
    rev = tm.revisions()[1]
    assert info["spectrogram_revision"] == rev
    tm.set_dB_range(50.0)
    fig2, info2 = tm.render_figure(4, 1, RGBA, 301, 120, box)
    assert info2["spectrogram_revision"] == tm.revisions()[1] != rev and not np.array_equal(fig2, fig)
    assert np.array_equal(fig2, R.figure(tm.img(4, 1), box, 301, 120, R.RGBA, CMAP))
    tm.remove_track(4)
    tm.apply_track_list_changes()
    with pytest.raises(ta.ThError) as e:
        tm.render_figure(4, 1, RGBA, 301, 120, box)
    assert e.value.code == _ffi.ERR_NOT_FOUND
    with pytest.raises(ta.ThError) as e:
        tm.figure_box(4, 1)
    assert e.value.code == _ffi.ERR_NOT_FOUND
    tm.close()
