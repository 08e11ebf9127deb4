"""The device tables th_ctx keeps for the last spec -> img, raster and quantise + raster batch (context.h KeyedTables): an identical
batch launches on them as they are, a different one replaces them, a refused one leaves nothing behind that a later call could
mistake for its own.  Every successful call is compared with the oracle bit for bit.  And the single spectrogram tile of a manager
that never had a colormap set, against the batched fetch."""
import numpy as np
import pytest

import thesia_amd as ta
from oracle import oracle as orc
from thesia_amd import _ffi

pytestmark = pytest.mark.gpu

LO, HI, CM = -100.0, -3.5, 258


@pytest.fixture(scope="module")
def ctx():
    with ta.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def cmap():
    return bytes(np.random.default_rng(5).integers(0, 256, CM * 4, dtype=np.uint8))


def _spec(seed, T, H):
    rng = np.random.default_rng(seed)
    s = (rng.random((T, H), dtype=np.float32) * 130.0 - 120.0).astype(np.float32)
    s.reshape(-1)[rng.integers(0, s.size, max(1, s.size // 50))] = np.float32("-inf")
    return s


def _reuse_sequence(run, A, B, bad):
    """batch A; A again (a key hit); B (another number of descriptors, more blocks); a refused batch; A again"""
    run(A)
    run(A)
    run(B)
    with pytest.raises(_ffi.ThError) as e:
        run(bad, check=False)
    assert e.value.code == _ffi.ERR_INVALID_ARG
    run(A)


# 70 frames x 33 rows and 5 x 130: the 64-frame and the 128-row tile of the quantiser crossed once each
SHAPES = [(70, 33), (5, 130)]


def test_spec_to_img_batch_tables_are_reused_and_replaced(ctx):
    specs = [_spec(i, T, H) for i, (T, H) in enumerate(SHAPES)]
    want = [orc.convert_spectrogram_to_img(s, (0, s.shape[1]), (LO, HI), CM) for s in specs]
    d_spec = [ctx.to_device(s) for s in specs]
    d_img = [ctx.alloc(s.size * 2) for s in specs]
    desc = [_ffi.ImgDesc(d_spec[i].ptr, d_img[i].ptr, T, H, 0, H, 0, 0) for i, (T, H) in enumerate(SHAPES)]

    def run(which, check=True):
        for b in d_img:
            b.upload(np.full(b.nbytes, 0xAB, np.uint8))
        ctx.spec_to_img_batch([desc[i] if i >= 0 else _ffi.ImgDesc(d_spec[0].ptr, d_img[0].ptr, 70, 33, 5, 4, 0, 0) for i in which], LO, HI, CM)
        if check:
            for i in which:
                T, H = SHAPES[i]
                assert np.array_equal(d_img[i].download((H, T), np.uint16), want[i]), (which, i)

    _reuse_sequence(run, [1], [0, 1], [1, -1])   # (-1: i_end < i_start)
    for b in d_spec + d_img:
        b.free()


def test_raster_tiles_tables_are_reused_and_replaced(ctx, cmap):
    W, H = 520, 9
    img = np.random.default_rng(11).integers(0, 65536, (H, W), dtype=np.uint16)
    d_img, d_cmap = ctx.to_device(img), ctx.to_device(np.frombuffer(cmap, np.uint8))
    # widths 5 and 513 at an odd origin
    rects = [(3, 1, 5, 7), (7, 1, 513, 8)]
    want = [np.frombuffer(orc.encode_spectrogram_tile(img[oy:oy + h, ox:ox + w], cmap, 1, 0, 0, 0, 0)[40:], np.uint8) for ox, oy, w, h in rects]
    d_out = [ctx.alloc(w * h * 4) for _, _, w, h in rects]
    desc = [_ffi.RasterDesc(d_img.ptr, d_out[i].ptr, W, H, ox, oy, w, h, 0, 0) for i, (ox, oy, w, h) in enumerate(rects)]
    outside = _ffi.RasterDesc(d_img.ptr, d_out[0].ptr, W, H, 516, 1, 5, 7, 0, 0)   # 516 + 5 > 520

    def run(which, check=True):
        for b in d_out:
            b.upload(np.full(b.nbytes, 0xAB, np.uint8))
        ctx.raster_tiles([desc[i] if i >= 0 else outside for i in which], d_cmap.ptr, CM)
        if check:
            for i in which:
                assert np.array_equal(d_out[i].download((want[i].size,), np.uint8), want[i]), (which, i)

    _reuse_sequence(run, [0], [0, 1], [0, -1])
    for b in [d_img, d_cmap] + d_out:
        b.free()


def test_fused_tables_are_reused_and_replaced(ctx, cmap):
    # 513 frames x 33 rows: two tile columns, two bands of 32 rows; the second image is the smaller one of the quantiser's case
    shapes = [(513, 33), (70, 33)]
    specs = [_spec(20 + i, T, H) for i, (T, H) in enumerate(shapes)]
    want_img = [orc.convert_spectrogram_to_img(s, (0, s.shape[1]), (LO, HI), CM) for s in specs]
    d_spec = [ctx.to_device(s) for s in specs]
    d_img = [ctx.alloc(s.size * 2) for s in specs]
    d_cmap = ctx.to_device(np.frombuffer(cmap, np.uint8))
    geoms = [[(tx, ta.spectrogram_tile_geometry(T, H, 0, 0, tx, 0)) for tx in range(-(-T // 512))] for T, H in shapes]
    d_tile = [[ctx.alloc(g.width * g.height * 4) for _, g in gs] for gs in geoms]
    item = [(_ffi.ImgDesc(d_spec[i].ptr, d_img[i].ptr, T, H, 0, H, 0, 0), [b.ptr for b in d_tile[i]]) for i, (T, H) in enumerate(shapes)]

    def run(which, check=True):
        for b in d_img + [t for ts in d_tile for t in ts]:
            b.upload(np.full(b.nbytes, 0xAB, np.uint8))
        descs = ctx.make_img_tiles_descs([item[i] for i in which if i >= 0])
        if -1 in which:
            descs[len(descs) - 1].img.i_start = 40   # i_end < i_start, on the last descriptor
        ctx.spec_to_img_raster_batch(descs, d_cmap.ptr, CM, min_dB=LO, max_dB=HI)
        if check:
            for i in which:
                T, H = shapes[i]
                assert np.array_equal(d_img[i].download((H, T), np.uint16), want_img[i]), (which, i)
                for (tx, g), b in zip(geoms[i], d_tile[i]):
                    want = orc.encode_spectrogram_tile(want_img[i], cmap, 1, 0, 0, tx, 0)[40:]
                    assert b.download((g.width * g.height * 4,), np.uint8).tobytes() == want, (which, i, tx)

    _reuse_sequence(run, [1], [0, 1], [1, 0, -1])
    for b in d_spec + d_img + [d_cmap] + [t for ts in d_tile for t in ts]:
        b.free()


def test_single_tile_without_a_colormap_equals_the_batched_fetch(ctx):
    """th_tm_get_spectrogram_tile on a manager that never had th_tm_set_colormap: the default map is uploaded on the way, level
    (0, 0) and a LOD level, from the mip pyramid and resampled per request, each byte-equal to the same request through
    th_tm_get_spectrogram_tiles; a short buffer gets ERR_BUFFER_TOO_SMALL and the length it needs.
    One image of 600 frames x 42 rows: two tile columns.  (600 x 40 was the shape asked for; no setting of the manager gives a 40-row
    image — mel rows at 48 kHz go 20, 42, 86 — and th_tm_put_img takes the resident shape only, so this is the nearest one, n_fft 256.)"""
    import ctypes as C
    n = 28752   # 600 frames at hop 48, window 192
    x = (0.3 * np.sin(2 * np.pi * 1500.0 * np.arange(n) / 48000) + 1e-3 * np.random.default_rng(3).uniform(-1, 1, n)).astype(np.float32)
    for per_request in (False, True):
        tm = ta.TrackManager(ctx)   # (a fresh one per route: the first tile request of each finds no colormap)
        tm.set_setting(4.0, 4, 1, ta.MEL)
        tm.add_tracks([(1, 48000, x[None])])
        tm.apply_track_list_changes()
        assert tm.img(1, 0).shape == (42, 600)
        if per_request:
            tm.set_lod_source(per_request=True)
        first_level = (1, 1) if per_request else (0, 0)   # the first request of a manager, on either path, has no colormap yet
        reqs = [first_level + (0, 0)] + [(lx, ly, tx, 0) for lx, ly in ((0, 0), (1, 1)) for tx in (0, 1, 2)]
        single = [tm.get_spectrogram_tile(1, 0, *r) for r in reqs]
        batched = tm.get_spectrogram_tiles([(1, 0) + r for r in reqs])
        assert single == batched, per_request
        g0 = ta.spectrogram_tile_geometry(600, 42, 0, 0, 0, 0)
        assert len(single[1]) == 40 + g0.width * g0.height * 4 and len(single[3]) == 40   # (tile 2 lies past the image: a header alone)
        out = np.empty(100, np.uint8)
        need = C.c_size_t()
        for lx, ly in ((0, 0), (1, 1)):
            rc = _ffi.lib.th_tm_get_spectrogram_tile(tm.handle, 1, 0, lx, ly, 0, 0, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size, C.byref(need))
            assert rc == _ffi.ERR_BUFFER_TOO_SMALL and need.value == len(single[1 if (lx, ly) == (0, 0) else 4]), (per_request, lx, ly)
        tm.close()
