"""The host side of the image, raster and waveform batch entries, on the CPU: the planners of thesia_amd/csrc/batch_plan.h are compiled
into the emulator library as api.hip calls them.  Nothing is allocated on a device, so the launch limits, the reciprocals the raster
kernel divides with and the tap windows of a LOD tile are checked here.  The tables of the fixed batches are pinned to
tests/golden/batch_plan_cases.json, recorded from the bodies the entries had before the planners were split off.

The block-count limits (2^27 blocks of the image, fused and raster launches, 2^31 of the waveform launch) are reached from both sides in
test_block_count_limits: a batch at the limit builds a block table of half a gigabyte (the waveform one takes 2^23 descriptors), so
those cases read back the plan's head alone; the test peaks near 2 GB for a few seconds.  The 2^31 tile pointers of plan_fused share
their condition and message with its block limit and cannot be passed on their own: an image has ceil(out_h / 512) tile rows and
ceil(out_h / 32) bands, so a batch never has more pointers than blocks, and the block limit is 2^27."""
import ctypes as C
import hashlib
import json
import os
import struct

import numpy as np
import pytest

from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "batch_plan_cases.json")
EMU = os.path.join(HERE, "emu", "_build", "libemu_stft.so")
U64 = np.uint64
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -2
IMG_TILE_T, IMG_TILE_F, FUSED_FB, RASTER_QPB, PYR_MAX_LEVELS = 64, 128, 32, 1024, 40
A = 0x7F0000000000   # a 16-byte aligned "device" address; the planners never read through one


def load(path=EMU):
    lib = C.CDLL(path)
    p64 = C.POINTER(C.c_uint64)
    lib.emu_blob.restype = C.c_uint64
    lib.emu_blob.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    lib.emu_blob_free.argtypes = [C.c_void_p]
    for name, args in (("emu_check_img", [p64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64]), ("emu_plan_img", [p64, C.c_uint64]),
                       ("emu_plan_fused", [p64, C.c_uint64, p64, C.c_uint32, C.c_uint32, C.c_uint64]), ("emu_plan_raster", [p64, C.c_uint64]),
                       ("emu_plan_wave_tiles", [p64, C.c_uint64]), ("emu_plan_stats", [p64, C.c_uint64]),
                       ("emu_plan_pyramid", [p64, C.c_uint64, C.c_uint64]), ("emu_plan_lod_tile", [C.c_uint64, C.c_uint64] + [C.c_uint32] * 4)):
        getattr(lib, name).restype = C.c_void_p
        getattr(lib, name).argtypes = args
    lib.emu_spectrogram_tile_header.restype = lib.emu_waveform_tile_header.restype = C.c_uint64
    lib.emu_spectrogram_tile_header.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64] + [C.c_uint32] * 4
    lib.emu_waveform_tile_header.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    return lib


@pytest.fixture(scope="module")
def emu():
    return load()


def _blobs(lib, handle, dtypes):
    assert handle
    try:
        out = []
        for i, dt in enumerate(dtypes):
            n = lib.emu_blob(handle, i, None, 0)
            assert n != 2 ** 64 - 1 and n % np.dtype(dt).itemsize == 0
            a = np.empty(n // np.dtype(dt).itemsize, dt)
            assert lib.emu_blob(handle, i, a.ctypes.data_as(C.c_void_p), a.nbytes) == n
            out.append(a)
        return out
    finally:
        lib.emu_blob_free(handle)


def _rows(rows, width):
    a = np.array([[int(v) & (2 ** 64 - 1) for v in r] for r in rows], U64).reshape(-1, width)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def _head(b, names):
    d = dict(zip(["err"] + names, (int(v) for v in b[0].view(np.int64))))
    d["text"] = b[1].tobytes().decode()
    return d


def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def check_img(lib, rows, lo=-100.0, hi=0.0, d_range=0):
    a, p = _rows(rows, 8)
    return _head(_blobs(lib, lib.emu_check_img(p, len(a), _f32_bits(lo), _f32_bits(hi), d_range), [U64, np.uint8]), ["all_neg_inf"])


def plan_img(lib, rows):
    a, p = _rows(rows, 8)
    b = _blobs(lib, lib.emu_plan_img(p, len(a)), [U64, np.uint8, U64, np.uint32])
    return dict(_head(b, ["n_blocks"]), jobs=b[2].reshape(-1, 10).astype(np.int64), block_job=b[3].astype(np.int64))


def plan_fused(lib, rows, tiles, lo=-100.0, hi=0.0, d_range=0):
    a, p = _rows(rows, 11)
    t = np.array(list(tiles) + [0], U64)
    b = _blobs(lib, lib.emu_plan_fused(p, len(a), t.ctypes.data_as(C.POINTER(C.c_uint64)), _f32_bits(lo), _f32_bits(hi), d_range),
               [U64, np.uint8, np.uint8, U64, np.uint32, U64])
    return dict(_head(b, ["n_blocks", "desc_bytes"]), key=b[2], jobs=b[3].reshape(-1, 13).astype(np.int64), block_job=b[4].astype(np.int64),
                ptrs=b[5].astype(np.int64))


def plan_raster(lib, rows):
    a, p = _rows(rows, 10)
    b = _blobs(lib, lib.emu_plan_raster(p, len(a)), [U64, np.uint8, U64, np.uint32])
    return dict(_head(b, ["n_blocks"]), jobs=b[2].reshape(-1, 13).astype(np.int64), block_job=b[3].astype(np.int64))


def plan_wave(lib, rows):
    a, p = _rows(rows, 6)
    b = _blobs(lib, lib.emu_plan_wave_tiles(p, len(a)), [U64, np.uint8, U64, np.uint32])
    return dict(_head(b, ["n_blocks"]), jobs=b[2].reshape(-1, 6).astype(np.int64), start=b[3].astype(np.int64))


def plan_stats(lib, rows):
    a, p = _rows(rows, 2)
    b = _blobs(lib, lib.emu_plan_stats(p, len(a)), [U64, np.uint8, U64])
    return dict(_head(b, ["max_samples"]), jobs=b[2].reshape(-1, 3).astype(np.int64))


def plan_pyramid(lib, rows, sums=A):
    a, p = _rows(rows, 5)
    b = _blobs(lib, lib.emu_plan_pyramid(p, len(a), sums), [U64, np.uint8, U64, U64])
    return dict(_head(b, ["sums_floats", "max_samples", "max_levels", "launch"]), jobs=b[2].reshape(-1, 47).astype(np.int64),
                sums_at=b[3].astype(np.int64))


LOD_HEAD = ["y_lo", "y_hi", "n_rows", "dw", "dh", "y_at", "taps_x", "taps_y", "lod_at", "scratch_bytes", "origin_x", "origin_y", "lod_w", "lod_h"]


def plan_lod(lib, W, H, lx, ly, tx, ty):
    h = lib.emu_plan_lod_tile(W, H, lx, ly, tx, ty)
    if not h:
        return None   # an empty tile
    b = _blobs(lib, h, [U64, np.uint8, np.float64, np.uint8])
    return dict(_head(b, LOD_HEAD), box=b[2], blob=b[3])


def lod_axis(blob, at, n_out, taps):
    """one axis of the blob, as the entry's axis_dev reads it: start i32, count i32, wsum f64, w f64 [n_out][taps]"""
    raw = blob[at:].tobytes()
    return (np.frombuffer(raw, np.int32, n_out, 0), np.frombuffer(raw, np.int32, n_out, 4 * n_out), np.frombuffer(raw, np.float64, n_out, 8 * n_out),
            np.frombuffer(raw, np.float64, n_out * taps, 16 * n_out).reshape(n_out, taps))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(lib, case):
    """a batch through its entry's planner(s), as the entry runs them, in a form JSON holds"""
    e = case["entry"]
    flat = lambda a: [int(v) for v in np.asarray(a).reshape(-1)]  # noqa: E731
    if e == "img":
        c = check_img(lib, case["rows"], case.get("lo", -100.0), case.get("hi", 0.0), case.get("d_range", 0))
        if c["err"]:
            return dict(check=c)
        p = plan_img(lib, case["rows"])
        return dict(check=c, err=p["err"], text=p["text"], n_blocks=p["n_blocks"], jobs=flat(p["jobs"]), block_job=_sha(p["block_job"]))
    if e == "fused":
        p = plan_fused(lib, case["rows"], case["tiles"], case.get("lo", -100.0), case.get("hi", 0.0), case.get("d_range", 0))
        if p["err"]:
            return dict(err=p["err"], text=p["text"])
        return dict(err=0, text="", n_blocks=p["n_blocks"], jobs=flat(p["jobs"]), block_job=_sha(p["block_job"]), ptrs=flat(p["ptrs"]))
    if e == "raster":
        p = plan_raster(lib, case["rows"])
        return dict(err=p["err"], text=p["text"], n_blocks=p["n_blocks"], jobs=flat(p["jobs"]), block_job=_sha(p["block_job"]))
    if e == "wave":
        p = plan_wave(lib, case["rows"])
        return dict(err=p["err"], text=p["text"], n_blocks=p["n_blocks"], jobs=flat(p["jobs"]), start=flat(p["start"]))
    if e == "stats":
        p = plan_stats(lib, case["rows"])
        return dict(err=p["err"], text=p["text"], max_samples=p["max_samples"], jobs=flat(p["jobs"]))
    if e == "pyramid":
        p = plan_pyramid(lib, case["rows"])
        if p["err"] or not p["launch"]:
            return dict(err=p["err"], text=p["text"], launch=p["launch"])
        return dict(err=0, text="", launch=1, sums_floats=p["sums_floats"], max_samples=p["max_samples"], max_levels=p["max_levels"],
                    jobs=_sha(p["jobs"]), first_job=flat(p["jobs"][0]), sums_at=flat(p["sums_at"]))
    if e == "lod":
        p = plan_lod(lib, *case["args"])
        if p is None or p["err"]:
            return dict(err=None if p is None else p["err"], text="" if p is None else p["text"])
        return dict({k: p[k] for k in ["err", "text"] + LOD_HEAD}, blob=_sha(p["blob"]))
    raise AssertionError(e)


def img_row(T, H, i0=0, i1=None, sp=0, ip=0, spec=A, img=A + (1 << 32)):
    return [spec, img, T, H, i0, H if i1 is None else i1, sp, ip]


def fused_rows(imgs):
    """imgs: img_row rows -> (rows of 11 with the right tile counts, the tile pointers)"""
    rows, tiles = [], []
    for r in imgs:
        out_h, T = r[5] - r[4], r[2]
        n_tx, n_ty = (-(-T // 512), -(-out_h // 512)) if out_h > 0 and T else (0, 0)
        rows.append(list(r) + [len(tiles), n_tx, n_ty])
        tiles += [A + (2 << 32) + 4 * (len(tiles) + k) * 0x41000 for k in range(n_tx * n_ty)]
    return rows, tiles


def raster_row(W, H, ox, oy, w, h, pitch=0, img=A, rgba=A + (3 << 32)):
    return [img, rgba, W, H, ox, oy, w, h, pitch, 0]


def random_case(entry, rng):
    n = int(rng.integers(1, 6))
    r = lambda lo, hi: int(rng.integers(lo, hi))  # noqa: E731
    if entry in ("img", "fused"):
        imgs = []
        for _ in range(n):
            T, H = r(0, 1400), r(1, 1100)
            i0 = r(0, H)
            i1 = r(i0, H + 40)
            row = img_row(T, H, i0, i1, r(0, 2) * (H + r(0, 70)), r(0, 2) * (T + r(0, 70)), A + 4 * r(0, 64), A + (1 << 32) + 2 * r(0, 64))
            if r(0, 25) == 0:
                row[r(2, 8)] = r(0, 3) << 31   # a bad size, now and then
            imgs.append(row)
        if entry == "img":
            return dict(entry="img", rows=imgs)
        rows, tiles = fused_rows(imgs)
        if tiles and r(0, 6) == 0:
            tiles[r(0, len(tiles))] = 0                 # NULL: a tile that is skipped
        if tiles and r(0, 20) == 0:
            tiles[r(0, len(tiles))] += 2                # a misaligned one
        if r(0, 20) == 0:
            rows[r(0, n)][9] += 1                       # a wrong tile count
        return dict(entry="fused", rows=rows, tiles=tiles)
    if entry == "raster":
        rows = []
        for _ in range(n):
            W, H = r(1, 3000), r(1, 1200)
            w, h = r(0, min(W, 700) + 1), r(0, min(H, 700) + 1)
            row = raster_row(W, H, r(0, W - w + 1), r(0, H - h + 1), w, h, r(0, 2) * (W + r(0, 64)), A + 2 * r(0, 16), A + (3 << 32) + 4 * r(0, 16))
            if r(0, 25) == 0:
                row[4] = W          # outside
            rows.append(row)
        return dict(entry="raster", rows=rows)
    if entry == "wave":
        rows = []
        for _ in range(n):
            level, bins = r(0, 41 if r(0, 10) == 0 else 20), r(0, 1025)
            ns = r(1, 1 << 34)
            start = r(0, ns)
            if bins and r(0, 4):   # most of them valid
                start = min(start, max(0, ns - 1 - (bins - 1) * (1 << min(level, 39))))
                if start + (bins - 1) * (1 << min(level, 39)) >= ns:
                    bins = 1
            rows.append([A + 4 * r(0, 8), A + (4 << 32) + 4 * r(0, 8), ns, start, level, bins])
        return dict(entry="wave", rows=rows)
    if entry == "stats":
        return dict(entry="stats", rows=[[A + 4 * r(0, 8), r(0, 1 << 41) if r(0, 20) == 0 else r(0, 1 << 30)] for _ in range(n)])
    if entry == "pyramid":
        return dict(entry="pyramid", rows=[[A + 4 * r(0, 8), A + (5 << 32) + 4 * r(0, 64), r(0, 1 << r(1, 36)), r(0, 42), r(0, 3 if r(0, 15) else 4)]
                                           for _ in range(n)])
    if entry == "lod":
        lx, ly = r(0, 6), r(0, 5)
        return dict(entry="lod", args=[r(1, 4000), r(1, 1200), lx or (ly == 0), ly, r(0, 3), r(0, 2)])   # (level (0, 0) is no LOD tile)
    raise AssertionError(entry)


ENTRIES = ["img", "fused", "raster", "wave", "stats", "pyramid", "lod"]


def fixed_cases():
    f1 = fused_rows([img_row(1030, 600, 5, 521, 608, 1088), img_row(513, 70), img_row(0, 9), img_row(37, 9, 4, 4)])
    f2 = fused_rows([img_row(2813, 1025)])
    f2[1][3] = 0
    return [
        dict(entry="img", rows=[img_row(70, 33), img_row(5, 130), img_row(1030, 600, 5, 521, 608, 1088), img_row(0, 4), img_row(9, 7, 3, 3)]),
        dict(entry="img", rows=[img_row(2813, 1025, 0, 1025, 1028, 2816)], lo=float("-inf"), hi=float("-inf")),
        dict(entry="img", rows=[img_row(64, 128), img_row(65, 129)], d_range=A + 4),
        dict(entry="img", rows=[img_row(64, 128), img_row(65, 129, spec=A + 2)]),
        dict(entry="img", rows=[img_row(64, 128, 9, 8), img_row(1 << 31, 4)]),
        dict(entry="fused", rows=f1[0], tiles=f1[1]),
        dict(entry="fused", rows=f2[0], tiles=f2[1], d_range=A),
        dict(entry="raster", rows=[raster_row(1100, 700, 508, 0, 516, 516, 1152), raster_row(1100, 700, 1020, 508, 80, 192), raster_row(9, 9, 3, 1, 5, 7, 0, A + 2, A + (3 << 32) + 4),
                                   raster_row(520, 9, 7, 1, 513, 8), raster_row(4, 4, 0, 0, 0, 4), raster_row(1, 1, 0, 0, 1, 1)]),
        dict(entry="raster", rows=[raster_row(520, 9, 7, 1, 513, 8), raster_row(520, 9, 8, 1, 513, 8)]),
        dict(entry="wave", rows=[[A, A + 64, 48000 * 30, 0, 0, 1024], [A + 4, A + 68, 48000 * 30, 1024 * 64, 6, 1024], [A, A, 1000, 999, 5, 1],
                                 [0, 0, 0, 0, 3, 0], [A, A, 1 << 40, 0, 39, 2]]),
        dict(entry="stats", rows=[[A, 1440000], [A + 4, 3], [0, 0], [A + 16, (1 << 40) - 1]]),
        dict(entry="pyramid", rows=[[A, A + 128, 1440000, 21, 2], [A + 4, A + 256, 4097, 13, 0], [A, A + 512, 5, 1, 1], [0, 0, 0, 40, 0],
                                    [A + 8, A + 640, (1 << 33) + 7, 34, 1]]),
        dict(entry="pyramid", rows=[[A, A, 0, 12, 0], [A, A, 100, 2, 2]]),
        dict(entry="lod", args=[1601, 347, 1, 0, 1, 0]),
        dict(entry="lod", args=[3000, 257, 2, 1, 0, 0]),
        dict(entry="lod", args=[513, 700, 0, 3, 0, 0]),
        dict(entry="lod", args=[1, 1, 4, 4, 0, 0]),
    ]


def test_fixed_batches_plan_as_the_entries_did(emu):
    """tests/golden/batch_plan_cases.json: the tables the entry bodies built for fixed_cases() before the planners existed (job tables
    field by field; block tables and tap blobs by their SHA-256)"""
    golden = json.load(open(GOLDEN))
    cases = fixed_cases()
    assert len(golden) == len(cases)
    for g, c in zip(golden, cases):
        assert json.loads(json.dumps(c)) == g["case"]
        assert json.loads(json.dumps(run_case(emu, c))) == g["want"], c


# ---------------------------------------------------------------------------------------------------------------- the rules
def _check_block_table(p, counts, what):
    counts = np.asarray(counts, np.int64)
    assert p["err"] == 0, (what, p["text"])
    assert p["n_blocks"] == counts.sum() and len(p["block_job"]) == counts.sum(), what
    assert np.array_equal(p["block_job"], np.repeat(np.arange(len(counts)), counts)), what   # monotone, job i its own count of times


def test_job_tables_follow_the_rules(emu):
    rng = np.random.default_rng(2027)
    done = dict(img=0, fused=0, raster=0)
    for k in range(150):
        entry = ("img", "fused", "raster")[k % 3]
        c = random_case(entry, rng)
        rows = np.array(c["rows"], dtype=object)
        if entry == "img":
            assert check_img(emu, c["rows"])["err"] == 0
            p = plan_img(emu, c["rows"])
            if p["err"]:
                continue
            T, out_h = rows[:, 2].astype(np.int64), (rows[:, 5] - rows[:, 4]).astype(np.int64)
            counts = -(-T // IMG_TILE_T) * -(-out_h // IMG_TILE_F)
            _check_block_table(p, counts, c)
            j = p["jobs"]
            assert np.array_equal(j[:, 9], counts) and np.array_equal(j[:, 8], np.cumsum(counts) - counts), c          # first_tile: prefix sums
            assert np.array_equal(j[:, :6], rows[:, :6].astype(np.int64)), c
            assert np.array_equal(j[:, 6], [r[6] or r[3] for r in c["rows"]]) and np.array_equal(j[:, 7], [r[7] or r[2] for r in c["rows"]]), c
        elif entry == "fused":
            p = plan_fused(emu, c["rows"], c["tiles"])
            if p["err"]:
                continue
            T, out_h = rows[:, 2].astype(np.int64), (rows[:, 5] - rows[:, 4]).astype(np.int64)
            live = (T > 0) & (out_h > 0)
            n_tx, n_ty = np.where(live, -(-T // 512), 0), np.where(live, -(-out_h // 512), 0)
            counts = n_tx * -(-out_h // FUSED_FB)
            _check_block_table(p, counts, c)
            j = p["jobs"]
            assert np.array_equal(j[:, 8], np.cumsum(counts) - counts), c                                              # first_block
            assert np.array_equal(j[:, 9], np.maximum(-(-out_h // FUSED_FB), 1)), c                                    # n_bands, 1 for an empty image
            assert np.array_equal(j[:, 10], n_tx) and np.array_equal(j[:, 11], n_ty), c
            assert np.array_equal(j[:, 12], np.cumsum(n_tx * n_ty) - n_tx * n_ty), c                                   # tile0
            assert np.array_equal(p["ptrs"], c["tiles"] if c["tiles"] else [0]), c                                     # (tx, ty) order; one NULL for none
            # the key: every descriptor's bytes (the image, the address of its pointer array, the tile counts), then its tile pointers
            assert p["desc_bytes"] == 80 and len(p["key"]) == 80 * len(c["rows"]) + 8 * len(c["tiles"]), c
            at = 0
            for r in c["rows"]:
                n_t = r[9] * r[10]
                d = np.frombuffer(p["key"][at:at + 80].tobytes(), U64)
                assert list(d[:8]) == r[:8] and d[9] == r[9] | r[10] << 32, c
                assert list(np.frombuffer(p["key"][at + 80:at + 80 + 8 * n_t].tobytes(), U64)) == c["tiles"][r[8]:r[8] + n_t], c
                at += 80 + 8 * n_t
        else:
            p = plan_raster(emu, c["rows"])
            if p["err"]:
                continue
            w, h = rows[:, 6].astype(np.int64), rows[:, 7].astype(np.int64)
            qpr = (w + 3) // 4
            counts = -(-(qpr * h + 1) // RASTER_QPB)
            _check_block_table(p, counts, c)
            j = p["jobs"]
            assert np.array_equal(j[:, 12], np.cumsum(counts) - counts) and np.array_equal(j[:, 9], qpr), c
            assert np.array_equal(j[:, 8], [r[8] or r[2] for r in c["rows"]]), c
        done[entry] += 1
    assert min(done.values()) >= 25, done


def test_empty_image_makes_a_fused_job_without_blocks(emu):
    rows, tiles = fused_rows([img_row(0, 9), img_row(37, 9, 4, 4), img_row(513, 33)])
    p = plan_fused(emu, rows, tiles)
    assert p["err"] == 0 and list(p["jobs"][:, 9]) == [1, 1, 2] and list(p["jobs"][:, 10]) == [0, 0, 2] and p["n_blocks"] == 4
    assert list(p["block_job"]) == [2, 2, 2, 2]
    rows, tiles = fused_rows([img_row(0, 9)])
    p = plan_fused(emu, rows, tiles)
    assert p["err"] == 0 and p["n_blocks"] == 0 and list(p["ptrs"]) == [0]


@pytest.mark.parametrize("height", [1, 2, 513])
def test_raster_reciprocals_divide_exactly(emu, height):
    """raster_quads (kernels_image.hip) divides with a multiply-high: in the row-quad path q // quads_per_row for the quads
    q < quads_per_row * height of a tile, in the flat-quad path p // width for the first pixel p < width * height of a quad.  (A job
    with quads_per_row or width 1 carries 0: the kernel does not divide then.)"""
    widths = list(range(1, 10)) + [511, 512, 513]
    p = plan_raster(emu, [raster_row(600, 600, 0, 0, w, height) for w in widths])
    assert p["err"] == 0
    for w, j in zip(widths, p["jobs"]):
        qpr, inv_qpr, inv_w = int(j[9]), int(j[10]), int(j[11])
        assert qpr == -(-w // 4)
        q = np.arange(qpr * height, dtype=np.uint64)
        if qpr > 1:
            assert np.array_equal((q * np.uint64(inv_qpr)) >> np.uint64(32), q // np.uint64(qpr)), (w, height)
        else:
            assert inv_qpr == 0
        px = np.arange(w * height, dtype=np.uint64)
        if w > 1:
            assert np.array_equal((px * np.uint64(inv_w)) >> np.uint64(32), px // np.uint64(w)), (w, height)
        else:
            assert inv_w == 0


def test_waveform_tiles(emu):
    rows = [[A, A, 5000, 0, 0, 1024], [A, A, 5000, 64, 6, 77], [A, A, 9, 0, 3, 0], [A, A, 1 << 30, 0, 5, 257], [A, A, 1 << 30, 0, 6, 5]]
    p = plan_wave(emu, rows)
    counts = [4, 20, 0, 2, 2]   # levels <= 5: 256 bins per block; above: 4
    assert p["err"] == 0 and len(p["start"]) == len(rows) + 1
    assert list(p["start"]) == list(np.concatenate([[0], np.cumsum(counts)])) and p["n_blocks"] == sum(counts)
    assert np.array_equal(p["jobs"], np.array(rows, np.int64))
    # the last bin may start at the channel's last sample, not behind it
    assert plan_wave(emu, [[A, A, 1000, 999 - 7 * 16, 4, 8]])["err"] == 0
    bad = plan_wave(emu, [[A, A, 1000, 0, 4, 1], [A, A, 1000, 1000 - 7 * 16, 4, 8]])
    assert (bad["err"], bad["text"]) == (ERR_INVALID_ARG, "desc 1: bins run past the end of the channel")
    assert plan_wave(emu, [[A, A, 1 << 41, 0, 39, 2]])["err"] == 0
    bad = plan_wave(emu, [[A, A, 1 << 41, 0, 40, 1]])
    assert (bad["err"], bad["text"]) == (ERR_INVALID_ARG, "desc 0: level 40 too large")


def pyramid_bins(n, level):
    return 0 if n == 0 else -(-n // (1 << level))


def pyramid_offset(n, level):
    return sum((3 * pyramid_bins(n, l) + 31) // 32 * 32 for l in range(level))


def test_pyramid(emu):
    rows = [[A, A + 4096, 1440000, 21, 2], [A + 4, A + 8192, 4097, 13, 1], [A, A + 512, 5, 1, 1], [A, A + 640, 777, 2, 2], [A + 16, A + 1024, 100000, 14, 0]]
    base = A + (7 << 32)
    p = plan_pyramid(emu, rows, base)
    assert p["err"] == 0 and p["launch"] == 1
    halves = [pyramid_bins(r[2], 12) for r in rows]
    assert list(p["sums_at"]) == list(np.cumsum([2 * h for h in halves]) - [2 * h for h in halves]) and p["sums_floats"] == 2 * sum(halves)
    for r, j, at in zip(rows, p["jobs"], p["sums_at"]):
        n, levels, first = r[2], r[3], r[4]
        assert j[1] == r[1] - 4 * pyramid_offset(n, first)                        # out, shifted back by the skipped levels
        assert j[2] == base + 4 * at                                             # sums, bound
        assert j[3] == (n if levels > first else 0)                              # nothing to do when no level is wanted
        assert j[4] == pyramid_bins(n, 12) and j[5] == levels and j[6] == (1 if r[0] % 16 == 0 else 0) | first << 1
        assert list(j[7:]) == [pyramid_offset(n, l) for l in range(PYR_MAX_LEVELS)]
    assert p["max_samples"] == 1440000 and p["max_levels"] == 21
    # an all-empty batch plans no launch
    for rows in ([[A, A, 0, 12, 0]], [[A, A, 100, 2, 2], [0, 0, 0, 0, 0]], [[A, A, 100, 0, 0]]):
        p = plan_pyramid(emu, rows)
        assert p["err"] == 0 and p["launch"] == 0


def _lod_levels():
    z = np.load(os.path.join(HERE, "golden", "lod_pillow_cases.npz"))
    out = set()
    for k in z.files:
        parts = k.split("/")
        if parts[0] == "whole" and len(parts) == 3:
            lx, ly = (int(v) for v in parts[2].split("_"))
            out.add((lx, ly))
    return sorted(out)


@pytest.mark.parametrize("W,H", [(1, 1), (513, 700), (3000, 257)])
def test_lod_tile_plans(emu, W, H):
    levels = _lod_levels()
    assert levels
    seen = 0
    for lx, ly in levels:
        for tx in range(3):
            for ty in range(2):
                p = plan_lod(emu, W, H, lx, ly, tx, ty)
                if p is None:
                    continue
                assert p["err"] == 0, p["text"]
                seen += 1
                dw, dh = p["dw"], p["dh"]
                left, top, cw, ch = p["box"]
                assert left == p["origin_x"] * W / p["lod_w"] and top == p["origin_y"] * H / p["lod_h"]
                assert abs(left + cw - (p["origin_x"] + dw) * W / p["lod_w"]) < 1e-9 and abs(top + ch - (p["origin_y"] + dh) * H / p["lod_h"]) < 1e-9
                assert 0 <= p["y_lo"] < p["y_hi"] <= H and p["n_rows"] == p["y_hi"] - p["y_lo"]
                sx, cx, wsx, wx = lod_axis(p["blob"], 0, dw, p["taps_x"])
                sy, cy, wsy, wy = lod_axis(p["blob"], p["y_at"], dh, p["taps_y"])
                assert p["y_at"] % 8 == 0 and len(p["blob"]) % 8 == 0
                assert p["y_at"] == 16 * dw + 8 * dw * p["taps_x"] and len(p["blob"]) == p["y_at"] + 16 * dh + 8 * dh * p["taps_y"]
                # starts are clamped to the image; every tap's source row lies in the window the horizontal pass fills
                assert (sx >= 0).all() and (cx >= 1).all() and (sx + cx <= W).all() and cx.max() <= p["taps_x"]
                assert (sy >= p["y_lo"]).all() and (cy >= 1).all() and (sy + cy <= p["y_hi"]).all() and cy.max() <= p["taps_y"]
                assert np.allclose(wsx, [wx[o, :cx[o]].sum() for o in range(dw)]) and np.allclose(wsy, [wy[o, :cy[o]].sum() for o in range(dh)])
                assert p["lod_at"] % 4 == 0 and p["lod_at"] >= p["n_rows"] * dw and p["scratch_bytes"] >= 2 * (p["lod_at"] + dw * dh)
    assert seen


def test_lod_refusal_at_256_mb(emu):
    """est = (6 max(crop_w / dw, crop_h / dh) + 4) * 8 * max(dw, dh) bytes; a level whose estimate passes 256 MB is refused.  A tall
    image at level_x 0: the tile is dw wide at scale 1, and the level that squeezes the H rows into one row has crop_h / dh = H —
    the estimate is large, the table itself (dw x 7 + 6 H taps) stays small."""
    limit = 256.0 * 1024 * 1024
    dw = plan_lod(emu, 600, 100, 0, 7, 0, 0)["dw"]
    assert dw > 500
    est = lambda scale: (6.0 * scale + 4.0) * 8.0 * dw  # noqa: E731
    # level 14 of 16384 rows is one row (scale 16384), the next smaller level two rows (scale 8192)
    assert est(16384) > limit >= est(8192)
    p = plan_lod(emu, 600, 16384, 0, 14, 0, 0)
    assert (p["err"], p["text"]) == (ERR_UNSUPPORTED, "LOD level (0,14) needs a tap table beyond 256 MB")
    p = plan_lod(emu, 600, 16384, 0, 13, 0, 0)
    assert p["err"] == 0 and p["dh"] == 2 and p["dw"] == dw
    # and to the row: the first height whose one-row level passes the limit, and the one below it
    H = next(h for h in range(8192, 16384) if est(h) > limit)
    p = plan_lod(emu, 600, H, 0, 14, 0, 0)
    assert (p["err"], p["text"]) == (ERR_UNSUPPORTED, "LOD level (0,14) needs a tap table beyond 256 MB")
    p = plan_lod(emu, 600, H - 1, 0, 14, 0, 0)
    assert p["err"] == 0 and p["dh"] == 1 and p["dw"] == dw


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refused(p, text):
    assert (p["err"], p["text"]) == (ERR_INVALID_ARG, text), p["text"]


def test_img_refusals(emu):
    ok = img_row(70, 33)
    B = 1 << 31
    for rows, lo, hi, dr, text in [([ok, img_row(70, 33, spec=A + 2)], -1.0, 0.0, 0, "desc 1: spec must be 4-byte aligned"),
                                   ([img_row(70, 33, img=A + 1), img_row(70, 33, spec=A + 2)], -1.0, 0.0, 0, "desc 0: img must be 2-byte aligned"),
                                   ([ok], float("inf"), 0.0, 0, "min_dB must be finite (drawing.rs:19)"),
                                   ([ok], float("nan"), 0.0, 0, "min_dB must be finite (drawing.rs:19)")]:
        _refused(check_img(emu, rows, lo, hi, dr), text)
    assert check_img(emu, [img_row(70, 33, spec=A + 4, img=A + 2)])["err"] == 0
    assert check_img(emu, [ok], float("inf"), 0.0, A)["err"] == 0                       # (a device range: the host values are not read)
    c = check_img(emu, [ok], float("-inf"), float("-inf"))
    assert c["err"] == 0 and c["all_neg_inf"] == 1 and check_img(emu, [ok], float("-inf"), float("-inf"), A)["all_neg_inf"] == 0
    for bad, good, text in [(img_row(70, 33, 9, 8), img_row(70, 33, 8, 8), "i_end < i_start"),
                            (img_row(B, 33, 0, 0), img_row(B - 1, 33, 0, 0), "too large"),
                            (img_row(0, B, 0, 0), img_row(0, B - 1, 0, 0), "too large"),
                            (img_row(0, 33, B, B), img_row(0, 33, B - 1, B - 1), "too large"),
                            (img_row(70, 33, spec=0), img_row(70, 33, 4, 4, spec=0, img=0), "NULL device pointer"),
                            (img_row(70, 33, img=0), img_row(0, 33, spec=0, img=0), "NULL device pointer"),
                            (img_row(70, 33, sp=32), img_row(70, 33, sp=33), "bad spec_pitch"),
                            (img_row(70, 33, sp=B), img_row(70, 33, sp=B - 1), "bad spec_pitch"),
                            (img_row(70, 33, ip=69), img_row(70, 33, ip=70), "bad img_pitch"),
                            (img_row(70, 33, ip=B), img_row(70, 33, ip=B - 1), "bad img_pitch")]:
        _refused(plan_img(emu, [ok, bad, img_row(70, 33, 9, 8)]), "desc 1: " + text)      # the earlier descriptor's error wins
        assert plan_img(emu, [ok, good])["err"] == 0, text


def test_fused_refusals(emu):
    def run(imgs, lo=-1.0, hi=0.0, dr=0, edit=None):
        rows, tiles = fused_rows(imgs)
        if edit:
            edit(rows, tiles)
        return plan_fused(emu, rows, tiles, lo, hi, dr)

    ok = img_row(513, 33)
    B = 1 << 31
    _refused(run([ok, img_row(70, 33, spec=A + 2)]), "desc 1: spec must be 4-byte aligned")
    _refused(run([ok, img_row(70, 33, img=A + 1)]), "desc 1: img must be 2-byte aligned")
    _refused(run([ok], float("inf")), "min_dB must be finite (drawing.rs:19)")
    assert run([ok], float("inf"), 0.0, A)["err"] == 0

    def no_tiles(rows, tiles):
        rows[1][8] = 2 ** 64 - 1
    _refused(run([ok, ok], edit=no_tiles), "desc 1: tiles is NULL")
    assert run([ok, img_row(0, 33)], edit=no_tiles)["err"] == 0                          # (an image without tiles needs no array)
    for bad, good, text in [(img_row(70, 33, 9, 8), img_row(70, 33, 8, 8), "i_end < i_start"),
                            (img_row(B, 33, 0, 0), img_row(B - 1, 33, 0, 0), "too large"),
                            (img_row(0, B, 0, 0), img_row(0, B - 1, 0, 0), "too large"),
                            (img_row(0, 33, B, B), img_row(0, 33, B - 1, B - 1), "too large"),
                            (img_row(70, 33, spec=0), img_row(70, 33, 4, 4, spec=0, img=0), "NULL device pointer or empty spec"),
                            (img_row(70, 0, 0, 5), img_row(70, 1, 0, 5), "NULL device pointer or empty spec"),
                            (img_row(70, 33, sp=32), img_row(70, 33, sp=33), "bad spec_pitch"),
                            (img_row(70, 33, ip=69), img_row(70, 33, ip=70), "bad img_pitch")]:
        _refused(run([ok, bad, img_row(70, 33, 9, 8)]), "desc 1: " + text)
        assert run([ok, good])["err"] == 0, text

    def one_more(rows, tiles):
        rows[1][9] += 1
    _refused(run([ok, ok], edit=one_more), "desc 1: the image has 2 x 1 level-0 tiles, not 3 x 1")

    def off_grid(rows, tiles):
        tiles[3] += 2
    _refused(run([ok, ok], edit=off_grid), "desc 1: tile 1 must be 4-byte aligned")


def _plan_head(lib, fn, rows, names, *more):
    """the head and the error text of a plan alone: the tables of these batches are not worth copying out"""
    rows = np.ascontiguousarray(rows, U64)
    return _head(_blobs(lib, fn(rows.ctypes.data_as(C.POINTER(C.c_uint64)), len(rows), *more), [U64, np.uint8]), names)


def test_block_count_limits(emu):
    """`batch too large for one launch`, every entry that has it, at the limit and one block below it"""
    text, B = "batch too large for one launch", 1 << 31
    # image: 2^27 tiles in one descriptor (2^20 x 2^7); one below: 127 x 2^20 and 2^20 - 1
    _refused(_plan_head(emu, emu.emu_plan_img, [img_row(64 << 20, 128 << 7)], ["n_blocks"]), text)
    p = _plan_head(emu, emu.emu_plan_img, [img_row(64 << 20, 128 * 127), img_row(64 * ((1 << 20) - 1), 128)], ["n_blocks"])
    assert (p["err"], p["n_blocks"]) == (0, (1 << 27) - 1)
    # fused: 2^22 tile columns x 32 bands (2^23 tile pointers, all NULL); one below: 2^22 x 31 and (2^22 - 1) x 1
    tiles = np.zeros((1 << 23) + (1 << 22), U64)
    more = (tiles.ctypes.data_as(C.POINTER(C.c_uint64)), _f32_bits(-1.0), _f32_bits(0.0), 0)
    _refused(_plan_head(emu, emu.emu_plan_fused, [img_row(B - 1, 1024) + [0, 1 << 22, 2]], ["n_blocks", "desc_bytes"], *more), text)
    p = _plan_head(emu, emu.emu_plan_fused, [img_row(B - 1, 992) + [0, 1 << 22, 2], img_row(512 * ((1 << 22) - 1), 32) + [1 << 23, (1 << 22) - 1, 1]],
                   ["n_blocks", "desc_bytes"], *more)
    assert (p["err"], p["n_blocks"]) == (0, (1 << 27) - 1)
    # raster: a 1 x (2^31 - 1) rectangle is 2^21 blocks, 64 of them 2^27; one below: the last one 1024 rows shorter, 2^21 - 1 blocks
    tall = raster_row(1, B - 1, 0, 0, 1, B - 1)
    p = _plan_head(emu, emu.emu_plan_raster, [raster_row(4, 4, 0, 0, 4, 4)] + [tall] * 64 + [raster_row(600, 600, 596, 0, 5, 7)], ["n_blocks"])
    _refused(p, text)                                                                    # (behind it an outside rectangle: the earlier refusal wins)
    p = _plan_head(emu, emu.emu_plan_raster, [tall] * 63 + [raster_row(1, B - 1, 0, 0, 1, B - 1025)], ["n_blocks"])
    assert (p["err"], p["n_blocks"]) == (0, (1 << 27) - 1)
    # waveform: 1024 bins above level 5 are 256 blocks, 2^23 such tiles 2^31; one below: the last tile four bins shorter, 255 blocks
    rows = np.empty((1 << 23, 6), U64)
    rows[:] = [A, A, 1 << 40, 0, 6, 1024]
    _refused(_plan_head(emu, emu.emu_plan_wave_tiles, rows, ["n_blocks"]), text)
    rows[-1, 5] = 1020
    p = _plan_head(emu, emu.emu_plan_wave_tiles, rows, ["n_blocks"])
    assert (p["err"], p["n_blocks"]) == (0, B - 1)


def test_raster_refusals(emu):
    ok = raster_row(600, 600, 3, 1, 5, 7)
    for bad, good, text in [(raster_row(600, 600, 596, 0, 5, 7), raster_row(600, 600, 595, 0, 5, 7), "tile rectangle outside the image"),
                            (raster_row(600, 600, 0, 594, 5, 7), raster_row(600, 600, 0, 593, 5, 7), "tile rectangle outside the image"),
                            (raster_row(1 << 16, 1 << 16, 0, 0, 1 << 16, 1 << 15), raster_row(1, (1 << 31) - 1, 0, 0, 1, (1 << 31) - 1), "tile too large"),
                            (raster_row(600, 600, 3, 1, 5, 7, img=0), raster_row(600, 600, 3, 1, 0, 7, img=0, rgba=0), "NULL device pointer"),
                            (raster_row(600, 600, 3, 1, 5, 7, rgba=A + 2), raster_row(600, 600, 3, 1, 5, 7, rgba=A + 4), "rgba must be 4-byte aligned"),
                            (raster_row(600, 600, 3, 1, 5, 7, img=A + 1), raster_row(600, 600, 3, 1, 5, 7, img=A + 2), "img must be 2-byte aligned"),
                            (raster_row(600, 600, 3, 1, 5, 7, 599), raster_row(600, 600, 3, 1, 5, 7, 600), "img_pitch < img_width"),
                            # (px + 4) * width < 2^32: 2048 x 1024 pixels pass, one more row does not
                            (raster_row(2048, 1100, 0, 0, 2048, 1024), raster_row(2048, 1100, 0, 0, 2048, 1023), "tile too large")]:
        _refused(plan_raster(emu, [ok, bad, raster_row(600, 600, 596, 0, 5, 7)]), "desc 1: " + text)
        assert plan_raster(emu, [ok, good])["err"] == 0, text


def test_wave_stats_pyramid_refusals(emu):
    ok = [A, A, 5000, 0, 0, 1024]
    for bad, good, text in [([A, A, 5000, 0, 0, 1025], ok, "bin_count > 1024"),
                            ([A, A, 5000, 0, 40, 0], [A, A, 5000, 0, 39, 0], "level 40 too large"),
                            ([0, A, 5000, 0, 0, 1], [0, 0, 5000, 0, 0, 0], "NULL device pointer"),
                            ([A + 2, A, 5000, 0, 0, 1], [A + 4, A, 5000, 0, 0, 1], "wav must be 4-byte aligned"),
                            ([A, A + 2, 5000, 0, 0, 1], [A, A + 4, 5000, 0, 0, 1], "bins must be 4-byte aligned"),
                            ([A, A, 5000, 5000, 0, 1], [A, A, 5000, 4999, 0, 1], "bins run past the end of the channel")]:
        _refused(plan_wave(emu, [ok, bad, [A, A, 5000, 0, 0, 1025]]), "desc 1: " + text)
        assert plan_wave(emu, [ok, good])["err"] == 0, text
    ok = [A, 100]
    for bad, good, text in [([0, 1], [0, 0], "NULL device pointer"), ([A + 2, 1], [A + 4, 1], "wav must be 4-byte aligned"),
                            ([A, 1 << 40], [A, (1 << 40) - 1], "too many samples")]:
        _refused(plan_stats(emu, [ok, bad, [0, 1]]), "desc 1: " + text)
        assert plan_stats(emu, [ok, good])["err"] == 0, text
    _refused(plan_stats(emu, [ok] * 65536), "at most 65535 channels per call")
    p = plan_stats(emu, [ok] * 65534 + [[A + 4, 7]])
    assert p["err"] == 0 and p["max_samples"] == 100 and list(p["jobs"][-1]) == [A + 4, 7, 0] and list(p["jobs"][0]) == [A, 100, 1]
    ok = [A, A, 5000, 13, 0]
    for bad, good, text in [([A, A, 5000, 41, 0], [A, A, 5000, 40, 0], "more than 40 levels"),
                            ([0, A, 5000, 1, 0], [0, 0, 5000, 0, 0], "NULL device pointer"), ([A, 0, 5000, 1, 0], [0, 0, 0, 5, 0], "NULL device pointer"),
                            ([A + 2, A, 5000, 1, 0], [A + 4, A, 5000, 1, 0], "wav must be 4-byte aligned"),
                            ([A, A + 2, 5000, 1, 0], [A, A + 4, 5000, 1, 0], "out must be 4-byte aligned"),
                            ([A, A, 1 << 40, 1, 0], [A, A, (1 << 40) - 1, 1, 0], "too many samples"),
                            ([A, A, 5000, 13, 3], [A, A, 5000, 13, 2], "first_level must be 0, 1 or 2")]:
        _refused(plan_pyramid(emu, [ok, bad, [A, A, 5000, 41, 0]]), "desc 1: " + text)
        assert plan_pyramid(emu, [ok, good])["err"] == 0, text
    _refused(plan_pyramid(emu, [ok] * 65536), "at most 65535 channels per call")
    assert plan_pyramid(emu, [ok] * 65535)["err"] == 0


# ---------------------------------------------------------------------------------------------------------------- tile headers
def test_tile_headers_equal_the_oracle(emu):
    cmap = bytes(range(8))
    rng = np.random.default_rng(9)
    out = np.zeros(40, np.uint8)
    for W, H, lx, ly, tx, ty in [(600, 40, 0, 0, 0, 0), (600, 40, 0, 0, 1, 0), (600, 40, 0, 0, 2, 0), (600, 40, 1, 1, 0, 0), (1100, 700, 0, 0, 1, 1),
                                 (1100, 700, 2, 1, 0, 0), (3, 5, 0, 0, 0, 0), (3, 5, 7, 9, 0, 0), (3, 5, 0, 0, 0, 1)]:
        img = rng.integers(0, 65536, (H, W), dtype=np.uint16)
        want = orc.encode_spectrogram_tile(img, cmap, 0x1122334455667788, lx, ly, tx, ty)
        px = emu.emu_spectrogram_tile_header(out.ctypes.data_as(C.c_void_p), 0x1122334455667788, W, H, lx, ly, tx, ty)
        assert out.tobytes() == want[:40] and len(want) == 40 + 4 * px, (W, H, lx, ly, tx, ty)
    out = np.zeros(24, np.uint8)
    x = rng.uniform(-1, 1, 5000).astype(np.float32)
    for n, level, tile in [(5000, 0, 0), (5000, 0, 4), (5000, 0, 5), (5000, 3, 0), (5000, 12, 0), (5000, 13, 0), (5000, 32, 0), (5000, 33, 0),
                           (5000, 63, 0), (5000, 64, 0), (0, 0, 0), (1, 40, 0), (5000, 33, 1)]:
        want = orc.encode_waveform_tile(x[:n], 77, level, tile)
        bins = emu.emu_waveform_tile_header(out.ctypes.data_as(C.c_void_p), 77, n, level, tile)
        assert out.tobytes() == want[:24] and len(want) == 24 + 12 * bins, (n, level, tile)
    assert struct.unpack_from("<I", out, 12)[0] == 0xFFFFFFFF   # (the last case: 2^33 samples per bin, saturated)
