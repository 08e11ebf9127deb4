"""Every stream-ordered ("_dev") entry on a CALLER's stream, against the oracle (include/thesia_amd.h, conventions).

A host drives the library on a stream of its own (a torch side stream in bench.py, the legacy default stream elsewhere): its
producer writes the input on that stream right before the call, its consumer reads the output right behind it, and nothing
synchronises in between.  Each case here is run that way, on one caller stream S and in one host thread:

  1. inputs hold NaN (or a sentinel), every output a first sentinel bit pattern; the device is idle;
  2. on S: torch.cuda._sleep (>= 20 ms), the producer's copy of the real input, the library call(s), the consumer's copy of
     every output, then the input overwritten with NaN and every output with a second sentinel;
  3. one torch.cuda.synchronize();
  4. the consumer's copies equal the oracle (read-after-write: a launch that ran off S read NaN or was not done yet), and
     every output holds only the second sentinel (write-after-write: no library write landed late).

Every case runs twice on the same buffers: cold (descriptor tables uploaded: that path synchronises S on purpose) and warm
(tables reused: nothing but launches), on a non-blocking torch side stream and on the legacy default stream.
Tolerances and oracle functions are those of tests/test_gpu_parity.py for the same entry.
"""
import sys

import numpy as np
import pytest
import torch

import thesia_amd as ta
from thesia_amd import _ffi
from oracle import oracle as orc
from tests.synth import synth_track
from tests.test_gpu_parity import (CHANNEL_STATS_SUM_REL, F32_FLOOR, MOMENT_FLOOR, WAVEFORM_MEAN_EXACT_MAX_LEVEL, WAVEFORM_MEAN_REL_PEAK,
                                   assert_spec_close)

pytestmark = pytest.mark.gpu


DEV = "cuda:0"
CM_LEN = 258
# first / second sentinel of an output buffer by element type (written through an integer view: bit patterns, no float ops)
SENT1 = {torch.float32: 0x7FC0DEAD, torch.int16: -0x4111, torch.uint8: 0xA5}   # (f32 NaN; u16 0xBEEF)
SENT2 = {torch.float32: 0x7FA5A5A5, torch.int16: 0x5A5A, torch.uint8: 0x5A}
_INT_VIEW = {torch.float32: torch.int32, torch.int16: torch.int16, torch.uint8: torch.uint8}


def _bits(t):
    return t.view(_INT_VIEW[t.dtype])


def _poison(t):
    """overwrite an input: NaN for f32, the first sentinel for integer data"""
    if t.dtype == torch.float32:
        t.fill_(float("nan"))
    else:
        _bits(t).fill_(SENT1[t.dtype])


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # (a writable copy)


def _cmap():
    rng = np.random.default_rng(5)
    return bytes(rng.integers(0, 256, CM_LEN * 4, dtype=np.uint8))


# ---------------------------------------------------------------- sleep calibration and the two stream kinds
@pytest.fixture(scope="module")
def cycles():
    """torch.cuda._sleep cycles for a delay of >= 20 ms (30 ms aimed at), measured with events on this card."""
    torch.cuda.init()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def ms(n):
        e0.record()
        torch.cuda._sleep(int(n))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    ms(1000)
    n = 1 << 16
    while ms(n) < 2.0:
        n *= 4
        assert n < 1 << 40, "torch.cuda._sleep does not sleep"
    n = int(n * 30.0 / ms(n)) + 1
    t = ms(n)
    while t < 20.0:
        n = int(n * 1.5)
        t = ms(n)
    print(f"\n[test_gpu_streams] torch.cuda._sleep: {n} cycles = {t:.2f} ms ({n / t / 1e3:.1f} cycles/us)", file=sys.stderr)
    return {"n": n, "ms": t}


@pytest.fixture(scope="module", params=["side", "legacy"])
def on_stream(request):
    """(context, caller stream S): a non-blocking torch side stream, or the legacy default stream (use_given_stream, NULL)."""
    if request.param == "side":
        s = torch.cuda.Stream(DEV)
        ctx = ta.Context(0, s.cuda_stream)
    else:
        s = torch.cuda.default_stream(DEV)
        assert s.cuda_stream == 0
        ctx = ta.Context(0, 0)
    yield ctx, s
    torch.cuda.synchronize()
    ctx.close()


def run_ordered(S, cycles, ins, outs, call):
    """One delayed-producer run on S.  ins: [(device buffer, resident real input)], outs: [device buffer].
    -> (consumer's copies of outs, what call() returned)."""
    for b, _ in ins:
        _poison(b)
    for o in outs:
        _bits(o).fill_(SENT1[o.dtype])
    res = [torch.empty_like(o) for o in outs]
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles["n"])
        for b, src in ins:
            b.copy_(src)                       # producer
        ret = call()
        for r, o in zip(res, outs):
            r.copy_(o)                         # consumer (RAW)
        for b, _ in ins:
            _poison(b)                         # WAR: the library must have read the input before this
        for o in outs:
            _bits(o).fill_(SENT2[o.dtype])     # WAW: no library write may land after this
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert bool((_bits(o) == SENT2[o.dtype]).all()), f"output {i}: a library write landed behind the caller's overwrite"
    return res, ret


def twice(S, cycles, ins, outs, call, check):
    """cold (tables uploaded) and warm (tables reused) run on the same buffers, each checked"""
    for rep in ("cold", "warm"):
        res, ret = run_ordered(S, cycles, ins, outs, call)
        check(res, ret, rep)


# ---------------------------------------------------------------- calc_spec on every route
# (sr, win, hop, n_fft, scale, n_mel, selector, kernel name, floor, lengths: shorter than n_fft, exactly n_fft, long)
ROUTES = {
    "generic-4": (4000, 4, 2, 4, 0, 0, 0, "stft_generic_kernel", F32_FLOOR, (3, 4, 1001)),
    "generic-6144": (48000, 1920, 480, 6144, 0, 0, 0, "stft_generic_kernel", F32_FLOOR, (1000, 6144, 3 * 6144 + 17)),
    "chirp-z-134": (4000, 2, 2, 134, 0, 0, 0, "stft_bluestein_kernel", F32_FLOOR, (50, 134, 3 * 134 + 17)),
    "wave-2048": (48000, 2048, 512, 2048, 0, 0, 0, "stft_wave_kernel", F32_FLOOR, (1000, 2048, 40017)),
    "multi-512": (48000, 512, 128, 512, 0, 0, 0, "stft_wave_kernel", F32_FLOOR, (300, 512, 40005)),
    "mel-banded-2048": (48000, 2048, 512, 2048, 1, 0, 0, "stft_wave_kernel(fused mel)", F32_FLOOR, (1000, 2048, 40017)),
    "mel-moment-4096": (48000, 4096, 1024, 4096, 1, 0, 0, "stft_wave_kernel(fused mel)", MOMENT_FLOOR, (3000, 4096, 40017)),
    "mel-rows-4096": (48000, 4096, 1024, 4096, 1, 0, 12, "stft_wave_kernel+mel_", F32_FLOOR, (3000, 4096, 40017)),
    "mel-rows-2048": (48000, 2048, 512, 2048, 1, 0, 3, "stft_wave_kernel+mel_", F32_FLOOR, (1000, 2048, 40017)),
    "block-mel-8192": (48000, 8192, 2048, 8192, 1, 0, 0, "stft_block_kernel(fused mel)", MOMENT_FLOOR, (4096, 8192, 5 * 8192 + 777)),
    "subwave-32768": (48000, 32768, 8192, 32768, 0, 0, 0, "stft_subwave_kernel", F32_FLOOR, (32768 // 3 + 5, 32768, 3 * 32768 + 17)),
}
_ORACLE = {}


def _route_oracle(name):
    """(wavs, [(dB, amp or None)], mel filterbank or None), computed once per route"""
    if name not in _ORACLE:
        sr, win, hop, n_fft, scale, n_mel, _, _, _, lens = ROUTES[name]
        wavs = [synth_track(1300 + 7 * i + n_fft, sr, n) for i, n in enumerate(lens)]
        fb = (orc.calc_mel_fb(sr, n_fft, n_mel) if n_mel else orc.calc_mel_fb_default(sr, n_fft)) if scale else None
        want = []
        for x in wavs:
            w, amp = orc.calc_spec(x, win, hop, n_fft, mel_fb=fb, return_amp=True)
            want.append((w, None if scale else amp))
        _ORACLE[name] = (wavs, want, fb)
    return _ORACLE[name]


def _make_plan(ctx, name):
    sr, win, hop, n_fft, scale, n_mel, which, kernel, _, _ = ROUTES[name]
    plan = ta.Plan(ctx, sr, win, hop, n_fft, ta.MEL if scale else ta.LINEAR, n_mel)
    if which:
        plan.set_kernel(which)
    assert plan.kernel_name.startswith(kernel) if kernel.endswith("_") else plan.kernel_name == kernel, (name, plan.kernel_name)
    if name == "mel-moment-4096":
        assert plan.mel_moments_info()["groups"] > 0
    return plan


def _spec_buffers(plan, wavs):
    Ts = [plan.n_frames(x.size) for x in wavs]
    srcs = [_dev(x) for x in wavs]
    ins = [(torch.empty_like(s), s) for s in srcs]
    specs = [torch.empty((T, plan.height), dtype=torch.float32, device=DEV) for T in Ts]
    mm = torch.empty((len(wavs), 2), dtype=torch.float32, device=DEV)
    descs = (ta.ChanDesc * len(wavs))(*[ta.ChanDesc(b.data_ptr(), s.data_ptr(), x.size, T, 0)
                                        for (b, _), s, x, T in zip(ins, specs, wavs, Ts)])
    return ins, specs, mm, descs


def _check_specs(name, got, mm, want, floor):
    for i, (g, (w, amp)) in enumerate(zip(got, want)):
        assert_spec_close(g, w, amp, floor=floor)
        assert mm[i, 0] == g.min() and mm[i, 1] == g.max(), (name, i, mm[i], g.min(), g.max())


@pytest.mark.parametrize("route", list(ROUTES))
def test_calc_spec_batch_dev_on_caller_stream(on_stream, cycles, route):
    """th_calc_spec_batch_dev on a ragged batch (shorter than n_fft, exactly n_fft, long: boundary frames and edge jobs):
    the wave / block routes add the generic kernel's launch for the boundary frames, the two-kernel mel routes a second mel
    kernel over amplitude rows (and zero their scratch with a memset) — every launch must follow the caller's stream."""
    ctx, S = on_stream
    wavs, want, _ = _route_oracle(route)
    plan = _make_plan(ctx, route)
    ins, specs, mm, descs = _spec_buffers(plan, wavs)

    def check(res, _, rep):
        got = [r.cpu().numpy() for r in res[:-1]]
        _check_specs(f"{route} {rep}", got, res[-1].cpu().numpy(), want, ROUTES[route][8])

    twice(S, cycles, ins, specs + [mm], lambda: plan.calc_spec_batch_dev(descs, mm.data_ptr()), check)
    plan.close()


def test_calc_spec_batch_ranged_dev_on_caller_stream(on_stream, cycles):
    """th_calc_spec_batch_ranged_dev (spec + per-channel (min, max) + the batch's dB range in one call), and for a
    one-channel batch (the range folded into the wave kernel's follow-up launch); th_minmax_reduce_range_dev behind it."""
    ctx, S = on_stream
    wavs, want, _ = _route_oracle("wave-2048")
    plan = _make_plan(ctx, "wave-2048")
    for sel in (slice(None), slice(2, 3)):
        ins, specs, mm, descs = _spec_buffers(plan, wavs[sel])
        rng_db = torch.empty(2, dtype=torch.float32, device=DEV)
        rng2, negmax = torch.empty(2, dtype=torch.float32, device=DEV), torch.empty(2, dtype=torch.float32, device=DEV)

        def call():
            plan.calc_spec_batch_ranged_dev(descs, mm.data_ptr(), 100.0, rng_db.data_ptr())
            ctx.minmax_reduce_range_dev(mm.data_ptr(), len(descs), 80.0, rng2.data_ptr(), negmax.data_ptr())

        def check(res, _, rep):
            got = [r.cpu().numpy() for r in res[:len(specs)]]
            m, r, r2, nm = (t.cpu().numpy() for t in res[len(specs):])
            _check_specs(f"ranged {rep}", got, m, want[sel], F32_FLOOR)
            lo, hi = orc.global_db_range(m[:, 0], m[:, 1], 100.0)
            assert (r[0], r[1]) == (np.float32(lo), np.float32(hi)), (rep, r, lo, hi)
            lo, hi = orc.global_db_range(m[:, 0], m[:, 1], 80.0)
            assert (r2[0], r2[1]) == (np.float32(lo), np.float32(hi)), (rep, r2, lo, hi)
            assert nm[0] == m[:, 0].min() and nm[1] == -m[:, 1].max()

        twice(S, cycles, ins, specs + [mm, rng_db, rng2, negmax], call, check)
    plan.close()


def test_device_range_chain_with_a_host_collective_in_between(on_stream, cycles):
    """INTEGRATION.md's N-GPU chain on one stream: calc_spec -> th_minmax_reduce_dev -> (the host's MIN all-reduce: a torch op
    on S) -> th_global_db_range_dev -> (a torch op on S rewrites the range) -> th_spec_to_img_batch_dev_ranged.  The images
    follow the rewritten range bit for bit: a quantiser that ran off S would have read the range before the rewrite."""
    ctx, S = on_stream
    wavs, want, _ = _route_oracle("wave-2048")
    plan = _make_plan(ctx, "wave-2048")
    ins, specs, mm, descs = _spec_buffers(plan, wavs)
    H = plan.height
    r2 = torch.empty(2, dtype=torch.float32, device=DEV)
    rng_db = torch.empty(2, dtype=torch.float32, device=DEV)
    other_rank = _dev(np.array([-150.0, -12.5], np.float32))    # [min, -max] of a "rank" with a lower min and a higher max
    shift = _dev(np.array([7.25, 1.5], np.float32))
    pitch = ta.pitch_u16(max(s.shape[0] for s in specs)) + 3     # (a pitch the kernel does not own: padding never written)
    imgs = [torch.empty((H, pitch), dtype=torch.int16, device=DEV) for _ in specs]
    imgd = [_ffi.ImgDesc(s.data_ptr(), im.data_ptr(), s.shape[0], H, 0, H, 0, pitch) for s, im in zip(specs, imgs)]

    def call():
        plan.calc_spec_batch_dev(descs, mm.data_ptr())
        ctx.minmax_reduce_dev(mm.data_ptr(), len(descs), r2.data_ptr())
        torch.minimum(r2, other_rank, out=r2)
        ctx.global_db_range_dev(r2.data_ptr(), 100.0, rng_db.data_ptr())
        rng_db.sub_(shift)
        ctx.spec_to_img_batch_ranged(imgd, rng_db.data_ptr(), CM_LEN)

    def check(res, _, rep):
        n = len(specs)
        got = [r.cpu().numpy() for r in res[:n]]
        m, red, rng = (t.cpu().numpy() for t in res[n:n + 3])
        _check_specs(f"chain {rep}", got, m, want, F32_FLOOR)
        assert red[0] == min(m[:, 0].min(), -150.0) and red[1] == min(-m[:, 1].max(), np.float32(-12.5)), (rep, red)
        lo, hi = orc.global_db_range([red[0]], [-red[1]], 100.0)
        want_rng = np.array([lo, hi], np.float32) - np.array([7.25, 1.5], np.float32)
        assert rng.tobytes() == want_rng.tobytes(), (rep, rng, want_rng)
        for k, (g, im) in enumerate(zip(got, res[n + 3:])):
            w = orc.convert_spectrogram_to_img(g, (0, H), (float(want_rng[0]), float(want_rng[1])), CM_LEN)
            assert np.array_equal(im.cpu().numpy().view(np.uint16)[:, :g.shape[0]], w), (rep, k)

    outs = specs + [mm, r2, rng_db] + imgs
    twice(S, cycles, ins, outs, call, check)
    plan.close()


# ---------------------------------------------------------------- quantiser and raster
def _rand_spec(seed, T, H):
    rng = np.random.default_rng(seed)
    spec = rng.uniform(-140, 10, (T, H)).astype(np.float32)
    spec.ravel()[rng.integers(0, spec.size, 7)] = -np.inf
    spec.ravel()[rng.integers(0, spec.size, 3)] = np.nan
    spec.ravel()[:3] = [-100.0, 0.0, -50.0]
    return spec


def test_spec_to_img_batch_dev_on_caller_stream(on_stream, cycles):
    """th_spec_to_img_batch_dev on a two-image batch (a row range past the spec's height, the library's padded pitch), then
    th_spec_to_img_dev, then the all -inf range (drawing.rs:16-18), which zero-fills with a memset instead of the kernel.
    (Each entry runs cold and warm on its own: a call with other descriptors re-uploads the shared tables.)"""
    ctx, S = on_stream
    shapes = [(300, 1025, 0, 1025, 0), (257, 128, 5, 140, ta.pitch_u16(257))]
    specs = [_rand_spec(40 + k, T, H) for k, (T, H, *_r) in enumerate(shapes)]
    ins = [(torch.empty(s.shape, dtype=torch.float32, device=DEV), _dev(s)) for s in specs]
    imgs = [torch.empty((i1 - i0, p or T), dtype=torch.int16, device=DEV) for T, H, i0, i1, p in shapes]
    descs = [_ffi.ImgDesc(b.data_ptr(), im.data_ptr(), T, H, i0, i1, 0, p) for (b, _), im, (T, H, i0, i1, p) in zip(ins, imgs, shapes)]

    def check_batch(res, _, rep):
        for k, ((T, H, i0, i1, p), s) in enumerate(zip(shapes, specs)):
            want = orc.convert_spectrogram_to_img(s, (i0, i1), (-100.0, 0.0), CM_LEN)
            assert np.array_equal(res[k].cpu().numpy().view(np.uint16)[:, :T], want), (rep, k)

    twice(S, cycles, ins, imgs, lambda: ctx.spec_to_img_batch(descs, -100.0, 0.0, CM_LEN), check_batch)

    T0, H0 = shapes[0][:2]
    one = torch.empty((H0, T0), dtype=torch.int16, device=DEV)

    def check_one(res, _, rep):
        assert np.array_equal(res[0].cpu().numpy().view(np.uint16), orc.convert_spectrogram_to_img(specs[0], (0, H0), (-100.0, 0.0), None)), rep

    twice(S, cycles, ins[:1], [one], lambda: ta.api.check(ta.api.lib.th_spec_to_img_dev(
        ctx.handle, ins[0][0].data_ptr(), T0, H0, 0, H0, -100.0, 0.0, 0, one.data_ptr())), check_one)

    def check_silent(res, _, rep):
        for k, (T, *_r) in enumerate(shapes):
            assert not res[k].cpu().numpy()[:, :T].any(), (rep, k)

    twice(S, cycles, ins, imgs, lambda: ctx.spec_to_img_batch(descs, float("-inf"), float("-inf"), CM_LEN), check_silent)


def _tile_layout(W, H, lead=0):
    geoms = [(tx, ty, ta.spectrogram_tile_geometry(W, H, 0, 0, tx, ty)) for tx in range(-(-W // 512)) for ty in range(-(-H // 512))]
    offs, off = [], lead
    for _, _, g in geoms:
        offs.append(off)
        off += g.width * g.height
    return geoms, offs, off


def test_spec_to_img_raster_batch_dev_on_caller_stream(on_stream, cycles):
    """th_spec_to_img_raster_batch_dev: the u16 image and every level-0 RGBA tile, bit for bit; the range on the device, written
    by the producer like the spec."""
    ctx, S = on_stream
    cmap = _cmap()
    T, H = 700, 347
    spec = _rand_spec(77, T, H)
    ip = ta.pitch_u16(T)
    d_cmap = _dev(np.frombuffer(cmap, np.uint8))
    ins = [(torch.empty((T, H), dtype=torch.float32, device=DEV), _dev(spec)),
           (torch.empty(2, dtype=torch.float32, device=DEV), _dev(np.array([-100.0, -3.5], np.float32)))]
    img = torch.empty((H, ip), dtype=torch.int16, device=DEV)
    geoms, offs, total = _tile_layout(T, H)
    tiles = torch.empty(total * 4, dtype=torch.uint8, device=DEV)
    descs = ctx.make_img_tiles_descs([(_ffi.ImgDesc(ins[0][0].data_ptr(), img.data_ptr(), T, H, 0, H, 0, ip),
                                       [tiles.data_ptr() + 4 * o for o in offs])])
    want_img = orc.convert_spectrogram_to_img(spec, (0, H), (-100.0, -3.5), CM_LEN)

    def check(res, _, rep):
        assert np.array_equal(res[0].cpu().numpy().view(np.uint16)[:, :T], want_img), rep
        flat = res[1].cpu().numpy()
        for (tx, ty, g), o in zip(geoms, offs):
            assert flat[4 * o:4 * (o + g.width * g.height)].tobytes() == orc.encode_spectrogram_tile(want_img, cmap, 1, 0, 0, tx, ty)[40:], (rep, tx, ty)

    twice(S, cycles, ins, [img, tiles], lambda: ctx.spec_to_img_raster_batch(descs, d_cmap.data_ptr(), CM_LEN, d_range=ins[1][0].data_ptr()), check)


def _raster_setup(W, H, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 65536, (H, W), dtype=np.uint16)
    pitch = ta.pitch_u16(W)
    src = _dev(np.pad(img, ((0, 0), (0, pitch - W))).view(np.int16))
    buf = torch.empty_like(src)
    geoms, offs, total = _tile_layout(W, H, lead=1)
    tiles = torch.empty(total * 4, dtype=torch.uint8, device=DEV)
    descs = [_ffi.RasterDesc(buf.data_ptr(), tiles.data_ptr() + 4 * o, W, H, g.origin_x, g.origin_y, g.width, g.height, pitch, 0)
             for (_, _, g), o in zip(geoms, offs)]
    return img, (buf, src), tiles, geoms, offs, descs


def test_raster_tiles_dev_on_caller_stream(on_stream, cycles):
    """th_raster_tiles_dev on a batch of level-0 tiles packed back to back: RGBA bit for bit (render_tiles.rs:281-352)."""
    ctx, S = on_stream
    cmap = _cmap()
    d_cmap = _dev(np.frombuffer(cmap, np.uint8))
    W, H = 1100, 700
    img, inp, tiles, geoms, offs, descs = _raster_setup(W, H, 9)

    def check(res, _, rep):
        flat = res[0].cpu().numpy()
        for (tx, ty, g), o in zip(geoms, offs):
            assert flat[4 * o:4 * (o + g.width * g.height)].tobytes() == orc.encode_spectrogram_tile(img, cmap, 1, 0, 0, tx, ty)[40:], (rep, tx, ty)

    twice(S, cycles, [inp], [tiles], lambda: ctx.raster_tiles(descs, d_cmap.data_ptr(), CM_LEN), check)


def test_encode_spectrogram_tile_dev_on_caller_stream(on_stream, cycles):
    """th_encode_spectrogram_tile_dev (level 0: the raster kernel; LOD: two resample passes and the raster) returns the
    oracle's bytes though the image is written by the caller's producer right before the call."""
    ctx, S = on_stream
    cmap = _cmap()
    rng = np.random.default_rng(21)
    img = rng.integers(0, 65536, (1025, 1400), dtype=np.uint16)
    src = _dev(img.view(np.int16))
    buf = torch.empty_like(src)
    for lx, ly, tx, ty in ((0, 0, 1, 1), (0, 0, 2, 0), (1, 1, 0, 0), (2, 1, 0, 1)):
        def check(res, got, rep):
            assert got == orc.encode_spectrogram_tile(img, cmap, 3, lx, ly, tx, ty), (rep, lx, ly, tx, ty)

        twice(S, cycles, [(buf, src)], [], lambda: ctx.encode_spectrogram_tile_dev(buf.data_ptr(), 1025, 1400, cmap, 3, lx, ly, tx, ty), check)


# ---------------------------------------------------------------- waveform
N_WAV = 300_001


def test_encode_waveform_tile_dev_on_caller_stream(on_stream, cycles):
    """th_encode_waveform_tile_dev: bytes equal to the oracle's (levels whose mean is a sequential sum: bit-exact)."""
    ctx, S = on_stream
    x = synth_track(5, 48000, N_WAV)
    src = _dev(x)
    buf = torch.empty_like(src)
    for level, tile in ((0, 0), (0, 292), (3, 10), (4, 18)):
        def check(res, got, rep):
            assert got == orc.encode_waveform_tile(x, 42, level, tile), (rep, level, tile)

        twice(S, cycles, [(buf, src)], [], lambda: ctx.encode_waveform_tile_dev(buf.data_ptr(), N_WAV, 42, level, tile), check)


def _want_bins(x, level, tile):
    return np.frombuffer(orc.encode_waveform_tile(x, 1, level, tile)[24:], np.float32).reshape(-1, 3)


def _assert_bins(got, want, level, peak, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got[:, :2], want[:, :2]), what
    assert np.abs(got[:, 2] - want[:, 2]).max() <= (0 if level <= WAVEFORM_MEAN_EXACT_MAX_LEVEL else WAVEFORM_MEAN_REL_PEAK * peak), what


def test_waveform_tiles_dev_on_caller_stream(on_stream, cycles):
    """th_waveform_tiles_dev: a batch of tiles of several levels (incl. each level's last, partial tile) against
    encode_waveform_tile's bins: min / max bit-exact, the mean bit-exact up to level 4 and within 1e-6 of the peak above."""
    ctx, S = on_stream
    x = synth_track(6, 48000, N_WAV)
    peak = float(np.abs(x).max())
    src = _dev(x)
    buf = torch.empty_like(src)
    jobs = []
    for level in (0, 3, 5, 9, 16):
        n_tiles = -(-(-(-N_WAV // (1 << level))) // 1024)
        for tile in sorted({0, n_tiles - 1}):
            start, bins, _ = ta.waveform_tile_geometry(N_WAV, level, tile)
            jobs.append((level, tile, start, bins, torch.empty((bins, 3), dtype=torch.float32, device=DEV)))
    descs = [_ffi.WaveDesc(buf.data_ptr(), o.data_ptr(), N_WAV, start, level, bins) for level, tile, start, bins, o in jobs]

    def check(res, _, rep):
        for (level, tile, *_r), r in zip(jobs, res):
            _assert_bins(r.cpu().numpy(), _want_bins(x, level, tile), level, peak, (rep, level, tile))

    twice(S, cycles, [(buf, src)], [j[-1] for j in jobs], lambda: ctx.waveform_tiles(descs), check)


def test_waveform_pyramid_dev_on_caller_stream(on_stream, cycles):
    """th_waveform_pyramid_dev (base pass + tree passes) on two channels, one with first_level = 2: every level's first and
    last tile against encode_waveform_tile."""
    ctx, S = on_stream
    lens, firsts, n_levels = (N_WAV, 70_001), (0, 2), 15
    xs = [synth_track(8 + i, 44100, n) for i, n in enumerate(lens)]
    ins = [(torch.empty(n, dtype=torch.float32, device=DEV), _dev(x)) for n, x in zip(lens, xs)]
    base = [ta.api.pyramid_offset(n, f) for n, f in zip(lens, firsts)]
    outs = [torch.empty(ta.api.pyramid_offset(n, n_levels) - b, dtype=torch.float32, device=DEV) for n, b in zip(lens, base)]
    descs = [_ffi.PyramidDesc(b.data_ptr(), o.data_ptr(), n, n_levels, f) for (b, _), o, n, f in zip(ins, outs, lens, firsts)]

    def check(res, _, rep):
        for x, n, f, b, r in zip(xs, lens, firsts, base, res):
            flat, peak = r.cpu().numpy(), float(np.abs(x).max())
            for level in range(f, n_levels):
                a = ta.api.pyramid_offset(n, level) - b
                lv = flat[a:a + 3 * ta.api.pyramid_bins(n, level)].reshape(-1, 3)
                n_tiles = -(-lv.shape[0] // 1024)
                for t in sorted({0, n_tiles - 1}):
                    _assert_bins(lv[1024 * t:1024 * (t + 1)], _want_bins(x, level, t), level, peak, (rep, n, level, t))

    twice(S, cycles, ins, outs, lambda: ctx.waveform_pyramid_dev(descs), check)


def test_channel_stats_dev_on_caller_stream(on_stream, cycles):
    """th_channel_stats_dev (accumulators zeroed by a memset on the stream, results returned to the host)."""
    ctx, S = on_stream
    rng = np.random.default_rng(17)
    xs = [rng.uniform(-1, 1, n).astype(np.float32) for n in (5, 4097, 300_001)]
    xs[2][1234] = -1.5
    ins = [(torch.empty(x.size, dtype=torch.float32, device=DEV), _dev(x)) for x in xs]
    descs = [_ffi.StatsDesc(b.data_ptr(), x.size) for (b, _), x in zip(ins, xs)]

    def check(res, ret, rep):
        ss, pk = ret
        for x, s, p in zip(xs, ss, pk):
            want_s = orc.sum_squares(x)
            assert p == orc.abs_max(x), (rep, x.size, p)
            assert abs(s - want_s) <= CHANNEL_STATS_SUM_REL * max(want_s, 1e-30), (rep, x.size, s, want_s)

    twice(S, cycles, ins, [], lambda: ctx.channel_stats_dev(descs), check)


# ---------------------------------------------------------------- th_dev_copy and the host copy helpers
@pytest.mark.parametrize("size", [16, 48, 4096 + 16, 64 * 2**20 + 48])
def test_dev_copy_on_caller_stream(on_stream, cycles, size):
    """th_dev_copy (the bench's copy-bandwidth yardstick): sizes of one, three and 257 lanes and 64 MiB + 3 lanes, at 16-byte
    offsets into larger buffers; the bytes outside [offset, offset + size) of the destination stay untouched."""
    ctx, S = on_stream
    pad = 256
    g = torch.Generator(device=DEV)
    g.manual_seed(size)
    real = torch.randint(0, 256, (size + pad,), dtype=torch.uint8, device=DEV, generator=g)
    src = torch.empty_like(real)
    dst = torch.empty(size + pad, dtype=torch.uint8, device=DEV)
    for so, do in ((0, 0), (16, 48), (48, 16), (pad - 16, pad - 16)):
        def check(res, _, rep):
            r = res[0]
            assert torch.equal(r[do:do + size], real[so:so + size]), (rep, so, do)
            assert bool((r[:do] == SENT1[torch.uint8]).all()) and bool((r[do + size:] == SENT1[torch.uint8]).all()), (rep, so, do)

        twice(S, cycles, [(src, real)], [dst], lambda: ctx.dev_copy(dst.data_ptr() + do, src.data_ptr() + so, size), check)


def test_dev_copy_refuses_misaligned_arguments(on_stream):
    """A pointer or a size off the 16-byte grid: TH_ERR_INVALID_ARG (-1) and nothing written."""
    ctx, S = on_stream
    src = torch.arange(512, dtype=torch.int32, device=DEV).view(torch.uint8)
    dst = torch.full((2048,), SENT1[torch.uint8], dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        for d_off, s_off, n in ((4, 0, 64), (0, 8, 64), (0, 0, 20), (1, 1, 16), (16, 16, 8)):
            with pytest.raises(ta.ThError) as e:
                ctx.dev_copy(dst.data_ptr() + d_off, src.data_ptr() + s_off, n)
            assert e.value.code == -1, (d_off, s_off, n)
    torch.cuda.synchronize()
    assert bool((dst == SENT1[torch.uint8]).all())


def test_dev_upload_download_follow_the_stream(on_stream, cycles):
    """th_dev_upload / th_dev_download into / out of a th_dev_alloc buffer, behind stream-ordered writes on the caller's
    stream: the download sees the write enqueued before it, the upload lands after the write enqueued before it."""
    ctx, S = on_stream
    n = 1 << 20
    a = np.random.default_rng(2).integers(0, 256, n, dtype=np.uint8)
    real = _dev(a)
    zeros = torch.zeros(n, dtype=torch.uint8, device=DEV)
    buf = ctx.alloc(n)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles["n"])
        ctx.dev_copy(buf.ptr, real.data_ptr(), n)
        got = buf.download((n,), np.uint8)
    assert np.array_equal(got, a)
    b = a[::-1].copy()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles["n"])
        ctx.dev_copy(buf.ptr, zeros.data_ptr(), n)
        buf.upload(b)
        out = torch.empty_like(real)
        ctx.dev_copy(out.data_ptr(), buf.ptr, n)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), b)
    buf.free()


# ---------------------------------------------------------------- two contexts on two streams, graph replay, no hidden wait
def test_two_contexts_ordered_by_an_event(cycles):
    """Context A on S1 computes spectrograms; S2 waits on an event torch recorded on S1; context B on S2 quantises and
    rasterises them.  The library orders its work only through the stream it was given, so B sees A's rows."""
    cmap = _cmap()
    S1, S2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    A, B = ta.Context(0, S1.cuda_stream), ta.Context(0, S2.cuda_stream)
    wavs, want, _ = _route_oracle("wave-2048")
    plan = _make_plan(A, "wave-2048")
    ins, specs, mm, descs = _spec_buffers(plan, wavs)
    H = plan.height
    d_cmap = _dev(np.frombuffer(cmap, np.uint8))
    imgs, tiles, rast, lays = [], [], [], []
    for s in specs:
        T = s.shape[0]
        imgs.append(torch.empty((H, T), dtype=torch.int16, device=DEV))
        geoms, offs, total = _tile_layout(T, H)
        tiles.append(torch.empty(total * 4, dtype=torch.uint8, device=DEV))
        lays.append((geoms, offs))
        rast += [_ffi.RasterDesc(imgs[-1].data_ptr(), tiles[-1].data_ptr() + 4 * o, T, H, g.origin_x, g.origin_y, g.width, g.height, 0, 0)
                 for (_, _, g), o in zip(geoms, offs)]
    imgd = [_ffi.ImgDesc(s.data_ptr(), im.data_ptr(), s.shape[0], H, 0, H, 0, 0) for s, im in zip(specs, imgs)]
    outs = specs + [mm] + imgs + tiles
    for rep in ("cold", "warm"):
        for b, _ in ins:
            _poison(b)
        for o in outs:
            _bits(o).fill_(SENT1[o.dtype])
        res = [torch.empty_like(o) for o in outs]
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        with torch.cuda.stream(S1):
            torch.cuda._sleep(cycles["n"])
            for b, src in ins:
                b.copy_(src)
            plan.calc_spec_batch_dev(descs, mm.data_ptr())
            ev.record(S1)
        with torch.cuda.stream(S2):
            S2.wait_event(ev)
            B.spec_to_img_batch(imgd, -100.0, 0.0, CM_LEN)
            B.raster_tiles(rast, d_cmap.data_ptr(), CM_LEN)
            for r, o in zip(res, outs):
                r.copy_(o)
            for o in outs:
                _bits(o).fill_(SENT2[o.dtype])
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert bool((_bits(o) == SENT2[o.dtype]).all()), (rep, i)
        n = len(specs)
        got = [r.cpu().numpy() for r in res[:n]]
        _check_specs(f"two streams {rep}", got, res[n].cpu().numpy(), want, F32_FLOOR)
        for k, g in enumerate(got):
            w = orc.convert_spectrogram_to_img(g, (0, H), (-100.0, 0.0), CM_LEN)
            assert np.array_equal(res[n + 1 + k].cpu().numpy().view(np.uint16), w), (rep, k)
            flat = res[n + 1 + n + k].cpu().numpy()
            for (tx, ty, gm), o in zip(*lays[k]):
                assert flat[4 * o:4 * (o + gm.width * gm.height)].tobytes() == orc.encode_spectrogram_tile(w, cmap, 1, 0, 0, tx, ty)[40:], (rep, k, tx, ty)
    plan.close()
    A.close()
    B.close()


def test_graph_replay_reads_the_input_written_before_it(cycles):
    """ctx.capture of one calc_spec -> range -> image step on a side-stream context, replayed twice; before each replay the
    caller's stream gets a torch write of a different input.  Each replay's rows, range and image follow its own input."""
    S = torch.cuda.Stream(DEV)
    ctx = ta.Context(0, S.cuda_stream)
    plan = _make_plan(ctx, "wave-2048")
    sr, win, hop, n_fft = 48000, 2048, 512, 2048
    n = 30000
    xs = [synth_track(2100 + k, sr, n) * (1.0 if k == 0 else 0.125) for k in range(3)]
    srcs = [_dev(x.astype(np.float32)) for x in xs]
    wav = srcs[0].clone()
    T, H = plan.n_frames(n), plan.height
    spec = torch.empty((T, H), dtype=torch.float32, device=DEV)
    mm = torch.empty((1, 2), dtype=torch.float32, device=DEV)
    rng_db = torch.empty(2, dtype=torch.float32, device=DEV)
    img = torch.empty((H, T), dtype=torch.int16, device=DEV)
    chan = (ta.ChanDesc * 1)(ta.ChanDesc(wav.data_ptr(), spec.data_ptr(), n, T, 0))
    imgd = [_ffi.ImgDesc(spec.data_ptr(), img.data_ptr(), T, H, 0, H, 0, 0)]

    def step():
        plan.calc_spec_batch_dev(chan, mm.data_ptr())
        ctx.minmax_reduce_range_dev(mm.data_ptr(), 1, 100.0, rng_db.data_ptr())
        ctx.spec_to_img_batch_ranged(imgd, rng_db.data_ptr(), CM_LEN)

    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        step()   # direct: uploads the tables, sizes the scratch
    torch.cuda.synchronize()
    graph = ctx.capture(step)
    outs = (spec, rng_db, img)
    res = [[torch.empty_like(o) for o in outs] for _ in (1, 2)]
    with torch.cuda.stream(S):
        for k in (1, 2):
            torch.cuda._sleep(cycles["n"])
            wav.copy_(srcs[k])
            graph.launch()
            for r, o in zip(res[k - 1], outs):
                r.copy_(o)
    torch.cuda.synchronize()
    for k in (1, 2):
        got_spec, got_rng, got_img = (r.cpu().numpy() for r in res[k - 1])
        w, amp = orc.calc_spec(xs[k].astype(np.float32), win, hop, n_fft, return_amp=True)
        assert_spec_close(got_spec, w, amp)
        lo, hi = orc.global_db_range([got_spec.min()], [got_spec.max()], 100.0)
        assert (got_rng[0], got_rng[1]) == (np.float32(lo), np.float32(hi)), (k, got_rng, lo, hi)
        assert np.array_equal(got_img.view(np.uint16), orc.convert_spectrogram_to_img(got_spec, (0, H), (lo, hi), CM_LEN)), k
    graph.close()
    plan.close()
    ctx.close()


@pytest.mark.parametrize("entry", ["calc_spec_batch_dev", "spec_to_img_batch_dev", "raster_tiles_dev"])
def test_repeat_calls_do_not_wait_on_the_host(on_stream, cycles, entry):
    """A repeat call with the same descriptors only enqueues: behind a >= 200 ms sleep on S, the call returns while S is busy.
    (A first call, or one with changed descriptors, uploads its tables and synchronises the stream on purpose.)"""
    ctx, S = on_stream
    cmap = _cmap()
    plan = None
    if entry == "calc_spec_batch_dev":
        wavs, want, _ = _route_oracle("wave-2048")
        plan = _make_plan(ctx, "wave-2048")
        ins, specs, mm, descs = _spec_buffers(plan, wavs)
        for b, src in ins:
            b.copy_(src)
        call = lambda: plan.calc_spec_batch_dev(descs, mm.data_ptr())  # noqa: E731
    elif entry == "spec_to_img_batch_dev":
        spec = _dev(_rand_spec(3, 500, 1025))
        img = torch.empty((1025, 500), dtype=torch.int16, device=DEV)
        descs = [_ffi.ImgDesc(spec.data_ptr(), img.data_ptr(), 500, 1025, 0, 1025, 0, 0)]
        call = lambda: ctx.spec_to_img_batch(descs, -100.0, 0.0, CM_LEN)  # noqa: E731
    else:
        d_cmap = _dev(np.frombuffer(cmap, np.uint8))
        img, (buf, src), tiles, geoms, offs, descs = _raster_setup(1100, 700, 4)
        buf.copy_(src)
        call = lambda: ctx.raster_tiles(descs, d_cmap.data_ptr(), CM_LEN)  # noqa: E731
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        call()
        call()
    torch.cuda.synchronize()
    long = int(cycles["n"] * max(200.0 / cycles["ms"], 1.0) * 1.2) + 1
    with torch.cuda.stream(S):
        torch.cuda._sleep(long)
        call()
        busy = not S.query()
    torch.cuda.synchronize()
    assert busy, f"{entry} waited on the host for the caller's stream"
    if plan is not None:
        plan.close()
