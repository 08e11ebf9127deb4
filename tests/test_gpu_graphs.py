"""HIP-graph capture and replay (th_ctx_capture_begin / _end, th_graph_launch) of every stream-ordered entry.

A replay runs only what the captured calls ENQUEUED; whatever a call did on the host at call time (a memset it chose to
skip, a scratch buffer it zeroed once, an initialising launch it left out for this batch) is not in the graph.  So every
case here goes through one protocol (replay_protocol) on buffers allocated once:

  direct on X0 | capture | replay A on X1 | a direct call on X1 (tables warm: it only enqueues) | replays B, C back to back
  on X2 | the graph closed | direct on X2 | direct on X0

with every output refilled with the first sentinel of tests/test_gpu_streams.py in front of each of them.  For the STFT
cases X1 = X0 / 8 and X2 = 4 X0 (exact scalings): a (max) left over from X0 shows in replay A, a (min) left over from X1 in
replay C.  Asserted for every replay:

  (a) no sentinel is left in the payload of any output (integer outputs: none where the direct call's result, which is held
      to the oracle bit for bit, has another value — 0xBEEF and 0xA5 are legitimate pixels);
  (b) the outputs are bit-identical to those of the direct call on the same input and buffers;
  (c) the outputs pass the check the same entry has in tests/test_gpu_streams.py, against the same oracle and with the same
      tolerance (the STFT oracle is evaluated once per route, on X0: its amplitudes are scaled by the power of two and the
      dB recomputed in float64);
  (d) STFT: the (min, max) slots equal the rows' own min and max exactly (part of _check_specs).

The STFT cases run on a side-stream context and on one on the legacy default stream (which records on a stream of its own:
HIP cannot capture the legacy stream), the others on the side stream.  The batches of tests/test_gpu_streams.py never put the
wave kernels' chunk queue in use; test_calc_spec_batch_dev_replay_with_the_chunk_queue_in_use does.
The refusal the header documents (a call that has to upload or allocate while capturing) runs in one child process.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import thesia_amd as ta
from thesia_amd import _ffi
from oracle import oracle as orc
from tests.synth import synth_track
from tests.test_gpu_parity import CHANNEL_STATS_SUM_REL
from tests.test_gpu_streams import (CM_LEN, DEV, N_WAV, ROUTES, SENT1, _assert_bins, _bits, _check_specs, _cmap, _dev, _make_plan,
                                    _rand_spec, _raster_setup, _route_oracle, _spec_buffers, _tile_layout, _want_bins)
from tests.test_gpu_streams import cycles  # noqa: F401  (the fixture: torch.cuda._sleep cycles of >= 20 ms)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPS = (0, -3, 2)     # X0, X1 = X0 * 2**-3, X2 = X0 * 2**2
_CTX = {}             # "side" / "legacy" -> (context, caller stream)
_PLANS = {}           # (stream kind, route) -> plan
_WANT = {}            # (route, exponent) -> [(dB in f64, amp in f64 or None)]
_OWN = {}             # a case with a batch of its own: name -> (signals, [(dB, amp)]) on X0


@pytest.fixture(scope="module", autouse=True)
def _close_module():
    yield
    torch.cuda.synchronize()
    for plan in _PLANS.values():
        plan.close()
    _PLANS.clear()
    for ctx, _ in _CTX.values():
        ctx.close()
    _CTX.clear()


def _on(kind):
    """(context, caller stream): a non-blocking torch side stream, or the legacy default stream"""
    if kind not in _CTX:
        torch.cuda.init()
        if kind == "side":
            s = torch.cuda.Stream(DEV)
            _CTX[kind] = (ta.Context(0, s.cuda_stream), s)
        else:
            s = torch.cuda.default_stream(DEV)
            assert s.cuda_stream == 0
            _CTX[kind] = (ta.Context(0, 0), s)
    return _CTX[kind]


def _plan(kind, route):
    if (kind, route) not in _PLANS:
        _PLANS[kind, route] = _make_plan(_on(kind)[0], route)
    return _PLANS[kind, route]


# ---------------------------------------------------------------- the protocol
def _whole(a):
    return a


def _cols(n):
    return lambda a: a[:, :n]


_SENT_NP = {np.dtype(np.float32): (np.uint32, SENT1[torch.float32]), np.dtype(np.int16): (np.int16, SENT1[torch.int16]),
            np.dtype(np.uint8): (np.uint8, SENT1[torch.uint8])}


def _sentinel_left(got, ref):
    """(a): elements of a payload that still hold the first sentinel (integer data: and are another value in `ref`)"""
    view, s = _SENT_NP[got.dtype]
    hit = got.view(view) == view(s)
    if got.dtype != np.float32:
        hit &= ref.view(view) != view(s)
    return int(hit.sum())


def replay_protocol(ctx, S, cycles, ins, outs, step, check, what):  # noqa: F811
    """ins: [(device buffer, (X0, X1, X2) resident)], outs: [(device buffer, payload of its host copy, kept or None)] — kept: the
    part of the host copy that is not the library's and must still hold the sentinel —, step(): the library calls,
    check(payloads, v, tag): assertion (c) (and (d)) for input X_v.  ((b) holds for every entry here: none
    needed a fall-back to (c) alone.)"""
    def write(v):
        for b, xs in ins:
            b.copy_(xs[v])

    def fill():
        for o, *_r in outs:
            _bits(o).fill_(SENT1[o.dtype])

    def take():
        return [o.clone() for o, *_r in outs]

    def host(res):
        full = [r.cpu().numpy() for r in res]
        for a, (_, _, kept) in zip(full, outs):
            if kept is not None:
                view, s = _SENT_NP[a.dtype]
                assert bool((kept(a).view(view) == view(s)).all()), f"{what}: a write landed outside the extent of the call"
        return [pay(a) for a, (_, pay, _) in zip(full, outs)]

    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        write(0)
        fill()
        step()                 # direct: uploads the tables, sizes the scratch
        d0 = take()
    torch.cuda.synchronize()
    graph = ctx.capture(step)
    try:
        with torch.cuda.stream(S):
            write(1)
            fill()
            graph.launch()     # replay A
            g_a = take()
            fill()
            torch.cuda._sleep(cycles["n"])
            step()             # a direct call between replays: warm tables, so nothing but launches
            busy = not S.query()
            d1 = take()
            write(2)
            fill()
            graph.launch()     # replays B and C
            graph.launch()
            g_c = take()
        torch.cuda.synchronize()
    finally:
        graph.close()
    with torch.cuda.stream(S):
        fill()
        step()
        d2 = take()
        write(0)
        fill()
        step()
        d0b = take()
    torch.cuda.synchronize()
    d0, g_a, d1, g_c, d2, d0b = (host(r) for r in (d0, g_a, d1, g_c, d2, d0b))

    assert busy, f"{what}: the direct call with warm tables waited on the host for the stream"
    for tag, got, ref, v in (("direct X0", d0, d0, 0), ("direct X1 between the replays", d1, d1, 1), ("replay A", g_a, d1, 1),
                             ("direct X2 behind the graph", d2, d2, 2), ("replay C", g_c, d2, 2), ("direct X0 behind the graph", d0b, d0, 0)):
        for i, (g, r) in enumerate(zip(got, ref)):
            left = _sentinel_left(g, r)
            assert left == 0, f"(a) {what}, {tag}: {left} elements of output {i} still hold the sentinel"
        if got is not ref:
            for i, (g, r) in enumerate(zip(got, ref)):
                assert g.tobytes() == r.tobytes(), f"(b) {what}, {tag}: output {i} differs from the direct call on the same input"
        check(got, v, f"(c) {what}, {tag}")


# ---------------------------------------------------------------- STFT routes
def _scaled_want(route, e):
    """the oracle of X0 * 2**e from the oracle of X0: amplitudes times 2**e (exact), dB from them in float64"""
    if (route, e) not in _WANT:
        out = []
        for w, amp in (_OWN[route] if route in _OWN else _route_oracle(route))[1]:
            a = np.power(10.0, w.astype(np.float64) / 20.0) if amp is None else amp.astype(np.float64)
            a = np.where(np.isneginf(w), 0.0, a) * 2.0 ** e
            with np.errstate(divide="ignore"):
                out.append((20.0 * np.log10(a), None if amp is None else a))
        _WANT[route, e] = out
    return _WANT[route, e]


def _stft_case(kind, cycles, route, sel=slice(None), minmax=True, dB_range=None, plan=None):  # noqa: F811
    ctx, S = _on(kind)
    wavs = (_OWN[route] if route in _OWN else _route_oracle(route))[0][sel]
    plan = plan or _plan(kind, route)
    ins, specs, mm, descs = _spec_buffers(plan, wavs)
    ins = [(b, tuple(src * 2.0 ** e for e in EXPS)) for b, src in ins]
    rng_db = torch.empty(2, dtype=torch.float32, device=DEV)
    outs = [(s, _whole, None) for s in specs] + ([(mm, _whole, None)] if minmax else []) + ([(rng_db, _whole, None)] if dB_range else [])
    floor = ROUTES[route.split("/")[0]][8]
    n = len(specs)

    def step():
        if dB_range:
            plan.calc_spec_batch_ranged_dev(descs, mm.data_ptr(), dB_range, rng_db.data_ptr())
        else:
            plan.calc_spec_batch_dev(descs, mm.data_ptr() if minmax else None)

    def check(got, v, tag):
        want = _scaled_want(route, EXPS[v])[sel]
        m = got[n] if minmax else np.array([[g.min(), g.max()] for g in got[:n]], np.float32)   # ((d) needs the slots)
        _check_specs(tag, got[:n], m, want, floor)
        if dB_range:
            lo, hi = orc.global_db_range(m[:, 0], m[:, 1], dB_range)
            assert (got[n + 1][0], got[n + 1][1]) == (np.float32(lo), np.float32(hi)), (tag, got[n + 1], lo, hi)

    replay_protocol(ctx, S, cycles, ins, outs, step, check, f"{route} on the {kind} stream")


@pytest.mark.parametrize("kind", ["side", "legacy"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_calc_spec_batch_dev_replay(cycles, route, kind):  # noqa: F811
    """th_calc_spec_batch_dev on the ragged batch of every route (edge jobs, the second mel kernel, the scratch buffers, the
    multi-frame tail guard), with d_minmax."""
    _stft_case(kind, cycles, route)


@pytest.mark.parametrize("kind", ["side", "legacy"])
@pytest.mark.parametrize("route", ["wave-2048", "multi-512", "mel-rows-2048", "generic-4"])
def test_calc_spec_batch_dev_replay_without_minmax(cycles, route, kind):  # noqa: F811
    """d_minmax = NULL, once per route family: a wave route, the multi-frame one, a two-kernel mel route, the generic kernel."""
    _stft_case(kind, cycles, route, minmax=False)


@pytest.mark.parametrize("kind", ["side", "legacy"])
@pytest.mark.parametrize("route,sel", [("wave-2048", slice(None)), ("wave-2048", slice(2, 3)), ("mel-rows-2048", slice(None)),
                                       ("generic-6144", slice(None))], ids=["wave-2048-batch", "wave-2048-one-channel", "mel-rows-2048", "generic-6144"])
def test_calc_spec_batch_ranged_dev_replay(cycles, route, sel, kind):  # noqa: F811
    """th_calc_spec_batch_ranged_dev: the one-channel batch folds the range into the wave kernel's follow-up launch, the others
    add the reduce launch; the range is that of the replay's own (min, max)."""
    _stft_case(kind, cycles, route, sel=sel, dB_range=100.0)


def test_calc_spec_batch_dev_replay_with_the_chunk_queue_in_use(cycles):  # noqa: F811
    """The wave kernels deal chunks out through a queue only when there are more chunks than resident waves (more than 32 frames
    per wave: a batch of hours); below that every chunk is some wave's first and the queue head, which the follow-up launch
    rewinds, is never read.  One frame per chunk (th_plan_set_kernel's tuning field) puts the queue in use at one channel of a
    little more than CUs x 12 frames: a head that a replay left where the launch had moved it makes the next launch skip rows."""
    route, name = "wave-2048", "wave-2048/queue"
    sr, win, hop, n_fft = ROUTES[route][:4]
    ctx, _ = _on("side")
    n_frames = torch.cuda.get_device_properties(0).multi_processor_count * 12 + 300
    if name not in _OWN:
        x = synth_track(4100, sr, n_frames * hop)
        w, amp = orc.calc_spec(x, win, hop, n_fft, return_amp=True)
        _OWN[name] = ([x], [(w, amp)])
    if ("side", name) not in _PLANS:
        plan = _make_plan(ctx, route)
        plan.set_kernel(1 << 16)   # bits 16-23: frames per chunk
        assert plan.kernel_name == ROUTES[route][7]
        _PLANS["side", name] = plan
    assert _PLANS["side", name].n_frames(n_frames * hop) > n_frames
    _stft_case("side", cycles, name, plan=_PLANS["side", name])


# ---------------------------------------------------------------- the device range chain and the image entries (side stream)
def test_device_range_chain_replay_behind_a_mel_stft(cycles):  # noqa: F811
    """th_minmax_reduce_dev -> th_global_db_range_dev -> th_spec_to_img_batch_dev_ranged, and th_minmax_reduce_range_dev, in one
    graph behind the mel-banded-2048 STFT."""
    route = "mel-banded-2048"
    ctx, S = _on("side")
    plan = _plan("side", route)
    ins, specs, mm, descs = _spec_buffers(plan, _route_oracle(route)[0])
    ins = [(b, tuple(src * 2.0 ** e for e in EXPS)) for b, src in ins]
    H, n = plan.height, len(specs)
    r2, rng_db, rng2, negmax = (torch.empty(2, dtype=torch.float32, device=DEV) for _ in range(4))
    pitch = ta.pitch_u16(max(s.shape[0] for s in specs)) + 3     # (a pitch the kernel does not own: padding never written)
    imgs = [torch.empty((H, pitch), dtype=torch.int16, device=DEV) for _ in specs]
    imgd = [_ffi.ImgDesc(s.data_ptr(), im.data_ptr(), s.shape[0], H, 0, H, 0, pitch) for s, im in zip(specs, imgs)]

    def step():
        plan.calc_spec_batch_dev(descs, mm.data_ptr())
        ctx.minmax_reduce_dev(mm.data_ptr(), n, r2.data_ptr())
        ctx.global_db_range_dev(r2.data_ptr(), 100.0, rng_db.data_ptr())
        ctx.spec_to_img_batch_ranged(imgd, rng_db.data_ptr(), CM_LEN)
        ctx.minmax_reduce_range_dev(mm.data_ptr(), n, 80.0, rng2.data_ptr(), negmax.data_ptr())

    def check(got, v, tag):
        m, red, rng, rng80, nm = got[n:n + 5]
        _check_specs(tag, got[:n], m, _scaled_want(route, EXPS[v]), ROUTES[route][8])
        assert red[0] == m[:, 0].min() and red[1] == -m[:, 1].max(), (tag, red)
        lo, hi = orc.global_db_range(m[:, 0], m[:, 1], 100.0)
        assert (rng[0], rng[1]) == (np.float32(lo), np.float32(hi)), (tag, rng, lo, hi)
        lo80, hi80 = orc.global_db_range(m[:, 0], m[:, 1], 80.0)
        assert (rng80[0], rng80[1]) == (np.float32(lo80), np.float32(hi80)), (tag, rng80, lo80, hi80)
        assert nm[0] == m[:, 0].min() and nm[1] == -m[:, 1].max(), (tag, nm)
        for k, (g, im) in enumerate(zip(got[:n], got[n + 5:])):
            assert np.array_equal(im.view(np.uint16), orc.convert_spectrogram_to_img(g, (0, H), (lo, hi), CM_LEN)), (tag, k)

    outs = ([(s, _whole, None) for s in specs] + [(t, _whole, None) for t in (mm, r2, rng_db, rng2, negmax)]
            + [(im, _cols(s.shape[0]), None) for im, s in zip(imgs, specs)])
    replay_protocol(ctx, S, cycles, ins, outs, step, check, "range chain behind mel-banded-2048")


def _three(make):
    return tuple(_dev(make(v)) for v in range(3))


def test_spec_to_img_dev_replay(cycles):  # noqa: F811
    """th_spec_to_img_dev on a changed spec (one dense image, no colour map length)."""
    ctx, S = _on("side")
    T, H = 300, 1025
    specs = [_rand_spec(140 + v, T, H) for v in range(3)]
    buf = torch.empty((T, H), dtype=torch.float32, device=DEV)
    img = torch.empty((H, T), dtype=torch.int16, device=DEV)

    def step():
        ta.api.check(ta.api.lib.th_spec_to_img_dev(ctx.handle, buf.data_ptr(), T, H, 0, H, -100.0, 0.0, 0, img.data_ptr()))

    def check(got, v, tag):
        assert np.array_equal(got[0].view(np.uint16), orc.convert_spectrogram_to_img(specs[v], (0, H), (-100.0, 0.0), None)), tag

    replay_protocol(ctx, S, cycles, [(buf, _three(lambda v: specs[v]))], [(img, _whole, None)], step, check, "th_spec_to_img_dev")


def test_spec_to_img_batch_dev_replay(cycles):  # noqa: F811
    """th_spec_to_img_batch_dev with the range on the host: two images (a row range past the spec's height, the library's padded
    pitch) on changed specs."""
    ctx, S = _on("side")
    shapes = [(300, 1025, 0, 1025, 0), (257, 128, 5, 140, ta.pitch_u16(257))]
    specs = [[_rand_spec(240 + 10 * k + v, T, H) for v in range(3)] for k, (T, H, *_r) in enumerate(shapes)]
    ins = [(torch.empty((T, H), dtype=torch.float32, device=DEV), _three(lambda v: specs[k][v])) for k, (T, H, *_r) in enumerate(shapes)]
    imgs = [torch.empty((i1 - i0, p or T), dtype=torch.int16, device=DEV) for T, H, i0, i1, p in shapes]
    descs = [_ffi.ImgDesc(b.data_ptr(), im.data_ptr(), T, H, i0, i1, 0, p) for (b, _), im, (T, H, i0, i1, p) in zip(ins, imgs, shapes)]

    def check(got, v, tag):
        for k, (T, H, i0, i1, p) in enumerate(shapes):
            assert np.array_equal(got[k].view(np.uint16), orc.convert_spectrogram_to_img(specs[k][v], (i0, i1), (-100.0, 0.0), CM_LEN)), (tag, k)

    replay_protocol(ctx, S, cycles, ins, [(im, _cols(s[0]), None) for im, s in zip(imgs, shapes)],
                    lambda: ctx.spec_to_img_batch(descs, -100.0, 0.0, CM_LEN), check, "th_spec_to_img_batch_dev")


RANGES = ((-100.0, -3.5), (-80.0, 0.0), (-120.5, -10.0))


@pytest.mark.parametrize("where", ["host-range", "device-range"])
def test_spec_to_img_raster_batch_dev_replay(cycles, where):  # noqa: F811
    """th_spec_to_img_raster_batch_dev: the u16 image and every level-0 RGBA tile of a changed spec; with d_range the range
    changes with the spec (a replay reads it from the device), with the host range it is the captured one."""
    ctx, S = _on("side")
    cmap = _cmap()
    T, H = 700, 347
    specs = [_rand_spec(177 + v, T, H) for v in range(3)]
    ip = ta.pitch_u16(T)
    d_cmap = _dev(np.frombuffer(cmap, np.uint8))
    spec = torch.empty((T, H), dtype=torch.float32, device=DEV)
    d_rng = torch.empty(2, dtype=torch.float32, device=DEV)
    ranges = RANGES if where == "device-range" else (RANGES[0],) * 3
    ins = [(spec, _three(lambda v: specs[v])), (d_rng, _three(lambda v: np.array(ranges[v], np.float32)))]
    img = torch.empty((H, ip), dtype=torch.int16, device=DEV)
    geoms, offs, total = _tile_layout(T, H)
    tiles = torch.empty(total * 4, dtype=torch.uint8, device=DEV)
    descs = ctx.make_img_tiles_descs([(_ffi.ImgDesc(spec.data_ptr(), img.data_ptr(), T, H, 0, H, 0, ip), [tiles.data_ptr() + 4 * o for o in offs])])

    def step():
        if where == "device-range":
            ctx.spec_to_img_raster_batch(descs, d_cmap.data_ptr(), CM_LEN, d_range=d_rng.data_ptr())
        else:
            ctx.spec_to_img_raster_batch(descs, d_cmap.data_ptr(), CM_LEN, ranges[0][0], ranges[0][1])

    def check(got, v, tag):
        want = orc.convert_spectrogram_to_img(specs[v], (0, H), ranges[v], CM_LEN)
        assert np.array_equal(got[0].view(np.uint16), want), tag
        for (tx, ty, g), o in zip(geoms, offs):
            assert got[1][4 * o:4 * (o + g.width * g.height)].tobytes() == orc.encode_spectrogram_tile(want, cmap, 1, 0, 0, tx, ty)[40:], (tag, tx, ty)

    replay_protocol(ctx, S, cycles, ins, [(img, _cols(T), None), (tiles, _whole, None)], step, check, f"th_spec_to_img_raster_batch_dev, {where}")


def test_raster_tiles_dev_replay(cycles):  # noqa: F811
    """th_raster_tiles_dev on a changed image: level-0 tiles packed back to back, RGBA bit for bit."""
    ctx, S = _on("side")
    cmap = _cmap()
    d_cmap = _dev(np.frombuffer(cmap, np.uint8))
    W, H = 1100, 700
    img0, (buf, src0), tiles, geoms, offs, descs = _raster_setup(W, H, 9)
    imgs = [img0] + [np.random.default_rng(90 + v).integers(0, 65536, (H, W), dtype=np.uint16) for v in (1, 2)]
    pitch = buf.shape[1]
    srcs = (src0,) + tuple(_dev(np.pad(im, ((0, 0), (0, pitch - W))).view(np.int16)) for im in imgs[1:])

    def check(got, v, tag):
        for (tx, ty, g), o in zip(geoms, offs):
            assert got[0][4 * o:4 * (o + g.width * g.height)].tobytes() == orc.encode_spectrogram_tile(imgs[v], cmap, 1, 0, 0, tx, ty)[40:], (tag, tx, ty)

    # (the tiles start one pixel into their buffer: that pixel is not the library's)
    replay_protocol(ctx, S, cycles, [(buf, srcs)], [(tiles, _whole, lambda a: a[:4])], lambda: ctx.raster_tiles(descs, d_cmap.data_ptr(), CM_LEN),
                    check, "th_raster_tiles_dev")


# ---------------------------------------------------------------- waveform entries and the copy (side stream)
def test_waveform_tiles_dev_replay(cycles):  # noqa: F811
    """th_waveform_tiles_dev: tiles of several levels (each level's first and last, partial tile) of a changed waveform; min / max
    bit-exact, the mean as in tests/test_gpu_streams.py."""
    ctx, S = _on("side")
    xs = [synth_track(60 + v, 48000, N_WAV) for v in range(3)]
    buf = torch.empty(N_WAV, dtype=torch.float32, device=DEV)
    jobs = []
    for level in (0, 3, 5, 9, 16):
        n_tiles = -(-(-(-N_WAV // (1 << level))) // 1024)
        for tile in sorted({0, n_tiles - 1}):
            start, bins, _ = ta.waveform_tile_geometry(N_WAV, level, tile)
            jobs.append((level, tile, start, bins, torch.empty((bins, 3), dtype=torch.float32, device=DEV)))
    descs = [_ffi.WaveDesc(buf.data_ptr(), o.data_ptr(), N_WAV, start, level, bins) for level, tile, start, bins, o in jobs]

    def check(got, v, tag):
        peak = float(np.abs(xs[v]).max())
        for (level, tile, *_r), g in zip(jobs, got):
            _assert_bins(g, _want_bins(xs[v], level, tile), level, peak, (tag, level, tile))

    replay_protocol(ctx, S, cycles, [(buf, _three(lambda v: xs[v]))], [(j[-1], _whole, None) for j in jobs], lambda: ctx.waveform_tiles(descs), check,
                    "th_waveform_tiles_dev")


def test_waveform_pyramid_dev_replay(cycles):  # noqa: F811
    """th_waveform_pyramid_dev (base pass + tree passes) on two channels, first_level 0 and 2, of changed waveforms: every level's
    first and last tile."""
    ctx, S = _on("side")
    lens, firsts, n_levels = (N_WAV, 70_001), (0, 2), 15
    xs = [[synth_track(80 + 10 * i + v, 44100, n) for v in range(3)] for i, n in enumerate(lens)]
    ins = [(torch.empty(n, dtype=torch.float32, device=DEV), _three(lambda v: xs[i][v])) for i, n in enumerate(lens)]
    base = [ta.api.pyramid_offset(n, f) for n, f in zip(lens, firsts)]
    outs = [torch.empty(ta.api.pyramid_offset(n, n_levels) - b, dtype=torch.float32, device=DEV) for n, b in zip(lens, base)]
    descs = [_ffi.PyramidDesc(b.data_ptr(), o.data_ptr(), n, n_levels, f) for (b, _), o, n, f in zip(ins, outs, lens, firsts)]

    # (a level starts on a 128-byte boundary: the floats between two levels are never written)
    spans = [[(ta.api.pyramid_offset(n, lv) - b, 3 * ta.api.pyramid_bins(n, lv)) for lv in range(f, n_levels)] for n, f, b in zip(lens, firsts, base)]

    def levels(i):
        return lambda a: np.concatenate([a[o:o + m] for o, m in spans[i]])

    def check(got, v, tag):
        for i, (n, f, flat) in enumerate(zip(lens, firsts, got)):
            x = xs[i][v]
            peak, pos = float(np.abs(x).max()), 0
            for level, (_, m) in zip(range(f, n_levels), spans[i]):
                lv = flat[pos:pos + m].reshape(-1, 3)
                pos += m
                n_tiles = -(-lv.shape[0] // 1024)
                for t in sorted({0, n_tiles - 1}):
                    _assert_bins(lv[1024 * t:1024 * (t + 1)], _want_bins(x, level, t), level, peak, (tag, n, level, t))

    replay_protocol(ctx, S, cycles, ins, [(o, levels(i), None) for i, o in enumerate(outs)], lambda: ctx.waveform_pyramid_dev(descs), check,
                    "th_waveform_pyramid_dev")


def test_dev_copy_replay(cycles):  # noqa: F811
    """th_dev_copy of 257 lanes between 16-byte offsets of larger buffers: the bytes of the replay's own source, nothing outside."""
    ctx, S = _on("side")
    size, pad, so, do = 4096 + 16, 256, 16, 48
    g = torch.Generator(device=DEV)
    g.manual_seed(size)
    reals = tuple(torch.randint(0, 256, (size + pad,), dtype=torch.uint8, device=DEV, generator=g) for _ in range(3))
    src = torch.empty_like(reals[0])
    dst = torch.empty(size + pad, dtype=torch.uint8, device=DEV)

    def check(got, v, tag):
        assert np.array_equal(got[0], reals[v][so:so + size].cpu().numpy()), tag

    replay_protocol(ctx, S, cycles, [(src, reals)], [(dst, lambda a: a[do:do + size], lambda a: np.concatenate([a[:do], a[do + size:]]))],
                    lambda: ctx.dev_copy(dst.data_ptr() + do, src.data_ptr() + so, size), check, "th_dev_copy")


# ---------------------------------------------------------------- the refusal the header documents
def _refusal_child():
    """One process, one side-stream context: (i) a cold th_calc_spec_batch_dev inside a capture, (ii) a cold th_channel_stats_dev
    inside a capture, (iii) a proper capture and replay afterwards.  Prints one JSON line."""
    import ctypes as C
    lib = ta.api.lib
    import traceback
    out = {}
    try:
        torch.cuda.init()
        S = torch.cuda.Stream(DEV)
        ctx = ta.Context(0, S.cuda_stream)

        def err():
            return (lib.th_last_error() or b"").decode()[:200]

        def refused(call):
            """call() inside a capture -> its status, th_ctx_capture_end's status, whether a graph came back, the two messages"""
            h = C.c_void_p()
            assert lib.th_ctx_capture_begin(ctx.handle) == 0, err()
            rc = call()
            e1 = err() if rc else ""
            rc_end = lib.th_ctx_capture_end(ctx.handle, C.byref(h))
            e2 = err() if rc_end else ""
            got_graph = bool(h.value)
            if got_graph:
                lib.th_graph_destroy(h)
            return {"call": rc, "end": rc_end, "graph": got_graph, "call_error": e1, "end_error": e2}

        def rows_right(route, specs, mm, want):
            try:
                _check_specs(route, [s.cpu().numpy() for s in specs], mm.cpu().numpy(), want, ROUTES[route][8])
                return True
            except AssertionError as e:
                return str(e)[:300]

        def load(ins, specs, mm):
            with torch.cuda.stream(S):
                for b, src in ins:
                    b.copy_(src)
                for o in specs + [mm]:
                    _bits(o).fill_(SENT1[o.dtype])
            torch.cuda.synchronize()

        # (i) descriptors this plan has never seen: the call has to upload its tables, which capture refuses
        route = "wave-2048"
        wavs, want, _ = _route_oracle(route)
        plan = _make_plan(ctx, route)
        ins, specs, mm, descs = _spec_buffers(plan, wavs)
        load(ins, specs, mm)
        out["i"] = refused(lambda: lib.th_calc_spec_batch_dev(plan.handle, descs, len(descs), mm.data_ptr()))
        rc = lib.th_calc_spec_batch_dev(plan.handle, descs, len(descs), mm.data_ptr())   # the same call, directly
        out["i"]["direct"] = rc
        out["i"]["direct_error"] = err() if rc else ""
        torch.cuda.synchronize()
        out["i"]["rows"] = rows_right(route, specs, mm, want) if rc == 0 else False

        # (ii) an entry that returns to host memory (the context's tables are cold as well)
        rng = np.random.default_rng(17)
        xs = [rng.uniform(-1, 1, n).astype(np.float32) for n in (5, 4097, 300_001)]
        xs[2][1234] = -1.5
        bufs = [_dev(x) for x in xs]
        sd = (_ffi.StatsDesc * len(xs))(*[_ffi.StatsDesc(b.data_ptr(), x.size) for b, x in zip(bufs, xs)])
        ss, pk = np.zeros(len(xs), np.float32), np.zeros(len(xs), np.float32)
        f32p = C.POINTER(C.c_float)
        torch.cuda.synchronize()
        stats = lambda: lib.th_channel_stats_dev(ctx.handle, sd, len(sd), ss.ctypes.data_as(f32p), pk.ctypes.data_as(f32p))  # noqa: E731
        out["ii"] = refused(stats)
        rc = stats()
        out["ii"]["direct"] = rc
        out["ii"]["direct_error"] = err() if rc else ""
        out["ii"]["stats"] = rc == 0 and all(p == orc.abs_max(x) and abs(s - orc.sum_squares(x)) <= CHANNEL_STATS_SUM_REL * max(orc.sum_squares(x), 1e-30)
                                              for x, s, p in zip(xs, ss, pk))

        # (iii) a proper capture on the same context: a further plan, its step run once directly, then captured and replayed
        route3 = "multi-512"
        wavs3, want3, _ = _route_oracle(route3)
        plan3 = _make_plan(ctx, route3)
        ins3, specs3, mm3, descs3 = _spec_buffers(plan3, wavs3)
        load(ins3, specs3, mm3)
        step = lambda: plan3.calc_spec_batch_dev(descs3, mm3.data_ptr())  # noqa: E731
        step()
        torch.cuda.synchronize()
        out["iii"] = {"direct_rows": rows_right(route3, specs3, mm3, want3)}
        graph = ctx.capture(step)
        load(ins3, specs3, mm3)
        graph.launch()
        torch.cuda.synchronize()
        out["iii"]["replay_rows"] = rows_right(route3, specs3, mm3, want3)
        graph.close()
        plan.close()
        plan3.close()
        ctx.close()
    except BaseException:
        out["exception"] = traceback.format_exc()[-1500:]
    finally:
        print(json.dumps(out), flush=True)


def test_refused_capture_leaves_library_and_context_usable():
    """A call that needs a table upload or a scratch allocation while capturing fails with TH_ERR_HIP, th_ctx_capture_end then
    returns an error and *out == NULL (include/thesia_amd.h) — and the library goes on: the same call made directly gives the
    right rows, a later capture on the same context works.  (The library refuses such a call itself, before the HIP call that
    would invalidate the capture: a stream whose capture HIP invalidated stays unusable after hipStreamEndCapture, and every
    later call on a context of that stream failed.)  One fresh child process, run once."""
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_gpu_graphs import _refusal_child; _refusal_child()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, f"the child ended with {r.returncode}: {r.stderr[-2000:]}"
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(rec, indent=1), file=sys.stderr)
    assert "exception" not in rec, rec["exception"]
    for k in ("i", "ii"):
        assert rec[k]["call"] == -3, (k, rec[k])                                  # TH_ERR_HIP
        assert rec[k]["end"] != 0 and not rec[k]["graph"], (k, rec[k])
        assert rec[k]["direct"] == 0, (k, rec[k])                                 # (no stale HIP error)
    assert rec["i"]["rows"] is True, rec["i"]
    assert rec["ii"]["stats"] is True, rec["ii"]
    assert rec["iii"]["direct_rows"] is True and rec["iii"]["replay_rows"] is True, rec["iii"]
