"""The host side of an STFT plan, on the CPU: the launch planner (plan_stft_launch) and the plan tables (build_mel_mfma,
build_mel_rows, build_wave_window; thesia_amd/csrc/stft_plan.h) are compiled into the emulator library as th_calc_spec_batch_dev
and th_plan_create call them.  A mistake in the planner does not crash a launch: it leaves spectrogram rows unwritten or written
twice — here every (channel, frame) pair is accounted for, for routes given by hand (the combinations resolve_route produces)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
GENERIC, BLUESTEIN, WAVE, WAVE_MULTI, BLOCK, SUBWAVE = range(6)  # StftRoute::Main
MEL_MFMA = 3                                                      # StftRoute::MelSecond::Mfma
MEL_TILE_FRAMES = 128
N_CU = 256


@pytest.fixture(scope="module")
def emu():
    lib = C.CDLL(os.path.join(HERE, "emu", "_build", "libemu_stft.so"))
    lib.emu_blob.restype = C.c_uint64
    lib.emu_blob.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    lib.emu_blob_free.argtypes = [C.c_void_p]
    lib.emu_plan_launch.restype = C.c_void_p
    lib.emu_plan_launch.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_int32), C.c_uint32, C.c_int32, C.POINTER(C.c_uint64), C.c_uint64]
    lib.emu_mel_tables.restype = C.c_void_p
    lib.emu_mel_tables.argtypes = [C.c_uint32] * 3
    lib.emu_wave_window.restype = C.c_void_p
    lib.emu_wave_window.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_int32]
    return lib


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


# (win, hop, n_fft, n_mel, main, mel_second, phase_mode, waves, tail_guard, edges_in_wave, block_plan)
ROUTES = {
    "wave_2048_edges_in_wave": (2048, 512, 2048, 0, WAVE, 0, 0, 12, 0, 1, 0),
    "wave_2048_phase1": (1920, 480, 2048, 0, WAVE, 0, 1, 12, 0, 0, 0),
    "wave_2048_phase2": (1764, 441, 2048, 0, WAVE, 0, 2, 12, 0, 0, 0),
    "multi_512_tail_guard2": (440, 110, 512, 0, WAVE_MULTI, 0, 0, 12, 2, 1, 0),  # hop % 4 == 2: stft_wave_multi_tail_guard
    "multi_512_tail_guard0": (512, 128, 512, 0, WAVE_MULTI, 0, 0, 16, 0, 1, 0),
    "block_8192": (8192, 2048, 8192, 0, BLOCK, 0, 0, 12, 0, 0, 1),
    "wave_2048_mel_mfma": (2048, 512, 2048, 256, WAVE, MEL_MFMA, 0, 12, 0, 0, 0),
    "generic_256": (256, 64, 256, 0, GENERIC, 0, 0, 0, 0, 0, 0),
}


def _lengths(n_fft):
    return [1, n_fft - 1, n_fft, n_fft + 1, 3 * n_fft + 7, 30 * 48000]


def _batches(n_fft):
    out = [("one_%d" % n, [n]) for n in _lengths(n_fft)]
    rng = np.random.default_rng(n_fft)
    out.append(("128_mixed", [int(n) for n in rng.permutation(np.resize(_lengths(n_fft), 128))]))
    return out


def _launch(lib, route, lens):
    win, hop, n_fft, n_mel, main, second, phase, waves, guard, edges, block = route
    r = (C.c_int32 * 9)(main, 0, second, phase, waves, guard, edges, block, 0)
    ns = (C.c_uint64 * len(lens))(*lens)
    h = lib.emu_plan_launch(win, hop, n_fft, n_mel, r, N_CU, 0, ns, len(lens))
    u64, u32 = np.uint64, np.uint32
    b = _blobs(lib, h, [u64, u64, u64, u32, u32, u32, u64, u32, u64, u64])
    names = ["err", "fpt", "phased", "sweep", "tiles", "edge_tiles", "mel_tiles", "amp_rows", "all_in_wave", "edge_fpt"]
    L = dict(zip(names, (int(v) for v in b[0].view(np.int64))))
    L.update(jobs=b[1].reshape(-1, 6).astype(np.int64), edge=b[2].reshape(-1, 6).astype(np.int64), tile_start=b[3].astype(np.int64),
             edge_start=b[4].astype(np.int64), chunk_tab=b[5].reshape(-1, 2).astype(np.int64), mel_jobs=b[6].reshape(-1, 3).astype(np.int64),
             mel_start=b[7].astype(np.int64), amp_row0=b[8].astype(np.int64), post=b[9].reshape(-1, 3).astype(np.int64))
    return L


N_SAMPLES, N_FRAMES, F_BEGIN, F_END, MM, EDGE = range(6)  # columns of a job row


@pytest.mark.parametrize("name", list(ROUTES))
def test_launch_plan_covers_every_frame_once(emu, name):
    route = ROUTES[name]
    win, hop, n_fft, n_mel, main, second, phase, waves, guard, edges, block = route
    wave = main not in (GENERIC, BLUESTEIN)
    pad_left = (n_fft - win) // 2
    for bname, lens in _batches(n_fft):
        what = "%s / %s" % (name, bname)
        L = _launch(emu, route, lens)
        assert L["err"] == 0, what
        T = [orc.stft_n_frames(n, win, hop) for n in lens]
        jobs, edge, fpt = L["jobs"], L["edge"], L["fpt"]
        assert L["phased"] == phase and L["edge_fpt"] == 1 and fpt >= 1, what
        for rows in (jobs, edge):  # a job describes its channel
            for j in rows:
                assert j[N_SAMPLES] == lens[j[MM]] and j[N_FRAMES] == T[j[MM]] and 0 <= j[F_BEGIN] < j[F_END] <= T[j[MM]], what
        if not wave:
            assert not len(edge) and not jobs[:, EDGE].any(), what

        # 1. every (channel, frame) exactly once: wave chunks / generic tiles of the main launch + the edge launch's tiles
        seen = [np.zeros(t, np.int32) for t in T]
        assert len(L["tile_start"]) == len(jobs) + 1 and L["tile_start"][-1] == L["tiles"], what
        assert len(L["edge_start"]) == len(edge) + 1 and L["edge_start"][-1] == L["edge_tiles"], what
        if wave:
            tab = L["chunk_tab"]
            assert len(tab) == L["tiles"], what
            # 3. rows name a valid job and a first frame inside it; consecutive rows of a job are frames_per_tile apart
            assert ((tab[:, 0] >= 0) & (tab[:, 0] < len(jobs))).all(), what
            step = np.where(jobs[tab[:, 0], EDGE] != 0, 1, fpt)
            assert ((tab[:, 1] >= jobs[tab[:, 0], F_BEGIN]) & (tab[:, 1] < jobs[tab[:, 0], F_END])).all(), what
            same = tab[1:, 0] == tab[:-1, 0]
            assert (tab[1:, 0] >= tab[:-1, 0]).all() and ((tab[1:, 1] - tab[:-1, 1])[same] == step[1:][same]).all(), what
            first = np.r_[len(tab) > 0, ~same][:len(tab)]
            assert (tab[first, 1] == jobs[tab[first, 0], F_BEGIN]).all(), what
            for (j, f0), st in zip(tab, step):
                seen[jobs[j, MM]][f0:min(f0 + st, jobs[j, F_END])] += 1
        else:
            assert not len(L["chunk_tab"]), what
            for j, (t0, t1) in zip(jobs, zip(L["tile_start"][:-1], L["tile_start"][1:])):
                assert t1 - t0 == -(-(j[F_END] - j[F_BEGIN]) // fpt), what
                for t in range(t1 - t0):
                    seen[j[MM]][j[F_BEGIN] + t * fpt:min(j[F_BEGIN] + (t + 1) * fpt, j[F_END])] += 1
        for j, (t0, t1) in zip(edge, zip(L["edge_start"][:-1], L["edge_start"][1:])):
            assert t1 - t0 == j[F_END] - j[F_BEGIN], what  # one frame per tile
            seen[j[MM]][j[F_BEGIN]:j[F_END]] += 1
        for i, s in enumerate(seen):
            assert (s == 1).all(), "%s: channel %d (%d samples) frames %s covered %s times" % (what, i, lens[i], np.flatnonzero(s != 1)[:8], s[s != 1][:8])
        assert sum(int(s.sum()) for s in seen) == sum(T), what

        if wave:
            # 2. an interior frame's n_fft-sample span lies inside the channel (the wave kernels load it unconditionally)
            for j in jobs[jobs[:, EDGE] == 0]:
                f = np.arange(j[F_BEGIN], j[F_END])
                if phase == 0:
                    s0 = f * hop - win // 2 - pad_left
                else:  # the 128-sample grid point at or below the frame's first window sample
                    s0 = (f * hop - win // 2) // 128 * 128
                assert (s0 >= 0).all() and (s0 + n_fft <= j[N_SAMPLES] - guard).all(), what
            if phase == 1:
                inner = jobs[tab[:, 0], EDGE] == 0
                assert fpt % 4 == 0 and (((tab[inner, 1] * hop - win // 2) % 128) == 0).all(), what
            # boundary frames inside the wave launch: only where the route says so, and only for channels of n_fft samples and more
            assert edges or not jobs[:, EDGE].any(), what
            assert (jobs[jobs[:, EDGE] != 0, N_SAMPLES] >= n_fft).all(), what
            # 4. wave_post_kernel's ranges: one per channel present, ascending, a partition of the tiles
            post = L["post"]
            present = sorted(set(jobs[:, MM].tolist()))
            assert post[:, 2].tolist() == present, what
            if len(post):
                assert post[0, 0] == 0 and post[-1, 1] == L["tiles"] and (post[1:, 0] == post[:-1, 1]).all() and (post[:, 1] > post[:, 0]).all(), what
                for t0, t1, mm in post:
                    assert (jobs[tab[t0:t1, 0], MM] == mm).all(), what
            # 6. channels shorter than n_fft: every frame in the generic kernel's edge jobs
            for i, n in enumerate(lens):
                if n < n_fft:
                    assert not (jobs[:, MM] == i).any() and sum(j[F_END] - j[F_BEGIN] for j in edge if j[MM] == i) == T[i], what
            assert L["all_in_wave"] == int(not second and not len(edge) and L["tiles"] > 0), what
        else:
            assert not len(L["post"]) and not L["all_in_wave"], what

        # 5. a second mel kernel: one job per channel with interior frames, over the interior job's frames; amplitude rows packed
        if second:
            inner = jobs[jobs[:, EDGE] == 0]
            mj = L["mel_jobs"]
            assert mj.tolist() == inner[:, [F_BEGIN, F_END, MM]].tolist() and len(set(mj[:, 2].tolist())) == len(mj), what
            rows = np.cumsum([0] + [T[i] for i in mj[:, 2]])
            assert L["amp_row0"][mj[:, 2]].tolist() == rows[:-1].tolist() and L["amp_rows"] == rows[-1], what
            tiles = np.cumsum([0] + [-(-(b - a) // MEL_TILE_FRAMES) for a, b, _ in mj])
            assert L["mel_start"].tolist() == tiles.tolist() and L["mel_tiles"] == tiles[-1], what
        else:
            assert not len(L["mel_jobs"]) and L["amp_rows"] == 0 and L["mel_tiles"] == 0, what


def test_launch_plan_reports_channel_errors(emu):
    """a channel the kernels' 32-bit sample indices cannot hold is refused while the channels are walked (TH_ERR_INVALID_ARG)"""
    L = _launch(emu, ROUTES["wave_2048_edges_in_wave"], [4096, 2 ** 31])
    assert L["err"] == -1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# (the dense 32768-point default bank is 365 MB: too large for a CPU test); the last two: n_fft 512 banks of filters at most 8 bins
# wide (the 8 kHz default count; 256 mels at 48 kHz), where the mel_rows table applies
@pytest.mark.parametrize("sr,n_fft,n_mel", [(48000, 2048, 256), (16000, 512, 64), (96000, 4096, 0), (48000, 8192, 0), (8000, 512, 0), (48000, 512, 256)])
def test_mel_tables_decode_to_the_filterbank(emu, sr, n_fft, n_mel):
    u32, f32 = np.uint32, np.float32
    fb, info, lo, hi, band, sl, bt, rows = _blobs(emu, emu.emu_mel_tables(sr, n_fft, n_mel), [f32, u32, u32, u32, u32, u32, f32, u32])
    n_mel_, kblocks, ntiles, zero_block, n_slices, rows_ok, rows_groups = (int(v) for v in info)
    n_freq = n_fft // 2 + 1
    assert n_mel_ == (n_mel or orc.mel_default_n_mel(sr, n_fft))
    n_mel = n_mel_
    fb = fb.reshape(n_freq, n_mel)
    assert np.array_equal(_bits(fb), _bits(orc.calc_mel_fb(sr, n_fft, n_mel)))
    # per-mel non-zero ranges
    for m in range(n_mel):
        nz = np.flatnonzero(fb[:, m])
        assert (lo[m], hi[m]) == ((nz[0], nz[-1] + 1) if len(nz) else (0, 0))
    # MFMA operand-order blocks, decoded through the per-tile bands: the filterbank bit for bit, zero elsewhere
    assert kblocks == -(-n_freq // 16) and ntiles == -(-n_mel // 16) and len(band) == 3 * ntiles
    assert len(bt) == 256 * (zero_block + 1) and not bt[256 * zero_block:].view(u32).any()
    dense = np.zeros((16 * kblocks, 16 * ntiles), f32)
    blocks = bt.reshape(-1, 64, 4)  # [block][lane][step]
    nxt = 0
    lane = np.arange(64)
    for j in range(ntiles):
        klo, khi, b0 = (int(v) for v in band[3 * j:3 * j + 3])
        assert klo <= khi <= kblocks and b0 == nxt
        nxt += khi - klo
        for kb in range(klo, khi):
            blk = blocks[b0 + kb - klo]
            for st in range(4):
                dense[16 * kb + 4 * (lane >> 4) + st, 16 * j + (lane & 15)] = blk[:, st]
    assert nxt == zero_block
    want = np.zeros_like(dense)
    want[:n_freq, :n_mel] = fb
    assert np.array_equal(_bits(dense), _bits(want))
    # slices of the tile range: contiguous, covering [0, n_tiles)
    assert len(sl) == n_slices + 1 and 1 <= n_slices <= 6 and sl[0] == 0 and sl[-1] == ntiles and (np.diff(sl.astype(np.int64)) > 0).all()
    # mel_rows_kernel's per-mel table, where the bank has its shape
    W = 8
    applies = kblocks <= 17 and n_freq - 1 + W <= 16 * 17 + 4 and int((hi.astype(np.int64) - lo).max()) <= W and -(-n_mel // 64) <= 8
    assert bool(rows_ok) == applies
    if rows_ok:
        assert rows_groups == -(-n_mel // 64) and len(rows) == rows_groups * (W + 1) * 64
        tab = rows.reshape(rows_groups, W + 1, 64)
        dec = np.zeros((n_freq + W, 64 * rows_groups), u32)
        for g in range(rows_groups):
            for t in range(W):
                dec[tab[g, 0] + t, 64 * g + np.arange(64)] |= tab[g, 1 + t]  # (weights past a filter's end are zero words)
        want = np.zeros_like(dec)
        want[:n_freq, :n_mel] = _bits(fb)
        assert np.array_equal(dec, want)
        per_mel = tab.transpose(0, 2, 1).reshape(-1, W + 1)  # [mel][first bin, weights]
        assert (per_mel[:n_mel, 0] == lo).all() and not per_mel[n_mel:].any()
    else:
        assert not len(rows)
    if (sr, n_fft) in ((8000, 512), (48000, 512)):
        assert rows_ok  # (so the decoding above has run)


@pytest.mark.parametrize("win,hop,n_fft", [(2048, 512, 2048), (1920, 480, 2048), (1764, 441, 2048)])
def test_wave_window_tables(emu, win, hop, n_fft):
    """wtab: the window behind pad_left zeros; phased (mode 1): behind 96; dynamic (modes 2, 3): behind 128, and again one sample
    earlier behind the even table — all 0.5 * 2^32 * calc_normalized_win"""
    w = orc.calc_normalized_win(win, n_fft)
    want = (np.float32(0.5 * 2.0 ** 32) * w).astype(np.float32)
    pad_left = (n_fft - win) // 2

    def tables(mode):
        return _blobs(emu, emu.emu_wave_window(w.ctypes.data_as(C.POINTER(C.c_float)), win, n_fft, mode), [np.float32, np.float32])

    def placed(total, *offsets):
        out = np.zeros(total, np.float32)
        for o, src in offsets:
            out[o:o + len(src)] = src
        return out

    for mode in (0, 1, 2, 3):
        wtab, ph = tables(mode)
        assert np.array_equal(_bits(wtab), _bits(placed(n_fft, (pad_left, want))))
        if mode == 0:
            assert not len(ph)
        elif mode == 1:
            assert np.array_equal(_bits(ph), _bits(placed(96 + n_fft, (96, want))))
        else:  # odd table: pairs (t0[2n+1], t0[2n+2]) of t0 = the window at offset 0
            assert np.array_equal(_bits(ph), _bits(placed(2 * (128 + n_fft), (128, want), (128 + n_fft + 128, want[1:]))))
