"""The host side of the export and loudness-meter readers, on the CPU: plan_export / bind_export and plan_meters / bind_meters /
meter_results (thesia_amd/csrc/reader_plan.h) are compiled into the emulator library as export_run and meters_run call them.  A mistake
in the piece cutting does not crash a launch: it leaves output bytes unwritten, written twice, or read by a 16-byte load outside what
the resampler wrote — here every byte, frame, chunk and scratch float is accounted for, nothing is allocated, so sizes are free.
The piece boundaries of the fixed cases are pinned to tests/golden/export_plan_cases.json, recorded from the loop export_run had
before the planner was split off."""
import ctypes as C
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import thesia_amd as ta
from tests import loudness_meter_ref as mref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "export_plan_cases.json")
PIECE = 32 << 20                       # TH_EXPORT_PIECE_BYTES
SCRATCH_MAX = 2 * PIECE + (64 << 10)   # RESAMPLE_SCRATCH_MAX
S16, S24, F32 = ta.api.PCM_S16, ta.api.PCM_S24, ta.api.PCM_F32
BPS = {S16: 2, S24: 3, F32: 4}
ERR_INVALID_ARG = ta._ffi.ERR_INVALID_ARG
U64 = np.uint64


@pytest.fixture(scope="module")
def emu():
    lib = C.CDLL(os.path.join(HERE, "emu", "_build", "libemu_stft.so"))
    p64 = C.POINTER(C.c_uint64)
    lib.emu_blob.restype = C.c_uint64
    lib.emu_blob.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    lib.emu_blob_free.argtypes = [C.c_void_p]
    for name, args in (("emu_plan_export", [p64, C.c_uint64]), ("emu_bind_export", [p64, C.c_uint64, p64, p64, C.c_uint64]),
                       ("emu_plan_meters", [p64, C.c_uint64]), ("emu_bind_meters", [p64, C.c_uint64, C.c_uint64, p64, C.c_uint64]),
                       ("emu_meter_results", [p64, C.c_uint64, C.c_void_p, C.c_uint64])):
        getattr(lib, name).restype = C.c_void_p
        getattr(lib, name).argtypes = args
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


def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


# ---------------------------------------------------------------------------------------------------------------- export
def export_chunk_frames(n_ch):
    return (4096 // n_ch) & ~3 or 4


def export_n_chunks(f0, f1, n_ch):
    F = export_chunk_frames(n_ch)
    return (f1 - 1) // F - f0 // F + 1 if f1 > f0 else 0


def n_out_of(n_in, sr_in, sr_out):
    r = Fraction(sr_out, sr_in)
    return -(-n_in * r.numerator // r.denominator)


def req(n_ch, n_in, sr, fmt, s0=0, s1=None, sr_out=None, dither=0, seed=0):
    """one request on a track of n_ch channels of n_in samples at sr: frames [s0, s1) at sr_out (s1 None: to the end)"""
    sr_out = sr_out or sr
    n = n_in if sr_out == sr else n_out_of(n_in, sr, sr_out)
    s1 = n if s1 is None else s1
    assert 0 <= s0 <= s1 <= n
    return dict(n_ch=n_ch, n_in=n_in, sr_in=sr, sr_out=sr_out, format=fmt, dither=dither, seed=seed, s0=s0, s1=s1, n=n)


def layout(reqs, first_offset=0):
    """export_layout: offsets that are multiples of 16 (first_offset: a single request behind a WAV header), the pad up to the next"""
    rows, at = [], first_offset
    for i, r in enumerate(reqs):
        n_bytes = (r["s1"] - r["s0"]) * r["n_ch"] * BPS[r["format"]]
        end = at + n_bytes
        nxt = (end + 15) & ~15
        pad = nxt - end if i + 1 < len(reqs) else 0
        rows.append([r["n_ch"], r["n_in"], r["sr_in"], r["sr_out"], r["format"], r["dither"], r["seed"], r["s0"], r["s1"], at, pad])
        at = nxt
    return np.array(rows, U64).reshape(-1, 11)


N_CH, N_IN, SR_IN, SR_OUT, FORMAT, DITHER, SEED, S0, S1, OFFSET, PAD = range(11)                         # columns of a request row
(J_REQ, J_F0, J_F1, J_N, J_NCH, J_FORMAT, J_DITHER, J_SEED, J_FIRST_CHUNK, J_PAD, J_STAGE, J_RESAMPLED, J_HULL0, J_STRIDE, J_SCRATCH,
 J_PTR) = range(16)                                                                                       # of a job row
R_JA, R_JB, R_NIN, R_STRIDE, R_NCH, R_NSB, R_FIRST_BLOCK = range(7)                                      # of a resample job row
P_JOB0, P_JOB1, P_CHUNKS, P_STAGE, P_RUN0, P_RUN1, P_RJOB0, P_RJOB1, P_RBLOCKS, P_SR_IN, P_SR_OUT, P_SCRATCH = range(12)  # of a piece row


def plan(lib, rows):
    b = _blobs(lib, lib.emu_plan_export(_p64(rows), len(rows)), [U64, np.uint8, U64, U64, U64, U64, U64, U64])
    names = ["err", "n_ptrs", "o_rjobs", "o_ptrs", "tab_bytes", "stage_need0", "stage_need1", "scratch_need"]
    p = dict(zip(names, (int(v) for v in b[0].view(np.int64))))
    i64 = lambda a, w: a.reshape(-1, w).astype(np.int64)  # noqa: E731
    p.update(text=b[1].tobytes().decode(), jobs=i64(b[2], 16), rjobs=i64(b[3], 7), pieces=i64(b[4], 12), runs=i64(b[5], 3),
             ptr0=b[6].astype(np.int64), per_req=i64(b[7], 3))
    return p


def check_export_plan(rows, p, what):
    rows = rows.astype(np.int64)
    assert p["err"] == 0, (what, p["text"])
    jobs, rjobs, pieces, runs = p["jobs"], p["rjobs"], p["pieces"], p["runs"]
    fbytes = rows[:, N_CH] * np.array([BPS[int(f)] for f in rows[:, FORMAT]], np.int64) if len(rows) else np.zeros(0, np.int64)
    resampled = rows[:, SR_IN] != rows[:, SR_OUT]
    # per request: its jobs in order tile [s0, s1) exactly once; the pad is on the last one
    for i, r in enumerate(rows):
        mine = jobs[jobs[:, J_REQ] == i]
        if r[S0] == r[S1]:
            assert not len(mine), what
            continue
        assert len(mine) and mine[0, J_F0] == r[S0] and mine[-1, J_F1] == r[S1], what
        assert (mine[1:, J_F0] == mine[:-1, J_F1]).all() and (mine[:, J_F1] > mine[:, J_F0]).all(), what
        assert (mine[:-1, J_PAD] == 0).all() and mine[-1, J_PAD] == r[PAD], what
        n = p["per_req"][i, 0] if resampled[i] else r[N_IN]
        assert (mine[:, J_N] == n).all() and (mine[:, J_RESAMPLED] == resampled[i]).all(), what
        for col_j, col_r in ((J_NCH, N_CH), (J_FORMAT, FORMAT), (J_DITHER, DITHER), (J_SEED, SEED)):
            assert (mine[:, col_j] == r[col_r]).all(), what
        if resampled[i]:  # every cut other than the request's end lies on the export kernel's chunk grid
            assert (mine[:-1, J_F1] % export_chunk_frames(int(r[N_CH])) == 0).all(), what
    assert (np.diff(jobs[:, J_REQ]) >= 0).all(), what
    job_out = rows[jobs[:, J_REQ], OFFSET] + (jobs[:, J_F0] - rows[jobs[:, J_REQ], S0]) * fbytes[jobs[:, J_REQ]]
    job_bytes = (jobs[:, J_F1] - jobs[:, J_F0]) * fbytes[jobs[:, J_REQ]] + jobs[:, J_PAD]
    # pieces partition the jobs and the resample jobs
    assert len(pieces) == 0 or (pieces[0, P_JOB0] == 0 and pieces[-1, P_JOB1] == len(jobs) and pieces[0, P_RJOB0] == 0
                                and pieces[-1, P_RJOB1] == len(rjobs) and pieces[0, P_RUN0] == 0 and pieces[-1, P_RUN1] == len(runs)), what
    assert (len(pieces) > 0) == (len(jobs) > 0), what
    assert (pieces[1:, P_JOB0] == pieces[:-1, P_JOB1]).all() and (pieces[1:, P_RJOB0] == pieces[:-1, P_RJOB1]).all(), what
    assert (pieces[1:, P_RUN0] == pieces[:-1, P_RUN1]).all(), what
    need = [0, 0, 0]
    for k, pc in enumerate(pieces):
        j0, j1 = pc[P_JOB0], pc[P_JOB1]
        assert j1 > j0 and pc[P_STAGE] <= PIECE + 15, what
        need[k & 1] = max(need[k & 1], pc[P_STAGE])
        need[2] = max(need[2], pc[P_SCRATCH])
        st, by = jobs[j0:j1, J_STAGE], job_bytes[j0:j1]
        assert ((st - job_out[j0:j1]) % 16 == 0).all(), what
        assert (st[1:] >= (st + by)[:-1]).all() and st[0] >= 0 and (st + by)[-1] <= pc[P_STAGE], what
        chunks = np.array([export_n_chunks(int(j[J_F0]), int(j[J_F1]), int(j[J_NCH])) for j in jobs[j0:j1]], np.int64)
        assert (jobs[j0:j1, J_FIRST_CHUNK] == np.cumsum(chunks) - chunks).all() and pc[P_CHUNKS] == chunks.sum(), what
        # every job lies in a run of its piece that carries it to its place in the output
        rr = runs[pc[P_RUN0]:pc[P_RUN1]]
        assert len(rr) and ((rr[:, 0] - rr[:, 1]) % 16 == 0).all() and (rr[:, 2] > 0).all(), what
        assert (rr[1:, 0] >= (rr[:, 0] + rr[:, 2])[:-1]).all() and (rr[:, 0] + rr[:, 2])[-1] <= pc[P_STAGE], what
        at = np.searchsorted(rr[:, 0], st, side="right") - 1
        assert (at >= 0).all() and (st + by <= (rr[:, 0] + rr[:, 2])[at]).all() and (rr[at, 1] - rr[at, 0] == job_out[j0:j1] - st).all(), what
        assert rr[:, 2].sum() == by.sum(), what
        # the resampled jobs of the piece are its resample jobs, in order
        rs = jobs[j0:j1][jobs[j0:j1, J_RESAMPLED] != 0]
        rj = rjobs[pc[P_RJOB0]:pc[P_RJOB1]]
        assert len(rs) == len(rj), what
        if not len(rj):
            assert pc[P_RBLOCKS] == 0 and pc[P_SCRATCH] == 0 and pc[P_SR_OUT] == 0, what
            continue
        rq = rs[:, J_REQ]
        assert (rows[rq, SR_IN] == pc[P_SR_IN]).all() and (rows[rq, SR_OUT] == pc[P_SR_OUT]).all(), what
        n_out, S, per = p["per_req"][rq, 0], p["per_req"][rq, 1], p["per_req"][rq, 2]
        hull0, stride = rs[:, J_HULL0], rs[:, J_STRIDE]
        assert (hull0 % 4 == 0).all() and (stride % 4 == 0).all(), what
        assert (rj[:, R_JA] == hull0).all() and (rj[:, R_STRIDE] == stride).all() and (rj[:, R_NCH] == rs[:, J_NCH]).all(), what
        assert (rj[:, R_NIN] == rows[rq, N_IN]).all(), what
        assert (rj[:, R_JA] <= rs[:, J_F0]).all() and (rj[:, R_JB] >= rs[:, J_F1]).all() and (rj[:, R_JB] <= n_out).all(), what
        assert (rj[:, R_JB] - rj[:, R_JA] <= stride).all() and (((rs[:, J_F1] + 3) & ~3) <= hull0 + stride).all(), what
        # (a 16-byte load of the export kernel inside [f0 & ~3, (f1 + 3) & ~3) reads what the resampler wrote, or the run's own slack)
        fl = stride * rs[:, J_NCH]
        assert (rs[:, J_SCRATCH] == np.cumsum(fl) - fl).all() and pc[P_SCRATCH] == fl.sum() and 4 * pc[P_SCRATCH] <= SCRATCH_MAX, what
        n_sb = -(-(rj[:, R_JB] - rj[:, R_JA]) // per)
        bl = n_sb * rj[:, R_NCH] * S
        assert (rj[:, R_NSB] == n_sb).all() and (rj[:, R_FIRST_BLOCK] == np.cumsum(bl) - bl).all() and pc[P_RBLOCKS] == bl.sum(), what
    assert [p["stage_need0"], p["stage_need1"], p["scratch_need"]] == need, what
    # the copy runs of all pieces cover every request's [offset, offset + n_bytes + pad) once and nothing else
    want = [(int(r[OFFSET]), int(r[OFFSET] + (r[S1] - r[S0]) * fb + r[PAD])) for r, fb in zip(rows, fbytes) if r[S1] > r[S0]]
    got = sorted((int(r[1]), int(r[1] + r[2])) for r in runs)
    assert all(b0 >= a1 for (_, a1), (b0, _) in zip(got, got[1:])), what

    def merged(iv):
        out = []
        for a, b in iv:
            if out and out[-1][1] == a:
                out[-1][1] = b
            else:
                out.append([a, b])
        return out
    assert merged(got) == merged(sorted(want)), what
    # the pointer table: a request's pointers, then those of each of its resampled jobs; the uploaded table's three parts
    slots = [(int(p["ptr0"][i]), int(r[N_CH])) for i, r in enumerate(rows)] + [(int(j[J_PTR]), int(j[J_NCH])) for j in jobs if j[J_RESAMPLED]]
    at = 0
    for s, n in sorted(slots):
        assert s == at, what
        at += n
    assert at == p["n_ptrs"] and p["o_rjobs"] == 72 * len(jobs) and p["o_ptrs"] == p["o_rjobs"] + 64 * len(rjobs), what
    assert p["tab_bytes"] == p["o_ptrs"] + 8 * p["n_ptrs"], what


BASES = np.array([0x7f0000000000, 0x7f1000000000, 0x7f2000000000, 0x7f3000000100, 0x7f4000000000], U64)  # 16-byte aligned, made up


def check_export_bind(lib, rows, p, what):
    chan = (0x100000000 + 4 * np.arange(int(rows[:, N_CH].sum()) if len(rows) else 0, dtype=U64) * 1000003).astype(U64)  # (4-byte aligned only)
    h = lib.emu_bind_export(_p64(rows), len(rows), _p64(BASES), _p64(chan), len(chan))
    b = _blobs(lib, h, [U64, U64, np.uint8])
    jp, rp, tab = b[0].reshape(-1, 3).astype(np.int64), b[1].reshape(-1, 2).astype(np.int64), b[2]
    stage, scratch, d_tab, cnt = [int(BASES[0]), int(BASES[1])], int(BASES[2]), int(BASES[3]), int(BASES[4])
    assert len(tab) == p["tab_bytes"], what
    ptrs = tab[p["o_ptrs"]:].view(U64).astype(np.int64) if p["n_ptrs"] else np.zeros(0, np.int64)
    jobs, d_ptrs = p["jobs"], d_tab + p["o_ptrs"]
    c0 = np.cumsum(rows[:, N_CH].astype(np.int64)) - rows[:, N_CH].astype(np.int64) if len(rows) else []
    for i, r in enumerate(rows):
        assert (ptrs[p["ptr0"][i]:p["ptr0"][i] + int(r[N_CH])] == chan[c0[i]:c0[i] + int(r[N_CH])].astype(np.int64)).all(), what
    for k, pc in enumerate(p["pieces"]):
        rj = pc[P_RJOB0]
        for j in range(pc[P_JOB0], pc[P_JOB1]):
            J = jobs[j]
            assert jp[j, 1] == stage[k & 1] + J[J_STAGE] and jp[j, 2] == cnt + 16 * J[J_REQ], what
            if not J[J_RESAMPLED]:
                assert jp[j, 0] == d_ptrs + 8 * p["ptr0"][J[J_REQ]], what
                continue
            assert jp[j, 0] == d_ptrs + 8 * J[J_PTR] and rp[rj, 0] == d_ptrs + 8 * p["ptr0"][J[J_REQ]], what
            assert rp[rj, 1] == scratch + 4 * J[J_SCRATCH], what
            biased = ptrs[J[J_PTR]:J[J_PTR] + J[J_NCH]]
            assert (biased == scratch + 4 * (J[J_SCRATCH] + np.arange(J[J_NCH]) * J[J_STRIDE] - J[J_HULL0])).all() and (biased % 16 == 0).all(), what
            rj += 1
        assert rj == pc[P_RJOB1], what
    # the table's first two parts are the jobs themselves
    raw = tab[:p["o_rjobs"]].view(U64).reshape(-1, 9).astype(np.int64)
    assert (raw[:, :3] == jp).all() and (raw[:, 3] == jobs[:, J_F0]).all() and (raw[:, 4] == jobs[:, J_F1]).all(), what
    raw = tab[p["o_rjobs"]:p["o_ptrs"]].view(U64).reshape(-1, 8).astype(np.int64)
    assert (raw[:, :2] == rp).all() and (raw[:, 2] == p["rjobs"][:, R_JA]).all() and (raw[:, 3] == p["rjobs"][:, R_JB]).all(), what


def _mixed():
    a = dict(n_ch=2, n_in=3 * 44100 + 17, sr=44100)
    b = dict(n_ch=1, n_in=5 * 48000 + 3, sr=48000)
    return [req(fmt=S16, **a), req(fmt=S24, sr_out=48000, s0=1001, **a), req(fmt=F32, s0=77, s1=40001, **a),  # (track a three times)
            req(fmt=S16, sr_out=44100, dither=1, seed=9, **b), req(fmt=S24, **b), req(fmt=F32, sr_out=48000, s1=99999, **a),
            req(fmt=S16, sr_out=44100, s0=5, s1=6, **b), req(fmt=S16, s0=100, s1=100, **b)]


# name -> (requests, offset of the first one)
CASES = {
    "no_request": ([], 0),
    "empty_range": ([req(1, 1000, 48000, S16, 500, 500)], 0),
    "one_mono_s16_frame": ([req(1, 1, 48000, S16)], 0),
    "stereo_s16_three_pieces": ([req(2, 2 * PIECE // 4 + 1001, 48000, S16)], 0),
    "three_ch_s24_two_pieces": ([req(3, PIECE // 9 + 5000, 44100, S24)], 0),
    "five_ch_from_4097": ([req(5, 100000, 48000, F32, s0=4097)], 0),
    "1024_ch_f32": ([req(1024, 20000, 48000, F32)], 0),
    "wav_offset_44": ([req(2, 12345, 44100, S16)], 44),
    "8000_to_48000_six_ch_s16": ([req(6, 1000000, 8000, S16, sr_out=48000)], 0),
    "44100_to_48000": ([req(2, 3 * 44100 + 1, 44100, S24, sr_out=48000, s0=3, s1=100003)], 0),
    "48000_to_44100": ([req(2, 3 * 48000 + 1, 48000, S24, sr_out=44100)], 0),
    "96000_to_8000": ([req(3, 4 * 96000 + 5, 96000, F32, sr_out=8000, s0=1)], 0),
    "plain_and_two_rate_pairs": (_mixed(), 0),
}


@pytest.fixture(scope="module")
def plans(emu):
    """every fixed case planned once: name -> (request rows, plan)"""
    out = {}
    for name, (reqs, first) in CASES.items():
        rows = layout(reqs, first)
        out[name] = (rows, plan(emu, rows))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_export_plan_accounts_for_every_byte(emu, plans, name):
    rows, p = plans[name]
    check_export_plan(rows, p, name)
    check_export_bind(emu, rows, p, name)


def test_export_plan_shapes_of_the_fixed_cases(plans):
    n_pieces = {name: len(p["pieces"]) for name, (_, p) in plans.items()}
    assert n_pieces["no_request"] == n_pieces["empty_range"] == 0 and n_pieces["one_mono_s16_frame"] == 1
    assert n_pieces["stereo_s16_three_pieces"] == 3 and n_pieces["three_ch_s24_two_pieces"] == 2
    assert n_pieces["8000_to_48000_six_ch_s16"] >= 3 and n_pieces["1024_ch_f32"] == 3
    rows, p = plans["three_ch_s24_two_pieces"]
    assert p["jobs"][1, J_STAGE] % 16 != 0  # (9-byte frames: the second piece starts off the 16-byte grid)
    rows, p = plans["wav_offset_44"]
    assert p["jobs"][0, J_STAGE] == 44 % 16 and p["runs"][0].tolist() == [12, 44, 12345 * 4]
    rows, p = plans["five_ch_from_4097"]
    assert export_chunk_frames(5) == 816 and p["pieces"][0, P_CHUNKS] == export_n_chunks(4097, 100000, 5)
    rows, p = plans["plain_and_two_rate_pairs"]  # a piece holds one rate pair: the second pair closes the piece of the first
    assert [tuple(pc) for pc in p["pieces"][:, [P_SR_IN, P_SR_OUT]]] == [(44100, 48000), (48000, 44100), (44100, 48000), (48000, 44100)]


def _golden_of(p):
    return dict(jobs=p["jobs"][:, [J_REQ, J_F0, J_F1, J_FIRST_CHUNK, J_PAD, J_STAGE, J_HULL0, J_STRIDE, J_SCRATCH]].tolist(),
                pieces=p["pieces"].tolist(), runs=p["runs"].tolist())


def test_export_piece_boundaries_are_the_parents(plans):
    """per job {request, f0, f1, first_chunk, pad, staging offset, hull start, stride, scratch offset}, per piece its ranges, counts
    and rate pair (the columns of a piece row above), and the copy runs: equal to what the loop inside export_run made of the same requests"""
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(CASES)
    for name, (_, p) in plans.items():
        assert _golden_of(p) == golden[name], name


TRACKS = [dict(n_ch=2, n_in=3 * 44100 + 17, sr=44100), dict(n_ch=1, n_in=5 * 48000 + 3, sr=48000), dict(n_ch=3, n_in=PIECE // 9 + 5000, sr=44100),
          dict(n_ch=5, n_in=100000, sr=48000), dict(n_ch=1024, n_in=20000, sr=48000), dict(n_ch=6, n_in=1000000, sr=8000),
          dict(n_ch=3, n_in=4 * 96000 + 5, sr=96000), dict(n_ch=2, n_in=2 * PIECE // 4 + 1001, sr=48000)]
RATES = [8000, 44100, 48000, 96000]


def test_export_plan_random_batches(emu):
    rng = np.random.default_rng(20240)
    n_pieces = 0
    for trial in range(300):
        reqs = []
        for _ in range(int(rng.integers(1, 9))):
            t = TRACKS[int(rng.integers(0, len(TRACKS)))]
            sr_out = RATES[int(rng.integers(0, len(RATES)))] if rng.random() < 0.5 else t["sr"]
            if sr_out * 64 < t["sr"] or t["n_ch"] == 1024 and sr_out != t["sr"]:
                sr_out = t["sr"]
            n = t["n_in"] if sr_out == t["sr"] else n_out_of(t["n_in"], t["sr"], sr_out)
            kind = rng.random()
            s0 = 0 if kind < 0.3 else int(rng.integers(0, n + 1))
            s1 = n if kind < 0.5 else s0 if kind < 0.55 else int(rng.integers(s0, n + 1))
            reqs.append(req(fmt=[S16, S24, F32][int(rng.integers(0, 3))], s0=s0, s1=s1, sr_out=sr_out, dither=int(rng.integers(0, 2)),
                            seed=int(rng.integers(0, 2 ** 32)), **t))
        rows = layout(reqs, 44 if len(reqs) == 1 and trial % 2 else 0)
        p = plan(emu, rows)
        check_export_plan(rows, p, "trial %d" % trial)
        if trial % 10 == 0:
            check_export_bind(emu, rows, p, "trial %d" % trial)
        n_pieces = max(n_pieces, len(p["pieces"]))
    assert n_pieces >= 8  # (the sweep reaches batches of many pieces)


# ---------------------------------------------------------------------------------------------------------------- meters
M_NAMES = ["err", "n_ch", "n_energies", "n_states", "max_chunks", "max_fchunks", "lds_floats", "tp_chunks0", "tp_chunks1", "max_m", "max_s",
           "o_sums", "o_pka", "o_pkt", "res_bytes", "o_z", "o_q", "mem_bytes", "t_rates", "t_m", "t_s", "t_tp4", "t_tp2", "tab_bytes",
           "sizeof_job", "sizeof_rate", "sizeof_tjob", "sizeof_tp"]
TP_CHUNK = 33 * 256


def meter_rows(tracks):
    """tracks: (sr, n_ch, n_samples); the id is 100 + the index"""
    return np.array([[100 + i, sr, n_ch, n] for i, (sr, n_ch, n) in enumerate(tracks)], U64).reshape(-1, 4)


def plan_m(lib, rows):
    b = _blobs(lib, lib.emu_plan_meters(_p64(rows), len(rows)), [U64, np.uint8, U64, U64, U64, U64, np.float64, U64, U64, U64])
    p = dict(zip(M_NAMES, (int(v) for v in b[0].view(np.int64))))
    i64 = lambda a, w: a.reshape(-1, w).astype(np.int64)  # noqa: E731
    p.update(text=b[1].tobytes().decode(), rates=i64(b[2], 4), jobs=i64(b[3], 4), tj_m=i64(b[4], 5), tj_s=i64(b[5], 5), w=b[6].reshape(-1, 8),
             tp4=i64(b[7], 3), tp2=i64(b[8], 3), per=i64(b[9], 6))
    return p


METER_BATCHES = {
    "rates": [(48000, 2, 3 * 48000 + 11), (44100, 1, 35 * 4410 + 3), (16, 1, 70), (8, 2, 40)],
    "oversampling": [(48000, 1, 48000), (96000, 1, 2 * 96000), (192000, 2, 192000 + 1)],
    "lengths": [(48000, 2, 0), (48000, 2, 4799), (48000, 2, 19199), (48000, 1, 168000), (44100, 6, 154350)],  # 0, < 400 ms, 3.5 s
    "channels": [(48000, 1, 48000 + 1), (48000, 2, 48000 + 2), (48000, 6, 48000 + 3), (48000, 9, 48000 + 4)],
    "shared_rate": [(44100, 2, 3 * 44100), (48000, 1, 1000), (44100, 1, 5 * 44100 + 1)],
}


@pytest.mark.parametrize("name", list(METER_BATCHES))
def test_meter_plan_layout_and_jobs(emu, name):
    tracks = METER_BATCHES[name]
    rows = meter_rows(tracks)
    p = plan_m(emu, rows)
    assert p["err"] == 0, p["text"]
    n, per, jobs = len(tracks), p["per"], p["jobs"]
    n_ch = sum(t[1] for t in tracks)
    assert p["n_ch"] == n_ch == len(jobs) and len(per) == len(p["tj_m"]) == len(p["tj_s"]) == n
    # the areas: energies, sums, two peak arrays | states | chunk energies — disjoint, in this order, inside mem_bytes
    areas = [(0, 8 * p["n_energies"]), (p["o_sums"], 8 * n_ch), (p["o_pka"], 4 * n_ch), (p["o_pkt"], 4 * n_ch), (p["o_z"], 64 * p["n_states"]),
             (p["o_q"], 8 * p["n_states"])]
    for (a, la), (b, _) in zip(areas, areas[1:]):
        assert a + la <= b and a % 8 == 0
    assert areas[3][0] + areas[3][1] <= p["res_bytes"] <= p["o_z"] and p["o_z"] % 256 == 0
    assert areas[-1][0] + areas[-1][1] <= p["mem_bytes"]
    # the tables: offsets that are multiples of 256, disjoint
    tabs = [(0, p["sizeof_job"] * n_ch), (p["t_rates"], p["sizeof_rate"] * len(p["rates"])), (p["t_m"], p["sizeof_tjob"] * n),
            (p["t_s"], p["sizeof_tjob"] * n), (p["t_tp4"], p["sizeof_tp"] * len(p["tp4"])), (p["t_tp2"], p["sizeof_tp"] * len(p["tp2"]))]
    for (a, la), (b, _) in zip(tabs + [(p["tab_bytes"], 0)], (tabs + [(p["tab_bytes"], 0)])[1:]):
        assert a % 256 == 0 and b % 256 == 0 and a + la <= b
    # per track
    seen_rates, e0, c0, tp = [], 0, 0, {4: [], 2: []}
    for i, (sr, nc, ns) in enumerate(tracks):
        ok = 16 <= sr <= 2822400
        F = 4 if sr < 96000 else 2 if sr < 192000 else 1
        n_m = ta.loudness_n_blocks(ns, sr) if ok else 0
        n_s = ta.loudness_n_short_term(ns, sr) if ok else 0
        assert per[i].tolist() == [c0, e0, ok, F, n_m, n_s], (name, i)
        geo = sr if ok else 48000  # (a refused rate: the peaks only, over chunks of a 48 kHz geometry)
        if geo not in seen_rates:
            seen_rates.append(geo)
        ri = seen_rates.index(geo)
        r_sr, s100, n_sub, cl = p["rates"][ri]
        assert r_sr == geo and s100 == (geo + 5) // 10 and n_sub * cl >= s100 and cl <= 4800
        nseg_any, nseg = -(-ns // s100), ns // s100
        nf = nseg * n_sub if ok and nseg >= 4 else 0
        for c in range(c0, c0 + nc):
            assert jobs[c].tolist() == [ns, ri, nseg_any * n_sub, nf], (name, i, c)
            if F > 1 and ns:
                tp[F].append([ns, -(-ns // TP_CHUNK), c])
        assert p["tj_m"][i].tolist() == [n_m, nc, n_sub, nf, 4 * s100] and p["tj_s"][i].tolist() == [n_s, nc, n_sub, nf, 30 * s100], (name, i)
        # the default channel map (L R C 1, LFE 0, Ls Rs 1.41; a channel above the eighth takes w[7]: nothing)
        assert nc in (4, 5) or p["w"][i].tolist() == [1.0, 1.0, 1.0, 0.0, 1.41, 1.41, 0.0, 0.0], (name, i)
        e0 += n_m + n_s
        c0 += nc
    assert len(p["rates"]) == len(seen_rates) and p["n_energies"] == e0
    assert p["n_states"] == jobs[:, 3].sum()
    # every true-peak job names the channel whose peak slot it gets
    assert p["tp4"].tolist() == tp[4] and p["tp2"].tolist() == tp[2]
    # the launch bounds are the maxima of the jobs
    assert p["max_chunks"] == jobs[:, 2].max() and p["max_fchunks"] == jobs[:, 3].max()
    assert p["max_m"] == per[:, 4].max() and p["max_s"] == per[:, 5].max() and p["lds_floats"] == max(4, p["rates"][:, 3].max() + 4)
    assert p["tp_chunks0"] == max([t[1] for t in tp[4]], default=0) and p["tp_chunks1"] == max([t[1] for t in tp[2]], default=0)

    # bind: every pointer from the one base and the channels' addresses
    mem = 0x7e0000000000
    wav = (0x200000000 + 4 * np.arange(n_ch, dtype=U64) * 1000003).astype(U64)
    wav[::3] &= U64(~15 & (2 ** 64 - 1))
    b = _blobs(emu, emu.emu_bind_meters(_p64(rows), n, mem, _p64(wav), n_ch), [U64, U64, U64, U64, U64, np.uint8])
    bj, bm, bs = b[0].reshape(-1, 6).astype(np.int64), b[1].reshape(-1, 2).astype(np.int64), b[2].reshape(-1, 2).astype(np.int64)
    b4, b2, tab = b[3].reshape(-1, 3).astype(np.int64), b[4].reshape(-1, 3).astype(np.int64), b[5]
    w64 = wav.astype(np.int64)
    si = np.cumsum(jobs[:, 3]) - jobs[:, 3]  # each channel's state and energy offsets: the running sums of n_fchunks
    c = np.arange(n_ch)
    assert (bj[:, 0] == w64).all() and (bj[:, 5] == (w64 % 16 == 0)).all()
    assert (bj[:, 1] == mem + p["o_z"] + 64 * si).all() and (bj[:, 2] == mem + p["o_q"] + 8 * si).all()
    assert (bj[:, 3] == mem + p["o_sums"] + 8 * c).all() and (bj[:, 4] == mem + p["o_pka"] + 4 * c).all()
    for i in range(n):
        q0 = mem + p["o_q"] + 8 * si[per[i, 0]] if tracks[i][1] else None
        if q0 is not None:
            assert bm[i, 0] == bs[i, 0] == q0
        assert bm[i, 1] == mem + 8 * per[i, 1] and bs[i, 1] == mem + 8 * (per[i, 1] + per[i, 4])
    for bt, want in ((b4, tp[4]), (b2, tp[2])):
        ch = np.array([t[2] for t in want], np.int64)
        assert (bt[:, 0] == w64[ch]).all() and (bt[:, 1] == mem + p["o_pkt"] + 4 * ch).all() and (bt[:, 2] == (w64[ch] % 16 == 0)).all()
    assert len(tab) == p["tab_bytes"]
    assert (tab[:p["sizeof_job"] * n_ch].view(U64).reshape(n_ch, -1)[:, :5].astype(np.int64) == bj[:, :5]).all()
    assert (tab[p["t_tp4"]:p["t_tp4"] + 32 * len(b4)].view(U64).reshape(-1, 4)[:, :2].astype(np.int64) == b4[:, :2]).all()


@pytest.mark.parametrize("tracks,text", [
    ([(48000, 1, 10)] * 65536, "at most 65535 tracks per call"),
    ([(48000, 1024, 10)] * 64, "at most 65535 channels per call"),
    ([(48000, 1, 10), (48000, 2, 1 << 40)], "track 101: too many samples"),
], ids=["tracks", "channels", "samples"])
def test_meter_plan_limits(emu, tracks, text):
    p = plan_m(emu, meter_rows(tracks))
    assert p["err"] == ERR_INVALID_ARG and p["text"] == text


def test_meter_result_from_a_made_up_area(emu):
    tracks = [(48000, 2, 7 * 48000 + 5), (8, 3, 100), (44100, 6, 40 * 4410), (96000, 1, 500), (192000, 2, 192000), (48000, 1, 0)]
    rows = meter_rows(tracks)
    p = plan_m(emu, rows)
    assert p["err"] == 0
    rng = np.random.default_rng(5)
    res = np.zeros(p["res_bytes"], np.uint8)
    E = 10.0 ** (rng.uniform(-7, -1, p["n_energies"]))
    E[3], E[5] = 0.0, np.nan
    res[:p["o_sums"]].view(np.float64)[:] = E
    pka = rng.uniform(0.1, 0.9, p["n_ch"]).astype(np.float32)
    pkt = rng.uniform(0.1, 1.2, p["n_ch"]).astype(np.float32)
    pkt[-1] = 0.0  # (the empty track: -inf dB)
    res[p["o_pka"]:p["o_pka"] + 4 * p["n_ch"]].view(np.float32)[:] = pka
    res[p["o_pkt"]:p["o_pkt"] + 4 * p["n_ch"]].view(np.float32)[:] = pkt
    h = emu.emu_meter_results(_p64(rows), len(rows), res.ctypes.data_as(C.c_void_p), res.size)
    out, series = _blobs(emu, h, [np.float64, np.float64])
    out = out.reshape(-1, 6)
    assert series.size == p["n_energies"]
    with np.errstate(divide="ignore"):
        lufs = 10.0 * np.log10(E) - 0.691
    assert np.allclose(series, lufs, rtol=0, atol=1e-12, equal_nan=True) and series[3] == -np.inf and np.isnan(series[5])
    for i, (sr, nc, ns) in enumerate(tracks):
        c0, e0, ok, F, n_m, n_s = p["per"][i]
        mx_m, mx_s, lra, peak, peak_db, ch = out[i]
        if ok:
            mom, st = series[e0:e0 + n_m], series[e0 + n_m:e0 + n_m + n_s]
            assert mx_m == (np.nanmax(mom) if n_m and not np.isnan(mom).all() else -np.inf), i
            assert mx_s == (np.nanmax(st) if n_s and not np.isnan(st).all() else -np.inf), i
            assert lra == mref.loudness_range(E[e0 + n_m:e0 + n_m + n_s][::10]) == ta.loudness_range(E[e0 + n_m:e0 + n_m + n_s][::10]), i
        else:
            assert np.isnan([mx_m, mx_s, lra]).all(), i
        pk = (pkt if F > 1 else pka)[c0:c0 + nc]
        assert peak == pk.max() and ch == int(np.argmax(pk)), i
        assert peak_db == (np.float32(20.0 * math.log10(float(peak))) if peak else -np.inf), i
    assert out[0, 0] > -np.inf and out[5, 3] == 0.0 and out[5, 4] == -np.inf  # (the empty track: a zero peak)
    assert out[4, 3] == pka[p["per"][4, 0]:p["per"][4, 0] + 2].max()             # (oversampling 1: pass A's peaks)
