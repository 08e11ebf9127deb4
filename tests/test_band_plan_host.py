"""plan_export / bind_export (thesia_amd/csrc/reader_plan.h) on requests that carry a band filter: where the BandJobs lie, what closes
a piece, the table's offsets and the addresses bind_export hands out.  CPU only: tests/emu/emu_band_plan.cpp is compiled here with g++
beside reader_plan.cpp and host_math.cpp (once; the library is kept under tests/emu/_build and rebuilt when a source is newer)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from thesia_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thesia_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "emu", "emu_band_plan.cpp"), os.path.join(CSRC, "reader_plan.cpp"), os.path.join(CSRC, "host_math.cpp")]
DEPS = SRC + [os.path.join(CSRC, h) for h in ("reader_plan.h", "host_math.h", "export_core.h", "plan_error.h")] + [os.path.join(ROOT, "include", "thesia_amd.h")]
LIB = os.path.join(ROOT, "tests", "emu", "_build", "libemu_band_plan.so")
BASES = (0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000)  # stage 0, stage 1, scratch, table, counters
CHAN0 = 0x60000000
PIECE, TILE = api.EXPORT_PIECE_BYTES, api.BAND_TILE
SCRATCH_MAX = 2 * PIECE + (64 << 10)
BYTES = {0: 2, 1: 3, 2: 4}
NONE = (0, 0, 0.0, 0.0)
A, B2, A_STOP = (64, 0, 1000.0, 2500.0), (64, 0, 1000.0, 2600.0), (64, 1, 1000.0, 2500.0)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-ffp-contract=off", "-o", LIB] + SRC)
    so = C.CDLL(LIB)
    so.emu_band_plan.restype = C.c_int64
    return so


def plan(lib, reqs):
    """reqs: (n_ch, n_in, fmt, s0, s1, band) -> dict of the plan; offsets are laid out as export_layout does"""
    rows, bands, at = [], [], 0
    for i, (n_ch, n_in, fmt, s0, s1, band) in enumerate(reqs):
        nbytes = (s1 - s0) * n_ch * BYTES[fmt]
        end = at + nbytes
        nxt = (end + 15) // 16 * 16
        rows += [n_ch, n_in, 8000, fmt, 1, 7, s0, s1, at, (nxt - end) if i + 1 < len(reqs) else 0]
        bands += list(band)
        at = nxt
    rows, bands = np.array(rows, np.uint64), np.array(bands, np.float64)
    out = np.zeros(1 << 16, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    n = lib.emu_band_plan(rows.ctypes.data_as(u64p), bands.ctypes.data_as(C.POINTER(C.c_double)), len(reqs), (C.c_uint64 * 5)(*BASES),
                          C.c_uint64(CHAN0), out.ctypes.data_as(u64p), out.size)
    assert n > 0
    v = [int(x) for x in out[:n]]
    assert v[0] == 0, v[0]
    keys = ("err", "n_jobs", "n_rjobs", "n_bjobs", "n_pieces", "o_rjobs", "o_bjobs", "o_ptrs", "tab_bytes", "scratch_need", "n_ptrs", "tab_len")
    p = dict(zip(keys, v[:12]))
    at = 12
    p["ptr0"] = v[at: at + len(reqs)]
    at += len(reqs)

    def take(count, names):
        nonlocal at
        recs = [dict(zip(names, v[at + k * len(names): at + (k + 1) * len(names)])) for k in range(count)]
        at += count * len(names)
        return recs
    p["jobs"] = take(p["n_jobs"], ("req", "f0", "f1", "n", "first_chunk", "stage_at", "filtered", "hull0", "stride", "scratch_at", "ptr_at", "chan", "dst"))
    p["bjobs"] = take(p["n_bjobs"], ("ja", "jb", "n_in", "ch_stride", "n_ch", "n_tiles", "first_block", "chan", "dst"))
    p["pieces"] = take(p["n_pieces"], ("job0", "job1", "bjob0", "bjob1", "n_bblocks", "half_taps", "band_sr", "scratch_floats", "n_chunks", "n_runs"))
    p["ptrs"] = v[at: at + p["n_ptrs"]]
    assert at + p["n_ptrs"] == n
    return p


def check(p, reqs):
    """what holds of every plan with filtered requests"""
    assert p["n_rjobs"] == 0 and p["o_bjobs"] == p["o_rjobs"] == 72 * p["n_jobs"] and p["o_ptrs"] == p["o_bjobs"] + 64 * p["n_bjobs"]
    assert p["tab_bytes"] == p["tab_len"] == p["o_ptrs"] + 8 * p["n_ptrs"]
    assert p["n_bjobs"] == sum(j["filtered"] for j in p["jobs"])
    d_ptrs = BASES[3] + p["o_ptrs"]
    chan_index = np.cumsum([0] + [r[0] for r in reqs])
    covered = {}
    for k, pc in enumerate(p["pieces"]):
        jobs = p["jobs"][pc["job0"]: pc["job1"]]
        bjobs = p["bjobs"][pc["bjob0"]: pc["bjob1"]]
        filtered = [j for j in jobs if j["filtered"]]
        assert len(filtered) == len(bjobs)
        assert len({reqs[j["req"]][5] for j in filtered}) <= 1  # one filter per piece
        assert pc["half_taps"] == (reqs[filtered[0]["req"]][5][0] if filtered else 0) and pc["band_sr"] == (8000 if filtered else 0)
        blocks, floats = 0, 0
        for j, b in zip(filtered, bjobs):
            n_ch, n_in, fmt, s0, s1, band = reqs[j["req"]]
            F = api.export_chunk_frames(n_ch)
            assert j["f0"] == s0 or j["f0"] % F == 0       # cut on multiples of the export chunk
            assert j["f1"] == s1 or j["f1"] % F == 0
            assert j["hull0"] == j["f0"] // 4 * 4 and j["stride"] % 4 == 0 and j["n"] == n_in
            hull1 = min((j["f1"] + 3) // 4 * 4, n_in)
            assert (b["ja"], b["jb"], b["n_in"], b["ch_stride"], b["n_ch"]) == (j["hull0"], hull1, n_in, j["stride"], n_ch)
            assert b["jb"] - b["ja"] <= j["stride"] < b["jb"] - b["ja"] + 4
            assert b["n_tiles"] == -(-(b["jb"] - b["ja"]) // TILE) and b["first_block"] == blocks
            blocks += b["n_tiles"] * n_ch
            assert j["scratch_at"] == floats and j["scratch_at"] % 4 == 0  # the runs lie one behind the other, 16-byte aligned
            floats += j["stride"] * n_ch
            # bind: the filter reads the track's channels and writes the run; the export reads the run through biased pointers
            assert b["chan"] == d_ptrs + 8 * p["ptr0"][j["req"]] and b["dst"] == BASES[2] + 4 * j["scratch_at"]
            assert j["chan"] == d_ptrs + 8 * j["ptr_at"]
            for c in range(n_ch):
                assert p["ptrs"][p["ptr0"][j["req"]] + c] == CHAN0 + 0x100000 * (chan_index[j["req"]] + c)
                assert p["ptrs"][j["ptr_at"] + c] == BASES[2] + 4 * (j["scratch_at"] + c * j["stride"]) - 4 * j["hull0"]
                assert p["ptrs"][j["ptr_at"] + c] % 16 == 0
        for j in jobs:
            assert j["dst"] == BASES[k & 1] + j["stage_at"]
            if not j["filtered"]:
                assert j["chan"] == d_ptrs + 8 * p["ptr0"][j["req"]]
            covered.setdefault(j["req"], []).append((j["f0"], j["f1"]))
        assert (pc["n_bblocks"], pc["scratch_floats"]) == (blocks, floats) and floats * 4 <= SCRATCH_MAX
    assert p["scratch_need"] == max(pc["scratch_floats"] for pc in p["pieces"])
    for i, (n_ch, n_in, fmt, s0, s1, band) in enumerate(reqs):  # the jobs of a request tile its range, in order
        spans = covered.get(i, [])
        if s1 == s0:
            assert spans == []
            continue
        assert spans[0][0] == s0 and spans[-1][1] == s1 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


def test_small_batches_and_what_closes_a_piece(lib):
    reqs = [(2, 5003, 1, 1, 2050, A), (1, 5003, 0, 0, 5003, A), (2, 5003, 2, 0, 5003, NONE), (6, 3001, 2, 7, 2999, A), (3, 5003, 0, 10, 10, A)]
    p = plan(lib, reqs)
    check(p, reqs)
    assert p["n_pieces"] == 1 and p["n_bjobs"] == 3 and p["n_jobs"] == 4  # one filter, a plain request among them: one piece
    for other in (B2, A_STOP, (65,) + A[1:]):  # another edge, another mode, another length: each closes the piece
        reqs2 = [(2, 5003, 1, 1, 2050, A), (1, 5003, 0, 0, 5003, other), (2, 5003, 2, 0, 5003, NONE), (1, 5003, 0, 0, 5003, A)]
        p = plan(lib, reqs2)
        check(p, reqs2)
        assert [(pc["job0"], pc["job1"], pc["half_taps"]) for pc in p["pieces"]] == [(0, 1, 64), (1, 3, other[0]), (3, 4, 64)]
    # a hull at the track's end that is not a multiple of 4, and at its start below a multiple of 4
    reqs3 = [(1, 5003, 2, 5001, 5003, A), (1, 5003, 2, 3, 5, A), (1, 1, 2, 0, 1, A)]
    p = plan(lib, reqs3)
    check(p, reqs3)
    assert [(b["ja"], b["jb"], b["ch_stride"]) for b in p["bjobs"]] == [(5000, 5003, 4), (0, 8, 8), (0, 1, 4)]


def test_no_band_plans_no_band_job(lib):
    reqs = [(2, 5003, 1, 1, 2050, NONE), (6, 3001, 0, 0, 3001, NONE)]
    p = plan(lib, reqs)
    check(p, reqs)
    assert p["n_bjobs"] == 0 and p["o_bjobs"] == p["o_ptrs"] and p["scratch_need"] == 0 and p["n_ptrs"] == 8


def test_a_request_of_more_than_two_pieces(lib):
    """16 bit, 6 channels: the scratch (4 bytes per sample) and the staging (2 bytes) bound a piece; every cut is on the chunk grid"""
    n_ch = 6
    n = 2 * (PIECE // (2 * n_ch)) + 5000
    reqs = [(n_ch, n, 0, 3, n - 1, A), (1, 9000, 2, 0, 9000, A)]
    p = plan(lib, reqs)
    check(p, reqs)
    assert p["n_pieces"] == 3 and p["n_bjobs"] == 4
    assert max(pc["scratch_floats"] for pc in p["pieces"]) * 4 > PIECE  # (a piece's scratch is twice its 16-bit bytes)
    # float output of many channels: the staging fills first, the scratch stays below its own bound
    reqs = [(64, 400000, 2, 0, 400000, A)]
    p = plan(lib, reqs)
    check(p, reqs)
    assert p["n_pieces"] == 4
