"""plan_flac / bind_flac (thesia_amd/csrc/flac_plan.h) under each flags value of the _ex entries: TH_FLAC_LPC changes nothing in a
plan, TH_FLAC_STEREO gives a 2-channel block four units whose slots have the side channel's size; pieces stay whole blocks within the
piece size and the unit limit.  CPU only: tests/emu/emu_flac_lpc_plan.cpp is compiled here with g++ beside flac_plan.cpp (once; the
library is kept under tests/emu/_build and rebuilt when a source is newer).  The flags == 0 plans are tests/test_flac_plan_host.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from thesia_amd import api
from tests import flac_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thesia_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "emu", "emu_flac_lpc_plan.cpp"), os.path.join(CSRC, "flac_plan.cpp")]
DEPS = SRC + [os.path.join(CSRC, h) for h in ("flac_plan.h", "flac_core.h", "stft_core.h")] + [os.path.join(ROOT, "include", "thesia_amd.h")]
LIB = os.path.join(ROOT, "tests", "emu", "_build", "libemu_flac_lpc_plan.so")
PIECE = api.EXPORT_PIECE_BYTES
MAX_UNITS = 1 << 16
BPS = {0: 16, 1: 24}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-o", LIB] + SRC)
    so = C.CDLL(LIB)
    so.emu_flac_lpc_plan.restype = C.c_int64
    return so


def frame_bound(n, n_ch, bps):
    return 16 + n_ch * (1 + n * bps // 8) + 3


def units_per_block(n_ch, flags):
    return 4 if n_ch == 2 and flags & 2 else n_ch


def plan(lib, reqs, flags, piece=PIECE, err=0):
    """reqs: (n_ch, fmt, s0, s1) -> dict of the plan"""
    rows, at = [], 0
    for n_ch, fmt, s0, s1 in reqs:
        rows += [n_ch, fmt, s0, s1, at, flags]
        at = (at + F.bound(s1 - s0, n_ch, BPS[fmt]) + 15) // 16 * 16
    rows = np.array(rows, np.uint64)
    out = np.zeros(1 << 20, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    n = lib.emu_flac_lpc_plan(rows.ctypes.data_as(u64p), C.c_uint64(len(reqs)), C.c_uint64(piece), out.ctypes.data_as(u64p), C.c_uint64(out.size))
    assert n > 0
    v = [int(x) for x in out[:n]]
    assert np.int64(np.uint64(v[0])) == err
    if err:
        return None
    keys = ("n_pieces", "n_runs", "stage0", "stage1", "slot_need", "unit_need", "block_need")
    p = dict(zip(keys, v[1:8]))
    at = 8
    p["pieces"] = [dict(zip(("run0", "run1", "n_units", "n_blocks", "bound", "slot_words"), v[at + 6 * i: at + 6 * i + 6])) for i in range(p["n_pieces"])]
    at += 6 * p["n_pieces"]
    rk = ("req", "b0", "nb", "first_unit", "first_block", "slot_words", "slot_at", "stage_at", "bound", "slots", "bits", "foff", "flags")
    p["runs"] = [dict(zip(rk, v[at + len(rk) * i: at + len(rk) * (i + 1)])) for i in range(p["n_runs"])]
    assert at + len(rk) * p["n_runs"] == n
    return p


def check_plan(p, reqs, flags, piece=PIECE):
    """every block once and in order; pieces of whole blocks within the piece size and the unit limit; units, slots and tables of the
    flags' sizes; the staged bytes are those of flags == 0"""
    next_block = [0] * len(reqs)
    run_at = 0
    for pi, pc in enumerate(p["pieces"]):
        assert pc["run0"] == run_at and pc["run1"] > pc["run0"]
        run_at = pc["run1"]
        units = blocks = bound = slots = 0
        for k in range(pc["run0"], pc["run1"]):
            r = p["runs"][k]
            n_ch, fmt, s0, s1 = reqs[r["req"]]
            bps, n, upb = BPS[fmt], s1 - s0, units_per_block(n_ch, flags)
            assert r["b0"] == next_block[r["req"]] and r["nb"] >= 1 and r["flags"] == flags
            next_block[r["req"]] += r["nb"]
            lens = [min(4096, n - 4096 * b) for b in range(r["b0"], r["b0"] + r["nb"])]
            assert min(lens) >= 1 and len(set(lens)) == 1
            assert r["bound"] == sum(frame_bound(m, n_ch, bps) for m in lens)  # (th_flac_bound's frames whatever the flags)
            slot_bps = bps + 1 if upb != n_ch else bps  # (a stereo block's four slots have the side channel's size)
            assert r["slot_words"] == (8 + lens[0] * slot_bps + 31) // 32
            assert (r["first_unit"], r["first_block"], r["slot_at"], r["stage_at"]) == (units, blocks, slots, bound)
            assert (r["slots"], r["bits"], r["foff"]) == (slots, units, blocks)
            units += r["nb"] * upb
            blocks += r["nb"]
            slots += r["nb"] * upb * r["slot_words"]
            bound += r["bound"]
        assert (pc["n_units"], pc["n_blocks"], pc["bound"], pc["slot_words"]) == (units, blocks, bound, slots)
        assert units <= MAX_UNITS and (bound <= piece or blocks == 1)
        assert 4 * slots <= 3 * bound + 4 * units  # (what the slot scratch is bounded by: 4 x 17 / (2 x 16) of the bound at most)
        assert bound <= p["stage%d" % (pi & 1)] and slots <= p["slot_need"] and units <= p["unit_need"] and blocks <= p["block_need"]
    assert run_at == p["n_runs"]
    assert next_block == [(r[3] - r[2] + 4095) // 4096 for r in reqs]
    for pc, nxt in zip(p["pieces"], p["pieces"][1:]):  # a piece is closed only when the next block would not fit
        r = p["runs"][nxt["run0"]]
        n_ch, fmt, s0, s1 = reqs[r["req"]]
        first = frame_bound(min(4096, s1 - s0 - 4096 * r["b0"]), n_ch, BPS[fmt])
        assert pc["bound"] + first > piece or pc["n_units"] + units_per_block(n_ch, flags) > MAX_UNITS


MIXED = [(1, 0, 0, 1), (2, 1, 3, 4099), (8, 1, 0, 4096 * 3), (2, 0, 1, 4095), (3, 0, 0, 4097), (2, 0, 100, 100 + 5003)]


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_a_mixed_batch(lib, flags):
    p = plan(lib, MIXED, flags)
    check_plan(p, MIXED, flags)
    assert p["n_pieces"] == 1
    want = [1, 3073, 3073, 2048, 2049, 1, 2049, (8 + 907 * 16 + 31) // 32]
    if flags & 2:  # the three stereo requests: slots of 25 and 17 bits a sample
        want = [1, (8 + 4096 * 25 + 31) // 32, 3073, (8 + 4094 * 17 + 31) // 32, 2049, 1, (8 + 4096 * 17 + 31) // 32, (8 + 907 * 17 + 31) // 32]
    assert [r["slot_words"] for r in p["runs"]] == want
    units = sum(((s1 - s0 + 4095) // 4096) * units_per_block(n_ch, flags) for n_ch, _, s0, s1 in MIXED)
    assert p["pieces"][0]["n_units"] == p["unit_need"] == units


def test_lpc_alone_changes_no_plan(lib):
    for reqs, piece in ((MIXED, PIECE), (MIXED, 30000), ([(2, 0, 0, 4096 * 40 + 7)], 3 * frame_bound(4096, 2, 16) + 100)):
        a, b = plan(lib, reqs, 0, piece), plan(lib, reqs, 1, piece)
        for r in a["runs"] + b["runs"]:
            del r["flags"]
        assert a == b
        c, d = plan(lib, reqs, 2, piece), plan(lib, reqs, 3, piece)
        for r in c["runs"] + d["runs"]:
            del r["flags"]
        assert c == d and [(r["req"], r["b0"], r["nb"]) for r in c["runs"]] == [(r["req"], r["b0"], r["nb"]) for r in a["runs"]]  # (the same pieces here)


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_small_pieces_cut_at_blocks(lib, flags):
    reqs = [(2, 0, 0, 4096 * 5 + 17), (1, 1, 9, 9 + 4096 * 2), (2, 1, 0, 300)]
    piece = 3 * frame_bound(4096, 2, 16) + 100
    p = plan(lib, reqs, flags, piece)
    check_plan(p, reqs, flags, piece)
    assert [(r["req"], r["b0"], r["nb"]) for r in p["runs"]][:4] == [(0, 0, 3), (0, 3, 2), (0, 5, 1), (1, 0, 1)]
    p = plan(lib, reqs, flags, 1000)  # a piece smaller than one block still takes it
    check_plan(p, reqs, flags, 1000)
    assert p["n_pieces"] == p["n_runs"] == 6 + 2 + 1


def test_a_stereo_call_whose_units_cross_the_limit(lib):
    """2-channel requests of 3 samples: 32 768 of them fill a piece's 65 536 units without TH_FLAC_STEREO, 16 384 with it"""
    reqs = [(2, 0, 0, 3)] * (MAX_UNITS // 2 + 3)
    p = plan(lib, reqs, 1)
    check_plan(p, reqs, 1)
    assert [pc["n_units"] for pc in p["pieces"]] == [MAX_UNITS, 6]
    p = plan(lib, reqs, 3)
    check_plan(p, reqs, 3)
    assert [pc["n_units"] for pc in p["pieces"]] == [MAX_UNITS, MAX_UNITS, 12] and [pc["n_blocks"] for pc in p["pieces"]] == [16384, 16384, 3]
    # and inside one long request: whole blocks until the limit, the piece size far away
    reqs = [(2, 0, 0, 4096 * 16385)]
    p = plan(lib, reqs, 2, 1 << 40)
    check_plan(p, reqs, 2, 1 << 40)
    assert [r["nb"] for r in p["runs"]] == [16384, 1] and p["slot_need"] == MAX_UNITS * ((8 + 4096 * 17 + 31) // 32)


def test_a_stereo_track_of_more_than_two_pieces(lib):
    """the GPU test's track: the pieces are those of flags == 0 (the bound decides), the slot scratch is 4 x 17 / 32 of it"""
    fb = frame_bound(4096, 2, 16)
    full = (2 * PIECE - 42) // fb
    rest = (2 * PIECE - 42 - full * fb - 21) // 4 + 1
    reqs = [(2, 0, 0, full * 4096 + rest)]
    p = plan(lib, reqs, 2)
    check_plan(p, reqs, 2)
    assert p["n_pieces"] == 3 and [r["nb"] for r in p["runs"]] == [PIECE // fb, PIECE // fb, 1]
    assert p["slot_need"] == (PIECE // fb) * 4 * 2177 and 4 * p["slot_need"] <= 3 * PIECE


def test_unknown_flags_do_not_reach_a_plan(lib):
    """(the entries refuse them as TH_ERR_INVALID_ARG; the planner, which only sees checked requests, says TH_ERR_INTERNAL)"""
    plan(lib, [(2, 0, 0, 100)], 4, err=-8)
