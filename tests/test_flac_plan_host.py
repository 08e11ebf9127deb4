"""plan_flac / bind_flac (thesia_amd/csrc/flac_plan.h): pieces of whole blocks, the bound per piece, where a job's slots, tables and
staging lie, and a call of more than two pieces.  CPU only: tests/emu/emu_flac_plan.cpp is compiled here with g++ beside flac_plan.cpp
(once; the library is kept under tests/emu/_build and rebuilt when a source is newer)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from thesia_amd import api
from tests import flac_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thesia_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "emu", "emu_flac_plan.cpp"), os.path.join(CSRC, "flac_plan.cpp")]
DEPS = SRC + [os.path.join(CSRC, h) for h in ("flac_plan.h", "flac_core.h", "stft_core.h")] + [os.path.join(ROOT, "include", "thesia_amd.h")]
LIB = os.path.join(ROOT, "tests", "emu", "_build", "libemu_flac_plan.so")
BASES = (0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000, 0x80000000)
PIECE = api.EXPORT_PIECE_BYTES
MAX_UNITS = 1 << 16
BPS = {0: 16, 1: 24}
JOB_BYTES = 128


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-o", LIB] + SRC)
    so = C.CDLL(LIB)
    so.emu_flac_plan.restype = C.c_int64
    return so


def frame_bound(n, n_ch, bps):
    return 16 + n_ch * (1 + n * bps // 8) + 3


def plan(lib, reqs, piece=PIECE):
    """reqs: (n_ch, fmt, s0, s1) -> dict of the plan"""
    rows, at = [], 0
    for n_ch, fmt, s0, s1 in reqs:
        rows += [n_ch, fmt, 1, 7, 48000, s0, s1, at]
        at = (at + F.bound(s1 - s0, n_ch, BPS[fmt]) + 15) // 16 * 16
    rows = np.array(rows, np.uint64)
    out = np.zeros(1 << 20, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    n = lib.emu_flac_plan(rows.ctypes.data_as(u64p), C.c_uint64(len(reqs)), C.c_uint64(piece), (C.c_uint64 * 8)(*BASES), out.ctypes.data_as(u64p),
                          C.c_uint64(out.size))
    assert n > 0
    v = [int(x) for x in out[:n]]
    assert v[0] == 0
    keys = ("n_pieces", "n_runs", "stage0", "stage1", "slot_need", "unit_need", "block_need", "o_ptrs", "tab_bytes")
    p = dict(zip(keys, v[1:10]))
    at = 10
    p["pieces"] = [dict(zip(("run0", "run1", "n_units", "n_blocks", "bound", "slot_words"), v[at + 6 * i: at + 6 * i + 6])) for i in range(p["n_pieces"])]
    at += 6 * p["n_pieces"]
    rk = ("req", "b0", "nb", "first_unit", "first_block", "slot_words", "slot_at", "stage_at", "bound", "chan", "slots", "bits", "foff", "dst", "cnt",
          "res", "s0", "s1", "jb0", "jnb", "n_ch", "format", "dither", "seed", "sr")
    p["runs"] = [dict(zip(rk, v[at + len(rk) * i: at + len(rk) * (i + 1)])) for i in range(p["n_runs"])]
    at += len(rk) * p["n_runs"]
    p["ptrs"] = v[at:]
    return p


def check_plan(p, reqs, piece=PIECE):
    """every block of every request once and in order; pieces of whole blocks within the piece size; addresses inside their areas"""
    assert p["o_ptrs"] == JOB_BYTES * p["n_runs"] and p["tab_bytes"] == p["o_ptrs"] + 8 * sum(r[0] for r in reqs)
    assert p["ptrs"] == [0x1000 * (i + 1) + c for i, r in enumerate(reqs) for c in range(r[0])]
    next_block = [0] * len(reqs)
    run_at, chan0 = 0, np.cumsum([0] + [r[0] for r in reqs])
    for pi, pc in enumerate(p["pieces"]):
        assert pc["run0"] == run_at and pc["run1"] > pc["run0"]
        run_at = pc["run1"]
        units = blocks = bound = slots = 0
        for k in range(pc["run0"], pc["run1"]):
            r = p["runs"][k]
            n_ch, fmt, s0, s1 = reqs[r["req"]]
            bps, n = BPS[fmt], s1 - s0
            assert r["b0"] == next_block[r["req"]] and r["nb"] >= 1
            next_block[r["req"]] += r["nb"]
            lens = [min(4096, n - 4096 * b) for b in range(r["b0"], r["b0"] + r["nb"])]
            assert min(lens) >= 1
            assert r["bound"] == sum(frame_bound(m, n_ch, bps) for m in lens)
            assert len(set(lens)) == 1 and r["slot_words"] == (8 + lens[0] * bps + 31) // 32  # (slots of the blocks' own size)
            assert (r["first_unit"], r["first_block"], r["slot_at"], r["stage_at"]) == (units, blocks, slots, bound)
            assert (r["s0"], r["s1"], r["jb0"], r["jnb"], r["n_ch"], r["format"], r["dither"], r["seed"], r["sr"]) == (s0, s1, r["b0"], r["nb"], n_ch, fmt, 1, 7, 48000)
            assert r["chan"] == BASES[6] + p["o_ptrs"] + 8 * int(chan0[r["req"]])
            assert r["slots"] == BASES[2] + 4 * slots and r["bits"] == BASES[3] + 4 * units and r["foff"] == BASES[4] + 4 * blocks
            assert r["dst"] == BASES[pi & 1] + bound and r["cnt"] == BASES[7] + 16 * r["req"] and r["res"] == BASES[5] + 16 * k
            units += r["nb"] * n_ch
            blocks += r["nb"]
            slots += r["nb"] * n_ch * r["slot_words"]
            bound += r["bound"]
        assert (pc["n_units"], pc["n_blocks"], pc["bound"], pc["slot_words"]) == (units, blocks, bound, slots)
        assert units <= MAX_UNITS and (bound <= piece or blocks == 1)
        assert 4 * slots <= bound + 4 * units  # (the slot scratch never exceeds a piece's bound and a word per unit)
        assert bound <= p["stage%d" % (pi & 1)] and slots <= p["slot_need"] and units <= p["unit_need"] and blocks <= p["block_need"]
    assert run_at == p["n_runs"]
    assert next_block == [(r[3] - r[2] + 4095) // 4096 for r in reqs]
    # a piece is closed only when the next block would not fit
    for pc, nxt in zip(p["pieces"], p["pieces"][1:]):
        r = p["runs"][nxt["run0"]]
        n_ch, fmt, s0, s1 = reqs[r["req"]]
        first = frame_bound(min(4096, s1 - s0 - 4096 * r["b0"]), n_ch, BPS[fmt])
        assert pc["bound"] + first > piece or pc["n_units"] + n_ch > MAX_UNITS


def test_one_small_request(lib):
    reqs = [(2, 0, 100, 100 + 5003)]
    p = plan(lib, reqs)
    check_plan(p, reqs)
    assert (p["n_pieces"], p["n_runs"]) == (1, 2) and [r["nb"] for r in p["runs"]] == [1, 1]  # (the short block is a run of its own)
    assert [r["slot_words"] for r in p["runs"]] == [2049, (8 + 907 * 16 + 31) // 32]
    assert p["pieces"][0]["bound"] == F.bound(5003, 2, 16) - 42


def test_empty_requests_have_no_runs(lib):
    reqs = [(1, 0, 5, 5), (2, 1, 0, 10), (3, 0, 7, 7)]
    p = plan(lib, reqs)
    check_plan(p, reqs)
    assert (p["n_pieces"], p["n_runs"]) == (1, 1) and p["runs"][0]["req"] == 1
    assert plan(lib, [(1, 0, 5, 5)])["n_pieces"] == 0


def test_a_mixed_batch_in_one_piece(lib):
    reqs = [(1, 0, 0, 1), (2, 1, 3, 4099), (8, 1, 0, 4096 * 3), (3, 0, 1, 4095), (6, 0, 0, 4097)]
    p = plan(lib, reqs)
    check_plan(p, reqs)
    assert p["n_pieces"] == 1 and p["n_runs"] == 6
    assert [r["slot_words"] for r in p["runs"]] == [1, 3073, 3073, 2048, 2049, 1]
    assert p["pieces"][0]["slot_words"] * 4 <= p["pieces"][0]["bound"] + 4 * p["pieces"][0]["n_units"]  # (what the slot scratch is bounded by)


def test_a_request_of_more_than_two_pieces(lib):
    """the GPU test's track: 5452 whole blocks fill two pieces, the short block opens a third"""
    fb = frame_bound(4096, 1, 24)
    full = (2 * PIECE - 42) // fb
    m = (2 * PIECE - 42 - full * fb - 20) // 3 + 1
    reqs = [(1, 1, 0, full * 4096 + m)]
    p = plan(lib, reqs)
    check_plan(p, reqs)
    assert p["n_pieces"] == 3 and [r["nb"] for r in p["runs"]] == [PIECE // fb, PIECE // fb, 1]
    assert p["stage0"] == (PIECE // fb) * fb == p["stage1"] and p["runs"][2]["slot_words"] == (8 + 24 * m + 31) // 32


def test_small_pieces_cut_at_blocks_and_across_requests(lib):
    reqs = [(2, 0, 0, 4096 * 5 + 17), (1, 1, 9, 9 + 4096 * 2), (2, 0, 0, 300)]
    piece = 3 * frame_bound(4096, 2, 16) + 100
    p = plan(lib, reqs, piece)
    check_plan(p, reqs, piece)
    assert p["n_pieces"] >= 3
    assert [(r["req"], r["b0"], r["nb"]) for r in p["runs"]][:4] == [(0, 0, 3), (0, 3, 2), (0, 5, 1), (1, 0, 1)]
    # a piece smaller than one block still takes it
    p = plan(lib, reqs, 1000)
    check_plan(p, reqs, 1000)
    assert p["n_pieces"] == p["n_runs"] == 6 + 2 + 1


def test_the_unit_limit_closes_a_piece(lib):
    reqs = [(8, 0, 0, 3)] * (MAX_UNITS // 8 + 2)
    p = plan(lib, reqs)
    check_plan(p, reqs)
    assert p["n_pieces"] == 2 and p["pieces"][0]["n_units"] == MAX_UNITS and p["pieces"][1]["n_units"] == 16


def test_many_requests_just_over_a_block(lib):
    """every request a whole block and a block of one sample: the short blocks' slots are small ones"""
    reqs = [(8, 1, 0, 4097)] * 300
    p = plan(lib, reqs)
    check_plan(p, reqs)
    assert p["n_runs"] == 600 and 4 * p["slot_need"] <= PIECE + 4 * MAX_UNITS
