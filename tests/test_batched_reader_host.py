"""The entry protocol of the batched readers (thesia_amd/csrc/batched_reader.h: br::batched_read, the split by owner, the scatter-back,
the two layouts, br::single_read) over fake readers and fake managers.  CPU only: tests/emu/emu_batched_reader.cpp is compiled here
with g++ (once; the library is kept under tests/emu/_build and rebuilt when a source is newer).  The fakes log what the driver asks of
them, in order; a manager is one owner or two owners (odd ids on slot 0, even ids on slot 1)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thesia_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "emu", "emu_batched_reader.cpp")]
DEPS = SRC + [os.path.join(CSRC, h) for h in ("batched_reader.h", "common.h")] + [os.path.join(ROOT, "include", "thesia_amd.h")]
LIB = os.path.join(ROOT, "tests", "emu", "_build", "libemu_batched_reader.so")
OK, INVALID, UNSUPPORTED, HIP, TOO_SMALL, NOT_FOUND = 0, -1, -2, -3, -6, -7
SINGLE, MULTI, NULL_MANAGER = 0, 1, 2
ALIGNED, COUNTING, OPTIONAL = 0, 1, 2  # the readers: records at multiples of 64 / back to back with infos the run updates / + optional out
REQS_NULL, INFO_NULL, OUT_NULL, LEN_NULL, FAIL_RUN = 1, 2, 4, 8, 16
BEFORE_LOCK, LOCK, LOCK_OWNER, CHECK, FIT, REVISION, BEFORE_RUN, RUN = range(1, 9)
CANARY, INFO_CANARY, LEN_CANARY = 0xA5, 0xDEAD, 0xBEEF
REV = {COUNTING: (41, 7777), OPTIONAL: (41, 7777), ALIGNED: (7777, 42)}  # (waveform, spectrogram): the manager's where the reader stamps
ABA = [(1, 10, 0), (2, 70, 0), (3, 5, 0)]  # owners A, B, A of the two-owner manager


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall", "-Werror", "-o", LIB] + SRC)
    return C.CDLL(LIB)


def test_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "thesia_amd.h")).read()
    for name, v in (("OK", OK), ("ERR_INVALID_ARG", INVALID), ("ERR_HIP", HIP), ("ERR_BUFFER_TOO_SMALL", TOO_SMALL), ("ERR_NOT_FOUND", NOT_FOUND)):
        assert re.search(r"TH_%s = %d\b" % (name, v), text)


def call(lib, manager, reader, reqs, cap=4096, flags=0, fit_limit=2 ** 63):
    """-> dict(rc, msg, len, infos (n x 6: offset, length, bytes, waveform_revision, spectrogram_revision, count), out, log)"""
    n = len(reqs)
    rq = np.array(reqs, np.int64).reshape(n, 3).view(np.uint64)  # (a fault is a negative code)
    out = np.full(max(cap, 1) + 64, CANARY, np.uint8)
    info = np.full((max(n, 1), 6), INFO_CANARY, np.uint64)
    out_len = C.c_uint64(LEN_CANARY)
    msg = C.create_string_buffer(512)
    log = np.zeros(4096, np.uint64)
    log_len = C.c_size_t(0)
    u64p = C.POINTER(C.c_uint64)
    rc = lib.emu_batched_reader(manager, reader, flags, C.c_uint64(fit_limit), rq.ctypes.data_as(u64p), C.c_size_t(n),
                                out.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(cap), info.ctypes.data_as(u64p), C.byref(out_len),
                                msg, C.c_size_t(512), log.ctypes.data_as(u64p), C.c_size_t(log.size), C.byref(log_len))
    assert log_len.value <= log.size
    return dict(rc=rc, msg=msg.value.decode(), len=out_len.value, infos=info[:n].astype(np.int64), out=out, log=parse(log[:log_len.value]))


def parse(v):
    v, at, ev = [int(x) for x in v], 0, []
    while at < len(v):
        k = v[at]
        if k == BEFORE_LOCK:
            ev.append(("before_lock", bool(v[at + 1])))
            at += 2
        elif k == LOCK:
            ev.append(("lock",))
            at += 1
        elif k == LOCK_OWNER:
            ev.append(("lock_owner", v[at + 1]))
            at += 2
        elif k == CHECK:
            ev.append(("check", v[at + 1], v[at + 2]))
            at += 3
        elif k == REVISION:
            ev.append(("revision", "spectrogram" if v[at + 1] else "waveform"))
            at += 2
        elif k == BEFORE_RUN:
            ev.append(("before_run", bool(v[at + 1]), tuple(v[at + 3: at + 3 + v[at + 2]])))
            at += 3 + v[at + 2]
        else:
            assert k == RUN, k
            n = v[at + 2]  # rows of (id, offset, plan.offset, waveform_revision, spectrogram_revision)
            ev.append(("run", v[at + 1], tuple(tuple(v[at + 3 + 5 * i: at + 8 + 5 * i]) for i in range(n))))
            at += 3 + 5 * n
    return ev


def untouched(r):
    return (r["out"] == CANARY).all()


def nothing_published(r, n_zeroed_len=True):
    return (r["infos"] == INFO_CANARY).all() and untouched(r) and r["len"] == (0 if n_zeroed_len else LEN_CANARY)


MANAGERS, READERS = (SINGLE, MULTI), (ALIGNED, COUNTING)


@pytest.mark.parametrize("reader", READERS)
@pytest.mark.parametrize("manager", MANAGERS)
def test_null_arguments_come_first(lib, manager, reader):
    bad = [(100, 1, 0), (1, 1, INVALID)]  # faulty requests and n == 0 do not get a word in
    for m, flags, reqs in ((NULL_MANAGER, 0, bad), (manager, LEN_NULL, bad), (manager, REQS_NULL, bad), (manager, INFO_NULL, bad), (manager, LEN_NULL, [])):
        r = call(lib, m, reader, reqs, flags=flags)
        assert (r["rc"], r["msg"], r["log"]) == (INVALID, "NULL argument", [])
        assert nothing_published(r, n_zeroed_len=False)


@pytest.mark.parametrize("reader", READERS)
@pytest.mark.parametrize("manager", MANAGERS)
def test_no_requests_is_ok_and_writes_only_the_length(lib, manager, reader):
    for flags in (0, REQS_NULL | INFO_NULL | OUT_NULL):  # the arrays may be NULL for n == 0
        r = call(lib, manager, reader, [], flags=flags)
        assert (r["rc"], r["len"], r["log"]) == (OK, 0, []) and nothing_published(r)  # not even a lock


@pytest.mark.parametrize("reader", READERS)
@pytest.mark.parametrize("manager", MANAGERS)
def test_the_first_faulty_request_decides_and_nothing_is_written(lib, manager, reader):
    r = call(lib, manager, reader, [(1, 10, 0), (2, 10, UNSUPPORTED), (3, 10, INVALID), (4, 10, 0)], cap=0, fit_limit=1)
    assert (r["rc"], r["msg"]) == (UNSUPPORTED, "request 1: fault -2") and nothing_published(r)  # before the fit and the short buffer
    assert [e for e in r["log"] if e[0] == "check"] == [("check", 0 if manager == SINGLE else s, i) for i, s in ((0, 0), (1, 1))]
    assert not [e for e in r["log"] if e[0] in ("run", "revision", "before_run")]
    r = call(lib, manager, reader, [(1, 10, 0), (100, 10, 0), (3, 10, INVALID)])
    assert r["rc"] == NOT_FOUND and nothing_published(r)
    # an unknown id: the single owner's check says so; with two owners nobody owns it and the driver says so
    assert r["msg"] == ("request 1: Track 100 does not exist" if manager == SINGLE else "Track 100 does not exist")


@pytest.mark.parametrize("reader", READERS)
@pytest.mark.parametrize("manager", MANAGERS)
def test_a_short_buffer_publishes_infos_and_length_and_leaves_out_alone(lib, manager, reader):
    want_off, total = ([0, 64, 192], 197) if reader == ALIGNED else ([0, 10, 80], 85)
    for cap, flags in ((total - 1, 0), (0, 0), (4096, OUT_NULL)):
        r = call(lib, manager, reader, ABA, cap=cap, flags=flags)
        assert (r["rc"], r["len"]) == (TOO_SMALL, total) and untouched(r)
        assert r["msg"] == "need %d %s" % (total, "bytes" if reader == ALIGNED else "doubles")
        assert r["infos"][:, 0].tolist() == want_off and r["infos"][:, 1].tolist() == [10, 70, 5]
        assert [tuple(x) for x in r["infos"][:, 3:5]] == [REV[reader]] * 3  # the manager's revision, not an owner's
        assert (r["infos"][:, 5] == 0).all() and not [e for e in r["log"] if e[0] in ("run", "before_run")]
    assert call(lib, manager, reader, ABA, cap=total)["rc"] == OK


@pytest.mark.parametrize("reader", READERS)
def test_one_owner_runs_the_whole_batch_in_order(lib, reader):
    r = call(lib, SINGLE, reader, ABA)
    off = [0, 64, 192] if reader == ALIGNED else [0, 10, 80]
    which = "spectrogram" if reader == ALIGNED else "waveform"
    assert r["log"] == [("before_lock", reader == ALIGNED), ("lock",), ("check", 0, 0), ("check", 0, 1), ("check", 0, 2), ("revision", which),
                        ("run", 0, tuple((i, o, o) + REV[reader] for (i, _, _), o in zip(ABA, off)))]
    check_output(r, reader, off)


def check_output(r, reader, off):
    want = np.full(r["out"].size, CANARY, np.uint8)
    for (i, length, _), o in zip(ABA, off):
        want[o: o + length] = i
    assert r["rc"] == OK and (r["out"] == want).all()  # the records, and canaries between and behind them
    assert r["infos"][:, 0].tolist() == off and r["infos"][:, 5].tolist() == ([0, 0, 0] if reader == ALIGNED else [1001, 1002, 1003])
    assert [tuple(x) for x in r["infos"][:, 3:5]] == [REV[reader]] * 3


@pytest.mark.parametrize("reader", READERS)
def test_two_owners_each_run_their_subset_with_the_batchs_offsets(lib, reader):
    r = call(lib, MULTI, reader, ABA)
    off = [0, 64, 192] if reader == ALIGNED else [0, 10, 80]
    rows = [(i, o, o) + REV[reader] for (i, _, _), o in zip(ABA, off)]
    which = "spectrogram" if reader == ALIGNED else "waveform"
    assert r["log"] == [("before_lock", reader == ALIGNED), ("lock",),
                        ("lock_owner", 0), ("check", 0, 0), ("lock_owner", 1), ("check", 1, 1), ("lock_owner", 0), ("check", 0, 2),
                        ("revision", which), ("before_run", reader == ALIGNED, (0, 1)),  # (after the short-buffer report: see above)
                        ("lock_owner", 0), ("run", 0, (rows[0], rows[2])), ("lock_owner", 1), ("run", 1, (rows[1],))]
    check_output(r, reader, off)  # the counts of A, B, A are back at 0, 1, 2
    r = call(lib, MULTI, reader, [(2, 3, 0), (4, 3, 0)])  # only one slot is busy
    assert [e for e in r["log"] if e[0] in ("before_run", "run")][0] == ("before_run", reader == ALIGNED, (1,))
    assert [e[1] for e in r["log"] if e[0] == "run"] == [1]


@pytest.mark.parametrize("reader", READERS)
@pytest.mark.parametrize("manager", MANAGERS)
def test_a_failed_run_leaves_the_published_infos(lib, manager, reader):
    r = call(lib, manager, reader, ABA, flags=FAIL_RUN)
    assert r["rc"] == HIP and r["msg"] == ("the run failed" if manager == SINGLE else "slot 1 (device 0): the run failed")
    assert r["len"] == (197 if reader == ALIGNED else 85) and r["infos"][:, 1].tolist() == [10, 70, 5]
    assert (r["infos"][:, 5] == 0).all()  # not even the counts of the slot that succeeded
    assert len([e for e in r["log"] if e[0] == "run"]) == (1 if manager == SINGLE else 2)


@pytest.mark.parametrize("reader", READERS)
def test_the_fit_step_is_the_single_owners_and_comes_before_the_short_buffer(lib, reader):
    r = call(lib, SINGLE, reader, ABA, cap=0, fit_limit=2)
    assert (r["rc"], r["msg"]) == (INVALID, "at most 2 requests per call") and nothing_published(r)
    assert [e[0] for e in r["log"]][-1] == "check"  # after every check, before the stamp
    assert call(lib, SINGLE, reader, ABA, fit_limit=3)["rc"] == OK
    r = call(lib, MULTI, reader, ABA, cap=0, fit_limit=2)
    assert r["rc"] == TOO_SMALL and r["len"] > 0
    assert call(lib, MULTI, reader, ABA, fit_limit=2)["rc"] == OK


@pytest.mark.parametrize("manager", MANAGERS)
def test_an_optional_output_may_be_null_but_not_short(lib, manager):
    r = call(lib, manager, OPTIONAL, ABA, cap=0, flags=OUT_NULL)  # NULL: the run still fills the infos
    assert (r["rc"], r["len"]) == (OK, 85) and r["infos"][:, 5].tolist() == [1001, 1002, 1003] and untouched(r)
    r = call(lib, manager, OPTIONAL, ABA, cap=84)
    assert (r["rc"], r["msg"], r["len"]) == (TOO_SMALL, "need 85 doubles", 85) and untouched(r) and (r["infos"][:, 5] == 0).all()
    assert call(lib, manager, OPTIONAL, ABA, cap=85)["rc"] == OK


def test_single_read_copies_the_info_when_one_was_published(lib):
    for rc, copied in ((OK, True), (TOO_SMALL, True), (INVALID, False), (NOT_FOUND, False), (HIP, False)):
        info = C.c_uint64(INFO_CANARY)
        assert lib.emu_single_read(rc, C.byref(info)) == rc and info.value == (5 if copied else INFO_CANARY)
        assert lib.emu_single_read(rc, None) == rc
