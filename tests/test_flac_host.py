"""The host half of the FLAC export (th_flac_encode_i32, th_flac_frame_header, th_flac_bound) against a strict decoder and a numpy
model of the encoder's decisions (tests/flac_ref.py).  CPU only.  FLAC is lossless, so the oracle is exact: decode(encode(x)) == x,
and every subframe's type, order, partition order and Rice parameters, and every file's length, equal the model's.  The decoder
itself is pinned to a real encoder's output: tests/golden/flac_libflac_head.flac is the head of a libFLAC file (40 frames)."""
import collections
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi
from thesia_amd._ffi import lib
from tests import flac_ref as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FMT = {16: ta.PCM_S16, 24: ta.PCM_S24}
LENGTHS = [1, 4, 5, 15, 16, 63, 64, 4095, 4096, 4097, 8192 + 17]


def raises(code, fn):
    with pytest.raises(ta.ThError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))


@pytest.fixture(scope="module")
def golden():
    data = open(os.path.join(GOLDEN, "flac_libflac_head.flac"), "rb").read()
    meta = json.load(open(os.path.join(GOLDEN, "flac_libflac_head.json")))
    return data, meta, F.decode(data)


def signal(kind, n, bps, seed=0):
    S = 1 << (bps - 1)
    i = np.arange(n, dtype=np.int64)
    if kind == "sine":
        return np.rint(0.4 * S * np.sin(2 * np.pi * 997.0 * i / 48000.0)).astype(np.int64)
    if kind == "ramp":
        return 3 * i - 1000
    if kind == "silence":
        return np.zeros(n, np.int64)
    if kind == "noise":
        return np.random.default_rng(seed).integers(-S, S, n, dtype=np.int64)
    if kind == "alternating":
        return np.where(i % 2 == 0, -S, S - 1).astype(np.int64)
    if kind == "music":  # a decaying chord over a little noise: partitions with different parameters
        env = np.exp(-(i % 3000) / 900.0)
        x = 0.3 * env * (np.sin(2 * np.pi * 220.0 * i / 48000.0) + 0.5 * np.sin(2 * np.pi * 331.0 * i / 48000.0))
        return np.rint(S * x + np.random.default_rng(seed).normal(0, 2.0, n)).astype(np.int64)
    raise ValueError(kind)


def check_stream(chans, bps, sr):
    """encode, decode, compare with the input and with the model; -> (file, decoded)"""
    chans = np.asarray(chans, np.int64).reshape(len(chans), -1)
    n_ch, n = chans.shape
    data = ta.flac_encode_i32(chans.astype(np.int32), FMT[bps], sr)
    dec = F.decode(data)
    assert (dec["sr"], dec["n_ch"], dec["bps"], dec["total"]) == (sr, n_ch, bps, n)
    assert (dec["min_block"], dec["max_block"]) == (4096, 4096) and dec["md5"] == bytes(16) and dec["first_frame"] == 42
    assert np.array_equal(np.array(dec["channels"], np.int64).reshape(n_ch, -1), chans)
    total, frames, sizes = F.model_stream(chans, bps, sr)
    assert len(data) == total
    assert [f["size"] for f in dec["frames"]] == sizes
    assert (dec["min_frame"], dec["max_frame"]) == ((min(sizes), max(sizes)) if sizes else (0, 0))
    for b, (f, want) in enumerate(zip(dec["frames"], frames)):
        assert f["number"] == b and f["variable"] == 0 and f["block"] == min(4096, n - 4096 * b)
        for c, (got, w) in enumerate(zip(f["subframes"], want)):
            assert F.same_decisions(got, w), (b, c, got, w)
    assert len(data) <= ta.flac_bound(n, n_ch, FMT[bps]) == F.bound(n, n_ch, bps)
    return data, dec


def test_decoder_on_a_real_encoders_file(golden):
    data, meta, dec = golden
    assert len(dec["frames"]) == meta["frames"] and len(dec["channels"][0]) == meta["samples"]
    assert (dec["sr"], dec["n_ch"], dec["bps"], dec["first_frame"]) == (meta["sr"], meta["channels"], meta["bps"], meta["first_frame"])
    assert all(f["block"] == meta["block"] for f in dec["frames"])
    assert hashlib.sha256(F.pcm_bytes(dec)).hexdigest() == meta["pcm_sha256"]
    census = collections.Counter("%s%d" % (s["type"], s["order"]) for f in dec["frames"] for s in f["subframes"])
    assert dict(census) == meta["census"]
    assert len(data) - dec["first_frame"] == meta["libflac_frame_bytes"]


@pytest.mark.parametrize("byte, bit", [(100 + 7, 3), (100 + 2000, 0), (112232 - 1, 7), (100 + 3, 6)])
def test_decoder_rejects_a_flipped_bit(golden, byte, bit):
    data = bytearray(golden[0])
    data[byte] ^= 1 << bit
    with pytest.raises(F.FlacError):
        F.decode(bytes(data))


def test_fixture_audio_size(golden):
    """this encoder's size of the fixture's audio is the model's, beside libFLAC's LPC encoding of the same samples"""
    _, meta, dec = golden
    x = np.array(dec["channels"], np.int64)
    data, _ = check_stream(x, 16, 44100)
    assert len(data) - 42 == meta["model_frame_bytes"]
    assert meta["libflac_frame_bytes"] < len(data) - 42 < 2 * x.size  # (above libFLAC's, well below the PCM's 2 bytes a sample)


@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("kind", ["sine", "ramp", "silence", "noise", "alternating", "music"])
def test_signals(kind, bps):
    _, dec = check_stream([signal(kind, 8192 + 17, bps)], bps, 48000)
    types = {(s["type"], s["order"]) for f in dec["frames"] for s in f["subframes"]}
    if kind == "ramp":
        assert types == {("fixed", 2)}
        assert all(set(s["params"]) == {0} for f in dec["frames"] for s in f["subframes"])
    elif kind == "silence":
        assert types == {("constant", 0)}
    elif kind == "noise":
        assert types == {("verbatim", 0)}
    elif kind == "alternating":  # order 0 is the cheapest: the higher orders' residuals only grow, to 2^(bps + 3) at order 4
        assert types <= {("fixed", 0), ("verbatim", 0)}
    else:
        assert all(t == "fixed" for t, _ in types)


@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(n, bps):
    check_stream([signal("sine", n, bps), signal("music", n, bps, seed=n)], bps, 44100)


@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("n_ch", [1, 2, 3, 8])
def test_channels(n_ch, bps):
    kinds = ["music", "sine", "silence", "noise", "ramp", "alternating", "music", "sine"]
    check_stream([signal(kinds[c], 4097, bps, seed=c) for c in range(n_ch)], bps, 12345)


def test_largest_order4_residual():
    """-S, S - 1 alternating at 24 bit: the order-4 residual reaches 2^27 - 8 in magnitude; the sums stay exact"""
    x = signal("alternating", 4096, 24)
    e = np.diff(x, 4)
    assert np.abs(e).max() == (1 << 27) - 8
    check_stream([x], 24, 96000)


def test_empty_stream():
    data, dec = check_stream(np.zeros((2, 0), np.int64), 16, 48000)
    assert len(data) == 42 and dec["frames"] == []


def header_ref(sr, n_ch, bps, number, n):
    """the frame header restated from the contract"""
    table = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
    rc = table.get(sr, 13 if sr <= 65535 else 14 if sr % 10 == 0 and sr // 10 <= 65535 else 0)
    bc = 12 if n == 4096 else 6 if n <= 256 else 7
    out = bytearray([0xFF, 0xF8, (bc << 4) | rc, ((n_ch - 1) << 4) | ((4 if bps == 16 else 6) << 1)])
    if number < 0x80:
        out.append(number)
    else:
        nb = next(k for k in range(2, 8) if number < (1 << (5 * k + 1)))
        out.append(((0xFF00 >> nb) & 0xFF) | (number >> (6 * (nb - 1))))
        out += bytes(0x80 | ((number >> (6 * (nb - 1 - j))) & 0x3F) for j in range(1, nb))
    if bc == 6:
        out.append(n - 1)
    elif bc == 7:
        out += (n - 1).to_bytes(2, "big")
    if rc == 13:
        out += sr.to_bytes(2, "big")
    elif rc == 14:
        out += (sr // 10).to_bytes(2, "big")
    out.append(F.crc8(out))
    return bytes(out)


@pytest.mark.parametrize("number", [0, 127, 128, 2047, 2048, 65535, 65536, 2 ** 31 - 1])
@pytest.mark.parametrize("n", [1, 256, 257, 4096])
def test_frame_header(number, n):
    for sr in (48000, 12345, 200000, 1048575):
        for n_ch, bps in ((1, 16), (8, 24)):
            got = ta.flac_frame_header(sr, n_ch, FMT[bps], number, n)
            assert got == header_ref(sr, n_ch, bps, number, n), (sr, n_ch, bps, number, n)
            assert len(got) == F.header_len(sr, number, n) <= 16


def test_frame_header_in_a_stream():
    """rates in and out of the table travel through a whole stream (the decoder checks them against STREAMINFO)"""
    for sr in (48000, 12345, 200000, 1048575):
        check_stream([signal("sine", 300, 16)], 16, sr)


def test_errors():
    x = np.zeros((9, 16), np.int32)
    raises(_ffi.ERR_UNSUPPORTED, lambda: ta.flac_encode_i32(x, ta.PCM_S16, 48000))
    raises(_ffi.ERR_UNSUPPORTED, lambda: ta.flac_encode_i32(x[:2], ta.PCM_S16, 1048576))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_encode_i32(x[:2], ta.PCM_F32, 48000))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_encode_i32(x[:2], ta.PCM_S16, 0))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_encode_i32(x[:2] + 32768, ta.PCM_S16, 48000))  # not a 16-bit integer
    raises(_ffi.ERR_UNSUPPORTED, lambda: ta.flac_bound(16, 9, ta.PCM_S16))
    raises(_ffi.ERR_UNSUPPORTED, lambda: ta.flac_bound(1 << 36, 1, ta.PCM_S16))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_bound(16, 2, ta.PCM_F32))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_bound(16, 0, ta.PCM_S16))
    raises(_ffi.ERR_UNSUPPORTED, lambda: ta.flac_frame_header(1048576, 1, ta.PCM_S16, 0, 4096))
    raises(_ffi.ERR_UNSUPPORTED, lambda: ta.flac_frame_header(48000, 9, ta.PCM_S16, 0, 4096))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_frame_header(48000, 1, ta.PCM_F32, 0, 4096))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_frame_header(48000, 1, ta.PCM_S16, 0, 0))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_frame_header(48000, 1, ta.PCM_S16, 0, 4097))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_frame_header(48000, 1, ta.PCM_S16, 1 << 36, 4096))
    # NULL pointers
    n = C.c_size_t()
    assert lib.th_flac_encode_i32(None, 1, 16, ta.PCM_S16, 48000, None, 0, C.byref(n)) == _ffi.ERR_INVALID_ARG
    ptrs = (C.POINTER(C.c_int32) * 1)()
    assert lib.th_flac_encode_i32(ptrs, 1, 16, ta.PCM_S16, 48000, None, 0, C.byref(n)) == _ffi.ERR_INVALID_ARG
    assert lib.th_flac_encode_i32(ptrs, 1, 0, ta.PCM_S16, 48000, None, 0, None) == _ffi.ERR_INVALID_ARG
    assert lib.th_flac_bound(16, 1, ta.PCM_S16, None) == _ffi.ERR_INVALID_ARG
    assert lib.th_flac_frame_header(48000, 1, ta.PCM_S16, 0, 4096, None, C.byref(n)) == _ffi.ERR_INVALID_ARG


def test_short_buffer_reports_the_bound():
    x = np.ascontiguousarray(signal("sine", 5000, 16).astype(np.int32))
    ptrs = (C.POINTER(C.c_int32) * 1)(x.ctypes.data_as(C.POINTER(C.c_int32)))
    n = C.c_size_t()
    want = F.bound(5000, 1, 16)
    assert want == 42 + (16 + 1 + 8192 + 3) + (16 + 1 + 2 * 904 + 3)
    buf = np.zeros(want, np.uint8)
    assert lib.th_flac_encode_i32(ptrs, 1, 5000, ta.PCM_S16, 48000, buf.ctypes.data, want - 1, C.byref(n)) == _ffi.ERR_BUFFER_TOO_SMALL
    assert n.value == want and not buf.any()
    assert lib.th_flac_encode_i32(ptrs, 1, 5000, ta.PCM_S16, 48000, buf.ctypes.data, want, C.byref(n)) == _ffi.OK
    assert 42 < n.value < want and bytes(buf[:4]) == b"fLaC"
