"""The host half of the FLAC export's _ex entries (th_flac_encode_i32_ex: TH_FLAC_LPC, TH_FLAC_STEREO) against the strict decoder
of tests/flac_ref.py and the model of tests/flac_lpc_ref.py.  CPU only.  For every flags value decode(encode(x)) == x; every subframe's
type, order, precision, shift, coefficients, partition order and Rice parameters, every frame's channel assignment and the file's
length are the model's; flags == 0 is th_flac_encode_i32 byte for byte; and no frame is longer than the flags == 0 frame."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi
from thesia_amd._ffi import lib
from tests import flac_lpc_ref as M
from tests import flac_ref as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FMT = {16: ta.PCM_S16, 24: ta.PCM_S24}
FLAGS = [0, 1, 2, 3]


def raises(code, fn):
    with pytest.raises(ta.ThError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))


def signal(kind, n, bps, seed=0):
    S = 1 << (bps - 1)
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed)
    if kind == "ar2":  # a resonance near sr / 4, pole radius 0.98, driven by noise
        e, y = rng.normal(0, 0.04 * S, n + 1000), np.zeros(n + 1002)
        a1, a2 = 2 * 0.98 * np.cos(2 * np.pi * 0.24), -0.98 * 0.98
        for t in range(n + 1000):
            y[t + 2] = a1 * y[t + 1] + a2 * y[t] + e[t]
        return np.clip(np.rint(y[-n:]), -S, S - 1).astype(np.int64)  # (the tail: the process has settled)
    if kind == "sine":
        return np.rint(0.5 * S * np.sin(2 * np.pi * 1000.0 * i / 48000.0)).astype(np.int64)
    if kind == "alternating":
        return np.where(i % 2 == 0, -S, S - 1).astype(np.int64)
    if kind == "square":
        return np.where((i // 24) % 2 == 0, S - 1, -S).astype(np.int64)
    if kind == "impulse":
        return np.where(i == n // 2, S - 1, 0).astype(np.int64)
    if kind == "ramp":
        return 3 * i - 1000
    if kind == "noise":
        return rng.integers(-S, S, n, dtype=np.int64)
    if kind == "quiet":  # +-5 counts, whatever the format
        return rng.integers(-5, 6, n, dtype=np.int64)
    if kind == "silence":
        return np.zeros(n, np.int64)
    if kind == "music":
        env = np.exp(-(i % 3000) / 900.0)
        x = 0.3 * env * (np.sin(2 * np.pi * 220.0 * i / 48000.0) + 0.5 * np.sin(2 * np.pi * 331.0 * i / 48000.0))
        return np.rint(S * x + rng.normal(0, 2.0, n)).astype(np.int64)
    raise ValueError(kind)


def frame_sizes(chans, bps, sr):
    return F.model_stream(chans, bps, sr)[2]


def check_stream(chans, bps, sr, flags):
    """encode with flags, decode, compare with the input, the model and the flags == 0 frames; -> (file, decoded)"""
    chans = np.asarray(chans, np.int64).reshape(len(chans), -1)
    n_ch, n = chans.shape
    data = ta.flac_encode_i32(chans.astype(np.int32), FMT[bps], sr, flags=flags)
    if flags == 0:
        assert data == ta.flac_encode_i32(chans.astype(np.int32), FMT[bps], sr)
    dec = M.decode(data)
    assert (dec["sr"], dec["n_ch"], dec["bps"], dec["total"]) == (sr, n_ch, bps, n)
    assert (dec["min_block"], dec["max_block"]) == (4096, 4096) and dec["md5"] == bytes(16) and dec["first_frame"] == 42
    assert np.array_equal(np.array(dec["channels"], np.int64).reshape(n_ch, -1), chans)
    total, frames, sizes = M.model_stream(chans, bps, sr, flags)
    assert len(data) == total
    assert [f["size"] for f in dec["frames"]] == sizes
    assert (dec["min_frame"], dec["max_frame"]) == ((min(sizes), max(sizes)) if sizes else (0, 0))
    for b, (f, (code, want)) in enumerate(zip(dec["frames"], frames)):
        assert f["number"] == b and f["variable"] == 0 and f["block"] == min(4096, n - 4096 * b)
        assert f["assign"] == code, (b, f["assign"], code)
        for c, (got, w) in enumerate(zip(f["subframes"], want)):
            assert M.same_decisions(got, w), (b, c, got, w)
    plain = frame_sizes(chans, bps, sr)
    assert len(sizes) == len(plain) and all(a <= b for a, b in zip(sizes, plain))  # frame by frame
    assert len(data) <= ta.flac_bound(n, n_ch, FMT[bps]) == F.bound(n, n_ch, bps)
    return data, dec


def kinds_of(dec):
    return {(s["type"], s["order"]) for f in dec["frames"] for s in f["subframes"]}


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", [4096, 4095, 257, 64, 33, 9, 5])
def test_ar2_resonance(n, flags):
    """fixed 0 becomes LPC 2 down to 33 samples; at 9 and 5 the predictors' overhead leaves VERBATIM"""
    x = signal("ar2", n, 16, seed=n)
    data, dec = check_stream([x], 16, 48000, flags)
    plain = M.decode(ta.flac_encode_i32(x.astype(np.int32), ta.PCM_S16, 48000))
    if n <= 9:
        assert kinds_of(dec) == kinds_of(plain) == {("verbatim", 0)}
    elif flags & 1:
        assert kinds_of(plain) == {("fixed", 0)} and kinds_of(dec) == {("lpc", 2)}
        if n == 4096:
            assert len(data) < 0.9 * (42 + plain["frames"][0]["size"])
    else:
        assert kinds_of(dec) == kinds_of(plain)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("kind", ["sine", "alternating", "square", "impulse", "ramp", "noise", "quiet", "silence", "music"])
def test_signals(kind, bps, flags):
    n = 4096 + 257
    x = signal(kind, n, bps)
    data, dec = check_stream([x], bps, 48000, flags)
    kinds = kinds_of(dec)
    lpc = bool(flags & 1)
    if kind == "sine":
        first = dec["frames"][0]["subframes"][0]  # (the 4096-sample block; the 257-sample one has fewer residuals to pay the header)
        # fixed 4 becomes LPC 8 at 16 bit at this level (half of full scale; 0.4 gives LPC 6, 0.9 keeps fixed 4); at 24 bit the pure
        # tone's high orders gain nothing over LPC 4 within 14-bit coefficients, at any level from 0.4 to 1.0
        assert (first["type"], first["order"]) == (("lpc", 8 if bps == 16 else 4) if lpc else ("fixed", 4))
    elif kind == "alternating":  # s[i] = -s[i - 1] - 1: one coefficient predicts it to a count
        assert all(t == "lpc" for t, _ in kinds) if lpc else kinds <= {("fixed", 0), ("verbatim", 0)}
        if lpc and bps == 16:
            assert dec["frames"][0]["subframes"][0]["order"] >= 1 and len(data) < (42 + 4096 * 2 + 257 * 2) // 8
    elif kind in ("square", "impulse", "ramp"):  # the fixed predictor stays: the fit stops early or LPC loses on cost
        assert all(t in ("fixed", "constant") for t, _ in kinds) and ("fixed", 0 if kind == "impulse" else 2 if kind == "ramp" else 1) in kinds, kinds
    elif kind == "noise":
        assert kinds == {("verbatim", 0)}
    elif kind == "silence":
        assert kinds == {("constant", 0)}
    elif kind == "quiet":
        assert all(t in ("fixed", "lpc") for t, _ in kinds)


def test_alternating_bits():
    """-S, S - 1 alternating, 4096 samples at 16 bit: VERBATIM's 65 544 bits become an LPC subframe of 4 537"""
    x = signal("alternating", 4096, 16)
    plain = M.decode(ta.flac_encode_i32(x.astype(np.int32), ta.PCM_S16, 48000))
    assert kinds_of(plain) == {("verbatim", 0)} and 8 * (plain["frames"][0]["size"] - 6 - 2) == 65544
    sub = M.model_subframe(x, 16, 16, True)
    assert sub["type"] == "lpc" and sub["bits"] == 4537
    data, _ = check_stream([x], 16, 48000, 1)
    assert len(data) == 42 + 6 + (4537 + 7) // 8 + 2


def test_level_adaptive_window():
    """+-5 counts in a 24-bit file: sh = 0, the window keeps the passage's precision and the fit is that of the 16-bit file"""
    x = signal("quiet", 4096, 24)
    assert M.lpc_fit(x, 14).keys() == M.lpc_fit(x, 12).keys() != set()
    loud = x << 16
    assert M.lpc_fit(loud, 14).keys() != set()
    check_stream([loud], 24, 44100, 1)


STEREO_CASES = {
    "near": lambda a, rng: a + rng.integers(-3, 4, a.size),
    "inverted": lambda a, rng: -a,
    "unrelated": lambda a, rng: signal("ar2", a.size, 16 if np.abs(a).max() < 32768 else 24, seed=11),
    "equal": lambda a, rng: a.copy(),
}


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("case", sorted(STEREO_CASES))
def test_stereo(case, bps, flags):
    S = 1 << (bps - 1)
    left = signal("music", 4096 + 33, bps, seed=3) // 2
    right = np.clip(STEREO_CASES[case](left, np.random.default_rng(5)), -S, S - 1)
    data, dec = check_stream([left, right], bps, 44100, flags)
    codes = {f["assign"] for f in dec["frames"]}
    if not flags & 2:
        assert codes == {1}
        return
    plain = ta.flac_encode_i32(np.array([left, right], np.int32), FMT[bps], 44100, flags=flags & 1)
    if case == "near":
        assert codes <= {8, 9, 10} and len(data) < len(plain)
    elif case == "inverted":
        assert codes <= {1, 10}
    elif case == "unrelated":
        assert codes == {1} and len(data) == len(plain)
    else:  # S is all zero: a CONSTANT subframe of bps + 1 bits
        assert codes <= {8, 9, 10}
        assert all(f["subframes"][0 if f["assign"] == 9 else 1]["type"] == "constant" for f in dec["frames"])


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n_ch", [1, 2, 3, 8])
def test_channels(n_ch, flags):
    kinds = ["music", "sine", "silence", "noise", "ramp", "alternating", "ar2", "quiet"]
    chans = np.array([signal(kinds[c], 4097, 16, seed=c) for c in range(n_ch)])
    data, dec = check_stream(chans, 16, 12345, flags)
    if n_ch != 2:  # TH_FLAC_STEREO changes nothing
        assert {f["assign"] for f in dec["frames"]} == {n_ch - 1}
        assert data == ta.flac_encode_i32(chans.astype(np.int32), ta.PCM_S16, 12345, flags=flags & 1)


@pytest.mark.parametrize("flags", [1, 3])
@pytest.mark.parametrize("n", [1, 4, 5, 9, 16, 33, 320, 4097, 8192 + 17])
def test_lengths(n, flags):
    """(320 = 64 x 5: the fixed predictors' partition order is 6, LPC 5's is 5 and LPC 8's 5)"""
    check_stream([signal("ar2", n, 24, seed=1), signal("music", n, 24, seed=n)], 24, 96000, flags)


def test_empty_stream():
    for flags in FLAGS:
        data, dec = check_stream(np.zeros((2, 0), np.int64), 16, 48000, flags)
        assert len(data) == 42 and dec["frames"] == []


def test_fixture_audio_size():
    """the fixture's audio with TH_FLAC_LPC: the model's size, below the fixed predictors' and below libFLAC's of the same samples"""
    meta = json.load(open(os.path.join(GOLDEN, "flac_libflac_head.json")))
    dec = F.decode(open(os.path.join(GOLDEN, "flac_libflac_head.flac"), "rb").read())
    x = np.array(dec["channels"], np.int64)
    data, got = check_stream(x, 16, 44100, 1)
    print("TH_FLAC_LPC frame bytes:", len(data) - 42, "fixed:", meta["model_frame_bytes"], "libFLAC:", meta["libflac_frame_bytes"])
    print(sorted(__import__("collections").Counter("%s%d" % (s["type"], s["order"]) for f in got["frames"] for s in f["subframes"]).items()))
    assert len(data) - 42 < meta["model_frame_bytes"]
    assert len(data) - 42 == 111086


def test_errors_and_bound():
    x = np.zeros((2, 16), np.int32)
    for bad in (4, 8, 0x80000000, 7):
        raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_encode_i32(x, ta.PCM_S16, 48000, flags=bad))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_encode_i32(x, ta.PCM_F32, 48000, flags=3))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_encode_i32(x, ta.PCM_S16, 0, flags=1))
    raises(_ffi.ERR_INVALID_ARG, lambda: ta.flac_encode_i32(x + 32768, ta.PCM_S16, 48000, flags=2))
    raises(_ffi.ERR_UNSUPPORTED, lambda: ta.flac_encode_i32(np.zeros((9, 16), np.int32), ta.PCM_S16, 48000, flags=3))
    raises(_ffi.ERR_UNSUPPORTED, lambda: ta.flac_encode_i32(x, ta.PCM_S16, 1048576, flags=3))
    n = C.c_size_t()
    assert lib.th_flac_encode_i32_ex(None, 1, 16, ta.PCM_S16, 48000, 3, None, 0, C.byref(n)) == _ffi.ERR_INVALID_ARG
    ptrs = (C.POINTER(C.c_int32) * 1)()
    assert lib.th_flac_encode_i32_ex(ptrs, 1, 16, ta.PCM_S16, 48000, 3, None, 0, C.byref(n)) == _ffi.ERR_INVALID_ARG
    assert lib.th_flac_encode_i32_ex(ptrs, 1, 0, ta.PCM_S16, 48000, 3, None, 0, None) == _ffi.ERR_INVALID_ARG
    # a short buffer reports th_flac_bound, whatever the flags
    y = np.ascontiguousarray(np.array([signal("sine", 5000, 16), signal("music", 5000, 16)], np.int32))
    ptrs = (C.POINTER(C.c_int32) * 2)(*[y[c].ctypes.data_as(C.POINTER(C.c_int32)) for c in range(2)])
    want = F.bound(5000, 2, 16)
    buf = np.zeros(want, np.uint8)
    for flags in FLAGS:
        assert lib.th_flac_encode_i32_ex(ptrs, 2, 5000, ta.PCM_S16, 48000, flags, buf.ctypes.data, want - 1, C.byref(n)) == _ffi.ERR_BUFFER_TOO_SMALL
        assert n.value == want and not buf.any()
    assert lib.th_flac_encode_i32_ex(ptrs, 2, 5000, ta.PCM_S16, 48000, 3, buf.ctypes.data, want, C.byref(n)) == _ffi.OK
    assert 42 < n.value < want and bytes(buf[:4]) == b"fLaC"
