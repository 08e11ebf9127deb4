"""Thin Python face of the C ABI (include/thesia_amd.h) used by tests and bench.py.

The host logic lives in C++ behind the C ABI (thesia_amd/csrc); this file only marshals numpy
arrays / device pointers.  Names follow the reference: SpecSetting, SpectrogramAnalyzer plan,
TrackManager, encode_*_tile (src-tauri/src/core/{spectrogram,mod,render_tiles}.rs).
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Sequence

import struct
import threading

import numpy as np

from . import _ffi
from ._ffi import (ChanDesc, ImgDesc, RasterDesc, ThError, TileGeom, WaveDesc, c_f32p, c_szp, c_u8p, c_u16p, check,
                   lib, vp)

LINEAR, MEL = 0, 1
NORM_OFF, NORM_LUFS, NORM_RMS_DB, NORM_PEAK_DB = 0, 1, 2, 3
GUARD_CLIP, GUARD_REDUCE_GLOBAL_LEVEL, GUARD_LIMITER = 0, 1, 2
GUARD_RESULT_GLOBAL_GAIN, GUARD_RESULT_BEFORE_CLIP, GUARD_RESULT_GAIN_SEQUENCE = 0, 1, 2
SPECTRUM_MEAN_AMP, SPECTRUM_MEAN_POWER, SPECTRUM_MAX = 0, 1, 2
PCM_S16, PCM_S24, PCM_F32 = 0, 1, 2
DITHER_NONE, DITHER_TPDF = 0, 1
WAV_HEADER_MAX = 64
EXPORT_PIECE_BYTES = 32 << 20      # TH_EXPORT_PIECE_BYTES
EXPORT_MAX_CHANNELS = 1024         # TH_EXPORT_MAX_CHANNELS
EXPORT_CHUNK_SAMPLES = 4096        # samples (frames x channels) of one workgroup of the export kernel, at most
RESAMPLE_MAX_TAPS = 16384          # TH_RESAMPLE_MAX_TAPS
RESAMPLE_MAX_COEFS = 1 << 24       # TH_RESAMPLE_MAX_COEFS
BAND_PASS, BAND_STOP = 0, 1        # TH_BAND_*
BAND_MAX_TAPS = 65536              # TH_BAND_MAX_TAPS
BAND_DEFAULT_HALF_TAPS = 2048      # TH_BAND_DEFAULT_HALF_TAPS
BAND_TILE, BAND_TAP_BLOCK = 2048, 64   # outputs of a workgroup and taps per step of the band kernel (reader_plan.h)
FIGURE_RGBA, FIGURE_GREY16 = 0, 1
FIGURE_MAX_DIM = 16384             # TH_FIGURE_MAX_DIM
FIGURE_PIECE_BYTES = 8 << 20       # TH_FIGURE_PIECE_BYTES
FIGURE_TMP_BYTES = 16 << 20        # TH_FIGURE_TMP_BYTES
ENVELOPE_MAX_COLS = 65536          # TH_ENVELOPE_MAX_COLS
ENVELOPE_PIECE_BYTES = 4 << 20     # TH_ENVELOPE_PIECE_BYTES
ENVELOPE_PART_BYTES = 32 << 20     # TH_ENVELOPE_PART_BYTES
ENVELOPE_CHUNK = 4096              # samples of one chunk of the envelope kernels' absolute grid (ENV_CHUNK, envelope_plan.h)
ENVELOPE_DENSE_MIN = 64            # samples per column, on average, from which a request goes through the chunk reduction
WAVEFORM_TILE_MAX_BYTES = 24 + 1024 * 12
SPECTROGRAM_TILE_MAX_BYTES = 40 + 520 * 520 * 4


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a: np.ndarray, t):
    return a.ctypes.data_as(t)


# ------------------------------------------------------------------ host-only helpers
def device_count() -> int:
    n = C.c_int(0)
    check(lib.th_device_count(C.byref(n)))
    return n.value


def calc_framing_params(win_ms: float, t_overlap: int, f_overlap: int, sr: int):
    """SpecSetting::calc_framing_params (spectrogram.rs:56-98) -> (hop, win, n_fft)."""
    h, w, n = C.c_size_t(), C.c_size_t(), C.c_size_t()
    check(lib.th_calc_framing_params(win_ms, t_overlap, f_overlap, sr, C.byref(h), C.byref(w), C.byref(n)))
    return h.value, w.value, n.value


def stft_n_frames(n_samples: int, win: int, hop: int) -> int:
    t = C.c_size_t()
    check(lib.th_stft_n_frames(n_samples, win, hop, C.byref(t)))
    return t.value


def calc_normalized_win(win: int, n_fft: int) -> np.ndarray:
    out = np.empty(win, np.float32)
    check(lib.th_calc_normalized_win(win, n_fft, _ptr(out, c_f32p)))
    return out


def calc_mel_fb(sr: int, n_fft: int, n_mel: int, fmin: float = 0.0, fmax: Optional[float] = None,
                do_norm: bool = True) -> np.ndarray:
    out = np.empty((n_fft // 2 + 1, n_mel), np.float32)
    check(lib.th_calc_mel_fb(sr, n_fft, n_mel, fmin, -1.0 if fmax is None else fmax, int(do_norm),
                             _ptr(out, c_f32p)))
    return out


def mel_default_n_mel(sr: int, n_fft: int) -> int:
    n = C.c_size_t()
    check(lib.th_mel_default_n_mel(sr, n_fft, C.byref(n)))
    return n.value


def hz_range_to_idx(freq_scale: int, hz_range, sr: int, n: int):
    a, b = C.c_size_t(), C.c_size_t()
    check(lib.th_hz_range_to_idx(freq_scale, hz_range[0], hz_range[1], sr, n, C.byref(a), C.byref(b)))
    return a.value, b.value


def global_db_range(mins, maxs, dB_range: float = 100.0):
    mins, maxs = _f32(mins).ravel(), _f32(maxs).ravel()
    lo, hi = C.c_float(), C.c_float()
    check(lib.th_global_db_range(_ptr(mins, c_f32p), _ptr(maxs, c_f32p), mins.size, dB_range, C.byref(lo),
                                 C.byref(hi)))
    return lo.value, hi.value


def pitch_f32(row_elems: int) -> int:
    """Recommended floats per row for device-resident specs (rows padded to 128 B)."""
    return lib.th_pitch_f32(row_elems)


def pitch_u16(row_elems: int) -> int:
    """Recommended u16 per row for device-resident images (rows padded to 128 B)."""
    return lib.th_pitch_u16(row_elems)


def pyramid_bins(n_samples: int, level: int) -> int:
    return lib.th_waveform_pyramid_bins(n_samples, level)


def pyramid_offset(n_samples: int, level: int) -> int:
    """float offset of level `level` in a channel's pyramid buffer (= total floats for level = n_levels)"""
    return lib.th_waveform_pyramid_offset(n_samples, level)


def ab_variants() -> bool:
    """True when the loaded library was built with -DTH_AB_VARIANTS=1 (the measured-and-dropped kernel variants behind
    th_plan_set_kernel: include/thesia_amd_testing.h); the product build answers False and refuses those selectors."""
    return bool(lib.th_build_ab_variants())


def shard_assign(weights, world: int):
    """th_shard_assign: owner rank of every (track, channel) unit, by frame-count weight."""
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    owner = np.empty(w.size, np.uint32)
    check(lib.th_shard_assign(w.ctypes.data_as(C.POINTER(C.c_uint64)), w.size, world,
                              owner.ctypes.data_as(C.POINTER(C.c_uint32))))
    return owner


def spectrogram_tile_geometry(img_width: int, img_height: int, level_x: int, level_y: int, tile_x: int,
                              tile_y: int) -> TileGeom:
    g = TileGeom()
    check(lib.th_spectrogram_tile_geometry(img_width, img_height, level_x, level_y, tile_x, tile_y, C.byref(g)))
    return g


def waveform_tile_geometry(n_samples: int, level: int, tile_index: int):
    s, b, p = C.c_size_t(), C.c_size_t(), C.c_size_t()
    check(lib.th_waveform_tile_geometry(n_samples, level, tile_index, C.byref(s), C.byref(b), C.byref(p)))
    return s.value, b.value, p.value


# ------------------------------------------------------------------ device context
def _audio_stats_dict(o) -> dict:
    return {"global_lufs": o.global_lufs, "rms_dB": o.rms_dB, "max_peak": o.max_peak, "max_peak_dB": o.max_peak_dB}


def normalize_gain(kind: int, target: float, stats: dict) -> float:
    """the normalise gain of NormalizeTarget (kind, target) from the AudioStats of the original (normalize.rs:23-45), as f32"""
    o = _ffi.AudioStats(stats["global_lufs"], stats["rms_dB"], stats["max_peak"], stats["max_peak_dB"])
    g = C.c_float()
    check(lib.th_normalize_gain(kind, target, C.byref(o), C.byref(g)))
    return np.float32(g.value)


def limiter_params(sr: int) -> dict:
    """what PerfectLimiter::with_default(sr) runs with: attack, hold_length, release_samples, box_len[3]"""
    o = _ffi.LimiterDesc()
    check(lib.th_limiter_params(sr, C.byref(o)))
    return {"attack": o.attack, "hold_length": o.hold_length, "release_samples": o.release_samples, "box_len": list(o.box_len)}


def spectrum_frame_range(sr: int, hop: int, n_frames: int, start_sec: float = 0.0, end_sec: float = float("inf")):
    """-> (frame_start, frame_end): the frames of n_frames whose centre t * hop lies in [start_sec, end_sec) (host arithmetic)"""
    f0, f1 = C.c_size_t(), C.c_size_t()
    check(lib.th_spectrum_frame_range(sr, hop, n_frames, start_sec, end_sec, C.byref(f0), C.byref(f1)))
    return f0.value, f1.value


def _spectrum_info_dict(o) -> dict:
    return {k: int(getattr(o, k)) for k, _ in o._fields_}


class _SpectrumMethods:
    """the spectrum of a time range of resident specs (th_tm_* and th_tmg_*: _PFX)"""

    def spectra(self, requests):
        """th_tm_get_spectra: requests = iterable of (track_id, ch, kind[, start_sec[, end_sec]]) -> list of (f32 row, info dict),
        in request order.  kind: SPECTRUM_MEAN_AMP / SPECTRUM_MEAN_POWER / SPECTRUM_MAX; the range defaults to the whole track."""
        reqs = [tuple(r) + (0.0, float("inf"))[len(r) - 3:] for r in requests]
        n = len(reqs)
        if n == 0:
            return []
        arr = (_ffi.SpectrumRequest * n)(*[_ffi.SpectrumRequest(*r) for r in reqs])
        info = (_ffi.SpectrumInfo * n)()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "get_spectra")
        rc = fn(self.handle, arr, n, None, 0, info, C.byref(need))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = np.empty(need.value, np.float32)
        check(fn(self.handle, arr, n, _ptr(out, c_f32p), out.size, info, C.byref(need)))
        return [(out[o.offset: o.offset + o.height], _spectrum_info_dict(o)) for o in info]

    def spectrum(self, track_id: int, ch: int, kind: int, start_sec: float = 0.0, end_sec: float = float("inf")):
        """th_tm_get_spectrum: the spectrum of one channel over [start_sec, end_sec) -> (f32 row of the spec's height, info dict)"""
        info = _ffi.SpectrumInfo()
        fn = getattr(lib, self._PFX + "get_spectrum")
        rc = fn(self.handle, track_id, ch, kind, start_sec, end_sec, None, 0, C.byref(info))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = np.empty(info.height, np.float32)
        check(fn(self.handle, track_id, ch, kind, start_sec, end_sec, _ptr(out, c_f32p), out.size, C.byref(info)))
        return out, _spectrum_info_dict(info)


def _meter_dict(o, series) -> dict:
    d = {k: getattr(o, k) for k, _ in o._fields_}
    for k in ("true_peak", "true_peak_dB"):
        d[k] = np.float32(d[k])
    if series is not None:
        d["momentary"] = series[o.momentary_offset: o.momentary_offset + o.n_momentary]
        d["short_term"] = series[o.short_term_offset: o.short_term_offset + o.n_short_term]
    return d


class _LoudnessMeterMethods:
    """true peak, loudness range and the momentary / short-term curves of resident tracks (th_tm_* and th_tmg_*: _PFX)"""

    def loudness_meters(self, track_ids, series: bool = True):
        """th_tm_get_loudness_meters: -> one dict per id, in request order: the th_loudness_meter fields and, with series, the
        f64 LUFS arrays "momentary" and "short_term" """
        ids = [int(i) for i in track_ids]
        n = len(ids)
        if n == 0:
            return []
        arr = (C.c_size_t * n)(*ids)
        ms = (_ffi.LoudnessMeter * n)()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "get_loudness_meters")
        if not series:
            check(fn(self.handle, arr, n, ms, None, 0, C.byref(need)))
            return [_meter_dict(m, None) for m in ms]
        one = np.empty(1, np.float64)
        rc = fn(self.handle, arr, n, ms, one.ctypes.data_as(C.POINTER(C.c_double)), 0, C.byref(need))  # (the size alone)
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = np.empty(max(need.value, 1), np.float64)
        check(fn(self.handle, arr, n, ms, out.ctypes.data_as(C.POINTER(C.c_double)), need.value, C.byref(need)))
        return [_meter_dict(m, out) for m in ms]

    def loudness_meter(self, track_id: int, series: bool = True) -> dict:
        """th_tm_get_loudness_meter: one track"""
        return self.loudness_meters([track_id], series)[0]


def export_chunk_frames(n_channels: int) -> int:
    """frames of one chunk of the export kernel (chunks lie on the track's absolute frame grid): kernels.h export_chunk_frames"""
    return max((EXPORT_CHUNK_SAMPLES // n_channels) & ~3, 4)


def audio_sample_range(sr: int, n_samples: int, start_sec: float = 0.0, end_sec: float = float("inf")):
    """-> (sample_start, sample_end): the samples of n_samples at or after start_sec and before end_sec (host arithmetic)"""
    s0, s1 = C.c_size_t(), C.c_size_t()
    check(lib.th_audio_sample_range(sr, n_samples, start_sec, end_sec, C.byref(s0), C.byref(s1)))
    return s0.value, s1.value


def export_dither(seed: int, ch: int, i: int):
    """-> (a, b): the two 24-bit uniform integers of the export's TPDF dither for absolute sample index i of channel ch (host)"""
    a, b = C.c_uint32(), C.c_uint32()
    check(lib.th_export_dither(seed, ch, i, C.byref(a), C.byref(b)))
    return a.value, b.value


def export_quantize(fmt: int, dither: int, seed: int, ch: int, first_index: int, x):
    """one channel through the export's quantiser on the host -> (int32 q, n_clamped, n_nan); PCM_F32: q holds the bit patterns"""
    x = _f32(x).ravel()
    q = np.empty(x.size, np.int32)
    nc, nn = C.c_uint64(), C.c_uint64()
    check(lib.th_export_quantize(fmt, dither, seed, ch, first_index, _ptr(x, c_f32p), x.size, q.ctypes.data_as(C.POINTER(C.c_int32)),
                                 C.byref(nc), C.byref(nn)))
    return q, nc.value, nn.value


def wav_header(fmt: int, sr: int, n_channels: int, n_frames: int):
    """-> (header bytes, pad_len): the RIFF / WAV header of n_frames frames and the zero bytes (0 or 1) that follow the data"""
    out = (C.c_uint8 * WAV_HEADER_MAX)()
    hl, pl = C.c_size_t(), C.c_size_t()
    check(lib.th_wav_header(fmt, sr, n_channels, n_frames, out, C.byref(hl), C.byref(pl)))
    return bytes(out[:hl.value]), pl.value


def _export_info_dict(o) -> dict:
    return {k: int(getattr(o, k)) for k, _ in o._fields_}


def _export_request(r) -> "_ffi.ExportRequest":
    """(track_id, fmt[, dither[, seed[, start_sec[, end_sec[, which]]]]]) or a dict with those names"""
    if isinstance(r, dict):
        r = (r["track_id"], r["fmt"], r.get("dither", DITHER_NONE), r.get("seed", 0), r.get("start_sec", 0.0),
             r.get("end_sec", float("inf")), r.get("which", 0))
    r = tuple(r) + (DITHER_NONE, 0, 0.0, float("inf"), 0)[len(r) - 2:]
    track_id, fmt, dither, seed, start_sec, end_sec, which = r
    return _ffi.ExportRequest(track_id, which, fmt, dither, seed, start_sec, end_sec)


class _ExportMethods:
    """a time range of resident audio as interleaved PCM / float bytes or a WAV file image (th_tm_* and th_tmg_*: _PFX)"""

    def export_pcm(self, requests, out: Optional[np.ndarray] = None):
        """th_tm_export_pcm: requests = iterable of (track_id, fmt[, dither[, seed[, start_sec[, end_sec[, which]]]]]) ->
        (uint8 buffer, list of info dicts); request i's bytes are buffer[offset: offset + n_bytes].  out: a uint8 array to fill
        (pinned memory, say) instead of a new one."""
        reqs = [_export_request(r) for r in requests]
        n = len(reqs)
        if n == 0:
            return np.empty(0, np.uint8), []
        arr = (_ffi.ExportRequest * n)(*reqs)
        info = (_ffi.ExportInfo * n)()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "export_pcm")
        if out is None:
            rc = fn(self.handle, arr, n, None, 0, info, C.byref(need))
            if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
                check(rc)
            out = np.empty(max(need.value, 1), np.uint8)
        check(fn(self.handle, arr, n, out.ctypes.data, out.size, info, C.byref(need)))
        return out[:need.value], [_export_info_dict(o) for o in info]

    def export_wav(self, track_id: int, fmt: int, dither: int = DITHER_NONE, seed: int = 0, start_sec: float = 0.0,
                   end_sec: float = float("inf"), which: int = 0):
        """th_tm_export_wav: -> (the complete file image as bytes, info dict)"""
        req = _ffi.ExportRequest(track_id, which, fmt, dither, seed, start_sec, end_sec)
        info = _ffi.ExportInfo()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "export_wav")
        rc = fn(self.handle, C.byref(req), None, 0, C.byref(info), C.byref(need))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = np.empty(need.value, np.uint8)
        check(fn(self.handle, C.byref(req), out.ctypes.data, out.size, C.byref(info), C.byref(need)))
        return out.tobytes(), _export_info_dict(info)


    def export_flac(self, requests, out: Optional[np.ndarray] = None, flags: Optional[int] = None):
        """th_tm_export_flac: requests as export_pcm (fmt PCM_S16 or PCM_S24) -> (uint8 buffer, list of info dicts); request i's
        complete FLAC file image is buffer[offset: offset + n_bytes], lossless for the bytes export_pcm returns for the same request.
        flags (FLAC_LPC | FLAC_STEREO, or 0): th_tm_export_flac_ex, the smaller files of LPC subframes and stereo decorrelation"""
        reqs = [_export_request(r) for r in requests]
        n = len(reqs)
        if n == 0:
            return np.empty(0, np.uint8), []
        arr = (_ffi.ExportRequest * n)(*reqs)
        info = (_ffi.ExportInfo * n)()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "export_flac")
        if flags is not None:
            ex = getattr(lib, self._PFX + "export_flac_ex")
            fn = lambda h, a, m, o, cap, inf, ln: ex(h, a, m, flags, o, cap, inf, ln)  # noqa: E731
        if out is None:
            rc = fn(self.handle, arr, n, None, 0, info, C.byref(need))
            if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
                check(rc)
            out = np.empty(max(need.value, 1), np.uint8)
        check(fn(self.handle, arr, n, out.ctypes.data, out.size, info, C.byref(need)))
        return out[:need.value], [_export_info_dict(o) for o in info]


FLAC_BLOCK = 4096
FLAC_LPC, FLAC_STEREO, FLAC_LPC_MAX_ORDER = 1, 2, 8


def flac_bound(n_frames: int, n_channels: int, fmt: int) -> int:
    """th_flac_bound: the most bytes a FLAC file image of n_frames frames can take (host)"""
    b = C.c_uint64()
    check(lib.th_flac_bound(n_frames, n_channels, fmt, C.byref(b)))
    return b.value


def flac_frame_header(sr: int, n_channels: int, fmt: int, frame_number: int, block_len: int) -> bytes:
    """th_flac_frame_header: sync .. CRC-8 of one frame of the export's FLAC stream (host)"""
    out = (C.c_uint8 * 16)()
    ln = C.c_size_t()
    check(lib.th_flac_frame_header(sr, n_channels, fmt, frame_number, block_len, out, C.byref(ln)))
    return bytes(out[:ln.value])


def flac_encode_i32(channels, fmt: int, sr: int, flags: Optional[int] = None) -> bytes:
    """th_flac_encode_i32: planar int32 channels (n_ch, n) -> the FLAC file image th_tm_export_flac makes of those integers (host);
    with flags (FLAC_LPC | FLAC_STEREO, or 0) th_flac_encode_i32_ex, the image of th_tm_export_flac_ex"""
    x = np.ascontiguousarray(channels, dtype=np.int32)
    if x.ndim == 1:
        x = x[None, :]
    n_ch, n = x.shape
    ptrs = (C.POINTER(C.c_int32) * max(n_ch, 1))(*[x[c].ctypes.data_as(C.POINTER(C.c_int32)) for c in range(n_ch)])
    need = C.c_size_t()
    fn = lib.th_flac_encode_i32
    if flags is not None:
        fn = lambda p, c, m, f, r, o, cap, ln: lib.th_flac_encode_i32_ex(p, c, m, f, r, flags, o, cap, ln)  # noqa: E731
    rc = fn(ptrs, n_ch, n, fmt, sr, None, 0, C.byref(need))
    if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
        check(rc)
    out = np.empty(max(need.value, 1), np.uint8)
    check(fn(ptrs, n_ch, n, fmt, sr, out.ctypes.data, out.size, C.byref(need)))
    return out[:need.value].tobytes()


def resample_plan(sr_in: int, sr_out: int) -> dict:
    """th_resample_plan_for -> {L, M, half_taps, rho, cutoff} of the polyphase resampler sr_in -> sr_out (host)"""
    p = _ffi.ResamplePlan()
    check(lib.th_resample_plan_for(sr_in, sr_out, C.byref(p)))
    return {"L": p.L, "M": p.M, "half_taps": p.half_taps, "rho": p.rho, "cutoff": p.cutoff}


def resample_n_out(n_in: int, sr_in: int, sr_out: int) -> int:
    """samples of a track of n_in samples at sr_in once it is resampled to sr_out: ceil(n_in L / M) (host)"""
    n = C.c_size_t()
    check(lib.th_resample_n_out(n_in, sr_in, sr_out, C.byref(n)))
    return n.value


def resample_coefs(sr_in: int, sr_out: int, r: int):
    """-> (f64 row, f32 row): the 2K taps of phase r of the resampler's table (host)"""
    taps = 2 * resample_plan(sr_in, sr_out)["half_taps"]
    h64, c32 = np.empty(taps, np.float64), np.empty(taps, np.float32)
    check(lib.th_resample_coefs(sr_in, sr_out, r, h64.ctypes.data_as(C.POINTER(C.c_double)), _ptr(c32, c_f32p)))
    return h64, c32


def resample_f32(x, sr_in: int, sr_out: int, j0: int = 0, n: Optional[int] = None) -> np.ndarray:
    """outputs [j0, j0 + n) of one channel x (the whole channel) resampled sr_in -> sr_out on the host: what the kernel computes,
    the same table, order and bits (n None: up to the end)"""
    x = _f32(x).ravel()
    if n is None:
        n = resample_n_out(x.size, sr_in, sr_out) - j0
    y = np.empty(max(n, 0), np.float32)
    check(lib.th_resample_f32(_ptr(x, c_f32p), x.size, sr_in, sr_out, j0, y.size, _ptr(y, c_f32p)))
    return y


def resample_tile(sr_in: int, sr_out: int) -> dict:
    """the resample kernel's tiling of the pair (kernels.h resample_tiling): a workgroup takes R consecutive outputs of one channel
    in each of P periods, Lp outputs (Mp input samples) apart; a period of Lp outputs is S such sub-tiles"""
    p = resample_plan(sr_in, sr_out)
    L, M = p["L"], p["M"]
    if L < 64:
        Lp = L * (64 // L)
        R, S = Lp, 1
    else:
        Lp, S = L, (L + 63) // 64
        R = (L + S - 1) // S
    Mp = M * (Lp // L)
    lanes = ((R - 1) * M) // L + 1 + 64
    for G, Pt in ((4, 8), (4, 4), (4, 2), (4, 1), (1, 2), (1, 1)):
        span = (G * Pt - 1) * Mp + lanes
        if span <= 5248:
            break
    return {"L": L, "M": M, "taps": 2 * p["half_taps"], "Lp": Lp, "Mp": Mp, "R": R, "S": S, "G": G, "Pt": Pt, "P": G * Pt, "span": span}


def _export_at_request(r) -> "_ffi.ExportAtRequest":
    """(track_id, sr_out, fmt[, dither[, seed[, start_sec[, end_sec[, which]]]]]) or a dict with those names"""
    if isinstance(r, dict):
        sr_out = r.get("sr_out", 0)
        base = _export_request(r)
    else:
        r = tuple(r)
        sr_out = r[1]
        base = _export_request((r[0],) + r[2:])
    return _ffi.ExportAtRequest(base, sr_out)


class _ExportAtMethods:
    """_ExportMethods at a caller-chosen sample rate: the polyphase sinc resampler in front of the same export (th_tm_* and th_tmg_*)"""

    def export_pcm_at(self, requests, out: Optional[np.ndarray] = None):
        """th_tm_export_pcm_at: requests = iterable of (track_id, sr_out, fmt[, dither[, seed[, start_sec[, end_sec[, which]]]]]) ->
        (uint8 buffer, list of info dicts), as export_pcm; sr_out 0 = the track's own rate"""
        reqs = [_export_at_request(r) for r in requests]
        n = len(reqs)
        if n == 0:
            return np.empty(0, np.uint8), []
        arr = (_ffi.ExportAtRequest * n)(*reqs)
        info = (_ffi.ExportInfo * n)()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "export_pcm_at")
        if out is None:
            rc = fn(self.handle, arr, n, None, 0, info, C.byref(need))
            if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
                check(rc)
            out = np.empty(max(need.value, 1), np.uint8)
        check(fn(self.handle, arr, n, out.ctypes.data, out.size, info, C.byref(need)))
        return out[:need.value], [_export_info_dict(o) for o in info]

    def export_wav_at(self, track_id: int, sr_out: int, fmt: int, dither: int = DITHER_NONE, seed: int = 0, start_sec: float = 0.0,
                      end_sec: float = float("inf"), which: int = 0):
        """th_tm_export_wav_at: -> (the complete file image at sr_out as bytes, info dict)"""
        req = _ffi.ExportAtRequest(_ffi.ExportRequest(track_id, which, fmt, dither, seed, start_sec, end_sec), sr_out)
        info = _ffi.ExportInfo()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "export_wav_at")
        rc = fn(self.handle, C.byref(req), None, 0, C.byref(info), C.byref(need))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = np.empty(need.value, np.uint8)
        check(fn(self.handle, C.byref(req), out.ctypes.data, out.size, C.byref(info), C.byref(need)))
        return out.tobytes(), _export_info_dict(info)


def _band_plan(plan) -> "_ffi.BandPlan":
    if isinstance(plan, _ffi.BandPlan):
        return plan
    return _ffi.BandPlan(plan["half_taps"], plan["mode"], plan["f_lo_hz"], plan["f_hi_hz"], plan["trans_hz"])


def band_plan(sr: int, mode: int, f_lo_hz: float, f_hi_hz: float, trans_hz: float = 0.0) -> dict:
    """th_band_plan_for -> {half_taps, mode, f_lo_hz, f_hi_hz, trans_hz} of the band filter at sr (host); half_taps 0: the identity"""
    p = _ffi.BandPlan()
    check(lib.th_band_plan_for(sr, mode, f_lo_hz, f_hi_hz, trans_hz, C.byref(p)))
    return {k: getattr(p, k) for k, _ in p._fields_}


def band_coefs(sr: int, plan):
    """-> (f64 row, f32 row): the 2K taps of the filter of a band_plan (host)"""
    p = _band_plan(plan)
    h64, c32 = np.empty(2 * p.half_taps, np.float64), np.empty(2 * p.half_taps, np.float32)
    check(lib.th_band_coefs(sr, C.byref(p), h64.ctypes.data_as(C.POINTER(C.c_double)), _ptr(c32, c_f32p)))
    return h64, c32


def band_response(sr: int, plan, hz) -> np.ndarray:
    """the magnitude of the filter's f32 row at the frequencies hz, in dB (host, summed in f64)"""
    p = _band_plan(plan)
    hz = np.ascontiguousarray(hz, np.float64).ravel()
    db = np.empty(hz.size, np.float64)
    f64p = C.POINTER(C.c_double)
    check(lib.th_band_response(sr, C.byref(p), hz.ctypes.data_as(f64p), hz.size, db.ctypes.data_as(f64p)))
    return db


def band_f32(x, c32, j0: int = 0, n: Optional[int] = None) -> np.ndarray:
    """outputs [j0, j0 + n) of one channel x (the whole channel) under the row c32 on the host: what the band kernel computes, the
    same order and bits (n None: up to the end)"""
    x, c32 = _f32(x).ravel(), _f32(c32).ravel()
    if n is None:
        n = x.size - j0
    y = np.empty(max(n, 0), np.float32)
    check(lib.th_band_f32(_ptr(x, c_f32p), x.size, _ptr(c32, c_f32p), c32.size // 2, j0, y.size, _ptr(y, c_f32p)))
    return y


def _export_band_request(r) -> "_ffi.ExportBandRequest":
    """(track_id, mode, f_lo_hz, f_hi_hz, trans_hz, fmt[, dither[, seed[, start_sec[, end_sec[, which]]]]]) or a dict with those names"""
    if isinstance(r, dict):
        band = (r.get("mode", BAND_PASS), r["f_lo_hz"], r["f_hi_hz"], r.get("trans_hz", 0.0))
        base = _export_request(r)
    else:
        r = tuple(r)
        band = r[1:5]
        base = _export_request((r[0],) + r[5:])
    return _ffi.ExportBandRequest(base, *band)


class _ExportBandMethods:
    """_ExportMethods through a band filter: what a box on the spectrogram holds, or everything but it (th_tm_* and th_tmg_*)"""

    def export_pcm_band(self, requests, out: Optional[np.ndarray] = None):
        """th_tm_export_pcm_band: requests = iterable of (track_id, mode, f_lo_hz, f_hi_hz, trans_hz, fmt[, dither[, seed[, start_sec[,
        end_sec[, which]]]]]) -> (uint8 buffer, list of info dicts), as export_pcm"""
        reqs = [_export_band_request(r) for r in requests]
        n = len(reqs)
        if n == 0:
            return np.empty(0, np.uint8), []
        arr = (_ffi.ExportBandRequest * n)(*reqs)
        info = (_ffi.ExportInfo * n)()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "export_pcm_band")
        if out is None:
            rc = fn(self.handle, arr, n, None, 0, info, C.byref(need))
            if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
                check(rc)
            out = np.empty(max(need.value, 1), np.uint8)
        check(fn(self.handle, arr, n, out.ctypes.data, out.size, info, C.byref(need)))
        return out[:need.value], [_export_info_dict(o) for o in info]

    def export_wav_band(self, track_id: int, mode: int, f_lo_hz: float, f_hi_hz: float, trans_hz: float, fmt: int,
                        dither: int = DITHER_NONE, seed: int = 0, start_sec: float = 0.0, end_sec: float = float("inf"), which: int = 0):
        """th_tm_export_wav_band: -> (the complete file image of the filtered audio as bytes, info dict)"""
        req = _ffi.ExportBandRequest(_ffi.ExportRequest(track_id, which, fmt, dither, seed, start_sec, end_sec), mode, f_lo_hz, f_hi_hz,
                                     trans_hz)
        info = _ffi.ExportInfo()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "export_wav_band")
        rc = fn(self.handle, C.byref(req), None, 0, C.byref(info), C.byref(need))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = np.empty(need.value, np.uint8)
        check(fn(self.handle, C.byref(req), out.ctypes.data, out.size, C.byref(info), C.byref(need)))
        return out.tobytes(), _export_info_dict(info)


def figure_axis(origin: float, extent: float, n_out: int, n_in: int):
    """th_figure_axis -> (start int32[n_out], count int32[n_out], weights f64[n_out, max_taps]): the normalised Lanczos3 taps of one
    axis of a figure, n_out pixels over [origin, origin + extent) of n_in source pixels (host)"""
    start, count = np.empty(n_out, np.int32), np.empty(n_out, np.int32)
    mt = C.c_uint32()
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rc = lib.th_figure_axis(origin, extent, n_out, n_in, _ptr(start, i32p), _ptr(count, i32p), None, 0, C.byref(mt))
    if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
        check(rc)
    w = np.empty((n_out, mt.value), np.float64)
    check(lib.th_figure_axis(origin, extent, n_out, n_in, _ptr(start, i32p), _ptr(count, i32p), _ptr(w, f64p), w.size, C.byref(mt)))
    return start, count, w


def figure_box(start_sec: float, end_sec: float, hz_min: float, hz_max: float, sr: int, n_samples: int, img_width: int,
               spec_height: int, img_height: int, freq_scale: int):
    """th_figure_box -> (left, top, width, height) in image pixels of a time / frequency range (host)"""
    b = [C.c_double() for _ in range(4)]
    check(lib.th_figure_box(start_sec, end_sec, hz_min, hz_max, sr, n_samples, img_width, spec_height, img_height, freq_scale,
                            *[C.byref(v) for v in b]))
    return tuple(v.value for v in b)


def _figure_request(r) -> "_ffi.FigureRequest":
    """(track_id, ch, kind, out_w, out_h, (left, top, width, height)) or a dict with those names (the box under "box")"""
    if isinstance(r, dict):
        r = (r["track_id"], r["ch"], r.get("kind", FIGURE_RGBA), r["out_w"], r["out_h"], r["box"])
    track_id, ch, kind, out_w, out_h, box = r
    return _ffi.FigureRequest(track_id, ch, kind, out_w, out_h, *[float(v) for v in box])


class _FigureMethods:
    """any region of a resident spectrogram image at any pixel size, coloured or 16-bit grey (th_tm_* and th_tmg_*: _PFX)"""

    def figure_box(self, track_id: int, ch: int, start_sec: float = 0.0, end_sec: float = float("inf"), hz_min: float = 0.0,
                   hz_max: float = float("inf")):
        """th_tm_figure_box -> (left, top, width, height) of the range in the channel's resident image"""
        b = [C.c_double() for _ in range(4)]
        check(getattr(lib, self._PFX + "figure_box")(self.handle, track_id, ch, start_sec, end_sec, hz_min, hz_max,
                                                     *[C.byref(v) for v in b]))
        return tuple(v.value for v in b)

    def render_figures(self, requests, out=None, cap: Optional[int] = None):
        """th_tm_render_figures: requests = iterable of (track_id, ch, kind, out_w, out_h, (left, top, width, height)) ->
        (list of arrays, list of info dicts); array i is uint8 [out_h, out_w, 4] (FIGURE_RGBA) or uint16 [out_h, out_w]
        (FIGURE_GREY16), the top row the highest frequency.  out: a uint8 array to fill instead of a new one, or the address of
        cap bytes (pinned memory of th_host_alloc, say); the arrays are then views into it."""
        reqs = [_figure_request(r) for r in requests]
        n = len(reqs)
        if n == 0:
            return [], []
        arr = (_ffi.FigureRequest * n)(*reqs)
        info = (_ffi.FigureInfo * n)()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "render_figures")
        if out is None:
            rc = fn(self.handle, arr, n, None, 0, info, C.byref(need))
            if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
                check(rc)
            out = np.empty(max(need.value, 1), np.uint8)
        if isinstance(out, np.ndarray):
            addr, cap, buf = out.ctypes.data, out.size, out
        else:
            addr = out.value if isinstance(out, C.c_void_p) else int(out)
            buf = None
        check(fn(self.handle, arr, n, addr, cap, info, C.byref(need)))
        if buf is None:
            buf = np.frombuffer((C.c_uint8 * need.value).from_address(addr), np.uint8)
        figs = []
        for r, o in zip(reqs, info):
            raw = buf[o.offset: o.offset + o.bytes]
            figs.append(raw.view(np.uint16).reshape(o.out_h, o.out_w) if r.kind == FIGURE_GREY16 else raw.reshape(o.out_h, o.out_w, 4))
        return figs, [_export_info_dict(o) for o in info]

    def render_figure(self, track_id: int, ch: int, kind: int, out_w: int, out_h: int, box):
        """th_tm_render_figure -> (array, info dict) of one figure"""
        req = _figure_request((track_id, ch, kind, out_w, out_h, box))
        info = _ffi.FigureInfo()
        fn = getattr(lib, self._PFX + "render_figure")
        rc = fn(self.handle, C.byref(req), None, 0, C.byref(info))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = np.empty(max(info.bytes, 1), np.uint8)
        check(fn(self.handle, C.byref(req), out.ctypes.data, out.size, C.byref(info)))
        raw = out[:info.bytes]
        fig = raw.view(np.uint16).reshape(out_h, out_w) if kind == FIGURE_GREY16 else raw.reshape(out_h, out_w, 4)
        return fig, _export_info_dict(info)


def envelope_edges(sr: int, n_samples: int, start_sec: float = 0.0, end_sec: float = float("inf"), n_cols: int = 1) -> np.ndarray:
    """th_envelope_edges -> uint64[n_cols + 1]: column j of the envelope of a time range owns samples [edges[j], edges[j + 1]) (host)"""
    e = np.empty(max(int(n_cols), 0) + 1, np.uint64)
    check(lib.th_envelope_edges(sr, n_samples, start_sec, end_sec, n_cols, _ptr(e, C.POINTER(C.c_uint64))))
    return e


edges = envelope_edges


def waveform_figure_span(col, left, out_h: int, amp_lo: float, amp_hi: float, thickness: int):
    """th_waveform_figure_span -> (y_top, y_bot) in 1/256 pixel of one column of a waveform lane, or None where it draws nothing; col and
    left: (min, max, mean, rms) of the column and of its left neighbour (None for column 0) (host)"""
    c = _f32(col)
    lf = None if left is None else _f32(left)
    yt, yb, dr = C.c_int32(), C.c_int32(), C.c_int()
    check(lib.th_waveform_figure_span(_ptr(c, c_f32p), None if lf is None else _ptr(lf, c_f32p), out_h, amp_lo, amp_hi, thickness,
                                      C.byref(yt), C.byref(yb), C.byref(dr)))
    return (yt.value, yb.value) if dr.value else None


def _envelope_request(r) -> "_ffi.EnvelopeRequest":
    """(track_id, ch, which, start_sec, end_sec, n_cols) or a dict with those names"""
    if isinstance(r, dict):
        r = (r["track_id"], r["ch"], r.get("which", 1), r.get("start_sec", 0.0), r.get("end_sec", float("inf")), r["n_cols"])
    track_id, ch, which, start_sec, end_sec, n_cols = r
    return _ffi.EnvelopeRequest(track_id, ch, which, start_sec, end_sec, n_cols, 0)


def _waveform_figure_request(r) -> "_ffi.WaveformFigureRequest":
    """(track_id, ch, which, start_sec, end_sec, out_w, out_h, amp_lo, amp_hi, thickness, fill, background) or a dict with those names"""
    if isinstance(r, dict):
        r = (r["track_id"], r["ch"], r.get("which", 1), r.get("start_sec", 0.0), r.get("end_sec", float("inf")), r["out_w"], r["out_h"],
             r.get("amp_lo", -1.0), r.get("amp_hi", 1.0), r.get("thickness", 256), r.get("fill", (255, 255, 255, 255)),
             r.get("background", (0, 0, 0, 0)))
    track_id, ch, which, start_sec, end_sec, out_w, out_h, amp_lo, amp_hi, thickness, fill, background = r
    return _ffi.WaveformFigureRequest(_ffi.EnvelopeRequest(track_id, ch, which, start_sec, end_sec, out_w, 0), out_h, amp_lo, amp_hi,
                                      thickness, (C.c_uint8 * 4)(*fill), (C.c_uint8 * 4)(*background))


class _EnvelopeMethods:
    """the exact (min, max, mean, rms) envelope of a time range at any pixel width, and its raster as a waveform lane (th_tm_* and
    th_tmg_*: _PFX)"""

    def get_envelopes(self, requests, out: Optional[np.ndarray] = None):
        """th_tm_get_envelopes: requests = iterable of (track_id, ch, which, start_sec, end_sec, n_cols) -> (list of float32
        [n_cols, 4] arrays (min, max, mean, rms), list of info dicts).  out: a float32 array to fill instead of a new one; the arrays
        are then views into it."""
        reqs = [_envelope_request(r) for r in requests]
        n = len(reqs)
        if n == 0:
            return [], []
        arr = (_ffi.EnvelopeRequest * n)(*reqs)
        info = (_ffi.EnvelopeInfo * n)()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "get_envelopes")
        if out is None:
            rc = fn(self.handle, arr, n, None, 0, info, C.byref(need))
            if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
                check(rc)
            out = np.empty(max(need.value, 1), np.float32)
        check(fn(self.handle, arr, n, _ptr(out, c_f32p), out.size, info, C.byref(need)))
        return [out[o.offset: o.offset + o.length].reshape(-1, 4) for o in info], [_export_info_dict(o) for o in info]

    def get_envelope(self, track_id: int, ch: int, which: int = 1, start_sec: float = 0.0, end_sec: float = float("inf"), n_cols: int = 1):
        """th_tm_get_envelope -> (float32 [n_cols, 4], info dict) of one request"""
        req = _envelope_request((track_id, ch, which, start_sec, end_sec, n_cols))
        info = _ffi.EnvelopeInfo()
        fn = getattr(lib, self._PFX + "get_envelope")
        rc = fn(self.handle, C.byref(req), None, 0, C.byref(info))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = np.empty(max(info.length, 1), np.float32)
        check(fn(self.handle, C.byref(req), _ptr(out, c_f32p), out.size, C.byref(info)))
        return out[:info.length].reshape(-1, 4), _export_info_dict(info)

    def render_waveform_figures(self, requests, out: Optional[np.ndarray] = None):
        """th_tm_render_waveform_figures: requests = iterable of (track_id, ch, which, start_sec, end_sec, out_w, out_h, amp_lo,
        amp_hi, thickness, fill, background) -> (list of uint8 [out_h, out_w, 4] arrays, the top row = amp_hi, list of info dicts).
        out: a uint8 array to fill instead of a new one; the arrays are then views into it."""
        reqs = [_waveform_figure_request(r) for r in requests]
        n = len(reqs)
        if n == 0:
            return [], []
        arr = (_ffi.WaveformFigureRequest * n)(*reqs)
        info = (_ffi.WaveformFigureInfo * n)()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "render_waveform_figures")
        if out is None:
            rc = fn(self.handle, arr, n, None, 0, info, C.byref(need))
            if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
                check(rc)
            out = np.empty(max(need.value, 1), np.uint8)
        check(fn(self.handle, arr, n, out.ctypes.data, out.size, info, C.byref(need)))
        return ([out[o.offset: o.offset + o.bytes].reshape(o.out_h, o.out_w, 4) for o in info], [_export_info_dict(o) for o in info])

    def render_waveform_figure(self, track_id: int, ch: int, which: int, start_sec: float, end_sec: float, out_w: int, out_h: int,
                               amp_lo: float = -1.0, amp_hi: float = 1.0, thickness: int = 256, fill=(255, 255, 255, 255),
                               background=(0, 0, 0, 0)):
        """th_tm_render_waveform_figure -> (uint8 [out_h, out_w, 4], info dict) of one lane"""
        req = _waveform_figure_request((track_id, ch, which, start_sec, end_sec, out_w, out_h, amp_lo, amp_hi, thickness, fill, background))
        info = _ffi.WaveformFigureInfo()
        fn = getattr(lib, self._PFX + "render_waveform_figure")
        rc = fn(self.handle, C.byref(req), None, 0, C.byref(info))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = np.empty(max(info.bytes, 1), np.uint8)
        check(fn(self.handle, C.byref(req), out.ctypes.data, out.size, C.byref(info)))
        return out[:info.bytes].reshape(out_h, out_w, 4), _export_info_dict(info)


FORMANT_WIN_GAUSS, FORMANT_WIN_RECT = 0, 1
FORMANT_OUT_FORMANTS, FORMANT_OUT_LPC = 0, 1
c_f64p = C.POINTER(C.c_double)


def formant_request(track_id: int = 0, ch: int = 0, which: int = 0, start_sec: float = 0.0, end_sec: float = float("inf"), **kw) -> "_ffi.FormantRequest":
    """th_formant_defaults (the speech settings: sr_analysis 11000, n_poles 10, win_sec 0.05, step_sec 0.0125, preemph_hz 50, Gaussian
    window, formants) with the given fields replaced; keywords are the fields of th_formant_request"""
    r = _ffi.FormantRequest()
    check(lib.th_formant_defaults(C.byref(r)))
    r.id, r.ch, r.which, r.start_sec, r.end_sec = track_id, ch, which, start_sec, end_sec
    for k, v in kw.items():
        if k not in dict(r._fields_):
            raise TypeError("th_formant_request has no field %r" % k)
        setattr(r, k, v)
    return r


def _formant_request(r) -> "_ffi.FormantRequest":
    """a FormantRequest (formant_request), or a dict of its keywords"""
    return r if isinstance(r, _ffi.FormantRequest) else formant_request(**r)


def formant_plan(sr: int, n_samples: int, req) -> dict:
    """th_formant_plan_for -> the numbers of a request as a dict (host); rs: the resampler's (L, M, half_taps)"""
    req, pl = _formant_request(req), _ffi.FormantPlan()
    check(lib.th_formant_plan_for(sr, n_samples, C.byref(req), C.byref(pl)))
    d = {k: getattr(pl, k) for k, _ in pl._fields_ if k != "rs"}
    d["rs"] = (pl.rs.L, pl.rs.M, pl.rs.half_taps)
    return d


def formant_window(window: int, win: int) -> np.ndarray:
    """th_formant_window -> float64[win] (host)"""
    g = np.empty(max(int(win), 1), np.float64)
    check(lib.th_formant_window(window, win, _ptr(g, c_f64p)))
    return g


def formant_start_points(n_poles: int) -> np.ndarray:
    """th_formant_start_points -> complex128[n_poles] (host)"""
    z = np.empty(2 * max(int(n_poles), 1), np.float64)
    check(lib.th_formant_start_points(n_poles, _ptr(z, c_f64p)))
    return z[:n_poles] + 1j * z[n_poles:]


def formants_f64(x, sr: int, req, frame0: int = 0, n_frames: Optional[int] = None):
    """th_formants_f64: frames [frame0, frame0 + n_frames) (default: to the track's last) of one channel on the host, through the
    functions the kernel runs -> (float64 [n_frames, 2 + n_poles], (n_invalid, n_unconverged))"""
    x, req = _f32(x).ravel(), _formant_request(req)
    if n_frames is None:
        n_frames = formant_plan(sr, x.size, req)["n_frames_total"] - frame0
    out = np.empty((max(int(n_frames), 0), 2 + req.n_poles), np.float64)
    cnt = (C.c_uint64 * 2)()
    check(lib.th_formants_f64(_ptr(x, c_f32p), x.size, sr, C.byref(req), frame0, out.shape[0], _ptr(out, c_f64p), cnt))
    return out, (int(cnt[0]), int(cnt[1]))


def formant_frame_f64(x, sr: int, req, frame: int) -> dict:
    """th_formant_frame_f64: one frame's raw fit on the host -> dict(r, a, r0_loaded, E, roots (complex128), sweeps, status)"""
    x, req = _f32(x).ravel(), _formant_request(req)
    p = max(int(req.n_poles), 1)
    r, a, r0e, z = np.zeros(p + 1), np.zeros(p + 1), np.zeros(2), np.zeros(2 * p)
    sw, st = C.c_uint32(), C.c_uint32()
    check(lib.th_formant_frame_f64(_ptr(x, c_f32p), x.size, sr, C.byref(req), frame, _ptr(r, c_f64p), _ptr(a, c_f64p), _ptr(r0e, c_f64p),
                                   _ptr(z, c_f64p), C.byref(sw), C.byref(st)))
    return {"r": r, "a": a, "r0_loaded": r0e[0], "E": r0e[1], "roots": z[:p] + 1j * z[p:], "sweeps": sw.value, "status": st.value}


class _FormantMethods:
    """formant candidates (LPC fit, roots, (frequency, bandwidth) pairs) of a time range of resident audio (th_tm_* and th_tmg_*: _PFX)"""

    def get_formants(self, requests, out: Optional[np.ndarray] = None):
        """th_tm_get_formants: requests = iterable of formant_request(...) or dicts of its keywords -> (list of float64
        [n_frames, 2 + n_poles] arrays, list of info dicts).  out: a float64 array to fill instead of a new one; the arrays are then
        views into it."""
        reqs = [_formant_request(r) for r in requests]
        n = len(reqs)
        if n == 0:
            return [], []
        arr = (_ffi.FormantRequest * n)(*reqs)
        info = (_ffi.FormantInfo * n)()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "get_formants")
        if out is None:
            rc = fn(self.handle, arr, n, None, 0, info, C.byref(need))
            if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
                check(rc)
            out = np.empty(max(need.value, 1), np.float64)
        check(fn(self.handle, arr, n, _ptr(out, c_f64p), out.size, info, C.byref(need)))
        return ([out[o.offset: o.offset + o.length].reshape(-1, 2 + r.n_poles) for o, r in zip(info, reqs)],
                [_export_info_dict(o) for o in info])

    def get_formant_track(self, track_id: int, ch: int, which: int = 0, start_sec: float = 0.0, end_sec: float = float("inf"), **kw):
        """th_tm_get_formant_track -> (float64 [n_frames, 2 + n_poles], info dict) of one request (keywords: formant_request)"""
        req = formant_request(track_id, ch, which, start_sec, end_sec, **kw)
        info = _ffi.FormantInfo()
        fn = getattr(lib, self._PFX + "get_formant_track")
        rc = fn(self.handle, C.byref(req), None, 0, C.byref(info))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = np.empty(max(info.length, 1), np.float64)
        check(fn(self.handle, C.byref(req), _ptr(out, c_f64p), out.size, C.byref(info)))
        return out[:info.length].reshape(-1, 2 + req.n_poles), _export_info_dict(info)


ALIGN_OUT_SUMMARY, ALIGN_OUT_CURVE = 0, 1
ALIGN_ABS = 1
ALIGN_SUMMARY_DOUBLES = 10
ALIGN_MAX_REF, ALIGN_MAX_LAG, ALIGN_MAX_WORK, ALIGN_PIECE_LAGS = 1 << 22, 1 << 20, 1 << 40, 65536
ALIGN_SUMMARY_FIELDS = ("status", "lag", "delta", "r", "e_ref", "e_probe", "rho", "gain", "null_dB", "polarity")


def align_request(ref_id: int = 0, ref_ch: int = 0, track_id: int = 0, ch: int = 0, start_sec: float = 0.0, end_sec: float = float("inf"),
                  max_lag_sec: float = 0.0, kind: int = ALIGN_OUT_SUMMARY, flags: int = 0, ref_which: int = 0, which: int = 0) -> "_ffi.AlignRequest":
    """th_align_request: the reference (ref_id, ref_ch, ref_which), the probe (track_id, ch, which), a range of the reference, the
    largest lag searched, ALIGN_OUT_*, ALIGN_ABS or 0"""
    return _ffi.AlignRequest(ref_id, ref_ch, ref_which, track_id, ch, which, start_sec, end_sec, max_lag_sec, kind, flags)


def _align_request(r) -> "_ffi.AlignRequest":
    """an AlignRequest (align_request), or a dict of its keywords"""
    return r if isinstance(r, _ffi.AlignRequest) else align_request(**r)


def align_plan(sr_ref: int, n_ref: int, sr: int, n: int, req) -> dict:
    """th_align_plan_for -> the numbers of a request as a dict (host)"""
    req, pl = _align_request(req), _ffi.AlignPlan()
    check(lib.th_align_plan_for(sr_ref, n_ref, sr, n, C.byref(req), C.byref(pl)))
    return {k: getattr(pl, k) for k, _ in pl._fields_}


def xcorr_f64(a, b, first: int, n_lags: int) -> np.ndarray:
    """th_xcorr_f64: r[i] = sum_k a[k] b[first + i + k], i < n_lags, in the reader's order (host) -> float64[n_lags]"""
    a, b = _f32(a).ravel(), _f32(b).ravel()
    r = np.empty(max(int(n_lags), 1), np.float64)
    check(lib.th_xcorr_f64(_ptr(a, c_f32p), a.size, _ptr(b, c_f32p), b.size, first, n_lags, _ptr(r, c_f64p)))
    return r[:n_lags]


def align_energy_f64(x, first: int, n_sum: int) -> float:
    """th_align_energy_f64: E(x, first, n_sum) in the reader's order (host)"""
    x, e = _f32(x).ravel(), C.c_double()
    check(lib.th_align_energy_f64(_ptr(x, c_f32p), x.size, first, n_sum, C.byref(e)))
    return e.value


def align_peak(r, flags: int, e_ref: float) -> dict:
    """th_align_peak: the host's step on a curve -> dict(status, peak (index into r), delta, polarity)"""
    r = np.ascontiguousarray(r, np.float64).ravel()
    st, pk, de, po = C.c_uint32(), C.c_size_t(), C.c_double(), C.c_double()
    check(lib.th_align_peak(_ptr(r, c_f64p), r.size, flags, e_ref, C.byref(st), C.byref(pk), C.byref(de), C.byref(po)))
    return {"status": st.value, "peak": pk.value, "delta": de.value, "polarity": po.value}


def align_f64(ref, sr_ref: int, probe, sr: int, req) -> np.ndarray:
    """th_align_f64: a whole request from two host channels, the reader's bits -> float64[ALIGN_SUMMARY_DOUBLES (+ n_lags)]"""
    ref, probe, req = _f32(ref).ravel(), _f32(probe).ravel(), _align_request(req)
    need = C.c_size_t()
    rc = lib.th_align_f64(_ptr(ref, c_f32p), ref.size, sr_ref, _ptr(probe, c_f32p), probe.size, sr, C.byref(req), None, 0, C.byref(need))
    if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
        check(rc)
    out = np.empty(max(need.value, 1), np.float64)
    check(lib.th_align_f64(_ptr(ref, c_f32p), ref.size, sr_ref, _ptr(probe, c_f32p), probe.size, sr, C.byref(req), _ptr(out, c_f64p), out.size,
                           C.byref(need)))
    return out[:need.value]


def align_summary(rec) -> dict:
    """the first ALIGN_SUMMARY_DOUBLES doubles of a request's record as a dict (ALIGN_SUMMARY_FIELDS)"""
    return dict(zip(ALIGN_SUMMARY_FIELDS, (float(v) for v in rec[:ALIGN_SUMMARY_DOUBLES])))


class _AlignMethods:
    """lag, gain and null depth of a probe channel against a range of a reference channel (th_tm_* and th_tmg_*: _PFX).  A positive lag:
    the probe is late; subtract lag / sr from the probe's time arguments"""

    def align_tracks(self, requests, out: Optional[np.ndarray] = None):
        """th_tm_align_tracks: requests = iterable of align_request(...) or dicts of its keywords -> (list of float64 records: the ten
        summary doubles, then the curve for ALIGN_OUT_CURVE; list of info dicts).  out: a float64 array to fill instead of a new one;
        the records are then views into it."""
        reqs = [_align_request(r) for r in requests]
        n = len(reqs)
        if n == 0:
            return [], []
        arr = (_ffi.AlignRequest * n)(*reqs)
        info = (_ffi.AlignInfo * n)()
        need = C.c_size_t()
        fn = getattr(lib, self._PFX + "align_tracks")
        if out is None:
            rc = fn(self.handle, arr, n, None, 0, info, C.byref(need))
            if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
                check(rc)
            out = np.empty(max(need.value, 1), np.float64)
        check(fn(self.handle, arr, n, _ptr(out, c_f64p), out.size, info, C.byref(need)))
        return [out[o.offset: o.offset + o.length] for o in info], [_export_info_dict(o) for o in info]

    def align_track(self, ref_id: int, ref_ch: int, track_id: int, ch: int, **kw):
        """th_tm_align_track -> (float64 record, info dict) of one request (keywords: align_request)"""
        req = align_request(ref_id, ref_ch, track_id, ch, **kw)
        info = _ffi.AlignInfo()
        fn = getattr(lib, self._PFX + "align_track")
        rc = fn(self.handle, C.byref(req), None, 0, C.byref(info))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = np.empty(max(info.length, 1), np.float64)
        check(fn(self.handle, C.byref(req), _ptr(out, c_f64p), out.size, C.byref(info)))
        return out[:info.length], _export_info_dict(info)


def true_peak_filter(sr: int):
    """-> (factor, coef f64, phase, delay) of the kept taps of the true-peak interpolator at rate sr, ascending tap index (host)"""
    f, n = C.c_uint32(), C.c_uint32()
    c, p, d = (C.c_double * 49)(), (C.c_uint32 * 49)(), (C.c_uint32 * 49)()
    check(lib.th_true_peak_filter(sr, C.byref(f), c, p, d, C.byref(n)))
    return f.value, np.array(c[:n.value]), np.array(p[:n.value], np.uint32), np.array(d[:n.value], np.uint32)


def loudness_n_short_term(n_samples: int, sr: int) -> int:
    n = C.c_size_t()
    check(lib.th_loudness_n_short_term(n_samples, sr, C.byref(n)))
    return n.value


def loudness_range(short_term_energies_1s) -> float:
    """EBU Tech 3342 loudness range (LU) of the 3 s block energies taken once per second (host arithmetic)"""
    e = np.ascontiguousarray(short_term_energies_1s, dtype=np.float64)
    out = C.c_double()
    check(lib.th_loudness_range(e.ctypes.data_as(C.POINTER(C.c_double)), e.size, C.byref(out)))
    return out.value


class _DynamicsMethods:
    """set_common_normalize / set_common_guard_clipping and what they leave to read (th_tm_* and th_tmg_*: _PFX)"""

    def _dyn(self, name):
        return getattr(lib, self._PFX + name)

    def set_common_normalize(self, kind: int, target: float = 0.0):
        check(self._dyn("set_common_normalize")(self.handle, kind, target))

    def set_common_guard_clipping(self, mode: int):
        check(self._dyn("set_common_guard_clipping")(self.handle, mode))

    def common_dynamics(self):
        """-> (normalize kind, target, guard-clipping mode)"""
        k, t, m = C.c_int(), C.c_float(), C.c_int()
        check(self._dyn("get_common_dynamics")(self.handle, C.byref(k), C.byref(t), C.byref(m)))
        return k.value, t.value, m.value

    def track_dynamics(self, track_id: int) -> dict:
        o = _ffi.TrackDynamics()
        check(self._dyn("get_track_dynamics")(self.handle, track_id, C.byref(o)))
        return {"normalize_gain": np.float32(o.normalize_gain), "guard_result": o.guard_result,
                "global_gain": np.float32(o.global_gain), "draws_before_clip": bool(o.draws_before_clip)}

    def guard_clip_stats(self, track_id: int):
        """the GuardClippingStats format_guard_clip_stats selects: [(max_reduction_gain_dB, reduction_cnt)]"""
        n = C.c_size_t()
        rc = self._dyn("get_guard_clip_stats")(self.handle, track_id, None, 0, C.byref(n))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        out = (_ffi.GuardClipStats * max(n.value, 1))()
        check(self._dyn("get_guard_clip_stats")(self.handle, track_id, out, n.value, C.byref(n)))
        return [(np.float32(out[i].max_reduction_gain_dB), int(out[i].reduction_cnt)) for i in range(n.value)]

    def limiter_gain(self, track_id: int):
        """guard_clipping_gain (audio.rs:80-92): None, [1.0], or the n_samples gains"""
        n = C.c_size_t()
        rc = self._dyn("get_limiter_gain")(self.handle, track_id, None, 0, C.byref(n))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        if n.value == 0:
            return None
        out = np.empty(n.value, np.float32)
        check(self._dyn("get_limiter_gain")(self.handle, track_id, _ptr(out, c_f32p), out.size, C.byref(n)))
        return out

    def audio(self, track_id: int, ch: int, which: int = 0) -> np.ndarray:
        """one channel's samples: which = 0 the audio, 1 what the waveform is drawn from, 2 the original"""
        m = self.render_metadata(track_id, ch, 0.0, False)
        out = np.empty(m["sample_count"], np.float32)
        check(self._dyn("copy_audio")(self.handle, track_id, ch, which, _ptr(out, c_f32p), out.size))
        return out


def k_weighting(sr: int):
    """-> (b[5], a[5]) of the K-weighting section at rate sr (host arithmetic)"""
    b, a = (C.c_double * 5)(), (C.c_double * 5)()
    check(lib.th_k_weighting(sr, b, a))
    return np.array(b[:]), np.array(a[:])


def loudness_n_blocks(n_samples: int, sr: int) -> int:
    n = C.c_size_t()
    check(lib.th_loudness_n_blocks(n_samples, sr, C.byref(n)))
    return n.value


def gated_loudness(block_energies) -> float:
    """integrated LUFS of a block-energy series (host arithmetic)"""
    e = np.ascontiguousarray(block_energies, dtype=np.float64)
    out = C.c_double()
    check(lib.th_gated_loudness(e.ctypes.data_as(C.POINTER(C.c_double)), e.size, C.byref(out)))
    return out.value


class DeviceBuffer:
    """hipMalloc'd buffer owned through the C ABI (th_dev_alloc / th_dev_free)."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = vp()
        check(lib.th_dev_alloc(ctx.handle, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        check(lib.th_dev_upload(self.ctx.handle, self.ptr, a.ctypes.data, a.nbytes))
        return self

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        check(lib.th_dev_download(self.ctx.handle, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            check(lib.th_dev_free(self.ctx.handle, self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Graph:
    """A captured launch sequence (Context.capture); launch() replays it on the context's stream."""

    def __init__(self, handle):
        self.handle = handle

    def launch(self):
        check(lib.th_graph_launch(self.handle))

    def close(self):
        if self.handle:
            lib.th_graph_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """th_ctx: one GPU + one HIP stream.  `stream=None` creates a private stream; an int is used as
    the raw hipStream_t (e.g. torch.cuda.current_stream().cuda_stream; 0 = legacy default stream)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        h = vp()
        if stream is None:
            check(lib.th_ctx_create(device, None, C.byref(h)))
        else:
            check(lib.th_ctx_create_ex(device, vp(stream), 1, C.byref(h)))
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            check(lib.th_ctx_destroy(self.handle))
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def synchronize(self):
        check(lib.th_ctx_synchronize(self.handle))

    def capture(self, fn) -> "Graph":
        """Record the library calls `fn()` makes on this context's stream into a HIP graph (th_ctx_capture_begin / _end).
        Call `fn()` once normally first: tables and scratch buffers are uploaded / sized on first use."""
        check(lib.th_ctx_capture_begin(self.handle))
        h = C.c_void_p()
        try:
            fn()
        except BaseException:
            lib.th_ctx_capture_end(self.handle, C.byref(h))  # leave capture mode; the error of fn() is the one to report
            if h.value:
                lib.th_graph_destroy(h)
            raise
        check(lib.th_ctx_capture_end(self.handle, C.byref(h)))
        return Graph(h)

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def to_device(self, a: np.ndarray) -> DeviceBuffer:
        a = np.ascontiguousarray(a)
        return DeviceBuffer(self, max(a.nbytes, 1)).upload(a)

    def dev_copy(self, dst_ptr: int, src_ptr: int, nbytes: int):
        """Stream-ordered device copy with the library's 16-byte-per-lane streaming kernel (the bench's bandwidth yardstick)."""
        check(lib.th_dev_copy(self.handle, dst_ptr, src_ptr, nbytes))

    def timer_start(self):
        check(lib.th_timer_start(self.handle))

    def timer_stop_ms(self) -> float:
        ms = C.c_float()
        check(lib.th_timer_stop_ms(self.handle, C.byref(ms)))
        return ms.value

    # ---- convert_spectrogram_to_img (drawing.rs:4-33), numpy in/out
    def spec_to_img(self, spec: np.ndarray, i_freq_range, dB_range, colormap_length: Optional[int]) -> np.ndarray:
        spec = _f32(spec)
        T, H = spec.shape
        i0, i1 = i_freq_range
        d_spec = self.to_device(spec)
        d_img = self.alloc(max((i1 - i0) * T * 2, 1))
        check(lib.th_spec_to_img_dev(self.handle, d_spec.ptr, T, H, i0, i1, dB_range[0], dB_range[1],
                                     0 if colormap_length is None else colormap_length, d_img.ptr))
        out = d_img.download((i1 - i0, T), np.uint16)
        d_spec.free()
        d_img.free()
        return out

    def spec_to_img_batch(self, descs: Sequence[ImgDesc], min_dB: float, max_dB: float, colormap_length: int):
        arr = descs if isinstance(descs, C.Array) else (ImgDesc * len(descs))(*descs)
        check(lib.th_spec_to_img_batch_dev(self.handle, arr, len(arr), min_dB, max_dB, colormap_length))

    # ---- encode_spectrogram_tile (render_tiles.rs:281-352), numpy image in, bytes out
    def encode_spectrogram_tile(self, img: np.ndarray, colormap_rgba: bytes, revision: int, level_x: int,
                                level_y: int, tile_x: int, tile_y: int) -> bytes:
        img = np.ascontiguousarray(img, dtype=np.uint16)
        d_img = self.to_device(img)
        try:
            return self.encode_spectrogram_tile_dev(d_img.ptr, img.shape[0], img.shape[1], colormap_rgba, revision,
                                                    level_x, level_y, tile_x, tile_y, 0)
        finally:
            d_img.free()

    def encode_spectrogram_tile_dev(self, d_img: int, img_height: int, img_width: int, colormap_rgba: bytes,
                                    revision: int, level_x: int, level_y: int, tile_x: int, tile_y: int,
                                    img_pitch: int = 0) -> bytes:
        cm = np.frombuffer(bytes(colormap_rgba), np.uint8)
        out = np.empty(SPECTROGRAM_TILE_MAX_BYTES, np.uint8)
        n = C.c_size_t()
        check(lib.th_encode_spectrogram_tile_dev(self.handle, d_img, img_height, img_width, img_pitch, _ptr(cm, c_u8p), cm.size,
                                                 revision, level_x, level_y, tile_x, tile_y, _ptr(out, c_u8p),
                                                 out.size, C.byref(n)))
        return out[: n.value].tobytes()

    def raster_tiles(self, descs: Sequence[RasterDesc], d_colormap: int, n_colors: int):
        arr = descs if isinstance(descs, C.Array) else (RasterDesc * len(descs))(*descs)
        check(lib.th_raster_tiles_dev(self.handle, arr, len(arr), d_colormap, n_colors))

    def make_img_tiles_descs(self, items):
        """items: iterable of (ImgDesc, [device pointer of tile (tx, ty) at tx * n_ty + ty, 0 = skip]) -> ctypes array of
        th_img_tiles_desc (keeps the pointer arrays alive)."""
        items = list(items)
        arr = (_ffi.ImgTilesDesc * len(items))()
        keep = []
        for i, (d, ptrs) in enumerate(items):
            out_h, w = int(d.i_end - d.i_start), int(d.n_frames)
            n_tx, n_ty = (-(-w // 512), -(-out_h // 512)) if out_h and w else (0, 0)
            assert len(ptrs) == n_tx * n_ty, (len(ptrs), n_tx, n_ty)
            pa = (C.c_void_p * max(len(ptrs), 1))(*[C.c_void_p(p or None) for p in ptrs])
            keep.append(pa)
            arr[i].img = d
            arr[i].tiles = C.cast(pa, C.POINTER(C.c_void_p))
            arr[i].n_tiles_x, arr[i].n_tiles_y = n_tx, n_ty
        arr._keep = keep
        return arr

    def spec_to_img_raster_batch(self, descs, d_colormap: int, n_colors: int, min_dB: float = 0.0, max_dB: float = 0.0,
                                 d_range: int = 0):
        """th_spec_to_img_raster_batch_dev: quantise + every level-0 tile in one pass.  descs: make_img_tiles_descs(...)."""
        check(lib.th_spec_to_img_raster_batch_dev(self.handle, descs, len(descs), min_dB, max_dB, d_range or None, d_colormap, n_colors))

    # ---- encode_waveform_tile (render_tiles.rs:232-279)
    def encode_waveform_tile(self, wav: np.ndarray, revision: int, level: int, tile_index: int) -> bytes:
        wav = _f32(wav)
        d = self.to_device(wav)
        try:
            return self.encode_waveform_tile_dev(d.ptr, wav.size, revision, level, tile_index)
        finally:
            d.free()

    def encode_waveform_tile_dev(self, d_wav: int, n_samples: int, revision: int, level: int,
                                 tile_index: int) -> bytes:
        out = np.empty(WAVEFORM_TILE_MAX_BYTES, np.uint8)
        n = C.c_size_t()
        check(lib.th_encode_waveform_tile_dev(self.handle, d_wav, n_samples, revision, level, tile_index,
                                              _ptr(out, c_u8p), out.size, C.byref(n)))
        return out[: n.value].tobytes()

    def waveform_tiles(self, descs: Sequence[WaveDesc]):
        arr = descs if isinstance(descs, C.Array) else (WaveDesc * len(descs))(*descs)
        check(lib.th_waveform_tiles_dev(self.handle, arr, len(arr)))

    def minmax_reduce_dev(self, d_minmax: int, n_chan: int, d_out: int):
        """[min, -max] over n_chan per-channel (min, max) pairs, device to device (core/mod.rs:169-178)"""
        check(lib.th_minmax_reduce_dev(self.handle, d_minmax, n_chan, d_out))

    def global_db_range_dev(self, d_min_negmax: int, dB_range: float, d_range: int):
        """[min, -max] -> [min_dB, max_dB] on the device (core/mod.rs:179-180)"""
        check(lib.th_global_db_range_dev(self.handle, d_min_negmax, dB_range, d_range))

    def minmax_reduce_range_dev(self, d_minmax: int, n_chan: int, dB_range: float, d_range: int, d_min_negmax: int = 0):
        """th_minmax_reduce_dev + th_global_db_range_dev in one launch (single GPU: no all-reduce in between)."""
        check(lib.th_minmax_reduce_range_dev(self.handle, d_minmax, n_chan, dB_range, d_min_negmax or None, d_range))

    def spec_to_img_batch_ranged(self, descs, d_range: int, colormap_len: int):
        arr = descs if isinstance(descs, C.Array) else (ImgDesc * len(descs))(*descs)
        check(lib.th_spec_to_img_batch_dev_ranged(self.handle, arr, len(arr), d_range, colormap_len))

    # ---- channel statistics (sum_squares / abs_max, simd.rs:113-183)
    def channel_stats_dev(self, descs):
        """-> (sum_squares[n], abs_max[n]) float32 host arrays"""
        arr = descs if isinstance(descs, C.Array) else (_ffi.StatsDesc * len(descs))(*descs)
        ss, pk = np.empty(len(arr), np.float32), np.empty(len(arr), np.float32)
        check(lib.th_channel_stats_dev(self.handle, arr, len(arr), _ptr(ss, c_f32p), _ptr(pk, c_f32p)))
        return ss, pk

    # ---- loudness (StatCalculator::calc, dynamics/stats.rs:56-86)
    def audio_stats_dev(self, tracks):
        """tracks: [(channel device pointers, n_samples, sr, block_energy device pointer or 0)] -> [dict] of th_audio_stats
        (global_lufs, rms_dB, max_peak, max_peak_dB); the block energies land in the given device buffers"""
        descs = (_ffi.AudioDesc * len(tracks))()
        keep = []
        for d, (chans, n, sr, be) in zip(descs, tracks):
            arr = (C.c_void_p * len(chans))(*chans)
            keep.append(arr)
            d.channels = C.cast(arr, C.POINTER(C.c_void_p))
            d.n_samples, d.n_channels, d.sr, d.block_energy = n, len(chans), sr, be or None
        out = (_ffi.AudioStats * max(len(tracks), 1))()
        check(lib.th_audio_stats_dev(self.handle, descs, len(tracks), out))
        return [_audio_stats_dict(o) for o in out[:len(tracks)]]

    # ---- waveform pyramid: all levels of a channel in one pass over the audio
    def waveform_pyramid_dev(self, descs):
        arr = descs if isinstance(descs, C.Array) else (_ffi.PyramidDesc * len(descs))(*descs)
        check(lib.th_waveform_pyramid_dev(self.handle, arr, len(arr)))

    def waveform_pyramid(self, wav: np.ndarray, n_levels: int):
        """Host convenience (tests): returns [level] -> ndarray [bins, 3] of (min, max, mean)."""
        wav = _f32(wav)
        total = pyramid_offset(wav.size, n_levels)
        d = self.to_device(wav)
        o = self.alloc(max(total, 1) * 4)
        try:
            self.waveform_pyramid_dev([_ffi.PyramidDesc(d.ptr, o.ptr, wav.size, n_levels, 0)])
            flat = o.download((max(total, 1),), np.float32)[:total]
        finally:
            d.free()
            o.free()
        return [flat[pyramid_offset(wav.size, l): pyramid_offset(wav.size, l) + 3 * pyramid_bins(wav.size, l)].reshape(-1, 3)
                for l in range(n_levels)]


# ------------------------------------------------------------------ SpectrogramAnalyzer plan
class Plan:
    """th_plan: device-resident window / twiddles / mel filterbank for one framing key
    (SpectrogramAnalyzer::prepare, spectrogram.rs:116-154)."""

    def __init__(self, ctx: Context, sr: int, win: int, hop: int, n_fft: int, freq_scale: int = LINEAR,
                 n_mel: int = 0):
        h = vp()
        check(lib.th_plan_create(ctx.handle, sr, win, hop, n_fft, freq_scale, n_mel, C.byref(h)))
        self.handle, self.ctx = h, ctx
        self.sr, self.win, self.hop, self.n_fft, self.freq_scale = sr, win, hop, n_fft, freq_scale
        f, hh = C.c_size_t(), C.c_size_t()
        check(lib.th_plan_dims(h, C.byref(f), C.byref(hh)))
        self.n_freq, self.height = f.value, hh.value

    def close(self):
        if self.handle:
            check(lib.th_plan_destroy(self.handle))
            self.handle = None

    def time_kernel(self, enable: bool = True):
        """record HIP events around the dominant kernel of every calc_spec_batch_dev (measurement hook)"""
        check(lib.th_plan_time_kernel(self.handle, int(enable)))

    def kernel_ms_history(self) -> np.ndarray:
        """durations (ms) of the most recent timed launches, oldest first (at most 64)"""
        out, n = np.empty(64, np.float32), C.c_size_t()
        check(lib.th_plan_kernel_ms_history(self.handle, _ptr(out, c_f32p), out.size, C.byref(n)))
        return out[: n.value].copy()

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        check(lib.th_plan_last_kernel_ms(self.handle, C.byref(ms)))
        return ms.value

    def mel_moments_info(self) -> dict:
        """the moment-form table of the fused mel epilogue (n_fft 4096 / 8192 / 16384), if the plan has one (groups == 0: it does not)"""
        g, t, d, a = C.c_uint32(), C.c_uint32(), C.c_double(), C.c_double()
        check(lib.th_plan_mel_moments_info(self.handle, C.byref(g), C.byref(t), C.byref(d), C.byref(a)))
        return {"groups": g.value, "taps": t.value, "max_dev": d.value, "max_amp": a.value}

    def set_kernel(self, which: int):
        check(lib.th_plan_set_kernel(self.handle, which))

    @property
    def kernel_name(self) -> str:
        return (lib.th_plan_kernel_name(self.handle) or b"").decode()

    def n_frames(self, n_samples: int) -> int:
        return stft_n_frames(n_samples, self.win, self.hop)

    def calc_spec_batch_dev(self, descs: Sequence[ChanDesc], d_minmax: Optional[int]):
        """Stream-ordered batched calc_spec on device pointers (no sync)."""
        arr = descs if isinstance(descs, C.Array) else (ChanDesc * len(descs))(*descs)
        check(lib.th_calc_spec_batch_dev(self.handle, arr, len(arr), d_minmax))

    def calc_spec_batch_ranged_dev(self, descs: Sequence[ChanDesc], d_minmax: int, dB_range: float, d_range: int):
        """calc_spec_batch_dev + the global dB range of the batch into d_range (single GPU), one call."""
        arr = descs if isinstance(descs, C.Array) else (ChanDesc * len(descs))(*descs)
        check(lib.th_calc_spec_batch_ranged_dev(self.handle, arr, len(arr), d_minmax, dB_range, d_range))

    def calc_spec(self, wav: np.ndarray):
        """calc_spec for one channel with host buffers -> (T x H f32 dB, min, max)."""
        wav = _f32(wav)
        T = self.n_frames(wav.size)
        out = np.empty((T, self.height), np.float32)
        n, mn, mx = C.c_size_t(), C.c_float(), C.c_float()
        check(lib.th_calc_spec_host(self.handle, _ptr(wav, c_f32p), wav.size, _ptr(out, c_f32p), out.size,
                                    C.byref(n), C.byref(mn), C.byref(mx)))
        assert n.value == T
        return out, mn.value, mx.value

    def calc_spec_batch(self, wavs: Iterable[np.ndarray]):
        """Batched calc_spec over host arrays -> (list of specs, (n,2) min/max)."""
        wavs = [_f32(w) for w in wavs]
        ctx = self.ctx
        d_w = [ctx.to_device(w) for w in wavs]
        Ts = [self.n_frames(w.size) for w in wavs]
        d_s = [ctx.alloc(max(T * self.height * 4, 4)) for T in Ts]
        d_mm = ctx.alloc(8 * len(wavs))
        descs = [ChanDesc(dw.ptr, ds.ptr, w.size, T, 0) for dw, ds, w, T in zip(d_w, d_s, wavs, Ts)]
        self.calc_spec_batch_dev(descs, d_mm.ptr)
        ctx.synchronize()
        specs = [ds.download((T, self.height), np.float32) for ds, T in zip(d_s, Ts)]
        mm = d_mm.download((len(wavs), 2), np.float32)
        for b in d_w + d_s + [d_mm]:
            b.free()
        return specs, mm


# ------------------------------------------------------------------ TrackManager mirror
class TileCache:
    """th_tile_cache: mirror of RenderTileCache (render_tiles.rs:51-230) — byte-budgeted LRU of encoded waveform
    tiles plus the waveform / spectrogram revision counters.  Host only."""

    def __init__(self, budget_bytes: int = 0, _borrowed=None):
        if _borrowed is not None:
            self.handle, self._own = _borrowed, False
            return
        h = vp()
        check(lib.th_tile_cache_create(budget_bytes, C.byref(h)))
        self.handle, self._own = h, True

    def close(self):
        if self.handle and self._own:
            check(lib.th_tile_cache_destroy(self.handle))
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def lookup(self, track_id: int, ch: int, level: int, tile_index: int):
        """-> (current waveform revision, bytes or None); a hit makes the entry most recently used."""
        cap = WAVEFORM_TILE_MAX_BYTES
        while True:
            out = np.empty(cap, np.uint8)
            n, rev, hit = C.c_size_t(), C.c_uint64(), C.c_int()
            rc = lib.th_tile_cache_lookup(self.handle, track_id, ch, level, tile_index, C.byref(rev), _ptr(out, c_u8p),
                                          out.size, C.byref(n), C.byref(hit))
            if rc == _ffi.ERR_BUFFER_TOO_SMALL and n.value > cap:
                cap = n.value
                continue
            check(rc)
            return rev.value, (out[: n.value].tobytes() if hit.value else None)

    def store(self, track_id: int, ch: int, revision: int, level: int, tile_index: int, data: bytes):
        a = np.frombuffer(bytes(data), np.uint8)
        check(lib.th_tile_cache_store(self.handle, track_id, ch, revision, level, tile_index, _ptr(a, c_u8p), a.size))

    def invalidate_waveform(self):
        check(lib.th_tile_cache_invalidate(self.handle, 1, 0))

    def invalidate_spectrogram(self):
        check(lib.th_tile_cache_invalidate(self.handle, 0, 1))

    def invalidate_all(self):
        check(lib.th_tile_cache_invalidate(self.handle, 1, 1))

    def set_budget(self, budget_bytes: int):
        check(lib.th_tile_cache_set_budget(self.handle, budget_bytes))

    def stats(self) -> dict:
        e, b, bud = C.c_size_t(), C.c_size_t(), C.c_size_t()
        wr, sr, h, m = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib.th_tile_cache_stats(self.handle, C.byref(e), C.byref(b), C.byref(bud), C.byref(wr), C.byref(sr),
                                      C.byref(h), C.byref(m)))
        return {"entries": e.value, "bytes": b.value, "budget_bytes": bud.value, "waveform_revision": wr.value,
                "spectrogram_revision": sr.value, "hits": h.value, "misses": m.value}


class TrackManager(_DynamicsMethods, _SpectrumMethods, _LoudnessMeterMethods, _ExportMethods, _ExportAtMethods, _ExportBandMethods, _FigureMethods, _EnvelopeMethods, _FormantMethods, _AlignMethods):
    """th_tm: mirror of core/mod.rs TrackManager with HBM-resident audio / specs / images."""
    _PFX = "th_tm_"

    def __init__(self, ctx: Context):
        h = vp()
        check(lib.th_tm_create(ctx.handle, C.byref(h)))
        self.handle, self.ctx = h, ctx
        # pinned output buffers of get_spectrogram_tiles(pinned=True): a small POOL, one buffer checked out per call (tile
        # getters run concurrently from IPC threads and ctypes drops the GIL during the C call — ADVICE r4: a buffer shared
        # by two calls in flight let one caller read another's pixels; ADVICE r5: a buffer per THREAD leaked one pinned block
        # per exited thread).  At most PIN_POOL_MAX idle buffers are kept; close() frees them all.
        self._pin_free = []  # idle buffers: (capacity, c_void_p), under _pin_lock
        self._pin_all = {}   # address -> c_void_p of every live pinned buffer, idle or checked out (for close())
        self._pin_lock = threading.Lock()

    PIN_POOL_MAX = 4

    def _pin_checkout(self, nbytes: int):
        """An idle pinned buffer of >= nbytes (the smallest that fits), else a new one.  The caller owns it until _pin_return."""
        with self._pin_lock:
            fit = [i for i, (cap, _) in enumerate(self._pin_free) if cap >= nbytes]
            if fit:
                return self._pin_free.pop(min(fit, key=lambda i: self._pin_free[i][0]))
        p = C.c_void_p()
        check(lib.th_host_alloc(self.ctx.handle, nbytes, C.byref(p)))
        with self._pin_lock:
            self._pin_all[p.value] = p
        return nbytes, p

    def _pin_return(self, cap: int, p) -> None:
        drop = None
        with self._pin_lock:
            self._pin_free.append((cap, p))
            if len(self._pin_free) > self.PIN_POOL_MAX:   # keep the large ones: they serve every request size
                drop = self._pin_free.pop(min(range(len(self._pin_free)), key=lambda i: self._pin_free[i][0]))
                self._pin_all.pop(drop[1].value, None)
        if drop is not None:
            check(lib.th_host_free(self.ctx.handle, drop[1]))

    def _free_pinned(self):
        """close(): every buffer (the caller guarantees no tile call is in flight, as for the handle itself)"""
        with self._pin_lock:
            bufs, self._pin_all, self._pin_free = list(self._pin_all.values()), {}, []
        for p in bufs:
            check(lib.th_host_free(self.ctx.handle, p))

    def close(self):
        if self.handle:
            self._free_pinned()
            check(lib.th_tm_destroy(self.handle))
            self.handle = None

    def set_colormap(self, rgba: bytes):
        a = np.frombuffer(bytes(rgba), np.uint8)
        check(lib.th_tm_set_colormap(self.handle, _ptr(a, c_u8p), a.size))

    def set_setting(self, win_ms: float, t_overlap: int, f_overlap: int, freq_scale: int):
        check(lib.th_tm_set_setting(self.handle, win_ms, t_overlap, f_overlap, freq_scale))

    def set_dB_range(self, dB_range: float):
        check(lib.th_tm_set_dB_range(self.handle, dB_range))

    def add_tracks(self, tracks):
        """tracks: iterable of (id, sr, planar ndarray [channels, samples])."""
        tracks = [(i, sr, np.atleast_2d(_f32(w))) for i, sr, w in tracks]
        n = len(tracks)
        ids = (C.c_size_t * n)(*[t[0] for t in tracks])
        srs = (C.c_uint32 * n)(*[t[1] for t in tracks])
        nch = (C.c_uint32 * n)(*[t[2].shape[0] for t in tracks])
        ns = (C.c_size_t * n)(*[t[2].shape[1] for t in tracks])
        rows = [np.ascontiguousarray(t[2][c]) for t in tracks for c in range(t[2].shape[0])]
        ptrs = (c_f32p * len(rows))(*[_ptr(r, c_f32p) for r in rows])
        check(lib.th_tm_add_tracks(self.handle, n, ids, srs, nch, ptrs, ns))

    def remove_track(self, track_id: int):
        check(lib.th_tm_remove_track(self.handle, track_id))

    def apply_track_list_changes(self):
        cap = 4096
        ids = (C.c_size_t * cap)()
        n, sr = C.c_size_t(), C.c_uint32()
        check(lib.th_tm_apply_track_list_changes(self.handle, ids, cap, C.byref(n), C.byref(sr)))
        return sorted(ids[i] for i in range(min(n.value, cap))), sr.value

    def db_state(self):
        lo, hi, sr = C.c_float(), C.c_float(), C.c_uint32()
        check(lib.th_tm_get_db_state(self.handle, C.byref(lo), C.byref(hi), C.byref(sr)))
        return lo.value, hi.value, sr.value

    def revisions(self):
        w, s = C.c_uint64(), C.c_uint64()
        check(lib.th_tm_revisions(self.handle, C.byref(w), C.byref(s)))
        return w.value, s.value

    def spec(self, track_id: int, ch: int) -> np.ndarray:
        t, h = C.c_size_t(), C.c_size_t()
        check(lib.th_tm_spec_shape(self.handle, track_id, ch, C.byref(t), C.byref(h)))
        out = np.empty((t.value, h.value), np.float32)
        check(lib.th_tm_copy_spec(self.handle, track_id, ch, _ptr(out, c_f32p), out.size))
        return out

    def img(self, track_id: int, ch: int) -> np.ndarray:
        h, w = C.c_size_t(), C.c_size_t()
        check(lib.th_tm_img_shape(self.handle, track_id, ch, C.byref(h), C.byref(w)))
        out = np.empty((h.value, w.value), np.uint16)
        check(lib.th_tm_copy_img(self.handle, track_id, ch, _ptr(out, c_u16p), out.size))
        return out

    def get_spectrogram_tile(self, track_id: int, ch: int, level_x: int, level_y: int, tile_x: int,
                             tile_y: int) -> bytes:
        out = np.empty(SPECTROGRAM_TILE_MAX_BYTES, np.uint8)
        n = C.c_size_t()
        check(lib.th_tm_get_spectrogram_tile(self.handle, track_id, ch, level_x, level_y, tile_x, tile_y,
                                             _ptr(out, c_u8p), out.size, C.byref(n)))
        return out[: n.value].tobytes()

    def get_spectrogram_tiles(self, requests, pinned: bool = False):
        """th_tm_get_spectrogram_tiles: requests = iterable of (track_id, ch, level_x, level_y, tile_x, tile_y); returns the
        list of tile byte strings (each equal to get_spectrogram_tile's).  pinned: the output buffer is pinned host memory
        (th_host_alloc), which the raster kernel writes directly; else a pageable numpy buffer (staged + copied)."""
        reqs = list(requests)
        n = len(reqs)
        arr = (_ffi.TileRequest * max(n, 1))(*[_ffi.TileRequest(*r, 0) for r in reqs])
        offs = (C.c_size_t * (n + 1))()
        need = C.c_size_t()
        rc = lib.th_tm_get_spectrogram_tiles(self.handle, arr, n, None, 0, offs, C.byref(need))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        if n == 0 or need.value == 0:
            return []
        if pinned:
            # a pooled pinned buffer for the duration of this call (a hipHostMalloc / hipHostFree pair per call
            # costs milliseconds, most of what the direct write saves; ADVICE r4: never shared by two calls in flight)
            cap, pin = self._pin_checkout(need.value)
            try:
                check(lib.th_tm_get_spectrogram_tiles(self.handle, arr, n, pin, cap, offs, C.byref(need)))
                out = bytes((C.c_uint8 * need.value).from_address(pin.value))
            finally:
                self._pin_return(cap, pin)
        else:
            b = np.empty(need.value, np.uint8)
            check(lib.th_tm_get_spectrogram_tiles(self.handle, arr, n, b.ctypes.data_as(C.c_void_p), b.size, offs, C.byref(need)))
            out = b.tobytes()
        tiles = []
        for i in range(n):
            w, h = struct.unpack_from("<II", out, offs[i] + 8)
            tiles.append(out[offs[i]: offs[i] + 40 + 4 * w * h])
        return tiles

    def set_lod_source(self, per_request: bool) -> None:
        """LOD > 0 tiles from the resident mip pyramid (False, default) or resampled per request (True)."""
        check(lib.th_tm_set_lod_source(self.handle, int(per_request)))

    def mip_level(self, track_id: int, ch: int, level_x: int, level_y: int) -> np.ndarray:
        """Dense copy of one resident level of the channel's LOD mip pyramid ((0, 0): the image itself)."""
        w, h = C.c_size_t(), C.c_size_t()
        check(lib.th_tm_mip_level(self.handle, track_id, ch, level_x, level_y, None, 0, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value), np.uint16)
        check(lib.th_tm_mip_level(self.handle, track_id, ch, level_x, level_y, _ptr(out, c_u16p), out.size, C.byref(w),
                                  C.byref(h)))
        return out

    def put_img(self, track_id: int, ch: int, img: np.ndarray) -> None:
        """Replace the pixels of a resident u16 image (same shape) and rebuild its mip pyramid (th_tm_put_img)."""
        img = np.ascontiguousarray(img, dtype=np.uint16)
        check(lib.th_tm_put_img(self.handle, track_id, ch, _ptr(img, c_u16p), img.shape[0], img.shape[1]))

    def lod_footprint(self) -> dict:
        """device memory of the LOD machinery: tap tables (count, bytes) and mip pyramids (bytes)"""
        n, ab, mb = C.c_size_t(), C.c_size_t(), C.c_size_t()
        check(lib.th_tm_lod_footprint(self.handle, C.byref(n), C.byref(ab), C.byref(mb)))
        return {"axis_tables": n.value, "axis_table_bytes": ab.value, "mip_bytes": mb.value}

    def render_metadata(self, track_id: int, ch: int, track_sec: float, is_clipped: bool) -> dict:
        """AudioRenderMetadata of get_audio_render_metadata (lib.rs:321-340)."""
        m = _ffi.RenderMetadata()
        check(lib.th_tm_get_audio_render_metadata(self.handle, track_id, ch, track_sec, int(is_clipped), C.byref(m)))
        return {k: getattr(m, k) for k, _ in m._fields_}

    def audio_stats(self, track_id: int) -> dict:
        """AudioStats of a resident track (get_global_lufs / get_rms_dB / get_max_peak_dB, lib.rs:463-489)."""
        o = _ffi.AudioStats()
        check(lib.th_tm_get_audio_stats(self.handle, track_id, C.byref(o)))
        return _audio_stats_dict(o)

    def tile_cache(self) -> TileCache:
        """The RenderTileCache in front of get_waveform_tile (borrowed; owned by the manager)."""
        h = vp()
        check(lib.th_tm_tile_cache(self.handle, C.byref(h)))
        return TileCache(_borrowed=h)

    def get_waveform_tile(self, track_id: int, ch: int, level: int, tile_index: int) -> bytes:
        out = np.empty(WAVEFORM_TILE_MAX_BYTES, np.uint8)
        n = C.c_size_t()
        check(lib.th_tm_get_waveform_tile(self.handle, track_id, ch, level, tile_index, _ptr(out, c_u8p), out.size,
                                          C.byref(n)))
        return out[: n.value].tobytes()


class MultiTrackManager(_DynamicsMethods, _SpectrumMethods, _LoudnessMeterMethods, _ExportMethods, _ExportAtMethods, _ExportBandMethods, _FigureMethods, _EnvelopeMethods, _FormantMethods, _AlignMethods):
    """th_tmg: the TrackManager over several devices of one process (duplicates allowed: [0, 0] is two slots on one card).
    Same method names as TrackManager; results are bit-identical to one TrackManager holding every track."""
    _PFX = "th_tmg_"

    def __init__(self, devices):
        devs = [int(d) for d in devices]
        arr = (C.c_int * max(len(devs), 1))(*devs)
        h = vp()
        check(lib.th_tmg_create(arr, len(devs), C.byref(h)))
        self.handle, self.devices = h, devs
        self._pin_ctx = None  # a context of devices[0], made on the first pinned tile batch (th_host_alloc needs one)
        self._pin_free, self._pin_all, self._pin_lock = [], {}, threading.Lock()

    PIN_POOL_MAX = TrackManager.PIN_POOL_MAX
    _pin_checkout = TrackManager._pin_checkout  # (the same pool of pinned output buffers, allocated through self.ctx)
    _pin_return = TrackManager._pin_return

    @property
    def ctx(self) -> Context:
        with self._pin_lock:
            if self._pin_ctx is None:
                self._pin_ctx = Context(self.devices[0])
            return self._pin_ctx

    @property
    def n_devices(self) -> int:
        n = C.c_size_t()
        check(lib.th_tmg_n_devices(self.handle, C.byref(n)))
        return n.value

    def device_of(self, track_id: int) -> int:
        """The slot (index into `devices`) that owns the track."""
        s = C.c_uint32()
        check(lib.th_tmg_track_device(self.handle, track_id, C.byref(s)))
        return s.value

    def close(self):
        if self.handle:
            if self._pin_ctx is not None:
                TrackManager._free_pinned(self)
            check(lib.th_tmg_destroy(self.handle))
            self.handle = None
            if self._pin_ctx is not None:
                self._pin_ctx.close()
                self._pin_ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_colormap(self, rgba: bytes):
        a = np.frombuffer(bytes(rgba), np.uint8)
        check(lib.th_tmg_set_colormap(self.handle, _ptr(a, c_u8p), a.size))

    def set_setting(self, win_ms: float, t_overlap: int, f_overlap: int, freq_scale: int):
        check(lib.th_tmg_set_setting(self.handle, win_ms, t_overlap, f_overlap, freq_scale))

    def set_dB_range(self, dB_range: float):
        check(lib.th_tmg_set_dB_range(self.handle, dB_range))

    def add_tracks(self, tracks):
        """tracks: iterable of (id, sr, planar ndarray [channels, samples])."""
        tracks = [(i, sr, np.atleast_2d(_f32(w))) for i, sr, w in tracks]
        n = len(tracks)
        ids = (C.c_size_t * n)(*[t[0] for t in tracks])
        srs = (C.c_uint32 * n)(*[t[1] for t in tracks])
        nch = (C.c_uint32 * n)(*[t[2].shape[0] for t in tracks])
        ns = (C.c_size_t * n)(*[t[2].shape[1] for t in tracks])
        rows = [np.ascontiguousarray(t[2][c]) for t in tracks for c in range(t[2].shape[0])]
        ptrs = (c_f32p * len(rows))(*[_ptr(r, c_f32p) for r in rows])
        check(lib.th_tmg_add_tracks(self.handle, n, ids, srs, nch, ptrs, ns))

    def remove_track(self, track_id: int):
        check(lib.th_tmg_remove_track(self.handle, track_id))

    def apply_track_list_changes(self):
        cap = 4096
        ids = (C.c_size_t * cap)()
        n, sr = C.c_size_t(), C.c_uint32()
        check(lib.th_tmg_apply_track_list_changes(self.handle, ids, cap, C.byref(n), C.byref(sr)))
        return sorted(ids[i] for i in range(min(n.value, cap))), sr.value

    def db_state(self):
        lo, hi, sr = C.c_float(), C.c_float(), C.c_uint32()
        check(lib.th_tmg_get_db_state(self.handle, C.byref(lo), C.byref(hi), C.byref(sr)))
        return lo.value, hi.value, sr.value

    def revisions(self):
        w, s = C.c_uint64(), C.c_uint64()
        check(lib.th_tmg_revisions(self.handle, C.byref(w), C.byref(s)))
        return w.value, s.value

    def spec(self, track_id: int, ch: int) -> np.ndarray:
        t, h = C.c_size_t(), C.c_size_t()
        check(lib.th_tmg_spec_shape(self.handle, track_id, ch, C.byref(t), C.byref(h)))
        out = np.empty((t.value, h.value), np.float32)
        check(lib.th_tmg_copy_spec(self.handle, track_id, ch, _ptr(out, c_f32p), out.size))
        return out

    def img(self, track_id: int, ch: int) -> np.ndarray:
        h, w = C.c_size_t(), C.c_size_t()
        check(lib.th_tmg_img_shape(self.handle, track_id, ch, C.byref(h), C.byref(w)))
        out = np.empty((h.value, w.value), np.uint16)
        check(lib.th_tmg_copy_img(self.handle, track_id, ch, _ptr(out, c_u16p), out.size))
        return out

    def get_spectrogram_tile(self, track_id: int, ch: int, level_x: int, level_y: int, tile_x: int,
                             tile_y: int) -> bytes:
        out = np.empty(SPECTROGRAM_TILE_MAX_BYTES, np.uint8)
        n = C.c_size_t()
        check(lib.th_tmg_get_spectrogram_tile(self.handle, track_id, ch, level_x, level_y, tile_x, tile_y,
                                              _ptr(out, c_u8p), out.size, C.byref(n)))
        return out[: n.value].tobytes()

    def get_spectrogram_tiles(self, requests, pinned: bool = False):
        """As TrackManager.get_spectrogram_tiles (th_tmg_get_spectrogram_tiles)."""
        reqs = list(requests)
        n = len(reqs)
        arr = (_ffi.TileRequest * max(n, 1))(*[_ffi.TileRequest(*r, 0) for r in reqs])
        offs = (C.c_size_t * (n + 1))()
        need = C.c_size_t()
        rc = lib.th_tmg_get_spectrogram_tiles(self.handle, arr, n, None, 0, offs, C.byref(need))
        if rc not in (_ffi.OK, _ffi.ERR_BUFFER_TOO_SMALL):
            check(rc)
        if n == 0 or need.value == 0:
            return []
        if pinned:
            cap, pin = self._pin_checkout(need.value)
            try:
                check(lib.th_tmg_get_spectrogram_tiles(self.handle, arr, n, pin, cap, offs, C.byref(need)))
                out = bytes((C.c_uint8 * need.value).from_address(pin.value))
            finally:
                self._pin_return(cap, pin)
        else:
            b = np.empty(need.value, np.uint8)
            check(lib.th_tmg_get_spectrogram_tiles(self.handle, arr, n, b.ctypes.data_as(C.c_void_p), b.size, offs,
                                                   C.byref(need)))
            out = b.tobytes()
        tiles = []
        for i in range(n):
            w, h = struct.unpack_from("<II", out, offs[i] + 8)
            tiles.append(out[offs[i]: offs[i] + 40 + 4 * w * h])
        return tiles

    def set_lod_source(self, per_request: bool) -> None:
        check(lib.th_tmg_set_lod_source(self.handle, int(per_request)))

    def audio_stats(self, track_id: int) -> dict:
        o = _ffi.AudioStats()
        check(lib.th_tmg_get_audio_stats(self.handle, track_id, C.byref(o)))
        return _audio_stats_dict(o)

    def render_metadata(self, track_id: int, ch: int, track_sec: float, is_clipped: bool) -> dict:
        m = _ffi.RenderMetadata()
        check(lib.th_tmg_get_audio_render_metadata(self.handle, track_id, ch, track_sec, int(is_clipped), C.byref(m)))
        return {k: getattr(m, k) for k, _ in m._fields_}

    def get_waveform_tile(self, track_id: int, ch: int, level: int, tile_index: int) -> bytes:
        out = np.empty(WAVEFORM_TILE_MAX_BYTES, np.uint8)
        n = C.c_size_t()
        check(lib.th_tmg_get_waveform_tile(self.handle, track_id, ch, level, tile_index, _ptr(out, c_u8p), out.size,
                                           C.byref(n)))
        return out[: n.value].tobytes()
