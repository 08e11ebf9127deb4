"""ctypes binding of libthesia_amd.so (the C ABI declared in include/thesia_amd.h).

The shared library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  Importing
this module fails loudly when it is missing: there is no CPU fallback of any kind.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# THESIA_AMD_LIB: development override to A/B a variant build of the same library (scripts/build_variant.sh)
LIB_PATH = os.environ.get("THESIA_AMD_LIB") or os.path.join(_HERE, "libthesia_amd.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build the HIP extension first "
        "(python -c 'import __graft_entry__ as g; g.build()').  thesia_amd has no CPU fallback."
    )



def _preload_hip_runtime() -> None:
    """One HIP runtime per process.  libthesia_amd.so needs `libamdhip64.so.7` by soname; PyTorch
    wheels bundle their own copy under torch/lib with that same soname.  If torch is (or may later
    be) in the process, load torch's copy first so the dynamic loader resolves our NEEDED entry to
    it instead of mapping /opt/rocm's as a second runtime (two runtimes = "no device" in the second).
    THESIA_AMD_SYSTEM_HIP=1 keeps the system runtime (pure C hosts, no torch)."""
    if "torch" in sys.modules or os.environ.get("THESIA_AMD_SYSTEM_HIP") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


_preload_hip_runtime()
lib = C.CDLL(LIB_PATH)

c_f32p = C.POINTER(C.c_float)
c_u8p = C.POINTER(C.c_uint8)
c_u16p = C.POINTER(C.c_uint16)
c_szp = C.POINTER(C.c_size_t)
vp = C.c_void_p


class ThError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"thesia_amd error {code}: {msg}")
        self.code = code


OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_NO_DEVICE, ERR_OOM, ERR_BUFFER_TOO_SMALL, ERR_NOT_FOUND, \
    ERR_INTERNAL = 0, -1, -2, -3, -4, -5, -6, -7, -8


class TileRequest(C.Structure):
    _fields_ = [("id", C.c_size_t), ("ch", C.c_uint32), ("level_x", C.c_uint32), ("level_y", C.c_uint32),
                ("tile_x", C.c_uint32), ("tile_y", C.c_uint32), ("reserved", C.c_uint32)]


class StatsDesc(C.Structure):
    _fields_ = [("wav", C.c_void_p), ("n_samples", C.c_uint64)]


class AudioStats(C.Structure):  # th_audio_stats
    _fields_ = [("global_lufs", C.c_double), ("rms_dB", C.c_float), ("max_peak", C.c_float), ("max_peak_dB", C.c_float),
                ("reserved", C.c_uint32 * 3)]


class AudioDesc(C.Structure):  # th_audio_desc
    _fields_ = [("channels", C.POINTER(C.c_void_p)), ("n_samples", C.c_uint64), ("n_channels", C.c_uint32), ("sr", C.c_uint32),
                ("block_energy", C.c_void_p)]


class LimiterDesc(C.Structure):  # th_limiter_desc
    _fields_ = [("attack", C.c_uint32), ("hold_length", C.c_uint32), ("release_samples", C.c_double), ("box_len", C.c_uint32 * 3),
                ("reserved", C.c_uint32)]


class TrackDynamics(C.Structure):  # th_track_dynamics
    _fields_ = [("normalize_gain", C.c_float), ("guard_result", C.c_int32), ("global_gain", C.c_float),
                ("draws_before_clip", C.c_uint32)]


class GuardClipStats(C.Structure):  # th_guard_clip_stats
    _fields_ = [("max_reduction_gain_dB", C.c_float), ("reserved", C.c_uint32), ("reduction_cnt", C.c_uint64)]


class SpectrumRequest(C.Structure):  # th_spectrum_request
    _fields_ = [("id", C.c_size_t), ("ch", C.c_uint32), ("kind", C.c_uint32), ("start_sec", C.c_double), ("end_sec", C.c_double)]


class SpectrumInfo(C.Structure):  # th_spectrum_info
    _fields_ = [("offset", C.c_uint64), ("height", C.c_uint64), ("frame_start", C.c_uint64), ("frame_end", C.c_uint64),
                ("spectrogram_revision", C.c_uint64)]


class LoudnessMeter(C.Structure):  # th_loudness_meter
    _fields_ = [("loudness_range", C.c_double), ("max_momentary_lufs", C.c_double), ("max_short_term_lufs", C.c_double),
                ("true_peak", C.c_float), ("true_peak_dB", C.c_float), ("true_peak_channel", C.c_uint32), ("oversampling", C.c_uint32),
                ("momentary_offset", C.c_uint64), ("n_momentary", C.c_uint64), ("short_term_offset", C.c_uint64),
                ("n_short_term", C.c_uint64), ("waveform_revision", C.c_uint64)]


class ExportRequest(C.Structure):  # th_export_request
    _fields_ = [("id", C.c_size_t), ("which", C.c_uint32), ("format", C.c_uint32), ("dither", C.c_uint32), ("seed", C.c_uint32),
                ("start_sec", C.c_double), ("end_sec", C.c_double)]


class ExportInfo(C.Structure):  # th_export_info
    _fields_ = [("offset", C.c_uint64), ("n_bytes", C.c_uint64), ("sample_start", C.c_uint64), ("sample_end", C.c_uint64),
                ("sr", C.c_uint32), ("n_channels", C.c_uint32), ("n_clamped", C.c_uint64), ("n_nan", C.c_uint64),
                ("waveform_revision", C.c_uint64)]


class ResamplePlan(C.Structure):  # th_resample_plan
    _fields_ = [("L", C.c_uint32), ("M", C.c_uint32), ("half_taps", C.c_uint32), ("rho", C.c_double), ("cutoff", C.c_double)]


class ExportAtRequest(C.Structure):  # th_export_at_request
    _fields_ = [("base", ExportRequest), ("sr_out", C.c_uint32)]


class ExportBandRequest(C.Structure):  # th_export_band_request
    _fields_ = [("base", ExportRequest), ("mode", C.c_uint32), ("f_lo_hz", C.c_double), ("f_hi_hz", C.c_double), ("trans_hz", C.c_double)]


class BandPlan(C.Structure):  # th_band_plan
    _fields_ = [("half_taps", C.c_uint32), ("mode", C.c_uint32), ("f_lo_hz", C.c_double), ("f_hi_hz", C.c_double), ("trans_hz", C.c_double)]


class FigureRequest(C.Structure):  # th_figure_request
    _fields_ = [("id", C.c_size_t), ("ch", C.c_uint32), ("kind", C.c_uint32), ("out_w", C.c_uint32), ("out_h", C.c_uint32),
                ("left", C.c_double), ("top", C.c_double), ("width", C.c_double), ("height", C.c_double)]


class FigureInfo(C.Structure):  # th_figure_info
    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint64), ("out_w", C.c_uint32), ("out_h", C.c_uint32),
                ("spectrogram_revision", C.c_uint64)]


class EnvelopeRequest(C.Structure):  # th_envelope_request
    _fields_ = [("id", C.c_size_t), ("ch", C.c_uint32), ("which", C.c_uint32), ("start_sec", C.c_double), ("end_sec", C.c_double),
                ("n_cols", C.c_uint32), ("reserved", C.c_uint32)]


class EnvelopeInfo(C.Structure):  # th_envelope_info
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint64), ("sample_start", C.c_uint64), ("sample_end", C.c_uint64),
                ("waveform_revision", C.c_uint64)]


class ResamplePlanC(C.Structure):  # th_resample_plan (as a member of th_formant_plan)
    _fields_ = [("L", C.c_uint32), ("M", C.c_uint32), ("half_taps", C.c_uint32), ("rho", C.c_double), ("cutoff", C.c_double)]


class FormantRequest(C.Structure):  # th_formant_request
    _fields_ = [("id", C.c_size_t), ("ch", C.c_uint32), ("which", C.c_uint32), ("start_sec", C.c_double), ("end_sec", C.c_double),
                ("sr_analysis", C.c_uint32), ("n_poles", C.c_uint32), ("win_sec", C.c_double), ("step_sec", C.c_double),
                ("preemph_hz", C.c_double), ("window", C.c_uint32), ("kind", C.c_uint32)]


class FormantPlan(C.Structure):  # th_formant_plan
    _fields_ = [("sr", C.c_uint32), ("sr_analysis", C.c_uint32), ("resampled", C.c_uint32), ("n_poles", C.c_uint32), ("win", C.c_uint32),
                ("hop", C.c_uint32), ("window", C.c_uint32), ("kind", C.c_uint32), ("rs", ResamplePlanC), ("n_analysis", C.c_uint64),
                ("n_frames_total", C.c_uint64), ("frame_first", C.c_uint64), ("frame_end", C.c_uint64), ("alpha", C.c_double)]


class FormantInfo(C.Structure):  # th_formant_info
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint64), ("frame_first", C.c_uint64), ("frame_end", C.c_uint64),
                ("sr_analysis", C.c_uint32), ("win", C.c_uint32), ("hop", C.c_uint32), ("reserved", C.c_uint32),
                ("n_invalid", C.c_uint64), ("n_unconverged", C.c_uint64), ("waveform_revision", C.c_uint64)]


class AlignRequest(C.Structure):  # th_align_request
    _fields_ = [("ref_id", C.c_size_t), ("ref_ch", C.c_uint32), ("ref_which", C.c_uint32), ("id", C.c_size_t), ("ch", C.c_uint32),
                ("which", C.c_uint32), ("start_sec", C.c_double), ("end_sec", C.c_double), ("max_lag_sec", C.c_double),
                ("kind", C.c_uint32), ("flags", C.c_uint32)]


class AlignPlan(C.Structure):  # th_align_plan
    _fields_ = [("sr", C.c_uint32), ("max_lag", C.c_uint32), ("kind", C.c_uint32), ("flags", C.c_uint32), ("sample_start", C.c_uint64),
                ("sample_end", C.c_uint64), ("n_lags", C.c_uint64), ("length", C.c_uint64)]


class AlignInfo(C.Structure):  # th_align_info
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint64), ("sr", C.c_uint32), ("max_lag", C.c_uint32), ("sample_start", C.c_uint64),
                ("sample_end", C.c_uint64), ("waveform_revision", C.c_uint64)]


class WaveformFigureRequest(C.Structure):  # th_waveform_figure_request
    _fields_ = [("env", EnvelopeRequest), ("out_h", C.c_uint32), ("amp_lo", C.c_float), ("amp_hi", C.c_float), ("thickness", C.c_uint32),
                ("fill", C.c_uint8 * 4), ("background", C.c_uint8 * 4)]


class WaveformFigureInfo(C.Structure):  # th_waveform_figure_info
    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint64), ("out_w", C.c_uint32), ("out_h", C.c_uint32),
                ("sample_start", C.c_uint64), ("sample_end", C.c_uint64), ("waveform_revision", C.c_uint64)]


class PyramidDesc(C.Structure):
    _fields_ = [("wav", C.c_void_p), ("out", C.c_void_p), ("n_samples", C.c_uint64), ("n_levels", C.c_uint32),
                ("first_level", C.c_uint32)]


class RenderMetadata(C.Structure):
    _fields_ = [("waveform_revision", C.c_uint64), ("spectrogram_revision", C.c_uint64), ("sample_rate", C.c_uint32),
                ("is_clipped", C.c_uint32), ("sample_count", C.c_uint64), ("track_sec", C.c_double),
                ("spectrogram_width", C.c_uint64), ("spectrogram_height", C.c_uint64), ("waveform_tile_bins", C.c_uint64),
                ("spectrogram_tile_size", C.c_uint64)]


class TileGeom(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("origin_x", C.c_uint32), ("origin_y", C.c_uint32),
                ("lod_width", C.c_uint64), ("lod_height", C.c_uint64)]


class ChanDesc(C.Structure):
    _fields_ = [("wav", vp), ("spec", vp), ("n_samples", C.c_uint64), ("n_frames", C.c_uint64),
                ("spec_pitch", C.c_uint64)]


class ImgDesc(C.Structure):
    _fields_ = [("spec", vp), ("img", vp), ("n_frames", C.c_uint64), ("height", C.c_uint64),
                ("i_start", C.c_uint64), ("i_end", C.c_uint64), ("spec_pitch", C.c_uint64), ("img_pitch", C.c_uint64)]


class RasterDesc(C.Structure):
    _fields_ = [("img", vp), ("rgba", vp), ("img_width", C.c_uint32), ("img_height", C.c_uint32),
                ("origin_x", C.c_uint32), ("origin_y", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("img_pitch", C.c_uint32), ("reserved", C.c_uint32)]


class ImgTilesDesc(C.Structure):  # th_img_tiles_desc
    _fields_ = [("img", ImgDesc), ("tiles", C.POINTER(vp)), ("n_tiles_x", C.c_uint32), ("n_tiles_y", C.c_uint32)]


class WaveDesc(C.Structure):
    _fields_ = [("wav", vp), ("bins", vp), ("n_samples", C.c_uint64), ("start", C.c_uint64),
                ("level", C.c_uint32), ("bin_count", C.c_uint32)]


# name -> argtypes (restype is int unless listed in _RESTYPES).  Keep in sync with include/thesia_amd.h;
# tests/test_abi.py checks that every TH_API symbol of the header is exported and declared here.
_SIGS = {
    "th_version": [],
    "th_device_count": [C.POINTER(C.c_int)],
    "th_calc_framing_params": [C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, c_szp, c_szp, c_szp],
    "th_stft_n_frames": [C.c_size_t, C.c_size_t, C.c_size_t, c_szp],
    "th_calc_normalized_win": [C.c_size_t, C.c_size_t, c_f32p],
    "th_calc_mel_fb": [C.c_uint32, C.c_size_t, C.c_size_t, C.c_float, C.c_float, C.c_int, c_f32p],
    "th_mel_default_n_mel": [C.c_uint32, C.c_size_t, c_szp],
    "th_hz_range_to_idx": [C.c_int, C.c_float, C.c_float, C.c_uint32, C.c_size_t, c_szp, c_szp],
    "th_global_db_range": [c_f32p, c_f32p, C.c_size_t, C.c_float, c_f32p, c_f32p],
    "th_shard_assign": [C.POINTER(C.c_uint64), C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32)],
    "th_spectrogram_tile_geometry": [C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.POINTER(TileGeom)],
    "th_waveform_tile_geometry": [C.c_size_t, C.c_uint32, C.c_uint32, c_szp, c_szp, c_szp],
    "th_ctx_create": [C.c_int, vp, C.POINTER(vp)],
    "th_ctx_create_ex": [C.c_int, vp, C.c_int, C.POINTER(vp)],
    "th_ctx_destroy": [vp],
    "th_ctx_synchronize": [vp],
    "th_ctx_capture_begin": [vp],
    "th_ctx_capture_end": [vp, C.POINTER(vp)],
    "th_graph_launch": [vp],
    "th_graph_destroy": [vp],
    "th_dev_alloc": [vp, C.c_size_t, C.POINTER(vp)],
    "th_dev_free": [vp, vp],
    "th_dev_upload": [vp, vp, vp, C.c_size_t],
    "th_dev_download": [vp, vp, vp, C.c_size_t],
    "th_dev_copy": [vp, vp, vp, C.c_size_t],
    "th_timer_start": [vp],
    "th_timer_stop_ms": [vp, c_f32p],
    "th_plan_create": [vp, C.c_uint32, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.POINTER(vp)],
    "th_plan_destroy": [vp],
    "th_plan_dims": [vp, c_szp, c_szp],
    "th_plan_set_kernel": [vp, C.c_int],
    "th_build_ab_variants": [],
    "th_plan_mel_moments_info": [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "th_plan_kernel_name": [vp],
    "th_calc_spec_batch_dev": [vp, C.POINTER(ChanDesc), C.c_size_t, vp],
    "th_calc_spec_batch_ranged_dev": [vp, C.POINTER(ChanDesc), C.c_size_t, vp, C.c_float, vp],
    "th_calc_spec_host": [vp, c_f32p, C.c_size_t, c_f32p, C.c_size_t, c_szp, c_f32p, c_f32p],
    "th_spec_to_img_dev": [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_float, C.c_float,
                           C.c_uint32, vp],
    "th_spec_to_img_batch_dev": [vp, C.POINTER(ImgDesc), C.c_size_t, C.c_float, C.c_float, C.c_uint32],
    "th_pitch_f32": [C.c_size_t],
    "th_pitch_u16": [C.c_size_t],
    "th_encode_spectrogram_tile_dev": [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, c_u8p, C.c_size_t, C.c_uint64, C.c_uint32,
                                       C.c_uint32, C.c_uint32, C.c_uint32, c_u8p, C.c_size_t, c_szp],
    "th_raster_tiles_dev": [vp, C.POINTER(RasterDesc), C.c_size_t, vp, C.c_uint32],
    "th_spec_to_img_raster_batch_dev": [vp, C.POINTER(ImgTilesDesc), C.c_size_t, C.c_float, C.c_float, C.c_void_p, vp, C.c_uint32],
    "th_encode_waveform_tile_dev": [vp, vp, C.c_size_t, C.c_uint64, C.c_uint32, C.c_uint32, c_u8p, C.c_size_t,
                                    c_szp],
    "th_waveform_tiles_dev": [vp, C.POINTER(WaveDesc), C.c_size_t],
    "th_tm_create": [vp, C.POINTER(vp)],
    "th_tm_destroy": [vp],
    "th_tm_set_colormap": [vp, c_u8p, C.c_size_t],
    "th_tm_set_setting": [vp, C.c_double, C.c_uint32, C.c_uint32, C.c_int],
    "th_tm_set_dB_range": [vp, C.c_float],
    "th_tm_add_track": [vp, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(c_f32p), C.c_size_t],
    "th_tm_add_tracks": [vp, C.c_size_t, c_szp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(c_f32p),
                         c_szp],
    "th_tm_remove_track": [vp, C.c_size_t],
    "th_tm_apply_track_list_changes": [vp, c_szp, C.c_size_t, c_szp, C.POINTER(C.c_uint32)],
    "th_tm_get_db_state": [vp, c_f32p, c_f32p, C.POINTER(C.c_uint32)],
    "th_tm_spec_shape": [vp, C.c_size_t, C.c_uint32, c_szp, c_szp],
    "th_tm_img_shape": [vp, C.c_size_t, C.c_uint32, c_szp, c_szp],
    "th_tm_copy_spec": [vp, C.c_size_t, C.c_uint32, c_f32p, C.c_size_t],
    "th_tm_copy_img": [vp, C.c_size_t, C.c_uint32, c_u16p, C.c_size_t],
    "th_tm_revisions": [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "th_tm_get_spectrogram_tile": [vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                   c_u8p, C.c_size_t, c_szp],
    "th_tm_get_waveform_tile": [vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, c_u8p, C.c_size_t, c_szp],
    "th_tm_get_spectrogram_tiles": [vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, c_szp, c_szp],
    "th_host_alloc": [vp, C.c_size_t, C.POINTER(C.c_void_p)],
    "th_host_free": [vp, C.c_void_p],
    "th_minmax_reduce_dev": [vp, C.c_void_p, C.c_size_t, C.c_void_p],
    "th_global_db_range_dev": [vp, C.c_void_p, C.c_float, C.c_void_p],
    "th_minmax_reduce_range_dev": [vp, vp, C.c_size_t, C.c_float, vp, vp],
    "th_spec_to_img_batch_dev_ranged": [vp, C.POINTER(ImgDesc), C.c_size_t, C.c_void_p, C.c_uint32],
    "th_plan_time_kernel": [vp, C.c_int],
    "th_plan_last_kernel_ms": [vp, C.POINTER(C.c_float)],
    "th_plan_kernel_ms_history": [vp, c_f32p, C.c_size_t, c_szp],
    "th_channel_stats_dev": [vp, C.POINTER(StatsDesc), C.c_size_t, c_f32p, c_f32p],
    "th_audio_stats_dev": [vp, C.POINTER(AudioDesc), C.c_size_t, C.POINTER(AudioStats)],
    "th_k_weighting": [C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "th_loudness_n_blocks": [C.c_size_t, C.c_uint32, c_szp],
    "th_gated_loudness": [C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_double)],
    "th_tm_get_audio_stats": [vp, C.c_size_t, C.POINTER(AudioStats)],
    "th_tmg_get_audio_stats": [vp, C.c_size_t, C.POINTER(AudioStats)],
    "th_waveform_pyramid_bins": [C.c_uint64, C.c_uint32],
    "th_waveform_pyramid_offset": [C.c_uint64, C.c_uint32],
    "th_waveform_pyramid_dev": [vp, C.POINTER(PyramidDesc), C.c_size_t],
    "th_tm_tile_cache": [vp, C.POINTER(vp)],
    "th_tm_set_lod_source": [vp, C.c_int],
    "th_tm_mip_level": [vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, c_u16p, C.c_size_t, c_szp, c_szp],
    "th_tm_put_img": [vp, C.c_size_t, C.c_uint32, c_u16p, C.c_size_t, C.c_size_t],
    "th_tm_lod_footprint": [vp, c_szp, c_szp, c_szp],
    "th_tm_get_audio_render_metadata": [vp, C.c_size_t, C.c_uint32, C.c_double, C.c_int, C.POINTER(RenderMetadata)],
    "th_tmg_create": [C.POINTER(C.c_int), C.c_size_t, C.POINTER(vp)],
    "th_tmg_destroy": [vp],
    "th_tmg_n_devices": [vp, c_szp],
    "th_tmg_track_device": [vp, C.c_size_t, C.POINTER(C.c_uint32)],
    "th_tmg_set_colormap": [vp, c_u8p, C.c_size_t],
    "th_tmg_set_setting": [vp, C.c_double, C.c_uint32, C.c_uint32, C.c_int],
    "th_tmg_set_dB_range": [vp, C.c_float],
    "th_tmg_add_tracks": [vp, C.c_size_t, c_szp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(c_f32p),
                          c_szp],
    "th_tmg_remove_track": [vp, C.c_size_t],
    "th_tmg_apply_track_list_changes": [vp, c_szp, C.c_size_t, c_szp, C.POINTER(C.c_uint32)],
    "th_tmg_get_db_state": [vp, c_f32p, c_f32p, C.POINTER(C.c_uint32)],
    "th_tmg_spec_shape": [vp, C.c_size_t, C.c_uint32, c_szp, c_szp],
    "th_tmg_img_shape": [vp, C.c_size_t, C.c_uint32, c_szp, c_szp],
    "th_tmg_copy_spec": [vp, C.c_size_t, C.c_uint32, c_f32p, C.c_size_t],
    "th_tmg_copy_img": [vp, C.c_size_t, C.c_uint32, c_u16p, C.c_size_t],
    "th_tmg_revisions": [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "th_tmg_get_spectrogram_tile": [vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                    c_u8p, C.c_size_t, c_szp],
    "th_tmg_get_spectrogram_tiles": [vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, c_szp, c_szp],
    "th_tmg_get_waveform_tile": [vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, c_u8p, C.c_size_t, c_szp],
    "th_tmg_get_audio_render_metadata": [vp, C.c_size_t, C.c_uint32, C.c_double, C.c_int, C.POINTER(RenderMetadata)],
    "th_tmg_set_lod_source": [vp, C.c_int],
    "th_normalize_gain": [C.c_int, C.c_float, C.POINTER(AudioStats), c_f32p],
    "th_limiter_params": [C.c_uint32, C.POINTER(LimiterDesc)],
    "th_tm_set_common_normalize": [vp, C.c_int, C.c_float],
    "th_tm_set_common_guard_clipping": [vp, C.c_int],
    "th_tm_get_common_dynamics": [vp, C.POINTER(C.c_int), c_f32p, C.POINTER(C.c_int)],
    "th_tm_get_track_dynamics": [vp, C.c_size_t, C.POINTER(TrackDynamics)],
    "th_tm_get_guard_clip_stats": [vp, C.c_size_t, C.POINTER(GuardClipStats), C.c_size_t, c_szp],
    "th_tm_get_limiter_gain": [vp, C.c_size_t, c_f32p, C.c_size_t, c_szp],
    "th_tm_copy_audio": [vp, C.c_size_t, C.c_uint32, C.c_int, c_f32p, C.c_size_t],
    "th_tmg_set_common_normalize": [vp, C.c_int, C.c_float],
    "th_tmg_set_common_guard_clipping": [vp, C.c_int],
    "th_tmg_get_common_dynamics": [vp, C.POINTER(C.c_int), c_f32p, C.POINTER(C.c_int)],
    "th_tmg_get_track_dynamics": [vp, C.c_size_t, C.POINTER(TrackDynamics)],
    "th_tmg_get_guard_clip_stats": [vp, C.c_size_t, C.POINTER(GuardClipStats), C.c_size_t, c_szp],
    "th_tmg_get_limiter_gain": [vp, C.c_size_t, c_f32p, C.c_size_t, c_szp],
    "th_tmg_copy_audio": [vp, C.c_size_t, C.c_uint32, C.c_int, c_f32p, C.c_size_t],
    "th_spectrum_frame_range": [C.c_uint32, C.c_size_t, C.c_size_t, C.c_double, C.c_double, c_szp, c_szp],
    "th_tm_get_spectra": [vp, C.POINTER(SpectrumRequest), C.c_size_t, c_f32p, C.c_size_t, C.POINTER(SpectrumInfo), c_szp],
    "th_tm_get_spectrum": [vp, C.c_size_t, C.c_uint32, C.c_int, C.c_double, C.c_double, c_f32p, C.c_size_t, C.POINTER(SpectrumInfo)],
    "th_tmg_get_spectra": [vp, C.POINTER(SpectrumRequest), C.c_size_t, c_f32p, C.c_size_t, C.POINTER(SpectrumInfo), c_szp],
    "th_tmg_get_spectrum": [vp, C.c_size_t, C.c_uint32, C.c_int, C.c_double, C.c_double, c_f32p, C.c_size_t, C.POINTER(SpectrumInfo)],
    "th_tm_get_loudness_meters": [vp, c_szp, C.c_size_t, C.POINTER(LoudnessMeter), C.POINTER(C.c_double), C.c_size_t, c_szp],
    "th_tm_get_loudness_meter": [vp, C.c_size_t, C.POINTER(LoudnessMeter), C.POINTER(C.c_double), C.c_size_t],
    "th_tmg_get_loudness_meters": [vp, c_szp, C.c_size_t, C.POINTER(LoudnessMeter), C.POINTER(C.c_double), C.c_size_t, c_szp],
    "th_tmg_get_loudness_meter": [vp, C.c_size_t, C.POINTER(LoudnessMeter), C.POINTER(C.c_double), C.c_size_t],
    "th_true_peak_filter": [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                            C.POINTER(C.c_uint32)],
    "th_loudness_n_short_term": [C.c_size_t, C.c_uint32, c_szp],
    "th_loudness_range": [C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_double)],
    "th_audio_sample_range": [C.c_uint32, C.c_size_t, C.c_double, C.c_double, c_szp, c_szp],
    "th_export_dither": [C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "th_export_quantize": [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, c_f32p, C.c_size_t, C.POINTER(C.c_int32),
                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "th_wav_header": [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, c_u8p, c_szp, c_szp],
    "th_tm_export_pcm": [vp, C.POINTER(ExportRequest), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tm_export_wav": [vp, C.POINTER(ExportRequest), C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tmg_export_pcm": [vp, C.POINTER(ExportRequest), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tmg_export_wav": [vp, C.POINTER(ExportRequest), C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_flac_bound": [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)],
    "th_flac_frame_header": [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, c_u8p, c_szp],
    "th_flac_encode_i32": [C.POINTER(C.POINTER(C.c_int32)), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, c_szp],
    "th_flac_encode_i32_ex": [C.POINTER(C.POINTER(C.c_int32)), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, c_szp],
    "th_tm_export_flac_ex": [vp, C.POINTER(ExportRequest), C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tmg_export_flac_ex": [vp, C.POINTER(ExportRequest), C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tm_export_flac": [vp, C.POINTER(ExportRequest), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tmg_export_flac": [vp, C.POINTER(ExportRequest), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_resample_plan_for": [C.c_uint32, C.c_uint32, C.POINTER(ResamplePlan)],
    "th_resample_n_out": [C.c_size_t, C.c_uint32, C.c_uint32, c_szp],
    "th_resample_coefs": [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), c_f32p],
    "th_resample_f32": [c_f32p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64, C.c_size_t, c_f32p],
    "th_tm_export_pcm_at": [vp, C.POINTER(ExportAtRequest), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tm_export_wav_at": [vp, C.POINTER(ExportAtRequest), C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tmg_export_pcm_at": [vp, C.POINTER(ExportAtRequest), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tmg_export_wav_at": [vp, C.POINTER(ExportAtRequest), C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_band_plan_for": [C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double, C.POINTER(BandPlan)],
    "th_band_coefs": [C.c_uint32, C.POINTER(BandPlan), C.POINTER(C.c_double), c_f32p],
    "th_band_response": [C.c_uint32, C.POINTER(BandPlan), C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_double)],
    "th_band_f32": [c_f32p, C.c_size_t, c_f32p, C.c_uint32, C.c_uint64, C.c_size_t, c_f32p],
    "th_tm_export_pcm_band": [vp, C.POINTER(ExportBandRequest), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tm_export_wav_band": [vp, C.POINTER(ExportBandRequest), C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tmg_export_pcm_band": [vp, C.POINTER(ExportBandRequest), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_tmg_export_wav_band": [vp, C.POINTER(ExportBandRequest), C.c_void_p, C.c_size_t, C.POINTER(ExportInfo), c_szp],
    "th_figure_axis": [C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                       C.c_size_t, C.POINTER(C.c_uint32)],
    "th_figure_box": [C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "th_tm_figure_box": [vp, C.c_size_t, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double),
                         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "th_tmg_figure_box": [vp, C.c_size_t, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double),
                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "th_tm_render_figures": [vp, C.POINTER(FigureRequest), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(FigureInfo), c_szp],
    "th_tm_render_figure": [vp, C.POINTER(FigureRequest), C.c_void_p, C.c_size_t, C.POINTER(FigureInfo)],
    "th_tmg_render_figures": [vp, C.POINTER(FigureRequest), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(FigureInfo), c_szp],
    "th_tmg_render_figure": [vp, C.POINTER(FigureRequest), C.c_void_p, C.c_size_t, C.POINTER(FigureInfo)],
    "th_envelope_edges": [C.c_uint32, C.c_size_t, C.c_double, C.c_double, C.c_uint32, C.POINTER(C.c_uint64)],
    "th_waveform_figure_span": [c_f32p, c_f32p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                C.POINTER(C.c_int)],
    "th_tm_get_envelopes": [vp, C.POINTER(EnvelopeRequest), C.c_size_t, c_f32p, C.c_size_t, C.POINTER(EnvelopeInfo), c_szp],
    "th_tm_get_envelope": [vp, C.POINTER(EnvelopeRequest), c_f32p, C.c_size_t, C.POINTER(EnvelopeInfo)],
    "th_tmg_get_envelopes": [vp, C.POINTER(EnvelopeRequest), C.c_size_t, c_f32p, C.c_size_t, C.POINTER(EnvelopeInfo), c_szp],
    "th_tmg_get_envelope": [vp, C.POINTER(EnvelopeRequest), c_f32p, C.c_size_t, C.POINTER(EnvelopeInfo)],
    "th_formant_defaults": [C.POINTER(FormantRequest)],
    "th_formant_plan_for": [C.c_uint32, C.c_size_t, C.POINTER(FormantRequest), C.POINTER(FormantPlan)],
    "th_formant_window": [C.c_uint32, C.c_uint32, C.POINTER(C.c_double)],
    "th_formant_start_points": [C.c_uint32, C.POINTER(C.c_double)],
    "th_formants_f64": [c_f32p, C.c_size_t, C.c_uint32, C.POINTER(FormantRequest), C.c_uint64, C.c_size_t, C.POINTER(C.c_double),
                        C.POINTER(C.c_uint64)],
    "th_formant_frame_f64": [c_f32p, C.c_size_t, C.c_uint32, C.POINTER(FormantRequest), C.c_uint64, C.POINTER(C.c_double),
                             C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                             C.POINTER(C.c_uint32)],
    "th_tm_get_formants": [vp, C.POINTER(FormantRequest), C.c_size_t, C.POINTER(C.c_double), C.c_size_t, C.POINTER(FormantInfo), c_szp],
    "th_tm_get_formant_track": [vp, C.POINTER(FormantRequest), C.POINTER(C.c_double), C.c_size_t, C.POINTER(FormantInfo)],
    "th_tmg_get_formants": [vp, C.POINTER(FormantRequest), C.c_size_t, C.POINTER(C.c_double), C.c_size_t, C.POINTER(FormantInfo), c_szp],
    "th_tmg_get_formant_track": [vp, C.POINTER(FormantRequest), C.POINTER(C.c_double), C.c_size_t, C.POINTER(FormantInfo)],
    "th_align_plan_for": [C.c_uint32, C.c_size_t, C.c_uint32, C.c_size_t, C.POINTER(AlignRequest), C.POINTER(AlignPlan)],
    "th_xcorr_f64": [c_f32p, C.c_size_t, c_f32p, C.c_size_t, C.c_int64, C.c_size_t, C.POINTER(C.c_double)],
    "th_align_energy_f64": [c_f32p, C.c_size_t, C.c_int64, C.c_size_t, C.POINTER(C.c_double)],
    "th_align_peak": [C.POINTER(C.c_double), C.c_size_t, C.c_uint32, C.c_double, C.POINTER(C.c_uint32), c_szp, C.POINTER(C.c_double),
                      C.POINTER(C.c_double)],
    "th_align_f64": [c_f32p, C.c_size_t, C.c_uint32, c_f32p, C.c_size_t, C.c_uint32, C.POINTER(AlignRequest), C.POINTER(C.c_double),
                     C.c_size_t, c_szp],
    "th_tm_align_tracks": [vp, C.POINTER(AlignRequest), C.c_size_t, C.POINTER(C.c_double), C.c_size_t, C.POINTER(AlignInfo), c_szp],
    "th_tm_align_track": [vp, C.POINTER(AlignRequest), C.POINTER(C.c_double), C.c_size_t, C.POINTER(AlignInfo)],
    "th_tmg_align_tracks": [vp, C.POINTER(AlignRequest), C.c_size_t, C.POINTER(C.c_double), C.c_size_t, C.POINTER(AlignInfo), c_szp],
    "th_tmg_align_track": [vp, C.POINTER(AlignRequest), C.POINTER(C.c_double), C.c_size_t, C.POINTER(AlignInfo)],
    "th_tm_render_waveform_figures": [vp, C.POINTER(WaveformFigureRequest), C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.POINTER(WaveformFigureInfo), c_szp],
    "th_tm_render_waveform_figure": [vp, C.POINTER(WaveformFigureRequest), C.c_void_p, C.c_size_t, C.POINTER(WaveformFigureInfo)],
    "th_tmg_render_waveform_figures": [vp, C.POINTER(WaveformFigureRequest), C.c_size_t, C.c_void_p, C.c_size_t,
                                       C.POINTER(WaveformFigureInfo), c_szp],
    "th_tmg_render_waveform_figure": [vp, C.POINTER(WaveformFigureRequest), C.c_void_p, C.c_size_t, C.POINTER(WaveformFigureInfo)],
    "th_tile_cache_create": [C.c_size_t, C.POINTER(vp)],
    "th_tile_cache_destroy": [vp],
    "th_tile_cache_lookup": [vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), c_u8p, C.c_size_t,
                             c_szp, C.POINTER(C.c_int)],
    "th_tile_cache_store": [vp, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, c_u8p, C.c_size_t],
    "th_tile_cache_invalidate": [vp, C.c_int, C.c_int],
    "th_tile_cache_set_budget": [vp, C.c_size_t],
    "th_tile_cache_stats": [vp, c_szp, c_szp, c_szp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                            C.POINTER(C.c_uint64)],
}
_RESTYPES = {"th_plan_kernel_name": C.c_char_p, "th_pitch_f32": C.c_size_t, "th_pitch_u16": C.c_size_t,
             "th_waveform_pyramid_bins": C.c_size_t, "th_waveform_pyramid_offset": C.c_size_t}

lib.th_last_error.restype = C.c_char_p
lib.th_last_error.argtypes = []
for _name, _args in _SIGS.items():
    _fn = getattr(lib, _name)  # AttributeError here = header/library mismatch: fail loudly
    _fn.argtypes = _args
    _fn.restype = _RESTYPES.get(_name, C.c_int)


def last_error() -> str:
    return (lib.th_last_error() or b"").decode()


def check(code: int) -> None:
    if code != OK:
        raise ThError(code, last_error())
