"""thesia_amd — MI355X-native spectrogram / waveform compute path for the thesia viewer.

The product is libthesia_amd.so (hand-written HIP kernels for gfx950 behind the C ABI in
include/thesia_amd.h).  This package is the ctypes face of that ABI; importing it fails loudly
if the library has not been built.  There is no CPU fallback.
"""
from ._ffi import LIB_PATH, ThError, ChanDesc, ImgDesc, RasterDesc, WaveDesc, TileGeom  # noqa: F401
from .api import (LINEAR, MEL, SPECTRUM_MAX, SPECTRUM_MEAN_AMP, SPECTRUM_MEAN_POWER, Context, ab_variants, DeviceBuffer, Graph, MultiTrackManager, Plan, TileCache, TrackManager, calc_framing_params,  # noqa: F401
                  calc_mel_fb, calc_normalized_win, device_count, gated_loudness, global_db_range, hz_range_to_idx, k_weighting,
                  limiter_params, loudness_n_blocks, loudness_n_short_term, loudness_range, true_peak_filter, normalize_gain, mel_default_n_mel, pitch_f32, pitch_u16, shard_assign, spectrogram_tile_geometry, spectrum_frame_range, stft_n_frames, waveform_tile_geometry,
                  PCM_S16, PCM_S24, PCM_F32, DITHER_NONE, DITHER_TPDF, audio_sample_range, export_chunk_frames, export_dither, export_quantize, wav_header, FLAC_BLOCK, FLAC_LPC, FLAC_STEREO, FLAC_LPC_MAX_ORDER, flac_bound, flac_frame_header, flac_encode_i32,
                  resample_plan, resample_n_out, resample_coefs, resample_f32, resample_tile,
                  BAND_PASS, BAND_STOP, band_plan, band_coefs, band_response, band_f32,
                  FIGURE_RGBA, FIGURE_GREY16, figure_axis, figure_box,
                  edges, envelope_edges, waveform_figure_span,
                  FORMANT_WIN_GAUSS, FORMANT_WIN_RECT, FORMANT_OUT_FORMANTS, FORMANT_OUT_LPC, formant_request, formant_plan, formant_window,
                  formant_start_points, formants_f64, formant_frame_f64,
                  ALIGN_OUT_SUMMARY, ALIGN_OUT_CURVE, ALIGN_ABS, ALIGN_SUMMARY_DOUBLES, align_request, align_plan, xcorr_f64, align_energy_f64,
                  align_peak, align_f64, align_summary)

__all__ = ["LINEAR", "MEL", "SPECTRUM_MEAN_AMP", "SPECTRUM_MEAN_POWER", "SPECTRUM_MAX", "Context", "ab_variants", "DeviceBuffer", "Graph", "MultiTrackManager", "Plan", "TileCache", "TrackManager", "ThError", "calc_framing_params",
           "calc_mel_fb", "calc_normalized_win", "device_count", "gated_loudness", "global_db_range", "hz_range_to_idx", "k_weighting",
           "limiter_params", "loudness_n_blocks", "loudness_n_short_term", "loudness_range", "true_peak_filter", "normalize_gain", "mel_default_n_mel", "pitch_f32", "pitch_u16", "shard_assign", "spectrogram_tile_geometry", "spectrum_frame_range", "stft_n_frames", "waveform_tile_geometry",
           "PCM_S16", "PCM_S24", "PCM_F32", "DITHER_NONE", "DITHER_TPDF", "audio_sample_range", "export_chunk_frames", "export_dither", "export_quantize", "wav_header", "FLAC_BLOCK", "FLAC_LPC", "FLAC_STEREO", "FLAC_LPC_MAX_ORDER", "flac_bound", "flac_frame_header", "flac_encode_i32",
           "resample_plan", "resample_n_out", "resample_coefs", "resample_f32", "resample_tile",
           "BAND_PASS", "BAND_STOP", "band_plan", "band_coefs", "band_response", "band_f32",
           "FIGURE_RGBA", "FIGURE_GREY16", "figure_axis", "figure_box",
           "edges", "envelope_edges", "waveform_figure_span",
           "FORMANT_WIN_GAUSS", "FORMANT_WIN_RECT", "FORMANT_OUT_FORMANTS", "FORMANT_OUT_LPC", "formant_request", "formant_plan", "formant_window",
           "formant_start_points", "formants_f64", "formant_frame_f64",
           "ALIGN_OUT_SUMMARY", "ALIGN_OUT_CURVE", "ALIGN_ABS", "ALIGN_SUMMARY_DOUBLES", "align_request", "align_plan", "xcorr_f64", "align_energy_f64",
           "align_peak", "align_f64", "align_summary",
           "ChanDesc", "ImgDesc", "RasterDesc", "WaveDesc", "TileGeom", "LIB_PATH"]
