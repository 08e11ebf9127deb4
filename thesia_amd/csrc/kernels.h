// kernels.h — launcher declarations (implemented in kernels_*.hip).  All launchers are
// stream-ordered, never synchronise, and return the launch status.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/thesia_amd.h"
#include "batch_plan.h"  // ImgJob, FusedJob, RasterJob, WaveJob, PyrJob, StatsJob, their constants, pyramid_bins / pyramid_offset / waveform_blocks_for
#include "host_math.h"
#include "stft_core.h"
#include "envelope_plan.h"  // EnvJob, LaneSpanJob, LaneRasterJob, ENV_* (the chunk grid of kernels_envelope.hip)
#include "formant_plan.h"  // FormantJob
#include "align_plan.h"  // AlignJob, ALIGN_* (the tile shape of kernels_align.hip)
#include "flac_plan.h"  // FlacJob
#include "figure_plan.h"  // FigHJob, FigVJob, FIG_* (the tile shape of kernels_figure.hip)
#include "reader_plan.h"  // LoudJob, LoudTrackJob, TruePeakJob, ExportJob, ResampleJob, ResampleTiling and their constants
#include "stft_plan.h"  // WavePostJob, MelJob, MEL_TILE_FRAMES, MEL_ROWS_*

// Measured-and-dropped kernel variants: the packed-f32 pipeline (selector 9), the sweep chunk schedule (11), the
// workgroup-per-frame Stockham kernels of n_fft 32768 / 65536 (14), the subwave plan at n_fft 8192 (15) and launch shapes other
// than each size's defaults (waves-per-workgroup tuning) are compiled only with -DTH_AB_VARIANTS=1 (scripts/build_variant.sh
// <tag> -DTH_AB_VARIANTS=1 ...); the product library carries the kernels a default route can reach.  th_build_ab_variants()
// reports which build this is; th_plan_set_kernel refuses the selectors that are not in it.
#if !defined(TH_AB_VARIANTS)
#define TH_AB_VARIANTS 0
#endif
// The banded mel table of the n_fft 1024 / 2048 wave kernels in its paired layout (mel_fuse.h build_mel_band, stft_wave.h
// mel_banded<true>): host table and device code must agree, so the switch lives here (0: plain layout, for A/B builds; the
// frame-pair epilogue reads the paired layout only and is then off: stft_wave_mel_pair_applies).
#if !defined(TH_MEL_BAND_PAIRED)
#define TH_MEL_BAND_PAIRED 1
#endif

// The same switch for mel_band_rows_kernel (n_fft 4096, two-kernel path): table from api.hip, reads in kernels_mel.hip.
// (2.139 against 2.158 ms at the 96 kHz default, 2.152 against 2.163 at 88.2 kHz: the kernel is bound by reading the amplitude rows)
#if !defined(TH_MEL_ROWS_PAIRED)
#define TH_MEL_ROWS_PAIRED 1
#endif

namespace th {

// ---- kernels_stft.hip
hipError_t launch_minmax_init(float *d_minmax, uint32_t n_chan, hipStream_t s);
// d_out = [min, -max] and / or d_range = [min_dB, max_dB] (core/mod.rs:179-180); either may be NULL
hipError_t launch_minmax_reduce(const float *d_minmax, uint32_t n_chan, float *d_out, float dB_range, float *d_range, hipStream_t s);
size_t stft_generic_lds_bytes(const StftGeom &g);
// n_fft >= 32768: the generic kernel keeps its two frame buffers in global scratch (d_scratch, at least
// stft_generic_scratch_bytes) instead of LDS and runs as a persistent grid; 0 bytes = the LDS variant, no scratch needed
size_t stft_generic_scratch_bytes(const StftGeom &g, uint32_t n_tiles, uint32_t n_cu);
// Bluestein plans (an odd factor of n_fft above 63; stft_bluestein_kernel): convolution length, scratch bytes of a launch, launch.
// d_chirp[nc], d_bhat[M], d_twm[M / 2], d_tws[nc / 2 + 1]: complex doubles (bluestein_tables, host_math.h)
constexpr uint32_t STFT_MAX_DIRECT_ODD = 63;  // the largest odd factor the generic kernel takes as one direct pass
uint32_t stft_bluestein_m(const StftGeom &g);
size_t stft_bluestein_scratch_bytes(const StftGeom &g, uint32_t n_tiles, uint32_t n_cu);
hipError_t launch_stft_bluestein(const StftGeom &g, const ChanJob *d_jobs, const uint32_t *d_tile_start, uint32_t n_chan, uint32_t n_tiles,
                                 const float *d_window, const void *d_chirp, const void *d_bhat, const void *d_twm, const void *d_tws,
                                 const float *d_mel_fb, const uint32_t *d_mel_lo, const uint32_t *d_mel_hi, float *d_minmax, hipStream_t s,
                                 void *d_scratch, uint32_t n_cu);
hipError_t launch_stft_generic(const StftGeom &g, const ChanJob *d_jobs, const uint32_t *d_tile_start,
                               uint32_t n_chan, uint32_t n_tiles, const float *d_window, const cf32 *d_tw,
                               const float *d_mel_fb, const uint32_t *d_mel_lo, const uint32_t *d_mel_hi,
                               float *d_minmax, hipStream_t s, void *d_scratch = nullptr, uint32_t n_cu = 256);

bool stft_wave_supported(const StftGeom &g);
// n_fft 8192 / 16384: launch_stft_wave runs the workgroup-per-frame kernel (stft_block.h): interior frames only, the
// boundary frames always go to the generic kernel
bool stft_is_block_plan(const StftGeom &g);
// n_fft 8192 / 16384 mel plans: the filterbank (moment form) in the block kernel's epilogue where that kernel is the plan that runs
bool stft_block_mel_fused_applies(const StftGeom &g, int long_plan);
uint32_t stft_block_mel_max_index(const StftGeom &g);
// the multi-frame kernel (two / four frames per wave) takes this launch: n_fft 512 or 1024, dB output, no grid-aligned mode
bool stft_wave_multi_applies(const StftGeom &g, int out_mode);
uint32_t stft_wave_multi_tail_guard(const StftGeom &g);  // samples an interior span must stay clear of the channel's end
int stft_wave_default_waves(const StftGeom &g);
// d_minmax of launch_stft_wave is a per-CHUNK (min, max) array (2 floats per tile).  launch_wave_post follows every wave
// launch: per channel it folds the chunk pairs of the channel's tiles [t0, t1) into the channel slot (store = the slot
// needs no initialisation: every frame of the channel was in the wave launch) and rewinds the queue (d_queue_head[0],
// zero before the first launch; the kernel counts from 0 behind its statically assigned first round of chunks: a wave's
// first chunk is its own index, TH_SCHED_ADVANCE adds the grid's wave count to what it pulls).
// d_range (may be NULL; single-job launches with store only): [min_dB, max_dB] of the one channel, clamped by dB_range
hipError_t launch_wave_post(const WavePostJob *d_pj, uint32_t n_pj, const float *d_chunk_mm, float *d_mm_slots, bool store,
                            uint32_t *d_queue_head, float dB_range, float *d_range, hipStream_t s);
// What the wave kernel writes: dB rows of the linear spectrum, linear amplitude rows (first half of the matrix-core
// mel path), or dB rows of the mel spectrum with the filterbank fused into the epilogue (mel_fuse.h tables).
struct WaveOut {
    int mode = 0;                     // 0 dB linear, 1 amplitude, 2 fused mel
    int multi = 0;                    // 1: the multi-frame kernel (n_fft 512 / 1024, stft_wave_multi.h; mode 0 only)
    int packed = 0;                   // 1: the packed-f32 pipeline (stft_pk.h) where it is instantiated (selector 9), else ignored
    int sweep = 0;                    // 1: the sweep chunk schedule (4-frame chunks dealt out in order; n_fft 2048, hop = n_fft / 4, dB rows, 12 waves)
    const uint32_t *mel_tab = nullptr;  // DEVICE: mel_fuse.h word table
    uint32_t mel_words = 0, mel_slots = 0, mel_groups = 0, n_mel = 0;
    // banded sums (mel_slots == 0, build_mel_band): the table's header again, as kernel arguments (scalar registers instead
    // of two LDS reads + v_readfirstlane per group and frame): block offset and taps of group g
    uint32_t band_off[8] = {0, 0, 0, 0, 0, 0, 0, 0}, band_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // banded sums, n_fft 2048: 1 = the frame-pair epilogue (two consecutive frames of a chunk share one pass over the table:
    // stft_wave_kernel<.., OUT = 3>; the host sets it where stft_wave_mel_pair_applies says so)
    uint32_t mel_pair = 0;
    // n_fft 1024 / 2048: 1 = the moment form of the filterbank (mel_tab = build_mel_moments' table, read from global memory; mel_words = 0):
    // mel counts above what an LDS table holds.  (n_fft 4096 .. 16384 mel plans are always this form.)
    uint32_t mel_moment = 0;
    const cf32 *subwave_twc = nullptr;  // DEVICE: stft_subwave_build_twc's table (n_fft 32768 plans)
    int long_plan = 1;  // n_fft 8192 .. 65536: 1 = stft_block_kernel, 2 = stft_subwave_kernel (the host resolves the size's default: stft_subwave_default)
};
// ---- kernels_stft_long.hip: n_fft 8192 / 16384 / 32768 as 4 / 8 / 16 wave transforms + one combining pass (interior frames, as the block kernel)
bool stft_subwave_applies(const StftGeom &g);
bool stft_subwave_default(const StftGeom &g);  // the sizes where it is the default (measured: profiles/r05_ab_subwave.txt)
hipError_t launch_stft_subwave(const StftGeom &g, const ChanJob *d_jobs, const uint32_t *d_chunk_tab, uint32_t n_tiles, const cf32 *d_wtab,
                               const cf32 *d_tw, const cf32 *d_twc, float *d_minmax, bool amp, uint32_t n_cu, hipStream_t s);
size_t stft_subwave_twc_len(const StftGeom &g);  // cf32 entries of the combining pass's per-thread constant table
void stft_subwave_build_twc(const StftGeom &g, const cf32 *h_tw, cf32 *out);  // host: out[stft_subwave_twc_len(g)] from the plan's tw table
// the frame-pair form of the banded mel epilogue exists for this launch (n_fft 2048, hop a multiple of 128 samples or no register
// reuse at all, default waves) and the table's reads stay inside the two amplitude rows a slab holds (reach: MelBandHost::reach)
bool stft_wave_mel_pair_applies(const StftGeom &g, int waves, uint32_t reach);
// pieces the per-wave (r, f) buffer of the fused mel epilogue can hold for this n_fft (0: not supported), and whether
// the launch shape leaves room in LDS for a table of `words`
int stft_wave_phased_mode(const StftGeom &g, int waves);  // 0 no, 1 phased (hop 480), 2 dynamic (e.g. 441)
int stft_wave_mel_phase_mode(const StftGeom &g, int waves);  // the same for a launch with the fused mel epilogue (n_fft 4096: only the modes it is instantiated for)
uint32_t stft_wave_mel_max_pieces(const StftGeom &g);
// the sweep chunk schedule exists for this launch (shape, output mode, wave count; the caller adds: batch large enough)
bool stft_wave_sweep_applies(const StftGeom &g, int waves, int out_mode);
// banded: the banded-sum table (no per-wave (r, f) buffer at n_fft 1024, which only the pieces / gather form uses)
bool stft_wave_mel_fits(const StftGeom &g, int waves, uint32_t words, bool banded = false);
// n_fft 512 (four frames per wave): does the mel_rows table fit the launch's LDS beside the slabs at this wave count?
bool stft_wave_multi_mel_fits(const StftGeom &g, int waves, uint32_t words);
uint32_t stft_wave_multi_amp_pitch();  // floats per amplitude row of that kernel's mel epilogue (a lane of the moment form reads inside its frame's row)
// waves: waves per workgroup (4, 8, 12 or 16; <= 0 selects the default for this n_fft)
// d_tile_start: HERE the per-chunk table, 2 words per chunk: (job, first frame) — not the jobs' first chunks as in
// launch_stft_generic; chunks 0 .. W - 1 are statically assigned (W = waves of the grid), the queue serves the rest
hipError_t launch_stft_wave(const StftGeom &g, const ChanJob *d_jobs, const uint32_t *d_tile_start, uint32_t n_chan,
                            uint32_t n_tiles, const cf32 *d_wtab, const cf32 *d_tw, float *d_minmax,
                            uint32_t *d_queue_head, uint32_t n_cu, int waves, const WaveOut &out, hipStream_t s);

// ---- kernels_mel.hip: mel filterbank contraction on the matrix cores (MelJob: stft_plan.h)
hipError_t launch_mel_mfma(const MelJob *d_jobs, const uint32_t *d_tile_start, uint32_t n_jobs, uint32_t n_tiles,
                           uint32_t amp_pitch, const float *d_bt, const uint32_t *d_tile_band, const uint32_t *d_slice_start,
                           uint32_t n_slices, uint32_t zero_block, uint32_t n_mel, float *d_minmax, hipStream_t s);
// short rows under narrow filters (n_fft 512): banded sums, lane = mel (d_tab: build_mel_rows, stft_plan.h)
hipError_t launch_mel_rows(const MelJob *d_jobs, const uint32_t *d_tile_start, uint32_t n_jobs, uint32_t n_tiles,
                           uint32_t amp_pitch, const uint32_t *d_tab, uint32_t n_groups, uint32_t n_mel, float *d_minmax,
                           uint32_t n_cu, hipStream_t s);

// long rows (n_fft 4096) under narrow filters: the banded sums of build_mel_band (mel_fuse.h) over the amplitude rows,
// one row per wave at a time through LDS.  hdr: the table's 16 header words (offset and taps per group).
bool mel_band_rows_fits(uint32_t n_freq, uint32_t words);
hipError_t launch_mel_band_rows(const MelJob *d_jobs, const uint32_t *d_tile_start, uint32_t n_jobs, uint32_t n_tiles,
                                uint32_t amp_pitch, uint32_t n_freq, const uint32_t *d_tab, uint32_t words, uint32_t groups,
                                const uint32_t *hdr, uint32_t n_mel, float *d_minmax, uint32_t n_cu, hipStream_t s);

// ---- kernels_image.hip (ImgJob, FusedJob, RasterJob, IMG_TILE_*, FUSED_*, RASTER_*: batch_plan.h)
hipError_t launch_spec_to_img(const ImgJob *d_jobs, const uint32_t *d_tile_job, uint32_t n_jobs,
                              uint32_t n_tiles, float min_dB, float max_dB, uint32_t colormap_len, const float *d_range,
                              hipStream_t s);
hipError_t launch_db_range(const float *d_in, float dB_range, float *d_out, hipStream_t s);

hipError_t launch_spec_to_img_raster(const FusedJob *d_jobs, const uint32_t *d_block_job, uint32_t n_blocks, uint8_t *const *d_tiles,
                                     float min_dB, float max_dB, const float *d_range, int all_zero, const uint8_t *d_colormap,
                                     uint32_t n_colors, hipStream_t s);

hipError_t launch_raster_level0(const RasterJob *d_jobs, const uint32_t *d_block_job, uint32_t n_jobs,
                                uint32_t n_blocks, const uint8_t *d_colormap, uint32_t n_colors, hipStream_t s);

// Separable Lanczos3 LOD resample of a crop of a u16 image (encode_spectrogram_tile, LOD > 0,
// render_tiles.rs:354-393).  Per output index of an axis the host tabulates the first source index,
// the tap count, the f64 tap weights and their sum (same order as the CPU restatement).
struct LodAxis {             // device pointers into one uploaded blob
    const int32_t *start;    // [n_out] first source index (already clamped to the image / row window)
    const int32_t *count;    // [n_out] number of taps
    const double *wsum;      // [n_out] sum of the taps
    const double *w;         // [n_out][max_taps]
    uint32_t n_out, max_taps;
    // batched pass only (launch_lod_vpass_batch): rows spanned by the tap windows of R consecutive outputs, maximum over
    // the aligned groups of R = 8, 4, 2 outputs (0: unknown, one output per thread)
    uint32_t span[3] = {0, 0, 0};
};
// horizontal pass: tmp[r][ox] for the source rows y_lo + r, r < n_rows; vertical pass: lod[oy][ox]
// (tmp_pitch / lod_pitch: elements per row of the intermediate and of the result)
hipError_t launch_lod_hpass(const uint16_t *d_img, uint32_t img_pitch, uint32_t y_lo, uint32_t n_rows, LodAxis ax,
                            uint16_t *d_tmp, uint32_t tmp_pitch, hipStream_t s);
hipError_t launch_lod_vpass(const uint16_t *d_tmp, uint32_t tmp_pitch, uint32_t y_lo, LodAxis ay, uint32_t dw,
                            uint16_t *d_lod, uint32_t lod_pitch, hipStream_t s);
// the vertical pass over many images of one shape (whole images: source rows from 0): one launch, grid z = job
struct LodPassJob {
    const uint16_t *src;
    uint16_t *dst;
    uint32_t src_pitch, dst_pitch;
};
hipError_t launch_lod_vpass_batch(const LodPassJob *d_jobs, uint32_t n_jobs, LodAxis ay, uint32_t dw, hipStream_t s);
// dst[x][y] = src[y][x] for w x h images (src_pitch / dst_pitch in elements)
hipError_t launch_transpose_u16_batch(const LodPassJob *d_jobs, uint32_t n_jobs, uint32_t w, uint32_t h, hipStream_t s);
// one tile rectangle of one image -> RGBA, job passed by value (tile requests: nothing to upload)
hipError_t launch_raster_tile(const uint16_t *d_img, uint32_t img_width, uint32_t img_height, uint32_t img_pitch,
                              uint32_t origin_x, uint32_t origin_y, uint32_t width, uint32_t height, uint8_t *d_rgba,
                              const uint8_t *d_colormap, uint32_t n_colors, hipStream_t s);

// streaming 16-byte-per-lane device copy of bytes / 16 * 16 bytes (the bandwidth yardstick of bench.py)
hipError_t launch_copy_f4(const void *d_src, void *d_dst, uint64_t bytes, hipStream_t s);

// ---- kernels_waveform.hip (WaveJob, PyrJob, StatsJob, PYR_MAX_LEVELS: batch_plan.h)
hipError_t launch_waveform(const WaveJob *d_jobs, const uint32_t *d_block_start, uint32_t n_jobs,
                           uint32_t n_blocks, hipStream_t s);

hipError_t launch_channel_stats(const StatsJob *d_jobs, uint32_t n_jobs, uint64_t max_samples, double *d_sumsq,
                                uint32_t *d_peak_bits, hipStream_t s);
hipError_t launch_pyramid_base(const PyrJob *d_jobs, uint32_t n_jobs, uint64_t max_samples, hipStream_t s);
hipError_t launch_pyramid_up(const PyrJob *d_jobs, uint32_t n_jobs, uint64_t max_samples, uint32_t level, uint32_t parity,
                             hipStream_t s);

// ---- kernels_loudness.hip: K-weighted chunk energies, per-channel sum of squares and peak, 400 ms block energies (LoudJob,
// LoudTrackJob: reader_plan.h)
hipError_t launch_loudness(const LoudJob *d_jobs, uint32_t n_jobs, uint32_t max_chunks, uint32_t max_fchunks, const LoudnessRate *d_rates,
                           uint32_t lds_floats, const LoudTrackJob *d_tjobs, uint32_t n_tracks, uint64_t max_blocks, hipStream_t s);
// pass D alone over the q of an earlier launch_loudness: blocks of `span` segments (4: the momentary series, 30: the short-term one;
// LoudTrackJob::L = span s100, n_blocks = n_seg - span + 1, n_fchunks >= n_seg n_sub), summed in the same order
hipError_t launch_loudness_blocks(const LoudTrackJob *d_tjobs, uint32_t n_tracks, uint64_t max_blocks, uint32_t span, hipStream_t s);

// ---- kernels_meter.hip: the true peak of a batch of channels (TruePeakJob, TP_*: reader_plan.h)
struct TruePeakCoef {      // f32 taps: phase p = 1 .. F - 1, delay d at c[(p - 1) T + d] (T = 12 at F = 4, 24 at F = 2), then phase 0's one tap
    float c[36];
    float c0;
    uint32_t d0;           // phase 0's delay (6 or 12)
};
void true_peak_coef(uint32_t factor, TruePeakCoef *out);  // host: from true_peak_filter, rounded to f32
// factor 4 or 2 (K = true_peak_coef(factor)); every job of d_jobs is of that factor; max_chunks: the largest n_chunks
hipError_t launch_true_peak(const TruePeakJob *d_jobs, uint32_t n_jobs, uint32_t max_chunks, uint32_t factor, const TruePeakCoef &K,
                            hipStream_t s);

// ---- kernels_dynamics.hip: normalise gain + clip guard (clip, global level, look-ahead limiter) of a batch of tracks
struct DynApplyJob {        // one track: y = gain x in f32, then the clamp or a global gain
    const float *x;         // channel c at x + c x_stride
    float *aud;             // channel c at aud + c y_stride
    float *before;          // Clip: gain x before the clamp (stride y_stride); else NULL
    uint64_t x_stride, y_stride, n;
    double g;               // scale: y <- clamp(f32(f64(y) g))   (reduce_global_level, audio.rs:145-159)
    float gain;
    uint32_t n_ch, clip, scale;
    uint32_t *peak_bits;         // Clip: n_ch slots, max |gain x| as float bits (zeroed by the caller)
    unsigned long long *cnt;     // Clip: n_ch slots, samples with |gain x| > 1 (zeroed by the caller)
};
hipError_t launch_dyn_apply(const DynApplyJob *d_jobs, uint32_t n_jobs, uint64_t max_n, hipStream_t s);
constexpr uint32_t LIM_CHUNK = 256;  // samples per chunk of the release scan
constexpr uint32_t LIM_BLOCK = 64;   // samples per block maximum of the peak hold (one wave)
struct LimJob {             // one track through PerfectLimiter::process_inplace (limiter.rs:110-156); N = n + attack
    const float *x;
    float *aud;
    float *gain_seq;        // n f32 gains
    uint64_t x_stride, y_stride, n;
    float *v;               // scratch, N: max over the channels of |gain x| (0 behind the track)
    float *bm;              // scratch, ceil(N / LIM_BLOCK): block maxima of v
    double *a, *b;          // scratch, N each: the envelope stages, ping-pong
    double *sum;            // scratch, 4 per release chunk: the chunk's map (A, D, C) and its start state
    double slew;            // 1 / (release_samples + 1)
    float gain;
    uint32_t n_ch, attack, hold, box_len[3];
    uint32_t *min_bits;          // least gain as float bits (set to the bits of 1.0f by the caller)
    unsigned long long *cnt;     // gains != 1 (zeroed by the caller)
};
hipError_t launch_limiter(const LimJob *h_jobs, const LimJob *d_jobs, uint32_t n_jobs, hipStream_t s);

// ---- kernels_spectrum.hip: per-column mean amplitude / mean power / maximum over a frame range of resident dB rows
struct SpectrumShape {      // how one job is cut (spectrum_shape: from the job's own height and frame count alone)
    uint32_t log_ct;        // a column tile is 2^log_ct quads of 4 columns (8 .. 64 quads)
    uint32_t n_ctiles, n_slices, slice_len;  // frames [f0 + s slice_len, ...) are slice s; n_slices = 0 for an empty range
};
SpectrumShape spectrum_shape(uint32_t height, uint32_t n_frames);
struct SpectrumJob {        // one (channel, frame range, kind)
    const float *rows;      // T x pitch f32 dB, frame-major, 16-byte aligned
    double *part;           // scratch: n_slices x (n_ctiles << (log_ct + 2)) partials
    float *out;             // H results (device memory or mapped host memory)
    uint64_t pitch;         // floats per row: a multiple of 4, >= H
    uint32_t H, f0, f1, kind;  // frames [f0, f1), TH_SPECTRUM_*
    uint32_t log_ct, n_ctiles, n_slices, slice_len;
};
static_assert(sizeof(SpectrumJob) == 64, "SpectrumJob must have no implicit padding");
// max_blocks: the largest n_ctiles * n_slices of the jobs; max_height: the largest H
hipError_t launch_spectrum(const SpectrumJob *d_jobs, uint32_t n_jobs, uint32_t max_blocks, uint32_t max_height, hipStream_t s);

// ---- kernels_export.hip: planar f32 channels to interleaved file bytes (ExportJob, export_chunk_frames: reader_plan.h)
constexpr uint32_t EXPORT_THREADS = 256;
// n_chunks: the sum over the jobs (the first_chunk a job behind the last would have)
hipError_t launch_export(const ExportJob *d_jobs, uint32_t n_jobs, uint32_t n_chunks, hipStream_t s);

// ---- kernels_resample.hip: polyphase sinc resampler (ResampleJob, ResampleTiling: reader_plan.h)
// table: L rows of `taps` floats (host_math.h resample_table); n_blocks: the sum over the jobs
hipError_t launch_resample(const ResampleJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, const float *d_table, const ResampleTiling &t,
                           hipStream_t s);

// ---- kernels_band.hip: one FIR row for every output (BandJob, BandTiling: reader_plan.h)
// row: t.taps floats (host_math.h band_row); n_blocks: the sum over the jobs
hipError_t launch_band(const BandJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, const float *d_row, const BandTiling &t, hipStream_t s);

// ---- kernels_flac.hip: the FLAC encoder of a piece (FlacJob: flac_plan.h), three launches in stream order.  n_units: the piece's
// (block, coded channel) pairs; n_blocks: its blocks; flags: the call's TH_FLAC_* (every job of the table carries the same; 0 runs the
// kernel instance that is compiled without LPC and stereo)
hipError_t launch_flac_subframes(const FlacJob *d_jobs, uint32_t n_jobs, uint32_t n_units, uint32_t flags, hipStream_t s);
hipError_t launch_flac_scan(const FlacJob *d_jobs, uint32_t n_jobs, hipStream_t s);
hipError_t launch_flac_frames(const FlacJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, hipStream_t s);

// ---- kernels_figure.hip: a region of a u16 image at any pixel size (FigHJob, FigVJob: figure_plan.h).  n_blocks: the sum over the jobs
hipError_t launch_figure_hpass(const FigHJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, hipStream_t s);
// d_colormap: n_colors RGBA entries (read by the TH_FIGURE_RGBA jobs only)
hipError_t launch_figure_vpass(const FigVJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, const uint8_t *d_colormap, uint32_t n_colors,
                               hipStream_t s);

// ---- kernels_envelope.hip: (min, max, mean, rms) per pixel column of a time range of resident audio, and its raster as a waveform
// lane (EnvJob, LaneSpanJob, LaneRasterJob: envelope_plan.h).  n_units: the chunks of the dense jobs; n_cblocks, n_blocks: the sum
// over the jobs.  The reduction runs in front of the column kernel, which adds the partials it leaves
hipError_t launch_envelope_reduce(const EnvJob *d_jobs, uint32_t n_jobs, uint32_t n_units, hipStream_t s);
hipError_t launch_envelope_columns(const EnvJob *d_jobs, uint32_t n_jobs, uint32_t n_cblocks, hipStream_t s);
hipError_t launch_lane_spans(const LaneSpanJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, hipStream_t s);
hipError_t launch_lane_raster(const LaneRasterJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, hipStream_t s);

// ---- kernels_formant.hip: the raw LPC / root record of every frame of a piece (FormantJob: formant_plan.h).  n_blocks: the piece's
// frames; max_W, max_p: the largest of its jobs (they size the launch's LDS)
hipError_t launch_formants(const FormantJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, uint32_t max_W, uint32_t max_p, hipStream_t s);

// ---- kernels_align.hip: the cross-correlation of one piece (AlignJob: align_plan.h; passed by value, no device table): the group
// values into job.scratch, then their fold over the groups, job.n_lags doubles, into d_rec.  launch_align_energy: the group values of
// E(x, first, N) (x: a track of n samples, +0 outside) into d_groups[0 .. align_n_groups(N)); the host folds them (align_fold)
hipError_t launch_align_xcorr(const AlignJob &job, double *d_rec, hipStream_t s);
hipError_t launch_align_energy(const float *d_x, uint64_t n, int64_t first, uint64_t N, double *d_groups, hipStream_t s);

}  // namespace th
