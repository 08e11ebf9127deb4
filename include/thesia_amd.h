/*
 * thesia_amd.h — C ABI of the MI355X-native spectrogram / waveform compute path for thesia.
 *
 * This is the drop-in boundary: a plain `extern "C"` surface (opaque handles, plain pointers
 * and sizes, int status codes, no C++/torch types) that replaces the five pure Rust functions
 * at the reference's internal seam and the TrackManager orchestration that calls them.
 * All file:line citations are relative to the reference checkout (Sytronik/thesia).
 *
 *   reference seam                                         → entry point(s) here
 *   ------------------------------------------------------------------------------------------
 *   SpecSetting::calc_framing_params  spectrogram.rs:56-98  → th_calc_framing_params
 *   calc_normalized_win               windows.rs:12-38      → th_calc_normalized_win
 *   calc_mel_fb / _default            src-common/lib.rs:46-103 → th_calc_mel_fb, th_mel_default_n_mel
 *   FreqScale::hz_range_to_idx        src-common/lib.rs:144-159 → th_hz_range_to_idx
 *   SpectrogramAnalyzer prepare/retain spectrogram.rs:101-185 → th_plan_create / th_plan_destroy
 *   SpectrogramAnalyzer::calc_spec    spectrogram.rs:187-212 → th_calc_spec_batch_dev, th_calc_spec_host
 *     (perform_stft stft.rs:16-149, norm :200, mel dot :207, dB decibel.rs:170-214)
 *   find_min_max + range clamp        simd.rs:14-36, core/mod.rs:169-180 → fused into th_calc_spec_*
 *                                                             (per-channel min/max), th_global_db_range
 *   convert_spectrogram_to_img        visualize/drawing.rs:4-33 → th_spec_to_img_dev
 *   encode_spectrogram_tile           render_tiles.rs:281-393 → th_encode_spectrogram_tile_dev, th_raster_tiles_dev
 *   encode_waveform_tile              render_tiles.rs:232-279 → th_encode_waveform_tile_dev, th_waveform_tiles_dev
 *   TrackManager (update_specs, update_spec_imgs, ...) core/mod.rs:33-230 → th_tm_*
 *   tile commands                     src-tauri/src/lib.rs:342-389 → th_tm_get_waveform_tile, th_tm_get_spectrogram_tile
 *   set_common_normalize / set_common_guard_clipping  lib.rs:287-319 (track.rs:152-171,329-337, audio.rs:50-63,133-179,
 *     dynamics/{normalize,guardclipping,limiter,envelope,stats}.rs) → th_tm_set_common_normalize, th_tm_set_common_guard_clipping,
 *     th_tm_get_track_dynamics, th_tm_get_guard_clip_stats, th_tm_get_limiter_gain; th_normalize_gain, th_limiter_params
 *
 * Conventions
 *   - Every function returns th_status (0 = ok, <0 = error) and never throws or aborts;
 *     th_last_error() returns a thread-local message for the last failure on this thread.
 *   - The caller owns every host buffer it passes.  Inputs are borrowed for the call only.
 *     Outputs go to caller buffers with a capacity; the written length is returned.
 *   - The library owns device memory behind opaque handles with explicit destroy.
 *   - "_dev" entries take DEVICE pointers and enqueue on the context's HIP stream.  A call that returns data to the
 *     host synchronises that stream; so does a first call, or one whose descriptors changed, when it uploads its
 *     descriptor tables or grows a scratch buffer.  A repeat call with the same descriptors only enqueues.
 *     All other entries take HOST pointers.
 *   - Alignment.  A DEVICE pointer — an argument, a struct field or an entry of a pointer array marked DEVICE — needs the
 *     alignment of its element type and no more (f32: 4 bytes, u16: 2, bytes: 1), unless its declaration says otherwise:
 *     th_dev_copy 16 bytes (pointers and size); rgba, tiles[] and d_colormap 4 bytes (one RGBA8 pixel / LUT entry);
 *     block_energy 8 bytes (f64).  So a channel may be a row of a planar channels x samples array of any length, spec
 *     rows and images sub-rectangles of wider arrays, outputs packed back to back.  Faster paths (8- and 16-byte
 *     accesses) are taken where base, pitch and origin allow them; the values written do not depend on the alignment,
 *     except where a sum is taken in another order (th_channel_stats_dev's sum of squares, th_audio_stats_dev's rms_dB:
 *     within their stated accuracy either way).  The entries check it: a device pointer below its stated alignment is
 *     refused with TH_ERR_INVALID_ARG before anything is launched, and th_last_error() names the argument.
 *   - Compute entries (th_calc_spec_*, th_tm_* mutators) may assume exclusive access, like the
 *     reference's single write-lock worker (interface.rs:12-56).  th_tm_* tile getters run
 *     concurrently with each other (each request has its own HIP stream and pinned staging buffer)
 *     and are excluded only while a th_tm_* mutator runs (reader / writer lock, as the reference's
 *     RwLock<TrackManager>, lib.rs:345,378); the context-level th_encode_*_tile_dev entries share
 *     the context stream and serialise on an internal mutex.
 *   - There is NO CPU fallback: compute entries fail with TH_ERR_NO_DEVICE without a GPU.
 */
#ifndef THESIA_AMD_H
#define THESIA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#define TH_EXTERN_C extern "C"
#else
#define TH_EXTERN_C
#endif
#define TH_API TH_EXTERN_C __attribute__((visibility("default")))

typedef enum {
    TH_OK = 0,
    TH_ERR_INVALID_ARG = -1,
    TH_ERR_UNSUPPORTED = -2,
    TH_ERR_HIP = -3,
    TH_ERR_NO_DEVICE = -4,
    TH_ERR_OOM = -5,
    TH_ERR_BUFFER_TOO_SMALL = -6,
    TH_ERR_NOT_FOUND = -7,
    TH_ERR_INTERNAL = -8
} th_status;

/* FreqScale (src-common/src/lib.rs:105-109) */
#define TH_FREQ_LINEAR 0
#define TH_FREQ_MEL 1

/* render_tiles.rs:14-16 */
#define TH_WAVEFORM_TILE_BINS 1024
#define TH_SPECTROGRAM_TILE_SIZE 512
#define TH_SPECTROGRAM_TILE_GUTTER 4
#define TH_WAVEFORM_TILE_MAX_BYTES (24 + 1024 * 12)
#define TH_SPECTROGRAM_TILE_MAX_BYTES (40 + 520 * 520 * 4)

typedef struct th_ctx th_ctx;   /* device + stream + scratch */
typedef struct th_plan th_plan; /* one SpectrogramAnalyzer cache entry */
typedef struct th_tm th_tm;     /* TrackManager mirror */
typedef struct th_tmg th_tmg;   /* TrackManager mirror over several devices of one process */

/* ---------------------------------------------------------------- errors / info */
TH_API const char *th_last_error(void);
TH_API int th_version(void);
TH_API int th_device_count(int *count);

/* ---------------------------------------------------------------- host-only helpers (no GPU) */
/* SpecSetting::calc_framing_params — spectrogram.rs:56-98 */
TH_API int th_calc_framing_params(double win_ms, uint32_t t_overlap, uint32_t f_overlap, uint32_t sr,
                                  size_t *hop, size_t *win, size_t *n_fft);
/* frame count of perform_stft — stft.rs:50-97 (T = floor((N + 2*(win/2) - win)/hop) + 1) */
TH_API int th_stft_n_frames(size_t n_samples, size_t win, size_t hop, size_t *n_frames);
/* calc_normalized_win(Hann, win, n_fft) — windows.rs:12-38,68-83; out[win] */
TH_API int th_calc_normalized_win(size_t win, size_t n_fft, float *out);
/* calc_mel_fb::<f32> — src-common/src/lib.rs:46-89; out[(n_fft/2+1) * n_mel], fmax < 0 = None */
TH_API int th_calc_mel_fb(uint32_t sr, size_t n_fft, size_t n_mel, float fmin, float fmax, int do_norm,
                          float *out);
/* n_mel chosen by calc_mel_fb_default — src-common/src/lib.rs:91-103 */
TH_API int th_mel_default_n_mel(uint32_t sr, size_t n_fft, size_t *n_mel);
/* FreqScale::hz_range_to_idx — src-common/src/lib.rs:144-159 */
TH_API int th_hz_range_to_idx(int freq_scale, float hz_min, float hz_max, uint32_t sr, size_t n_freqs_or_mels,
                              size_t *i_start, size_t *i_end);
/* max = min(max,0); min = max(min, max - dB_range) over per-spec (min,max) — core/mod.rs:169-180 */
TH_API int th_global_db_range(const float *mins, const float *maxs, size_t n, float dB_range, float *min_dB,
                              float *max_dB);

/* Multi-GPU partitioning of independent (track, channel) units (core/mod.rs:153-163 fans the same
 * units out over rayon threads): deterministic longest-processing-time assignment of units to
 * `world` ranks by weight (frame count).  owner[i] receives the rank of unit i.  No data-path
 * collective is involved; the only exchange of the path is the 2-float dB-range all-reduce. */
TH_API int th_shard_assign(const uint64_t *weights, size_t n_units, uint32_t world, uint32_t *owner);

typedef struct {
    uint32_t width, height;       /* tile size in LOD pixels (0,0 = empty tile) */
    uint32_t origin_x, origin_y;  /* tile origin in LOD pixels */
    uint64_t lod_width, lod_height;
} th_tile_geom;
/* tile geometry of encode_spectrogram_tile — render_tiles.rs:290-313 */
TH_API int th_spectrogram_tile_geometry(size_t img_width, size_t img_height, uint32_t level_x, uint32_t level_y,
                                        uint32_t tile_x, uint32_t tile_y, th_tile_geom *geom);
/* bin geometry of encode_waveform_tile — render_tiles.rs:233-241 */
TH_API int th_waveform_tile_geometry(size_t n_samples, uint32_t level, uint32_t tile_index, size_t *start,
                                     size_t *bin_count, size_t *samples_per_bin);

/* ---------------------------------------------------------------- device context */
/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL to create one. */
TH_API int th_ctx_create(int device, void *hip_stream, th_ctx **out);
/* use_given_stream != 0: run on `hip_stream` exactly as given, NULL meaning the legacy default stream
 * (what torch.cuda.current_stream() is unless a side stream is active); 0: same as th_ctx_create. */
TH_API int th_ctx_create_ex(int device, void *hip_stream, int use_given_stream, th_ctx **out);
TH_API int th_ctx_destroy(th_ctx *ctx);
TH_API int th_ctx_synchronize(th_ctx *ctx);
/* HIP-graph capture of a sequence of this library's stream-ordered calls on the context's stream (a launch-bound
 * sequence like the 8 small kernels of a single-track update: STFT -> range -> quantise -> raster).  Run the sequence
 * once normally first: descriptor tables and scratch buffers are uploaded / sized on first use, which needs the host.
 *   - Entries that can be captured (with warm tables they only enqueue): th_calc_spec_batch_dev,
 *     th_calc_spec_batch_ranged_dev, th_minmax_reduce_dev, th_global_db_range_dev, th_minmax_reduce_range_dev,
 *     th_spec_to_img_dev, th_spec_to_img_batch_dev, th_spec_to_img_batch_dev_ranged, th_spec_to_img_raster_batch_dev,
 *     th_raster_tiles_dev, th_waveform_tiles_dev, th_waveform_pyramid_dev, th_dev_copy.
 *   - Entries that cannot, because they return to host memory or synchronise: th_calc_spec_host, th_encode_*_tile_dev,
 *     th_channel_stats_dev, th_audio_stats_dev, th_dev_upload / th_dev_download (and th_dev_alloc / th_dev_free,
 *     th_ctx_synchronize, th_plan_create / th_plan_destroy), every th_tm_* / th_tmg_*.
 *   - A call of the first group that has to upload a table or size a scratch buffer, and every call of the second group
 *     but th_tm_* / th_tmg_*, is refused while this thread is capturing: it fails with TH_ERR_HIP before it touches the
 *     stream.  The capture must still be ended; th_ctx_capture_end then returns an error and *out = NULL.  Context,
 *     plans and stream are usable afterwards, and the same call made directly works.  th_tm_* / th_tmg_* are not checked:
 *     a synchronisation of theirs on a capturing stream invalidates the capture inside the HIP runtime, which can leave
 *     that stream unusable.
 *   - The graph replays the same launches with the same arguments: the same device pointers, the descriptor tables and
 *     scratch buffers of the plans and the context as they were when it was captured.  It is INVALID after any later
 *     call that uses other descriptors on a plan or a context the graph touched (descriptor tables are rewritten in
 *     place and plan scratch may be reallocated: a replay would read another batch's tables or freed memory — undefined),
 *     and once a plan, the context or a buffer it touched is gone.  Direct calls with the SAME descriptors in between
 *     are fine.  What the data in the buffers is at replay time is the caller's: a replay reads its inputs anew.
 *   - A context on the legacy default stream (which HIP cannot capture) records on a stream of its own and th_graph_launch
 *     replays on the legacy default stream; on any other stream the capture is the stream's own, so the host's own work
 *     enqueued on it between begin and end is recorded as well.
 * Capture is per thread (hipStreamCaptureModeThreadLocal), one at a time. */
typedef struct th_graph th_graph;
TH_API int th_ctx_capture_begin(th_ctx *ctx);
TH_API int th_ctx_capture_end(th_ctx *ctx, th_graph **out); /* *out = NULL and an error if the capture was invalidated */
TH_API int th_graph_launch(th_graph *graph);                /* stream-ordered on the context's stream, no sync */
TH_API int th_graph_destroy(th_graph *graph);
/* device memory helpers for callers without their own allocator (tests, C hosts) */
TH_API int th_dev_alloc(th_ctx *ctx, size_t bytes, void **dptr);
TH_API int th_dev_free(th_ctx *ctx, void *dptr);
TH_API int th_dev_upload(th_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
TH_API int th_dev_download(th_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* HIP-event timing on the context's stream (bench.py roofline leg) */
/* stream-ordered device-to-device copy with the library's own 16-byte-per-lane streaming kernel (pointers and size
 * multiples of 16): the copy-bandwidth yardstick bench.py reports beside the roofline fractions */
TH_API int th_dev_copy(th_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
TH_API int th_timer_start(th_ctx *ctx);
TH_API int th_timer_stop_ms(th_ctx *ctx, float *ms);

/* ---------------------------------------------------------------- SpectrogramAnalyzer plan */
/* largest transform a plan takes: 2^20 samples = 5.5 s at 192 kHz */
#define TH_MAX_N_FFT (1u << 20)
/* Device-resident window / twiddles / mel filterbank for one (sr, win, hop, n_fft, scale, n_mel)
 * key; mirrors prepare()/retain() (spectrogram.rs:116-185).  n_mel = 0 with TH_FREQ_MEL selects
 * calc_mel_fb_default's count.  n_fft: every EVEN value in [2, TH_MAX_N_FFT], win <= n_fft (else TH_ERR_UNSUPPORTED; mel
 * plans whose dense filterbank would exceed 1 GiB are refused the same way): every next_pow2(win) * f_overlap of
 * spectrogram.rs:66-72 up to the limit — powers of two run on the wave / block kernels, 2^a * odd with odd <= 63
 * (f_overlap 3, 5, 6, ...) on the generic kernel with the odd factor as one more pass, larger odd factors (f_overlap 67,
 * 71, 130, ...; round 6) as a chirp-z convolution in double precision.  No UI control offers the last two kinds. */
TH_API int th_plan_create(th_ctx *ctx, uint32_t sr, size_t win, size_t hop, size_t n_fft, int freq_scale,
                          size_t n_mel, th_plan **out);
TH_API int th_plan_destroy(th_plan *plan);
/* n_freq = n_fft/2+1; height = n_freq (linear) or n_mel (mel) = columns of the spec */
TH_API int th_plan_dims(const th_plan *plan, size_t *n_freq, size_t *height);
/* find_min_max over every resident spec (core/mod.rs:169-178) without leaving the device: reduces the n_chan
 * (min, max) pairs a th_calc_spec_batch_dev left in d_minmax to d_out = [min, -max] (2 floats, DEVICE), the form
 * in which ONE element-wise MIN all-reduce merges the ranks of a multi-GPU job.  n_chan = 0 gives [+inf, +inf]. */
TH_API int th_minmax_reduce_dev(th_ctx *ctx, const float *d_minmax, size_t n_chan, float *d_out);
/* update_spec_imgs' range clamp (core/mod.rs:179-180) on the device: d_min_negmax = [min, -max] (DEVICE, as
 * th_minmax_reduce_dev and a MIN all-reduce leave it) -> d_range = [min_dB, max_dB] (DEVICE) with
 * max_dB = min(max, 0), min_dB = max(min, max_dB - dB_range). */
TH_API int th_global_db_range_dev(th_ctx *ctx, const float *d_min_negmax, float dB_range, float *d_range);
/* Both of the above in one launch, for a single GPU (no all-reduce in between): d_range = [min_dB, max_dB];
 * d_min_negmax (may be NULL) additionally receives [min, -max]. */
TH_API int th_minmax_reduce_range_dev(th_ctx *ctx, const float *d_minmax, size_t n_chan, float dB_range,
                                      float *d_min_negmax, float *d_range);
/* name of the kernel th_calc_spec_batch_dev will launch for this plan (for profiles / tests) */
TH_API const char *th_plan_kernel_name(const th_plan *plan);

/* Recommended row pitches (elements) for device-resident specs / images: rows padded to a multiple of
 * 128 bytes so that every row starts on a cache line.  The reference layout (dense rows) is what the
 * copy-out accessors return; the pitch is an HBM-layout choice of this library.
 * Rows laid out at exactly these pitches OWN their padding (elements [row_elems, pitch) of every row): the kernels
 * may fill it with zeros so that the last 128-byte line of a row is written whole (a partially written line costs
 * HBM a read-modify-write: 3.9 -> 5.4 TB/s for 1025-float rows, scripts/ubench/row_stores.hip).  Any other pitch
 * (dense rows, or rows embedded in a wider caller-owned array) is never written outside [0, row_elems). */
TH_API size_t th_pitch_f32(size_t row_elems);
TH_API size_t th_pitch_u16(size_t row_elems);

/* ---------------------------------------------------------------- calc_spec (layer A, device pointers) */
typedef struct {
    const float *wav;    /* DEVICE: n_samples f32, one channel */
    float *spec;         /* DEVICE: n_frames rows of f32 dB, frame-major like the reference's Array2 (T x H) */
    uint64_t n_samples;
    uint64_t n_frames;   /* must equal th_stft_n_frames(n_samples, win, hop) */
    uint64_t spec_pitch; /* floats per row, >= height; 0 = dense (height).  Pitches that are multiples of
                            32 floats (128 B) keep every row cache-line aligned (th_pitch_f32). */
} th_chan_desc;

/* Batched calc_spec over n_chan independent channels (core/mod.rs:153-163 → spectrogram.rs:187-212):
 * reflect-centred framing → Hann/n_fft → real FFT → |X| → [mel] → 20*log10.
 * d_minmax (DEVICE, 2*n_chan f32, may be NULL) receives per-channel (min, max) of the dB values
 * (find_min_max, simd.rs:14-36), fused into the same launch.  Stream-ordered, no sync. */
TH_API int th_calc_spec_batch_dev(th_plan *plan, const th_chan_desc *chans, size_t n_chan, float *d_minmax);
/* The same, and the global dB range of these channels — max_dB = min(max, 0), min_dB = max(min, max_dB - dB_range),
 * core/mod.rs:169-180 — into d_range (DEVICE, 2 floats) in the same call: for a single GPU whose batch is the whole
 * project (one launch fewer than th_calc_spec_batch_dev + th_minmax_reduce_range_dev when the batch is one channel). */
TH_API int th_calc_spec_batch_ranged_dev(th_plan *plan, const th_chan_desc *chans, size_t n_chan, float *d_minmax,
                                         float dB_range, float *d_range);

/* Single-channel convenience with HOST buffers (upload, compute, download; synchronous).
 * out_spec[n_frames * height]; out_min/out_max may be NULL. */
TH_API int th_calc_spec_host(th_plan *plan, const float *wav, size_t n_samples, float *out_spec,
                             size_t out_capacity_floats, size_t *n_frames, float *out_min, float *out_max);

/* ---------------------------------------------------------------- f32 dB spec → u16 grey image */
/* convert_spectrogram_to_img — visualize/drawing.rs:4-33.
 * d_spec: n_frames x height f32; d_img: (i_end - i_start) x n_frames u16 (row 0 = lowest frequency).
 * colormap_len = 0 means None. */
TH_API int th_spec_to_img_dev(th_ctx *ctx, const float *d_spec, size_t n_frames, size_t height, size_t i_start,
                              size_t i_end, float min_dB, float max_dB, uint32_t colormap_len, uint16_t *d_img);

typedef struct {
    const float *spec; /* DEVICE */
    uint16_t *img;     /* DEVICE */
    uint64_t n_frames, height, i_start, i_end;
    uint64_t spec_pitch; /* floats per spec row, 0 = dense (height) */
    uint64_t img_pitch;  /* u16 per image row, 0 = dense (n_frames); multiples of 64 recommended (th_pitch_u16).
                          * NOTE: when img_pitch is a multiple of 64 and img_pitch - n_frames < 64 — i.e. exactly the
                          * library's own padded pitch th_pitch_u16(n_frames) — the kernel owns the row padding and
                          * writes zeros into columns [n_frames, img_pitch) (a whole 128-byte line per store instead of a
                          * read-modify-write).  An image that is a sub-rectangle of a wider surface must therefore use a
                          * pitch with at least 64 columns to the right of it, or a pitch that is not a multiple of 64;
                          * with any such pitch nothing outside [0, n_frames) of a row is written. */
} th_img_desc;
/* batched form: one launch for many channels sharing (min_dB, max_dB, colormap_len) — core/mod.rs:204-227 */
TH_API int th_spec_to_img_batch_dev(th_ctx *ctx, const th_img_desc *descs, size_t n, float min_dB, float max_dB,
                                    uint32_t colormap_len);
/* same with the range left on the device by th_global_db_range_dev (no host round trip between the STFT stage
 * and the quantiser); an all -inf range zero-fills the images as drawing.rs:16-18 */
TH_API int th_spec_to_img_batch_dev_ranged(th_ctx *ctx, const th_img_desc *descs, size_t n, const float *d_range,
                                           uint32_t colormap_len);

/* Quantise + level-0 raster in one pass over the f32 spec (round 4): what th_spec_to_img_batch_dev[_ranged] followed by
 * th_raster_tiles_dev over EVERY level-0 tile of every image produces — the same u16 images, the same RGBA tiles, bit for
 * bit — moving 10 bytes per pixel instead of 6 + 6 (drawing.rs:4-33 + render_tiles.rs:290-351).
 * tiles: HOST array of n_tiles_x * n_tiles_y DEVICE pointers, tile (tx, ty) of the level-0 grid of the (i_end - i_start) x
 * n_frames image (th_spectrogram_tile_geometry with levels 0) at [tx * n_tiles_y + ty]: a dense width x height RGBA8 array,
 * top row = highest frequency, 4-byte aligned (16-byte aligned bases are faster); NULL entries are skipped.
 * d_range != NULL: [min_dB, max_dB] on the DEVICE (th_global_db_range_dev), else the host values.  d_colormap: DEVICE RGBA8
 * LUT of n_colors entries (1 .. 65536), 4-byte aligned; the quantiser's colormap_len is n_colors. */
typedef struct {
    th_img_desc img;
    uint8_t *const *tiles; /* HOST array of DEVICE pointers */
    uint32_t n_tiles_x, n_tiles_y; /* ceil(n_frames / 512), ceil((i_end - i_start) / 512) */
} th_img_tiles_desc;
TH_API int th_spec_to_img_raster_batch_dev(th_ctx *ctx, const th_img_tiles_desc *descs, size_t n, float min_dB, float max_dB,
                                           const float *d_range, const uint8_t *d_colormap, uint32_t n_colors);

/* ---------------------------------------------------------------- tiles */
/* encode_spectrogram_tile — render_tiles.rs:281-352.  d_img: img_height x img_width u16 (DEVICE).
 * colormap: HOST RGBA8 bytes.  Writes the 40-byte LE header + RGBA (top row = highest frequency)
 * to the HOST buffer `out`.  Level (0,0) is an exact crop copy; level > 0 uses a separable
 * Lanczos3 resample in the arithmetic of Pillow's ImagingResample: bit-identical to Pillow 12.2's 16-bit resize on the
 * committed fixtures, formally unpinned vs fast_image_resize itself. */
TH_API int th_encode_spectrogram_tile_dev(th_ctx *ctx, const uint16_t *d_img, size_t img_height, size_t img_width,
                                          size_t img_pitch /* u16 per row, 0 = dense */,
                                          const uint8_t *colormap_rgba, size_t colormap_bytes, uint64_t revision,
                                          uint32_t level_x, uint32_t level_y, uint32_t tile_x, uint32_t tile_y,
                                          uint8_t *out, size_t out_capacity, size_t *out_len);

typedef struct {
    const uint16_t *img;  /* DEVICE: img_height x img_width */
    uint8_t *rgba;        /* DEVICE: height x width x 4, top row = highest frequency; 4-byte aligned (tiles may be
                           * packed back to back: the kernel lays its 16-byte stores on the address grid) */
    uint32_t img_width, img_height;
    uint32_t origin_x, origin_y, width, height; /* level-0 tile rectangle (th_spectrogram_tile_geometry) */
    uint32_t img_pitch;                         /* u16 per image row, 0 = dense (img_width) */
    uint32_t reserved;
} th_raster_desc;
/* Batched level-0 colormap raster of many tile rectangles in one launch (device → device).
 * d_colormap: DEVICE RGBA8, n_colors entries, 4-byte aligned. */
TH_API int th_raster_tiles_dev(th_ctx *ctx, const th_raster_desc *descs, size_t n, const uint8_t *d_colormap,
                               uint32_t n_colors);

/* encode_waveform_tile — render_tiles.rs:232-279.  d_wav: DEVICE samples.  Writes the 24-byte LE
 * header + bins x (min, max, mean) f32 to the HOST buffer `out`. */
TH_API int th_encode_waveform_tile_dev(th_ctx *ctx, const float *d_wav, size_t n_samples, uint64_t revision,
                                       uint32_t level, uint32_t tile_index, uint8_t *out, size_t out_capacity,
                                       size_t *out_len);

typedef struct {
    const float *wav; /* DEVICE */
    float *bins;      /* DEVICE: bin_count x 3 f32 (min, max, mean) */
    uint64_t n_samples;
    uint64_t start;   /* first sample of the tile */
    uint32_t level;
    uint32_t bin_count;
} th_wave_desc;
/* Batched waveform decimation (many tiles / levels / channels in one launch, device → device). */
TH_API int th_waveform_tiles_dev(th_ctx *ctx, const th_wave_desc *descs, size_t n);

/* Channel statistics upstream of the path: sum of squares and absolute peak per channel in one
 * pass — simd.rs:113-183 sum_squares / abs_max as StatCalculator::calc uses them (dynamics/stats.rs:56-86:
 * mean_squared = Σ_ch sum_squares / n_elem, max_peak = max_ch abs_max).  Results are written to HOST arrays. */
typedef struct {
    const float *wav; /* DEVICE */
    uint64_t n_samples;
} th_stats_desc;
TH_API int th_channel_stats_dev(th_ctx *ctx, const th_stats_desc *descs, size_t n, float *out_sum_squares,
                                float *out_abs_max);

/* Loudness of whole tracks — StatCalculator::calc (dynamics/stats.rs:56-86), the AudioStats behind get_global_lufs, get_rms_dB and
 * get_max_peak_dB (lib.rs:463-489).  global_lufs: EBU R128 integrated loudness as the ebur128 crate computes it with Mode::all()
 * (histogram gating: 0.1 LU bins; K-weighting in f64; default channel map: 4 ch L R Ls Rs, 5 ch L R C Ls Rs, otherwise channel 3 and
 * channels from 6 on unused, Ls / Rs weigh 1.41); -inf when no 400 ms block passes the gates.  rms_dB = 10 log10(sum of squares over
 * all channels / (n_channels n_samples)) and max_peak_dB = 20 log10(max |x|), both in f32 (0 gives -inf, NaN stays NaN; no samples
 * give rms_dB = NaN, max_peak = 0, max_peak_dB = -inf). */
typedef struct {
    double global_lufs;
    float rms_dB;
    float max_peak;
    float max_peak_dB;
    uint32_t reserved[3];
} th_audio_stats;
typedef struct {
    const float *const *channels; /* HOST array of n_channels DEVICE pointers (n_samples f32 each) */
    uint64_t n_samples;
    uint32_t n_channels;          /* >= 1 */
    uint32_t sr;                  /* 16 .. 2 822 400 (the rates EbuR128::new accepts), else TH_ERR_UNSUPPORTED */
    double *block_energy;         /* DEVICE, 8-byte aligned, may be NULL: receives the th_loudness_n_blocks values E_k of the momentary (400 ms, hop
                                   * 100 ms) series, E_k = sum_c w_c sum_(block) y_c^2 / block length, in stream order */
} th_audio_desc;
/* A batch of tracks; out_host[n].  Returns to the host: synchronises the context's stream. */
TH_API int th_audio_stats_dev(th_ctx *ctx, const th_audio_desc *descs, size_t n, th_audio_stats *out_host);
/* The host arithmetic around it (no GPU).  th_k_weighting: the 4th-order K-weighting section at rate sr, b[5] and a[5] (a[0] = 1),
 * designed as libebur128 does; TH_ERR_UNSUPPORTED outside 16 .. 2 822 400 Hz.  th_loudness_n_blocks: (n - 4 s100) / s100 + 1 blocks
 * of 4 s100 samples, s100 = (sr + 5) / 10, or 0 when n < 4 s100.  th_gated_loudness: integrated LUFS of a block-energy series
 * (histogram-mode absolute and relative gates; NaN energies never count). */
TH_API int th_k_weighting(uint32_t sr, double b[5], double a[5]);
TH_API int th_loudness_n_blocks(size_t n_samples, uint32_t sr, size_t *n_blocks);
TH_API int th_gated_loudness(const double *block_energies, size_t n, double *lufs);

/* Waveform pyramid: every decimation level of a channel from one pass over the audio.  Level L
 * (samples per bin 2^L, exactly the bins encode_waveform_tile emits for that level — render_tiles.rs:232-279)
 * has th_waveform_pyramid_bins(n, L) = ceil(n / 2^L) bins of (min, max, mean) f32 and starts at float offset
 * th_waveform_pyramid_offset(n, L) of `out` (every level starts on a 128-byte boundary: the offsets are multiples of 32
 * floats, with up to 31 unused floats behind a level); tile t of level L is bins [1024 t, 1024 (t + 1)) of that level.
 * `out` must hold th_waveform_pyramid_offset(n, n_levels) floats.
 * first_level = F in {1, 2}: levels below F are NOT materialised — level 0 is (x, x, x) per sample, half of all the
 * pyramid's bytes, level 1 a quarter, and a tile of either is no larger as samples (4 / 8 KB) than as bins (12 KB): the
 * TrackManager serves them from the resident audio — and the layout starts at level F: level L >= F at float offset
 * th_waveform_pyramid_offset(n, L) - th_waveform_pyramid_offset(n, F); `out` holds
 * th_waveform_pyramid_offset(n, n_levels) - th_waveform_pyramid_offset(n, F) floats. */
typedef struct {
    const float *wav; /* DEVICE */
    float *out;       /* DEVICE */
    uint64_t n_samples;
    uint32_t n_levels; /* levels 0 .. n_levels-1, at most 40 */
    uint32_t first_level; /* 0 (all levels), 1 or 2 (levels first_level .. n_levels-1); > 2: TH_ERR_INVALID_ARG.  ABI note:
                           * this field was `reserved` (unvalidated) before round 3 — callers must zero it */
} th_pyramid_desc;
TH_API size_t th_waveform_pyramid_bins(uint64_t n_samples, uint32_t level);
TH_API size_t th_waveform_pyramid_offset(uint64_t n_samples, uint32_t level);
TH_API int th_waveform_pyramid_dev(th_ctx *ctx, const th_pyramid_desc *descs, size_t n);

/* ---------------------------------------------------------------- waveform-tile cache (host only, no GPU needed) */
/* Mirror of RenderTileCache — src-tauri/src/core/render_tiles.rs:51-230: a byte-budgeted LRU of encoded
 * waveform tiles keyed by (id, ch, waveform_revision, level, tile_index) plus the waveform / spectrogram
 * revision counters.  th_tm_* owns one; hosts that keep thesia's own lib.rs:342-367 flow can use it directly. */
typedef struct th_tile_cache th_tile_cache;
/* budget_bytes = 0 selects DEFAULT_WAVEFORM_CACHE_BUDGET_BYTES (32 MiB, render_tiles.rs:17) */
TH_API int th_tile_cache_create(size_t budget_bytes, th_tile_cache **out);
TH_API int th_tile_cache_destroy(th_tile_cache *cache);
/* cached_waveform_tile (:124-144): *revision = current waveform revision; *hit = 1 and the bytes on a hit
 * (which also makes the entry most recently used) */
TH_API int th_tile_cache_lookup(th_tile_cache *cache, size_t id, uint32_t ch, uint32_t level, uint32_t tile_index,
                                uint64_t *revision, uint8_t *out, size_t out_capacity, size_t *out_len, int *hit);
/* store_waveform_tile (:146-169): ignored when `revision` is no longer current; evicts least recently used
 * entries until the budget holds (:205-218) */
TH_API int th_tile_cache_store(th_tile_cache *cache, size_t id, uint32_t ch, uint64_t revision, uint32_t level,
                               uint32_t tile_index, const uint8_t *bytes, size_t len);
/* invalidate_waveform (bumps the revision, drops every tile) / invalidate_spectrogram (:87-99) */
TH_API int th_tile_cache_invalidate(th_tile_cache *cache, int waveform, int spectrogram);
TH_API int th_tile_cache_set_budget(th_tile_cache *cache, size_t budget_bytes);
/* any out pointer may be NULL */
TH_API int th_tile_cache_stats(const th_tile_cache *cache, size_t *entries, size_t *bytes, size_t *budget_bytes,
                               uint64_t *waveform_revision, uint64_t *spectrogram_revision, uint64_t *hits,
                               uint64_t *misses);

/* ---------------------------------------------------------------- TrackManager mirror (layer B, host buffers) */
/* Mirrors core/mod.rs:33-230 with decoded audio handed over as planar host f32 (the output of
 * the reference's decode step, audio.rs:65-78).  Audio, f32 dB specs and u16 images stay
 * resident in HBM, so set_dB_range / set_colormap re-quantise without redoing the STFT. */
TH_API int th_tm_create(th_ctx *ctx, th_tm **out);
TH_API int th_tm_destroy(th_tm *tm);
/* init(colormap_rgba) — lib.rs:51-98, render_tiles.rs:80-85; sets colormap_length = bytes/4 */
TH_API int th_tm_set_colormap(th_tm *tm, const uint8_t *rgba, size_t bytes);
/* TrackManager::set_setting — core/mod.rs:107-115 (recomputes every resident track).  Transactional: when the new
 * setting cannot be planned (this library takes every n_fft = next_pow2(win) * f_overlap up to TH_MAX_N_FFT = 2^20 — any
 * f_overlap since round 6; beyond the limit, or with a mel filterbank above 1 GiB, TH_ERR_UNSUPPORTED) or memory runs out, the call
 * fails and the manager — settings, plans,
 * specs, images, revisions — is exactly as before.  th_tm_add_tracks gives the same guarantee. */
TH_API int th_tm_set_setting(th_tm *tm, double win_ms, uint32_t t_overlap, uint32_t f_overlap, int freq_scale);
/* TrackManager::set_dB_range — core/mod.rs:123-126 */
TH_API int th_tm_set_dB_range(th_tm *tm, float dB_range);
/* TrackList::add_tracks + TrackManager::add_tracks — core/mod.rs:62-71.
 * channels[c] points to n_samples f32 of channel c (planar). */
TH_API int th_tm_add_track(th_tm *tm, size_t id, uint32_t sr, uint32_t n_channels, const float *const *channels,
                           size_t n_samples);
/* batch form: computes all added tracks' specs in one launch per plan */
TH_API int th_tm_add_tracks(th_tm *tm, size_t n_tracks, const size_t *ids, const uint32_t *srs,
                            const uint32_t *n_channels, const float *const *channels_flat,
                            const size_t *n_samples);
TH_API int th_tm_remove_track(th_tm *tm, size_t id);
/* TrackManager::apply_track_list_changes — core/mod.rs:102-105,168-230.
 * updated_ids (may be NULL) receives up to cap ids whose images were re-made. */
TH_API int th_tm_apply_track_list_changes(th_tm *tm, size_t *updated_ids, size_t cap, size_t *n_updated,
                                          uint32_t *max_sr);
TH_API int th_tm_get_db_state(const th_tm *tm, float *min_dB, float *max_dB, uint32_t *max_sr);
/* shapes and copy-out accessors (parity tests, get_audio_render_metadata lib.rs:321-340) */
TH_API int th_tm_spec_shape(const th_tm *tm, size_t id, uint32_t ch, size_t *n_frames, size_t *height);
TH_API int th_tm_img_shape(const th_tm *tm, size_t id, uint32_t ch, size_t *img_height, size_t *img_width);
TH_API int th_tm_copy_spec(th_tm *tm, size_t id, uint32_t ch, float *out, size_t capacity_floats);
TH_API int th_tm_copy_img(th_tm *tm, size_t id, uint32_t ch, uint16_t *out, size_t capacity_px);
TH_API int th_tm_revisions(const th_tm *tm, uint64_t *waveform_revision, uint64_t *spectrogram_revision);
/* get_spectrogram_tile / get_waveform_tile — lib.rs:342-389 */
TH_API int th_tm_get_spectrogram_tile(th_tm *tm, size_t id, uint32_t ch, uint32_t level_x, uint32_t level_y,
                                      uint32_t tile_x, uint32_t tile_y, uint8_t *out, size_t out_capacity,
                                      size_t *out_len);
TH_API int th_tm_get_waveform_tile(th_tm *tm, size_t id, uint32_t ch, uint32_t level, uint32_t tile_index,
                                   uint8_t *out, size_t out_capacity, size_t *out_len);
/* Many spectrogram tiles in one call (the initial paint of a view, a zoom that invalidates every visible tile): ONE raster
 * launch and one transfer for all of them instead of a launch + synchronisation per tile.  Tile i is written at
 * out + offsets[i] as the very bytes th_tm_get_spectrogram_tile returns for it (40-byte header + RGBA); records start on
 * 64-byte boundaries, offsets[n] = bytes used, *out_len = bytes needed (TH_ERR_BUFFER_TOO_SMALL when out_capacity is
 * less; out may then be NULL to query the size).  When `out` is pinned host memory (th_host_alloc, or memory the caller
 * registered with HIP) the kernel writes it directly over PCIe; otherwise the tiles pass through a pinned staging buffer
 * of the manager and are copied.  The reference's consumer asks tile by tile (lib.rs:369-389); a host that wants the
 * batch sends its visible-tile list once instead. */
typedef struct {
    size_t id;
    uint32_t ch, level_x, level_y, tile_x, tile_y;
    uint32_t reserved; /* 0 */
} th_tile_request;
TH_API int th_tm_get_spectrogram_tiles(th_tm *tm, const th_tile_request *reqs, size_t n, uint8_t *out, size_t out_capacity,
                                       size_t *offsets /* n + 1 */, size_t *out_len);
/* pinned, device-visible host memory for tile batches (and for audio handed to th_tm_add_tracks: uploads from pinned
 * memory run at PCIe speed) */
TH_API int th_host_alloc(th_ctx *ctx, size_t bytes, void **ptr);
TH_API int th_host_free(th_ctx *ctx, void *ptr);
/* AudioRenderMetadata — render_tiles.rs:36-49, filled as RenderTileCache::metadata (:101-122) does for
 * get_audio_render_metadata (lib.rs:321-340).  track_sec and is_clipped come from the reference's TrackList
 * (decode / clip guard, upstream of this path) and are passed through unchanged; an absent spectrogram gives
 * width = height = 0 (`unwrap_or_default`, :109). */
typedef struct {
    uint64_t waveform_revision, spectrogram_revision;
    uint32_t sample_rate;
    uint32_t is_clipped;
    uint64_t sample_count;
    double track_sec;
    uint64_t spectrogram_width, spectrogram_height;
    uint64_t waveform_tile_bins;    /* WAVEFORM_TILE_BINS = 1024, :14 */
    uint64_t spectrogram_tile_size; /* SPECTROGRAM_TILE_SIZE = 512, :15 */
} th_render_metadata;
TH_API int th_tm_get_audio_render_metadata(th_tm *tm, size_t id, uint32_t ch, double track_sec, int is_clipped,
                                           th_render_metadata *out);
/* AudioStats of a resident track (get_global_lufs / get_rms_dB / get_max_peak_dB, lib.rs:463-489): computed by th_tm_add_tracks from
 * the uploaded samples, replaced when the id is added again, dropped by remove_track, untouched by every other call.  A reader: no
 * GPU work.  TH_ERR_NOT_FOUND when the id is not resident (the reference then answers -inf); a track whose rate the ebur128 crate
 * refuses (outside 16 .. 2 822 400 Hz) has global_lufs = NaN. */
TH_API int th_tm_get_audio_stats(th_tm *tm, size_t id, th_audio_stats *out);
/* the RenderTileCache in front of get_waveform_tile (lib.rs:350-366): borrowed, owned by tm */
TH_API int th_tm_tile_cache(th_tm *tm, th_tile_cache **out);
/* Spectrogram tiles with level_x or level_y > 0 (resize_spectrogram_tile, render_tiles.rs:354-393).
 * Default (per_request = 0): every channel's image gets a mip pyramid when it is (re)made — the whole image resized
 * to ceil(W / 2^lx) x ceil(H / 2^ly) with the separable Lanczos3 — and a LOD tile is a crop of that level + colour
 * LUT, like a level-0 tile.  per_request = 1: the reference's own flow, the tile's crop box is
 * resampled from the level-0 image on every request (also used for levels the pyramid does not hold: images
 * smaller than 16 px at that level); the pyramids are then not kept at all (and come back with per_request = 0).  The
 * two routes agree on whole tiles, core and gutter — both clip the filter at the image, never at the crop box — up to one
 * u16 step in rare pixels (f64 rounding of the tap centres).  PARITY UNPINNED against fast_image_resize in both modes. */
TH_API int th_tm_set_lod_source(th_tm *tm, int per_request);
/* shape of (and, with out != NULL, a dense copy of) one resident mip level; (0, 0) is the image itself */
TH_API int th_tm_mip_level(th_tm *tm, size_t id, uint32_t ch, uint32_t level_x, uint32_t level_y, uint16_t *out,
                           size_t capacity_px, size_t *width, size_t *height);
/* device memory the manager holds besides audio, specs and images (accounting / leak checks): the Lanczos tap tables of
 * the pyramid passes (one per (axis length, level) some resident image needs; dropped with the last such image) and the
 * mip pyramids.  Any out pointer may be NULL. */
TH_API int th_tm_lod_footprint(th_tm *tm, size_t *n_axis_tables, size_t *axis_table_bytes, size_t *mip_bytes);

/* ---------------------------------------------------------------- common normalisation and clip guarding */
/* set_common_normalize / set_common_guard_clipping — lib.rs:287-319 -> track.rs:152-171,329-337,432-436 -> audio.rs:50-63,133-179
 * -> dynamics/{normalize,guardclipping,limiter,envelope,stats}.rs, on the resident audio.  A track keeps its ORIGINAL samples as
 * they were added; its AUDIO (what the spectrogram is made from and th_tm_get_audio_stats describes) is derived from them:
 *   gain = th_normalize_gain(kind, target, stats of the original).  gain == 1 or not finite (Off, a silent track, a NaN target):
 *   the audio IS the original — no second copy, result GlobalGain(1), default guard stats (AudioTrack::apply_gain, track.rs:158-170).
 *   Otherwise y = gain * x in f32 and the guard: TH_GUARD_CLIP keeps y as the before-clip audio (which the waveform is then drawn
 *   from) and clamps to [-1, 1]; TH_GUARD_REDUCE_GLOBAL_LEVEL scales by 1 / peak when the peak is above 1; TH_GUARD_LIMITER runs
 *   PerfectLimiter::with_default (threshold 1, attack 5 ms, hold 15 ms, release 40 ms, three box filters) when the peak is above 1.
 * Defaults: TH_NORM_OFF and TH_GUARD_REDUCE_GLOBAL_LEVEL (track.rs:203-204); with them every other call returns what it returned
 * before these entries existed and no extra device memory is held.  th_tm_add_tracks derives new tracks under the common
 * settings.  A setter re-derives every track, recomputes pyramids, stats, specs and images, and bumps both revisions once
 * (invalidate_all); like set_setting it is transactional.  An unknown kind / mode: TH_ERR_INVALID_ARG, nothing changed.
 * The limiter needs sr >= 100 (an attack of at least one sample), else TH_ERR_UNSUPPORTED. */
#define TH_NORM_OFF 0
#define TH_NORM_LUFS 1
#define TH_NORM_RMS_DB 2
#define TH_NORM_PEAK_DB 3
#define TH_GUARD_CLIP 0
#define TH_GUARD_REDUCE_GLOBAL_LEVEL 1
#define TH_GUARD_LIMITER 2
/* which GuardClippingResult a track holds (guardclipping.rs:24-29) */
#define TH_GUARD_RESULT_GLOBAL_GAIN 0
#define TH_GUARD_RESULT_BEFORE_CLIP 1
#define TH_GUARD_RESULT_GAIN_SEQUENCE 2
/* Host only.  th_normalize_gain: 10f32.powf((target - stat) / 20) in f32, stat = global_lufs (cast to f32 first), rms_dB or
 * max_peak_dB of the ORIGINAL (normalize.rs:23-45); Off gives 1.  th_limiter_params: what PerfectLimiter::with_default(sr) runs
 * with — attack = round(5 sr / 1000), hold_length = round(20 sr / 1000) (half away from zero), release_samples = 40 sr / 1000 and
 * the three box lengths of BoxStackFilter::set(attack) (envelope.rs:229-265; their sum is attack + 2). */
typedef struct {
    uint32_t attack, hold_length;
    double release_samples;
    uint32_t box_len[3];
    uint32_t reserved;
} th_limiter_desc;
TH_API int th_normalize_gain(int kind, float target, const th_audio_stats *orig, float *gain);
TH_API int th_limiter_params(uint32_t sr, th_limiter_desc *out);
typedef struct {
    float normalize_gain;       /* the gain that was used (1 when the audio is the original) */
    int32_t guard_result;       /* TH_GUARD_RESULT_* */
    float global_gain;          /* GlobalGain's value (1 under the other results) */
    uint32_t draws_before_clip; /* 1: waveform tiles come from the before-clip audio (channel_for_drawing, audio.rs:70-78) */
} th_track_dynamics;
typedef struct { /* GuardClippingStats, stats.rs:111-174 */
    float max_reduction_gain_dB;
    uint32_t reserved;
    uint64_t reduction_cnt;
} th_guard_clip_stats;
TH_API int th_tm_set_common_normalize(th_tm *tm, int kind, float target);
TH_API int th_tm_set_common_guard_clipping(th_tm *tm, int mode);
TH_API int th_tm_get_common_dynamics(th_tm *tm, int *kind, float *target, int *mode); /* any out pointer may be NULL */
TH_API int th_tm_get_track_dynamics(th_tm *tm, size_t id, th_track_dynamics *out);
/* the entries format_guard_clip_stats selects (audio.rs:94-111): one per channel under TH_GUARD_CLIP, else one.  *n = entries
 * there are; TH_ERR_BUFFER_TOO_SMALL when cap is less (out may then be NULL) */
TH_API int th_tm_get_guard_clip_stats(th_tm *tm, size_t id, th_guard_clip_stats *out, size_t cap, size_t *n);
/* guard_clipping_gain (audio.rs:80-92): *n = 0 when the track holds no gain sequence, 1 ([1.0]) when no gain is below 1, else
 * n_samples f32 gains.  TH_ERR_BUFFER_TOO_SMALL when cap is less than *n (out may then be NULL) */
TH_API int th_tm_get_limiter_gain(th_tm *tm, size_t id, float *out, size_t cap, size_t *n);
/* n_samples f32 of one channel: which = 0 the audio (what the spectrogram is made from), 1 the audio the waveform is drawn from
 * (channel_for_drawing), 2 the original */
TH_API int th_tm_copy_audio(th_tm *tm, size_t id, uint32_t ch, int which, float *out, size_t cap);

/* ---------------------------------------------------------------- spectrum of a time range */
/* The per-channel spectrum over a time range, on the channel's own frequency axis (linear bins or the Mel bank): what upstream's
 * planned "average FFT magnitude", "region selection" and "export as figures" need.  No reference implementation exists; the
 * definition is this one.  For the resident spec s[t][h] of a channel (f32 dB, frame-major, the values th_tm_copy_spec returns,
 * unclamped), frames [f0, f1), n = f1 - f0, column h:
 *   TH_SPECTRUM_MEAN_AMP    20 log10((1 / n) sum_t 10^(s / 20))
 *   TH_SPECTRUM_MEAN_POWER  10 log10((1 / n) sum_t 10^(s / 10))
 *   TH_SPECTRUM_MAX         max_t s
 * H = the spec's height f32 values, index 0 the lowest frequency.  A row value of -inf is amplitude 0 and still counts in n; a
 * column that is all -inf gives -inf; a NaN anywhere in the column's range gives NaN under every kind; n = 0 gives a row of NaN.
 * The sums are f64 in a fixed order, 10^x to f32 accuracy: a mean is within max(2e-5 dB, 2 f32 ulps) of the f64 evaluation, the
 * maximum is exact (where a column's maximum is zero and the range holds both +0 and -0, which of the two is returned is not
 * specified).
 * Frames from seconds (tracks of one project differ in rate and hop): frame t is centred on sample t hop and is selected when
 * its centre lies in [start_sec, end_sec): f0 = clamp(ceil(start_sec sr / hop), 0, T); f1 = T for end_sec = +inf, else
 * max(f0, clamp(ceil(end_sec sr / hop), 0, T)); the arithmetic is C double, (sec * (double)sr) / (double)hop.
 * th_spectrum_frame_range (host only) is that definition; TH_ERR_INVALID_ARG when start_sec is NaN, negative or infinite,
 * end_sec is NaN or below start_sec, or sr or hop is zero.
 * th_tm_get_spectra: rows packed dense, back to back, in request order; info[i] says where row i starts, its length, the frames
 * it covers and the spectrogram revision it belongs to (a host caches by it).  *out_len = floats needed; TH_ERR_BUFFER_TOO_SMALL
 * when cap_floats is less, with info and *out_len filled (out may then be NULL to query the size).  An unknown id or a channel
 * without a resident spec: TH_ERR_NOT_FOUND; a channel the track does not have, an unknown kind or a bad time:
 * TH_ERR_INVALID_ARG; the first faulty request in request order decides; on any error nothing is written to out.  These are
 * readers, like the tile getters: they share the lock, run on a reader slot's own stream and wait for no other reader — except
 * when a slot's scratch grows (the first call, or a batch larger than any before on that slot): the allocation waits for the
 * device.  Scratch (partial sums, and a result buffer for results above the slot's pinned staging) is made on the first call and
 * only grows; a manager that never calls them holds none.  A request's values
 * depend on its rows, range and kind only — not on the rest of the batch, the slot, the call, or th_tm against th_tmg.
 * th_tm_get_spectrum: one request; info may be NULL (info->height is the size needed on TH_ERR_BUFFER_TOO_SMALL). */
#define TH_SPECTRUM_MEAN_AMP 0
#define TH_SPECTRUM_MEAN_POWER 1
#define TH_SPECTRUM_MAX 2
typedef struct {
    size_t id;
    uint32_t ch;
    uint32_t kind; /* TH_SPECTRUM_* */
    double start_sec, end_sec;
} th_spectrum_request;
typedef struct {
    uint64_t offset; /* floats into out */
    uint64_t height; /* H of that channel's spec */
    uint64_t frame_start, frame_end;
    uint64_t spectrogram_revision;
} th_spectrum_info;
TH_API int th_spectrum_frame_range(uint32_t sr, size_t hop, size_t n_frames, double start_sec, double end_sec,
                                   size_t *frame_start, size_t *frame_end);
TH_API int th_tm_get_spectra(th_tm *tm, const th_spectrum_request *reqs, size_t n, float *out, size_t cap_floats,
                             th_spectrum_info *info /* n */, size_t *out_len);
TH_API int th_tm_get_spectrum(th_tm *tm, size_t id, uint32_t ch, int kind, double start_sec, double end_sec, float *out,
                              size_t cap_floats, th_spectrum_info *info);

/* ---------------------------------------------------------------- loudness meter of resident tracks */
/* What an R128 loudness display shows beside the integrated value of th_tm_get_audio_stats, computed from a track's AUDIO (the
 * derived audio while a normalise gain is in force, else the original): true peak, loudness range, maximum momentary and
 * short-term loudness, and the two curves along the track.  No reference implementation exists (upstream reads loudness_global
 * only); the arithmetic is libebur128's, restated, and these definitions are the contract:
 *   s100 = (sr + 5) / 10, n_seg = n_samples / s100, q_c[k] = the K-weighted energy (sum of y^2) of segment k of channel c, w_c the
 *   channel map of th_audio_stats.  Momentary M_k = sum_c w_c (q_c[k] + .. + q_c[k + 3]) / (4 s100), k <= n_seg - 4: the values and
 *   bits of th_audio_desc.block_energy.  Short-term S_k = sum_c w_c (q_c[k] + .. + q_c[k + 29]) / (30 s100), k <= n_seg - 30.  f64,
 *   segments summed in ascending order per channel, then the channels in ascending order.  A series is returned as LUFS,
 *   10 log10(E) - 0.691 in f64 (E = 0: -inf; NaN stays NaN); max_*_lufs is the largest non-NaN value, -inf when there is none.
 *   loudness_range (EBU Tech 3342) takes S_0, S_10, S_20, .. (one 3 s block per second) through the 1000 histogram bins of the
 *   integrated loudness: blocks below -70 LUFS and NaN never count; the relative gate is 0.01 of the mean bin energy; of what passes,
 *   lo = (size_t)((size - 1) 0.1 + 0.5) and hi = (size_t)((size - 1) 0.95 + 0.5) index the sorted blocks, and the range is
 *   10 log10(E_hi) - 10 log10(E_lo) of their bins' centres; 0 when nothing passes.  th_loudness_range (host) is that definition.
 *   true_peak: the oversampling factor F is 4 for sr < 96000, 2 for sr < 192000, else 1 (then true_peak = max_peak).  The
 *   interpolator has 49 taps, c_j = sinc((j - 24) pi / F) 0.5 (1 - cos(2 pi j / 48)) in f64, kept when |c_j| > 1e-6; tap j belongs
 *   to phase j mod F with delay j div F (th_true_peak_filter lists the kept taps in ascending j).  y_f[i] = sum_d c x[i - d] for
 *   i in [0, n_samples), x[i < 0] = 0, nothing behind the last sample; on the device the coefficients are f32 and a phase is one
 *   fmaf chain in ascending delay from 0.  true_peak = the largest |y| over channels, phases and i (NaN ignored; 0 for silence),
 *   true_peak_dB = 20 log10 of it, taken in f64 and rounded once; true_peak_channel = the lowest channel that attains it.
 * A track at a rate outside 16 .. 2 822 400 Hz (global_lufs = NaN) has no series: both counts are 0 and loudness_range and the two
 * maxima are NaN; its true peak is still measured.
 * th_tm_get_loudness_meters: meters[i] describes ids[i] (an id may repeat).  The series are f64 LUFS packed dense in request order,
 * within a track the momentary series, then the short-term one; the offsets and counts are in the meter and *out_len is the number
 * of doubles needed.  series == NULL: the series are not wanted, which is no error: the meters are filled, with counts and
 * offsets.  A non-NULL series with cap_doubles < *out_len: TH_ERR_BUFFER_TOO_SMALL, nothing is written to series; the meters then
 * carry the counts, offsets, oversampling and revision only.  An unknown id: TH_ERR_NOT_FOUND; a NULL handle, NULL ids with n > 0,
 * NULL meters or NULL out_len: TH_ERR_INVALID_ARG; the first faulty request decides and nothing is written.  A reader like
 * th_tm_get_spectra: shared lock, a reader slot's own stream, one batched launch sequence for all ids; its scratch on the slot is
 * made on the first call and only grows.  Nothing is cached and nothing happens at add time: every call computes.  A track's
 * values depend on its audio alone - not on the batch, the slot, or th_tm against th_tmg.  waveform_revision: the revision the
 * values belong to (a host caches by it).
 * th_tm_get_loudness_meter: one id; the doubles needed are meter->n_momentary + meter->n_short_term. */
typedef struct {
    double loudness_range; /* LU */
    double max_momentary_lufs, max_short_term_lufs;
    float true_peak, true_peak_dB;
    uint32_t true_peak_channel, oversampling; /* 4, 2 or 1 */
    uint64_t momentary_offset, n_momentary;   /* doubles into `series` */
    uint64_t short_term_offset, n_short_term;
    uint64_t waveform_revision;
} th_loudness_meter;
TH_API int th_tm_get_loudness_meters(th_tm *tm, const size_t *ids, size_t n, th_loudness_meter *meters /* n */, double *series,
                                     size_t cap_doubles, size_t *out_len);
TH_API int th_tm_get_loudness_meter(th_tm *tm, size_t id, th_loudness_meter *meter, double *series, size_t cap_doubles);
/* The host arithmetic around it (no GPU).  th_true_peak_filter: the factor for sr and the kept taps in ascending j (coefficient,
 * phase, delay; arrays of 49).  th_loudness_n_short_term: n_seg - 29 blocks, or 0 when n_seg < 30; TH_ERR_UNSUPPORTED outside
 * 16 .. 2 822 400 Hz.  th_loudness_range: LU from the short-term ENERGIES taken once per second. */
TH_API int th_true_peak_filter(uint32_t sr, uint32_t *factor, double coef[49], uint32_t phase[49], uint32_t delay[49],
                               uint32_t *n_taps);
TH_API int th_loudness_n_short_term(size_t n_samples, uint32_t sr, size_t *n_blocks);
TH_API int th_loudness_range(const double *short_term_energies_1s, size_t n, double *lra);

/* ---------------------------------------------------------------- PCM / WAV export of resident tracks */
/* A time range of a track's resident audio as file-ready bytes, made on the device: the channels interleaved, quantised to 16- or
 * 24-bit PCM (with or without TPDF dither) or copied as float32, and the WAV header around them: the last step of normalise ->
 * guard -> save (upstream's planned "save normalized audio" and "region selection").  No reference implementation exists; these
 * definitions are the contract.
 *   Samples from seconds: s0 = clamp(ceil(start_sec sr), 0, n); s1 = n for end_sec = +inf, else max(s0, clamp(ceil(end_sec sr), 0,
 *   n)); C double arithmetic; the argument rules are those of th_spectrum_frame_range (th_audio_sample_range is that definition:
 *   TH_ERR_INVALID_ARG when start_sec is NaN, negative or infinite, end_sec is NaN or below start_sec, or sr is zero).
 *   Dither generator (th_export_dither), counter-based: fmix32(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35;
 *   h ^= h >> 16 in uint32.  k0 = fmix32(seed + 0x9e3779b9 (ch + 1)) mod 2^32; k1 = fmix32(hi32(i) ^ k0); k = fmix32(lo32(i) ^ k1);
 *   a = fmix32(k ^ 0x68bc21eb) >> 8; b = fmix32(k ^ 0x02e5be93) >> 8.  i is the ABSOLUTE sample index in the track, not the index
 *   inside the range: the bytes of a range are the same bytes cut from the whole-track export, and a host may export a long track in
 *   successive ranges and concatenate them.
 *   Quantiser (th_export_quantize, one channel): S = 32768 (TH_PCM_S16) or 8388608 (TH_PCM_S24); v = (double)x S + d, d = 0 under
 *   TH_DITHER_NONE and ((double)a - (double)b) 2^-24 under TH_DITHER_TPDF; q = rint(v), ties to even; a q outside [-S, S - 1] is
 *   clamped and counted in n_clamped (so is +-inf); a NaN sample gives 0 and is counted in n_nan.  Little-endian, 2 or 3 bytes.
 *   TH_PCM_F32 copies the sample's 4 bytes unchanged, NaN included: n_clamped = 0, n_nan is still counted, dither and seed are
 *   ignored (th_export_quantize then returns the bit patterns in q).
 *   Frames are interleaved: channel 0, 1, .. of sample s0, then of s0 + 1, and so on.
 *   WAV header (th_wav_header): PCM formats the canonical 44 bytes ("fmt " of 16 bytes, tag 1); TH_PCM_F32 58 bytes ("fmt " of 18
 *   bytes with tag 3 and cbSize 0, then a 12-byte "fact" chunk holding n_frames).  *pad_len is 1 when the data byte count is odd (24
 *   bit, odd n_ch n_frames): one zero byte behind the data, which the RIFF size counts and the "data" size does not.  A file whose
 *   RIFF size would exceed 2^32 - 1, more than 65535 channels, a block (n_ch x bytes per sample) above 65535 bytes or a byte rate
 *   above 2^32 - 1: TH_ERR_UNSUPPORTED.  n_ch == 0, sr == 0 or an unknown format: TH_ERR_INVALID_ARG.
 * th_tm_export_pcm: request i's bytes start at out + info[i].offset; the offsets are multiples of 16 in request order (offset[i + 1]
 * = offset[i] + n_bytes[i] rounded up to 16) and the up to 15 bytes of padding between two requests are written as ZERO; nothing is
 * written behind the last request's bytes, and *out_len = its offset + n_bytes.  The size query and the error rules are those of
 * th_tm_get_spectra: out == NULL or cap_bytes < *out_len gives TH_ERR_BUFFER_TOO_SMALL with info (offsets, sizes, sample ranges,
 * rate, channels, revision; the two counts zero) and *out_len filled; an unknown id: TH_ERR_NOT_FOUND; an unknown which, format or
 * dither or a bad time: TH_ERR_INVALID_ARG; a track of more than TH_EXPORT_MAX_CHANNELS channels: TH_ERR_UNSUPPORTED; the first
 * faulty request decides; on any of these errors nothing is written to out.  An empty range is valid: 0 bytes.
 * th_tm_export_wav: one request as a complete file image, header + data + pad; info (may be NULL) then has offset = the header's
 * length (44 or 58, not a multiple of 16) and n_bytes = the data bytes without the pad; an empty range gives a header-only file.
 * A request's bytes and counts depend on the track's audio and the request alone - not on the batch, the reader slot, the pieces
 * below, or th_tm against th_tmg.  waveform_revision: the revision the bytes belong to.
 * Readers, like th_tm_get_spectra: shared lock, a reader slot's own stream.  The device staging is BOUNDED: a call is processed in
 * pieces of at most TH_EXPORT_PIECE_BYTES output bytes, cut at frame boundaries, through two device buffers (piece p + 1 is computed
 * while piece p is copied into the caller's buffer).  A slot's export scratch is made on its first export and never exceeds two
 * pieces (each TH_EXPORT_PIECE_BYTES + 64 bytes) plus the job tables and counters of the largest call so far; a manager that never
 * exports holds none. */
#define TH_PCM_S16 0
#define TH_PCM_S24 1
#define TH_PCM_F32 2
#define TH_DITHER_NONE 0
#define TH_DITHER_TPDF 1
#define TH_WAV_HEADER_MAX 64
#define TH_EXPORT_PIECE_BYTES (32u << 20)
#define TH_EXPORT_MAX_CHANNELS 1024
typedef struct {
    size_t id;
    uint32_t which; /* as th_tm_copy_audio: 0 audio, 1 drawing, 2 original */
    uint32_t format, dither, seed; /* TH_PCM_*, TH_DITHER_* */
    double start_sec, end_sec;
} th_export_request;
typedef struct {
    uint64_t offset, n_bytes; /* into out */
    uint64_t sample_start, sample_end;
    uint32_t sr, n_channels;
    uint64_t n_clamped, n_nan, waveform_revision;
} th_export_info;
TH_API int th_audio_sample_range(uint32_t sr, size_t n_samples, double start_sec, double end_sec, size_t *sample_start,
                                 size_t *sample_end);
TH_API int th_export_dither(uint32_t seed, uint32_t ch, uint64_t i, uint32_t *a, uint32_t *b);
TH_API int th_export_quantize(uint32_t format, uint32_t dither, uint32_t seed, uint32_t ch, uint64_t first_index, const float *x,
                              size_t n, int32_t *q, uint64_t *n_clamped, uint64_t *n_nan);
TH_API int th_wav_header(uint32_t format, uint32_t sr, uint32_t n_ch, uint64_t n_frames, uint8_t out[TH_WAV_HEADER_MAX],
                         size_t *header_len, size_t *pad_len);
TH_API int th_tm_export_pcm(th_tm *tm, const th_export_request *reqs, size_t n, uint8_t *out, size_t cap_bytes,
                            th_export_info *info /* n */, size_t *out_len);
TH_API int th_tm_export_wav(th_tm *tm, const th_export_request *req, uint8_t *out, size_t cap_bytes,
                            th_export_info *info /* may be NULL */, size_t *out_len);

/* ---------------------------------------------------------------- Export at a target sample rate (polyphase sinc resampler) */
/* th_tm_export_pcm_at / th_tm_export_wav_at: th_tm_export_pcm / _wav with the audio converted to sr_out first, by a band-limited
 * resampler on the device, an exact rational polyphase FIR of the kind the reference's player runs on the CPU (player/stream.rs: a
 * rubato windowed-sinc resampler, sinc_len 256, BlackmanHarris2).  With TH_PCM_F32 the call is the player's interleaved float feed
 * at the device rate.  No reference implementation can be pinned; these definitions are the contract.
 *   Ratio and length.  g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, rho = min(1, L / M), Z = 128, FC = 0.95,
 *   K = Z when L >= M, else ceil(Z M / L); an output sample has 2K taps (th_resample_plan_for).
 *   Prototype, in input samples, C double: h(t) = rho FC sinc(rho FC t) w(rho t / Z); sinc(x) = sin(pi x) / (pi x), sinc(0) = 1;
 *   w(u) = b(u)^2 for |u| < 1, else 0; b(u) = 0.35875 + 0.48829 cos(pi u) + 0.14128 cos(2 pi u) + 0.01168 cos(3 pi u) (the 4-term
 *   Blackman-Harris window, squared).  No per-phase normalisation: the DC gain of every phase is 1 within 1e-11.
 *   Output sample j (the ABSOLUTE index on the output grid; its time is j / sr_out, no delay): j M = q L + r with 0 <= r < L in 64-bit
 *   integers (TH_ERR_UNSUPPORTED for a track whose n_out M does not fit 64 bits);
 *   y[j] = sum over k = 0 .. 2K - 1 of c[r][k] x[q - K + 1 + k], c[r][k] = (float)h(k - K + 1 - r / L) (th_resample_coefs),
 *   x[n] = 0 outside [0, n_in).
 *   Summation, in f32: tap k, in ascending k, goes into partial sum k mod 4 by one fmaf (a = fmaf(c, x, a), all four from +0, the
 *   taps outside the track included, with x = 0); y = (a0 + a1) + (a2 + a3).  The order depends on nothing but k, and
 *   th_resample_f32 (host, one channel, x = the whole channel) runs the very function the kernel runs: the same bits.
 *   Length and ranges.  n_out = ceil(n_in L / M) (th_resample_n_out); th_audio_sample_range(sr_out, n_out, start_sec, end_sec) gives
 *   [j0, j1) on the output grid; the dither index of the export is j.  The bytes of a range are therefore a slice of the whole-track
 *   export at that rate: a sample depends on the track's audio, the two rates and j alone.
 *   Same rate.  sr_out == 0 or sr_out == the track's rate applies no filter: bytes, counts and infos are exactly those of
 *   th_tm_export_pcm / _wav for the same request (the filter at L = M = 1 is not an identity).
 *   Limits.  TH_ERR_UNSUPPORTED when 2K > TH_RESAMPLE_MAX_TAPS (reduction by more than 64) or L 2K > TH_RESAMPLE_MAX_COEFS (a 64 MiB
 *   table): 96000 -> 95999 and 192000 -> 2000 are refused; every pair of standard rates from 8 kHz to 192 kHz is far inside.
 *   One deliberate difference from the reference: rubato interpolates cubically in a 128x oversampled table of the same kind of
 *   kernel; here the kernel is evaluated at the exact rational phase, so there is no interpolation error and L table rows, not 128.
 * Infos: th_export_info unchanged; sr = the output rate, sample_start/_end = [j0, j1) on the output grid, n_nan / n_clamped count
 * OUTPUT samples; the WAV header carries sr_out.  Layout and errors are those of th_tm_export_pcm word for word (offsets multiples
 * of 16, zero padding between requests, the first faulty request decides, nothing written on error, the size query, an empty range
 * is valid), plus TH_ERR_UNSUPPORTED for an unsupported rate pair.
 * A reader like th_tm_export_pcm, through the same pieces and staging buffers.  A slot that resamples also holds, from its first such
 * call until it is destroyed, the planar f32 scratch of one piece (piece frames x channels x 4 bytes: at most
 * 2 x TH_EXPORT_PIECE_BYTES + 64 KiB, reached with 16-bit output) and the coefficient table of the LAST rate pair it served (at most
 * TH_RESAMPLE_MAX_COEFS floats); a manager that never resamples holds neither. */
#define TH_RESAMPLE_MAX_TAPS 16384u
#define TH_RESAMPLE_MAX_COEFS (1u << 24)
typedef struct {
    uint32_t L, M, half_taps; /* half_taps = K */
    double rho, cutoff;       /* cutoff = rho FC */
} th_resample_plan;
/* host arithmetic.  th_resample_plan_for: TH_ERR_INVALID_ARG on a zero rate, TH_ERR_UNSUPPORTED per the limits.  th_resample_coefs:
 * row r (< L) of the table, 2K taps, as f64 (h64, may be NULL) and rounded to f32 (c32, may be NULL).  th_resample_f32: outputs
 * [j0, j0 + n) of one channel, j0 + n <= n_out */
TH_API int th_resample_plan_for(uint32_t sr_in, uint32_t sr_out, th_resample_plan *out);
TH_API int th_resample_n_out(size_t n_in, uint32_t sr_in, uint32_t sr_out, size_t *n_out);
TH_API int th_resample_coefs(uint32_t sr_in, uint32_t sr_out, uint32_t r, double *h64, float *c32);
TH_API int th_resample_f32(const float *x, size_t n_in, uint32_t sr_in, uint32_t sr_out, uint64_t j0, size_t n, float *y);
typedef struct {
    th_export_request base;
    uint32_t sr_out; /* 0 = the track's own */
} th_export_at_request;
TH_API int th_tm_export_pcm_at(th_tm *tm, const th_export_at_request *reqs, size_t n, uint8_t *out, size_t cap_bytes,
                               th_export_info *info /* n */, size_t *out_len);
TH_API int th_tm_export_wav_at(th_tm *tm, const th_export_at_request *req, uint8_t *out, size_t cap_bytes,
                               th_export_info *info /* may be NULL */, size_t *out_len);

/* ---------------------------------------------------------------- Export what a spectrogram box holds: band-limited audio */
/* th_tm_export_pcm_band / th_tm_export_wav_band: th_tm_export_pcm / _wav with the audio filtered to a frequency band first (or with
 * that band taken out), by a linear-phase FIR on the device: a box on the spectrogram has seconds AND hertz, th_tm_figure_box takes
 * both, and these entries take the same two frequency edges (upstream's "region selection and loop playback": listen to the box,
 * save it, save everything but it).  No reference implementation exists; these definitions are the contract.  Host arithmetic is
 * C double.
 *   Edges.  f_hi = min(f_hi_hz, sr / 2) (+inf is allowed), f_lo = f_lo_hz.  TH_ERR_INVALID_ARG: a NaN, f_lo < 0, f_lo >= f_hi after
 *   the clamp, an unknown mode, trans_hz NaN, negative or above sr / 2, sr == 0, TH_BAND_STOP of the whole band (f_lo == 0 and
 *   f_hi == sr / 2).
 *   Length.  K = TH_BAND_DEFAULT_HALF_TAPS when trans_hz == 0, else ceil((16.0 sr) / (5.0 trans_hz)); TH_ERR_UNSUPPORTED when
 *   2K > TH_BAND_MAX_TAPS (at 48 kHz: anything narrower than 4.6875 Hz).  The window below puts the -6.02 dB point on each edge and
 *   the stopband within 3.2 sr / K Hz of it (the 0.05-of-Nyquist at Z = 128 of the resampler); th_band_plan.trans_hz reports that
 *   width, 16 sr / (5 K).
 *   Row (th_band_coefs).  2K taps, k = 0 .. 2K - 1, t = k - K + 1 (an integer), a = 2 f_hi / sr, c = 2 f_lo / sr:
 *   h_pass(t) = (A(t) - c sinc(c t)) w(t / K), A(t) = a sinc(a t) when a < 1 and [t == 0] exactly when a == 1; sinc and w (the
 *   squared 4-term Blackman-Harris window, 0 for |u| >= 1) are those of "Export at a target sample rate", character for character.
 *   h_stop(t) = [t == 0] - h_pass(t).  c32[k] = (float)h; tap 2K - 1 is +-0 and is kept.
 *   Output.  y[j] = sum over k of c32[k] x[j - K + 1 + k], x = 0 outside [0, n): no delay, n_out = n, the rate is unchanged.
 *   Summation: that of "Export at a target sample rate", unchanged: tap k goes into partial sum k mod 4 by one fmaf, all four from
 *   +0, taps outside the track included; y = (a0 + a1) + (a2 + a3).  The order depends on k alone: tile, tap block, piece, range
 *   and slot cannot change a bit, and th_band_f32 (host, one channel, x = the whole channel) runs the same functions.
 *   Ranges.  th_audio_sample_range(sr, n, start_sec, end_sec) gives [s0, s1); the dither index is the absolute j; the bytes of a
 *   range are a slice of the whole-track export with the same filter.  A NaN sample i makes exactly the 2K outputs
 *   j = i - K .. i + K - 1 NaN, the zero tap included.
 *   Identity.  TH_BAND_PASS with f_lo == 0 and f_hi == sr / 2 applies no filter: bytes, counts and infos are exactly those of
 *   th_tm_export_pcm / _wav for `base` (th_band_plan.half_taps == 0).
 *   th_band_response (host): the magnitude of the f32 row at hz[i], in dB (20 log10 |sum of c32[k] e^(-i 2 pi hz t / sr)|),
 *   evaluated in f64: what a host draws over th_tm_get_spectrum.
 * Infos: th_export_info unchanged; n_nan / n_clamped count OUTPUT samples.  Layout and errors are those of th_tm_export_pcm word for
 * word (offsets multiples of 16, zero padding between requests, the first faulty request decides, nothing written on error, the
 * size query, an empty range is valid), plus the two rules above.
 * A reader like th_tm_export_pcm_at, through the same pieces, staging buffers and planar scratch; a piece holds one filter.  A slot
 * that filters also holds the row of the LAST filter it served (at most TH_BAND_MAX_TAPS floats, 256 KiB); a manager that never
 * filters holds none. */
#define TH_BAND_PASS 0
#define TH_BAND_STOP 1
#define TH_BAND_MAX_TAPS 65536u
#define TH_BAND_DEFAULT_HALF_TAPS 2048u
typedef struct {
    th_export_request base;  /* id, which, format, dither, seed, start_sec, end_sec: unchanged meaning */
    uint32_t mode;           /* TH_BAND_PASS / TH_BAND_STOP */
    double f_lo_hz, f_hi_hz; /* the box's frequency edges: the same numbers th_tm_figure_box takes */
    double trans_hz;         /* half transition width; 0 = default */
} th_export_band_request;
typedef struct {
    uint32_t half_taps;      /* K; 0 = no filter (identity) */
    uint32_t mode;
    double f_lo_hz, f_hi_hz; /* after clamping */
    double trans_hz;         /* the width the filter has: 16 sr / (5 K) */
} th_band_plan;
/* host arithmetic.  th_band_coefs: the row of a plan with half_taps > 0, as f64 (h64, may be NULL) and rounded to f32 (c32, may be
 * NULL).  th_band_response: see above.  th_band_f32: outputs [j0, j0 + n) of one channel under the row c32 of 2 half_taps taps,
 * j0 + n <= n_in */
TH_API int th_band_plan_for(uint32_t sr, uint32_t mode, double f_lo_hz, double f_hi_hz, double trans_hz, th_band_plan *out);
TH_API int th_band_coefs(uint32_t sr, const th_band_plan *plan, double *h64, float *c32);
TH_API int th_band_response(uint32_t sr, const th_band_plan *plan, const double *hz, size_t n, double *db);
TH_API int th_band_f32(const float *x, size_t n_in, const float *c32, uint32_t half_taps, uint64_t j0, size_t n, float *y);
TH_API int th_tm_export_pcm_band(th_tm *tm, const th_export_band_request *reqs, size_t n, uint8_t *out, size_t cap_bytes,
                                 th_export_info *info /* n */, size_t *out_len);
TH_API int th_tm_export_wav_band(th_tm *tm, const th_export_band_request *req, uint8_t *out, size_t cap_bytes,
                                 th_export_info *info /* may be NULL */, size_t *out_len);

/* ---------------------------------------------------------------- FLAC export: a lossless encoder for resident audio */
/* th_tm_export_flac: request i as a complete FLAC file image of the request's time range, encoded on the device (blocks are
 * independent, so the encoder is block-parallel integer work, and the file that crosses the bus is the small one).  The request is
 * th_export_request with the same sample-range rule and the same error order; format is TH_PCM_S16 or TH_PCM_S24 (TH_PCM_F32:
 * TH_ERR_INVALID_ARG).  The samples that are coded are exactly the integers th_export_quantize gives (absolute-index dither, clamp,
 * NaN -> 0, counted in n_clamped / n_nan), so the file DECODES TO THE BYTES th_tm_export_pcm RETURNS for the same request.  FLAC is
 * an entry, not a format value: no existing entry, format or error code changes.
 *   The stream (a subset of RFC 9639, every choice fixed so that the bytes are a function of the samples):
 *   Stream header, 42 bytes: "fLaC", one STREAMINFO block with the last-block flag: minimum and maximum block size 4096 / 4096, the
 *   minimum and maximum frame size actually produced (24 bits each; 0 0 without frames), sr (20 bits), channels - 1 (3), bits per
 *   sample - 1 (5), total samples (36), MD5 all zero ("not computed").
 *   Limits: sr > 1 048 575, more than 8 channels, 2^36 or more samples: TH_ERR_UNSUPPORTED.  An empty range is the header alone.
 *   Frames: fixed block size TH_FLAC_BLOCK = 4096; block b holds samples s0 + 4096 b .. of the range and its frame number is b; the
 *   last block may be shorter.  Frame header: sync 0xFFF8; block-size code 1100 for 4096, else 0110 (n <= 256, 8 bits of n - 1) or 0111
 *   (16 bits of n - 1); rate code from the table where the rate is in it (88.2, 176.4, 192, 8, 16, 22.05, 24, 32, 44.1, 48, 96 kHz ->
 *   0001 .. 1011), else 1101 (sr <= 65 535, 16 bits of Hz), else 1110 (sr a multiple of 10 and sr / 10 <= 65 535, 16 bits), else
 *   0000; channel assignment n_ch - 1 (independent); size code 100 (16 bit) or 110 (24 bit); the frame number in the UTF-8-like form;
 *   CRC-8.  Then the subframes in channel order, zero bits to the byte boundary, CRC-16 of the whole frame.
 *   Subframe of n samples (no wasted bits, no escape codes; all costs exact 64-bit integers): CONSTANT when all n samples are equal.
 *   Else, for n >= 5, the fixed predictors of order o = 0 .. 4: residuals e from sample o on, u = zigzag(e) = (e << 1) ^ (e >> 31);
 *   partition order p = the largest p <= 6 with 2^p | n and (n >> p) >= 5; a partition's Rice parameter is the smallest k minimising
 *   sum(u >> k) + m (k + 1) over its m residuals, k in 0 .. 14 with 4-bit parameters (coding method 0) at 16 bit, 0 .. 30 with 5-bit
 *   parameters (method 1) at 24 bit; cost(o) = o bps + 6 + sum over the partitions of (parameter bits + residual bits); the lowest
 *   order of the smallest cost wins.  VERBATIM when that cost >= n bps, and always for n <= 4 unless CONSTANT.
 *   Not in this stream: LPC subframes and stereo decorrelation (the _ex entries below add them by flags), a searched partition
 *   order, the MD5, seek tables and comments.
 * Layout.  Sizes are not known before encoding, so the offsets come from bounds: offset[0] = 0, offset[i + 1] = offset[i] +
 * th_flac_bound(request i) rounded up to 16, with th_flac_bound = 42 + per block (16 bytes of frame header at most + n_ch x (1 +
 * n bps / 8) bytes of verbatim subframes + 1 byte of padding + 2 of CRC-16).  A size query (out == NULL or cap_bytes too small:
 * TH_ERR_BUFFER_TOO_SMALL) returns in *out_len the last offset + the last bound and in info[i].n_bytes the bounds.  A successful call
 * sets info[i].n_bytes to the ACTUAL file length and *out_len to the last offset + that request's n_bytes.  Bytes between a file's
 * end and the next offset are unspecified; nothing is written at or beyond the last request's bound.  Errors, first faulty request
 * and revision: as th_tm_export_pcm.
 * A reader like th_tm_export_pcm: shared lock, a reader slot's streams, pieces of whole blocks whose bound stays within
 * TH_EXPORT_PIECE_BYTES through two device buffers (piece p + 1 is encoded while piece p is copied out).  A slot's FLAC scratch is
 * made on its first FLAC call and never exceeds two staging buffers of TH_EXPORT_PIECE_BYTES, one piece of subframe slots (at most
 * TH_EXPORT_PIECE_BYTES + 4 bytes x 65 536 units), two tables of 65 536 words and the job table of the largest call; a manager that
 * never exports FLAC holds none.  A file depends on the track's audio and the request alone.
 * Host functions.  th_flac_bound: the bound above.  th_flac_frame_header: sync .. CRC-8 of one frame (1 <= block_len <= 4096,
 * frame_number < 2^36).  th_flac_encode_i32: the same stream made on the host, byte for byte, from n_ch planar int32 channels of n
 * samples, each inside the format's range (else TH_ERR_INVALID_ARG); cap must hold th_flac_bound (else TH_ERR_BUFFER_TOO_SMALL with
 * the bound in *out_len), *out_len = the file's length. */
#define TH_FLAC_BLOCK 4096
TH_API int th_flac_bound(uint64_t n_frames, uint32_t n_ch, uint32_t format, uint64_t *bytes);
TH_API int th_flac_frame_header(uint32_t sr, uint32_t n_ch, uint32_t format, uint64_t frame_number, uint32_t block_len,
                                uint8_t out[16], size_t *len);
TH_API int th_flac_encode_i32(const int32_t *const *chan, uint32_t n_ch, uint64_t n, uint32_t format, uint32_t sr, uint8_t *out,
                              size_t cap, size_t *out_len);
TH_API int th_tm_export_flac(th_tm *tm, const th_export_request *reqs, size_t n, uint8_t *out, size_t cap_bytes,
                             th_export_info *info /* n */, size_t *out_len);

/* The _ex entries: the same export with two more coding tools, chosen by flags.  flags == 0 gives the bytes of the entries above, byte
 * for byte; a bit outside TH_FLAC_LPC | TH_FLAC_STEREO is TH_ERR_INVALID_ARG (checked where the format is).  Request, sample-range
 * rule, error order, offsets from th_flac_bound, size query, info, revision, pieces and reader slot: those of th_tm_export_flac.  The
 * stream is a function of the samples and the flags alone, and th_flac_encode_i32_ex is the same source run on the host: the same
 * file, byte for byte.  All rules are integer arithmetic, or f64 in a fixed serial order (one rounded operation after the other, no
 * fused multiply-add).
 *   TH_FLAC_LPC: per subframe, LPC predictors of order 1 .. TH_FLAC_LPC_MAX_ORDER join the candidates, wherever the fixed predictors
 *   are tried (n >= 5, not CONSTANT).  For a block s[0 .. n) of one coded channel:
 *   1. Window: w[i] = (((2 i + 1) (2 n - 2 i - 1)) << 14) / (n n) in unsigned 64-bit division (Welch, 0 <= w <= 2^14).  L = the bit
 *      length of max |s[i]|, sh = max(0, L - 8), x[i] = (s[i] w[i]) >> sh (arithmetic, 64 bit), so |x| < 2^22 at any level.
 *   2. Autocorrelation r[m] = sum x[i] x[i + m], m = 0 .. min(8, n - 1), exact in int64 (|r| < 2^56).  r[0] == 0: no LPC candidates.
 *   3. Levinson-Durbin in f64: E = (double)r[0]; for m = 1 ..: acc = (double)r[m], then acc = acc - a[j - 1] (double)r[m - j] for
 *      j = 1 .. m - 1; k = acc / E; the new a[j - 1] = a[j - 1] - k a[m - j - 1] (from the old ones), a[m - 1] = k; E = E (1 - k k).
 *      When E is not finite or not > 0, order m and all higher orders are no candidates.
 *   4. Order m's coefficients in P bits, P = 12 for 16-bit files and 14 for 24-bit files: cmax = max |a|; zero or non-finite: no
 *      candidate.  e = cmax's binary exponent as frexp gives it; shift = P - e - 1, above 15 set to 15, below 0 no candidate.  With
 *      fb = 0, for j = 1 .. m: fb = fb + a[j - 1] 2^shift; q[j] = floor(fb + 0.5) clamped to [-2^(P-1), 2^(P-1) - 1]; fb = fb - q[j].
 *   5. Residual e[i] = s[i] - ((sum over j = 1 .. m of q[j] s[i - j]) >> shift) for i >= m, exact in int64, arithmetic shift.  If any
 *      e[i] lies outside [-(2^31 - 1), 2^31 - 1], order m is no candidate (checked on every residual).
 *   6. Cost, exact: partition order p = the largest p <= 6 with 2^p | n and (n >> p) >= max(5, m + 1); Rice parameters as for the
 *      fixed predictors (all k, the file's coding method); cost(LPC m) = m bps + 4 + 5 + m P + 6 + the partitions.
 *   7. The candidates are fixed 0 .. 4, then LPC 1 .. 8: the smallest cost wins, the earlier one on ties; VERBATIM when that cost is
 *      >= n bps.  The subframe (RFC 9639 9.2.6): type 1xxxxx with order - 1, the warm-up samples, 4 bits of P - 1, 5 bits of shift,
 *      the coefficients q[1] .. q[m] as P-bit two's complement, then the residual as in a FIXED subframe.
 *   TH_FLAC_STEREO: files of exactly 2 channels only (no effect on others).  Per block four channels are coded from the quantised
 *   integers: L and R at bps bits, M = (L + R) >> 1 at bps bits, S = L - R at bps + 1 bits, each by the rules above (LPC candidates
 *   only with TH_FLAC_LPC; for S, warm-up, CONSTANT and VERBATIM sizes and the VERBATIM threshold use bps + 1; the Rice method and P
 *   stay the file's).  The frame takes the assignment of the fewest subframe bits, the earlier one on ties: independent L R (code
 *   0001), left/side L S (1000), side/right S R (1001), mid/side M S (1010).  Only the header's assignment bits and CRC-8 change.
 *   Every subframe is a minimum over a superset of the flags == 0 candidates and "independent" is among the assignments, so no
 *   frame is longer than the flags == 0 frame: th_flac_bound, the offsets and the size query are unchanged and still bounds, and the
 *   decoded samples are the bytes th_tm_export_pcm returns whatever the flags.  A slot's subframe scratch with TH_FLAC_STEREO: four
 *   units per stereo block, each of the side channel's verbatim size (at most 3 x TH_EXPORT_PIECE_BYTES + 4 bytes x 65 536 units).
 *   Not in the stream: a searched partition order, orders above 8, the MD5, seek tables and comments. */
#define TH_FLAC_LPC 1u    /* LPC subframes of order 1 .. TH_FLAC_LPC_MAX_ORDER among the candidates */
#define TH_FLAC_STEREO 2u /* for 2-channel files: the cheapest of the four channel assignments per frame */
#define TH_FLAC_LPC_MAX_ORDER 8
TH_API int th_flac_encode_i32_ex(const int32_t *const *chan, uint32_t n_ch, uint64_t n, uint32_t format, uint32_t sr, uint32_t flags,
                                 uint8_t *out, size_t cap, size_t *out_len);
TH_API int th_tm_export_flac_ex(th_tm *tm, const th_export_request *reqs, size_t n, uint32_t flags, uint8_t *out, size_t cap_bytes,
                                th_export_info *info /* n */, size_t *out_len);

/* ---------------------------------------------------------------- Export as figures: a spectrogram region at any pixel size */
/* Any region of a channel's resident u16 image, resampled on the device to any pixel size and coloured (or left as 16-bit grey): what
 * a host saves as a figure, without fetching tiles, stitching them and resampling a second time (upstream's roadmap item "export as
 * figures"; no reference implementation exists, these definitions are the contract).
 *   A figure is the region box = (left, top, width, height) of the image resampled to out_w x out_h pixels.  Box coordinates are
 *   doubles in image pixels: x = frame columns, y = image rows, row 0 = the lowest frequency (the coordinates of a LOD tile's crop
 *   box).  The resampling is the separable Lanczos3 of the LOD tiles: the horizontal pass, then the vertical one; a pass takes the
 *   taps of th_figure_axis (normalised on the host), adds pixel x tap in ascending tap order from 0.0 in f64 (a multiplication, then an
 *   addition), rounds half up (floor(v + 0.5)) and clamps to [0, 65535].  The filter is clipped at the IMAGE, never at the box: a
 *   figure of a region is filtered with the pixels around the region.
 *   TH_FIGURE_RGBA: out_h x out_w x 4 bytes, the top row = the highest frequency (output row j = vertical output out_h - 1 - j); the
 *   colour is entry (v (n_colors - 1) + 32767) / 65535 of the manager's colormap, as in a tile.  TH_FIGURE_GREY16: out_h x out_w
 *   little-endian u16 in the same row order.  The whole image at its own size is an exact copy (rows flipped).
 *   th_figure_axis (host): the taps of one axis of n_in source pixels: for output o, source pixels start[o] .. start[o] + count[o] - 1
 *   with the weights w[o * *max_taps + t].  scale = extent / n_out, f = max(scale, 1), centre = origin + (o + 0.5) scale, the window
 *   [(long)(centre - 3 f + 0.5), (long)(centre + 3 f + 0.5)) clipped to [0, n_in), tap t = L(((t + start) - centre + 0.5) / f),
 *   L(x) = sinc(x) sinc(x / 3) on -3 <= x < 3, sinc(x) = sin(pi x) / (pi x), each tap divided by the window's sum; C double (Pillow's
 *   ImagingResample coefficients with the box kept in double).  start and count: n_out entries; weights may be NULL or
 *   cap_weights < n_out x *max_taps: TH_ERR_BUFFER_TOO_SMALL with start, count and *max_taps filled.
 *   th_figure_box (host): the box of (start_sec, end_sec, hz_min, hz_max) for a track of n_samples at sr whose image is img_width
 *   columns x img_height rows over a spectrogram of spec_height rows.  x(sec) = sec sr / n_samples img_width (the viewer's mapping:
 *   pixels per second = image width / track seconds); y(hz) = r(hz) spec_height, r = hz / (sr / 2) under TH_FREQ_LINEAR and
 *   mel(hz) / mel(sr / 2) under TH_FREQ_MEL, mel = the library's Slaney scale; all in C double, so that integral results are the rows
 *   of th_hz_range_to_idx.  end_sec = +inf: the track's end; hz_max = +inf: the image's top row.  The result is clamped to the image.
 *   TH_ERR_INVALID_ARG: a NaN argument, a negative or infinite start_sec or hz_min, an end not above its start after clamping, a zero
 *   sr, n_samples, img_width, spec_height or img_height.  th_tm_figure_box fills in what the manager knows of (id, ch).
 * th_tm_render_figures: request i's record starts at out + info[i].offset, a multiple of 64, and holds info[i].bytes bytes; the bytes
 * between two records are not written; *out_len = the last record's end.  A reader like th_tm_export_pcm: shared lock, a reader
 * slot's own streams; out == NULL or cap_bytes < *out_len: TH_ERR_BUFFER_TOO_SMALL with info and *out_len filled.  The first faulty
 * request decides: an unknown id or a channel without a resident image: TH_ERR_NOT_FOUND; a bad channel or kind, out_w or out_h zero
 * or above TH_FIGURE_MAX_DIM, a box with a non-finite or non-positive extent or one that is not inside the image:
 * TH_ERR_INVALID_ARG; a tap table beyond 256 MB (the rule of the LOD tiles): TH_ERR_UNSUPPORTED.  On any error nothing is written to
 * out.  A request's bytes depend on its image, box, size, kind and the colormap alone: not on the batch, the slot, the pieces below,
 * or th_tm against th_tmg.  spectrogram_revision: the revision the bytes belong to.
 * Device memory is BOUNDED: a call is cut into pieces, bands of whole output rows of one or more requests; a piece is at most
 * TH_FIGURE_PIECE_BYTES of output in one of two staging buffers (piece p + 1 is computed while piece p is copied out; into pinned
 * memory, th_host_alloc, that copy is the only one), and the horizontal pass's intermediate of a piece (u16, the source rows its
 * bands' filter windows span x out_w) is at most TH_FIGURE_TMP_BYTES, or what ONE output row needs where that alone is more (at
 * most 6 r + 2 source rows, r = the vertical reduction, of out_w pixels rounded up to 8: the 256 MB rule, (6 r + 4) x 8 x out_w <=
 * 256 MB, keeps that at 64 MiB for out_w >= 8, and it is never more than the image's rows).  Adjacent bands recompute the source rows their windows share: a row's
 * horizontal pass does not depend on the band.  Tap tables are built and uploaded once per call and distinct (axis length, origin,
 * extent, output size).  A slot's figure scratch is made on its first figure and only grows. */
#define TH_FIGURE_RGBA 0
#define TH_FIGURE_GREY16 1
#define TH_FIGURE_MAX_DIM 16384u
#define TH_FIGURE_PIECE_BYTES (8u << 20)
#define TH_FIGURE_TMP_BYTES (16u << 20)
typedef struct {
    size_t id;
    uint32_t ch;
    uint32_t kind;         /* TH_FIGURE_* */
    uint32_t out_w, out_h; /* 1 .. TH_FIGURE_MAX_DIM */
    double left, top, width, height;
} th_figure_request;
typedef struct {
    uint64_t offset, bytes; /* into out */
    uint32_t out_w, out_h;
    uint64_t spectrogram_revision;
} th_figure_info;
TH_API int th_figure_axis(double origin, double extent, uint32_t n_out, uint32_t n_in, int32_t *start /* n_out */,
                          int32_t *count /* n_out */, double *weights, size_t cap_weights, uint32_t *max_taps);
TH_API int th_figure_box(double start_sec, double end_sec, double hz_min, double hz_max, uint32_t sr, size_t n_samples,
                         size_t img_width, size_t spec_height, size_t img_height, int freq_scale, double *left, double *top,
                         double *width, double *height);
TH_API int th_tm_figure_box(th_tm *tm, size_t id, uint32_t ch, double start_sec, double end_sec, double hz_min, double hz_max,
                            double *left, double *top, double *width, double *height);
TH_API int th_tm_render_figures(th_tm *tm, const th_figure_request *reqs, size_t n, uint8_t *out, size_t cap_bytes,
                                th_figure_info *info /* n */, size_t *out_len);
TH_API int th_tm_render_figure(th_tm *tm, const th_figure_request *req, uint8_t *out, size_t cap_bytes, th_figure_info *info);

/* ---------------------------------------------------------------- Waveform envelope: any time range at any pixel width */
/* The exact (min, max, mean, rms) of every pixel column of a time range of a channel's resident audio, and that envelope rasterised
 * as the RGBA waveform lane that sits under a figure: one streaming pass over the samples the request covers, without picking a
 * pyramid level, fetching its tiles and re-binning them (no reference implementation exists, these definitions are the contract).
 *   A request is (id, ch, which, start_sec, end_sec, n_cols); which as in th_tm_copy_audio: 0 the audio the spectrogram is made
 *   from, 1 the audio the waveform is drawn from, 2 the original.  The channel has n >= 1 samples at rate sr; all of this in C double:
 *   A = clamp(start_sec (double)sr, 0, n); B = n for end_sec = +inf, else clamp(end_sec (double)sr, 0, n); B > A is required; W = n_cols;
 *   e[W] = ceil(B); e[j] = min(ceil(A + (B - A) (double)j / (double)W), e[W]) for j < W (a product, a quotient, a sum).  Column j owns
 *   samples [e[j], e[j + 1]): those whose index lies in the column's real interval.  The edges never decrease.  A range between
 *   two samples (B > A, ceil(A) = ceil(B)) is a valid request: every column is empty and holds the sample below.
 *   th_envelope_edges (host) is that definition.  TH_ERR_INVALID_ARG: a NaN argument, a negative or infinite start_sec, an end not
 *   above the start after clamping, a zero sr, n_samples or n_cols, n_cols above TH_ENVELOPE_MAX_COLS.
 *   Values: four f32 per column, interleaved (min, max, mean, rms), 16 bytes per column.  With c = e[j + 1] - e[j] > 0: min and max by
 *   fminf / fmaxf, which ignore NaN, as the waveform tiles do (an all-NaN column gives (+inf, -inf); where an extremum is zero and the
 *   column holds both +0 and -0, which of the two comes back is not specified); mean = (f32)((sum x) / c) and
 *   rms = (f32)sqrt((sum x x) / c) with both sums in f64, so any NaN sample makes both NaN.  c = 0 (a view zoomed in past one sample
 *   per column): a zero-order hold of sample max(e[j], 1) - 1: min = max = mean = x, rms = |x| (a NaN sample: NaN in all four).
 *   The order of the f64 sums is fixed by the channel, the request's edges and the kernels' absolute chunk grid alone (4096-sample
 *   chunks counted from sample 0 of the channel): a request's bytes do not depend on the rest of the batch, the reader slot, how the
 *   call was cut into pieces, the call itself, or th_tm against th_tmg.
 *   A waveform figure (lane) is an envelope request whose n_cols is out_w, plus out_h, amp_lo < amp_hi (finite f32), thickness in
 *   1/256 pixel (0 .. 256 out_h), fill[4] and background[4] (RGBA bytes).  Everything behind the envelope is integer arithmetic:
 *   1. join to the left neighbour (j > 0, both columns not all-NaN, the neighbour's values un-joined): max_j < min_(j-1): max_j :=
 *   min_(j-1); min_j > max_(j-1): min_j := max_(j-1).  2. Y(v) = clamp(floor(((double)amp_hi - v) / ((double)amp_hi - amp_lo) out_h
 *   256 + 0.5), 0, 256 out_h), one rounded f64 operation per step in that order, v the f32 widened; Ytop = Y(max), Ybot = Y(min).
 *   3. a column with max < min (all NaN) or a NaN mean draws nothing.  4. Ybot - Ytop < thickness: Ytop := floor((Ytop + Ybot -
 *   thickness) / 2), Ybot := Ytop + thickness, both clamped to [0, 256 out_h].  5. row r counts from the top (amp_hi): cov = max(0,
 *   min(Ybot, 256 (r + 1)) - max(Ytop, 256 r)), and each of the four bytes is (fill cov + background (256 - cov) + 128) >> 8.
 *   th_waveform_figure_span (host): (Ytop, Ybot) of one column, *draws = 0 where it draws nothing; col and left are the four values of
 *   the column and of its left neighbour (NULL for column 0).  TH_ERR_INVALID_ARG: out_h zero or above TH_FIGURE_MAX_DIM, an amplitude
 *   range that is not finite and ascending, a thickness above 256 out_h.
 * th_tm_get_envelopes: request i's 4 n_cols floats start at out + info[i].offset (floats, requests back to back); *out_len = the
 * floats of all.  th_tm_render_waveform_figures: request i's record is out_h x out_w x 4 bytes, the top row = amp_hi, starts at
 * out + info[i].offset, a multiple of 64; the bytes between two records are not written; *out_len = the last record's end.  Readers
 * like th_tm_get_spectra and th_tm_render_figures: shared lock, a reader slot's own streams; out == NULL or a cap below *out_len:
 * TH_ERR_BUFFER_TOO_SMALL with info and *out_len filled.  The first faulty request in request order decides: an unknown id:
 * TH_ERR_NOT_FOUND; a bad channel, which, time range, size, amplitude range or thickness: TH_ERR_INVALID_ARG.  On any error nothing
 * is written to out.  info[i]: sample_start = e[0], sample_end = e[n_cols], waveform_revision: the revision the values belong to.
 * Device memory is BOUNDED.  An envelope call is cut into pieces of whole requests of at most TH_ENVELOPE_PIECE_BYTES of results
 * (one request is at most TH_ENVELOPE_MAX_COLS x 16 bytes = 1 MiB); beside the results a piece holds its edge tables (8 bytes per
 * column) and, for requests of 64 samples per column or more, 48 bytes of partial sums per 16 KiB chunk of audio it reads (0.3 %),
 * at most TH_ENVELOPE_PART_BYTES unless ONE request alone needs more.  A lane call computes the envelopes of such a piece once (16
 * bytes per column, and 8 for the spans), keeps them on the device across the bands, and rasterises bands of whole output rows of at
 * most TH_FIGURE_PIECE_BYTES through two staging buffers, piece p + 1 computed while piece p is copied out.  The edge tables of a
 * call are built and uploaded once.  A slot's scratch is made on first use and only grows. */
#define TH_ENVELOPE_MAX_COLS 65536u
#define TH_ENVELOPE_PIECE_BYTES (4u << 20)
#define TH_ENVELOPE_PART_BYTES (32u << 20)
typedef struct {
    size_t id;
    uint32_t ch;
    uint32_t which;   /* 0 audio, 1 drawn, 2 original */
    double start_sec, end_sec;
    uint32_t n_cols;  /* 1 .. TH_ENVELOPE_MAX_COLS */
    uint32_t reserved;
} th_envelope_request;
typedef struct {
    uint64_t offset, length;            /* into out, floats; length = 4 n_cols */
    uint64_t sample_start, sample_end;  /* e[0], e[n_cols] */
    uint64_t waveform_revision;
} th_envelope_info;
typedef struct {
    th_envelope_request env; /* n_cols = out_w: 1 .. TH_FIGURE_MAX_DIM */
    uint32_t out_h;          /* 1 .. TH_FIGURE_MAX_DIM */
    float amp_lo, amp_hi;
    uint32_t thickness;      /* 1/256 pixel: 0 .. 256 out_h */
    uint8_t fill[4], background[4];
} th_waveform_figure_request;
typedef struct {
    uint64_t offset, bytes; /* into out */
    uint32_t out_w, out_h;
    uint64_t sample_start, sample_end;
    uint64_t waveform_revision;
} th_waveform_figure_info;
TH_API int th_envelope_edges(uint32_t sr, size_t n_samples, double start_sec, double end_sec, uint32_t n_cols,
                             uint64_t *edges /* n_cols + 1 */);
TH_API int th_waveform_figure_span(const float *col /* 4 */, const float *left /* 4, or NULL */, uint32_t out_h, float amp_lo,
                                   float amp_hi, uint32_t thickness, int32_t *y_top, int32_t *y_bot, int *draws);
TH_API int th_tm_get_envelopes(th_tm *tm, const th_envelope_request *reqs, size_t n, float *out, size_t cap_floats,
                               th_envelope_info *info /* n */, size_t *out_len);
TH_API int th_tm_get_envelope(th_tm *tm, const th_envelope_request *req, float *out, size_t cap_floats, th_envelope_info *info);
TH_API int th_tm_render_waveform_figures(th_tm *tm, const th_waveform_figure_request *reqs, size_t n, uint8_t *out, size_t cap_bytes,
                                         th_waveform_figure_info *info /* n */, size_t *out_len);
TH_API int th_tm_render_waveform_figure(th_tm *tm, const th_waveform_figure_request *req, uint8_t *out, size_t cap_bytes,
                                        th_waveform_figure_info *info);

/* ---------------------------------------------------------------- Formant candidates of a time range (LPC on resident audio) */
/* Per analysis frame of a channel's resident audio: an autocorrelation-LPC fit of the decimated, pre-emphasised, windowed frame, the
 * roots of the prediction polynomial, and those roots as (frequency, bandwidth) pairs in ascending frequency: the candidates a
 * formant overlay draws.  Which candidate is F1 .. F4 along time is a tracker's decision and is not made here.  No reference
 * implementation exists; these definitions are the contract.  The parameters are Praat's ("To Formant (burg)": 2 x 5 formants up to
 * 5500 Hz, a Gaussian window of 2 x 25 ms, pre-emphasis from 50 Hz); the fit is the autocorrelation method, not Burg's.
 *   Request and plan.  th_formant_request: id, ch, which as th_tm_copy_audio; [start_sec, end_sec); sr_analysis (0 = the track's rate);
 *   n_poles p, even, 2 .. TH_FORMANT_MAX_POLES; win_sec, step_sec; preemph_hz; window TH_FORMANT_WIN_*; kind TH_FORMANT_OUT_*.
 *   th_formant_defaults fills the speech settings: sr_analysis 11000, p 10, win_sec 0.05, step_sec 0.0125, preemph_hz 50, Gaussian,
 *   formants, the whole track.  th_formant_plan_for(sr, n_samples, req, &plan) (host) is the one place where numbers are made from
 *   seconds, all in C double: sr_a = sr_analysis or sr; when sr_a != sr, th_resample_plan_for(sr, sr_a) must accept the pair (its
 *   TH_ERR_UNSUPPORTED is this reader's; so is that of th_resample_n_out) and n_a = th_resample_n_out, else n_a = n_samples;
 *   W = rint(win_sec sr_a), p + 2 <= W <= TH_FORMANT_MAX_WIN; H = max(1, rint(step_sec sr_a)), H <= TH_FORMANT_MAX_HOP;
 *   alpha = exp(-2 pi preemph_hz / sr_a) (libm), and preemph_hz = +inf gives alpha = 0: no pre-emphasis.
 *   Frames are ABSOLUTE: frame f has its centre at analysis sample c_f = f H, f = 0 .. ceil(n_a / H) - 1 (n_frames_total; 0 for an
 *   empty track), its window covers analysis samples [b, b + W), b = c_f - floor(W / 2) (signed 64-bit), and the signal is zero
 *   outside [0, n_a).  The time range selects frames [f0, f1): with [s0, s1) = th_audio_sample_range(sr_a, n_a, start_sec, end_sec),
 *   f0 = ceil(s0 / H), f1 = ceil(s1 / H) in integers: the frames whose centre lies in [s0, s1).  A range is therefore a slice of the
 *   whole-track analysis, and an empty range is valid.  TH_ERR_INVALID_ARG: a zero sr, anything NaN, a bad time range, an odd or
 *   out-of-range p, W or H out of range (win_sec and step_sec must be finite and win_sec > 0, step_sec >= 0), a negative preemph_hz,
 *   an unknown window, kind or which, a bad channel.
 *   Analysis signal u: the channel itself when sr_a = sr, else exactly the resampler's output at sr_a, the bits of th_resample_f32
 *   (f32).
 *   Per frame, in f64, ONE rounded operation per written operation, no fma, no libm:
 *   1. d[n] = (double)u[n] - alpha (double)u[n - 1] for 0 <= n < n_a, with u[-1] = +0, and d[n] = +0 outside [0, n_a) (the
 *      pre-emphasised signal is what is zero outside the track: d[n_a] is 0, not -alpha u[n_a - 1]); s[k] = d[b + k] g[k], g the f64
 *      table of th_formant_window: Gaussian
 *      g[k] = (exp(-48 (k - (W - 1) / 2)^2 / (W + 1)^2) - e^-12) / (1 - e^-12) (libm, host-built), rectangular all ones.
 *   2. Autocorrelation r[m], m = 0 .. p: partial sum q (0 .. 63) takes k = q, q + 64, ... in ascending k over k = 0 .. W - 1 - m, each
 *      step acc = acc + (s[k] s[k + m]) from +0; then part[q] = part[q] + part[q + h] for q < h, h = 32, 16, 8, 4, 2, 1; r[m] = part[0].
 *   3. The frame is INVALID if r[0] is not finite or r[0] <= 0.  Else r0' = r[0] (1 + 2^-30) (the product of r[0] and the double
 *      1 + 2^-30): a white-noise loading that keeps a pure tone solvable.
 *   4. Levinson-Durbin, literally: E = r0'; for i = 1 .. p: acc = r[i]; for j = 1 .. i - 1: acc = acc + a[j] r[i - j];
 *      kappa = -acc / E (the negation of acc, divided); new a[j] = a[j] + kappa a[i - j] for j < i (from the old a), a[i] = kappa;
 *      E = E (1 - kappa kappa); if !(E > 0) the frame is INVALID.
 *   5. (kind TH_FORMANT_OUT_FORMANTS only) The roots of z^p + a1 z^(p-1) + .. + ap by Aberth-Ehrlich in Jacobi form: z_i starts at
 *      0.9 (cos t_i, sin t_i), t_i = 2 pi (i + 1/4) / p (th_formant_start_points, libm, host-built); at most TH_FORMANT_MAX_SWEEPS = 64
 *      sweeps; in a sweep, for every i from the OLD z: Horner P = (1, 0), D = (0, 0), for k = 1 .. p: D = D z + P, then P = P z + a[k];
 *      q = P / D; sigma = sum over j != i in ascending j of 1 / (z_i - z_j), from (0, 0); w_i = q / (1 - q sigma); z_i = z_i - w_i.
 *      Complex product (ar br - ai bi, ar bi + ai br); complex sum and difference by components; quotient u / v =
 *      ((ur vr + ui vi) / n, (ui vr - ur vi) / n), n = vr vr + vi vi; 1 / v and 1 - v are that quotient and that difference with
 *      (1, 0), nothing simplified; "+ a[k]" adds a[k] to the real part alone.  The sweeps stop after the one in which every w_r^2 + w_i^2 <= 2^-80 (a NaN never stops).  A frame that
 *      has not stopped after 64 sweeps is INVALID and counted in n_unconverged.  The sweep count of a frame is the number run.
 *   6. Host only, after the read-back, C double with libm: per root with imag > 0: f = atan2(im, re) sr_a / (2 pi),
 *      bw = -log(re^2 + im^2) sr_a / (2 pi); keep 50 <= f <= sr_a / 2 - 50; sort by ascending f, ties by ascending bw; keep the first p / 2.
 *   Output: doubles, requests back to back in request order, frames in order, 2 + p doubles per frame.  TH_FORMANT_OUT_FORMANTS:
 *   (n_found, E / r0', f_1 .. f_(p/2), bw_1 .. bw_(p/2)), NaN in the unused slots.  TH_FORMANT_OUT_LPC: (r0', E, a_1 .. a_p): the LPC
 *   envelope is E / |A(e^jw)|^2; step 5 is not run and n_unconverged is 0.  An invalid frame is all NaN.  info[i]: offset and length
 *   in doubles, [frame_first, frame_end) = [f0, f1), sr_analysis, win = W, hop = H, n_invalid (every invalid frame, the unconverged
 *   ones included), n_unconverged, waveform_revision.
 *   A frame's doubles depend on the channel's audio, the plan and f alone: not on the range, the batch, the reader slot, the pieces,
 *   the call, or th_tm against th_tmg.  th_formants_f64 (host, one channel, x = the whole channel at rate sr) runs the very
 *   functions the kernel runs and gives the same bits; counts = {n_invalid, n_unconverged} (may be NULL).  th_formant_frame_f64: one
 *   frame's raw fit: r (p + 1), a (p + 1, a[0] = 1), r0e = {r0', E}, roots (2 p: p real parts, then p imaginary parts), *sweeps,
 *   *status (0 valid, 1 invalid at step 3 or 4, 2 unconverged); what the steps did not reach is zero; step 5 runs for either kind.
 * th_tm_get_formants / th_tm_get_formant_track: a reader like th_tm_get_envelopes: shared lock, a reader slot's own stream; out ==
 * NULL or a cap below *out_len: TH_ERR_BUFFER_TOO_SMALL with info (the two counts zero) and *out_len filled.  The first faulty request
 * in request order decides: an unknown id: TH_ERR_NOT_FOUND; a bad argument: TH_ERR_INVALID_ARG; a refused rate pair:
 * TH_ERR_UNSUPPORTED.  On any error nothing is written to out.
 * Device memory is BOUNDED.  A call is cut into pieces of runs of frames, each run of one request, of at most
 * TH_FORMANT_PIECE_FRAMES frames and at most TH_FORMANT_PIECE_SAMPLES analysis samples of resampled signal (a run's hull:
 * (frames - 1) H + W + 1 samples; one frame always fits) and of one rate pair; a piece is one launch of the resampler for its resampled
 * runs, one of the formant kernel (4 + 3 p doubles of raw record per frame, into one of two buffers) and one copy; step 6 and the
 * packing of piece k run on the host while piece k + 1 computes.  A slot's scratch is made on first use and only grows. */
#define TH_FORMANT_MAX_POLES 32u
#define TH_FORMANT_MAX_WIN 4096u
#define TH_FORMANT_MAX_HOP 65536u
#define TH_FORMANT_MAX_SWEEPS 64u
#define TH_FORMANT_PIECE_FRAMES 16384u
#define TH_FORMANT_PIECE_SAMPLES (4u << 20)
#define TH_FORMANT_WIN_GAUSS 0
#define TH_FORMANT_WIN_RECT 1
#define TH_FORMANT_OUT_FORMANTS 0
#define TH_FORMANT_OUT_LPC 1
typedef struct {
    size_t id;
    uint32_t ch;
    uint32_t which;       /* 0 audio, 1 drawn, 2 original */
    double start_sec, end_sec;
    uint32_t sr_analysis; /* 0 = the track's rate */
    uint32_t n_poles;     /* even, 2 .. TH_FORMANT_MAX_POLES */
    double win_sec, step_sec, preemph_hz;
    uint32_t window, kind; /* TH_FORMANT_WIN_*, TH_FORMANT_OUT_* */
} th_formant_request;
typedef struct {
    uint32_t sr, sr_analysis;
    uint32_t resampled;    /* 1: sr_analysis != sr, and rs is the pair's plan */
    uint32_t n_poles, win, hop, window, kind;
    th_resample_plan rs;
    uint64_t n_analysis;   /* n_a */
    uint64_t n_frames_total, frame_first, frame_end;
    double alpha;
} th_formant_plan;
typedef struct {
    uint64_t offset, length; /* into out, doubles; length = (frame_end - frame_first) (2 + n_poles) */
    uint64_t frame_first, frame_end;
    uint32_t sr_analysis, win, hop, reserved;
    uint64_t n_invalid, n_unconverged;
    uint64_t waveform_revision;
} th_formant_info;
TH_API int th_formant_defaults(th_formant_request *req);
TH_API int th_formant_plan_for(uint32_t sr, size_t n_samples, const th_formant_request *req, th_formant_plan *plan);
TH_API int th_formant_window(uint32_t window, uint32_t win, double *g /* win */);
TH_API int th_formant_start_points(uint32_t n_poles, double *z /* 2 n_poles: real parts, then imaginary parts */);
TH_API int th_formants_f64(const float *x, size_t n, uint32_t sr, const th_formant_request *req, uint64_t frame0, size_t n_frames,
                           double *out /* n_frames (2 + n_poles) */, uint64_t *counts /* 2, or NULL */);
TH_API int th_formant_frame_f64(const float *x, size_t n, uint32_t sr, const th_formant_request *req, uint64_t frame, double *r,
                                double *a, double *r0e, double *roots, uint32_t *sweeps, uint32_t *status);
TH_API int th_tm_get_formants(th_tm *tm, const th_formant_request *reqs, size_t n, double *out, size_t cap_doubles,
                              th_formant_info *info /* n */, size_t *out_len);
TH_API int th_tm_get_formant_track(th_tm *tm, const th_formant_request *req, double *out, size_t cap_doubles, th_formant_info *info);

/* ---------------------------------------------------------------- Align two tracks: lag, gain and null depth */
/* By how many samples a PROBE channel is shifted against a REFERENCE channel, with what gain it matches it, and how deep the two
 * null once shifted and scaled: the time-domain cross-correlation of a range of the reference with the probe over the lags
 * -D .. D, in f64, on the resident audio.  No reference implementation exists; these definitions are the contract.
 *   SIGN CONVENTION.  A positive lag means the probe is LATE: probe[n + l*] matches reference[n].  A host that wants the two on one
 *   time axis subtracts l* / sr seconds from the probe's time arguments (or draws the probe l* / sr seconds to the left).
 *   Request and plan.  th_align_request: the reference (ref_id, ref_ch, ref_which) and the probe (id, ch, which), `which` as
 *   th_tm_copy_audio; the two may be the same track, even the same channel.  [start_sec, end_sec) is a range of the REFERENCE;
 *   max_lag_sec >= 0, finite; kind TH_ALIGN_OUT_*; flags: TH_ALIGN_ABS or 0.  th_align_plan_for(sr_ref, n_ref, sr, n, req, &plan)
 *   (host) is the one place where numbers are made from seconds, all in C double: [s0, s1) = th_audio_sample_range(sr_ref, n_ref,
 *   start_sec, end_sec), N = s1 - s0; D = rint(max_lag_sec sr); the lags are l = -D .. D, n_lags = 2 D + 1, and an empty range has
 *   n_lags = 0.  TH_ERR_INVALID_ARG: a NaN anywhere, a bad range (as th_audio_sample_range), a negative or infinite max_lag_sec, an
 *   unknown kind, which or flag bit, a zero rate.  Then TH_ERR_UNSUPPORTED: sr_ref != sr; N > TH_ALIGN_MAX_REF; D >
 *   TH_ALIGN_MAX_LAG; N n_lags > TH_ALIGN_MAX_WORK.
 *   Arithmetic.  a[k] = ref[s0 + k], k < N; b[n] = the probe, +0 outside [0, n_b); indices are signed 64-bit.
 *     r[l] = sum over k < N of (double)a[k] (double)b[s0 + k + l].
 *   The product of two f32 is exact in f64, so whether a product and its addition are fused changes no bit.  Products with b outside
 *   the track are formed (with b = +0).  The ORDER of the additions depends on k alone: block j = k div TH_ALIGN_BLOCK (4096);
 *   inside a block, partial sum q = k mod 4 takes its terms in ascending k, from +0; the block's value is (p0 + p1) + (p2 + p3);
 *   group g = j div TH_ALIGN_GROUP_BLOCKS (32) adds its blocks' values in ascending j, from +0; r adds the groups' values in ascending
 *   g, from +0.  It does not depend on the lag, the piece, the batch, the reader slot, or th_tm against th_tmg.
 *   E(x, first, N): the same order over (double)x[first + k] (double)x[first + k] (x = +0 outside its track).  E_ref = E(ref, s0, N);
 *   E_probe = E(probe, s0 + l*, N).
 *   The host's step, on the read-back r, in C double with libm's sqrt and log10 (th_align_peak and the lines below it):
 *     the result is INVALID when n_lags = 0, when any r[l] or E_ref is not finite, or when E_ref <= 0;
 *     m = r (with TH_ALIGN_ABS: |r|, so that an inverted copy aligns too); l* = the smallest l at which m is largest;
 *     polarity = -1 when r[l*] < 0, else +1;
 *     delta (a parabola's vertex through m at l* - 1, l*, l* + 1): at the first or the last searched lag 0; otherwise den =
 *     (m- - 2 m0) + m+ and delta = den < 0 ? (0.5 (m- - m+)) / den : 0;
 *     r* = r[l*]; gain = r* / E_ref; resid = E_probe - r* gain (the product rounded, then the difference), 0 when that is negative;
 *     rho = r* / sqrt(E_ref E_probe); null_dB = 10 log10(resid / E_probe).
 *   gain is the factor by which the reference, shifted by l*, best matches the probe in the least-squares sense; null_dB is the energy
 *   of what is left of the probe's window after that match is subtracted, relative to the window's own energy (-inf: a perfect null).
 *   Output: doubles, requests back to back in request order.  TH_ALIGN_SUMMARY_DOUBLES = 10 per request: status (0 valid, 1
 *   invalid), l*, delta, r*, E_ref, E_probe, rho, gain, null_dB, polarity; an invalid result has status 1 and NaN in the other nine.
 *   kind TH_ALIGN_OUT_CURVE: the n_lags values r[-D .. D] follow (whatever the status).  r is additive over channels: a host that
 *   wants a joint fit over a track's channels adds their curves.  Where this text says "the same bits", a NaN is a NaN: its sign and
 *   payload are the machine's.
 *   info[i]: offset and length in doubles, sr, max_lag = D, [sample_start, sample_end) = [s0, s1), waveform_revision.
 *   Host functions, which run the kernel's own arithmetic (align_core.h) and give the reader's bits: th_xcorr_f64: r[i] = sum over k <
 *   n_a of a[k] b[first + i + k] for i < n_lags (a: the reference's range; b: the whole probe; first = s0 + the first lag);
 *   th_align_energy_f64: E(x, first, n_sum); th_align_peak: the step above up to delta (status, the peak's index into r, delta,
 *   polarity); th_align_f64: a whole request from two host channels (ids and channels of the request are not looked at).
 * th_tm_align_tracks / th_tm_align_track: a reader like th_tm_get_formants: shared lock, a reader slot's own stream; out == NULL or a
 * cap below *out_len: TH_ERR_BUFFER_TOO_SMALL with info and *out_len filled.  The first faulty request in request order decides; of
 * one request: an unknown probe id, then an unknown reference id: TH_ERR_NOT_FOUND; a bad channel or argument: TH_ERR_INVALID_ARG;
 * then TH_ERR_UNSUPPORTED as above.  On any error nothing is written to out.
 * Device memory is BOUNDED.  A request is cut into pieces of at most TH_ALIGN_PIECE_LAGS lags; a piece is one launch of the
 * correlation kernel (a workgroup: a tile of lags x one group of the reference, its group values into a scratch of n_groups x lags
 * doubles, at most 16 MiB), one of the fold over the groups into one of two record buffers, and one copy; piece k + 1 computes while
 * piece k is copied.  The two energies are small launches of the same order, E_probe after the host has found l*. */
#define TH_ALIGN_MAX_REF (1u << 22)
#define TH_ALIGN_MAX_LAG (1u << 20)
#define TH_ALIGN_MAX_WORK (1ull << 40)
#define TH_ALIGN_PIECE_LAGS 65536u
#define TH_ALIGN_BLOCK 4096u
#define TH_ALIGN_GROUP_BLOCKS 32u
#define TH_ALIGN_SUMMARY_DOUBLES 10u
#define TH_ALIGN_OUT_SUMMARY 0
#define TH_ALIGN_OUT_CURVE 1
#define TH_ALIGN_ABS 1u
typedef struct {
    size_t ref_id;
    uint32_t ref_ch, ref_which; /* which: 0 audio, 1 drawn, 2 original */
    size_t id;
    uint32_t ch, which;
    double start_sec, end_sec;  /* a range of the reference */
    double max_lag_sec;
    uint32_t kind, flags;       /* TH_ALIGN_OUT_*; TH_ALIGN_ABS or 0 */
} th_align_request;
typedef struct {
    uint32_t sr, max_lag;       /* max_lag = D */
    uint32_t kind, flags;
    uint64_t sample_start, sample_end; /* [s0, s1) of the reference */
    uint64_t n_lags;            /* 2 D + 1; 0 for an empty range */
    uint64_t length;            /* doubles of output: TH_ALIGN_SUMMARY_DOUBLES (+ n_lags for TH_ALIGN_OUT_CURVE) */
} th_align_plan;
typedef struct {
    uint64_t offset, length;    /* into out, doubles */
    uint32_t sr, max_lag;
    uint64_t sample_start, sample_end;
    uint64_t waveform_revision;
} th_align_info;
TH_API int th_align_plan_for(uint32_t sr_ref, size_t n_ref, uint32_t sr, size_t n, const th_align_request *req, th_align_plan *plan);
TH_API int th_xcorr_f64(const float *a, size_t n_a, const float *b, size_t n_b, int64_t first, size_t n_lags, double *r /* n_lags */);
TH_API int th_align_energy_f64(const float *x, size_t n, int64_t first, size_t n_sum, double *energy);
TH_API int th_align_peak(const double *r, size_t n_lags, uint32_t flags, double e_ref, uint32_t *status, size_t *peak, double *delta,
                         double *polarity);
TH_API int th_align_f64(const float *ref, size_t n_ref, uint32_t sr_ref, const float *probe, size_t n, uint32_t sr,
                        const th_align_request *req, double *out, size_t cap_doubles, size_t *out_len);
TH_API int th_tm_align_tracks(th_tm *tm, const th_align_request *reqs, size_t n, double *out, size_t cap_doubles,
                              th_align_info *info /* n */, size_t *out_len);
TH_API int th_tm_align_track(th_tm *tm, const th_align_request *req, double *out, size_t cap_doubles, th_align_info *info);

/* ---------------------------------------------------------------- TrackManager over several devices (one process) */
/* th_tmg: the th_tm_* calls above, call for call, with a th_tmg * in place of the th_tm *; a multi-GPU host swaps one for
 * the other.  Every result — updated ids, max_sr, db state, revisions, specs, images, tile bytes, batch offsets, render
 * metadata — is bit-identical to that of ONE th_tm holding all the tracks after the same sequence of calls.
 *   - Slots.  Each entry of `devices` is a slot with its own th_ctx and th_tm.  Duplicates are allowed ({0, 0}: two slots on
 *     one card, which is how a one-GPU box runs the N-slot code).  th_tmg_create checks, in this order: devices != NULL,
 *     1 <= n_devices <= 64, no negative entry (else TH_ERR_INVALID_ARG); a GPU at all (else TH_ERR_NO_DEVICE, no CPU
 *     fallback); every entry < th_device_count (else TH_ERR_INVALID_ARG).
 *   - Placement.  A track lives whole on one slot.  The new ids of an add_tracks batch (for an id given twice, its last
 *     entry) are placed longest-first by weight = n_samples x n_channels, ties in input order, each on the slot with the
 *     least resident weight, ties to the lowest slot (th_shard_assign starting from the resident loads).  A resident id
 *     that is added again is replaced on its own slot.  Tracks never migrate; removals do not rebalance.
 *   - The one coupling.  apply_track_list_changes, set_dB_range, set_setting and set_colormap fold every slot's channel
 *     (min, max) in ascending (id, ch) order and every track's sample rate into one (min_dB, max_dB, max_sr), as one th_tm
 *     does, and every slot quantises against it; when one slot must re-make all its images, every slot does.  updated_ids
 *     is the ascending union over the slots.
 *   - Concurrency.  The per-slot work of a mutator (staging, STFT, quantisation, pyramids) runs on one host thread per slot.
 *     A slot's failure is reported on the caller's thread (th_last_error) with the slot and its device.  Tile getters run on
 *     the caller's thread against the owning slot.  th_tmg has its own reader / writer lock: a tile reader never sees one
 *     slot re-made while another is not.
 *   - Transactions.  set_setting and add_tracks prepare on every slot, then commit everywhere or discard everywhere: a
 *     failure leaves every slot exactly as it was (nothing added anywhere, revisions unchanged).
 *   - Revisions.  One pair for the whole manager, moved exactly as one th_tm moves its own (lib.rs:192,221,243-245,265,284);
 *     every slot stamps its tiles with it.
 *   - Batched tiles.  get_spectrogram_tiles splits the requests by owner and serves the slots side by side; the records and
 *     offsets are those of one th_tm (request order, 64-byte boundaries). */
TH_API int th_tmg_create(const int *devices, size_t n_devices, th_tmg **out);
TH_API int th_tmg_destroy(th_tmg *tmg);
TH_API int th_tmg_n_devices(const th_tmg *tmg, size_t *n_devices);
/* the slot (index into `devices`) that owns track id; TH_ERR_NOT_FOUND when it is not resident */
TH_API int th_tmg_track_device(const th_tmg *tmg, size_t id, uint32_t *slot);
TH_API int th_tmg_set_colormap(th_tmg *tmg, const uint8_t *rgba, size_t bytes);
TH_API int th_tmg_set_setting(th_tmg *tmg, double win_ms, uint32_t t_overlap, uint32_t f_overlap, int freq_scale);
TH_API int th_tmg_set_dB_range(th_tmg *tmg, float dB_range);
TH_API int th_tmg_add_tracks(th_tmg *tmg, size_t n_tracks, const size_t *ids, const uint32_t *srs,
                             const uint32_t *n_channels, const float *const *channels_flat, const size_t *n_samples);
TH_API int th_tmg_remove_track(th_tmg *tmg, size_t id);
TH_API int th_tmg_apply_track_list_changes(th_tmg *tmg, size_t *updated_ids, size_t cap, size_t *n_updated,
                                           uint32_t *max_sr);
TH_API int th_tmg_get_db_state(const th_tmg *tmg, float *min_dB, float *max_dB, uint32_t *max_sr);
TH_API int th_tmg_spec_shape(const th_tmg *tmg, size_t id, uint32_t ch, size_t *n_frames, size_t *height);
TH_API int th_tmg_img_shape(const th_tmg *tmg, size_t id, uint32_t ch, size_t *img_height, size_t *img_width);
TH_API int th_tmg_copy_spec(th_tmg *tmg, size_t id, uint32_t ch, float *out, size_t capacity_floats);
TH_API int th_tmg_copy_img(th_tmg *tmg, size_t id, uint32_t ch, uint16_t *out, size_t capacity_px);
TH_API int th_tmg_revisions(const th_tmg *tmg, uint64_t *waveform_revision, uint64_t *spectrogram_revision);
TH_API int th_tmg_get_spectrogram_tile(th_tmg *tmg, size_t id, uint32_t ch, uint32_t level_x, uint32_t level_y,
                                       uint32_t tile_x, uint32_t tile_y, uint8_t *out, size_t out_capacity,
                                       size_t *out_len);
TH_API int th_tmg_get_spectrogram_tiles(th_tmg *tmg, const th_tile_request *reqs, size_t n, uint8_t *out,
                                        size_t out_capacity, size_t *offsets /* n + 1 */, size_t *out_len);
TH_API int th_tmg_get_waveform_tile(th_tmg *tmg, size_t id, uint32_t ch, uint32_t level, uint32_t tile_index,
                                    uint8_t *out, size_t out_capacity, size_t *out_len);
TH_API int th_tmg_get_audio_render_metadata(th_tmg *tmg, size_t id, uint32_t ch, double track_sec, int is_clipped,
                                            th_render_metadata *out);
TH_API int th_tmg_set_lod_source(th_tmg *tmg, int per_request);
TH_API int th_tmg_get_audio_stats(th_tmg *tmg, size_t id, th_audio_stats *out);
/* the common normalisation and clip guard: every slot prepares, then all commit or all discard; one global dB range is folded */
TH_API int th_tmg_set_common_normalize(th_tmg *tmg, int kind, float target);
TH_API int th_tmg_set_common_guard_clipping(th_tmg *tmg, int mode);
TH_API int th_tmg_get_common_dynamics(th_tmg *tmg, int *kind, float *target, int *mode);
TH_API int th_tmg_get_track_dynamics(th_tmg *tmg, size_t id, th_track_dynamics *out);
TH_API int th_tmg_get_guard_clip_stats(th_tmg *tmg, size_t id, th_guard_clip_stats *out, size_t cap, size_t *n);
TH_API int th_tmg_get_limiter_gain(th_tmg *tmg, size_t id, float *out, size_t cap, size_t *n);
TH_API int th_tmg_copy_audio(th_tmg *tmg, size_t id, uint32_t ch, int which, float *out, size_t cap);
/* spectra: the batch is split by owning slot and the slots are served side by side; the floats and infos are those of one th_tm
 * (request order, packed dense), the revision stamped is the manager's own */
TH_API int th_tmg_get_spectra(th_tmg *tmg, const th_spectrum_request *reqs, size_t n, float *out, size_t cap_floats,
                              th_spectrum_info *info /* n */, size_t *out_len);
TH_API int th_tmg_get_spectrum(th_tmg *tmg, size_t id, uint32_t ch, int kind, double start_sec, double end_sec, float *out,
                               size_t cap_floats, th_spectrum_info *info);

/* loudness meters: every id goes to its owning slot, the slots are served side by side; meters and series are those of one th_tm
 * (request order, packed dense), the revision stamped is the manager's own */
TH_API int th_tmg_get_loudness_meters(th_tmg *tmg, const size_t *ids, size_t n, th_loudness_meter *meters /* n */, double *series,
                                      size_t cap_doubles, size_t *out_len);
TH_API int th_tmg_get_loudness_meter(th_tmg *tmg, size_t id, th_loudness_meter *meter, double *series, size_t cap_doubles);

/* export: every request goes to its owning slot and the slots are served side by side, each writing its requests' bytes straight
 * into the caller's buffer; the bytes, offsets (zero padding included) and infos are those of one th_tm, the revision stamped is
 * the manager's own */
TH_API int th_tmg_export_pcm(th_tmg *tmg, const th_export_request *reqs, size_t n, uint8_t *out, size_t cap_bytes,
                             th_export_info *info /* n */, size_t *out_len);
TH_API int th_tmg_export_wav(th_tmg *tmg, const th_export_request *req, uint8_t *out, size_t cap_bytes,
                             th_export_info *info /* may be NULL */, size_t *out_len);
/* export at a target sample rate: as above; every slot keeps its own scratch and coefficient table */
TH_API int th_tmg_export_pcm_at(th_tmg *tmg, const th_export_at_request *reqs, size_t n, uint8_t *out, size_t cap_bytes,
                                th_export_info *info /* n */, size_t *out_len);
TH_API int th_tmg_export_wav_at(th_tmg *tmg, const th_export_at_request *req, uint8_t *out, size_t cap_bytes,
                                th_export_info *info /* may be NULL */, size_t *out_len);
/* band-limited export: as above, bit-identical to one th_tm; every slot keeps the row of its own last filter */
TH_API int th_tmg_export_pcm_band(th_tmg *tmg, const th_export_band_request *reqs, size_t n, uint8_t *out, size_t cap_bytes,
                                  th_export_info *info /* n */, size_t *out_len);
TH_API int th_tmg_export_wav_band(th_tmg *tmg, const th_export_band_request *req, uint8_t *out, size_t cap_bytes,
                                  th_export_info *info /* may be NULL */, size_t *out_len);
/* FLAC export: as above; every slot keeps its own FLAC scratch, files and infos are those of one th_tm */
TH_API int th_tmg_export_flac(th_tmg *tmg, const th_export_request *reqs, size_t n, uint8_t *out, size_t cap_bytes,
                              th_export_info *info /* n */, size_t *out_len);
TH_API int th_tmg_export_flac_ex(th_tmg *tmg, const th_export_request *reqs, size_t n, uint32_t flags, uint8_t *out, size_t cap_bytes,
                                 th_export_info *info /* n */, size_t *out_len);

/* figures: every request goes to its owning slot and the slots are served side by side, each copying its records straight into the
 * caller's buffer; bytes, offsets and infos are those of one th_tm, the revision stamped is the manager's own */
TH_API int th_tmg_figure_box(th_tmg *tmg, size_t id, uint32_t ch, double start_sec, double end_sec, double hz_min, double hz_max,
                             double *left, double *top, double *width, double *height);
TH_API int th_tmg_render_figures(th_tmg *tmg, const th_figure_request *reqs, size_t n, uint8_t *out, size_t cap_bytes,
                                 th_figure_info *info /* n */, size_t *out_len);
TH_API int th_tmg_render_figure(th_tmg *tmg, const th_figure_request *req, uint8_t *out, size_t cap_bytes, th_figure_info *info);

/* waveform envelopes and lanes: the same; a request's bytes are those of one th_tm, bit for bit */
TH_API int th_tmg_get_envelopes(th_tmg *tmg, const th_envelope_request *reqs, size_t n, float *out, size_t cap_floats,
                                th_envelope_info *info /* n */, size_t *out_len);
TH_API int th_tmg_get_envelope(th_tmg *tmg, const th_envelope_request *req, float *out, size_t cap_floats, th_envelope_info *info);
TH_API int th_tmg_render_waveform_figures(th_tmg *tmg, const th_waveform_figure_request *reqs, size_t n, uint8_t *out,
                                          size_t cap_bytes, th_waveform_figure_info *info /* n */, size_t *out_len);
TH_API int th_tmg_render_waveform_figure(th_tmg *tmg, const th_waveform_figure_request *req, uint8_t *out, size_t cap_bytes,
                                         th_waveform_figure_info *info);

/* formant candidates: the same; a request's doubles and counts are those of one th_tm, bit for bit */
TH_API int th_tmg_get_formants(th_tmg *tmg, const th_formant_request *reqs, size_t n, double *out, size_t cap_doubles,
                               th_formant_info *info /* n */, size_t *out_len);
TH_API int th_tmg_get_formant_track(th_tmg *tmg, const th_formant_request *req, double *out, size_t cap_doubles, th_formant_info *info);

/* alignment: the same; the probe's slot runs a request.  A reference that lives on another slot is copied, its range only (at most
 * TH_ALIGN_MAX_REF floats), through pinned host memory into the probe's slot before the run, so a request's doubles are those of one
 * th_tm, bit for bit */
TH_API int th_tmg_align_tracks(th_tmg *tmg, const th_align_request *reqs, size_t n, double *out, size_t cap_doubles,
                               th_align_info *info /* n */, size_t *out_len);
TH_API int th_tmg_align_track(th_tmg *tmg, const th_align_request *req, double *out, size_t cap_doubles, th_align_info *info);

/* Test and measurement entry points (kernel selectors for A/B runs, per-launch kernel timing, replacing a resident image
 * with given pixels) are NOT part of this interface: include/thesia_amd_testing.h declares them; a thesia host binds none. */

#endif /* THESIA_AMD_H */
