// api.hip — C ABI: errors, host helpers, device context, SpectrogramAnalyzer plan and the
// device-pointer ("layer A") entry points.  The TrackManager mirror lives in track_manager.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "common.h"
#include "context.h"
#include "export_core.h"
#include "flac_block.h"
#include "host_math.h"
#include "kernels.h"
#include "mel_fuse.h"
#include "resample_core.h"
#include "track_manager_internal.h"  // wav_header_checked
#if !defined(TH_MEL_BAND_TAPS_2048)
#define TH_MEL_BAND_TAPS_2048 64u  // (measured thresholds: th_plan_create)
#define TH_MEL_BAND_TAPS_1024 80u
#endif
#if !defined(TH_MEL_BAND_SPREAD)
#define TH_MEL_BAND_SPREAD 1  // the banded tables' first bins on distinct LDS banks (mel_fuse.h; 0: as the filters start, for A/B runs)
#endif

// ------------------------------------------------------------------------------------------ errors
namespace th {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_err; }
}  // namespace th

using namespace th;

TH_API const char *th_last_error(void) { return th::get_error(); }
TH_API int th_version(void) { return 100; }

TH_API int th_device_count(int *count) {
    TH_TRY
    TH_REQUIRE(count, "count is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return TH_OK;
    TH_CATCH
}

// ------------------------------------------------------------------------------------------ host helpers
TH_API int th_calc_framing_params(double win_ms, uint32_t t_overlap, uint32_t f_overlap, uint32_t sr, size_t *hop,
                                  size_t *win, size_t *n_fft) {
    TH_TRY
    TH_REQUIRE(hop && win && n_fft, "output pointer is NULL");
    // the reference asserts these in set_spec_setting (src-tauri/src/lib.rs:275-277)
    TH_REQUIRE(win_ms > 0. && t_overlap >= 1 && f_overlap >= 1, "win_ms > 0, t_overlap >= 1, f_overlap >= 1 required");
    calc_framing_params(win_ms, t_overlap, f_overlap, sr, hop, win, n_fft);
    return TH_OK;
    TH_CATCH
}

TH_API int th_stft_n_frames(size_t n_samples, size_t win, size_t hop, size_t *n_frames) {
    TH_TRY
    TH_REQUIRE(n_frames, "n_frames is NULL");
    TH_REQUIRE(win >= 1 && hop >= 1, "win and hop must be >= 1");
    *n_frames = stft_n_frames(n_samples, win, hop);
    return TH_OK;
    TH_CATCH
}

TH_API int th_calc_normalized_win(size_t win, size_t n_fft, float *out) {
    TH_TRY
    TH_REQUIRE(out, "out is NULL");
    TH_REQUIRE(win > 1 && n_fft >= 1, "win must be > 1");  // windows.rs:73 debug_assert!(size > 1)
    const std::vector<float> w = normalized_hann(win, n_fft);
    std::memcpy(out, w.data(), sizeof(float) * win);
    return TH_OK;
    TH_CATCH
}

TH_API int th_calc_mel_fb(uint32_t sr, size_t n_fft, size_t n_mel, float fmin, float fmax, int do_norm, float *out) {
    TH_TRY
    TH_REQUIRE(out, "out is NULL");
    TH_REQUIRE(n_fft % 2 == 0 && n_mel != 0, "n_fft must be even and n_mel non-zero");  // lib.rs:59-60
    const std::vector<float> fb = calc_mel_fb(sr, n_fft, n_mel, fmin, fmax, do_norm != 0);
    std::memcpy(out, fb.data(), sizeof(float) * fb.size());
    return TH_OK;
    TH_CATCH
}

TH_API int th_mel_default_n_mel(uint32_t sr, size_t n_fft, size_t *n_mel) {
    TH_TRY
    TH_REQUIRE(n_mel, "n_mel is NULL");
    TH_REQUIRE(sr > 0 && n_fft >= 2 && n_fft % 2 == 0, "sr > 0 and even n_fft >= 2 required");
    *n_mel = mel_default_n_mel(sr, n_fft);
    return TH_OK;
    TH_CATCH
}

TH_API int th_hz_range_to_idx(int freq_scale, float hz_min, float hz_max, uint32_t sr, size_t n, size_t *i_start,
                              size_t *i_end) {
    TH_TRY
    TH_REQUIRE(i_start && i_end, "output pointer is NULL");
    TH_REQUIRE(freq_scale == TH_FREQ_LINEAR || freq_scale == TH_FREQ_MEL, "bad freq_scale %d", freq_scale);
    hz_range_to_idx(freq_scale, hz_min, hz_max, sr, n, i_start, i_end);
    return TH_OK;
    TH_CATCH
}

TH_API int th_global_db_range(const float *mins, const float *maxs, size_t n, float dB_range, float *min_dB,
                              float *max_dB) {
    TH_TRY
    TH_REQUIRE(min_dB && max_dB && (n == 0 || (mins && maxs)), "NULL pointer");
    global_db_range(mins, maxs, n, dB_range, min_dB, max_dB);
    return TH_OK;
    TH_CATCH
}

TH_API int th_shard_assign(const uint64_t *weights, size_t n_units, uint32_t world, uint32_t *owner) {
    TH_TRY
    TH_REQUIRE(world >= 1, "world must be >= 1");
    TH_REQUIRE(n_units == 0 || (weights && owner), "NULL pointer");
    shard_assign(weights, n_units, world, owner);
    return TH_OK;
    TH_CATCH
}

TH_API int th_spectrogram_tile_geometry(size_t W, size_t Hh, uint32_t lx, uint32_t ly, uint32_t tx, uint32_t ty,
                                        th_tile_geom *geom) {
    TH_TRY
    TH_REQUIRE(geom, "geom is NULL");
    const TileGeom g = spectrogram_tile_geometry(W, Hh, lx, ly, tx, ty);
    geom->width = (uint32_t)g.width;
    geom->height = (uint32_t)g.height;
    geom->origin_x = (uint32_t)g.origin_x;
    geom->origin_y = (uint32_t)g.origin_y;
    geom->lod_width = g.lod_w;
    geom->lod_height = g.lod_h;
    return TH_OK;
    TH_CATCH
}

TH_API int th_waveform_tile_geometry(size_t n_samples, uint32_t level, uint32_t tile_index, size_t *start,
                                     size_t *bin_count, size_t *samples_per_bin) {
    TH_TRY
    TH_REQUIRE(start && bin_count && samples_per_bin, "output pointer is NULL");
    waveform_tile_geometry(n_samples, level, tile_index, start, bin_count, samples_per_bin);
    return TH_OK;
    TH_CATCH
}

// ------------------------------------------------------------------------------------------ context
TH_API int th_ctx_create(int device, void *hip_stream, th_ctx **out) {
    return th_ctx_create_ex(device, hip_stream, hip_stream != nullptr, out);
}

TH_API int th_ctx_create_ex(int device, void *hip_stream, int use_given_stream, th_ctx **out) {
    TH_TRY
    TH_REQUIRE(out, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(TH_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    TH_REQUIRE(device >= 0 && device < n, "device %d out of range (have %d)", device, n);
    TH_HIP(hipSetDevice(device));
    std::unique_ptr<th_ctx> c(new th_ctx());
    c->device = device;
    {
        int n_cu = 0;
        if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n_cu > 0)
            c->n_cu = (uint32_t)n_cu;
    }
    if (use_given_stream) {
        c->stream = reinterpret_cast<hipStream_t>(hip_stream);  // NULL = legacy default stream
        c->own_stream = false;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) return fail(TH_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
        c->own_stream = true;
    }
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) return fail(TH_ERR_HIP, "hipEventCreate failed");
    *out = c.release();
    return TH_OK;
    TH_CATCH
}

TH_API int th_ctx_destroy(th_ctx *c) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("destroying the context"));
    if (!c) return TH_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    delete c;
    return TH_OK;
    TH_CATCH
}

TH_API int th_ctx_synchronize(th_ctx *c) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("synchronising the stream"));
    TH_REQUIRE(c, "ctx is NULL");
    TH_HIP(hipStreamSynchronize(c->stream));
    return TH_OK;
    TH_CATCH
}

struct th_graph {
    th_ctx *ctx = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

// The capture of this thread (hipStreamCaptureModeThreadLocal: begin, the captured calls and end are one thread's)
namespace {
struct CaptureState {
    th_ctx *ctx = nullptr;
    bool refused = false;
    char what[160] = "";
};
thread_local CaptureState g_capture;
}  // namespace

int th::refuse_while_capturing(const char *what) {
    if (g_capture.ctx == nullptr) return TH_OK;
    if (!g_capture.refused) snprintf(g_capture.what, sizeof g_capture.what, "%s", what);
    g_capture.refused = true;
    return fail(TH_ERR_HIP, "%s is not possible while this thread is capturing (th_ctx_capture_begin); end the capture: it yields "
                            "no graph", what);
}

TH_API int th_ctx_capture_begin(th_ctx *c) {
    TH_TRY
    TH_REQUIRE(c, "ctx is NULL");
    TH_REQUIRE(g_capture.ctx == nullptr, "this thread is capturing already (one capture per thread at a time)");
    TH_HIP(hipSetDevice(c->device));
    if (c->stream == nullptr) {  // the legacy default stream: record on a stream of the context's own (context.h)
        if (c->capture_stream == nullptr) TH_HIP(hipStreamCreateWithFlags(&c->capture_stream, hipStreamNonBlocking));
        c->stream = c->capture_stream;
        c->capture_swapped = true;
    }
    const hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (c->capture_swapped) c->stream = nullptr;
        c->capture_swapped = false;
        return fail(TH_ERR_HIP, "hipStreamBeginCapture: %s", hipGetErrorString(e));
    }
    g_capture = CaptureState();
    g_capture.ctx = c;
    return TH_OK;
    TH_CATCH
}

TH_API int th_ctx_capture_end(th_ctx *c, th_graph **out) {
    TH_TRY
    TH_REQUIRE(c && out, "NULL argument");
    *out = nullptr;
    TH_REQUIRE(g_capture.ctx == c, "th_ctx_capture_begin was not called on this context by this thread");
    const CaptureState cap = g_capture;
    g_capture = CaptureState();
    (void)hipSetDevice(c->device);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(c->stream, &g);
    if (c->capture_swapped) c->stream = nullptr;  // (back on the legacy default stream: the graph is launched there)
    c->capture_swapped = false;
    if (e != hipSuccess || g == nullptr || cap.refused) {
        (void)hipGetLastError();
        if (g) (void)hipGraphDestroy(g);
        if (cap.refused) return fail(TH_ERR_HIP, "no graph: a call was refused while capturing (%s)", cap.what);
        return fail(TH_ERR_HIP, "stream capture failed or was invalidated: %s", hipGetErrorString(e));
    }
    hipGraphExec_t x = nullptr;
    const hipError_t e2 = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    if (e2 != hipSuccess) {
        (void)hipGetLastError();
        (void)hipGraphDestroy(g);
        return fail(TH_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e2));
    }
    th_graph *gr = new th_graph;
    gr->ctx = c;
    gr->graph = g;
    gr->exec = x;
    *out = gr;
    return TH_OK;
    TH_CATCH
}

TH_API int th_graph_launch(th_graph *g) {
    TH_TRY
    TH_REQUIRE(g && g->exec, "graph is NULL");
    TH_HIP(hipSetDevice(g->ctx->device));
    TH_HIP(hipGraphLaunch(g->exec, g->ctx->stream));
    return TH_OK;
    TH_CATCH
}

TH_API int th_graph_destroy(th_graph *g) {
    TH_TRY
    if (!g) return TH_OK;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    return TH_OK;
    TH_CATCH
}

TH_API int th_dev_alloc(th_ctx *c, size_t bytes, void **dptr) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("th_dev_alloc"));
    TH_REQUIRE(c && dptr, "NULL argument");
    *dptr = nullptr;
    TH_HIP(hipSetDevice(c->device));
    TH_HIP(hipMalloc(dptr, bytes ? bytes : 1));
    return TH_OK;
    TH_CATCH
}
TH_API int th_dev_free(th_ctx *c, void *dptr) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("th_dev_free"));
    TH_REQUIRE(c, "ctx is NULL");
    if (dptr) {
        TH_HIP(hipSetDevice(c->device));
        TH_HIP(hipStreamSynchronize(c->stream));
        TH_HIP(hipFree(dptr));
    }
    return TH_OK;
    TH_CATCH
}
TH_API int th_dev_upload(th_ctx *c, void *dst, const void *src, size_t bytes) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("th_dev_upload (a copy from host memory)"));
    TH_REQUIRE(c && (bytes == 0 || (dst && src)), "NULL argument");
    if (bytes) {
        TH_HIP(hipSetDevice(c->device));
        TH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
        TH_HIP(hipStreamSynchronize(c->stream));
    }
    return TH_OK;
    TH_CATCH
}
TH_API int th_dev_download(th_ctx *c, void *dst, const void *src, size_t bytes) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("th_dev_download (a copy to host memory)"));
    TH_REQUIRE(c && (bytes == 0 || (dst && src)), "NULL argument");
    if (bytes) {
        TH_HIP(hipSetDevice(c->device));
        TH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
        TH_HIP(hipStreamSynchronize(c->stream));
    }
    return TH_OK;
    TH_CATCH
}
TH_API int th_dev_copy(th_ctx *c, void *d_dst, const void *d_src, size_t bytes) {
    TH_TRY
    TH_REQUIRE(c && (bytes == 0 || (d_dst && d_src)), "NULL argument");
    TH_REQUIRE(((reinterpret_cast<uintptr_t>(d_dst) | reinterpret_cast<uintptr_t>(d_src) | bytes) & 15u) == 0,
               "pointers and size must be multiples of 16 bytes");
    TH_HIP(hipSetDevice(c->device));
    TH_HIP(launch_copy_f4(d_src, d_dst, bytes, c->stream));
    return TH_OK;
    TH_CATCH
}
TH_API int th_timer_start(th_ctx *c) {
    TH_TRY
    TH_REQUIRE(c, "ctx is NULL");
    TH_HIP(hipSetDevice(c->device));
    TH_HIP(hipEventRecord(c->ev0, c->stream));
    return TH_OK;
    TH_CATCH
}
TH_API int th_timer_stop_ms(th_ctx *c, float *ms) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("reading a timer"));
    TH_REQUIRE(c && ms, "NULL argument");
    TH_HIP(hipSetDevice(c->device));
    TH_HIP(hipEventRecord(c->ev1, c->stream));
    TH_HIP(hipEventSynchronize(c->ev1));
    TH_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return TH_OK;
    TH_CATCH
}

// ------------------------------------------------------------------------------------------ plan
namespace th {

int DeviceTable::ensure(size_t bytes) {
    if (bytes <= cap) return TH_OK;
    TH_CHECK(refuse_while_capturing("allocating a scratch buffer or a descriptor table"));
    if (dptr) {
        TH_HIP(hipFree(dptr));
        dptr = nullptr;
        cap = 0;
    }
    size_t want = bytes < 4096 ? 4096 : bytes + bytes / 2;
    TH_HIP(hipMalloc(&dptr, want));
    cap = want;
    last.clear();
    return TH_OK;
}

// Upload `bytes` of `src` unless the table already holds exactly these bytes (bench loops and
// repeated tile requests re-send identical descriptor tables).  Synchronous on purpose: the
// previous launch may still be reading the old table.
int DeviceTable::upload(hipStream_t s, const void *src, size_t bytes) {
    if (bytes == last.size() && bytes && std::memcmp(last.data(), src, bytes) == 0) return TH_OK;
    TH_CHECK(refuse_while_capturing("uploading a descriptor table (a first call, or one with other descriptors)"));
    TH_HIP(hipStreamSynchronize(s));
    int rc = ensure(bytes);
    if (rc != TH_OK) return rc;
    if (bytes) TH_HIP(hipMemcpy(dptr, src, bytes, hipMemcpyHostToDevice));
    last.assign(static_cast<const unsigned char *>(src), static_cast<const unsigned char *>(src) + bytes);
    return TH_OK;
}

void DeviceTable::release() {
    if (dptr) (void)hipFree(dptr);
    dptr = nullptr;
    cap = 0;
    last.clear();
}

}  // namespace th

// Fills p.route from the plan's geometry, the tables th_plan_create built and the selector: the one place that decides which
// kernels a launch runs.  The table-fit checks see p.g (phased = 0); the frame-loop checks behind phase_mode see the launch's.
static void resolve_route(th_plan &p) {
    using R = StftRoute;
    const StftGeom &g = p.g;
    const int k = p.kernel_choice, wv = p.wave_waves;
    R r;
    r.block_plan = stft_is_block_plan(g);
    const bool wave = k != SEL_GENERIC && stft_wave_supported(g) && (g.n_mel == 0 || p.d_mel_bt != nullptr);
    r.no_wave_kernel = k >= SEL_WAVE && !wave;
    // n_fft 8192 .. 65536: the block or the subwave plan (stft_subwave_default: the sizes where the subwave plan is the default).
    // Mel plans at n_fft 16384 that have a moment table: the workgroup-per-frame kernel with the filterbank in its epilogue at EVERY
    // hop.  For linear rows the subwave plan is the faster one at hops other than n_fft / 4 (0.63 against 0.67 ms at 16320 / 4080,
    // the UI's 340 ms window), but it has no epilogue and would need the second kernel: 0.99 against 0.82 ms there, 1.23 against 1.04
    // at 12000 / 3000, 1.79 against 1.50 at 16320 / 2040 (64 ch x 30 s).  Selector 12 (the two kernels) keeps the size's default.
    r.long_plan = k == SEL_BLOCK ? 1 : k == SEL_SUBWAVE ? 2
                : (g.n_mel != 0 && g.log2_nc == 13 && p.d_mel_mom != nullptr && k != SEL_MEL_TWO_KERNELS) ? 1
                : stft_subwave_default(g) ? 2 : 1;
    // mel plans on the wave kernels: the filterbank fused into the FFT kernel's epilogue where one of its table forms applies, else
    // amplitude rows out of the FFT kernel and a second mel kernel
    bool fused = false, mom_small = false, bsum_fits = false;
    if (g.n_mel != 0 && wave && k != SEL_MEL_AMP && k != SEL_MEL_MFMA) {
        bsum_fits = k != SEL_MEL_PIECES && p.d_mel_bsum != nullptr && stft_wave_mel_fits(g, wv, p.mel_bsum_words, true);
        const bool pieces_fit = p.d_mel_fuse != nullptr && stft_wave_mel_fits(g, wv, p.mel_fuse_words);
        // n_fft 512 .. 2048 under more mels than an LDS table form holds (low sample rates under long windows, or f_overlap 2 / 4):
        // the moment form with its table in global memory, as at n_fft 4096 (one-frame epilogue; any frame loop of the size).
        // n_fft 512 (four frames per wave): where the banded rows table does not exist — filters wider than its 8 bins: 10 / 20 ms
        // windows at 16 .. 48 kHz.  Selectors 12 / 8 keep the two kernels / the table forms.
        if (g.log2_nc >= 8 && g.log2_nc <= 10 && p.d_mel_mom != nullptr && k != SEL_MEL_TWO_KERNELS && k != SEL_MEL_PIECES)
            mom_small = g.log2_nc == 8 ? p.d_mel_rows == nullptr && stft_wave_multi_applies(g, 2) && stft_wave_multi_mel_fits(g, wv, 0)
                                       : !bsum_fits && !pieces_fit && stft_wave_mel_fits(g, wv, 0, true);
        if (g.log2_nc == 11)  // n_fft 4096 (round 6): the moment form as the FFT kernel's epilogue — no table in LDS (the eight slabs
            // leave none), any mel count; instantiated for hop 1024 and for the even-offset grid-aligned shapes of the 96 / 88.2 kHz
            // defaults (not when selector 4 switches that mode off)
            fused = k != SEL_MEL_TWO_KERNELS && p.d_mel_mom != nullptr && stft_wave_mel_fits(g, wv, 1, true);
        else if (g.log2_nc == 12 || g.log2_nc == 13)  // n_fft 8192 / 16384 (round 6): the same moment form in the epilogue of the
            // workgroup-per-frame kernel, where that kernel is the plan that runs
            fused = k != SEL_MEL_TWO_KERNELS && p.d_mel_mom != nullptr && stft_block_mel_fused_applies(g, r.long_plan);
        else if (g.log2_nc == 8)  // n_fft 512 under narrow filters: the banded sums of mel_rows_kernel as the epilogue of the four-frames-per-wave kernel
            fused = (p.d_mel_rows != nullptr && stft_wave_multi_mel_fits(g, wv, p.mel_rows_groups * (uint32_t)(MEL_ROWS_W + 1) * 64u)) || mom_small;
        else
            fused = bsum_fits || pieces_fit || mom_small;
    }
    const bool mel_amp = g.n_mel != 0 && wave && !fused;
    if (fused)
        r.mel_fused = (g.log2_nc >= 11 || mom_small) ? (r.block_plan ? R::MelFused::MomentLanes : R::MelFused::Moment)
                    : g.log2_nc == 8 ? R::MelFused::Rows
                    // frame pairs (round 5): two consecutive frames per pass over the table; selector 13 keeps the one-frame epilogue (A/B)
                    : bsum_fits ? (k != SEL_MEL_ONE_FRAME && stft_wave_mel_pair_applies(g, wv, p.mel_bsum_reach) ? R::MelFused::BandedPairs : R::MelFused::Banded)
                    : R::MelFused::Pieces;
    if (mel_amp)
        r.mel_second = (p.d_mel_rows != nullptr && k != SEL_MEL_MFMA) ? R::MelSecond::Rows
                     : (g.log2_nc >= 11 && p.d_mel_bsum != nullptr && k != SEL_MEL_MFMA) ? R::MelSecond::BandRows : R::MelSecond::Mfma;
    const int mode = r.out_mode();
    // phased mode of the wave kernel (hop = 480-style framings): frames are loaded from the 128-sample grid below their first window
    // sample (not with the fused mel epilogue unless selector 5 asks for it: measured no gain there, with or without idle gaps —
    // 48 kHz / 347 mels 0.522 vs 0.521 ms, 44.1 kHz / 370 mels 0.513 vs 0.541 — the window then comes from LDS instead of
    // registers and the mel kernel is not bound by its loads)
    // (n_fft 4096 — the 40 ms default at 88.2 / 96 kHz — also with amplitude output for the matrix-core mel kernel)
    if (wave && (!mel_amp || g.log2_nc == 11) && (!fused || k == SEL_PHASE_FUSED || g.log2_nc == 11) && k != SEL_NO_PHASE && p.d_wtab_phased != nullptr)
        r.phase_mode = fused ? stft_wave_mel_phase_mode(g, wv) : stft_wave_phased_mode(g, wv);
    StftGeom gl = g;  // the launch's geometry
    gl.phased = (uint32_t)r.phase_mode;
    r.waves = wv > 0 ? wv : stft_wave_default_waves(gl);
    const bool multi = wave && stft_wave_multi_applies(gl, mode);
    // (multi-frame kernel with staged loads and hop % 4 == 2: see stft_wave_multi_tail_guard)
    if (multi && g.log2_nc == 8) r.tail_guard = stft_wave_multi_tail_guard(gl);
    // boundary frames of channels with at least n_fft samples also go to the wave kernel (one-frame chunks with a
    // reflect-indexed fetch): no second launch on the fast path.  Not on the matrix-core mel path (its amplitude rows
    // are laid out for the interior jobs), not for channels shorter than n_fft (a single reflection is not enough there).
    r.edges_in_wave = wave && !mel_amp && r.phase_mode == 0 && !r.block_plan;
    r.sweep = wave && k == SEL_SWEEP && p.wave_chunk == 0 && g.n_mel == 0 && r.phase_mode == 0 && stft_wave_sweep_applies(gl, wv, 0);
    r.packed = k == SEL_PACKED;
    // n_fft 512, linear dB: four frames per wave (stft_wave_multi.h).  The same plan with two frames per wave exists for
    // n_fft 1024 (selector 6) but measures 0.72 ms against 0.64 for the one-frame plan on the bench tracks (it reloads
    // every frame in full: 16 loads per iteration against 4), so 1024 keeps the one-frame kernel by default.
    // (n_fft 32768, round 5: sixteen wave transforms + a combining pass, kernels_stft_long.hip; selector 14 keeps the block kernel)
    if (!wave) r.main = p.bluestein() ? R::Main::Bluestein : R::Main::Generic;
    else if (multi && (g.log2_nc == 8 || k == SEL_MULTI_1024)) r.main = R::Main::WaveMulti;
    else if (!r.block_plan) r.main = R::Main::Wave;
    else r.main = (mode != 2 && stft_subwave_applies(g) && p.d_twc != nullptr && r.long_plan == 2) ? R::Main::Subwave : R::Main::Block;
    static const char *const main_name[] = {"stft_generic_kernel", "stft_bluestein_kernel", "stft_wave_kernel", "stft_wave_kernel",
                                            "stft_block_kernel", "stft_subwave_kernel"};
    static const char *const second_name[] = {"", "+mel_rows_kernel", "+mel_band_rows_kernel", "+mel_mfma_kernel"};
    std::snprintf(r.name, sizeof r.name, "%s%s%s", main_name[(int)r.main], fused ? "(fused mel)" : "", second_name[(int)r.mel_second]);
    p.route = r;
}

TH_API int th_plan_create(th_ctx *c, uint32_t sr, size_t win, size_t hop, size_t n_fft, int freq_scale,
                          size_t n_mel, th_plan **out) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("creating a plan"));
    TH_REQUIRE(c && out, "NULL argument");
    *out = nullptr;
    TH_REQUIRE(freq_scale == TH_FREQ_LINEAR || freq_scale == TH_FREQ_MEL, "bad freq_scale %d", freq_scale);
    TH_REQUIRE(win > 1 && hop >= 1 && win <= n_fft, "need 1 < win <= n_fft and hop >= 1 (win=%zu hop=%zu n_fft=%zu)",
               win, hop, n_fft);
    TH_REQUIRE(sr > 0, "sr must be > 0");
    // Any power of two from 2 to 2^20: what SpecSetting::calc_framing_params (spectrogram.rs:56-98) yields for every window
    // the UI accepts with f_overlap a power of two — winMillisec has a lower bound only (tracks.ts:205, Control.tsx:96-107),
    // so e.g. 400 ms at 48 kHz is n_fft 32768 and 1 ms at 4 kHz is n_fft 4.  (The reference's realfft takes any length: a
    // non-power-of-two n_fft needs f_overlap = 3, 5, ..., which no control offers.)
    // Round 5: n_fft = 2^a * odd with a >= 1 and odd <= 63 — f_overlap = 3, 5, 6, 7, ... (spectrogram.rs:66-72: n_fft =
    // next_pow2(win) * f_overlap; no UI control offers them, the reference's realfft plans any length) run on the generic
    // kernel, which takes the odd factor as one more Stockham pass.
    size_t odd_part = n_fft;
    while (odd_part > 1 && odd_part % 2 == 0) odd_part /= 2;
    // Round 6: an odd factor above 63 (f_overlap = 67, 71, 130, ...) runs as a chirp-z convolution (stft_bluestein_kernel): every
    // even n_fft up to TH_MAX_N_FFT is planned.  (n_fft = next_pow2(win) * f_overlap is even for every win > 1.)
    if (n_fft < 2 || n_fft % 2 != 0 || n_fft > TH_MAX_N_FFT)
        return fail(TH_ERR_UNSUPPORTED, "n_fft=%zu: supported is every even n_fft from 2 to %u", n_fft, (unsigned)TH_MAX_N_FFT);
    TH_HIP(hipSetDevice(c->device));

    std::unique_ptr<th_plan> owner(new th_plan());  // (a failure below frees the plan and what it has uploaded so far)
    th_plan *p = owner.get();
    p->ctx = c;
    p->sr = sr;
    p->freq_scale = freq_scale;
    StftGeom &g = p->g;
    g = stft_geom(win, hop, n_fft);

    // every table is built on the host (stft_plan.h, mel_fuse.h, host_math.h) and uploaded as it is:
    // window (windows.rs), twiddles W_{n_fft}^i and the wave kernels' window tables (grid-aligned forms: kernels_stft.hip)
    const std::vector<float> w = normalized_hann(win, n_fft);
    const std::vector<cf32> tw = build_twiddles(n_fft);
    {
        const WaveWindowHost ww = build_wave_window(w.data(), win, n_fft, th::stft_wave_phased_mode(g, 0));
        TH_CHECK(p->d_wtab.fill(ww.wtab));
        if (!ww.phased.empty()) TH_CHECK(p->d_wtab_phased.fill(ww.phased));
    }
    TH_CHECK(p->d_window.fill(w));
    {
        const uint32_t zero[4] = {0, 0, 0, 0};  // [0] chunk queue head (rewound by wave_post_kernel after every launch), [1..3] spare
        TH_CHECK(p->d_queue_head.fill(zero, sizeof zero));
    }
    TH_CHECK(p->d_tw.fill(tw));
    if (odd_part > th::STFT_MAX_DIRECT_ODD) {  // Bluestein plan: chirp, FFT_M(b), twiddles of the M-point passes and of the split pass (doubles)
        const BluesteinTables bt = bluestein_tables(n_fft, th::stft_bluestein_m(g));
        TH_CHECK(p->d_bs_chirp.fill(bt.chirp));
        TH_CHECK(p->d_bs_bhat.fill(bt.bhat));
        TH_CHECK(p->d_bs_twm.fill(bt.twm));
        TH_CHECK(p->d_bs_tws.fill(bt.tws));
    }
    if (th::stft_subwave_applies(g)) {  // n_fft 32768: per-thread constants of stft_subwave_kernel's combining pass
        std::vector<cf32> twc(th::stft_subwave_twc_len(g));
        th::stft_subwave_build_twc(g, tw.data(), twc.data());
        TH_CHECK(p->d_twc.fill(twc));
    }
    if (freq_scale == TH_FREQ_MEL) {
        if (n_mel == 0) n_mel = mel_default_n_mel(sr, n_fft);  // calc_mel_fb_default, lib.rs:91-103
        if (n_mel == 0 || n_mel > 65535) return fail(TH_ERR_INVALID_ARG, "n_mel=%zu out of range", n_mel);
        // the dense (F x n_mel) filterbank of calc_mel_fb (src-common/src/lib.rs:46-89) is what the generic kernel reads: at the
        // default mel counts of very long windows it no longer fits anything (n_fft 131072 at 48 kHz: 65537 x ~22000 floats)
        if ((double)(n_fft / 2 + 1) * (double)n_mel * sizeof(float) > (double)((size_t)1 << 30))
            return fail(TH_ERR_UNSUPPORTED, "mel filterbank of %zu bins x %zu mels exceeds 1 GiB", n_fft / 2 + 1, n_mel);
        g.n_mel = (uint32_t)n_mel;
        g.height = (uint32_t)n_mel;
        p->h_mel_fb = calc_mel_fb(sr, n_fft, n_mel, 0.f, -1.f, true);
        const float *fb = p->h_mel_fb.data();
        const MelRangeHost rg = build_mel_ranges(fb, g.n_freq, g.n_mel);
        if (th::stft_wave_supported(g)) {   // (no wave / block kernel for this geometry: the generic kernel reads none of these)
            // MFMA mel path tables (kernels_mel.hip; any mel count since round 4 — the Mel default of long windows, e.g. 5571 mels
            // at n_fft 32768 / 48 kHz, used to fall back to the generic kernel: 12 ms where the linear plan takes 2)
            const MelMfmaHost mt = build_mel_mfma(fb, rg, g.n_freq, g.n_mel);
            p->mel_zero_block = mt.zero_block;
            p->mel_kblocks = mt.kblocks;
            p->mel_ntiles = mt.ntiles;
            p->mel_slices = mt.n_slices;
            // short rows under narrow filters (n_fft 512 at the default mel counts): the per-mel table of mel_rows_kernel
            // (only n_fft 512 plans on the wave kernel ever read it — ADVICE r3: n_fft 128 / 256 used to pay the upload too)
            if (g.log2_nc == 8) {
                const MelRowsHost mr = build_mel_rows(fb, rg, g.n_freq, g.n_mel);
                if (mr.ok) {
                    p->mel_rows_groups = mr.n_groups;
                    TH_CHECK(p->d_mel_rows.fill(mr.words));
                }
            }
            TH_CHECK(p->d_mel_bt.fill(mt.bt));
            TH_CHECK(p->d_mel_band.fill(mt.band));
            TH_CHECK(p->d_mel_slice.fill(mt.slice));
        }
        if (th::stft_wave_supported(g) && n_mel <= 512) {  // (the fused forms: lane = mel in at most 8 groups of 64)
            // fused mel epilogue of the wave kernel: piece / gather tables, when the filterbank has the expected structure
            const th::MelFuseHost mf = th::build_mel_fuse(fb, g.n_freq, (uint32_t)n_mel, th::stft_wave_mel_max_pieces(g));
            auto keep_band = [&](const th::MelBandHost &mb) {
                p->mel_bsum_words = (uint32_t)mb.words.size();
                std::copy(mb.words.begin(), mb.words.begin() + 16, p->mel_bsum_hdr);
                p->mel_bsum_groups = mb.n_groups;
                return p->d_mel_bsum.fill(mb.words);
            };
            if (g.log2_nc == 11) {
                // n_fft 4096 (two kernels): the same banded table for mel_band_rows_kernel, where it fits LDS beside four rows
                // (the paired layout as in the wave kernels; with dword reads the bank-spread table had measured 3 % SLOWER here, 2.08 ->
                // 2.15 ms at the 96 kHz default, profiles/r04_ab_mel_bank_spread.txt — the paired one is 1 % faster than the plain table)
                const th::MelBandHost mb = th::build_mel_band(fb, g.n_freq, (uint32_t)n_mel, 1u << 16, false, TH_MEL_ROWS_PAIRED != 0);
                if (mb.ok && th::mel_band_rows_fits(g.n_freq, (uint32_t)mb.words.size())) TH_CHECK(keep_band(mb));
            }
            if (g.log2_nc == 9 || g.log2_nc == 10) {
                // (the wave kernels of n_fft 1024 / 2048 read the table's paired layout, mel_banded<true>)
                const th::MelBandHost mb = th::build_mel_band(fb, g.n_freq, (uint32_t)n_mel, 1u << 16, TH_MEL_BAND_SPREAD != 0, TH_MEL_BAND_PAIRED != 0);
                // Measured against the pieces / gather form (same box, alternating; taps = the sum over the groups of their
                // widest filter): n_fft 2048 — 56 / 60 / 64 taps (256 mels, the 44.1 / 48 kHz defaults) 6 / 8 / 10 % faster; 72 taps
                // (128 mels) 4 % faster in the register-reuse kernel (hop a multiple of 128: config 4), 6 % slower in the full-reload
                // one (hop 480); 96 (200 mels) 5 % slower, 124 (64 mels) 40 % slower; n_fft 1024 — 32 / 36 / 44 taps (22.05 kHz
                // default, 128 mels, 16 kHz default) 22 / 13 / 12 % faster, 76 (48 kHz, 80 mels) 1 % faster
                // (round 4: the table's first bins are spread over the LDS banks, which may add 4 taps to a group; the limits
                // were measured on, and still apply to, the tap count before that)
                const uint32_t taps = mb.taps_unshifted;
                const uint32_t max_taps = g.log2_nc == 9 ? TH_MEL_BAND_TAPS_1024 : (g.hop % 128 == 0 ? TH_MEL_BAND_TAPS_2048 + 8u : TH_MEL_BAND_TAPS_2048);
                if (mb.ok && taps <= max_taps) {
                    p->mel_bsum_reach = mb.reach;
                    TH_CHECK(keep_band(mb));
                }
            }
            if (mf.ok) {
                p->mel_fuse_words = (uint32_t)mf.words.size();
                p->mel_fuse_slots = mf.n_slots;
                p->mel_fuse_groups = mf.n_groups;
                TH_CHECK(p->d_mel_fuse.fill(mf.words));
            }
        }
        // (n_fft 1024 / 2048: only where no LDS table form exists — more than 512 mels)
        const bool small_mom = ((g.log2_nc == 9 || g.log2_nc == 10) && p->d_mel_bsum == nullptr && p->d_mel_fuse == nullptr) || (g.log2_nc == 8 && p->d_mel_rows == nullptr);
        if ((g.log2_nc == 11 || g.log2_nc == 12 || g.log2_nc == 13 || small_mom) && th::stft_wave_supported(g)) {
            // n_fft 4096 (the wave kernel) and 8192 / 16384 (the workgroup-per-frame kernel): the moment form (lane = segment of the
            // triangle points; mel_fuse.h) for the fused epilogue, any mel count
            std::vector<float> lin, mfp;
            mel_fb_points(sr, n_fft, n_mel, 0.f, -1.f, lin, mfp);
            const th::MelMomHost mm = th::build_mel_moments(fb, lin.data(), mfp.data(), g.n_freq, (uint32_t)n_mel,
                                                            g.log2_nc == 8 ? th::stft_wave_multi_amp_pitch() : g.log2_nc <= 11 ? 2u * (g.nc + g.nc / 16u) : th::stft_block_mel_max_index(g), g.log2_nc <= 11 && TH_MEL_BAND_SPREAD != 0);
            // (the workgroup-per-frame kernels walk a batch of groups in lockstep: a lane reads up to the table's widest group's
            // taps behind its first bin — inside the exchange buffer)
            const bool reach_ok = g.log2_nc <= 11 || (uint64_t)g.n_freq + mm.max_taps <= th::stft_block_mel_max_index(g);
            // (the workgroup-per-frame kernels: the same numbers at fixed addresses, build_mel_mom_lanes)
            const std::vector<uint32_t> lanes = g.log2_nc <= 11 ? std::vector<uint32_t>() : th::build_mel_mom_lanes(mm);
            const std::vector<uint32_t> &tab = g.log2_nc <= 11 ? mm.words : lanes;
            if (mm.ok && reach_ok && !tab.empty()) {
                p->mel_mom_groups = mm.n_groups;
                p->mel_mom_taps = mm.taps;
                p->mel_mom_max_dev = mm.max_dev;
                p->mel_mom_max_amp = mm.max_amp;
                TH_CHECK(p->d_mel_mom.fill(tab));
            }
        }
        TH_CHECK(p->d_mel_fb.fill(p->h_mel_fb));
        TH_CHECK(p->d_mel_lo.fill(rg.lo));
        TH_CHECK(p->d_mel_hi.fill(rg.hi));
    }
    resolve_route(*p);
    *out = owner.release();
    return TH_OK;
    TH_CATCH
}

TH_API int th_plan_destroy(th_plan *p) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("destroying a plan"));
    if (!p) return TH_OK;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    delete p;
    return TH_OK;
    TH_CATCH
}

TH_API int th_plan_dims(const th_plan *p, size_t *n_freq, size_t *height) {
    TH_TRY
    TH_REQUIRE(p, "plan is NULL");
    if (n_freq) *n_freq = p->g.n_freq;
    if (height) *height = p->g.height;
    return TH_OK;
    TH_CATCH
}

TH_API int th_plan_set_kernel(th_plan *p, int which) {
    TH_TRY
    TH_REQUIRE(p, "plan is NULL");
    // bits 0-7: the kernel selector (th::StftSelector; include/thesia_amd_testing.h describes them), bits 8-15 (tuning): waves per
    // workgroup, bits 16-23 (tuning): frames per chunk of the wave kernel
    const int k = which & 0xff, wv = (which >> 8) & 0xff;
    TH_REQUIRE(k >= 0 && k <= 15, "kernel selector must be 0 .. 15");
    TH_REQUIRE(wv == 0 || wv == 4 || wv == 6 || wv == 7 || wv == 8 || wv == 10 || wv == 12 || wv == 14 || wv == 16,
               "waves per workgroup must be 4, 6, 7, 8, 10, 12, 14 or 16");
    // the multi-frame plans (n_fft 512; n_fft 1024 under selector 6) are instantiated for 8, 12 and 16 waves only
    const bool multi = p->g.n_mel == 0 ? (p->g.log2_nc == 8 || (p->g.log2_nc == 9 && k == SEL_MULTI_1024)) : p->g.log2_nc == 8;
    if (multi && !(wv == 0 || wv == 8 || wv == 12 || wv == 16))
        return fail(TH_ERR_UNSUPPORTED, "the multi-frame wave kernel of n_fft %u runs with 8, 12 or 16 waves per workgroup, not %d",
                    p->g.n_fft, wv);
    // Variants that were measured and dropped are not in the product library (kernels.h, TH_AB_VARIANTS): refuse them by name
    // instead of a launch failure later
    if (!TH_AB_VARIANTS) {
        const char *what = nullptr;
        if (k == SEL_PACKED) what = "selector 9 (packed-f32 pipeline)";
        else if (k == SEL_SWEEP) what = "selector 11 (sweep chunk schedule)";
        else if (k == SEL_BLOCK && p->g.log2_nc >= 14) what = "selector 14 at n_fft 32768 / 65536 (workgroup-per-frame Stockham kernels)";
        else if (k == SEL_SUBWAVE && p->g.log2_nc == 12) what = "selector 15 at n_fft 8192 (stft_subwave_kernel with four waves)";
        else if (!multi && p->g.log2_nc >= 9 && p->g.log2_nc <= 11 && wv != 0 && !(p->g.log2_nc == 11 ? (wv == 7 || wv == 8) : wv == 12))
            what = "a waves-per-workgroup shape other than the size's own (n_fft 1024 / 2048: 12; n_fft 4096: 8 or 7)";
        if (what) return fail(TH_ERR_UNSUPPORTED, "%s is an A/B variant: build with -DTH_AB_VARIANTS=1 (scripts/build_variant.sh)", what);
    }
    p->kernel_choice = k;
    p->wave_waves = wv;
    p->wave_chunk = (which >> 16) & 0xff;  // tuning: frames per chunk of the wave kernel (0 = default)
    resolve_route(*p);
    return TH_OK;
    TH_CATCH
}

TH_API int th_build_ab_variants(void) { return TH_AB_VARIANTS ? 1 : 0; }

TH_API int th_plan_mel_moments_info(const th_plan *p, uint32_t *n_groups, uint32_t *taps, double *max_dev, double *max_amp) {
    TH_TRY
    TH_REQUIRE(p, "plan is NULL");
    const bool have = p->d_mel_mom != nullptr;
    if (n_groups) *n_groups = have ? p->mel_mom_groups : 0u;
    if (taps) *taps = have ? p->mel_mom_taps : 0u;
    if (max_dev) *max_dev = have ? p->mel_mom_max_dev : 0.0;
    if (max_amp) *max_amp = have ? p->mel_mom_max_amp : 0.0;
    return TH_OK;
    TH_CATCH
}

TH_API const char *th_plan_kernel_name(const th_plan *p) { return p ? p->route.name : ""; }

TH_API size_t th_pitch_f32(size_t n) { return (n + 31) / 32 * 32; }
TH_API size_t th_pitch_u16(size_t n) { return (n + 63) / 64 * 64; }

// ------------------------------------------------------------------------------------------ calc_spec
// d_range != NULL: also leave the global dB range [min_dB, max_dB] of these channels (core/mod.rs:169-180) in d_range —
// folded into the wave kernel's follow-up launch when the batch is one channel, else one more small launch
// Selector 11 (the in-order "sweep" chunk schedule, measurement apparatus): a wave whose ring slot never arrives gives its chunk
// up and raises word 1 of the queue block.  Read it back (4 bytes; blocks until the stream is idle) and fail the call that
// finds it: rows of that launch were left unwritten.
static int sweep_check(th_plan *p) {
    uint32_t flag = 0;
    TH_HIP(hipMemcpy(&flag, p->d_queue_head + 1, sizeof flag, hipMemcpyDeviceToHost));
    if (!flag) return TH_OK;
    TH_HIP(hipMemset(p->d_queue_head + 1, 0, sizeof flag));
    return fail(TH_ERR_INTERNAL, "sweep schedule (kernel selector 11): a wave gave up waiting for its chunk block; rows of the last launch are unwritten");
}

// What the wave kernel of this plan writes, and the mel table its epilogue reads: the route's choices as launch arguments
static th::WaveOut wave_out(const th_plan &p, const StftGeom &g, bool sweep) {
    const StftRoute &r = p.route;
    th::WaveOut wo;
    wo.mode = r.out_mode();
    wo.multi = r.main == StftRoute::Main::WaveMulti ? 1 : 0;
    wo.packed = r.packed ? 1 : 0;
    wo.sweep = sweep ? 1 : 0;
    wo.long_plan = r.long_plan;
    wo.subwave_twc = p.d_twc;
    if (r.mel_fused != StftRoute::MelFused::None) wo.n_mel = g.n_mel;
    switch (r.mel_fused) {
        case StftRoute::MelFused::None: break;
        case StftRoute::MelFused::Moment:
        case StftRoute::MelFused::MomentLanes:  // moment form: the table stays in global memory (scalar + 16-byte lane loads)
            wo.mel_moment = r.mel_fused == StftRoute::MelFused::Moment && g.log2_nc < 11 ? 1u : 0u;  // (n_fft 4096 and up: their only form)
            wo.mel_tab = p.d_mel_mom;
            wo.mel_groups = p.mel_mom_groups;
            break;
        case StftRoute::MelFused::Rows:  // (the per-mel table of the banded sums, kernels.h)
            wo.mel_tab = p.d_mel_rows;
            wo.mel_groups = p.mel_rows_groups;
            wo.mel_words = p.mel_rows_groups * (uint32_t)(th::MEL_ROWS_W + 1) * 64u;
            break;
        case StftRoute::MelFused::Banded:
        case StftRoute::MelFused::BandedPairs:  // banded sums (mel_slots = 0 tells the kernel)
            wo.mel_tab = p.d_mel_bsum;
            wo.mel_words = p.mel_bsum_words;
            wo.mel_groups = p.mel_bsum_groups;
            for (uint32_t gq = 0; gq < 8; gq++) {
                wo.band_off[gq] = p.mel_bsum_hdr[2 * gq];
                wo.band_n[gq] = p.mel_bsum_hdr[2 * gq + 1];
            }
            wo.mel_pair = r.mel_fused == StftRoute::MelFused::BandedPairs ? 1u : 0u;
            break;
        case StftRoute::MelFused::Pieces:
            wo.mel_tab = p.d_mel_fuse;
            wo.mel_words = p.mel_fuse_words;
            wo.mel_slots = p.mel_fuse_slots;
            wo.mel_groups = p.mel_fuse_groups;
            break;
    }
    return wo;
}

static int calc_spec_batch_impl(th_plan *p, const th_chan_desc *chans, size_t n_chan, float *d_minmax, float dB_range,
                                float *d_range) {
    TH_TRY
    TH_REQUIRE(p, "plan is NULL");
    TH_REQUIRE(d_range == nullptr || d_minmax != nullptr, "d_range needs d_minmax");
    if (n_chan == 0) return TH_OK;
    TH_REQUIRE(chans, "chans is NULL");
    TH_REQUIRE(n_chan < (1u << 24), "too many channels");
    TH_REQUIRE_ALIGNED(d_minmax, 4, "d_minmax must be 4-byte aligned");
    TH_REQUIRE_ALIGNED(d_range, 4, "d_range must be 4-byte aligned");
    for (size_t i = 0; i < n_chan; i++) {
        TH_REQUIRE_ALIGNED(chans[i].wav, 4, "channel %zu: wav must be 4-byte aligned", i);
        TH_REQUIRE_ALIGNED(chans[i].spec, 4, "channel %zu: spec must be 4-byte aligned", i);
    }
    th_ctx *c = p->ctx;
    const StftRoute &r = p->route;
    const bool wave = r.wave(), mel_mfma = r.mel_second != StftRoute::MelSecond::None;
    if (r.no_wave_kernel) return fail(TH_ERR_UNSUPPORTED, "the wave kernels cover n_fft 512 .. 32768");
    // everything the batch decides (stft_plan.h): launch geometry, jobs and chunk / tile tables, edge and mel jobs
    StftLaunch l = plan_stft_launch(p->g, r, c->n_cu, p->wave_chunk, chans, n_chan);
    if (l.err != TH_OK) return fail(l.err, "%s", l.err_text.c_str());
    const StftGeom &g = l.g, &ge = l.ge;  // main launch; edge launch (generic kernel)
    const bool phased = r.phase_mode != 0, sweep = l.sweep, all_in_wave = l.all_in_wave;
    std::vector<ChanJob> &jobs = l.jobs, &edge = l.edge;
    const uint64_t tiles = l.tiles, edge_tiles = l.edge_tiles, mel_tiles = l.mel_tiles;
    // (selector 11: an earlier launch of this plan that dropped a chunk is found here when the stream has gone idle — no stall
    // otherwise — and in th_calc_spec_host behind its synchronisation)
    if (sweep && hipStreamQuery(c->stream) == hipSuccess) {
        const int src = sweep_check(p);
        if (src != TH_OK) return src;
    }
    // mel on the matrix cores: the wave kernel stores |X| rows (pitch amp_pitch) into plan-owned
    // scratch, mel_mfma_kernel contracts them with the filterbank into the caller's spec
    const uint32_t amp_pitch = (uint32_t)th_pitch_f32((size_t)p->mel_kblocks * 16);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TH_HIP(hipSetDevice(c->device));
    int rc = TH_OK;
    bool range_done = false;
    if (mel_mfma && l.amp_rows) {
        const size_t need = (size_t)l.amp_rows * amp_pitch * sizeof(float);
        if (need > p->amp_buf.cap || p->amp_zeroed < need) {
            TH_CHECK(refuse_while_capturing("sizing the amplitude scratch"));
            TH_HIP(hipStreamSynchronize(c->stream));
            rc = p->amp_buf.ensure(need);
            if (rc != TH_OK) return rc;
            // the K tail (columns >= n_freq) must read as zero: the wave kernel never writes it
            TH_HIP(hipMemsetAsync(p->amp_buf.dptr, 0, p->amp_buf.cap, c->stream));
            p->amp_zeroed = p->amp_buf.cap;
        }
        float *amp = static_cast<float *>(p->amp_buf.dptr);
        size_t mj = 0;
        for (ChanJob &j : jobs) {  // interior jobs are in channel order, one per channel with interior frames
            j.spec = amp + l.amp_row0[j.mm_index] * amp_pitch;
            j.spec_pitch = amp_pitch;
            l.mel_jobs[mj++].amp = j.spec;
        }
        rc = p->mel_jobs.upload(c->stream, l.mel_jobs.data(), l.mel_jobs.size() * sizeof(MelJob));
        if (rc == TH_OK) rc = p->mel_tile_start.upload(c->stream, l.mel_start.data(), l.mel_start.size() * sizeof(uint32_t));
        if (rc != TH_OK) return rc;
    }
    rc = p->jobs.upload(c->stream, jobs.data(), jobs.size() * sizeof(ChanJob));
    if (rc == TH_OK) {  // the wave kernels look a chunk up directly; the generic kernel finds its job from the jobs' first tiles
        const std::vector<uint32_t> &tab = wave ? l.chunk_tab : l.tile_start;
        rc = p->tile_start.upload(c->stream, tab.data(), tab.size() * sizeof(uint32_t));
    }
    if (rc == TH_OK && !edge.empty()) {
        rc = p->edge_jobs.upload(c->stream, edge.data(), edge.size() * sizeof(ChanJob));
        if (rc == TH_OK) rc = p->edge_tile_start.upload(c->stream, l.edge_start.data(), l.edge_start.size() * sizeof(uint32_t));
    }
    if (rc != TH_OK) return rc;
    {   // n_fft >= 32768: the generic kernel's frame buffers live in global scratch (all frames of a plan without a fast
        // kernel, or the boundary frames of the n_fft 32768 block plan)
        const size_t need = !wave ? (r.main == StftRoute::Main::Bluestein ? th::stft_bluestein_scratch_bytes(g, (uint32_t)tiles, c->n_cu) : th::stft_generic_scratch_bytes(g, (uint32_t)tiles, c->n_cu))
                                  : (edge.empty() ? 0 : th::stft_generic_scratch_bytes(ge, (uint32_t)edge_tiles, c->n_cu));
        if (need) {
            if (need > p->gen_scratch.cap) {
                TH_CHECK(refuse_while_capturing("sizing the frame scratch"));
                TH_HIP(hipStreamSynchronize(c->stream));  // (a launch may still use the old buffer)
            }
            rc = p->gen_scratch.ensure(need);
            if (rc != TH_OK) return rc;
        }
    }
    // (min, max) slots: the wave launch's follow-up fills them when every frame was in it (StftLaunch::all_in_wave);
    // otherwise initialise here and let every kernel add with atomics
    if (!all_in_wave) TH_HIP(launch_minmax_init(d_minmax, (uint32_t)n_chan, c->stream));
    // optional timing of the dominant kernel alone (th_plan_time_kernel): two events on the launch stream
    const bool timed = p->time_kernel && !p->ev_k0.empty();
    const size_t slot = (size_t)(p->timed_launches % th_plan::TIMER_SLOTS);
    if (timed) TH_HIP(hipEventRecord(p->ev_k0[slot], c->stream));
    if (wave) {
        const th::WaveOut wo = wave_out(*p, g, sweep);
        // min / max: the wave kernel stores one pair per chunk and its last workgroup folds them into the channel slots
        float *chunk_mm = nullptr;
        if (d_minmax != nullptr && wo.mode != 1 && tiles) {
            rc = p->chunk_mm.ensure((size_t)tiles * 2 * sizeof(float));
            if (rc != TH_OK) return rc;
            chunk_mm = static_cast<float *>(p->chunk_mm.dptr);
        }
        uint32_t n_post = 0;
        if (chunk_mm) {  // per-channel tile ranges for wave_post_kernel
            rc = p->post_jobs.upload(c->stream, l.post.data(), l.post.size() * sizeof(th::WavePostJob));
            if (rc != TH_OK) return rc;
            n_post = (uint32_t)l.post.size();
        }
        // The chunk queue head is rewound by wave_post_kernel right behind the wave kernel.  Should anything between the
        // two launches fail (the event record, the post launch itself), queue_dirty stays set and the next launch zeroes
        // the head itself — a stale head would make it skip chunks and leave spectrogram rows unwritten without an error.
        if (p->queue_dirty) TH_HIP(hipMemsetAsync(p->d_queue_head, 0, sizeof(uint32_t), c->stream));
        p->queue_dirty = true;
        TH_HIP(launch_stft_wave(g, (const ChanJob *)p->jobs.dptr, (const uint32_t *)p->tile_start.dptr,
                                (uint32_t)jobs.size(), (uint32_t)tiles, phased ? p->d_wtab_phased : p->d_wtab, p->d_tw, chunk_mm, p->d_queue_head,
                                c->n_cu, r.waves, wo, c->stream));
        if (timed) TH_HIP(hipEventRecord(p->ev_k1[slot], c->stream));
        // fold the per-chunk (min, max) pairs into the channel slots and rewind the chunk queue
        range_done = d_range != nullptr && all_in_wave && n_post == 1 && n_chan == 1;
        TH_HIP(launch_wave_post((const th::WavePostJob *)p->post_jobs.dptr, n_post, chunk_mm, d_minmax, all_in_wave,
                                p->d_queue_head, dB_range, range_done ? d_range : nullptr, c->stream));
        p->queue_dirty = false;
        if (r.mel_second == StftRoute::MelSecond::Rows)
            TH_HIP(launch_mel_rows((const MelJob *)p->mel_jobs.dptr, (const uint32_t *)p->mel_tile_start.dptr,
                                   (uint32_t)l.mel_jobs.size(), (uint32_t)mel_tiles, amp_pitch, p->d_mel_rows, p->mel_rows_groups,
                                   g.n_mel, d_minmax, c->n_cu, c->stream));
        else if (r.mel_second == StftRoute::MelSecond::BandRows)
            TH_HIP(launch_mel_band_rows((const MelJob *)p->mel_jobs.dptr, (const uint32_t *)p->mel_tile_start.dptr,
                                        (uint32_t)l.mel_jobs.size(), (uint32_t)mel_tiles, amp_pitch, g.n_freq, p->d_mel_bsum,
                                        p->mel_bsum_words, p->mel_bsum_groups, p->mel_bsum_hdr, g.n_mel, d_minmax, c->n_cu,
                                        c->stream));
        else if (r.mel_second == StftRoute::MelSecond::Mfma)
            TH_HIP(launch_mel_mfma((const MelJob *)p->mel_jobs.dptr, (const uint32_t *)p->mel_tile_start.dptr,
                                   (uint32_t)l.mel_jobs.size(), (uint32_t)mel_tiles, amp_pitch, p->d_mel_bt, p->d_mel_band,
                                   p->d_mel_slice, p->mel_slices, p->mel_zero_block, g.n_mel, d_minmax, c->stream));
        if (!edge.empty())  // boundary frames the wave kernel did not take: generic kernel (reflect padding; mel included)
            TH_HIP(launch_stft_generic(ge, (const ChanJob *)p->edge_jobs.dptr, (const uint32_t *)p->edge_tile_start.dptr,
                                       (uint32_t)edge.size(), (uint32_t)edge_tiles, p->d_window, p->d_tw, p->d_mel_fb,
                                       p->d_mel_lo, p->d_mel_hi, d_minmax, c->stream, p->gen_scratch.dptr, c->n_cu));
    } else {
        if (r.main == StftRoute::Main::Bluestein)
            TH_HIP(launch_stft_bluestein(g, (const ChanJob *)p->jobs.dptr, (const uint32_t *)p->tile_start.dptr, (uint32_t)jobs.size(),
                                         (uint32_t)tiles, p->d_window, p->d_bs_chirp, p->d_bs_bhat, p->d_bs_twm, p->d_bs_tws, p->d_mel_fb,
                                         p->d_mel_lo, p->d_mel_hi, d_minmax, c->stream, p->gen_scratch.dptr, c->n_cu));
        else
        TH_HIP(launch_stft_generic(g, (const ChanJob *)p->jobs.dptr, (const uint32_t *)p->tile_start.dptr,
                                   (uint32_t)jobs.size(), (uint32_t)tiles, p->d_window, p->d_tw, p->d_mel_fb,
                                   p->d_mel_lo, p->d_mel_hi, d_minmax, c->stream, p->gen_scratch.dptr, c->n_cu));
        if (timed) TH_HIP(hipEventRecord(p->ev_k1[slot], c->stream));
    }
    if (timed) p->timed_launches++;
    if (d_range != nullptr && !range_done)
        TH_HIP(launch_minmax_reduce(d_minmax, (uint32_t)n_chan, nullptr, dB_range, d_range, c->stream));
    return TH_OK;
    TH_CATCH
}

TH_API int th_calc_spec_batch_dev(th_plan *p, const th_chan_desc *chans, size_t n_chan, float *d_minmax) {
    return calc_spec_batch_impl(p, chans, n_chan, d_minmax, 0.0f, nullptr);
}

TH_API int th_calc_spec_batch_ranged_dev(th_plan *p, const th_chan_desc *chans, size_t n_chan, float *d_minmax, float dB_range,
                                         float *d_range) {
    if (!d_range) return fail(TH_ERR_INVALID_ARG, "d_range is NULL");
    return calc_spec_batch_impl(p, chans, n_chan, d_minmax, dB_range, d_range);
}

TH_API int th_minmax_reduce_dev(th_ctx *c, const float *d_minmax, size_t n_chan, float *d_out) {
    TH_TRY
    TH_REQUIRE(c && d_out, "NULL argument");
    TH_REQUIRE(n_chan == 0 || d_minmax, "d_minmax is NULL");
    TH_REQUIRE(n_chan < (1ull << 31), "too many channels");
    TH_REQUIRE_ALIGNED(d_minmax, 4, "d_minmax must be 4-byte aligned");
    TH_REQUIRE_ALIGNED(d_out, 4, "d_out must be 4-byte aligned");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TH_HIP(hipSetDevice(c->device));
    TH_HIP(launch_minmax_reduce(d_minmax, (uint32_t)n_chan, d_out, 0.0f, nullptr, c->stream));
    return TH_OK;
    TH_CATCH
}

// single-GPU form of th_minmax_reduce_dev + th_global_db_range_dev: one launch instead of two
TH_API int th_minmax_reduce_range_dev(th_ctx *c, const float *d_minmax, size_t n_chan, float dB_range, float *d_min_negmax,
                                      float *d_range) {
    TH_TRY
    TH_REQUIRE(c && d_range, "NULL argument");
    TH_REQUIRE(n_chan == 0 || d_minmax, "d_minmax is NULL");
    TH_REQUIRE(n_chan < (1ull << 31), "too many channels");
    TH_REQUIRE_ALIGNED(d_minmax, 4, "d_minmax must be 4-byte aligned");
    TH_REQUIRE_ALIGNED(d_min_negmax, 4, "d_min_negmax must be 4-byte aligned");
    TH_REQUIRE_ALIGNED(d_range, 4, "d_range must be 4-byte aligned");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TH_HIP(hipSetDevice(c->device));
    TH_HIP(launch_minmax_reduce(d_minmax, (uint32_t)n_chan, d_min_negmax, dB_range, d_range, c->stream));
    return TH_OK;
    TH_CATCH
}

TH_API int th_plan_time_kernel(th_plan *p, int enable) {
    TH_TRY
    TH_REQUIRE(p, "plan is NULL");
    std::lock_guard<std::recursive_mutex> lk(p->ctx->mu);
    TH_HIP(hipSetDevice(p->ctx->device));
    if (enable && p->ev_k0.empty()) {
        for (size_t i = 0; i < th_plan::TIMER_SLOTS; i++) {
            hipEvent_t a = nullptr, b = nullptr;
            TH_HIP(hipEventCreate(&a));
            p->ev_k0.push_back(a);
            TH_HIP(hipEventCreate(&b));
            p->ev_k1.push_back(b);
        }
    }
    p->time_kernel = enable != 0;
    p->timed_launches = 0;
    return TH_OK;
    TH_CATCH
}

TH_API int th_plan_kernel_ms_history(th_plan *p, float *out_ms, size_t capacity, size_t *n_out) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("reading kernel times"));
    TH_REQUIRE(p && n_out && (out_ms || capacity == 0), "NULL argument");
    std::lock_guard<std::recursive_mutex> lk(p->ctx->mu);
    const size_t have = (size_t)std::min<uint64_t>(p->timed_launches, th_plan::TIMER_SLOTS);
    const size_t n = std::min(have, capacity);
    *n_out = n;
    for (size_t i = 0; i < n; i++) {  // oldest kept launch first
        const size_t slot = (size_t)((p->timed_launches - n + i) % th_plan::TIMER_SLOTS);
        TH_HIP(hipEventSynchronize(p->ev_k1[slot]));
        TH_HIP(hipEventElapsedTime(&out_ms[i], p->ev_k0[slot], p->ev_k1[slot]));
    }
    // (selector 11, A/B builds: a pipelined caller never lets the stream go idle between launches, so the launch path's check for a
    // dropped chunk never runs there — this call has just waited for the launches it reports, check here as well: ADVICE r5)
    if (n > 0 && p->route.sweep) {
        TH_HIP(hipStreamSynchronize(p->ctx->stream));
        const int src = sweep_check(p);
        if (src != TH_OK) return src;
    }
    return TH_OK;
    TH_CATCH
}

TH_API int th_plan_last_kernel_ms(th_plan *p, float *ms) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("reading kernel times"));
    TH_REQUIRE(p && ms, "NULL argument");
    size_t n = 0;
    const int rc = th_plan_kernel_ms_history(p, ms, 1, &n);
    if (rc != TH_OK) return rc;
    TH_REQUIRE(n == 1, "no timed launch: call th_plan_time_kernel(plan, 1) and th_calc_spec_batch_dev first");
    return TH_OK;
    TH_CATCH
}

TH_API int th_calc_spec_host(th_plan *p, const float *wav, size_t n_samples, float *out_spec, size_t cap,
                             size_t *n_frames, float *out_min, float *out_max) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("th_calc_spec_host (host buffers)"));
    TH_REQUIRE(p && wav && out_spec && n_frames, "NULL argument");
    TH_REQUIRE(n_samples >= 1, "empty input");
    const StftGeom &g = p->g;
    const size_t T = stft_n_frames(n_samples, g.win, g.hop);
    *n_frames = T;
    if ((size_t)T * g.height > cap) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu floats", (size_t)T * g.height);
    th_ctx *c = p->ctx;
    TH_HIP(hipSetDevice(c->device));
    DeviceBuf<float> d_wav, d_spec, d_mm;
    int rc = TH_OK;
    auto hipok = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == TH_OK) rc = fail(e == hipErrorOutOfMemory ? TH_ERR_OOM : TH_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
        return e == hipSuccess;
    };
    if (hipok(d_wav.alloc(n_samples * sizeof(float)), "hipMalloc wav") &&
        hipok(d_spec.alloc(std::max<size_t>(1, T * g.height) * sizeof(float)), "hipMalloc spec") &&
        hipok(d_mm.alloc(2 * sizeof(float)), "hipMalloc minmax") &&
        hipok(hipMemcpy(d_wav, wav, n_samples * sizeof(float), hipMemcpyHostToDevice), "upload")) {
        th_chan_desc d{d_wav, d_spec, n_samples, T, 0};
        rc = th_calc_spec_batch_dev(p, &d, 1, d_mm);
        if (rc == TH_OK) {
            float mm[2];
            if (hipok(hipStreamSynchronize(c->stream), "sync") && (!p->route.sweep || (rc = sweep_check(p)) == TH_OK) &&
                hipok(hipMemcpy(out_spec, d_spec, T * g.height * sizeof(float), hipMemcpyDeviceToHost), "download") &&
                hipok(hipMemcpy(mm, d_mm, sizeof mm, hipMemcpyDeviceToHost), "download minmax")) {
                if (out_min) *out_min = mm[0];
                if (out_max) *out_max = mm[1];
            }
        }
    }
    return rc;
    TH_CATCH
}

// ------------------------------------------------------------------------------------------ spec → img
// The batch entries below decide nothing here: batch_plan.h checks the descriptors and builds the job tables (plain data, tested on
// the CPU), th_ctx's KeyedTables keep the device copies of the last batch, and what is left is upload and launch.
static int plan_failed(const PlanStatus &p) { return fail(p.err, "%s", p.err_text.c_str()); }

// shared body: host range (d_range == nullptr) or device-resident range [min_dB, max_dB]
static int spec_to_img_impl(th_ctx *c, const th_img_desc *descs, size_t n, float min_dB, float max_dB, const float *d_range,
                            uint32_t colormap_len) {
    TH_TRY
    TH_REQUIRE(c, "ctx is NULL");
    if (n == 0) return TH_OK;
    TH_REQUIRE(descs, "descs is NULL");
    TH_REQUIRE_ALIGNED(d_range, 4, "d_range must be 4-byte aligned");
    const PlanStatus ok = check_img(descs, n, min_dB, max_dB, d_range);
    if (ok.err != TH_OK) return plan_failed(ok);
    const bool all_neg_inf = db_range_all_neg_inf(min_dB, max_dB, d_range);
    const size_t key_bytes = n * sizeof(th_img_desc);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TH_HIP(hipSetDevice(c->device));
    if (all_neg_inf || !c->img.hit(descs, key_bytes)) {
        const ImgPlan p = plan_img(descs, n);
        if (p.err != TH_OK) return plan_failed(p);
        if (all_neg_inf) {
            for (size_t i = 0; i < n; i++) {
                const size_t rows = descs[i].i_end - descs[i].i_start, pitch = p.jobs[i].img_pitch;
                if (rows && descs[i].n_frames)
                    TH_HIP(hipMemset2DAsync(descs[i].img, pitch * sizeof(uint16_t), 0, descs[i].n_frames * sizeof(uint16_t), rows,
                                            c->stream));
            }
            return TH_OK;
        }
        TH_CHECK(c->img.store(c->stream, descs, key_bytes, p.n_blocks,
                              {{p.jobs.data(), p.jobs.size() * sizeof(ImgJob)}, {p.block_job.data(), p.block_job.size() * sizeof(uint32_t)}}));
    }
    TH_HIP(launch_spec_to_img(c->img.at<ImgJob>(0), c->img.at<uint32_t>(1), (uint32_t)n, c->img.n_blocks, min_dB, max_dB, colormap_len,
                              d_range, c->stream));
    return TH_OK;
    TH_CATCH
}

TH_API int th_spec_to_img_batch_dev(th_ctx *c, const th_img_desc *descs, size_t n, float min_dB, float max_dB,
                                    uint32_t colormap_len) {
    return spec_to_img_impl(c, descs, n, min_dB, max_dB, nullptr, colormap_len);
}

// the dB range stays on the device (th_minmax_reduce_dev -> [all-reduce] -> th_global_db_range_dev): no host round
// trip between the STFT stage and the quantiser
TH_API int th_spec_to_img_batch_dev_ranged(th_ctx *c, const th_img_desc *descs, size_t n, const float *d_range,
                                           uint32_t colormap_len) {
    if (!d_range) return fail(TH_ERR_INVALID_ARG, "d_range is NULL");
    return spec_to_img_impl(c, descs, n, 0.0f, 0.0f, d_range, colormap_len);
}

// Quantise + level-0 raster of every tile in one pass (kernels_image.hip: spec_to_img_raster_kernel)
TH_API int th_spec_to_img_raster_batch_dev(th_ctx *c, const th_img_tiles_desc *descs, size_t n, float min_dB, float max_dB,
                                           const float *d_range, const uint8_t *d_colormap, uint32_t n_colors) {
    TH_TRY
    TH_REQUIRE(c, "ctx is NULL");
    if (n == 0) return TH_OK;
    TH_REQUIRE(descs && d_colormap && n_colors >= 1, "NULL descs / colormap or empty colormap");
    TH_REQUIRE(n_colors <= 65536, "colormaps of more than 65536 entries are not supported");
    TH_REQUIRE_ALIGNED(d_colormap, 4, "d_colormap must be 4-byte aligned");
    TH_REQUIRE_ALIGNED(d_range, 4, "d_range must be 4-byte aligned");
    std::vector<unsigned char> key;
    const PlanStatus ok = check_fused(descs, n, min_dB, max_dB, d_range, &key);
    if (ok.err != TH_OK) return plan_failed(ok);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TH_HIP(hipSetDevice(c->device));
    if (!c->fused.hit(key.data(), key.size())) {
        const FusedPlan p = plan_fused(descs, n);
        if (p.err != TH_OK) return plan_failed(p);
        TH_CHECK(c->fused.store(c->stream, key.data(), key.size(), p.n_blocks,
                                {{p.jobs.data(), p.jobs.size() * sizeof(FusedJob)},
                                 {p.block_job.data(), p.block_job.size() * sizeof(uint32_t)},
                                 {p.ptrs.data(), p.ptrs.size() * sizeof(uint8_t *)}}));
    }
    TH_HIP(launch_spec_to_img_raster(c->fused.at<FusedJob>(0), c->fused.at<uint32_t>(1), c->fused.n_blocks, c->fused.at<uint8_t *>(2), min_dB,
                                     max_dB, d_range, db_range_all_neg_inf(min_dB, max_dB, d_range) ? 1 : 0, d_colormap, n_colors, c->stream));
    return TH_OK;
    TH_CATCH
}

TH_API int th_global_db_range_dev(th_ctx *c, const float *d_min_negmax, float dB_range, float *d_range) {
    TH_TRY
    TH_REQUIRE(c && d_min_negmax && d_range, "NULL argument");
    TH_REQUIRE_ALIGNED(d_min_negmax, 4, "d_min_negmax must be 4-byte aligned");
    TH_REQUIRE_ALIGNED(d_range, 4, "d_range must be 4-byte aligned");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TH_HIP(hipSetDevice(c->device));
    TH_HIP(launch_db_range(d_min_negmax, dB_range, d_range, c->stream));
    return TH_OK;
    TH_CATCH
}

TH_API int th_spec_to_img_dev(th_ctx *c, const float *d_spec, size_t n_frames, size_t height, size_t i_start,
                              size_t i_end, float min_dB, float max_dB, uint32_t colormap_len, uint16_t *d_img) {
    th_img_desc d{d_spec, d_img, n_frames, height, i_start, i_end, 0, 0};
    return th_spec_to_img_batch_dev(c, &d, 1, min_dB, max_dB, colormap_len);
}

// ------------------------------------------------------------------------------------------ raster
TH_API int th_raster_tiles_dev(th_ctx *c, const th_raster_desc *descs, size_t n, const uint8_t *d_colormap,
                               uint32_t n_colors) {
    TH_TRY
    TH_REQUIRE(c, "ctx is NULL");
    if (n == 0) return TH_OK;
    TH_REQUIRE(descs && d_colormap && n_colors >= 1, "NULL descs/colormap or empty colormap");
    TH_REQUIRE(n_colors <= 65536, "colormaps of more than 65536 entries are not supported");
    TH_REQUIRE_ALIGNED(d_colormap, 4, "d_colormap must be 4-byte aligned");
    const size_t key_bytes = n * sizeof(th_raster_desc);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TH_HIP(hipSetDevice(c->device));
    if (!c->raster.hit(descs, key_bytes)) {
        const RasterPlan p = plan_raster(descs, n);
        if (p.err != TH_OK) return plan_failed(p);
        TH_CHECK(c->raster.store(c->stream, descs, key_bytes, p.n_blocks,
                                 {{p.jobs.data(), p.jobs.size() * sizeof(RasterJob)}, {p.block_job.data(), p.block_job.size() * sizeof(uint32_t)}}));
    }
    TH_HIP(launch_raster_level0(c->raster.at<RasterJob>(0), c->raster.at<uint32_t>(1), (uint32_t)n, c->raster.n_blocks, d_colormap, n_colors,
                                c->stream));
    return TH_OK;
    TH_CATCH
}

TH_API int th_encode_spectrogram_tile_dev(th_ctx *c, const uint16_t *d_img, size_t img_height, size_t img_width,
                                          size_t img_pitch, const uint8_t *colormap_rgba, size_t colormap_bytes, uint64_t revision,
                                          uint32_t level_x, uint32_t level_y, uint32_t tile_x, uint32_t tile_y,
                                          uint8_t *out, size_t cap, size_t *out_len) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("th_encode_spectrogram_tile_dev (it returns the tile to host memory)"));
    TH_REQUIRE(c && out && out_len, "NULL argument");
    TH_REQUIRE(colormap_rgba && colormap_bytes >= 4 && colormap_bytes % 4 == 0, "colormap must be a non-empty RGBA8 array");
    TH_REQUIRE(img_width < (1ull << 31) && img_height < (1ull << 31), "image too large");
    TH_REQUIRE(img_pitch == 0 || (img_pitch >= img_width && img_pitch < (1ull << 31)), "img_pitch < img_width");
    TH_REQUIRE_ALIGNED(d_img, 2, "d_img must be 2-byte aligned");
    const TileGeom g = spectrogram_tile_geometry(img_width, img_height, level_x, level_y, tile_x, tile_y);
    const size_t need = 40 + g.width * g.height * 4;
    *out_len = need;
    if (cap < need) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu bytes", need);
    put_spectrogram_tile_header(out, revision, g, level_x, level_y, tile_x, tile_y);
    if (g.width == 0 || g.height == 0) return TH_OK;
    TH_REQUIRE(d_img, "d_img is NULL");
    const uint32_t n_colors = (uint32_t)(colormap_bytes / 4);
    const uint32_t pitch = (uint32_t)(img_pitch ? img_pitch : img_width), dw = (uint32_t)g.width, dh = (uint32_t)g.height;
    const bool lod = level_x != 0 || level_y != 0;
    // LOD > 0: separable Lanczos3 of the crop box (render_tiles.rs:354-393), then the same raster
    const LodTilePlan lp = lod ? plan_lod_tile(img_width, img_height, g, level_x, level_y) : LodTilePlan{};
    if (lp.err != TH_OK) return plan_failed(lp);
    std::lock_guard<std::recursive_mutex> lk(c->mu);  // tile_out / colormap / lod scratch: whole request
    TH_HIP(hipSetDevice(c->device));
    TH_CHECK(c->colormap.upload(c->stream, colormap_rgba, colormap_bytes));
    TH_CHECK(c->tile_out.ensure(g.width * g.height * 4));
    // level (0, 0): integral crop box equal to the destination size: exact copy (pinned by render_tiles.rs:464-471)
    th_raster_desc d{d_img, (uint8_t *)c->tile_out.dptr, (uint32_t)img_width, (uint32_t)img_height,
                     (uint32_t)g.origin_x, (uint32_t)g.origin_y, dw, dh, pitch, 0};
    if (lod) {
        TH_CHECK(c->lod_tabs.upload(c->stream, lp.blob.data(), lp.blob.size()));
        TH_CHECK(c->lod_tmp.ensure(lp.scratch_bytes));
        auto axis_dev = [](unsigned char *base, size_t n_out, uint32_t taps) {
            LodAxis a;
            a.start = reinterpret_cast<const int32_t *>(base);
            a.count = reinterpret_cast<const int32_t *>(base + n_out * 4);
            a.wsum = reinterpret_cast<const double *>(base + n_out * 8);
            a.w = reinterpret_cast<const double *>(base + n_out * 16);
            a.n_out = (uint32_t)n_out;
            a.max_taps = taps;
            return a;
        };
        unsigned char *dtab = static_cast<unsigned char *>(c->lod_tabs.dptr);
        uint16_t *d_tmp = static_cast<uint16_t *>(c->lod_tmp.dptr);
        uint16_t *d_lod = d_tmp + lp.lod_at;
        TH_HIP(launch_lod_hpass(d_img, pitch, (uint32_t)lp.y_lo, (uint32_t)lp.n_rows, axis_dev(dtab, dw, lp.taps_x), d_tmp, dw, c->stream));
        TH_HIP(launch_lod_vpass(d_tmp, dw, (uint32_t)lp.y_lo, axis_dev(dtab + lp.y_at, dh, lp.taps_y), dw, d_lod, dw, c->stream));
        d = th_raster_desc{d_lod, (uint8_t *)c->tile_out.dptr, dw, dh, 0, 0, dw, dh, dw, 0};
    }
    TH_CHECK(th_raster_tiles_dev(c, &d, 1, (const uint8_t *)c->colormap.dptr, n_colors));
    TH_HIP(hipMemcpyAsync(out + 40, c->tile_out.dptr, g.width * g.height * 4, hipMemcpyDeviceToHost, c->stream));
    TH_HIP(hipStreamSynchronize(c->stream));
    return TH_OK;
    TH_CATCH
}

// ------------------------------------------------------------------------------------------ waveform
TH_API int th_waveform_tiles_dev(th_ctx *c, const th_wave_desc *descs, size_t n) {
    TH_TRY
    TH_REQUIRE(c, "ctx is NULL");
    if (n == 0) return TH_OK;
    TH_REQUIRE(descs, "descs is NULL");
    const WavePlan p = plan_wave_tiles(descs, n);
    if (p.err != TH_OK) return plan_failed(p);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TH_HIP(hipSetDevice(c->device));
    TH_CHECK(c->wave_jobs.upload(c->stream, p.jobs.data(), p.jobs.size() * sizeof(WaveJob)));
    TH_CHECK(c->wave_start.upload(c->stream, p.start.data(), p.start.size() * sizeof(uint32_t)));
    TH_HIP(launch_waveform((const WaveJob *)c->wave_jobs.dptr, (const uint32_t *)c->wave_start.dptr, (uint32_t)n, p.n_blocks, c->stream));
    return TH_OK;
    TH_CATCH
}

// ------------------------------------------------------------------------------------------ channel statistics
TH_API int th_channel_stats_dev(th_ctx *c, const th_stats_desc *descs, size_t n, float *out_sum_squares,
                                float *out_abs_max) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("th_channel_stats_dev (it returns to host memory)"));
    TH_REQUIRE(c, "ctx is NULL");
    if (n == 0) return TH_OK;
    TH_REQUIRE(descs && out_sum_squares && out_abs_max, "NULL argument");
    const StatsPlan p = plan_stats(descs, n);
    if (p.err != TH_OK) return plan_failed(p);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TH_HIP(hipSetDevice(c->device));
    TH_CHECK(c->pyr_sums.ensure(n * (sizeof(double) + sizeof(uint32_t))));
    double *d_sum = reinterpret_cast<double *>(c->pyr_sums.dptr);
    uint32_t *d_pk = reinterpret_cast<uint32_t *>(d_sum + n);
    TH_HIP(hipMemsetAsync(d_sum, 0, n * (sizeof(double) + sizeof(uint32_t)), c->stream));  // sum = 0, peak = +0.0 (:841,876)
    TH_CHECK(c->pyr_jobs.upload(c->stream, p.jobs.data(), p.jobs.size() * sizeof(StatsJob)));
    TH_HIP(launch_channel_stats((const StatsJob *)c->pyr_jobs.dptr, (uint32_t)n, p.max_samples, d_sum, d_pk, c->stream));
    std::vector<double> hs(n);
    std::vector<uint32_t> hp(n);
    TH_HIP(hipMemcpyAsync(hs.data(), d_sum, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TH_HIP(hipMemcpyAsync(hp.data(), d_pk, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    TH_HIP(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++) {
        out_sum_squares[i] = (float)hs[i];
        std::memcpy(&out_abs_max[i], &hp[i], sizeof(float));
    }
    return TH_OK;
    TH_CATCH
}

// ------------------------------------------------------------------------------------------ waveform pyramid
TH_API size_t th_waveform_pyramid_bins(uint64_t n_samples, uint32_t level) { return (size_t)pyramid_bins(n_samples, level); }
TH_API size_t th_waveform_pyramid_offset(uint64_t n_samples, uint32_t level) {
    return (size_t)pyramid_offset(n_samples, level < PYR_MAX_LEVELS ? level : PYR_MAX_LEVELS);
}

TH_API int th_waveform_pyramid_dev(th_ctx *c, const th_pyramid_desc *descs, size_t n) {
    TH_TRY
    TH_REQUIRE(c, "ctx is NULL");
    if (n == 0) return TH_OK;
    TH_REQUIRE(descs, "descs is NULL");
    PyrPlan p = plan_pyramid(descs, n);
    if (p.err != TH_OK) return plan_failed(p);
    if (!p.launch) return TH_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TH_HIP(hipSetDevice(c->device));
    TH_CHECK(c->pyr_sums.ensure(std::max<uint64_t>(p.sums_floats, 1) * sizeof(float)));
    bind_pyramid(p, reinterpret_cast<float *>(c->pyr_sums.dptr));
    TH_CHECK(c->pyr_jobs.upload(c->stream, p.jobs.data(), p.jobs.size() * sizeof(PyrJob)));
    const PyrJob *dj = (const PyrJob *)c->pyr_jobs.dptr;
    TH_HIP(launch_pyramid_base(dj, (uint32_t)n, p.max_samples, c->stream));
    for (uint32_t l = 13; l < p.max_levels; l++) TH_HIP(launch_pyramid_up(dj, (uint32_t)n, p.max_samples, l, (l - 13) & 1u, c->stream));
    return TH_OK;
    TH_CATCH
}

TH_API int th_encode_waveform_tile_dev(th_ctx *c, const float *d_wav, size_t n_samples, uint64_t revision,
                                       uint32_t level, uint32_t tile_index, uint8_t *out, size_t cap,
                                       size_t *out_len) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("th_encode_waveform_tile_dev (it returns the tile to host memory)"));
    TH_REQUIRE(c && out && out_len, "NULL argument");
    TH_REQUIRE_ALIGNED(d_wav, 4, "d_wav must be 4-byte aligned");
    size_t start, bins, spb;
    waveform_tile_geometry(n_samples, level, tile_index, &start, &bins, &spb);
    const size_t need = 24 + bins * 12;
    *out_len = need;
    if (cap < need) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu bytes", need);
    put_waveform_tile_header(out, revision, bins, spb, tile_index);
    if (bins == 0) return TH_OK;
    TH_REQUIRE(d_wav, "d_wav is NULL");
    std::lock_guard<std::recursive_mutex> lk(c->mu);  // tile_out scratch: whole request
    TH_HIP(hipSetDevice(c->device));
    TH_CHECK(c->tile_out.ensure(bins * 12));
    // levels whose bins are longer than the channel all give one bin; keep the shift in range
    const uint32_t level_eff = level < 39 ? level : 39;
    th_wave_desc d{d_wav, (float *)c->tile_out.dptr, n_samples, start, level_eff, (uint32_t)bins};
    TH_CHECK(th_waveform_tiles_dev(c, &d, 1));
    TH_HIP(hipMemcpyAsync(out + 24, c->tile_out.dptr, bins * 12, hipMemcpyDeviceToHost, c->stream));
    TH_HIP(hipStreamSynchronize(c->stream));
    return TH_OK;
    TH_CATCH
}

// ------------------------------------------------------------------------------------------ loudness (StatCalculator::calc)
TH_API int th_k_weighting(uint32_t sr, double b[5], double a[5]) {
    TH_TRY
    TH_REQUIRE(b && a, "NULL argument");
    if (!loudness_rate_ok(sr)) return fail(TH_ERR_UNSUPPORTED, "sample rate %u outside [16, 2822400]", sr);
    k_weighting(sr, b, a);
    return TH_OK;
    TH_CATCH
}

TH_API int th_loudness_n_blocks(size_t n_samples, uint32_t sr, size_t *n_blocks) {
    TH_TRY
    TH_REQUIRE(n_blocks, "NULL argument");
    if (!loudness_rate_ok(sr)) return fail(TH_ERR_UNSUPPORTED, "sample rate %u outside [16, 2822400]", sr);
    *n_blocks = loudness_n_blocks(n_samples, sr);
    return TH_OK;
    TH_CATCH
}

TH_API int th_gated_loudness(const double *block_energies, size_t n, double *lufs) {
    TH_TRY
    TH_REQUIRE(lufs && (n == 0 || block_energies), "NULL argument");
    *lufs = gated_loudness(block_energies, n);
    return TH_OK;
    TH_CATCH
}

TH_API int th_true_peak_filter(uint32_t sr, uint32_t *factor, double coef[49], uint32_t phase[49], uint32_t delay[49], uint32_t *n_taps) {
    TH_TRY
    TH_REQUIRE(factor && coef && phase && delay && n_taps, "NULL argument");
    *factor = true_peak_factor(sr);
    *n_taps = true_peak_filter(*factor, coef, phase, delay);
    return TH_OK;
    TH_CATCH
}

TH_API int th_loudness_n_short_term(size_t n_samples, uint32_t sr, size_t *n_blocks) {
    TH_TRY
    TH_REQUIRE(n_blocks, "NULL argument");
    if (!loudness_rate_ok(sr)) return fail(TH_ERR_UNSUPPORTED, "sample rate %u outside [16, 2822400]", sr);
    *n_blocks = loudness_n_short_term(n_samples, sr);
    return TH_OK;
    TH_CATCH
}

TH_API int th_loudness_range(const double *short_term_energies_1s, size_t n, double *lra) {
    TH_TRY
    TH_REQUIRE(lra && (n == 0 || short_term_energies_1s), "NULL argument");
    *lra = loudness_range(short_term_energies_1s, n);
    return TH_OK;
    TH_CATCH
}

TH_API int th_normalize_gain(int kind, float target, const th_audio_stats *orig, float *gain) {
    TH_TRY
    TH_REQUIRE(orig && gain, "NULL argument");
    TH_REQUIRE(normalize_gain(kind, target, orig->global_lufs, orig->rms_dB, orig->max_peak_dB, gain), "unknown normalize kind %d", kind);
    return TH_OK;
    TH_CATCH
}

TH_API int th_limiter_params(uint32_t sr, th_limiter_desc *out) {
    TH_TRY
    TH_REQUIRE(out, "NULL argument");
    LimiterParams p{};
    if (!limiter_params(sr, &p)) return fail(TH_ERR_UNSUPPORTED, "sample rate %u: the limiter's attack would be 0 samples", sr);
    *out = th_limiter_desc{};
    out->attack = p.attack;
    out->hold_length = p.hold_length;
    out->release_samples = p.release_samples;
    for (int i = 0; i < 3; i++) out->box_len[i] = p.box_len[i];
    return TH_OK;
    TH_CATCH
}

TH_API int th_spectrum_frame_range(uint32_t sr, size_t hop, size_t n_frames, double start_sec, double end_sec, size_t *frame_start,
                                   size_t *frame_end) {
    TH_TRY
    TH_REQUIRE(frame_start && frame_end, "NULL argument");
    TH_REQUIRE(spectrum_frame_range(sr, hop, n_frames, start_sec, end_sec, frame_start, frame_end),
               "bad time range [%g, %g) s at sr %u, hop %zu", start_sec, end_sec, sr, hop);
    return TH_OK;
    TH_CATCH
}

// ---- the host arithmetic of the PCM / WAV export (export_core.h is what the kernel runs too)
TH_API int th_audio_sample_range(uint32_t sr, size_t n_samples, double start_sec, double end_sec, size_t *sample_start,
                                 size_t *sample_end) {
    TH_TRY
    TH_REQUIRE(sample_start && sample_end, "NULL argument");
    TH_REQUIRE(spectrum_frame_range(sr, 1, n_samples, start_sec, end_sec, sample_start, sample_end),
               "bad time range [%g, %g) s at sr %u", start_sec, end_sec, sr);
    return TH_OK;
    TH_CATCH
}

TH_API int th_export_dither(uint32_t seed, uint32_t ch, uint64_t i, uint32_t *a, uint32_t *b) {
    TH_TRY
    TH_REQUIRE(a && b, "NULL argument");
    export_dither_ab(export_dither_k1(export_dither_k0(seed, ch), i), i, a, b);
    return TH_OK;
    TH_CATCH
}

TH_API int th_export_quantize(uint32_t format, uint32_t dither, uint32_t seed, uint32_t ch, uint64_t first_index, const float *x,
                              size_t n, int32_t *q, uint64_t *n_clamped, uint64_t *n_nan) {
    TH_TRY
    TH_REQUIRE(n_clamped && n_nan && (n == 0 || (x && q)), "NULL argument");
    TH_REQUIRE(format <= TH_PCM_F32, "unknown format %u", format);
    TH_REQUIRE(dither <= TH_DITHER_TPDF, "unknown dither %u", dither);
    uint64_t clamped = 0, nan = 0;
    const uint32_t k0 = export_dither_k0(seed, ch);
    const bool tpdf = dither == TH_DITHER_TPDF;
    const double S = export_scale(format);
    for (size_t j = 0; j < n; j++) {
        if (format == TH_PCM_F32) {
            std::memcpy(&q[j], &x[j], 4);
            nan += x[j] != x[j];
            continue;
        }
        const uint64_t i = first_index + j;
        uint32_t a = 0, b = 0;
        if (tpdf) export_dither_ab(export_dither_k1(k0, i), i, &a, &b);
        ExportCounts c{0, 0};
        q[j] = export_quantize_one(x[j], S, tpdf, a, b, &c);
        clamped += c.clamped;
        nan += c.nan;
    }
    *n_clamped = clamped;
    *n_nan = nan;
    return TH_OK;
    TH_CATCH
}

TH_API int th_wav_header(uint32_t format, uint32_t sr, uint32_t n_ch, uint64_t n_frames, uint8_t out[TH_WAV_HEADER_MAX],
                         size_t *header_len, size_t *pad_len) {
    TH_TRY
    return tmi::wav_header_checked(format, sr, n_ch, n_frames, out, header_len, pad_len);
    TH_CATCH
}

// ---- the FLAC stream on the host (flac_core.h and flac_block.h are what the kernels run too)
namespace th {
namespace tmi {
int flac_stream_checked(uint32_t sr, uint32_t n_ch, uint32_t format, uint64_t n_frames) {
    TH_REQUIRE(format == TH_PCM_S16 || format == TH_PCM_S24, "a FLAC stream is TH_PCM_S16 or TH_PCM_S24 (format %u)", format);
    TH_REQUIRE(n_ch != 0 && sr != 0, "a FLAC stream needs at least one channel and a sample rate (%u channels at %u Hz)", n_ch, sr);
    if (n_ch > FLAC_MAX_CHANNELS || sr > FLAC_MAX_RATE || n_frames >= FLAC_MAX_SAMPLES)
        return fail(TH_ERR_UNSUPPORTED, "%llu frames of %u channels at %u Hz do not fit a FLAC stream (8 channels, 1048575 Hz, 2^36 - 1 frames)",
                    (unsigned long long)n_frames, n_ch, sr);
    return TH_OK;
}
}  // namespace tmi
}  // namespace th

TH_API int th_flac_bound(uint64_t n_frames, uint32_t n_ch, uint32_t format, uint64_t *bytes) {
    TH_TRY
    TH_REQUIRE(bytes, "NULL argument");
    TH_CHECK(tmi::flac_stream_checked(1, n_ch, format, n_frames));
    *bytes = flac_stream_bound(n_frames, n_ch, flac_bps(format));
    return TH_OK;
    TH_CATCH
}

TH_API int th_flac_frame_header(uint32_t sr, uint32_t n_ch, uint32_t format, uint64_t frame_number, uint32_t block_len, uint8_t out[16],
                                size_t *len) {
    TH_TRY
    TH_REQUIRE(out && len, "NULL argument");
    TH_CHECK(tmi::flac_stream_checked(sr, n_ch, format, 0));
    TH_REQUIRE(block_len >= 1 && block_len <= FLAC_BLOCK, "a block of %u samples (1 .. %u)", block_len, FLAC_BLOCK);
    TH_REQUIRE(frame_number < FLAC_MAX_SAMPLES, "frame number %llu (below 2^36)", (unsigned long long)frame_number);
    *len = flac_frame_header(sr, n_ch, flac_bps(format), frame_number, block_len, out);
    return TH_OK;
    TH_CATCH
}

TH_API int th_flac_encode_i32(const int32_t *const *chan, uint32_t n_ch, uint64_t n, uint32_t format, uint32_t sr, uint8_t *out, size_t cap,
                              size_t *out_len) {
    return th_flac_encode_i32_ex(chan, n_ch, n, format, sr, 0u, out, cap, out_len);
}

TH_API int th_flac_encode_i32_ex(const int32_t *const *chan, uint32_t n_ch, uint64_t n, uint32_t format, uint32_t sr, uint32_t flags,
                                 uint8_t *out, size_t cap, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(out_len && (n == 0 || chan), "NULL argument");
    *out_len = 0;
    TH_REQUIRE(format == TH_PCM_S16 || format == TH_PCM_S24, "a FLAC stream is TH_PCM_S16 or TH_PCM_S24 (format %u)", format);
    TH_REQUIRE((flags & ~FLAC_FLAGS) == 0, "FLAC flags %#x (TH_FLAC_LPC | TH_FLAC_STEREO)", flags);
    TH_CHECK(tmi::flac_stream_checked(sr, n_ch, format, n));
    const uint32_t bps = flac_bps(format);
    const int32_t lim = 1 << (bps - 1);
    for (uint32_t c = 0; c < n_ch && n; c++) {
        TH_REQUIRE(chan[c], "NULL argument");
        for (uint64_t i = 0; i < n; i++)
            TH_REQUIRE(chan[c][i] >= -lim && chan[c][i] < lim, "channel %u sample %llu is not a %u-bit integer", c, (unsigned long long)i, bps);
    }
    const uint64_t bound = flac_stream_bound(n, n_ch, bps);
    *out_len = (size_t)bound;
    if (!out || cap < bound) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %llu bytes", (unsigned long long)bound);
    // the device's pipeline, run by run: pieces, slots, tables and staging of the plan's sizes
    const FlacPlanRequest pr{n_ch, format, TH_DITHER_NONE, 0u, sr, 0, n, 0, flags};
    FlacPlan pl = plan_flac(&pr, 1, TH_EXPORT_PIECE_BYTES);
    if (pl.err != TH_OK) return fail(pl.err, "%s", pl.err_text.c_str());
    uint64_t at = FLAC_STREAM_HEADER;
    uint32_t mn = 0xffffffffu, mx = 0;
    for (size_t pi = 0; pi < pl.pieces.size(); pi++) {
        const FlacPiece &pc = pl.pieces[pi];
        std::vector<uint8_t> stage(pc.bound);
        std::vector<uint32_t> slots(pc.slot_words), bits(pc.n_units), foff(pc.n_blocks);
        std::vector<FlacJobResult> res(pl.runs.size());
        std::vector<unsigned char> tab_mem(pl.tab_bytes);
        bind_flac(pl, FlacBases{{stage.data(), stage.data()}, slots.data(), bits.data(), foff.data(), res.data(), tab_mem.data(), nullptr}, &pr, 1,
                  nullptr);
        for (size_t k = pc.run0; k < pc.run1; k++) {
            flac_run_job_host(pl.jobs[k], chan, nullptr);
            std::memcpy(out + at, pl.jobs[k].dst, res[k].bytes);
            at += res[k].bytes;
            mn = std::min(mn, res[k].min_frame);
            mx = std::max(mx, res[k].max_frame);
        }
    }
    flac_stream_header(sr, n_ch, bps, n, mx ? mn : 0u, mx, out);
    *out_len = (size_t)at;
    return TH_OK;
    TH_CATCH
}

// ---- the host arithmetic of the resampler (resample_core.h is what the kernel runs too)
namespace {
int resample_plan_checked(uint32_t sr_in, uint32_t sr_out, th_resample_plan *p) {
    const int rc = th::resample_plan(sr_in, sr_out, p);
    TH_REQUIRE(rc != 1, "a sample rate of zero (%u -> %u Hz)", sr_in, sr_out);
    if (rc != 0) return th::fail(TH_ERR_UNSUPPORTED, "%u -> %u Hz needs more than %u taps or %u coefficients", sr_in, sr_out,
                                 TH_RESAMPLE_MAX_TAPS, TH_RESAMPLE_MAX_COEFS);
    return TH_OK;
}
}  // namespace

TH_API int th_resample_plan_for(uint32_t sr_in, uint32_t sr_out, th_resample_plan *out) {
    TH_TRY
    TH_REQUIRE(out, "NULL argument");
    return resample_plan_checked(sr_in, sr_out, out);
    TH_CATCH
}

TH_API int th_resample_n_out(size_t n_in, uint32_t sr_in, uint32_t sr_out, size_t *n_out) {
    TH_TRY
    TH_REQUIRE(n_out, "NULL argument");
    th_resample_plan p;
    TH_CHECK(resample_plan_checked(sr_in, sr_out, &p));
    if (!resample_n_out(n_in, p, n_out)) return fail(TH_ERR_UNSUPPORTED, "%zu samples at %u -> %u Hz: indices beyond 64 bits", n_in, sr_in, sr_out);
    return TH_OK;
    TH_CATCH
}

TH_API int th_resample_coefs(uint32_t sr_in, uint32_t sr_out, uint32_t r, double *h64, float *c32) {
    TH_TRY
    th_resample_plan p;
    TH_CHECK(resample_plan_checked(sr_in, sr_out, &p));
    TH_REQUIRE(r < p.L, "phase %u of %u", r, p.L);
    resample_row(p, r, h64, c32);
    return TH_OK;
    TH_CATCH
}

TH_API int th_resample_f32(const float *x, size_t n_in, uint32_t sr_in, uint32_t sr_out, uint64_t j0, size_t n, float *y) {
    TH_TRY
    TH_REQUIRE(n == 0 || y, "NULL argument");
    TH_REQUIRE(n_in == 0 || x, "NULL argument");
    th_resample_plan p;
    TH_CHECK(resample_plan_checked(sr_in, sr_out, &p));
    size_t n_out = 0;
    if (!resample_n_out(n_in, p, &n_out)) return fail(TH_ERR_UNSUPPORTED, "%zu samples at %u -> %u Hz: indices beyond 64 bits", n_in, sr_in, sr_out);
    TH_REQUIRE(j0 <= n_out && n <= n_out - j0, "outputs [%llu, +%zu) of %zu", (unsigned long long)j0, n, n_out);
    const uint32_t taps = 2 * p.half_taps;
    const int64_t K = p.half_taps;
    std::vector<float> win(taps);
    std::vector<std::vector<float>> rows(p.L);  // (made when first met: outputs j and j + L share a row)
    for (size_t i = 0; i < n; i++) {
        uint64_t q;
        uint32_t r;
        resample_phase(j0 + i, p.L, p.M, &q, &r);
        std::vector<float> &row = rows[r];
        if (row.empty()) {
            row.resize(taps);
            resample_row(p, r, nullptr, row.data());
        }
        const int64_t first = (int64_t)q - K + 1;
        for (int64_t k = 0; k < (int64_t)taps; k++) win[k] = first + k >= 0 && first + k < (int64_t)n_in ? x[first + k] : 0.0f;
        ResampleAcc acc;
        resample_taps(acc, row.data(), win.data(), taps);
        y[i] = resample_fold(acc);
    }
    return TH_OK;
    TH_CATCH
}

// ---- the host arithmetic of the band filter (the summation is the resampler's: resample_core.h)
TH_API int th_band_plan_for(uint32_t sr, uint32_t mode, double f_lo_hz, double f_hi_hz, double trans_hz, th_band_plan *out) {
    TH_TRY
    TH_REQUIRE(out, "NULL argument");
    const int rc = th::band_plan_for(sr, mode, f_lo_hz, f_hi_hz, trans_hz, out);
    TH_REQUIRE(rc != 1, "bad band (mode %u, [%g, %g] Hz, transition %g Hz) at %u Hz", mode, f_lo_hz, f_hi_hz, trans_hz, sr);
    if (rc != 0) return fail(TH_ERR_UNSUPPORTED, "a transition of %g Hz at %u Hz needs more than %u taps", trans_hz, sr, TH_BAND_MAX_TAPS);
    return TH_OK;
    TH_CATCH
}

namespace {
int band_plan_usable(uint32_t sr, const th_band_plan *p) {
    TH_REQUIRE(p, "NULL argument");
    TH_REQUIRE(sr != 0 && p->half_taps != 0 && 2 * (uint64_t)p->half_taps <= TH_BAND_MAX_TAPS && p->mode <= TH_BAND_STOP,
               "not a filter's plan (%u half taps, mode %u, %u Hz)", p->half_taps, p->mode, sr);
    return TH_OK;
}
}  // namespace

TH_API int th_band_coefs(uint32_t sr, const th_band_plan *plan, double *h64, float *c32) {
    TH_TRY
    TH_CHECK(band_plan_usable(sr, plan));
    band_row(sr, *plan, h64, c32);
    return TH_OK;
    TH_CATCH
}

TH_API int th_band_response(uint32_t sr, const th_band_plan *plan, const double *hz, size_t n, double *db) {
    TH_TRY
    TH_CHECK(band_plan_usable(sr, plan));
    TH_REQUIRE(n == 0 || (hz && db), "NULL argument");
    std::vector<float> row(2 * (size_t)plan->half_taps);
    band_row(sr, *plan, nullptr, row.data());
    band_response(sr, row.data(), plan->half_taps, hz, n, db);
    return TH_OK;
    TH_CATCH
}

TH_API int th_band_f32(const float *x, size_t n_in, const float *c32, uint32_t half_taps, uint64_t j0, size_t n, float *y) {
    TH_TRY
    TH_REQUIRE(n == 0 || y, "NULL argument");
    TH_REQUIRE(n_in == 0 || x, "NULL argument");
    TH_REQUIRE(c32 && half_taps != 0 && 2 * (uint64_t)half_taps <= TH_BAND_MAX_TAPS, "a row of 2 x %u taps", half_taps);
    TH_REQUIRE(j0 <= n_in && n <= n_in - j0, "outputs [%llu, +%zu) of %zu", (unsigned long long)j0, n, n_in);
    const uint32_t taps = 2 * half_taps;
    const int64_t K = half_taps;
    // x with K - 1 zeros in front and K behind outputs [j0, j0 + n): output i's window starts at padded[i]
    std::vector<float> padded(n + taps - 1, 0.0f);
    for (size_t p = 0; p < padded.size(); p++) {
        const int64_t at = (int64_t)j0 - K + 1 + (int64_t)p;
        if (at >= 0 && at < (int64_t)n_in) padded[p] = x[at];
    }
    for (size_t i = 0; i < n; i++) {
        ResampleAcc acc;
        resample_taps(acc, c32, padded.data() + i, taps);
        y[i] = resample_fold(acc);
    }
    return TH_OK;
    TH_CATCH
}

namespace th {

LoudnessBatch::~LoudnessBatch() {
    if (d_own) (void)hipSetDevice(ctx->device);  // (d_own goes behind this body)
}

int loudness_enqueue(th_ctx *c, const th_audio_desc *descs, size_t n, bool own_memory, bool allow_bad_rate, LoudnessBatch *b) {
    b->ctx = c;
    std::vector<uint32_t> rate_of(n, 0);
    std::vector<const LoudnessRate *> rates;
    std::vector<LoudJob> jobs;
    std::vector<LoudTrackJob> tjobs;
    size_t n_states = 0, n_blocks = 0;
    uint32_t max_chunks = 0, max_fchunks = 0, lds_floats = 4;
    uint64_t max_blocks = 0;
    for (size_t t = 0; t < n; t++) {
        const th_audio_desc &d = descs[t];
        TH_REQUIRE(d.n_channels >= 1 && d.channels, "track %zu: no channels", t);
        TH_REQUIRE(d.n_samples < (1ull << 40), "track %zu: too many samples", t);
        TH_REQUIRE_ALIGNED(d.block_energy, 8, "track %zu: block_energy must be 8-byte aligned", t);
        const bool ok = loudness_rate_ok(d.sr);
        if (!ok && !allow_bad_rate) return fail(TH_ERR_UNSUPPORTED, "track %zu: sample rate %u outside [16, 2822400]", t, d.sr);
        // (a refused rate: the sums only, over chunks of a 48 kHz geometry)
        const LoudnessRate &R = loudness_rate(ok ? d.sr : 48000);
        size_t ri = 0;
        while (ri < rates.size() && rates[ri] != &R) ri++;
        if (ri == rates.size()) rates.push_back(&R);
        const uint64_t nb = ok ? loudness_n_blocks(d.n_samples, d.sr) : 0;
        const uint64_t nseg = (d.n_samples + R.s100 - 1) / R.s100;
        TH_REQUIRE(nseg * R.n_sub < (1ull << 31), "track %zu: too many samples", t);
        const uint32_t nch = (uint32_t)(nseg * R.n_sub), nf = nb ? (uint32_t)((nb + 3) * R.n_sub) : 0u;
        b->ch0.push_back(jobs.size());
        b->blk0.push_back(n_blocks);
        b->srs.push_back(d.sr);
        b->ns.push_back(d.n_samples);
        for (uint32_t k = 0; k < d.n_channels; k++) {
            TH_REQUIRE(d.n_samples == 0 || d.channels[k], "track %zu channel %u: NULL device pointer", t, k);
            TH_REQUIRE_ALIGNED(d.channels[k], 4, "track %zu channel %u: channels[] must be 4-byte aligned", t, k);
            LoudJob j{};
            j.wav = d.channels[k];
            j.n = d.n_samples;
            j.rate = (uint32_t)ri;
            j.n_chunks = nch;
            j.n_fchunks = nf;
            j.aligned16 = (reinterpret_cast<uintptr_t>(d.channels[k]) & 15u) == 0;
            jobs.push_back(j);
            n_states += nf;
        }
        LoudTrackJob tj{};
        tj.n_blocks = nb;
        for (uint32_t k = 0; k < 8; k++) tj.w[k] = loudness_channel_weight(k, d.n_channels);
        tj.n_ch = d.n_channels;
        tj.n_sub = R.n_sub;
        tj.n_fchunks = nf;
        tj.L = 4 * R.s100;
        tjobs.push_back(tj);
        n_blocks += nb;
        max_chunks = std::max(max_chunks, nch);
        max_fchunks = std::max(max_fchunks, nf);
        max_blocks = std::max<uint64_t>(max_blocks, nb);
        lds_floats = std::max(lds_floats, R.cl + 4);
    }
    TH_REQUIRE(jobs.size() <= 65535 && n <= 65535, "at most 65535 channels and tracks per call");
    b->n_ch = jobs.size();
    b->n_blocks = n_blocks;
    // device layout: [jobs][rates][track jobs] | [sums n_ch][peaks n_ch (u32, padded)][block energies] | [states 8 / chunk][energies]
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_rates = up(jobs.size() * sizeof(LoudJob)), o_tj = o_rates + up(rates.size() * sizeof(LoudnessRate));
    const size_t o_sums = o_tj + up(tjobs.size() * sizeof(LoudTrackJob));
    const size_t sums_bytes = b->n_ch * 8 + (b->n_ch * 4 + 7) / 8 * 8;
    const size_t o_blk = o_sums + sums_bytes, o_z = up(o_blk + n_blocks * 8), o_q = o_z + n_states * 64;
    const size_t total = o_q + n_states * 8 + 8;
    TH_HIP(hipSetDevice(c->device));
    unsigned char *dm;
    if (own_memory) {
        TH_HIP(b->d_own.alloc(total));
        dm = b->d_own;
    } else {
        TH_HIP(hipStreamSynchronize(c->stream));  // (the last call's launches may still read the tables)
        const int rc = c->loud_mem.ensure(total);
        if (rc != TH_OK) return rc;
        dm = static_cast<unsigned char *>(c->loud_mem.dptr);
    }
    b->d_sums = reinterpret_cast<double *>(dm + o_sums);
    double *d_blk = reinterpret_cast<double *>(dm + o_blk), *d_z = reinterpret_cast<double *>(dm + o_z), *d_q = reinterpret_cast<double *>(dm + o_q);
    uint32_t *d_pk = reinterpret_cast<uint32_t *>(dm + o_sums + b->n_ch * 8);
    size_t si = 0;
    for (size_t t = 0, jc = 0; t < n; t++) {
        const size_t q0 = si;
        for (uint32_t k = 0; k < descs[t].n_channels; k++, jc++) {
            LoudJob &j = jobs[jc];
            j.z = d_z + 8 * si;
            j.q = d_q + si;
            j.sumsq = b->d_sums + jc;
            j.peak = d_pk + jc;
            si += j.n_fchunks;
        }
        tjobs[t].q = d_q + q0;
        tjobs[t].out = d_blk + b->blk0[t];
    }
    std::vector<unsigned char> h(o_sums, 0);
    std::memcpy(h.data(), jobs.data(), jobs.size() * sizeof(LoudJob));
    for (size_t r = 0; r < rates.size(); r++) std::memcpy(h.data() + o_rates + r * sizeof(LoudnessRate), rates[r], sizeof(LoudnessRate));
    std::memcpy(h.data() + o_tj, tjobs.data(), tjobs.size() * sizeof(LoudTrackJob));
    TH_HIP(hipMemcpy(dm, h.data(), o_sums, hipMemcpyHostToDevice));  // (nothing on the stream reads this memory yet)
    TH_HIP(hipMemsetAsync(b->d_sums, 0, sums_bytes, c->stream));      // sums = 0, peaks = +0.0
    TH_HIP(launch_loudness(reinterpret_cast<const LoudJob *>(dm), (uint32_t)jobs.size(), max_chunks, max_fchunks,
                           reinterpret_cast<const LoudnessRate *>(dm + o_rates), lds_floats, reinterpret_cast<const LoudTrackJob *>(dm + o_tj),
                           (uint32_t)n, max_blocks, c->stream));
    for (size_t t = 0; t < n; t++)
        if (descs[t].block_energy && tjobs[t].n_blocks)
            TH_HIP(hipMemcpyAsync(descs[t].block_energy, tjobs[t].out, tjobs[t].n_blocks * 8, hipMemcpyDeviceToDevice, c->stream));
    return TH_OK;
}

int loudness_collect(LoudnessBatch *b, bool sync_stream) {
    th_ctx *c = b->ctx;
    TH_HIP(hipSetDevice(c->device));
    const size_t sums_bytes = b->n_ch * 8 + (b->n_ch * 4 + 7) / 8 * 8;
    b->h_sums.assign(sums_bytes / 8 + b->n_blocks, 0.0);
    if (sync_stream) {
        TH_HIP(hipMemcpyAsync(b->h_sums.data(), b->d_sums, sums_bytes + b->n_blocks * 8, hipMemcpyDeviceToHost, c->stream));
        TH_HIP(hipStreamSynchronize(c->stream));
    } else {
        TH_HIP(hipMemcpy(b->h_sums.data(), b->d_sums, sums_bytes + b->n_blocks * 8, hipMemcpyDeviceToHost));
    }
    return TH_OK;
}

void loudness_result(const LoudnessBatch &b, size_t t, th_audio_stats *out) {
    *out = th_audio_stats{};
    const size_t c0 = b.ch0[t], c1 = t + 1 < b.ch0.size() ? b.ch0[t + 1] : b.n_ch;
    const size_t sums_words = (b.n_ch * 8 + (b.n_ch * 4 + 7) / 8 * 8) / 8;
    const uint32_t *pk = reinterpret_cast<const uint32_t *>(b.h_sums.data() + b.n_ch);
    // StatCalculator::calc (stats.rs:62-77): f32 sums of the channels' f32 sums of squares, f32 division, log_for_dB (amin = 0)
    float ss = 0.0f, peak = 0.0f;
    for (size_t k = c0; k < c1; k++) {
        ss += (float)b.h_sums[k];
        float p;
        std::memcpy(&p, &pk[k], 4);
        peak = std::max(peak, p);
    }
    const float mean_sq = ss / (float)((double)(c1 - c0) * (double)b.ns[t]);
    // (the logarithms in f64, rounded once: within half an ulp of the exact f32 result, where log10f itself may be off by one)
    out->rms_dB = mean_sq == 0.0f ? -INFINITY : (float)(10.0 * std::log10((double)mean_sq));
    out->max_peak = peak;
    out->max_peak_dB = peak == 0.0f ? -INFINITY : (float)(20.0 * std::log10((double)peak));
    const size_t nb = (t + 1 < b.blk0.size() ? b.blk0[t + 1] : b.n_blocks) - b.blk0[t];
    out->global_lufs = loudness_rate_ok(b.srs[t]) ? gated_loudness(b.h_sums.data() + sums_words + b.blk0[t], nb) : NAN;
}

}  // namespace th

TH_API int th_audio_stats_dev(th_ctx *c, const th_audio_desc *descs, size_t n, th_audio_stats *out_host) {
    TH_TRY
    TH_CHECK(refuse_while_capturing("th_audio_stats_dev (it returns to host memory)"));
    TH_REQUIRE(c, "ctx is NULL");
    if (n == 0) return TH_OK;
    TH_REQUIRE(descs && out_host, "NULL argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    LoudnessBatch b;
    int rc = loudness_enqueue(c, descs, n, false, false, &b);
    if (rc == TH_OK) rc = loudness_collect(&b, true);
    if (rc != TH_OK) return rc;
    for (size_t t = 0; t < n; t++) loudness_result(b, t, &out_host[t]);
    return TH_OK;
    TH_CATCH
}
