// context.h — definitions of the opaque handles (th_ctx, th_plan) shared by api.hip and
// track_manager.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "common.h"
#include "stft_core.h"

namespace th {

// Small device buffer holding a descriptor table; remembers the last uploaded bytes so that
// re-sending an identical table (bench loops, repeated tile requests) costs nothing.
struct DeviceTable {
    void *dptr = nullptr;
    size_t cap = 0;
    std::vector<unsigned char> last;
    int ensure(size_t bytes);
    int upload(hipStream_t s, const void *src, size_t bytes);
    void release();
};

// th_plan_set_kernel's selectors (bits 0-7), described in include/thesia_amd_testing.h.  Product builds refuse the A/B-only
// ones there (9, 11, 14 at n_fft 32768 / 65536, 15 at n_fft 8192, and wave counts other than a size's own).
enum StftSelector : int {
    SEL_AUTO = 0,
    SEL_GENERIC = 1,
    SEL_WAVE = 2,              // every selector from here on asks for a wave kernel
    SEL_MEL_AMP = 3,           // amplitude rows + a second mel kernel
    SEL_NO_PHASE = 4,
    SEL_PHASE_FUSED = 5,
    SEL_MULTI_1024 = 6,
    SEL_MEL_MFMA = 7,          // as 3, the matrix-core kernel also where 3 runs mel_rows / mel_band_rows
    SEL_MEL_PIECES = 8,
    SEL_PACKED = 9,
    SEL_RESERVED = 10,         // as 2
    SEL_SWEEP = 11,
    SEL_MEL_TWO_KERNELS = 12,
    SEL_MEL_ONE_FRAME = 13,
    SEL_BLOCK = 14,
    SEL_SUBWAVE = 15,
};

// Which kernels a plan launches, and how: everything about a th_calc_spec_batch_dev launch that the batch does not change.
// resolve_route (api.hip) fills it from the plan's geometry, its tables and its kernel selector — at th_plan_create and at every
// th_plan_set_kernel — and nothing else reads the selector.
struct StftRoute {
    enum class Main : uint8_t { Generic, Bluestein, Wave, WaveMulti, Block, Subwave };
    // the mel filterbank in the main kernel's epilogue (mel_fuse.h): moment form with its table in global memory, the same as
    // per-lane constants of the block kernel, mel_rows_kernel's table (n_fft 512), banded sums one frame or two at a time, pieces / gather
    enum class MelFused : uint8_t { None, Moment, MomentLanes, Rows, Banded, BandedPairs, Pieces };
    enum class MelSecond : uint8_t { None, Rows, BandRows, Mfma };  // the mel kernel behind amplitude rows
    Main main = Main::Generic;
    MelFused mel_fused = MelFused::None;
    MelSecond mel_second = MelSecond::None;
    bool no_wave_kernel = false;   // a selector >= 2 asked for a wave kernel this plan has none of: th_calc_spec_batch_dev fails
    int phase_mode = 0;            // StftGeom::phased of the launch (grid-aligned frame loop; window table d_wtab_phased when != 0)
    int waves = 0;                 // waves per workgroup of the wave kernels
    uint32_t tail_guard = 0;       // stft_wave_multi_tail_guard, or 0
    bool edges_in_wave = false;    // boundary frames of channels of at least n_fft samples run inside the wave launch
    int long_plan = 1;             // WaveOut::long_plan: 1 stft_block_kernel, 2 stft_subwave_kernel (read at n_fft 8192 and above)
    bool sweep = false;            // selector 11's sweep schedule exists for this plan (the launch adds: the batch is large enough)
    bool packed = false;           // selector 9: WaveOut::packed
    char name[48] = "";            // th_plan_kernel_name
    bool wave() const { return main != Main::Generic && main != Main::Bluestein; }
    int out_mode() const { return mel_second != MelSecond::None ? 1 : mel_fused != MelFused::None ? 2 : 0; }  // WaveOut::mode
};

}  // namespace th

struct th_ctx {
    int device = 0;
    uint32_t n_cu = 256;  // compute units (persistent-grid size of the wave kernel)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // Serialises use of the stream-side scratch below; recursive so composed entry points
    // (tile encoders → batched launchers) can hold it across the whole request.
    std::recursive_mutex mu;
    th::DeviceTable img_jobs, img_start, raster_jobs, raster_start, wave_jobs, wave_start, colormap, tile_out, lod_tabs, lod_tmp,
        pyr_jobs, pyr_sums, fused_jobs, fused_start, fused_ptrs, loud_mem;
    // the descriptor batches the img / raster tables were built from (identical batch -> tables reused as they are)
    std::vector<unsigned char> img_descs_key, raster_descs_key, fused_key;
    uint32_t img_tiles_key = 0, raster_blocks_key = 0, fused_blocks_key = 0;
    void release_scratch() {
        img_descs_key.clear();
        raster_descs_key.clear();
        fused_key.clear();
        fused_jobs.release();
        fused_start.release();
        fused_ptrs.release();
        img_jobs.release();
        img_start.release();
        raster_jobs.release();
        raster_start.release();
        wave_jobs.release();
        wave_start.release();
        colormap.release();
        tile_out.release();
        lod_tabs.release();
        lod_tmp.release();
        pyr_jobs.release();
        pyr_sums.release();
        loud_mem.release();
    }
};

struct th_plan {
    th_ctx *ctx = nullptr;
    uint32_t sr = 0;
    int freq_scale = 0;
    int kernel_choice = 0;  // th_plan_set_kernel's selector (th::StftSelector); read by resolve_route only
    int wave_waves = 0;     // tuning: waves per workgroup of the wave kernel (0 = default)
    int wave_chunk = 0;     // tuning: frames per chunk of the wave kernel (0 = default)
    // th_plan_time_kernel: a ring of event pairs around the STFT kernel launch (no synchronisation while recording)
    static constexpr size_t TIMER_SLOTS = 64;
    bool time_kernel = false;
    uint64_t timed_launches = 0;
    std::vector<hipEvent_t> ev_k0, ev_k1;
    th::StftGeom g{};
    float *d_window = nullptr;
    th::cf32 *d_tw = nullptr;
    // Bluestein plans (an odd factor of n_fft above 63; stft_bluestein_kernel): complex-double tables, NULL otherwise
    double *d_bs_chirp = nullptr, *d_bs_bhat = nullptr, *d_bs_twm = nullptr, *d_bs_tws = nullptr;
    bool bluestein() const { return d_bs_chirp != nullptr; }
    uint32_t *d_queue_head = nullptr;  // wave kernel: chunk queue head (rewound by wave_post_kernel after every launch)
    bool queue_dirty = false;          // a wave launch went out whose rewind did not: the next launch zeroes the head first
    th::cf32 *d_wtab = nullptr;  // wave kernel: 0.5 * zero-padded window as (even, odd) pairs
    th::cf32 *d_wtab_phased = nullptr;  // phased mode: 48 zero pairs + the table with the window at offset 0 (NULL: not applicable)
    float *d_mel_fb = nullptr;
    uint32_t *d_mel_lo = nullptr, *d_mel_hi = nullptr;
    std::vector<float> h_mel_fb;
    // MFMA mel path: filterbank packed per (N tile of 16 mels, K block of 16 bins) in operand order (256 floats per
    // block, band blocks only, + one all-zero block), per-tile band {klo, khi, first block}
    float *d_mel_bt = nullptr;
    uint32_t *d_mel_band = nullptr, *d_mel_slice = nullptr;  // + slices of the tile range with ~equal K-group counts
    uint32_t mel_kblocks = 0, mel_ntiles = 0, mel_zero_block = 0, mel_slices = 0;
    uint32_t *d_mel_rows = nullptr;  // short rows under narrow filters: the per-mel table of mel_rows_kernel (kernels.h)
    uint32_t mel_rows_groups = 0;
    th::DeviceTable amp_buf, mel_jobs, mel_tile_start;  // amplitude scratch + job tables of mel_mfma_kernel
    size_t amp_zeroed = 0;                               // bytes of amp_buf known to be zero-initialised
    th::DeviceTable chunk_mm;                            // (min, max) per chunk of the wave kernel's last launch
    th::DeviceTable gen_scratch;                         // n_fft >= 32768: frame buffers of the generic kernel (global scratch)
    th::DeviceTable post_jobs;                           // per-channel tile ranges for wave_post_kernel
    // fused mel epilogue: device copy of the mel_fuse.h word table
    uint32_t *d_mel_fuse = nullptr;
    uint32_t mel_fuse_words = 0, mel_fuse_slots = 0, mel_fuse_groups = 0;
    // the same epilogue as banded sums, lane = mel (build_mel_band): the default where its table fits; selector 8 keeps the pieces
    uint32_t *d_mel_bsum = nullptr;
    uint32_t mel_bsum_words = 0, mel_bsum_groups = 0, mel_bsum_hdr[16] = {};  // (header: offset and taps per group)
    th::cf32 *d_twc = nullptr;  // n_fft 32768: the combining pass's per-thread constants (kernels_stft_long.hip)
    uint32_t mel_bsum_reach = 0;  // one past the highest amplitude index the banded sums read (MelBandHost::reach)
    // n_fft 4096 mel plans (round 6): the moment form of the filterbank in the FFT kernel's epilogue (build_mel_moments, mel_fuse.h)
    uint32_t *d_mel_mom = nullptr;
    uint32_t mel_mom_groups = 0, mel_mom_taps = 0;
    double mel_mom_max_dev = 0.0, mel_mom_max_amp = 0.0;
    th::DeviceTable jobs, tile_start;            // main launch: jobs + first chunk of every job (generic kernel) or the
                                                 // per-chunk (job, first frame) table (wave kernels)
    th::DeviceTable edge_jobs, edge_tile_start;  // boundary frames handed to the generic kernel
    th::StftRoute route;                         // resolve_route (api.hip)
};

namespace th {
// A batch of th_audio_desc tracks on a context's stream (th_audio_stats_dev; th_tm_add_tracks: one per group of tracks).
// loudness_enqueue uploads the tables (synchronously, into `scratch` after the stream has drained, or into a fresh allocation of
// the batch's own) and enqueues the passes; loudness_collect reads the results back once the stream has got that far.
struct LoudnessBatch {
    th_ctx *ctx = nullptr;
    void *d_own = nullptr;     // the batch's own device memory (NULL: the context's loud_mem)
    double *d_sums = nullptr;  // n_ch sums of squares, then n_ch peaks (u32), then the block energies of every track
    size_t n_ch = 0, n_blocks = 0;
    std::vector<size_t> ch0, blk0;  // per track: first channel, first block
    std::vector<uint32_t> srs;
    std::vector<uint64_t> ns;
    std::vector<double> h_blocks;
    std::vector<double> h_sums;
    LoudnessBatch() = default;
    LoudnessBatch(const LoudnessBatch &) = delete;
    LoudnessBatch &operator=(const LoudnessBatch &) = delete;
    ~LoudnessBatch();
};
// allow_bad_rate: a track at a rate outside [16, 2 822 400] gets its sums only (global_lufs = NaN) instead of TH_ERR_UNSUPPORTED
int loudness_enqueue(th_ctx *c, const th_audio_desc *descs, size_t n, bool own_memory, bool allow_bad_rate, LoudnessBatch *b);
int loudness_collect(LoudnessBatch *b, bool sync_stream);
void loudness_result(const LoudnessBatch &b, size_t t, th_audio_stats *out);
}  // namespace th
