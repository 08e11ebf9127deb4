// context.h — definitions of the opaque handles (th_ctx, th_plan) shared by api.hip and
// track_manager.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "common.h"
#include "stft_core.h"
#include "stft_plan.h"  // StftRoute

namespace th {

// One hipMalloc allocation, freed with its owner (move-only).  The device it was allocated on must be current when it goes:
// th_plan_destroy / th_ctx_destroy set it before they delete, th_plan_create before its first allocation.
template <class T>
struct DeviceBuf {
    T *ptr = nullptr;
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf &) = delete;
    DeviceBuf &operator=(const DeviceBuf &) = delete;
    DeviceBuf(DeviceBuf &&o) noexcept : ptr(o.ptr) { o.ptr = nullptr; }
    DeviceBuf &operator=(DeviceBuf &&o) noexcept {
        if (this != &o) {
            reset();
            ptr = o.ptr;
            o.ptr = nullptr;
        }
        return *this;
    }
    ~DeviceBuf() { reset(); }
    void reset() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
    }
    T *get() const { return ptr; }
    operator T *() const { return ptr; }
    hipError_t alloc(size_t bytes) {
        reset();
        return hipMalloc((void **)&ptr, bytes);
    }
    int fill(const void *h, size_t bytes) {  // allocate and fill from host
        reset();
        void **d = (void **)&ptr;
        TH_HIP(hipMalloc(d, bytes));
        TH_HIP(hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice));
        return TH_OK;
    }
    template <class V>
    int fill(const std::vector<V> &h) { return fill(h.data(), h.size() * sizeof(V)); }
};

// Small device buffer holding a descriptor table; remembers the last uploaded bytes so that
// re-sending an identical table (bench loops, repeated tile requests) costs nothing.
struct DeviceTable {
    void *dptr = nullptr;
    size_t cap = 0;
    std::vector<unsigned char> last;
    int ensure(size_t bytes);
    int upload(hipStream_t s, const void *src, size_t bytes);
    void release();  // (for callers that free early; the destructor does the same)
    DeviceTable() = default;
    DeviceTable(const DeviceTable &) = delete;
    DeviceTable &operator=(const DeviceTable &) = delete;
    ~DeviceTable() { release(); }
};

// The device tables built from one batch of descriptors, named by the bytes of that batch: an identical batch (re-quantising after a
// dB-range or colormap change, benchmark loops) launches on them as they are.
struct KeyedTables {
    struct Src {
        const void *data;
        size_t bytes;
    };
    DeviceTable tab[3];
    std::vector<unsigned char> key;
    uint32_t n_blocks = 0;
    // (the key is set only behind a complete store, so a matching key says that every table is the batch's; a batch without blocks
    // never uploads its block table, and a launcher given no blocks reads none)
    bool hit(const void *k, size_t bytes) const { return !key.empty() && key.size() == bytes && std::memcmp(key.data(), k, bytes) == 0; }
    // The tables are about to be overwritten: the key is cleared first and names them again only once EVERY upload succeeded, so a
    // partly failed store never leaves an old key on mixed tables.  An empty source is skipped.
    int store(hipStream_t s, const void *k, size_t bytes, uint32_t blocks, std::initializer_list<Src> srcs) {
        key.clear();
        size_t i = 0;
        for (const Src &src : srcs) {
            if (src.bytes) TH_CHECK(tab[i].upload(s, src.data, src.bytes));
            i++;
        }
        key.assign(static_cast<const unsigned char *>(k), static_cast<const unsigned char *>(k) + bytes);
        n_blocks = blocks;
        return TH_OK;
    }
    template <class T>
    const T *at(size_t i) const { return static_cast<const T *>(tab[i].dptr); }
};

// Between th_ctx_capture_begin and th_ctx_capture_end on this thread: TH_ERR_HIP, and the capture marked as failed
// (th_ctx_capture_end then returns an error and no graph); TH_OK otherwise.  Called in front of everything that needs the host —
// a table upload, a scratch allocation, a synchronisation, a result read back — so that the HIP call the capture forbids is never
// made: it would invalidate the capture, and a stream whose capture was invalidated stays unusable after hipStreamEndCapture
// (hipStreamIsCapturing goes on reporting it: ROCm 7.2), and with it a context on a caller's stream.
int refuse_while_capturing(const char *what);

}  // namespace th

struct th_ctx {
    int device = 0;
    uint32_t n_cu = 256;  // compute units (persistent-grid size of the wave kernel)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // The legacy default stream cannot be captured (hipStreamBeginCapture refuses it), but a graph can be launched on it: a
    // context on it records on this stream of its own, which `stream` names between th_ctx_capture_begin and _end.
    hipStream_t capture_stream = nullptr;
    bool capture_swapped = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // Serialises use of the stream-side scratch below; recursive so composed entry points
    // (tile encoders → batched launchers) can hold it across the whole request.
    std::recursive_mutex mu;
    th::DeviceTable wave_jobs, wave_start, colormap, tile_out, lod_tabs, lod_tmp, pyr_jobs, pyr_sums, loud_mem;
    // jobs, block -> job table (and, fused, the tile pointers) of the last spec -> img / raster / quantise + raster batch
    th::KeyedTables img, raster, fused;
    ~th_ctx() {  // (th_ctx_destroy: device current, stream idle; the scratch tables above go after this body)
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
        if (capture_stream) (void)hipStreamDestroy(capture_stream);
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
    th::DeviceBuf<float> d_window;
    th::DeviceBuf<th::cf32> d_tw;
    // Bluestein plans (an odd factor of n_fft above 63; stft_bluestein_kernel): complex-double tables, NULL otherwise
    th::DeviceBuf<double> d_bs_chirp, d_bs_bhat, d_bs_twm, d_bs_tws;
    bool bluestein() const { return d_bs_chirp != nullptr; }
    th::DeviceBuf<uint32_t> d_queue_head;  // wave kernel: chunk queue head (rewound by wave_post_kernel after every launch)
    bool queue_dirty = false;          // a wave launch went out whose rewind did not: the next launch zeroes the head first
    th::DeviceBuf<th::cf32> d_wtab;  // wave kernel: 0.5 * zero-padded window as (even, odd) pairs
    th::DeviceBuf<th::cf32> d_wtab_phased;  // phased mode: 48 zero pairs + the table with the window at offset 0 (NULL: not applicable)
    th::DeviceBuf<float> d_mel_fb;
    th::DeviceBuf<uint32_t> d_mel_lo, d_mel_hi;
    std::vector<float> h_mel_fb;
    // MFMA mel path: filterbank packed per (N tile of 16 mels, K block of 16 bins) in operand order (256 floats per
    // block, band blocks only, + one all-zero block), per-tile band {klo, khi, first block}
    th::DeviceBuf<float> d_mel_bt;
    th::DeviceBuf<uint32_t> d_mel_band, d_mel_slice;  // + slices of the tile range with ~equal K-group counts
    uint32_t mel_kblocks = 0, mel_ntiles = 0, mel_zero_block = 0, mel_slices = 0;
    th::DeviceBuf<uint32_t> d_mel_rows;  // short rows under narrow filters: the per-mel table of mel_rows_kernel (kernels.h)
    uint32_t mel_rows_groups = 0;
    th::DeviceTable amp_buf, mel_jobs, mel_tile_start;  // amplitude scratch + job tables of mel_mfma_kernel
    size_t amp_zeroed = 0;                               // bytes of amp_buf known to be zero-initialised
    th::DeviceTable chunk_mm;                            // (min, max) per chunk of the wave kernel's last launch
    th::DeviceTable gen_scratch;                         // n_fft >= 32768: frame buffers of the generic kernel (global scratch)
    th::DeviceTable post_jobs;                           // per-channel tile ranges for wave_post_kernel
    // fused mel epilogue: device copy of the mel_fuse.h word table
    th::DeviceBuf<uint32_t> d_mel_fuse;
    uint32_t mel_fuse_words = 0, mel_fuse_slots = 0, mel_fuse_groups = 0;
    // the same epilogue as banded sums, lane = mel (build_mel_band): the default where its table fits; selector 8 keeps the pieces
    th::DeviceBuf<uint32_t> d_mel_bsum;
    uint32_t mel_bsum_words = 0, mel_bsum_groups = 0, mel_bsum_hdr[16] = {};  // (header: offset and taps per group)
    th::DeviceBuf<th::cf32> d_twc;  // n_fft 32768: the combining pass's per-thread constants (kernels_stft_long.hip)
    uint32_t mel_bsum_reach = 0;  // one past the highest amplitude index the banded sums read (MelBandHost::reach)
    // n_fft 4096 mel plans (round 6): the moment form of the filterbank in the FFT kernel's epilogue (build_mel_moments, mel_fuse.h)
    th::DeviceBuf<uint32_t> d_mel_mom;
    uint32_t mel_mom_groups = 0, mel_mom_taps = 0;
    double mel_mom_max_dev = 0.0, mel_mom_max_amp = 0.0;
    th::DeviceTable jobs, tile_start;            // main launch: jobs + first chunk of every job (generic kernel) or the
                                                 // per-chunk (job, first frame) table (wave kernels)
    th::DeviceTable edge_jobs, edge_tile_start;  // boundary frames handed to the generic kernel
    th::StftRoute route;                         // resolve_route (api.hip)
    ~th_plan() {  // (th_plan_destroy, or th_plan_create giving up: the context's device is current)
        for (hipEvent_t e : ev_k0) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_k1) (void)hipEventDestroy(e);
    }
};

namespace th {
// A batch of th_audio_desc tracks on a context's stream (th_audio_stats_dev; th_tm_add_tracks: one per group of tracks).
// loudness_enqueue uploads the tables (synchronously, into `scratch` after the stream has drained, or into a fresh allocation of
// the batch's own) and enqueues the passes; loudness_collect reads the results back once the stream has got that far.
struct LoudnessBatch {
    th_ctx *ctx = nullptr;
    DeviceBuf<unsigned char> d_own;  // the batch's own device memory (NULL: the context's loud_mem)
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
