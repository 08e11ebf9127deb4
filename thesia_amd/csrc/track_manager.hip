// track_manager.hip — C++ mirror of the reference's TrackManager orchestration
// (src-tauri/src/core/mod.rs:33-230) and of the tile commands that read it
// (src-tauri/src/lib.rs:342-389), with audio / f32 dB specs / u16 images resident in HBM.
//
// What is mirrored:  add_tracks → update_specs (mod.rs:62-71,137-164), remove_tracks (:84-100),
// apply_track_list_changes → update_spec_imgs (:102-105,168-230) incl. no_spec_img_ids /
// need_update_all, set_setting (:107-115), set_dB_range (:123-126), set_colormap_length (:128-131),
// the revision bumps the command layer applies around them (lib.rs:192,221,244,265,284), and
// get_waveform_tile / get_spectrogram_tile.
// set_common_normalize / set_common_guard_clipping (lib.rs:287-319 -> track.rs:152-171,329-337 -> audio.rs:50-63,133-179): every
// track keeps its original samples and derives its audio from them on the device (kernels_dynamics.hip).
// What is not: file decoding (the path starts at an in-memory planar f32 channel, audio.rs:65-78).
#include <hip/hip_runtime.h>

#include <cmath>
#include <condition_variable>
#include <cstring>
#include <chrono>
#include <list>
#include <map>
#include <memory>
#include <set>
#include <thread>
#include <atomic>
#include <shared_mutex>
#include <tuple>
#include <vector>

#include "common.h"
#include "context.h"
#include "export_core.h"
#include "figure_plan.h"
#include "flac_core.h"
#include "flac_plan.h"
#include "host_math.h"
#include "kernels.h"
#include "resample_core.h"
#include "tile_cache.h"
#include "track_manager_internal.h"

using namespace th;

namespace {

// One level of a channel's LOD mip pyramid: the whole u16 image resized to ceil(W / 2^lx) x ceil(H / 2^ly) with the
// separable Lanczos3 of resize_spectrogram_tile (render_tiles.rs:354-393).  A LOD tile is then a crop of it.
struct MipLevel {
    uint16_t *d = nullptr;
    uint32_t w = 0, h = 0, pitch = 0;
};

struct Channel {
    float *d_wav = nullptr;      // the AUDIO (Audio::channel): what the spectrogram is made from
    size_t n = 0;
    float *d_draw = nullptr;     // what the waveform is drawn from (channel_for_drawing): d_wav, or the before-clip audio
    float *d_pyr = nullptr;      // resident waveform pyramid of d_draw: every level's (min, max, mean) bins, th_waveform_pyramid_offset
    float *d_orig = nullptr, *d_pyr_orig = nullptr;  // the samples as they were added and their pyramid (the track's pool)
    uint32_t pyr_levels = 0;     // levels 0 .. pyr_levels - 1 (the last one has a single bin)
    DeviceBuf<float> d_spec;
    size_t T = 0, H = 0, spec_pitch = 0;   // rows padded to 128 B (th_pitch_f32)
    DeviceBuf<uint16_t> d_img;
    size_t img_h = 0, img_w = 0, img_pitch = 0;  // rows padded to 128 B (th_pitch_u16)
    std::map<std::pair<uint32_t, uint32_t>, MipLevel> mips;  // (level_x, level_y) != (0, 0): views into d_mips
    DeviceBuf<uint16_t> d_mips;                               // one allocation for every level
    size_t mips_elems = 0;                                    // its size (re-made images of the same shape reuse it)
    float mn = INFINITY, mx = -INFINITY;  // find_min_max of this spec (simd.rs:14-36)
    bool has_spec = false;
};

// Tile requests (lib.rs:342-389) are served concurrently, as the reference's IPC readers are (RwLock::read, lib.rs:345,378;
// thread-local Resizer, render_tiles.rs:366-368): each request borrows a reader slot — its own HIP stream, a device tile
// buffer and a pinned host staging buffer — so that no request waits for another's kernel or copy.
struct ReaderSlot {
    hipStream_t stream = nullptr;
    uint8_t *h_tile = nullptr;  // pinned, mapped into the device's address space
    uint8_t *h_tile_dev = nullptr;  // its device-side address
    bool busy = false;
    // th_tm_get_spectra: job table, f64 partial sums, and the results of batches above h_tile (empty until the first such call;
    // grow-only, freed with the slot)
    th::DeviceTable spec_jobs, spec_part, spec_out;
    // th_tm_get_loudness_meters: the job tables; the results (series energies, sums, peaks) and the filter states behind them
    // (the same rule: empty until the first call, grow-only)
    th::DeviceTable meter_tab, meter_mem;
    // th_tm_export_pcm: two staging buffers (each at most EXPORT_STAGE_MAX bytes: a piece of TH_EXPORT_PIECE_BYTES and its
    // alignment slack), the job table with the channel pointers, the counters, and a second stream with events so that piece p is
    // copied out while piece p + 1 is computed.  Empty until the slot's first export; freed with the slot
    th::DeviceBuf<uint8_t> exp_stage[2];
    size_t exp_stage_cap[2] = {0, 0};
    th::DeviceTable exp_tab, exp_cnt;
    hipStream_t exp_copy = nullptr;
    hipEvent_t exp_done[2] = {nullptr, nullptr}, exp_copied[2] = {nullptr, nullptr};
    // th_tm_export_pcm_at: the planar f32 scratch of one piece (the resampler writes it, the export kernel reads it; at most
    // RESAMPLE_SCRATCH_MAX bytes) and the coefficient table of the last rate pair served.  Empty until the slot first resamples
    th::DeviceBuf<float> rs_scratch, rs_table;
    size_t rs_scratch_cap = 0, rs_table_cap = 0;  // floats
    uint32_t rs_sr_in = 0, rs_sr_out = 0;         // the pair rs_table holds (0: none)
    // th_tm_export_pcm_band: the row of the last filter served (at most TH_BAND_MAX_TAPS floats); the scratch is the resampler's.
    // Empty until the slot first filters
    th::DeviceBuf<float> band_table;
    size_t band_table_cap = 0;  // floats
    uint32_t band_sr = 0;       // the rate and the plan band_table holds (0: none)
    th_band_plan band{};
    // th_tm_export_flac: the subframe slots of one piece (words; at most a piece's bound and a word per unit; with TH_FLAC_STEREO three
    // times the bound, for a stereo block's four units of the side channel's size), the call's table (jobs,
    // channel pointers) and the piece's tables with the call's results (bit lengths, frame offsets, one FlacJobResult per job).  The
    // staging buffers, counters, copy stream and events are the export's.  Empty until the slot's first FLAC call
    th::DeviceBuf<uint32_t> flac_slots;
    size_t flac_slots_cap = 0;  // words
    th::DeviceTable flac_tab, flac_aux;
    // th_tm_render_figures: two staging buffers (each at most TH_FIGURE_PIECE_BYTES), the horizontal pass's intermediate of one piece
    // (u16; at most TH_FIGURE_TMP_BYTES unless one output row alone needs more) and the call's table (tap tables, then the job tables).
    // The copy stream and its events are the export's.  Empty until the slot's first figure
    th::DeviceBuf<uint8_t> fig_stage[2];
    size_t fig_stage_cap[2] = {0, 0};
    th::DeviceBuf<uint16_t> fig_tmp;
    size_t fig_tmp_cap = 0;  // elements
    th::DeviceTable fig_tab;
    // th_tm_get_envelopes / th_tm_render_waveform_figures: the call's table (edge tables, then the job tables), the envelopes of one
    // piece (at most TH_ENVELOPE_PIECE_BYTES), its partial sums (at most TH_ENVELOPE_PART_BYTES unless one request needs more) and,
    // for the lanes, its spans; the lanes' staging buffers, copy stream and events are the figures'.  Empty until the first such call
    th::DeviceTable env_tab, env_out, env_part, lane_span;
    // th_tm_get_formants: the call's table (windows, start points, jobs, the resampler's jobs, channel pointers) and the raw records
    // of two pieces (each at most TH_FORMANT_PIECE_FRAMES x (4 + 3 p) doubles); the analysis signal of a resampled piece lies in the
    // resampler's scratch (at most TH_FORMANT_PIECE_SAMPLES floats of it), the copy stream and its events are the export's.  Empty
    // until the slot's first formant call
    th::DeviceTable fm_tab;
    th::DeviceBuf<double> fm_rec[2];
    size_t fm_rec_cap[2] = {0, 0};  // doubles
    // th_tm_align_tracks: the group values of one piece (n_groups x lags doubles, at most 32 x TH_ALIGN_PIECE_LAGS = 16 MiB), the folded
    // curve of two pieces (each at most TH_ALIGN_PIECE_LAGS doubles) and the group values of the two energies (2 x 32 doubles); under
    // th_tmg the range of a reference that lives in another manager (at most TH_ALIGN_MAX_REF floats) and the pinned host buffer it
    // comes through.  The copy stream and its events are the export's.  Empty until the slot's first alignment
    th::DeviceBuf<double> al_scratch, al_rec[2], al_en;
    size_t al_scratch_cap = 0, al_rec_cap[2] = {0, 0};  // doubles
    th::DeviceBuf<float> al_ref;
    size_t al_ref_cap = 0;  // floats
    float *al_ref_host = nullptr;  // pinned
    size_t al_ref_host_cap = 0;    // floats
};
constexpr size_t TILE_BYTES_MAX = 520 * 520 * 4;  // 512 core + 2 x 4 gutter (render_tiles.rs:15-16); >= 1024 * 12 waveform bins
constexpr size_t MAX_READER_SLOTS = 16;

// Lanczos tap table of one image axis at one LOD level, resident on the device (shared by every channel of that size)
struct AxisTable {
    std::shared_ptr<DeviceBuf<unsigned char>> owner;  // the allocation shared by the tap tables that were made together (freed when the last of them goes): d_blob points into it
    void *d_blob = nullptr;
    uint32_t n_out = 0, max_taps = 0;
    uint32_t span[3] = {0, 0, 0};  // LodAxis::span
    size_t bytes = 0;
};

struct Track {
    uint32_t sr = 0;
    std::vector<Channel> ch;
    // ONE device allocation for the samples and waveform pyramids of all channels (round 6: two hipMalloc per channel were 0.7 ms
    // of a 32-track add); Channel::d_wav / d_pyr are views into it and live exactly as long as the track
    DeviceBuf<float> d_pool;
    th_audio_stats stats{};       // AudioStats (StatCalculator::calc, dynamics/stats.rs:56-86) of the audio
    th_audio_stats orig_stats{};  // ... of the samples as they were added: what the normalise gain is computed from
    // The audio derived from the original under the common normalise target and clip guard (AudioTrack::apply_gain).  d_dyn == NULL:
    // the audio IS the original (gain 1 or not finite) and nothing below is held.  One allocation: per channel the audio, in Clip mode
    // the before-clip audio, and the pyramid of what is drawn; then the limiter's gain sequence.
    DeviceBuf<float> d_dyn;
    float norm_gain = 1.0f;
    int guard_result = TH_GUARD_RESULT_GLOBAL_GAIN;
    float global_gain = 1.0f;
    float *d_gain = nullptr;    // GainSequence: n gains (a view into d_dyn), or NULL when the limiter had nothing to do (all ones)
    bool gain_below_one = false;
    std::vector<th_guard_clip_stats> guard_stats;  // Audio::guard_clip_stats: one per channel, or one for a gain sequence
};

using PlanKey = std::tuple<uint32_t, size_t, size_t, size_t, int>;  // sr, win, hop, n_fft, scale

}  // namespace

struct th_tm {
    th_ctx *ctx = nullptr;
    // SpecSetting::new — spectrogram.rs:47-54
    double win_ms = 40.;
    uint32_t t_overlap = 4, f_overlap = 1;
    int freq_scale = TH_FREQ_MEL;
    // TrackManager::new — core/mod.rs:46-60
    float max_dB = -INFINITY, min_dB = INFINITY;
    uint32_t max_sr = 0;
    float dB_range = 100.f;
    uint32_t colormap_length = 258;
    std::vector<size_t> no_spec_img_ids;
    std::map<size_t, Track> tracks;
    std::map<PlanKey, th_plan *> plans;  // SpectrogramAnalyzer caches, spectrogram.rs:101-105
    // RenderTileCache state that the tile encoders need — render_tiles.rs:68-96
    std::vector<uint8_t> colormap_rgba{0, 0, 0, 255, 255, 255, 255, 255};
    DeviceBuf<uint8_t> d_colormap;  // device copy of colormap_rgba (uploaded when it changes, not per tile request)
    th_tile_cache cache{th_tile_cache::DEFAULT_BUDGET};  // revisions + waveform-tile LRU, render_tiles.rs:51-230
    // Writers (every mutator) take `rw` exclusively, tile readers share it — the reference's RwLock<TrackManager>.
    // A mutator leaves the context stream idle before it releases the lock, so readers never see half-made images.
    mutable std::shared_mutex rw;
    std::mutex slot_mu;
    std::condition_variable slot_cv;
    std::vector<std::unique_ptr<ReaderSlot>> slots;
    // 0: LOD > 0 tiles are crops of the pre-built mip pyramid (default); 1: resampled per request from the level-0 image
    // (the reference's own flow; kept as the comparison path).  Levels the pyramid does not hold always use 1.
    int lod_source = 0;
    // TrackList::new — track.rs:203-204
    int norm_kind = TH_NORM_OFF;
    float norm_target = 0.0f;
    int guard_mode = TH_GUARD_REDUCE_GLOBAL_LEVEL;
    std::map<std::pair<uint32_t, uint32_t>, AxisTable> axis_tabs;  // (source length, level) -> taps
    th::DeviceTable mip_jobs;                                       // job table of the batched mip-pyramid passes
    th::DeviceTable mip_scratch;                                    // transposed images of one chunk of the batch
    std::list<std::vector<unsigned char>> axis_staging;             // host copies of tap tables whose upload may still be in flight (cleared by writer_done)
    hipStream_t copy_stream = nullptr;                              // th_tm_add_tracks: uploads of group g + 1 beside the kernels of group g
    hipEvent_t copy_ev = nullptr;
    // update_spec_imgs records img_ev behind the quantiser and mips_ev behind the last pass of the mip pyramids.  The two
    // interactive mutators (apply_track_list_changes, set_dB_range) return when the IMAGES are made and leave the pyramids — an
    // acceleration structure of this library for LOD > 0 tiles, 2.7 of the 4 ms of a 32-track update; the reference has none —
    // building on the context stream: a tile reader that crops a mip level makes its own stream wait for mips_ev (on the
    // device, not on the host), level-0 tiles do not wait at all, and everything else that touches images or levels runs on
    // the context stream, i.e. behind the build anyway.
    hipEvent_t img_ev = nullptr, mips_ev = nullptr;
    bool img_ev_recorded = false;
    uint64_t stat_tiles_served = 0;
    // th_tm_get_spectrogram_tiles: pinned staging for callers whose buffer the GPU cannot write directly (one batch at a time)
    std::mutex batch_mu;
    void *batch_stage = nullptr, *batch_stage_dev = nullptr;
    size_t batch_stage_cap = 0;

    void invalidate_waveform() { cache.invalidate_waveform(); }
    void invalidate_spectrogram() { cache.invalidate_spectrogram(); }
    void invalidate_all() { cache.invalidate_all(); }
    uint64_t waveform_revision() const {
        std::lock_guard<std::mutex> lk(cache.mu);
        return cache.waveform_revision;
    }
    uint64_t spectrogram_revision() const {
        std::lock_guard<std::mutex> lk(cache.mu);
        return cache.spectrogram_revision;
    }
};

namespace {

// th_tm as the manager of a batched reader (batched_reader.h): one owner.  The default colormap is uploaded before the shared lock
// is taken (ensure_colormap takes the lock exclusively when it has to)
struct TmReaders {
    static constexpr bool single_owner = true;
    th_tm *tm;
    bool null() const { return !tm; }
    int before_lock(bool colormap) const { return colormap ? tmi::ensure_colormap(tm) : TH_OK; }
    std::shared_lock<std::shared_mutex> lock() const { return std::shared_lock<std::shared_mutex>(tm->rw); }
    uint64_t revision(br::Revision which) const {
        return which == br::Revision::waveform ? tm->waveform_revision() : tm->spectrogram_revision();
    }
    th_tm *owner() const { return tm; }
};

void free_mips(Channel &c) {
    c.d_mips.reset();
    c.mips_elems = 0;
    c.mips.clear();
}

// DeviceBuf::reset() with the failure reported (update_spec_imgs, upload_colormap)
template <class T>
int free_checked(DeviceBuf<T> &b) {
    TH_HIP(hipFree(b.ptr));
    b.ptr = nullptr;
    return TH_OK;
}

struct Setting {
    double win_ms;
    uint32_t t_overlap, f_overlap;
    int freq_scale;
};
Setting setting_of(const th_tm *tm) { return Setting{tm->win_ms, tm->t_overlap, tm->f_overlap, tm->freq_scale}; }

PlanKey plan_key(const Setting &st, uint32_t sr) {
    size_t hop, win, n_fft;
    calc_framing_params(st.win_ms, st.t_overlap, st.f_overlap, sr, &hop, &win, &n_fft);
    return PlanKey{sr, win, hop, n_fft, st.freq_scale};
}

// the plan of (setting, sr): the cached one, or a new one recorded in `created` (the caller commits or destroys those)
int get_plan(th_tm *tm, const Setting &st, uint32_t sr, std::map<PlanKey, th_plan *> &created, th_plan **out) {
    const PlanKey key = plan_key(st, sr);
    auto it = tm->plans.find(key);
    if (it != tm->plans.end()) {
        *out = it->second;
        return TH_OK;
    }
    auto ic = created.find(key);
    if (ic != created.end()) {
        *out = ic->second;
        return TH_OK;
    }
    th_plan *p = nullptr;
    int rc = th_plan_create(tm->ctx, sr, std::get<1>(key), std::get<2>(key), std::get<3>(key), st.freq_scale, 0, &p);
    if (rc != TH_OK) return rc;
    created[key] = p;
    *out = p;
    return TH_OK;
}

// SpectrogramAnalyzer::retain — spectrogram.rs:156-185: drop plans no resident track needs
void retain_plans(th_tm *tm) {
    std::set<PlanKey> need;
    const Setting st = setting_of(tm);
    for (auto &kv : tm->tracks) need.insert(plan_key(st, kv.second.sr));
    for (auto it = tm->plans.begin(); it != tm->plans.end();) {
        if (!need.count(it->first)) {
            th_plan_destroy(it->second);
            it = tm->plans.erase(it);
        } else {
            ++it;
        }
    }
}

// A freshly computed spec, not yet attached to its channel: (track id, channel index) is looked up when it is attached
struct NewSpec {
    size_t id = 0;
    uint32_t ch = 0;
    DeviceBuf<float> d_spec;
    size_t T = 0, H = 0, pitch = 0;
    float mn = INFINITY, mx = -INFINITY;
};
// What a spec is computed from: n samples at d_wav, which need not be the audio of a resident channel (yet)
struct SpecInput {
    size_t id;
    uint32_t ch, sr;
    const float *d_wav;
    size_t n;
};

// TrackManager::update_specs — core/mod.rs:137-164: one batched launch per plan, INTO FRESH BUFFERS.  Nothing the
// manager owns is touched: the caller attaches the results (tmi::commit) once every launch has succeeded, so a
// failure (unsupported n_fft, out of memory) leaves settings, specs and has_spec exactly as they were.
// pending != NULL: the per-channel (min, max) pairs stay on the device (entries appended to *pending) and NOTHING here waits for
// the launches — the caller synchronises once and calls finish_specs (th_tm_add_tracks launches group after group this way,
// beside the next group's upload)
struct PendingMinMax {
    DeviceBuf<float> d_mm;
    size_t first = 0, count = 0;
};
int finish_specs(std::vector<PendingMinMax> &pending, std::vector<NewSpec> *out) {
    for (PendingMinMax &pm : pending) {
        std::vector<float> mm(2 * pm.count);
        TH_HIP(hipMemcpy(mm.data(), pm.d_mm, mm.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < pm.count; i++) {
            (*out)[pm.first + i].mn = mm[2 * i];
            (*out)[pm.first + i].mx = mm[2 * i + 1];
        }
    }
    pending.clear();
    return TH_OK;
}
int compute_specs(th_tm *tm, const Setting &st, const std::vector<SpecInput> &chans, std::map<PlanKey, th_plan *> &created,
                  std::vector<NewSpec> *out, std::vector<PendingMinMax> *pending = nullptr) {
    th_ctx *c = tm->ctx;
    std::map<th_plan *, std::vector<const SpecInput *>> groups;
    for (const SpecInput &in : chans) {
        th_plan *p = nullptr;
        TH_CHECK(get_plan(tm, st, in.sr, created, &p));
        groups[p].push_back(&in);
    }
    for (auto &kv : groups) {
        th_plan *p = kv.first;
        const std::vector<const SpecInput *> &ins = kv.second;
        std::vector<th_chan_desc> descs(ins.size());
        PendingMinMax pm;
        pm.first = out->size();
        pm.count = ins.size();
        for (size_t i = 0; i < ins.size(); i++) {
            NewSpec ns;
            ns.id = ins[i]->id;
            ns.ch = ins[i]->ch;
            ns.T = stft_n_frames(ins[i]->n, p->g.win, p->g.hop);
            ns.H = p->g.height;
            ns.pitch = th_pitch_f32(ns.H);
            TH_HIP(ns.d_spec.alloc(std::max<size_t>(1, ns.T * ns.pitch) * sizeof(float)));
            descs[i] = th_chan_desc{ins[i]->d_wav, ns.d_spec, ins[i]->n, ns.T, ns.pitch};
            out->push_back(std::move(ns));
        }
        TH_HIP(pm.d_mm.alloc(2 * ins.size() * sizeof(float)));
        float *const d_mm = pm.d_mm;
        if (pending != nullptr) {
            pending->push_back(std::move(pm));  // (before the launch: it has to outlive it on any outcome)
            TH_CHECK(th_calc_spec_batch_dev(p, descs.data(), descs.size(), d_mm));
            continue;
        }
        TH_CHECK(th_calc_spec_batch_dev(p, descs.data(), descs.size(), d_mm));
        std::vector<float> mm(2 * ins.size());
        TH_HIP(hipMemcpyAsync(mm.data(), d_mm, mm.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        TH_HIP(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < ins.size(); i++) {
            (*out)[pm.first + i].mn = mm[2 * i];
            (*out)[pm.first + i].mx = mm[2 * i + 1];
        }
    }
    return TH_OK;
}

// ---------------------------------------------------------------------------------------------- LOD mip pyramid
// (levels beyond these are resampled per request: the frontend's level = floor(log2(source pixels per screen pixel)),
// AudioTrackViewport.tsx:91,406,439 — rows are hundreds of pixels high, so level_y rarely exceeds 2)
constexpr uint32_t MIP_MAX_LX = 12, MIP_MAX_LY = 3, MIP_MIN_DIM = 16;
constexpr uint32_t PYR_FIRST = 2;  // first materialised level of the resident waveform pyramids (levels 0, 1: from the samples)

// The host half of a tap table: Lanczos3 taps of the whole axis as the crop box (origin 0, extent n_in:
// resize_spectrogram_tile with the full image as the crop), packed as LodAxis reads it, + the span of R = 8, 4, 2 outputs
struct AxisHostTable {
    std::vector<unsigned char> blob;
    uint32_t n_out = 0, max_taps = 0, span[3] = {0, 0, 0};
};
void build_axis_host(uint32_t n_in, uint32_t level, AxisHostTable &h) {
    const size_t n_out = (n_in + ((size_t)1 << level) - 1) >> level;
    LodAxisHost ax;
    build_lod_axis(0.0, (double)n_in, n_out, 0, (long)n_in, ax);
    h.blob.resize(ax.blob_bytes(n_out));
    ax.pack(h.blob.data(), n_out);
    h.n_out = (uint32_t)n_out;
    h.max_taps = ax.max_taps;
    for (int k = 0; k < 3; k++) {  // source rows under the tap windows of R = 8, 4, 2 consecutive outputs
        const size_t r = (size_t)8 >> k;
        int64_t span = 0;
        for (size_t o0 = 0; o0 < n_out; o0 += r) {
            int64_t hi = 0;
            for (size_t o = o0; o < std::min(n_out, o0 + r); o++) hi = std::max<int64_t>(hi, (int64_t)ax.start[o] + ax.count[o]);
            span = std::max(span, hi - (int64_t)ax.start[o0]);
        }
        h.span[k] = (uint32_t)span;
    }
}

// Make every tap table in `keys` that is not resident yet: the host halves side by side on a few threads (a table is ~6 taps per
// SOURCE element whatever the level — 17 k sinc evaluations for a 30 s track's x axis — and a batch of tracks needs a dozen
// levels per distinct length: 2.1 of the 3.7 ms an apply_track_list_changes took for 32 equal tracks, and proportionally more
// for tracks of different lengths), then the uploads, stream-ordered in front of the passes that read them.  The blobs stay
// alive in tm->axis_staging until the writer's final synchronisation (writer_done): nothing waits per table.
int make_axis_tables(th_tm *tm, const std::set<std::pair<uint32_t, uint32_t>> &keys) {
    std::vector<std::pair<uint32_t, uint32_t>> todo;
    for (auto &k : keys)
        if (!tm->axis_tabs.count(k)) todo.push_back(k);
    if (todo.empty()) return TH_OK;
    std::vector<AxisHostTable> host(todo.size());
    {
        const size_t n_thr = std::min<size_t>(todo.size(), std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
        std::atomic<size_t> next{0};
        std::atomic<bool> failed{false};
        auto work = [&]() {
            try {
                for (size_t i = next.fetch_add(1); i < todo.size(); i = next.fetch_add(1)) build_axis_host(todo[i].first, todo[i].second, host[i]);
            } catch (...) {
                failed = true;
            }
        };
        std::vector<std::thread> thr;
        try {
            for (size_t i = 1; i < n_thr; i++) thr.emplace_back(work);
        } catch (...) {  // (no more threads: the ones that started and this one do all of it)
        }
        work();
        for (auto &t : thr) t.join();
        if (failed) return th::fail(TH_ERR_OOM, "host allocation failed while building LOD tap tables");
    }
    // ONE allocation and ONE upload for the tables of this call (fifteen small pageable copies were 0.3 ms of host time)
    std::vector<size_t> at(todo.size());
    size_t total = 0;
    for (size_t i = 0; i < todo.size(); i++) {
        at[i] = total;
        total += (host[i].blob.size() + 255) / 256 * 256;
    }
    tm->axis_staging.emplace_back(total);
    std::vector<unsigned char> &stage = tm->axis_staging.back();
    for (size_t i = 0; i < todo.size(); i++) std::memcpy(stage.data() + at[i], host[i].blob.data(), host[i].blob.size());
    auto blk = std::make_shared<DeviceBuf<unsigned char>>();
    TH_HIP(blk->alloc(total));
    const hipError_t e = hipMemcpyAsync(blk->get(), stage.data(), total, hipMemcpyHostToDevice, tm->ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(tm->ctx->stream);
        TH_HIP(e);
    }
    for (size_t i = 0; i < todo.size(); i++) {
        AxisTable t;
        t.owner = blk;
        t.d_blob = blk->get() + at[i];
        t.n_out = host[i].n_out;
        t.max_taps = host[i].max_taps;
        t.bytes = host[i].blob.size();
        for (int k = 0; k < 3; k++) t.span[k] = host[i].span[k];
        tm->axis_tabs.emplace(todo[i], t);
    }
    return TH_OK;
}

int axis_table(th_tm *tm, uint32_t n_in, uint32_t level, AxisTable **out) {
    const auto key = std::make_pair(n_in, level);
    auto it = tm->axis_tabs.find(key);
    if (it == tm->axis_tabs.end()) {
        const int rc = make_axis_tables(tm, {key});
        if (rc != TH_OK) return rc;
        it = tm->axis_tabs.find(key);
    }
    *out = &it->second;
    return TH_OK;
}

LodAxis axis_view(const AxisTable &t) {
    unsigned char *base = static_cast<unsigned char *>(t.d_blob);
    LodAxis a;
    a.start = reinterpret_cast<const int32_t *>(base);
    a.count = reinterpret_cast<const int32_t *>(base + (size_t)t.n_out * 4);
    a.wsum = reinterpret_cast<const double *>(base + (size_t)t.n_out * 8);
    a.w = reinterpret_cast<const double *>(base + (size_t)t.n_out * 16);
    a.n_out = t.n_out;
    a.max_taps = t.max_taps;
    for (int k = 0; k < 3; k++) a.span[k] = t.span[k];
    return a;
}

// Tap tables are keyed by (axis length, level); the x-axis length is a track's frame count, i.e. different for practically
// every track.  Drop the tables no resident image refers to (they survived remove_track / set_setting, ~48 W bytes
// per level each, so a long session that adds and removes tracks grew device memory without bound).  hipFree waits for the
// device, so a table still read by a launched pass is safe.
void prune_axis_tabs(th_tm *tm) {
    std::set<std::pair<uint32_t, uint32_t>> live;
    for (auto &kv : tm->tracks)
        for (Channel &ch : kv.second.ch)
            for (auto &m : ch.mips) {
                if (m.first.first) live.insert({(uint32_t)ch.img_w, m.first.first});
                if (m.first.second) live.insert({(uint32_t)ch.img_h, m.first.second});
            }
    for (auto it = tm->axis_tabs.begin(); it != tm->axis_tabs.end();) {
        if (live.count(it->first)) {
            ++it;
        } else {
            it = tm->axis_tabs.erase(it);  // (its block goes with the last table made beside it)
        }
    }
}

// Build every (lx, ly) level of the images of `chans`: horizontal pass from level 0 for each lx, vertical pass from
// (lx, 0) for each ly — the same order and the same one-rounding-per-pass as the per-request resize.  Images of one shape
// go through every pass together (grid z = image): a launch per level, not per level and channel (32 tracks: ~1000 launches
// of a few microseconds of work each took 27 ms of the 28 ms an apply_track_list_changes spent behind the STFT).
int build_mips(th_tm *tm, const std::vector<Channel *> &chans) {
    hipStream_t s = tm->ctx->stream;
    if (tm->lod_source == 1) {  // per-request route selected: no pyramid is kept (2.75x the image memory, and the passes)
        for (Channel *ch : chans) free_mips(*ch);
        return TH_OK;
    }
    struct Shape {
        uint32_t w, h, pitch;
        bool operator<(const Shape &o) const { return std::tie(w, h, pitch) < std::tie(o.w, o.h, o.pitch); }
    };
    std::map<Shape, std::vector<Channel *>> groups;
    for (Channel *ch : chans) {
        if (!ch->d_img || !ch->img_w || !ch->img_h) {
            free_mips(*ch);
            continue;
        }
        ch->mips.clear();
        const uint32_t W = (uint32_t)ch->img_w, Hh = (uint32_t)ch->img_h;
        uint32_t Lx = 0, Ly = 0;
        while (Lx < MIP_MAX_LX && ((W + (2u << Lx) - 1) >> (Lx + 1)) >= MIP_MIN_DIM) Lx++;
        while (Ly < MIP_MAX_LY && ((Hh + (2u << Ly) - 1) >> (Ly + 1)) >= MIP_MIN_DIM) Ly++;
        // shapes first, then ONE allocation for all levels (a hipMalloc per level cost more than the resampling)
        size_t total = 0;
        for (uint32_t lx = 0; lx <= Lx; lx++)
            for (uint32_t ly = 0; ly <= Ly; ly++) {
                if (!lx && !ly) continue;
                MipLevel m;
                m.w = (W + (1u << lx) - 1) >> lx;
                m.h = (Hh + (1u << ly) - 1) >> ly;
                m.pitch = (uint32_t)th_pitch_u16(m.w);
                m.d = reinterpret_cast<uint16_t *>(total);  // offset for now
                total += ((size_t)m.h * m.pitch + 127) / 128 * 128;
                ch->mips[{lx, ly}] = m;
            }
        if (!total) {
            free_mips(*ch);
            continue;
        }
        // (a dB-range or colour-map change re-makes every image at its old shape: keep the allocation — hipFree
        // synchronises the device and a hipMalloc of this size takes longer than the resampling)
        if (!ch->d_mips || ch->mips_elems != total) {
            const std::map<std::pair<uint32_t, uint32_t>, MipLevel> views = ch->mips;
            free_mips(*ch);
            TH_HIP(ch->d_mips.alloc(total * sizeof(uint16_t)));
            ch->mips = views;
            ch->mips_elems = total;
        }
        for (auto &kv : ch->mips) kv.second.d = ch->d_mips.get() + reinterpret_cast<size_t>(kv.second.d);
        groups[Shape{W, Hh, (uint32_t)ch->img_pitch}].push_back(ch);
    }
    // One job table for all launches (uploaded once), then the launches in dependency order per shape.  The horizontal
    // pass runs as transpose -> vertical pass along x -> transpose back (kernels_image.hip: same taps, same order, same
    // rounding: bit-identical to lod_hpass_kernel); the transposed level-0 image and the transposed result of one level
    // live in a scratch buffer of the manager, MIP_CHUNK images at a time.
    enum Kind { TRANSPOSE, VPASS };
    struct Launch {
        Kind kind;
        uint32_t level, first, count, n_in, a, b;  // TRANSPOSE: a x b image;  VPASS: axis of length n_in at `level`, dw = a
    };
    constexpr size_t MIP_CHUNK = 32;
    std::vector<LodPassJob> jobs;
    std::vector<Launch> launches;
    size_t scratch_elems = 0;
    for (auto &g : groups) {
        const uint32_t W = g.first.w, Hh = g.first.h;
        uint32_t Lx = 0;
        for (auto &kv : g.second[0]->mips) Lx = std::max(Lx, kv.first.first);
        if (Lx == 0) continue;
        const size_t pT = th_pitch_u16(Hh);  // row pitch of the transposed images (rows = x, columns = y)
        const size_t per_img = (size_t)W * pT + (size_t)((W + 1) / 2) * pT;
        scratch_elems = std::max(scratch_elems, per_img * std::min(MIP_CHUNK, g.second.size()));
    }
    if (scratch_elems) {
        int rc = tm->mip_scratch.ensure(scratch_elems * sizeof(uint16_t));
        if (rc != TH_OK) return rc;
    }
    uint16_t *const scratch = static_cast<uint16_t *>(tm->mip_scratch.dptr);
    for (auto &g : groups) {
        const uint32_t W = g.first.w, Hh = g.first.h;
        uint32_t Lx = 0, Ly = 0;
        for (auto &kv : g.second[0]->mips) {
            Lx = std::max(Lx, kv.first.first);
            Ly = std::max(Ly, kv.first.second);
        }
        const uint32_t pT = (uint32_t)th_pitch_u16(Hh);
        const size_t t0_elems = (size_t)W * pT, per_img = t0_elems + (size_t)((W + 1) / 2) * pT;
        for (size_t c0 = 0; c0 < g.second.size(); c0 += MIP_CHUNK) {
            const std::vector<Channel *> cs(g.second.begin() + c0, g.second.begin() + std::min(g.second.size(), c0 + MIP_CHUNK));
            const uint32_t nc = (uint32_t)cs.size();
            auto t0 = [&](size_t i) { return scratch + i * per_img; };            // transposed level 0: W rows of Hh
            auto tl = [&](size_t i) { return scratch + i * per_img + t0_elems; };  // transposed level lx: w_lx rows of Hh
            if (Lx > 0) {
                launches.push_back(Launch{TRANSPOSE, 0, (uint32_t)jobs.size(), nc, 0, W, Hh});
                for (size_t i = 0; i < nc; i++) jobs.push_back(LodPassJob{cs[i]->d_img, t0(i), (uint32_t)cs[i]->img_pitch, pT});
            }
            for (uint32_t lx = 0; lx <= Lx; lx++) {
                if (lx > 0) {
                    const uint32_t wl = cs[0]->mips[{lx, 0u}].w;
                    launches.push_back(Launch{VPASS, lx, (uint32_t)jobs.size(), nc, W, Hh, 0});  // along x, Hh columns
                    for (size_t i = 0; i < nc; i++) jobs.push_back(LodPassJob{t0(i), tl(i), pT, pT});
                    launches.push_back(Launch{TRANSPOSE, 0, (uint32_t)jobs.size(), nc, 0, Hh, wl});  // (Hh x wl)^T -> wl x Hh image
                    for (size_t i = 0; i < nc; i++) {
                        const MipLevel &m = cs[i]->mips[{lx, 0u}];
                        jobs.push_back(LodPassJob{tl(i), m.d, pT, m.pitch});
                    }
                }
                for (uint32_t ly = 1; ly <= Ly; ly++) {
                    const uint32_t src_w = lx > 0 ? cs[0]->mips[{lx, 0u}].w : W;
                    launches.push_back(Launch{VPASS, ly, (uint32_t)jobs.size(), nc, Hh, src_w, 0});
                    for (Channel *ch : cs) {
                        const MipLevel &m = ch->mips[{lx, ly}];
                        if (lx > 0) {
                            const MipLevel &src = ch->mips[{lx, 0u}];
                            jobs.push_back(LodPassJob{src.d, m.d, src.pitch, m.pitch});
                        } else {
                            jobs.push_back(LodPassJob{ch->d_img, m.d, (uint32_t)ch->img_pitch, m.pitch});
                        }
                    }
                }
            }
        }
    }
    if (launches.empty()) return TH_OK;
    const bool prof = getenv("TH_TM_PROF") != nullptr;
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tb0 = now();
    double t_axis = 0.0;
    int rc = tm->mip_jobs.upload(s, jobs.data(), jobs.size() * sizeof(LodPassJob));
    if (rc != TH_OK) return rc;
    const LodPassJob *dj = static_cast<const LodPassJob *>(tm->mip_jobs.dptr);
    {   // every tap table the passes below read, made together (in parallel on the host) before the first launch
        std::set<std::pair<uint32_t, uint32_t>> keys;
        for (const Launch &l : launches)
            if (l.kind == VPASS) keys.insert({l.n_in, l.level});
        const double ta_ = now();
        rc = make_axis_tables(tm, keys);
        t_axis += now() - ta_;
        if (rc != TH_OK) return rc;
    }
    for (const Launch &l : launches) {
        if (l.kind == TRANSPOSE) {
            // a x b: the SOURCE has b rows of a elements (dst[x][y] = src[y][x], x < a, y < b)
            TH_HIP(launch_transpose_u16_batch(dj + l.first, l.count, l.a, l.b, s));
        } else {
            AxisTable *t = nullptr;
            const double ta_ = now();
            rc = axis_table(tm, l.n_in, l.level, &t);
            t_axis += now() - ta_;
            if (rc != TH_OK) return rc;
            TH_HIP(launch_lod_vpass_batch(dj + l.first, l.count, axis_view(*t), l.a, s));
        }
    }
    if (prof) fprintf(stderr, "build_mips prof: %zu launches %.2f ms of which axis tables %.2f\n", launches.size(), now() - tb0, t_axis);
    return TH_OK;
}

// TrackManager::update_spec_imgs — core/mod.rs:168-230.  `global` (th_tmg): the range and max_sr of the tracks of every slot,
// folded by the caller, in place of this manager's own
int update_spec_imgs(th_tm *tm, bool force_update_all, std::vector<size_t> *updated, const tmi::DbRange *global = nullptr) {
    float mn = INFINITY, mx = -INFINITY;
    if (global) {
        mn = global->min_dB;
        mx = global->max_dB;
    } else {
        std::vector<float> mins, maxs;
        for (auto &kv : tm->tracks)
            for (Channel &ch : kv.second.ch)
                if (ch.has_spec) {
                    mins.push_back(ch.mn);
                    maxs.push_back(ch.mx);
                }
        global_db_range(mins.data(), maxs.data(), mins.size(), tm->dB_range, &mn, &mx);  // :169-180
    }
    bool need_update_all = force_update_all;
    if (!(tm->max_dB == mx)) {  // `!=` on f32 (NaN never equal)  :182-185
        tm->max_dB = mx;
        need_update_all = true;
    }
    if (!(tm->min_dB == mn)) {
        tm->min_dB = mn;
        need_update_all = true;
    }
    uint32_t max_sr = 0;  // TrackList::max_sr, track.rs:371-376
    for (auto &kv : tm->tracks) max_sr = std::max(max_sr, kv.second.sr);
    if (global) max_sr = global->max_sr;
    if (tm->max_sr != max_sr) {
        tm->max_sr = max_sr;
        need_update_all = true;
    }
    std::set<size_t> ids;
    if (need_update_all) {
        tm->no_spec_img_ids.clear();
        for (auto &kv : tm->tracks) ids.insert(kv.first);
    } else {
        ids.insert(tm->no_spec_img_ids.begin(), tm->no_spec_img_ids.end());
        tm->no_spec_img_ids.clear();
    }
    updated->assign(ids.begin(), ids.end());
    if (ids.empty()) return TH_OK;

    if (need_update_all)  // spec_imgs.clear()  :224-226
        for (auto &kv : tm->tracks)
            for (Channel &ch : kv.second.ch)
                if (ch.d_img && !ids.count(kv.first)) {
                    TH_CHECK(free_checked(ch.d_img));
                    ch.img_h = ch.img_w = 0;
                    free_mips(ch);
                }
    std::vector<th_img_desc> descs;
    std::vector<Channel *> made;
    const bool prof = getenv("TH_TM_PROF") != nullptr;
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tq0 = now();
    for (size_t id : ids) {
        auto it = tm->tracks.find(id);
        if (it == tm->tracks.end()) continue;  // filter over specs: ids without a spec are skipped
        for (Channel &ch : it->second.ch) {
            if (!ch.has_spec) continue;
            size_t i0, i1;
            hz_range_to_idx(tm->freq_scale, 0.f, float(tm->max_sr) / 2.f, it->second.sr, ch.H, &i0, &i1);  // :210-214
            const size_t h = i1 - i0, w = ch.T;
            if (ch.d_img && (ch.img_h != h || ch.img_w != w)) TH_CHECK(free_checked(ch.d_img));
            const size_t ipitch = th_pitch_u16(w);
            if (!ch.d_img) TH_HIP(ch.d_img.alloc(std::max<size_t>(1, h * ipitch) * sizeof(uint16_t)));
            ch.img_h = h;
            ch.img_w = w;
            ch.img_pitch = ipitch;
            descs.push_back(th_img_desc{ch.d_spec, ch.d_img, ch.T, ch.H, i0, i1, ch.spec_pitch, ipitch});
            made.push_back(&ch);
        }
    }
    const double tq1 = now();
    int rc = th_spec_to_img_batch_dev(tm->ctx, descs.data(), descs.size(), tm->min_dB, tm->max_dB, tm->colormap_length);
    if (rc == TH_OK) {
        TH_HIP(hipEventRecord(tm->img_ev, tm->ctx->stream));
        tm->img_ev_recorded = true;
    }
    const double tq2 = now();
    // the LOD mip pyramid of every image that was just re-made (render_tiles.rs:290-313,354-393)
    if (rc == TH_OK) rc = build_mips(tm, made);
    if (rc == TH_OK) TH_HIP(hipEventRecord(tm->mips_ev, tm->ctx->stream));
    if (prof) {
        const double tq3 = now();
        (void)hipStreamSynchronize(tm->ctx->stream);
        fprintf(stderr, "update_spec_imgs prof: image allocations %.2f ms, quantise launch %.2f, build_mips (host side) %.2f, drain %.2f\n", tq1 - tq0, tq2 - tq1,
                tq3 - tq2, now() - tq3);
    }
    if (rc != TH_OK) {
        // Not failure-atomic otherwise: the images above are already re-quantised, so a pyramid that was only
        // partly rebuilt would serve pixels of the old dB range under the new revision.  Without levels every LOD request
        // falls back to the per-request resize of the (new) level-0 image.
        (void)hipStreamSynchronize(tm->ctx->stream);
        for (Channel *ch : made) free_mips(*ch);
    }
    prune_axis_tabs(tm);
    return rc;
}

Channel *find_channel(th_tm *tm, size_t id, uint32_t ch) {
    auto it = tm->tracks.find(id);
    if (it == tm->tracks.end() || ch >= it->second.ch.size()) return nullptr;
    return &it->second.ch[ch];
}

// ---------------------------------------------------------------------------------------------- reader slots
struct SlotLease {
    th_tm *tm;
    ReaderSlot *slot;
    ~SlotLease() {
        if (slot) {
            {
                std::lock_guard<std::mutex> lk(tm->slot_mu);
                slot->busy = false;
            }
            tm->slot_cv.notify_one();
        }
    }
};

int acquire_slot(th_tm *tm, ReaderSlot **out) {
    std::unique_lock<std::mutex> lk(tm->slot_mu);
    for (;;) {
        for (auto &sp : tm->slots)
            if (!sp->busy) {
                sp->busy = true;
                *out = sp.get();
                return TH_OK;
            }
        if (tm->slots.size() < MAX_READER_SLOTS) {
            std::unique_ptr<ReaderSlot> sl(new ReaderSlot());
            hipError_t e = hipStreamCreateWithFlags(&sl->stream, hipStreamNonBlocking);
            if (e == hipSuccess) e = hipHostMalloc((void **)&sl->h_tile, TILE_BYTES_MAX, hipHostMallocMapped);
            if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&sl->h_tile_dev, sl->h_tile, 0);
            if (e != hipSuccess) {
                if (sl->h_tile) (void)hipHostFree(sl->h_tile);
                if (sl->stream) (void)hipStreamDestroy(sl->stream);
                if (tm->slots.empty()) TH_HIP(e);
                // out of resources with slots in use: wait for one of those instead
            } else {
                sl->busy = true;
                *out = sl.get();
                tm->slots.push_back(std::move(sl));
                return TH_OK;
            }
        }
        tm->slot_cv.wait(lk);
    }
}


// a mutator's last act before it releases the write lock: readers use their own streams
int writer_done(th_tm *tm, int rc) {
    hipError_t e = hipStreamSynchronize(tm->ctx->stream);
    tm->axis_staging.clear();  // (every upload from these host copies has completed)
    tm->img_ev_recorded = false;
    if (rc == TH_OK && e != hipSuccess) TH_HIP(e);
    return rc;
}

// the same for the mutators that only re-make images (see th_tm::img_ev): wait for the quantiser, not for the mip pyramids behind
// it.  The tap tables' host copies (axis_staging) stay until a later mutator has drained the stream.
int writer_done_images(th_tm *tm, int rc) {
    if (rc != TH_OK || !tm->img_ev_recorded || tm->lod_source != 0) return writer_done(tm, rc);
    const hipError_t e = hipEventSynchronize(tm->img_ev);
    tm->img_ev_recorded = false;
    if (e != hipSuccess) TH_HIP(e);
    return TH_OK;
}

}  // namespace

TH_API int th_tm_create(th_ctx *c, th_tm **out) {
    TH_TRY
    TH_REQUIRE(c && out, "NULL argument");
    std::unique_ptr<th_tm> tm(new th_tm());
    tm->ctx = c;
    // the manager's own device objects up front (a stream takes milliseconds to create: not inside the first add_tracks)
    TH_HIP(hipSetDevice(c->device));
    hipError_t e = hipStreamCreateWithFlags(&tm->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&tm->copy_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&tm->img_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&tm->mips_ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (tm->mips_ev) (void)hipEventDestroy(tm->mips_ev);
        if (tm->img_ev) (void)hipEventDestroy(tm->img_ev);
        if (tm->copy_ev) (void)hipEventDestroy(tm->copy_ev);
        if (tm->copy_stream) (void)hipStreamDestroy(tm->copy_stream);
        TH_HIP(e);
    }
    *out = tm.release();
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_destroy(th_tm *tm) {
    TH_TRY
    if (!tm) return TH_OK;
    (void)hipSetDevice(tm->ctx->device);
    (void)hipStreamSynchronize(tm->ctx->stream);
    for (auto &sp : tm->slots) {
        (void)hipStreamSynchronize(sp->stream);
        (void)hipStreamDestroy(sp->stream);
        (void)hipHostFree(sp->h_tile);
        if (sp->al_ref_host) (void)hipHostFree(sp->al_ref_host);
        if (sp->exp_copy) (void)hipStreamDestroy(sp->exp_copy);
        for (int b = 0; b < 2; b++) {
            if (sp->exp_done[b]) (void)hipEventDestroy(sp->exp_done[b]);
            if (sp->exp_copied[b]) (void)hipEventDestroy(sp->exp_copied[b]);
        }
    }
    tm->tracks.clear();
    for (auto &kv : tm->plans) th_plan_destroy(kv.second);
    tm->axis_tabs.clear();
    if (tm->batch_stage) (void)hipHostFree(tm->batch_stage);
    tm->mip_jobs.release();
    tm->mip_scratch.release();
    tm->d_colormap.reset();
    if (tm->copy_ev) (void)hipEventDestroy(tm->copy_ev);
    if (tm->img_ev) (void)hipEventDestroy(tm->img_ev);
    if (tm->mips_ev) (void)hipEventDestroy(tm->mips_ev);
    if (tm->copy_stream) {
        (void)hipStreamSynchronize(tm->copy_stream);
        (void)hipStreamDestroy(tm->copy_stream);
    }
    delete tm;
    return TH_OK;
    TH_CATCH
}

namespace {
int upload_colormap(th_tm *tm) {
    if (tm->d_colormap) TH_CHECK(free_checked(tm->d_colormap));
    TH_HIP(tm->d_colormap.alloc(tm->colormap_rgba.size()));
    TH_HIP(hipMemcpyAsync(tm->d_colormap, tm->colormap_rgba.data(), tm->colormap_rgba.size(), hipMemcpyHostToDevice,
                          tm->ctx->stream));
    TH_HIP(hipStreamSynchronize(tm->ctx->stream));
    return TH_OK;
}
}  // namespace

TH_API int th_tm_set_colormap(th_tm *tm, const uint8_t *rgba, size_t bytes) {
    TH_TRY
    TH_REQUIRE(tm && rgba, "NULL argument");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    int rc = tmi::set_colormap_only(tm, rgba, bytes);
    if (rc != TH_OK) return rc;
    tm->invalidate_spectrogram();
    // → update_spec_imgs(force) — lib.rs:61, core/mod.rs:128-131
    std::vector<size_t> upd;
    return writer_done(tm, update_spec_imgs(tm, true, &upd));
    TH_CATCH
}

TH_API int th_tm_set_setting(th_tm *tm, double win_ms, uint32_t t_overlap, uint32_t f_overlap, int freq_scale) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    TH_REQUIRE(win_ms > 0. && t_overlap >= 1 && f_overlap >= 1, "invalid SpecSetting (lib.rs:275-277)");
    TH_REQUIRE(freq_scale == TH_FREQ_LINEAR || freq_scale == TH_FREQ_MEL, "bad freq_scale");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    tmi::StagedPtr staged;
    int rc = tmi::prepare_setting(tm, win_ms, t_overlap, f_overlap, freq_scale, &staged);
    if (rc != TH_OK) return rc;
    tmi::commit(tm, std::move(staged));
    std::vector<size_t> upd;
    rc = update_spec_imgs(tm, true, &upd);
    tm->invalidate_spectrogram();  // lib.rs:284
    return writer_done(tm, rc);
    TH_CATCH
}

TH_API int th_tm_set_dB_range(th_tm *tm, float dB_range) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    TH_REQUIRE(dB_range > 0.f, "dB_range must be > 0 (lib.rs:259)");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    TH_HIP(hipSetDevice(tm->ctx->device));
    tm->dB_range = dB_range;
    std::vector<size_t> upd;
    int rc = update_spec_imgs(tm, true, &upd);
    tm->invalidate_spectrogram();  // lib.rs:265
    return writer_done_images(tm, rc);
    TH_CATCH
}

TH_API int th_tm_add_tracks(th_tm *tm, size_t n_tracks, const size_t *ids, const uint32_t *srs,
                            const uint32_t *n_channels, const float *const *channels_flat, const size_t *n_samples) {
    TH_TRY
    TH_REQUIRE(tm && ids && srs && n_channels && channels_flat && n_samples, "NULL argument");
    TH_REQUIRE(n_tracks >= 1, "no tracks (lib.rs:182)");
    {   // validate everything before anything is allocated
        size_t flat = 0;
        for (size_t t = 0; t < n_tracks; t++) {
            TH_REQUIRE(srs[t] > 0 && n_channels[t] >= 1 && n_samples[t] >= 1, "track %zu: empty or invalid", ids[t]);
            for (uint32_t k = 0; k < n_channels[t]; k++, flat++)
                TH_REQUIRE(channels_flat[flat], "track %zu channel %u: NULL data", ids[t], k);
        }
    }
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    tmi::StagedPtr staged;
    int rc = tmi::prepare_add(tm, n_tracks, ids, srs, n_channels, channels_flat, n_samples, &staged);
    if (rc != TH_OK) return rc;
    tmi::commit(tm, std::move(staged));
    tm->invalidate_all();  // lib.rs:192
    return writer_done(tm, TH_OK);
    TH_CATCH
}

TH_API int th_tm_add_track(th_tm *tm, size_t id, uint32_t sr, uint32_t n_channels, const float *const *channels,
                           size_t n_samples) {
    return th_tm_add_tracks(tm, 1, &id, &sr, &n_channels, channels, &n_samples);
}

TH_API int th_tm_remove_track(th_tm *tm, size_t id) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    TH_HIP(hipSetDevice(tm->ctx->device));
    auto it = tm->tracks.find(id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", id);
    TH_HIP(hipStreamSynchronize(tm->ctx->stream));
    tm->tracks.erase(it);
    prune_axis_tabs(tm);
    retain_plans(tm);      // core/mod.rs:96-99
    tm->invalidate_all();  // lib.rs:221
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_apply_track_list_changes(th_tm *tm, size_t *updated_ids, size_t cap, size_t *n_updated,
                                          uint32_t *max_sr) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    TH_HIP(hipSetDevice(tm->ctx->device));
    std::vector<size_t> upd;
    int rc = writer_done_images(tm, update_spec_imgs(tm, false, &upd));
    if (rc != TH_OK) return rc;
    if (n_updated) *n_updated = upd.size();
    if (updated_ids)
        for (size_t i = 0; i < upd.size() && i < cap; i++) updated_ids[i] = upd[i];
    if (max_sr) *max_sr = tm->max_sr;
    if (!upd.empty()) tm->invalidate_spectrogram();  // lib.rs:243-245
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_get_db_state(const th_tm *tm, float *min_dB, float *max_dB, uint32_t *max_sr) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    if (min_dB) *min_dB = tm->min_dB;
    if (max_dB) *max_dB = tm->max_dB;
    if (max_sr) *max_sr = tm->max_sr;
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_spec_shape(const th_tm *tm, size_t id, uint32_t ch, size_t *n_frames, size_t *height) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    const Channel *c = find_channel(const_cast<th_tm *>(tm), id, ch);
    if (!c || !c->has_spec) return fail(TH_ERR_NOT_FOUND, "Spectrogram %zu_%u does not exist", id, ch);
    if (n_frames) *n_frames = c->T;
    if (height) *height = c->H;
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_img_shape(const th_tm *tm, size_t id, uint32_t ch, size_t *img_height, size_t *img_width) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    const Channel *c = find_channel(const_cast<th_tm *>(tm), id, ch);
    if (!c || !c->d_img) return fail(TH_ERR_NOT_FOUND, "Spectrogram %zu_%u does not exist", id, ch);
    if (img_height) *img_height = c->img_h;
    if (img_width) *img_width = c->img_w;
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_copy_spec(th_tm *tm, size_t id, uint32_t ch, float *out, size_t cap) {
    TH_TRY
    TH_REQUIRE(tm && out, "NULL argument");
    std::unique_lock<std::shared_mutex> wl(tm->rw);  // uses the context stream: exclusive, like a mutator
    TH_HIP(hipSetDevice(tm->ctx->device));
    Channel *c = find_channel(tm, id, ch);
    if (!c || !c->has_spec) return fail(TH_ERR_NOT_FOUND, "Spectrogram %zu_%u does not exist", id, ch);
    if (cap < c->T * c->H) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu floats", c->T * c->H);
    // de-pad to the reference's dense T x H layout
    if (c->T && c->H)
        TH_HIP(hipMemcpy2DAsync(out, c->H * sizeof(float), c->d_spec, c->spec_pitch * sizeof(float), c->H * sizeof(float),
                                c->T, hipMemcpyDeviceToHost, tm->ctx->stream));
    TH_HIP(hipStreamSynchronize(tm->ctx->stream));
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_copy_img(th_tm *tm, size_t id, uint32_t ch, uint16_t *out, size_t cap) {
    TH_TRY
    TH_REQUIRE(tm && out, "NULL argument");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    TH_HIP(hipSetDevice(tm->ctx->device));
    Channel *c = find_channel(tm, id, ch);
    if (!c || !c->d_img) return fail(TH_ERR_NOT_FOUND, "Spectrogram %zu_%u does not exist", id, ch);
    if (cap < c->img_h * c->img_w) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu pixels", c->img_h * c->img_w);
    if (c->img_h && c->img_w)
        TH_HIP(hipMemcpy2DAsync(out, c->img_w * sizeof(uint16_t), c->d_img, c->img_pitch * sizeof(uint16_t),
                                c->img_w * sizeof(uint16_t), c->img_h, hipMemcpyDeviceToHost, tm->ctx->stream));
    TH_HIP(hipStreamSynchronize(tm->ctx->stream));
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_put_img(th_tm *tm, size_t id, uint32_t ch, const uint16_t *img, size_t height, size_t width) {
    TH_TRY
    TH_REQUIRE(tm && img, "NULL argument");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    TH_HIP(hipSetDevice(tm->ctx->device));
    Channel *c = find_channel(tm, id, ch);
    if (!c || !c->d_img) return fail(TH_ERR_NOT_FOUND, "Spectrogram %zu_%u does not exist", id, ch);
    if (height != c->img_h || width != c->img_w)
        return fail(TH_ERR_INVALID_ARG, "image is %zu x %zu, the resident one %zu x %zu", height, width, c->img_h, c->img_w);
    if (height && width)
        TH_HIP(hipMemcpy2DAsync(c->d_img, c->img_pitch * sizeof(uint16_t), img, width * sizeof(uint16_t), width * sizeof(uint16_t),
                                height, hipMemcpyHostToDevice, tm->ctx->stream));
    TH_HIP(hipStreamSynchronize(tm->ctx->stream));  // img is the caller's
    std::vector<Channel *> one{c};
    int rc = build_mips(tm, one);
    if (rc != TH_OK) free_mips(*c);
    tm->invalidate_spectrogram();
    return writer_done(tm, rc);
    TH_CATCH
}

TH_API int th_tm_revisions(const th_tm *tm, uint64_t *waveform_revision, uint64_t *spectrogram_revision) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    if (waveform_revision) *waveform_revision = tm->waveform_revision();
    if (spectrogram_revision) *spectrogram_revision = tm->spectrogram_revision();
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_set_lod_source(th_tm *tm, int per_request) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    const int want = per_request ? 1 : 0;
    if (want == tm->lod_source) return TH_OK;
    TH_HIP(hipSetDevice(tm->ctx->device));
    std::vector<Channel *> have;
    for (auto &kv : tm->tracks)
        for (Channel &ch : kv.second.ch)
            if (ch.d_img) have.push_back(&ch);
    // 1: the pyramids go (build_mips frees them); 0: every resident image gets its levels back
    TH_HIP(hipStreamSynchronize(tm->ctx->stream));  // (may fail: the route has not changed yet)
    const int old_source = tm->lod_source;
    tm->lod_source = want;  // build_mips reads it
    int rc = build_mips(tm, have);
    if (rc != TH_OK) {
        // failure-atomic like the other writers: the route stays what it was.  The channels are left without
        // levels — never with stale ones — and are served through the per-request fallback, which is correct on either route.
        for (Channel *ch : have) free_mips(*ch);
        tm->lod_source = old_source;
    }
    prune_axis_tabs(tm);
    return writer_done(tm, rc);
    TH_CATCH
}

// get_spectrogram_tile — lib.rs:369-389 → RenderTileCache::spectrogram_tile (render_tiles.rs:171-188).
// Level (0, 0): a crop of the u16 image; LOD > 0: a crop of the pre-built mip level — either way one
// raster launch on the request's own stream, one copy into pinned memory, no table upload, no lock shared with other
// requests.
TH_API int th_tm_get_spectrogram_tile(th_tm *tm, size_t id, uint32_t ch, uint32_t level_x, uint32_t level_y,
                                      uint32_t tile_x, uint32_t tile_y, uint8_t *out, size_t cap, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(tm && out && out_len, "NULL argument");
    TH_CHECK(tmi::ensure_colormap(tm));  // (takes the lock exclusively when it has to upload the default map)
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    tmi::TileInfo it;
    TH_CHECK(tmi::tile_request_info(tm, th_tile_request{id, ch, level_x, level_y, tile_x, tile_y, 0}, &it));
    const uint64_t revision = tm->spectrogram_revision();
    if (it.single) {
        // per-request resampling of the crop box from the level-0 image (the reference's own flow): the
        // context-stream path, serialised by the context mutex
        return th_encode_spectrogram_tile_dev(tm->ctx, it.src, it.src_h, it.src_w, it.src_pitch, tm->colormap_rgba.data(),
                                              tm->colormap_rgba.size(), revision, level_x, level_y, tile_x, tile_y, out, cap, out_len);
    }
    const TileGeom &g = it.g;
    const size_t px_bytes = g.width * g.height * 4, need = 40 + px_bytes;
    *out_len = need;
    if (cap < need) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu bytes", need);
    put_spectrogram_tile_header(out, revision, g, level_x, level_y, tile_x, tile_y);
    if (g.width == 0 || g.height == 0) return TH_OK;
    if (px_bytes > TILE_BYTES_MAX) return fail(TH_ERR_INTERNAL, "tile larger than a reader slot");
    TH_HIP(hipSetDevice(tm->ctx->device));
    SlotLease lease{tm, nullptr};
    int rc = acquire_slot(tm, &lease.slot);
    if (rc != TH_OK) return rc;
    ReaderSlot &sl = *lease.slot;
    // (a mip level may still be building behind the mutator that re-made the images: th_tm::mips_ev)
    // (asked of the host first: a wait packet for an event that completed long ago still costs a request ~20 us)
    if ((level_x != 0 || level_y != 0) && tm->mips_ev != nullptr && hipEventQuery(tm->mips_ev) != hipSuccess) {
        (void)hipGetLastError();  // (hipErrorNotReady is the answer, not a failure)
        TH_HIP(hipStreamWaitEvent(sl.stream, tm->mips_ev, 0));
    }
    // The raster kernel writes the pixels straight into the slot's pinned, device-visible host buffer (16 bytes per lane,
    // 1 KB per wave-instruction over PCIe): no device staging tile, no copy-engine transfer queued behind other readers'.
    TH_HIP(launch_raster_tile(it.src, it.src_w, it.src_h, it.src_pitch, (uint32_t)g.origin_x, (uint32_t)g.origin_y, (uint32_t)g.width,
                              (uint32_t)g.height, sl.h_tile_dev, tm->d_colormap, (uint32_t)(tm->colormap_rgba.size() / 4),
                              sl.stream));
    TH_HIP(hipStreamSynchronize(sl.stream));
    std::memcpy(out + 40, sl.h_tile, px_bytes);
    return TH_OK;
    TH_CATCH
}

// get_waveform_tile — lib.rs:342-367: cache lookup (:350-355); on a miss the tile's bins are a contiguous piece of the
// channel's resident pyramid level (built once at add_tracks from one pass over the audio): one copy, no kernel.
TH_API int th_host_alloc(th_ctx *c, size_t bytes, void **ptr) {
    TH_TRY
    TH_REQUIRE(c && ptr, "NULL argument");
    TH_HIP(hipSetDevice(c->device));
    TH_HIP(hipHostMalloc(ptr, std::max<size_t>(bytes, 1), hipHostMallocMapped | hipHostMallocPortable));
    return TH_OK;
    TH_CATCH
}
TH_API int th_host_free(th_ctx *c, void *ptr) {
    TH_TRY
    TH_REQUIRE(c, "ctx is NULL");
    if (!ptr) return TH_OK;
    TH_HIP(hipSetDevice(c->device));
    TH_HIP(hipHostFree(ptr));
    return TH_OK;
    TH_CATCH
}

// N tiles, one raster launch (th_raster_tiles_dev on the context stream), one wait.  Level (0, 0) tiles are crops of the
// u16 image, LOD > 0 tiles crops of their mip level; requests for levels the pyramid does not hold (or with the per-request
// route selected) go through the single-tile path one by one.
namespace th {
namespace tmi {
int ensure_colormap(th_tm *tm) {
    {
        std::shared_lock<std::shared_mutex> rl(tm->rw);
        if (tm->d_colormap) return TH_OK;
    }
    std::unique_lock<std::shared_mutex> wl(tm->rw);  // no th_tm_set_colormap yet: the default two-colour map
    TH_HIP(hipSetDevice(tm->ctx->device));
    return tm->d_colormap ? TH_OK : upload_colormap(tm);
}

int tile_request_info(th_tm *tm, const th_tile_request &r, TileInfo *info) {
    Channel *c = find_channel(tm, r.id, r.ch);
    if (!c || !c->d_img) return fail(TH_ERR_NOT_FOUND, "Spectrogram %zu_%u does not exist", r.id, r.ch);
    TileInfo &it = *info;
    it = TileInfo{spectrogram_tile_geometry(c->img_w, c->img_h, r.level_x, r.level_y, r.tile_x, r.tile_y), c->d_img,
                  (uint32_t)c->img_w, (uint32_t)c->img_h, (uint32_t)c->img_pitch, false, 0, r};
    if (r.level_x != 0 || r.level_y != 0) {
        auto im = c->mips.find({r.level_x, r.level_y});
        if (tm->lod_source != 0 || im == c->mips.end()) {
            it.single = true;  // (src: the level-0 image the single-tile path resamples)
        } else {
            it.src = im->second.d;
            it.src_w = im->second.w;
            it.src_h = im->second.h;
            it.src_pitch = im->second.pitch;
            if (it.g.width && it.g.height && (it.g.lod_w != it.src_w || it.g.lod_h != it.src_h))
                return fail(TH_ERR_INTERNAL, "mip level (%u, %u) has the wrong shape", r.level_x, r.level_y);
        }
    }
    return TH_OK;
}

size_t tiles_layout(TileInfo *info, size_t n, size_t *offsets) {
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        offsets[i] = info[i].offset = total;
        total += tile_record_bytes(info[i].g);
    }
    return offsets[n] = total;
}

int tiles_run(th_tm *tm, size_t n, const TileInfo *info, uint8_t *out) {
    TH_HIP(hipSetDevice(tm->ctx->device));
    const uint64_t revision = tm->spectrogram_revision();
    // where the kernel writes: the caller's buffer when the GPU can reach it, else the manager's pinned staging buffer
    uint8_t *dev_base = nullptr;
    {
        hipPointerAttribute_t at{};
        void *dp = nullptr;
        const hipError_t qe = hipPointerGetAttributes(&at, out);
        if (qe == hipSuccess && at.type == hipMemoryTypeDevice)
            return fail(TH_ERR_INVALID_ARG, "out is device memory: th_tm_get_spectrogram_tiles writes tile headers from the host");
        if (qe == hipSuccess && at.type == hipMemoryTypeHost && hipHostGetDevicePointer(&dp, out, 0) == hipSuccess && dp)
            dev_base = static_cast<uint8_t *>(dp);
        else
            (void)hipGetLastError();  // (pageable memory: the query fails, that is the answer)
    }
    std::unique_lock<std::mutex> bl(tm->batch_mu, std::defer_lock);
    const bool staged = dev_base == nullptr;
    // request i's record under dev_base: at the caller's offset, or, staged, packed with this run's own records
    std::vector<size_t> at(n);
    size_t own = 0;
    for (size_t i = 0; i < n; i++) {
        at[i] = staged ? own : info[i].offset;
        own += tile_record_bytes(info[i].g);
    }
    if (staged) {
        bl.lock();
        if (tm->batch_stage_cap < own) {
            if (tm->batch_stage) (void)hipHostFree(tm->batch_stage);
            tm->batch_stage = tm->batch_stage_dev = nullptr;
            tm->batch_stage_cap = 0;
            TH_HIP(hipHostMalloc(&tm->batch_stage, own, hipHostMallocMapped));
            TH_HIP(hipHostGetDevicePointer(&tm->batch_stage_dev, tm->batch_stage, 0));
            tm->batch_stage_cap = own;
        }
        dev_base = static_cast<uint8_t *>(tm->batch_stage_dev);
    }
    std::vector<th_raster_desc> descs;
    descs.reserve(n);
    for (size_t i = 0; i < n; i++) {
        const TileInfo &it = info[i];
        if (it.single || !it.g.width || !it.g.height) continue;
        th_raster_desc d{};
        d.img = it.src;
        d.rgba = dev_base + at[i] + 40;
        d.img_width = it.src_w;
        d.img_height = it.src_h;
        d.origin_x = (uint32_t)it.g.origin_x;
        d.origin_y = (uint32_t)it.g.origin_y;
        d.width = (uint32_t)it.g.width;
        d.height = (uint32_t)it.g.height;
        d.img_pitch = it.src_pitch;
        descs.push_back(d);
    }
    if (!descs.empty()) {
        std::lock_guard<std::recursive_mutex> lk(tm->ctx->mu);  // the context stream: one user at a time
        int rc = th_raster_tiles_dev(tm->ctx, descs.data(), descs.size(), tm->d_colormap, (uint32_t)(tm->colormap_rgba.size() / 4));
        if (rc != TH_OK) return rc;
        TH_HIP(hipStreamSynchronize(tm->ctx->stream));
    }
    if (staged) {
        // the staging buffer is held only until its pixels are copied out: the per-request fallbacks and the
        // headers below no longer keep other pageable-buffer callers waiting
        for (size_t i = 0; i < n; i++) {
            const size_t px = info[i].g.width * info[i].g.height * 4;
            if (!info[i].single && px) std::memcpy(out + info[i].offset + 40, static_cast<uint8_t *>(tm->batch_stage) + at[i] + 40, px);
        }
        bl.unlock();
    }
    for (size_t i = 0; i < n; i++) {
        const TileInfo &it = info[i];
        const th_tile_request &r = it.r;
        uint8_t *rec = out + it.offset;
        if (it.single) {
            size_t len = 0;
            int rc = th_encode_spectrogram_tile_dev(tm->ctx, it.src, it.src_h, it.src_w, it.src_pitch, tm->colormap_rgba.data(),
                                                    tm->colormap_rgba.size(), revision, r.level_x, r.level_y, r.tile_x, r.tile_y,
                                                    rec, tile_record_bytes(it.g), &len);
            if (rc != TH_OK) return rc;
            continue;
        }
        put_spectrogram_tile_header(rec, revision, it.g, r.level_x, r.level_y, r.tile_x, r.tile_y);
    }
    return TH_OK;
}
}  // namespace tmi
}  // namespace th

TH_API int th_tm_get_spectrogram_tiles(th_tm *tm, const th_tile_request *reqs, size_t n, uint8_t *out, size_t cap,
                                       size_t *offsets, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(tm && out_len && (n == 0 || (reqs && offsets)), "NULL argument");
    *out_len = 0;
    if (n == 0) {
        if (offsets) offsets[0] = 0;
        return TH_OK;
    }
    TH_CHECK(tmi::ensure_colormap(tm));
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    std::vector<tmi::TileInfo> infos(n);
    for (size_t i = 0; i < n; i++) TH_CHECK(tmi::tile_request_info(tm, reqs[i], &infos[i]));
    const size_t total = tmi::tiles_layout(infos.data(), n, offsets);
    *out_len = total;
    if (cap < total || !out) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu bytes", total);
    return tmi::tiles_run(tm, n, infos.data(), out);
    TH_CATCH
}

// The spectrum of a time range of N (channel, range, kind) requests: a reader.  One job per request; the two launches of
// kernels_spectrum.hip on the slot's stream; results of up to h_tile's size are written by the kernel into the slot's pinned
// staging and copied out, larger ones go through the slot's device result buffer.
namespace th {
namespace tmi {
// in the order every caller reports: the id, the channel, the kind, the spec, the time range, the shape
int spectrum_request_info(th_tm *tm, const th_spectrum_request &r, size_t i, SpectrumInfo *info) {
    auto it = tm->tracks.find(r.id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", r.id);
    const Track &tr = it->second;
    TH_REQUIRE(r.ch < tr.ch.size(), "request %zu: track %zu has no channel %u", i, r.id, r.ch);
    TH_REQUIRE(r.kind <= TH_SPECTRUM_MAX, "request %zu: unknown spectrum kind %u", i, r.kind);
    const Channel &c = tr.ch[r.ch];
    if (!c.has_spec) return fail(TH_ERR_NOT_FOUND, "Spectrogram %zu_%u does not exist", r.id, r.ch);
    size_t hop, win, n_fft, f0 = 0, f1 = 0;
    calc_framing_params(tm->win_ms, tm->t_overlap, tm->f_overlap, tr.sr, &hop, &win, &n_fft);
    TH_REQUIRE(spectrum_frame_range(tr.sr, hop, c.T, r.start_sec, r.end_sec, &f0, &f1), "request %zu: bad time range [%g, %g) s", i,
               r.start_sec, r.end_sec);
    if (c.T > INT32_MAX || c.H > INT32_MAX || (c.spec_pitch & 3) != 0)
        return fail(TH_ERR_UNSUPPORTED, "Spectrogram %zu_%u: %zu x %zu rows of pitch %zu", r.id, r.ch, c.T, c.H, c.spec_pitch);
    const SpectrumShape sh = spectrum_shape((uint32_t)c.H, (uint32_t)(f1 - f0));
    if ((uint64_t)sh.n_ctiles * sh.n_slices > INT32_MAX) return fail(TH_ERR_UNSUPPORTED, "Spectrogram %zu_%u: too many blocks", r.id, r.ch);
    *info = SpectrumInfo{{0, c.H, f0, f1, 0}, r.kind, c.d_spec, c.spec_pitch};
    return TH_OK;
}

int SpectrumReader::fit(const SpectrumInfo *, size_t n) {
    TH_REQUIRE(n <= UINT32_MAX, "too many requests");
    return TH_OK;
}

size_t SpectrumReader::layout(SpectrumInfo *info, size_t n) {
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        info[i].offset = total;
        total += info[i].height;
    }
    return total;
}

int spectra_run(th_tm *tm, size_t n, SpectrumInfo *info, float *out) {
    TH_REQUIRE(n <= UINT32_MAX, "too many requests");
    std::vector<SpectrumJob> jobs(n);
    std::vector<size_t> part0(n), res0(n);  // job i in the slot's areas: its first partial, in doubles, and its first result, in floats
    size_t total = 0, part_total = 0;
    uint32_t max_blocks = 0, max_h = 0;
    for (size_t i = 0; i < n; i++) {
        const SpectrumShape sh = spectrum_shape((uint32_t)info[i].height, (uint32_t)(info[i].frame_end - info[i].frame_start));
        SpectrumJob &j = jobs[i];
        j.rows = info[i].rows;
        j.pitch = info[i].pitch;
        j.H = (uint32_t)info[i].height;
        j.f0 = (uint32_t)info[i].frame_start;
        j.f1 = (uint32_t)info[i].frame_end;
        j.kind = info[i].kind;
        j.log_ct = sh.log_ct;
        j.n_ctiles = sh.n_ctiles;
        j.n_slices = sh.n_slices;
        j.slice_len = sh.slice_len;
        part0[i] = part_total;
        part_total += (size_t)sh.n_slices * ((size_t)sh.n_ctiles << (sh.log_ct + 2));
        max_blocks = std::max(max_blocks, sh.n_ctiles * sh.n_slices);
        max_h = std::max(max_h, j.H);
        res0[i] = total;
        total += info[i].height;
    }
    TH_HIP(hipSetDevice(tm->ctx->device));
    SlotLease lease{tm, nullptr};
    int rc = acquire_slot(tm, &lease.slot);
    if (rc != TH_OK) return rc;
    ReaderSlot &sl = *lease.slot;
    const bool pinned = total * sizeof(float) <= TILE_BYTES_MAX;
    TH_CHECK(sl.spec_part.ensure(std::max<size_t>(part_total, 1) * sizeof(double)));
    if (!pinned) TH_CHECK(sl.spec_out.ensure(total * sizeof(float)));
    float *res = pinned ? reinterpret_cast<float *>(sl.h_tile_dev) : static_cast<float *>(sl.spec_out.dptr);
    for (size_t i = 0; i < n; i++) {
        jobs[i].part = static_cast<double *>(sl.spec_part.dptr) + part0[i];
        jobs[i].out = res + res0[i];
    }
    TH_CHECK(sl.spec_jobs.upload(sl.stream, jobs.data(), n * sizeof(SpectrumJob)));
    TH_HIP(launch_spectrum(static_cast<const SpectrumJob *>(sl.spec_jobs.dptr), (uint32_t)n, max_blocks, max_h, sl.stream));
    if (pinned) TH_HIP(hipStreamSynchronize(sl.stream));
    // one copy per maximal run of adjacent destinations (a batch this manager owns whole: one copy); a failed enqueue still waits
    // for the copies in front of it, which write the caller's memory
    hipError_t e = hipSuccess;
    for (size_t i = 0, k; i < n; i = k) {
        k = i + 1;
        while (k < n && info[k].offset == info[k - 1].offset + info[k - 1].height) k++;
        const size_t bytes = (res0[k - 1] + info[k - 1].height - res0[i]) * sizeof(float);
        if (pinned)
            std::memcpy(out + info[i].offset, reinterpret_cast<const float *>(sl.h_tile) + res0[i], bytes);
        else if (e == hipSuccess)
            e = hipMemcpyAsync(out + info[i].offset, res + res0[i], bytes, hipMemcpyDeviceToHost, sl.stream);
    }
    if (!pinned) {
        const hipError_t waited = hipStreamSynchronize(sl.stream);
        TH_HIP(e);
        TH_HIP(waited);
    }
    return TH_OK;
}
}  // namespace tmi
}  // namespace th

TH_API int th_tm_get_spectra(th_tm *tm, const th_spectrum_request *reqs, size_t n, float *out, size_t cap, th_spectrum_info *info,
                             size_t *out_len) {
    TH_TRY
    return br::batched_read<tmi::SpectrumReader>(TmReaders{tm}, reqs, n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_get_spectrum(th_tm *tm, size_t id, uint32_t ch, int kind, double start_sec, double end_sec, float *out, size_t cap,
                              th_spectrum_info *info) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    TH_REQUIRE(kind >= 0, "unknown spectrum kind %d", kind);
    const th_spectrum_request r{id, ch, (uint32_t)kind, start_sec, end_sec};
    return br::single_read(info, [&](th_spectrum_info *one, size_t *len) { return th_tm_get_spectra(tm, &r, 1, out, cap, one, len); });
    TH_CATCH
}

TH_API int th_tm_get_waveform_tile(th_tm *tm, size_t id, uint32_t ch, uint32_t level, uint32_t tile_index,
                                   uint8_t *out, size_t cap, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(tm && out && out_len, "NULL argument");
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    Channel *c = find_channel(tm, id, ch);
    if (!c) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", id);
    uint64_t revision = 0;
    std::vector<uint8_t> cached;
    if (tm->cache.lookup(id, ch, level, tile_index, &revision, &cached)) {
        *out_len = cached.size();
        if (cap < cached.size()) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu bytes", cached.size());
        std::memcpy(out, cached.data(), cached.size());
        return TH_OK;
    }
    size_t start, bins, spb;
    waveform_tile_geometry(c->n, level, tile_index, &start, &bins, &spb);
    const size_t need = 24 + bins * 12;
    *out_len = need;
    if (cap < need) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu bytes", need);
    put_waveform_tile_header(out, revision, bins, spb, tile_index);
    if (bins) {
        if (!c->d_draw || !c->pyr_levels) return fail(TH_ERR_INTERNAL, "channel %zu_%u has no waveform pyramid", id, ch);
        // a level above the pyramid's last one still has exactly one bin, over the same samples
        const uint32_t lv = level < c->pyr_levels ? level : c->pyr_levels - 1;
        const size_t first_bin = lv == level ? (size_t)tile_index * 1024 : 0;
        TH_HIP(hipSetDevice(tm->ctx->device));
        SlotLease lease{tm, nullptr};
        int rc = acquire_slot(tm, &lease.slot);
        if (rc != TH_OK) return rc;
        ReaderSlot &sl = *lease.slot;
        if (lv < PYR_FIRST) {
            // levels 0 and 1 are not materialised: copy the tile's samples (4 / 8 KB against 12 KB of bins) and form the bins
            // here exactly as waveform_bin_stats does for short slices (render_tiles.rs:261-279: f32::min / f32::max folds,
            // sequential sum / len — one or two samples per bin)
            const size_t spb_lv = (size_t)1 << lv;
            const size_t s0 = lv == level ? start : 0, s1 = std::min<size_t>(c->n, s0 + bins * spb_lv);
            TH_HIP(hipMemcpyAsync(sl.h_tile, c->d_draw + s0, (s1 - s0) * 4, hipMemcpyDeviceToHost, sl.stream));
            TH_HIP(hipStreamSynchronize(sl.stream));
            const float *x = reinterpret_cast<const float *>(sl.h_tile);
            for (size_t b = 0; b < bins; b++) {
                const size_t a = b * spb_lv, e = std::min(s1 - s0, a + spb_lv);
                float mn = INFINITY, mx = -INFINITY, sum = 0.0f;
                for (size_t i = a; i < e; i++) {
                    mn = std::fmin(mn, x[i]);
                    mx = std::fmax(mx, x[i]);
                    sum = sum + x[i];
                }
                const float mean = sum / (float)(e - a);
                std::memcpy(out + 24 + 12 * b, &mn, 4);
                std::memcpy(out + 28 + 12 * b, &mx, 4);
                std::memcpy(out + 32 + 12 * b, &mean, 4);
            }
        } else {
            const float *d_src = c->d_pyr + (th_waveform_pyramid_offset(c->n, lv) - th_waveform_pyramid_offset(c->n, PYR_FIRST)) + 3 * first_bin;
            TH_HIP(hipMemcpyAsync(sl.h_tile, d_src, bins * 12, hipMemcpyDeviceToHost, sl.stream));
            TH_HIP(hipStreamSynchronize(sl.stream));
            std::memcpy(out + 24, sl.h_tile, bins * 12);
        }
    }
    tm->cache.store(id, ch, revision, level, tile_index, out, need);
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_get_audio_stats(th_tm *tm, size_t id, th_audio_stats *out) {
    TH_TRY
    TH_REQUIRE(tm && out, "NULL argument");
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    auto it = tm->tracks.find(id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", id);
    *out = it->second.stats;
    return TH_OK;
    TH_CATCH
}

// ---------------------------------------------------------------------------------------------- loudness meter
namespace {
// what is known of a track's meter without the GPU: the factor and the lengths of the two series
void meter_counts(const Track &tr, th_loudness_meter *m) {
    *m = th_loudness_meter{};
    const size_t n = tr.ch.empty() ? 0 : tr.ch[0].n;
    m->oversampling = true_peak_factor(tr.sr);
    if (loudness_rate_ok(tr.sr)) {
        m->n_momentary = loudness_n_blocks(n, tr.sr);
        m->n_short_term = loudness_n_short_term(n, tr.sr);
    }
}

}  // namespace

namespace th {
namespace tmi {
int loudness_meter_info(th_tm *tm, size_t id, MeterInfo *m) {
    auto it = tm->tracks.find(id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", id);
    meter_counts(it->second, m);
    m->id = id;
    m->track = &it->second;
    m->n_channels = it->second.ch.size();
    return TH_OK;
}

// as th_tm's entry point reports them before a short buffer
int MeterReader::fit(const MeterInfo *ms, size_t n) {
    size_t n_ch = 0;
    for (size_t i = 0; i < n; i++) n_ch += ms[i].n_channels;
    if (const char *text = meter_limits_text(n, n_ch)) return fail(TH_ERR_INVALID_ARG, "%s", text);
    return TH_OK;
}

size_t MeterReader::layout(MeterInfo *m, size_t n) {
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        m[i].momentary_offset = total;
        total += m[i].n_momentary;
        m[i].short_term_offset = total;
        total += m[i].n_short_term;
    }
    return total;
}
}  // namespace tmi
}  // namespace th

// The loudness meters of N tracks: a reader.  plan_meters (reader_plan.h) makes the job tables and lays the slot's memory out,
// bind_meters gives them their addresses.  Everything runs on the slot's stream; the results come back in one copy (through the slot's
// pinned staging when they fit) and meter_results turns them into LUFS, maxima and the loudness range.
namespace th {
namespace tmi {
int meters_run(th_tm *tm, size_t n, MeterInfo *ms, double *series) {
    TH_CHECK(MeterReader::fit(ms, n));  // (before n tracks are gathered)
    std::vector<MeterPlanTrack> trs(n);
    std::vector<const float *> wav;
    for (size_t i = 0; i < n; i++) {
        const Track &tr = *static_cast<const Track *>(ms[i].track);
        const uint64_t ns = tr.ch.empty() ? 0 : tr.ch[0].n;
        trs[i] = MeterPlanTrack{ms[i].id, tr.sr, (uint32_t)tr.ch.size(), ms[i].oversampling, ns, ms[i].n_momentary, ms[i].n_short_term};
        for (size_t k = 0; k < tr.ch.size(); k++) {
            TH_REQUIRE(ns == 0 || tr.ch[k].d_wav, "track %zu channel %zu has no audio", ms[i].id, k);
            wav.push_back(tr.ch[k].d_wav);
        }
    }
    MeterPlan pl = plan_meters(trs.data(), n);
    if (pl.err != TH_OK) return fail(pl.err, "%s", pl.err_text.c_str());
    TH_HIP(hipSetDevice(tm->ctx->device));
    SlotLease lease{tm, nullptr};
    int rc = acquire_slot(tm, &lease.slot);
    if (rc != TH_OK) return rc;
    ReaderSlot &sl = *lease.slot;
    TH_CHECK(sl.meter_mem.ensure(pl.mem_bytes));
    unsigned char *dm = static_cast<unsigned char *>(sl.meter_mem.dptr);
    const std::vector<unsigned char> h = bind_meters(pl, dm, wav.data());
    TH_CHECK(sl.meter_tab.upload(sl.stream, h.data(), h.size()));
    const unsigned char *dt = static_cast<const unsigned char *>(sl.meter_tab.dptr);
    TH_HIP(hipMemsetAsync(dm + pl.o_sums, 0, pl.res_bytes - pl.o_sums, sl.stream));  // sums = 0, peaks = +0.0
    TH_HIP(launch_loudness(reinterpret_cast<const LoudJob *>(dt), (uint32_t)pl.jobs.size(), pl.max_chunks, pl.max_fchunks,
                           reinterpret_cast<const LoudnessRate *>(dt + pl.t_rates), pl.lds_floats, nullptr, 0, 0, sl.stream));
    TH_HIP(launch_loudness_blocks(reinterpret_cast<const LoudTrackJob *>(dt + pl.t_m), (uint32_t)n, pl.max_m, 4, sl.stream));
    TH_HIP(launch_loudness_blocks(reinterpret_cast<const LoudTrackJob *>(dt + pl.t_s), (uint32_t)n, pl.max_s, 30, sl.stream));
    for (int f = 0; f < 2; f++) {
        if (pl.tp[f].empty()) continue;
        TruePeakCoef K;
        true_peak_coef(f ? 2 : 4, &K);
        TH_HIP(launch_true_peak(reinterpret_cast<const TruePeakJob *>(dt + (f ? pl.t_tp2 : pl.t_tp4)), (uint32_t)pl.tp[f].size(), pl.tp_chunks[f],
                                f ? 2 : 4, K, sl.stream));
    }
    std::vector<unsigned char> big;
    const unsigned char *res = sl.h_tile;
    if (pl.res_bytes <= TILE_BYTES_MAX) {
        TH_HIP(hipMemcpyAsync(sl.h_tile, dm, pl.res_bytes, hipMemcpyDeviceToHost, sl.stream));
    } else {
        big.resize(pl.res_bytes);
        res = big.data();
        TH_HIP(hipMemcpyAsync(big.data(), dm, pl.res_bytes, hipMemcpyDeviceToHost, sl.stream));
    }
    TH_HIP(hipStreamSynchronize(sl.stream));
    std::vector<th_loudness_meter *> meters(n);
    for (size_t i = 0; i < n; i++) meters[i] = &ms[i];
    meter_results(res, pl, meters.data(), series);
    return TH_OK;
}
}  // namespace tmi
}  // namespace th

TH_API int th_tm_get_loudness_meters(th_tm *tm, const size_t *ids, size_t n, th_loudness_meter *meters, double *series, size_t cap,
                                     size_t *out_len) {
    TH_TRY
    TH_REQUIRE(meters, "NULL argument");  // (also for n == 0)
    return br::batched_read<tmi::MeterReader>(TmReaders{tm}, ids, n, series, cap, meters, out_len);
    TH_CATCH
}

TH_API int th_tm_get_loudness_meter(th_tm *tm, size_t id, th_loudness_meter *meter, double *series, size_t cap) {
    TH_TRY
    TH_REQUIRE(tm && meter, "NULL argument");
    size_t len = 0;
    return th_tm_get_loudness_meters(tm, &id, 1, meter, series, cap, &len);
    TH_CATCH
}

// get_audio_render_metadata — lib.rs:321-340 → RenderTileCache::metadata (render_tiles.rs:101-122)
TH_API int th_tm_get_audio_render_metadata(th_tm *tm, size_t id, uint32_t ch, double track_sec, int is_clipped,
                                           th_render_metadata *out) {
    TH_TRY
    TH_REQUIRE(tm && out, "NULL argument");
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    auto it = tm->tracks.find(id);
    if (it == tm->tracks.end() || ch >= it->second.ch.size()) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", id);
    const Channel &c = it->second.ch[ch];
    *out = th_render_metadata{};
    out->waveform_revision = tm->waveform_revision();
    out->spectrogram_revision = tm->spectrogram_revision();
    out->sample_rate = it->second.sr;
    // (lib.rs:328: channel_for_drawing's flag; a host that guards clipping itself passes its own)
    out->is_clipped = (is_clipped || it->second.guard_result == TH_GUARD_RESULT_BEFORE_CLIP) ? 1u : 0u;
    out->sample_count = c.n;
    out->track_sec = track_sec;
    out->spectrogram_height = c.d_img ? c.img_h : 0;  // (shape[0], shape[1]) of the u16 image, lib.rs:330-332
    out->spectrogram_width = c.d_img ? c.img_w : 0;
    out->waveform_tile_bins = 1024;
    out->spectrogram_tile_size = 512;
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_tile_cache(th_tm *tm, th_tile_cache **out) {
    TH_TRY
    TH_REQUIRE(tm && out, "NULL argument");
    *out = &tm->cache;
    return TH_OK;
    TH_CATCH
}

// device pointer + shape of one level of a channel's LOD mip pyramid ((0, 0) = the image itself): parity tests
TH_API int th_tm_lod_footprint(th_tm *tm, size_t *n_axis_tables, size_t *axis_table_bytes, size_t *mip_bytes) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    size_t ab = 0, mb = 0;
    for (auto &kv : tm->axis_tabs) ab += kv.second.bytes;
    for (auto &kv : tm->tracks)
        for (Channel &ch : kv.second.ch) mb += ch.mips_elems * sizeof(uint16_t);
    if (n_axis_tables) *n_axis_tables = tm->axis_tabs.size();
    if (axis_table_bytes) *axis_table_bytes = ab;
    if (mip_bytes) *mip_bytes = mb;
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_mip_level(th_tm *tm, size_t id, uint32_t ch, uint32_t level_x, uint32_t level_y, uint16_t *out, size_t cap,
                           size_t *width, size_t *height) {
    TH_TRY
    TH_REQUIRE(tm, "NULL argument");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    TH_HIP(hipSetDevice(tm->ctx->device));
    Channel *c = find_channel(tm, id, ch);
    if (!c || !c->d_img) return fail(TH_ERR_NOT_FOUND, "Spectrogram %zu_%u does not exist", id, ch);
    const uint16_t *src = c->d_img;
    size_t w = c->img_w, h = c->img_h, pitch = c->img_pitch;
    if (level_x || level_y) {
        auto im = c->mips.find({level_x, level_y});
        if (im == c->mips.end()) return fail(TH_ERR_NOT_FOUND, "mip level (%u, %u) is not resident", level_x, level_y);
        src = im->second.d;
        w = im->second.w;
        h = im->second.h;
        pitch = im->second.pitch;
    }
    if (width) *width = w;
    if (height) *height = h;
    if (!out) return TH_OK;
    if (cap < w * h) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu pixels", w * h);
    if (w && h)
        TH_HIP(hipMemcpy2DAsync(out, w * sizeof(uint16_t), src, pitch * sizeof(uint16_t), w * sizeof(uint16_t), h,
                                hipMemcpyDeviceToHost, tm->ctx->stream));
    TH_HIP(hipStreamSynchronize(tm->ctx->stream));
    return TH_OK;
    TH_CATCH
}

// ---------------------------------------------------------------------------------------------- normalise + clip guard
namespace {

// One channel's piece of a track's pool: `wav_copies` times the samples, then the materialised levels of its waveform pyramid
// (256-byte pieces: every view starts on a 256-byte boundary).  The original pool holds the samples once; the derived one holds
// the audio and, in Clip mode, the before-clip audio.
// levels: up to the one whose single bin spans the channel (render_tiles.rs:232-259); PYR_FIRST .. levels - 1 are resident: level 0
// would be (x, x, x) per sample — half of the pyramid's bytes — and level 1 a quarter; tiles of both are served from the resident
// samples instead (th_pyramid_desc.first_level)
struct PoolLayout {
    uint32_t levels;
    size_t wav_f, pyr_f, stride;  // in floats; stride: from one channel's piece to the next
};
PoolLayout pool_layout(size_t n, size_t wav_copies) {
    PoolLayout p{};
    p.levels = 1;
    while (p.levels < PYR_MAX_LEVELS && ((uint64_t)1 << (p.levels - 1)) < n) p.levels++;
    p.wav_f = (n + 63) / 64 * 64;
    p.pyr_f = (std::max<size_t>(1, th_waveform_pyramid_offset(n, std::max(p.levels, PYR_FIRST)) - th_waveform_pyramid_offset(n, PYR_FIRST)) + 63) / 64 * 64;
    p.stride = p.wav_f * wav_copies + p.pyr_f;
    return p;
}

// One track's audio derived from its original under (kind, target, mode) — AudioTrack::apply_gain, track.rs:158-170 — staged beside
// the track until install_derived()
struct Derived {
    bool active = false;  // false: gain 1 or not finite, the audio is the original
    DeviceBuf<float> d_pool;
    float gain = 1.0f, global_gain = 1.0f;
    int result = TH_GUARD_RESULT_GLOBAL_GAIN;
    float *d_gain = nullptr;
    bool limiting = false, gain_below_one = false;
    std::vector<float *> aud, draw, pyr;
    th_audio_stats stats{};
    std::vector<th_guard_clip_stats> guard_stats;
    size_t red0 = 0, loud_index = 0;  // its first reduction slot; its place in the loudness batch
};
// The tracks of one mutator re-derived under the common settings (kind, target, mode), which it installs with them
struct DeriveBatch {
    int kind = TH_NORM_OFF, mode = TH_GUARD_REDUCE_GLOBAL_LEVEL;
    float target = 0.0f;
    std::map<size_t, Derived> of;
    DeviceBuf<unsigned char> d_tab, d_scratch;  // job tables and reduction slots; the limiter's scratch
    std::unique_ptr<LoudnessBatch> loud;
    size_t n_red = 0, o_cnt = 0;
};

// Enqueue, on the context stream, the derived audio of `tracks` with its waveform pyramids and loudness passes.  Nothing waits.
int derive_enqueue(th_tm *tm, const std::vector<std::pair<size_t, Track *>> &tracks, DeriveBatch *b) {
    th_ctx *c = tm->ctx;
    const int kind = b->kind, mode = b->mode;
    std::vector<DynApplyJob> ajobs;
    std::vector<LimJob> ljobs;
    std::vector<size_t> l_scratch;  // bytes of scratch of every limiter job
    std::vector<uint32_t> red_init;
    std::vector<th_pyramid_desc> pdescs;
    std::vector<th_audio_desc> adescs;
    std::vector<std::vector<const float *>> aptrs;
    uint64_t max_n = 0;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    for (auto &it : tracks) {
        Track &tr = *it.second;
        Derived &d = b->of[it.first];
        float gain = 1.0f;
        TH_REQUIRE(normalize_gain(kind, b->target, tr.orig_stats.global_lufs, tr.orig_stats.rms_dB, tr.orig_stats.max_peak_dB, &gain),
                   "unknown normalize kind %d", kind);
        if (!std::isfinite(gain) || gain == 1.0f) continue;  // the audio is the original
        const size_t n = tr.ch[0].n, n_ch = tr.ch.size();
        // f32 multiplication by a positive gain is monotone: the peak of gain x is fl(gain max|x|) — no pass over the audio
        const float peak = gain * tr.orig_stats.max_peak;
        const bool clip = mode == TH_GUARD_CLIP;
        d.limiting = mode == TH_GUARD_LIMITER && peak > 1.0f;
        LimiterParams lp{};
        if (d.limiting) {
            if (!limiter_params(tr.sr, &lp)) return fail(TH_ERR_UNSUPPORTED, "track %zu: sample rate %u: the limiter's attack would be 0 samples", it.first, tr.sr);
            if ((uint64_t)n + lp.attack >= (1ull << 31)) return fail(TH_ERR_UNSUPPORTED, "track %zu: too long for the limiter (2^31 samples)", it.first);
        }
        const PoolLayout pl = pool_layout(n, clip ? 2 : 1);
        const size_t wav_f = pl.wav_f, per_ch = pl.stride;
        TH_HIP(d.d_pool.alloc((per_ch * n_ch + (d.limiting ? wav_f : 0)) * sizeof(float)));
        d.active = true;
        d.gain = gain;
        float *base = d.d_pool;
        aptrs.emplace_back();
        for (size_t k = 0; k < n_ch; k++) {
            d.aud.push_back(base + k * per_ch);
            d.draw.push_back(clip ? base + k * per_ch + wav_f : base + k * per_ch);
            d.pyr.push_back(base + k * per_ch + wav_f * (clip ? 2 : 1));
            pdescs.push_back(th_pyramid_desc{d.draw[k], d.pyr[k], n, tr.ch[k].pyr_levels, PYR_FIRST});
            aptrs.back().push_back(d.aud[k]);
        }
        d.loud_index = adescs.size();
        adescs.push_back(th_audio_desc{nullptr, (uint64_t)n, (uint32_t)n_ch, tr.sr, nullptr});
        const uint64_t x_stride = n_ch > 1 ? (uint64_t)(tr.ch[1].d_orig - tr.ch[0].d_orig) : 0;
        d.red0 = red_init.size();
        if (d.limiting) {
            d.result = TH_GUARD_RESULT_GAIN_SEQUENCE;
            d.d_gain = base + n_ch * per_ch;
            LimJob j{};
            j.x = tr.ch[0].d_orig;
            j.aud = d.aud[0];
            j.gain_seq = d.d_gain;
            j.x_stride = x_stride;
            j.y_stride = per_ch;
            j.n = n;
            j.slew = 1.0 / (lp.release_samples + 1.0);  // ExponentialRelease::with_initial_value (limiter.rs:24-31)
            j.gain = gain;
            j.n_ch = (uint32_t)n_ch;
            j.attack = lp.attack;
            j.hold = lp.hold_length;
            for (int i = 0; i < 3; i++) j.box_len[i] = lp.box_len[i];
            const size_t N = n + lp.attack;
            l_scratch.push_back(up(N * 4) + up((N / LIM_BLOCK + 1) * 4) + 2 * up(N * 8) + up((N / LIM_CHUNK + 1) * 32));
            ljobs.push_back(j);
            red_init.push_back(0x3f800000u);  // the least gain starts at 1.0f
        } else {
            d.result = clip ? TH_GUARD_RESULT_BEFORE_CLIP : mode == TH_GUARD_LIMITER ? TH_GUARD_RESULT_GAIN_SEQUENCE : TH_GUARD_RESULT_GLOBAL_GAIN;
            DynApplyJob j{};
            j.x = tr.ch[0].d_orig;
            j.aud = d.aud[0];
            j.before = clip ? d.draw[0] : nullptr;
            j.x_stride = x_stride;
            j.y_stride = per_ch;
            j.n = n;
            j.gain = gain;
            j.n_ch = (uint32_t)n_ch;
            j.clip = clip;
            if (mode == TH_GUARD_REDUCE_GLOBAL_LEVEL && peak > 1.0f) {  // audio.rs:145-159
                j.scale = 1;
                j.g = 1.0 / (double)peak;
                d.global_gain = (float)j.g;
            }
            ajobs.push_back(j);
            if (clip) red_init.insert(red_init.end(), n_ch, 0u);
            max_n = std::max<uint64_t>(max_n, n);
        }
    }
    if (adescs.empty()) return TH_OK;
    // device tables: [apply jobs][limiter jobs][counts u64][peak / least-gain bits u32]
    b->n_red = red_init.size();
    const size_t o_lim = up(ajobs.size() * sizeof(DynApplyJob)), o_cnt = o_lim + up(ljobs.size() * sizeof(LimJob)), o_bits = o_cnt + up(b->n_red * 8);
    const size_t tab_bytes = o_bits + up(b->n_red * 4);
    b->o_cnt = o_cnt;
    TH_HIP(b->d_tab.alloc(tab_bytes));
    unsigned char *dt = b->d_tab;
    // the limiter's scratch: groups of jobs under 1 GiB run one after the other on the stream and share one buffer
    constexpr size_t SCRATCH_CAP = (size_t)1 << 30;
    std::vector<std::pair<size_t, size_t>> groups;  // [first, last) limiter jobs
    size_t scratch_bytes = 0;
    for (size_t j0 = 0; j0 < ljobs.size();) {
        size_t j1 = j0, bytes = 0;
        while (j1 < ljobs.size() && (j1 == j0 || bytes + l_scratch[j1] <= SCRATCH_CAP)) bytes += l_scratch[j1++];
        groups.push_back({j0, j1});
        scratch_bytes = std::max(scratch_bytes, bytes);
        j0 = j1;
    }
    if (scratch_bytes) TH_HIP(b->d_scratch.alloc(scratch_bytes));
    {
        size_t ri = 0, ai = 0, li = 0;
        for (auto &it : tracks) {  // (the order the jobs were made in)
            Derived &d = b->of[it.first];
            if (!d.active) continue;
            uint32_t *bits = reinterpret_cast<uint32_t *>(dt + o_bits) + ri;
            unsigned long long *cnt = reinterpret_cast<unsigned long long *>(dt + o_cnt) + ri;
            if (d.limiting) {
                ljobs[li].min_bits = bits;
                ljobs[li].cnt = cnt;
                li++;
                ri += 1;
            } else {
                if (ajobs[ai].clip) {
                    ajobs[ai].peak_bits = bits;
                    ajobs[ai].cnt = cnt;
                    ri += ajobs[ai].n_ch;
                }
                ai++;
            }
        }
        for (auto &g : groups) {
            size_t off = 0;
            for (size_t j = g.first; j < g.second; j++) {
                unsigned char *p = b->d_scratch.get() + off;
                const size_t N = ljobs[j].n + ljobs[j].attack;
                ljobs[j].v = reinterpret_cast<float *>(p);
                p += up(N * 4);
                ljobs[j].bm = reinterpret_cast<float *>(p);
                p += up((N / LIM_BLOCK + 1) * 4);
                ljobs[j].a = reinterpret_cast<double *>(p);
                p += up(N * 8);
                ljobs[j].b = reinterpret_cast<double *>(p);
                p += up(N * 8);
                ljobs[j].sum = reinterpret_cast<double *>(p);
                off += l_scratch[j];
            }
        }
    }
    std::vector<unsigned char> h(tab_bytes, 0);
    if (!ajobs.empty()) std::memcpy(h.data(), ajobs.data(), ajobs.size() * sizeof(DynApplyJob));
    if (!ljobs.empty()) std::memcpy(h.data() + o_lim, ljobs.data(), ljobs.size() * sizeof(LimJob));
    if (b->n_red) std::memcpy(h.data() + o_bits, red_init.data(), b->n_red * 4);
    TH_HIP(hipMemcpy(dt, h.data(), tab_bytes, hipMemcpyHostToDevice));  // (a fresh allocation: nothing on the stream reads it yet)
    TH_HIP(launch_dyn_apply(reinterpret_cast<const DynApplyJob *>(dt), (uint32_t)ajobs.size(), max_n, c->stream));
    for (auto &g : groups)
        TH_HIP(launch_limiter(ljobs.data() + g.first, reinterpret_cast<const LimJob *>(dt + o_lim) + g.first, (uint32_t)(g.second - g.first), c->stream));
    int rc = th_waveform_pyramid_dev(c, pdescs.data(), pdescs.size());
    if (rc != TH_OK) return rc;
    for (size_t i = 0; i < adescs.size(); i++) adescs[i].channels = aptrs[i].data();
    b->loud.reset(new LoudnessBatch);
    return loudness_enqueue(c, adescs.data(), adescs.size(), true, true, b->loud.get());
}

// after the stream has drained: the derived audio's stats and guard stats (GuardClippingStats, stats.rs:134-205)
int derive_collect(const std::vector<std::pair<size_t, Track *>> &tracks, DeriveBatch *b) {
    if (!b->loud) return TH_OK;
    int rc = loudness_collect(b->loud.get(), false);
    if (rc != TH_OK) return rc;
    std::vector<unsigned long long> cnt(b->n_red);
    std::vector<uint32_t> bits(b->n_red);
    if (b->n_red) {
        const size_t o_bits = b->o_cnt + (b->n_red * 8 + 255) / 256 * 256;
        TH_HIP(hipMemcpy(cnt.data(), b->d_tab.get() + b->o_cnt, b->n_red * 8, hipMemcpyDeviceToHost));
        TH_HIP(hipMemcpy(bits.data(), b->d_tab.get() + o_bits, b->n_red * 4, hipMemcpyDeviceToHost));
    }
    for (auto &it : tracks) {
        Derived &d = b->of[it.first];
        if (!d.active) continue;
        loudness_result(*b->loud, d.loud_index, &d.stats);
        const size_t n_ch = it.second->ch.size();
        if (d.result == TH_GUARD_RESULT_BEFORE_CLIP) {  // from_wav_before_clip, per channel
            for (size_t k = 0; k < n_ch; k++) {
                float pk;
                std::memcpy(&pk, &bits[d.red0 + k], 4);
                th_guard_clip_stats st{};
                if (pk > 1.0f) {
                    st.max_reduction_gain_dB = db_from_amp(1.0f / pk);
                    st.reduction_cnt = cnt[d.red0 + k];
                }
                d.guard_stats.push_back(st);
            }
        } else if (d.result == TH_GUARD_RESULT_GLOBAL_GAIN) {  // from_global_gain, for every channel
            th_guard_clip_stats st{};
            st.max_reduction_gain_dB = db_from_amp(d.global_gain);
            d.guard_stats.assign(n_ch, st);
        } else {  // from_gain_seq of the one gain row
            th_guard_clip_stats st{};
            if (d.limiting) {
                float mn;
                std::memcpy(&mn, &bits[d.red0], 4);
                st.max_reduction_gain_dB = db_from_amp(mn);
                st.reduction_cnt = cnt[d.red0];
                d.gain_below_one = mn < 1.0f;
            }
            d.guard_stats.assign(1, st);
        }
    }
    b->loud.reset();  // (read: only the pools are kept for install_derived)
    b->d_scratch.reset();
    b->d_tab.reset();
    return TH_OK;
}

// the track takes its derived audio (or goes back to its original); the stream is idle
void install_derived(Track &tr, Derived &d) {
    tr.d_dyn = std::move(d.d_pool);
    for (size_t k = 0; k < tr.ch.size(); k++) {
        Channel &ch = tr.ch[k];
        ch.d_wav = d.active ? d.aud[k] : ch.d_orig;
        ch.d_draw = d.active ? d.draw[k] : ch.d_orig;
        ch.d_pyr = d.active ? d.pyr[k] : ch.d_pyr_orig;
    }
    tr.norm_gain = d.gain;
    tr.guard_result = d.result;
    tr.global_gain = d.global_gain;
    tr.d_gain = d.d_gain;
    tr.gain_below_one = d.gain_below_one;
    tr.stats = d.active ? d.stats : tr.orig_stats;
    if (d.active) tr.guard_stats = std::move(d.guard_stats);
    else tr.guard_stats.assign(tr.ch.size(), th_guard_clip_stats{});  // Audio::new: GlobalGain(1), default stats per channel
}

}  // namespace

// ---------------------------------------------------------------------------------------------- steps th_tmg drives per slot
// What a mutator has made beside the manager.  Every part is present or empty in its own right; commit() applies what is there.
// THE DISCARD RULE: a Staged that was not committed may still be read or written by work on either stream, so its destructor makes
// the manager's device current and drains the copy stream, then the context stream; only then do the members below free what
// they hold.  Nothing else in this file frees staged memory.  It runs on whatever thread drops the StagedPtr — under th_tmg the
// caller's, with another slot's device current.
struct th::tmi::Staged {
    th_tm *tm;
    bool committed = false;  // set by commit(): everything was moved out with both streams idle, nothing to wait for
    std::map<PlanKey, th_plan *> created;
    std::vector<NewSpec> fresh;
    std::map<size_t, Track> tracks;  // add_tracks
    std::set<size_t> added;          // ... and every id it was given
    std::unique_ptr<DeriveBatch> derive;  // set_common_normalize / set_common_guard_clipping; add_tracks under a normalise target
    std::unique_ptr<Setting> setting;     // set_setting
    explicit Staged(th_tm *m) : tm(m) {}
    ~Staged() {
        if (committed) return;
        (void)hipSetDevice(tm->ctx->device);
        (void)hipStreamSynchronize(tm->copy_stream);
        (void)hipStreamSynchronize(tm->ctx->stream);
        for (auto &kv : created) th_plan_destroy(kv.second);
    }
};

namespace {
using th::tmi::Staged;

// Derive `trs` (resident tracks, or the staged ones of an add) under stg.derive's settings and compute the spec of every channel
// whose audio changes, from the staged audio; ONE synchronisation, between the launches and the stats
int stage_derived(Staged &stg, const std::vector<std::pair<size_t, Track *>> &trs) {
    th_tm *tm = stg.tm;
    TH_CHECK(derive_enqueue(tm, trs, stg.derive.get()));
    std::vector<SpecInput> chans;
    for (auto &it : trs) {
        const Track &tr = *it.second;
        const Derived &d = stg.derive->of[it.first];
        // (a track with specs that is and stays its original is left alone: they would come out the same bits)
        if (!d.active && !tr.d_dyn && tr.ch[0].has_spec) continue;
        for (size_t k = 0; k < tr.ch.size(); k++)
            chans.push_back({it.first, (uint32_t)k, tr.sr, d.active ? d.aud[k] : tr.ch[k].d_orig, tr.ch[k].n});
    }
    TH_CHECK(compute_specs(tm, setting_of(tm), chans, stg.created, &stg.fresh));
    TH_HIP(hipStreamSynchronize(tm->ctx->stream));
    return derive_collect(trs, stg.derive.get());
}

// add_tracks arguments (th_tm_add_tracks), de-duplicated: of an id given twice the later one wins, as sequential adds would —
// only its data is uploaded
struct AddArgs {
    size_t n_tracks;
    const size_t *ids;
    const uint32_t *srs, *n_channels;
    const float *const *channels_flat;
    const size_t *n_samples;
    std::map<size_t, size_t> last_of;  // id -> the index that counts
    std::vector<size_t> flat0;         // track index -> its first entry of channels_flat
};
// What add_tracks leaves in flight until its one drain
struct AddInFlight {
    std::vector<PendingMinMax> pending;                // (min, max) pairs of every spec launch
    std::vector<std::unique_ptr<LoudnessBatch>> loud;  // one per group
    std::vector<std::pair<size_t, size_t>> loud_ids;   // (id, its group), in the order of the groups' descriptors
};

// groups of about 96 MB of samples (at least one track each): a group's launches cost ~0.2 ms of host time (descriptor tables,
// spec allocations: six groups of 32 MB were SLOWER than no pipeline, 6.0 against 5.1 ms for 32 tracks), the last group's
// kernels are the only ones nothing hides.  (Round 6, tried: the uploads on a helper thread so that this thread's launches do
// not hold up the copy engine — the launches then take 1.15 ms of host time instead of 0.67 and the call 5.2 instead of 4.9 ms:
// the runtime serialises the pageable copy path and the launches of the two threads.)
constexpr size_t GROUP_BYTES = (size_t)96 << 20;

// One group of an add, from track *t on: the tracks staged in stg.tracks (one pool each, uploads on the copy stream); then, on the
// context stream behind an event of the copy stream, their waveform pyramids, their loudness and, with normalise off, their specs
int stage_group(Staged &stg, const AddArgs &a, size_t *t, AddInFlight *fl, double *t_launch) {
    th_tm *tm = stg.tm;
    th_ctx *c = tm->ctx;
    std::vector<SpecInput> chans;
    std::vector<th_pyramid_desc> pdescs;
    std::vector<th_audio_desc> adescs;
    std::vector<std::vector<const float *>> aptrs;
    for (size_t bytes = 0; *t < a.n_tracks && (bytes == 0 || bytes < GROUP_BYTES); ++*t) {
        const size_t i = *t, id = a.ids[i], n = a.n_samples[i];
        if (a.last_of.at(id) != i) continue;
        Track &tr = stg.tracks[id];
        tr.sr = a.srs[i];
        tr.ch.resize(a.n_channels[i]);
        tr.guard_stats.assign(tr.ch.size(), th_guard_clip_stats{});
        const PoolLayout pl = pool_layout(n, 1);
        TH_HIP(tr.d_pool.alloc(pl.stride * tr.ch.size() * sizeof(float)));
        aptrs.emplace_back();
        for (uint32_t k = 0; k < a.n_channels[i]; k++) {
            Channel &ch = tr.ch[k];
            ch.n = n;
            ch.pyr_levels = pl.levels;
            ch.d_wav = ch.d_draw = ch.d_orig = tr.d_pool.get() + (size_t)k * pl.stride;
            ch.d_pyr = ch.d_pyr_orig = ch.d_wav + pl.wav_f;
            TH_HIP(hipMemcpyAsync(ch.d_wav, a.channels_flat[a.flat0[i] + k], n * sizeof(float), hipMemcpyHostToDevice, tm->copy_stream));
            bytes += n * sizeof(float);
            chans.push_back({id, k, tr.sr, ch.d_wav, n});
            pdescs.push_back(th_pyramid_desc{ch.d_wav, ch.d_pyr, n, ch.pyr_levels, PYR_FIRST});
            aptrs.back().push_back(ch.d_wav);
        }
        adescs.push_back(th_audio_desc{nullptr, (uint64_t)n, a.n_channels[i], a.srs[i], nullptr});
        fl->loud_ids.emplace_back(id, fl->loud.size());
    }
    if (chans.empty()) return TH_OK;
    const auto t0 = std::chrono::steady_clock::now();
    TH_HIP(hipEventRecord(tm->copy_ev, tm->copy_stream));
    TH_HIP(hipStreamWaitEvent(c->stream, tm->copy_ev, 0));
    TH_CHECK(th_waveform_pyramid_dev(c, pdescs.data(), pdescs.size()));
    // the group's loudness, behind its pyramid (read back after the one synchronisation)
    for (size_t i = 0; i < adescs.size(); i++) adescs[i].channels = aptrs[i].data();
    fl->loud.emplace_back(new LoudnessBatch);
    TH_CHECK(loudness_enqueue(c, adescs.data(), adescs.size(), true, true, fl->loud.back().get()));
    // (with a normalise target the specs come from the derived audio, which needs the stats first: stage_derived)
    if (tm->norm_kind == TH_NORM_OFF) TH_CHECK(compute_specs(tm, setting_of(tm), chans, stg.created, &stg.fresh, &fl->pending));
    *t_launch += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return TH_OK;
}

// after the drain: the (min, max) of every spec and the AudioStats of every staged track
int collect_added(Staged &stg, AddInFlight *fl) {
    TH_CHECK(finish_specs(fl->pending, &stg.fresh));
    for (size_t g = 0, i = 0; g < fl->loud.size(); g++) {
        TH_CHECK(loudness_collect(fl->loud[g].get(), false));
        for (size_t k = 0; i < fl->loud_ids.size() && fl->loud_ids[i].second == g; i++, k++) {
            Track &tr = stg.tracks[fl->loud_ids[i].first];
            loudness_result(*fl->loud[g], k, &tr.stats);
            tr.orig_stats = tr.stats;
        }
    }
    return TH_OK;
}

}  // namespace

namespace th {
namespace tmi {

void StagedDeleter::operator()(Staged *s) const { delete s; }

std::shared_mutex &rw_of(th_tm *tm) { return tm->rw; }

void list_extrema(th_tm *tm, std::vector<ChanExtremum> *out) {
    for (auto &kv : tm->tracks)
        for (size_t k = 0; k < kv.second.ch.size(); k++)
            if (kv.second.ch[k].has_spec) out->push_back(ChanExtremum{kv.first, (uint32_t)k, kv.second.ch[k].mn, kv.second.ch[k].mx});
}

void list_rates(th_tm *tm, std::vector<uint32_t> *out) {
    for (auto &kv : tm->tracks) out->push_back(kv.second.sr);
}

// Transactional: plans and specs of the NEW setting are made first, into fresh buffers; the manager's own state changes only
// in commit.  (The reference cannot fail here: realfft takes any even length.  This library plans every even n_fft up to
// TH_MAX_N_FFT (th_plan_create): 2^a * odd with odd <= 63 on the FFT kernels, any other odd factor through the chirp-z route.
// Only an n_fft above TH_MAX_N_FFT or a mel bank above 1 GiB is refused, and leaves everything as it was.)
int prepare_setting(th_tm *tm, double win_ms, uint32_t t_overlap, uint32_t f_overlap, int freq_scale, StagedPtr *out) {
    TH_HIP(hipSetDevice(tm->ctx->device));
    StagedPtr stg(new Staged(tm));
    stg->setting.reset(new Setting{win_ms, t_overlap, f_overlap, freq_scale});
    std::vector<SpecInput> chans;
    for (auto &kv : tm->tracks)
        for (size_t k = 0; k < kv.second.ch.size(); k++) chans.push_back({kv.first, (uint32_t)k, kv.second.sr, kv.second.ch[k].d_wav, kv.second.ch[k].n});
    TH_CHECK(compute_specs(tm, *stg->setting, chans, stg->created, &stg->fresh));
    *out = std::move(stg);
    return TH_OK;
}

// set_common_normalize / set_common_guard_clipping (track.rs:329-337,432-436): every track re-derived from its resident original
// into staged buffers, and the specs of every channel whose audio changes.
int prepare_dynamics(th_tm *tm, int kind, float target, int mode, StagedPtr *out) {
    TH_REQUIRE(kind == TH_NORM_OFF || kind == TH_NORM_LUFS || kind == TH_NORM_RMS_DB || kind == TH_NORM_PEAK_DB, "unknown normalize kind %d", kind);
    TH_REQUIRE(mode == TH_GUARD_CLIP || mode == TH_GUARD_REDUCE_GLOBAL_LEVEL || mode == TH_GUARD_LIMITER, "unknown guard-clipping mode %d", mode);
    TH_HIP(hipSetDevice(tm->ctx->device));
    StagedPtr stg(new Staged(tm));
    stg->derive.reset(new DeriveBatch);
    stg->derive->kind = kind;
    stg->derive->target = target;
    stg->derive->mode = mode;
    std::vector<std::pair<size_t, Track *>> trs;
    for (auto &kv : tm->tracks) trs.push_back({kv.first, &kv.second});
    TH_CHECK(stage_derived(*stg, trs));
    *out = std::move(stg);
    return TH_OK;
}

void get_common_dynamics(th_tm *tm, int *kind, float *target, int *mode) {
    if (kind) *kind = tm->norm_kind;
    if (target) *target = tm->norm_target;
    if (mode) *mode = tm->guard_mode;
}

int prepare_add(th_tm *tm, size_t n_tracks, const size_t *ids, const uint32_t *srs, const uint32_t *n_channels,
                const float *const *channels_flat, const size_t *n_samples, StagedPtr *out) {
    th_ctx *c = tm->ctx;
    TH_HIP(hipSetDevice(c->device));
    // Transactional: the new tracks are staged (audio upload, waveform pyramid, spec) beside the resident ones and
    // swapped in when everything has succeeded.  A failure drops the staging area (Staged's discard rule) and changes nothing.
    // Pipelined (round 6; the reference overlaps decode and calc_spec across rayon tasks, core/track.rs:211-239 -> core/mod.rs:
    // 153-163): the tracks go up in GROUPS on a copy stream of the manager's own; the waveform pyramids and the STFT of group g run
    // on the context stream (behind an event of the copy stream) while the host feeds group g + 1 to the copy engine — a pageable
    // source keeps the calling thread inside hipMemcpyAsync for the length of the transfer, so the kernels of the group before
    // cost nothing; nothing waits for the device until the end (one synchronisation, then the per-channel (min, max) read-back).
    // Inputs stay borrowed until the call returns.
    TH_REQUIRE(tm->copy_stream != nullptr && tm->copy_ev != nullptr, "manager without its copy stream");  // (th_tm_create)
    AddInFlight fl;  // (before stg: on an early return stg goes first, and drains both streams before these free anything)
    StagedPtr stg(new Staged(tm));
    const bool prof = getenv("TH_TM_PROF") != nullptr;
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tp0 = now();
    AddArgs a{n_tracks, ids, srs, n_channels, channels_flat, n_samples, {}, std::vector<size_t>(n_tracks, 0)};
    for (size_t t = 0, flat = 0; t < n_tracks; t++) {
        a.last_of[ids[t]] = t;
        a.flat0[t] = flat;
        flat += n_channels[t];
        stg->added.insert(ids[t]);
    }
    double t_launch = 0.0;
    for (size_t t = 0; t < n_tracks;) TH_CHECK(stage_group(*stg, a, &t, &fl, &t_launch));
    const double tp1 = now();
    TH_HIP(hipStreamSynchronize(tm->copy_stream));  // inputs are borrowed for this call only
    TH_HIP(hipStreamSynchronize(c->stream));
    int rc = collect_added(*stg, &fl);
    if (rc == TH_OK && tm->norm_kind != TH_NORM_OFF) {
        // track.normalize(common_normalize, common_guard_clipping) — track.rs:217, under the settings in force
        stg->derive.reset(new DeriveBatch);
        get_common_dynamics(tm, &stg->derive->kind, &stg->derive->target, &stg->derive->mode);
        std::vector<std::pair<size_t, Track *>> trs;
        for (auto &kv : stg->tracks) trs.push_back({kv.first, &kv.second});
        rc = stage_derived(*stg, trs);
    }
    if (prof) fprintf(stderr, "th_tm_add_tracks prof: staging + launches %.2f ms (of which pyramid / STFT launches %.2f), drain %.2f\n", tp1 - tp0, t_launch, now() - tp1);
    if (rc != TH_OK) return rc;
    *out = std::move(stg);
    return TH_OK;
}

// Reached with the context stream and the copy stream idle; cannot fail.  One sequence: whatever part is present is applied.
void commit(th_tm *tm, StagedPtr s) {
    (void)hipSetDevice(tm->ctx->device);
    // re-adding an id replaces it (reload_tracks, core/mod.rs:73-82): the old track's buffers go with the assignment
    for (auto &kv : s->tracks) tm->tracks[kv.first] = std::move(kv.second);
    if (s->derive) {
        tm->norm_kind = s->derive->kind;
        tm->norm_target = s->derive->target;
        tm->guard_mode = s->derive->mode;
        for (auto &kv : s->derive->of) install_derived(tm->tracks.find(kv.first)->second, kv.second);
    }
    for (auto &kv : s->created) tm->plans[kv.first] = kv.second;
    for (NewSpec &n : s->fresh) {
        Channel &ch = *find_channel(tm, n.id, n.ch);
        ch.d_spec = std::move(n.d_spec);
        ch.T = n.T;
        ch.H = n.H;
        ch.spec_pitch = n.pitch;
        ch.mn = n.mn;
        ch.mx = n.mx;
        ch.has_spec = true;
    }
    if (s->setting) {
        tm->win_ms = s->setting->win_ms;
        tm->t_overlap = s->setting->t_overlap;
        tm->f_overlap = s->setting->f_overlap;
        tm->freq_scale = s->setting->freq_scale;
        retain_plans(tm);  // spec_analyzer.retain(...)  core/mod.rs:111-112; add_tracks does not prune (:62-71)
    }
    tm->no_spec_img_ids.insert(tm->no_spec_img_ids.end(), s->added.begin(), s->added.end());  // core/mod.rs:70
    s->committed = true;
}

int requantise(th_tm *tm, const DbRange *global, bool force_update_all, bool images_only, std::vector<size_t> *updated) {
    TH_HIP(hipSetDevice(tm->ctx->device));
    const int rc = update_spec_imgs(tm, force_update_all, updated, global);
    return images_only ? writer_done_images(tm, rc) : writer_done(tm, rc);
}

int set_colormap_only(th_tm *tm, const uint8_t *rgba, size_t bytes) {
    TH_HIP(hipSetDevice(tm->ctx->device));
    // RenderTileCache::set_colormap keeps the old map for malformed input — render_tiles.rs:80-85
    if (bytes >= 4 && bytes % 4 == 0) {
        tm->colormap_rgba.assign(rgba, rgba + bytes);
        int rc = upload_colormap(tm);
        if (rc != TH_OK) return rc;
    }
    // init: TM.set_colormap_length(len / 4) — lib.rs:61, core/mod.rs:128-131 (its update_spec_imgs(force) is the caller's)
    tm->colormap_length = (uint32_t)(bytes / 4);
    return TH_OK;
}

int settle(th_tm *tm) {
    TH_HIP(hipSetDevice(tm->ctx->device));
    return writer_done(tm, TH_OK);
}

}  // namespace tmi
}  // namespace th

// ---------------------------------------------------------------------------------------------- normalise + clip guard: the entries
namespace {
int set_common_dynamics(th_tm *tm, int kind, float target, int mode) {
    tmi::StagedPtr staged;
    int rc = tmi::prepare_dynamics(tm, kind, target, mode, &staged);
    if (rc != TH_OK) return rc;
    tmi::commit(tm, std::move(staged));
    std::vector<size_t> upd;
    rc = update_spec_imgs(tm, true, &upd);  // update_all_specs_imgs (forced)
    tm->invalidate_all();
    return writer_done(tm, rc);
}
}  // namespace

TH_API int th_tm_set_common_normalize(th_tm *tm, int kind, float target) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    return set_common_dynamics(tm, kind, target, tm->guard_mode);
    TH_CATCH
}

TH_API int th_tm_set_common_guard_clipping(th_tm *tm, int mode) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    return set_common_dynamics(tm, tm->norm_kind, tm->norm_target, mode);
    TH_CATCH
}

TH_API int th_tm_get_common_dynamics(th_tm *tm, int *kind, float *target, int *mode) {
    TH_TRY
    TH_REQUIRE(tm, "tm is NULL");
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    tmi::get_common_dynamics(tm, kind, target, mode);
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_get_track_dynamics(th_tm *tm, size_t id, th_track_dynamics *out) {
    TH_TRY
    TH_REQUIRE(tm && out, "NULL argument");
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    auto it = tm->tracks.find(id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", id);
    const Track &tr = it->second;
    *out = th_track_dynamics{};
    out->normalize_gain = tr.norm_gain;
    out->guard_result = tr.guard_result;
    out->global_gain = tr.global_gain;
    out->draws_before_clip = tr.guard_result == TH_GUARD_RESULT_BEFORE_CLIP;
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_get_guard_clip_stats(th_tm *tm, size_t id, th_guard_clip_stats *out, size_t cap, size_t *n) {
    TH_TRY
    TH_REQUIRE(tm && n, "NULL argument");
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    auto it = tm->tracks.find(id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", id);
    const std::vector<th_guard_clip_stats> &gs = it->second.guard_stats;
    // format_guard_clip_stats (audio.rs:94-111): every channel's entry under Clip, else the first
    *n = tm->guard_mode == TH_GUARD_CLIP ? gs.size() : std::min<size_t>(1, gs.size());
    if (cap < *n || (*n && !out)) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu entries", *n);
    for (size_t i = 0; i < *n; i++) out[i] = gs[i];
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_get_limiter_gain(th_tm *tm, size_t id, float *out, size_t cap, size_t *n) {
    TH_TRY
    TH_REQUIRE(tm && n, "NULL argument");
    std::unique_lock<std::shared_mutex> wl(tm->rw);  // uses the context stream: exclusive, like th_tm_copy_spec
    TH_HIP(hipSetDevice(tm->ctx->device));
    auto it = tm->tracks.find(id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", id);
    const Track &tr = it->second;
    // guard_clipping_gain (audio.rs:80-92)
    const bool seq = tr.guard_result == TH_GUARD_RESULT_GAIN_SEQUENCE, full = seq && tr.d_gain && tr.gain_below_one;
    *n = !seq ? 0 : full ? tr.ch[0].n : 1;
    if (cap < *n || (*n && !out)) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu floats", *n);
    if (full) {
        TH_HIP(hipMemcpyAsync(out, tr.d_gain, *n * sizeof(float), hipMemcpyDeviceToHost, tm->ctx->stream));
        TH_HIP(hipStreamSynchronize(tm->ctx->stream));
    } else if (seq) {
        out[0] = 1.0f;
    }
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_copy_audio(th_tm *tm, size_t id, uint32_t ch, int which, float *out, size_t cap) {
    TH_TRY
    TH_REQUIRE(tm && out, "NULL argument");
    TH_REQUIRE(which >= 0 && which <= 2, "which must be 0 (audio), 1 (drawn) or 2 (original)");
    std::unique_lock<std::shared_mutex> wl(tm->rw);
    TH_HIP(hipSetDevice(tm->ctx->device));
    Channel *c = find_channel(tm, id, ch);
    if (!c) return fail(TH_ERR_NOT_FOUND, "Track %zu channel %u does not exist", id, ch);
    if (cap < c->n) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu floats", c->n);
    const float *src = which == 0 ? c->d_wav : which == 1 ? c->d_draw : c->d_orig;
    TH_HIP(hipMemcpyAsync(out, src, c->n * sizeof(float), hipMemcpyDeviceToHost, tm->ctx->stream));
    TH_HIP(hipStreamSynchronize(tm->ctx->stream));
    return TH_OK;
    TH_CATCH
}

// ---------------------------------------------------------------------------------------------- PCM / WAV export
// th_tm_export_pcm / th_tm_export_wav: a reader.  The requests are cut into PIECES of at most TH_EXPORT_PIECE_BYTES staged bytes (at
// frame boundaries); a piece is one launch of kernels_export.hip into one of the slot's two staging buffers and one copy per
// contiguous run of output bytes into the caller's buffer, on the slot's copy stream, while the next piece is computed.  The bytes in
// staging sit at the same address modulo 16 as in the caller's image, so a run is one copy.
namespace {
// the check of one request; *info: the track, the resampler of a request that leaves the track's rate, the sample range at info->sr
int check_export_request(th_tm *tm, const tmi::ExportReq &ar, size_t i, tmi::ExportInfo *info) {
    const th_export_request &r = ar.base;
    auto it = tm->tracks.find(r.id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", r.id);
    const Track &tr = it->second;
    TH_REQUIRE(r.which <= 2, "request %zu: which must be 0 (audio), 1 (drawn) or 2 (original)", i);
    TH_REQUIRE(r.format <= TH_PCM_F32, "request %zu: unknown format %u", i, r.format);
    TH_REQUIRE(r.dither <= TH_DITHER_TPDF, "request %zu: unknown dither %u", i, r.dither);
    size_t n = tr.ch.empty() ? 0 : tr.ch[0].n;
    *info = tmi::ExportInfo{};
    info->sr = tr.sr;
    if (ar.sr_out != 0 && ar.sr_out != tr.sr) {
        const int rc = resample_plan(tr.sr, ar.sr_out, &info->plan);
        TH_REQUIRE(rc != 1, "request %zu: Track %zu has no sample rate", i, r.id);
        if (rc != 0 || !resample_n_out(n, info->plan, &info->n_out))
            return fail(TH_ERR_UNSUPPORTED, "request %zu: %u -> %u Hz is beyond the resampler's limits (%u taps, %u coefficients, 64-bit indices)",
                        i, tr.sr, ar.sr_out, TH_RESAMPLE_MAX_TAPS, TH_RESAMPLE_MAX_COEFS);
        n = info->n_out;
        info->sr = ar.sr_out;
    }
    if (ar.has_band) {
        const int rc = band_plan_for(tr.sr, ar.mode, ar.f_lo_hz, ar.f_hi_hz, ar.trans_hz, &info->band);
        TH_REQUIRE(rc != 1, "request %zu: bad band (mode %u, [%g, %g] Hz, transition %g Hz) at %u Hz", i, ar.mode, ar.f_lo_hz, ar.f_hi_hz,
                   ar.trans_hz, tr.sr);
        if (rc != 0)
            return fail(TH_ERR_UNSUPPORTED, "request %zu: a transition of %g Hz at %u Hz needs more than %u taps", i, ar.trans_hz, tr.sr,
                        TH_BAND_MAX_TAPS);
    }
    size_t s0 = 0, s1 = 0;
    TH_REQUIRE(spectrum_frame_range(info->sr, 1, n, r.start_sec, r.end_sec, &s0, &s1), "request %zu: bad time range [%g, %g) s", i,
               r.start_sec, r.end_sec);
    if (tr.ch.empty() || tr.ch.size() > TH_EXPORT_MAX_CHANNELS)
        return fail(TH_ERR_UNSUPPORTED, "Track %zu: %zu channels (1 .. %d can be exported)", r.id, tr.ch.size(), TH_EXPORT_MAX_CHANNELS);
    info->sample_start = s0;
    info->sample_end = s1;
    info->track = &tr;
    return TH_OK;
}

// both streams of a slot idle before the call's host memory goes away (also on an error path)
struct ExportDrain {
    ReaderSlot *sl;
    ~ExportDrain() {
        (void)hipStreamSynchronize(sl->stream);
        if (sl->exp_copy) (void)hipStreamSynchronize(sl->exp_copy);
    }
};

// One of the slot's export buffers grows to hold `need` elements: `floor` doubled until it does, at most `ceil`.  The stream that
// uses it (and `also`, when a second one does) is idle before the old buffer goes; the capacity is 0 while the allocation is pending
template <class T>
int grow_export_buf(ReaderSlot &sl, DeviceBuf<T> &buf, size_t &cap, size_t need, size_t floor, size_t ceil, hipStream_t also) {
    if (need <= cap) return TH_OK;
    size_t want = floor;
    while (want < need) want <<= 1;
    want = std::min(want, ceil);
    TH_HIP(hipStreamSynchronize(sl.stream));
    if (also) TH_HIP(hipStreamSynchronize(also));
    cap = 0;
    TH_HIP(buf.alloc(want * sizeof(T)));
    cap = want;
    return TH_OK;
}

// the slot's coefficient table becomes that of (sr_in, sr_out): built on the host (host_math.h resample_table, the rows
// th_resample_coefs returns) into *host, which must outlive the upload, and sent on the slot's stream
int ensure_resample_table(ReaderSlot &sl, uint32_t sr_in, uint32_t sr_out, const th_resample_plan &plan, std::vector<float> *host) {
    if (sl.rs_sr_in == sr_in && sl.rs_sr_out == sr_out) return TH_OK;
    const size_t floats = (size_t)plan.L * 2 * plan.half_taps;
    host->resize(floats);
    resample_table(plan, host->data());
    sl.rs_sr_in = sl.rs_sr_out = 0;
    TH_CHECK(grow_export_buf(sl, sl.rs_table, sl.rs_table_cap, floats, floats, floats, nullptr));  // (exactly the table)
    TH_HIP(hipMemcpyAsync(sl.rs_table.get(), host->data(), floats * sizeof(float), hipMemcpyHostToDevice, sl.stream));
    sl.rs_sr_in = sr_in;
    sl.rs_sr_out = sr_out;
    return TH_OK;
}

// the slot's filter row becomes that of (sr, band): built on the host (host_math.h band_row, the row th_band_coefs returns) into
// *host, which must outlive the upload, and sent on the slot's stream
int ensure_band_table(ReaderSlot &sl, uint32_t sr, const th_band_plan &band, std::vector<float> *host) {
    if (sl.band_sr == sr && same_band(sl.band, band)) return TH_OK;
    const size_t floats = 2 * (size_t)band.half_taps;
    host->resize(floats);
    band_row(sr, band, nullptr, host->data());
    sl.band_sr = 0;
    TH_CHECK(grow_export_buf(sl, sl.band_table, sl.band_table_cap, floats, floats, floats, nullptr));  // (exactly the row)
    TH_HIP(hipMemcpyAsync(sl.band_table.get(), host->data(), floats * sizeof(float), hipMemcpyHostToDevice, sl.stream));
    sl.band_sr = sr;
    sl.band = band;
    return TH_OK;
}
}  // namespace

namespace th {
namespace tmi {
int wav_header_checked(uint32_t format, uint32_t sr, uint32_t n_ch, uint64_t n_frames, uint8_t out[TH_WAV_HEADER_MAX], size_t *header_len,
                       size_t *pad_len) {
    TH_REQUIRE(out && header_len && pad_len, "NULL argument");
    TH_REQUIRE(format <= TH_PCM_F32, "unknown format %u", format);
    const int rc = wav_header(export_bytes_per_sample(format), sr, n_ch, n_frames, out, header_len, pad_len);
    TH_REQUIRE(rc != 1, "a WAV file needs at least one channel and a sample rate (%u channels at %u Hz)", n_ch, sr);
    if (rc != 0) return fail(TH_ERR_UNSUPPORTED, "%llu frames of %u channels at %u Hz do not fit a RIFF / WAV header",
                             (unsigned long long)n_frames, n_ch, sr);
    return TH_OK;
}

int export_request_info(th_tm *tm, const ExportReq &r, size_t i, ExportInfo *info) {
    TH_CHECK(check_export_request(tm, r, i, info));
    info->n_channels = (uint32_t)static_cast<const Track *>(info->track)->ch.size();
    info->n_bytes = (uint64_t)(info->sample_end - info->sample_start) * info->n_channels * export_bytes_per_sample(r.base.format);
    info->req = r.base;
    return TH_OK;
}

size_t ExportReader::layout(ExportInfo *info, size_t n) {
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        info[i].offset = at;
        const uint64_t end = at + info[i].n_bytes;
        at = (end + 15) & ~(uint64_t)15;
        info[i].pad = i + 1 < n ? (uint32_t)(at - end) : 0u;
        if (i + 1 == n) at = end;
    }
    return (size_t)at;
}

// plan_export (reader_plan.h) cuts the requests into pieces and bind_export gives the jobs their addresses; what is left here is the
// slot, its buffers, the upload and the pipeline of the two streams
int export_run(th_tm *tm, size_t n, ExportInfo *info, uint8_t *out) {
    std::vector<ExportPlanRequest> prs(n);
    std::vector<const float *> chan;
    for (size_t i = 0; i < n; i++) {
        const th_export_request &r = info[i].req;
        const Track &tr = *static_cast<const Track *>(info[i].track);
        ExportPlanRequest &pr = prs[i];
        pr.n_ch = info[i].n_channels;
        pr.sr_in = tr.sr;
        pr.sr_out = info[i].sr;
        pr.n_in = tr.ch[0].n;
        pr.plan = info[i].plan;
        pr.n_out = info[i].n_out;
        pr.band = info[i].band;
        pr.format = r.format;
        pr.dither = r.dither;
        pr.seed = r.seed;
        pr.s0 = info[i].sample_start;
        pr.s1 = info[i].sample_end;
        pr.offset = info[i].offset;
        pr.pad = info[i].pad;
        for (const Channel &c : tr.ch) chan.push_back(r.which == 0 ? c.d_wav : r.which == 1 ? c.d_draw : c.d_orig);
        info[i].n_clamped = info[i].n_nan = 0;
    }
    ExportPlan pl = plan_export(prs.data(), n);
    if (pl.err != TH_OK) return fail(pl.err, "%s", pl.err_text.c_str());
    const std::vector<ExportPiece> &pieces = pl.pieces;
    if (pieces.empty()) return TH_OK;

    TH_HIP(hipSetDevice(tm->ctx->device));
    SlotLease lease{tm, nullptr};
    int rc = acquire_slot(tm, &lease.slot);
    if (rc != TH_OK) return rc;
    ReaderSlot &sl = *lease.slot;
    if (!sl.exp_copy) {
        TH_HIP(hipStreamCreateWithFlags(&sl.exp_copy, hipStreamNonBlocking));
        for (int b = 0; b < 2; b++) {
            TH_HIP(hipEventCreateWithFlags(&sl.exp_done[b], hipEventDisableTiming));
            TH_HIP(hipEventCreateWithFlags(&sl.exp_copied[b], hipEventDisableTiming));
        }
    }
    std::vector<std::vector<float>> host_tables(pieces.size()), host_rows(pieces.size());  // (behind the drain: alive until the uploads are done)
    ExportDrain drain{&sl};
    for (int b = 0; b < 2; b++)  // powers of two from 1 MiB, never above one piece; the copy stream reads them too
        TH_CHECK(grow_export_buf(sl, sl.exp_stage[b], sl.exp_stage_cap[b], pl.stage_need[b], 1 << 20, EXPORT_STAGE_MAX, sl.exp_copy));
    // (floats) powers of two from 1 MiB, never above the bound
    TH_CHECK(grow_export_buf(sl, sl.rs_scratch, sl.rs_scratch_cap, pl.scratch_need, 1 << 18, RESAMPLE_SCRATCH_MAX / sizeof(float), nullptr));
    // one table for the whole call: the export jobs of every piece, the resampler's jobs, the band filter's, then the channel pointers
    TH_CHECK(sl.exp_tab.ensure(pl.tab_bytes));
    TH_CHECK(sl.exp_cnt.ensure(n * 2 * sizeof(unsigned long long)));
    unsigned char *d_tab = static_cast<unsigned char *>(sl.exp_tab.dptr);
    unsigned long long *d_cnt = static_cast<unsigned long long *>(sl.exp_cnt.dptr);
    const std::vector<unsigned char> tab =
        bind_export(pl, ExportBases{{sl.exp_stage[0].get(), sl.exp_stage[1].get()}, sl.rs_scratch.get(), d_tab, d_cnt}, chan.data());
    TH_CHECK(sl.exp_tab.upload(sl.stream, tab.data(), tab.size()));
    TH_HIP(hipMemsetAsync(d_cnt, 0, n * 2 * sizeof(unsigned long long), sl.stream));
    const ExportJob *d_jobs = reinterpret_cast<const ExportJob *>(d_tab);
    const ResampleJob *d_rjobs = reinterpret_cast<const ResampleJob *>(d_tab + pl.o_rjobs);
    const BandJob *d_bjobs = reinterpret_cast<const BandJob *>(d_tab + pl.o_bjobs);
    auto launch_piece = [&](size_t p) -> int {
        const ExportPiece &pc = pieces[p];
        if (pc.n_rblocks) {  // (the stream's order keeps the scratch and the table from the last piece's readers)
            TH_CHECK(ensure_resample_table(sl, pc.sr_in, pc.sr_out, pc.plan, &host_tables[p]));
            TH_HIP(launch_resample(d_rjobs + pc.rjob0, (uint32_t)(pc.rjob1 - pc.rjob0), pc.n_rblocks, sl.rs_table.get(), resample_tiling(pc.plan), sl.stream));
        }
        if (pc.n_bblocks) {
            TH_CHECK(ensure_band_table(sl, pc.band_sr, pc.band, &host_rows[p]));
            TH_HIP(launch_band(d_bjobs + pc.bjob0, (uint32_t)(pc.bjob1 - pc.bjob0), pc.n_bblocks, sl.band_table.get(), band_tiling(pc.band), sl.stream));
        }
        if (p >= 2) TH_HIP(hipStreamWaitEvent(sl.stream, sl.exp_copied[p & 1], 0));  // (the buffer's last piece has left it)
        TH_HIP(launch_export(d_jobs + pc.job0, (uint32_t)(pc.job1 - pc.job0), pc.n_chunks, sl.stream));
        TH_HIP(hipEventRecord(sl.exp_done[p & 1], sl.stream));
        return TH_OK;
    };
    TH_CHECK(launch_piece(0));
    for (size_t p = 0; p < pieces.size(); p++) {
        if (p + 1 < pieces.size()) TH_CHECK(launch_piece(p + 1));  // (ahead of the copy: a copy into pageable memory holds the host)
        TH_HIP(hipStreamWaitEvent(sl.exp_copy, sl.exp_done[p & 1], 0));
        for (const ExportRun &run : pieces[p].runs)
            TH_HIP(hipMemcpyAsync(out + run.out_at, sl.exp_stage[p & 1].get() + run.stage_at, run.bytes, hipMemcpyDeviceToHost, sl.exp_copy));
        TH_HIP(hipEventRecord(sl.exp_copied[p & 1], sl.exp_copy));
    }
    std::vector<unsigned long long> cnt(n * 2);
    TH_HIP(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, sl.stream));
    TH_HIP(hipStreamSynchronize(sl.stream));
    TH_HIP(hipStreamSynchronize(sl.exp_copy));
    for (size_t i = 0; i < n; i++) {
        info[i].n_clamped = cnt[2 * i];
        info[i].n_nan = cnt[2 * i + 1];
    }
    return TH_OK;
}
}  // namespace tmi
}  // namespace th

namespace {
int export_pcm_any(th_tm *tm, const tmi::ExportReq *reqs, size_t n, uint8_t *out, size_t cap, th_export_info *info, size_t *out_len) {
    return br::batched_read<tmi::ExportReader>(TmReaders{tm}, reqs, n, out, cap, info, out_len);
}

int export_wav_any(th_tm *tm, const tmi::ExportReq *req, uint8_t *out, size_t cap, th_export_info *info, size_t *out_len) {
    TH_REQUIRE(tm && req && out_len, "NULL argument");
    *out_len = 0;
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    tmi::ExportInfo one{};
    TH_CHECK(tmi::export_request_info(tm, *req, 0, &one));
    one.waveform_revision = tm->waveform_revision();
    uint8_t hdr[TH_WAV_HEADER_MAX];
    size_t hl = 0, pl = 0;
    TH_CHECK(tmi::wav_header_checked(req->base.format, one.sr, one.n_channels, one.sample_end - one.sample_start, hdr, &hl, &pl));
    one.offset = hl;
    const size_t total = hl + (size_t)one.n_bytes + pl;
    if (info) *info = one;
    *out_len = total;
    if (cap < total || !out) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu bytes", total);
    TH_CHECK(tmi::export_run(tm, 1, &one, out));
    std::memcpy(out, hdr, hl);
    if (pl) out[hl + one.n_bytes] = 0;
    if (info) *info = one;
    return TH_OK;
}
}  // namespace

TH_API int th_tm_export_pcm(th_tm *tm, const th_export_request *reqs, size_t n, uint8_t *out, size_t cap, th_export_info *info,
                            size_t *out_len) {
    TH_TRY
    TH_REQUIRE(n == 0 || reqs, "NULL argument");
    return export_pcm_any(tm, tmi::export_requests(reqs, n).data(), n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_export_wav(th_tm *tm, const th_export_request *req, uint8_t *out, size_t cap, th_export_info *info, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(req, "NULL argument");
    const tmi::ExportReq one = tmi::export_req(*req);
    return export_wav_any(tm, &one, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_export_pcm_at(th_tm *tm, const th_export_at_request *reqs, size_t n, uint8_t *out, size_t cap, th_export_info *info,
                               size_t *out_len) {
    TH_TRY
    TH_REQUIRE(n == 0 || reqs, "NULL argument");
    return export_pcm_any(tm, tmi::export_requests(reqs, n).data(), n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_export_wav_at(th_tm *tm, const th_export_at_request *req, uint8_t *out, size_t cap, th_export_info *info, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(req, "NULL argument");
    const tmi::ExportReq one = tmi::export_req(*req);
    return export_wav_any(tm, &one, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_export_pcm_band(th_tm *tm, const th_export_band_request *reqs, size_t n, uint8_t *out, size_t cap, th_export_info *info,
                                 size_t *out_len) {
    TH_TRY
    TH_REQUIRE(n == 0 || reqs, "NULL argument");
    return export_pcm_any(tm, tmi::export_requests(reqs, n).data(), n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_export_wav_band(th_tm *tm, const th_export_band_request *req, uint8_t *out, size_t cap, th_export_info *info,
                                 size_t *out_len) {
    TH_TRY
    TH_REQUIRE(req, "NULL argument");
    const tmi::ExportReq one = tmi::export_req(*req);
    return export_wav_any(tm, &one, out, cap, info, out_len);
    TH_CATCH
}

// ---------------------------------------------------------------------------------------------- FLAC export
// th_tm_export_flac: a reader.  plan_flac (flac_plan.h) cuts the requests into pieces of whole blocks and bind_flac gives the jobs
// their addresses; what is left here is the slot, its buffers, the upload and the pipeline of the two streams: per piece the three
// launches of kernels_flac.hip into staging buffer p & 1, the jobs' lengths read back on the copy stream, then one copy per job to
// where its request's file has got to, while the next piece is encoded.  The host writes the 42 header bytes of each file last.
namespace th {
namespace tmi {
int flac_request_info(th_tm *tm, const th_export_request &r, uint32_t flags, size_t i, ExportInfo *info) {
    // (where the export checks the format: behind the track and `which`)
    if (tm->tracks.count(r.id) && r.which <= 2) {
        TH_REQUIRE(r.format != TH_PCM_F32, "request %zu: FLAC is TH_PCM_S16 or TH_PCM_S24", i);
        TH_REQUIRE((flags & ~FLAC_FLAGS) == 0, "request %zu: unknown FLAC flags (TH_FLAC_LPC | TH_FLAC_STEREO)", i);
    }
    TH_CHECK(export_request_info(tm, export_req(r), i, info));
    info->flac_flags = flags;
    const uint64_t frames = info->sample_end - info->sample_start;
    TH_CHECK(flac_stream_checked(info->sr, info->n_channels, r.format, frames));
    info->n_bytes = flac_stream_bound(frames, info->n_channels, flac_bps(r.format));
    return TH_OK;
}

size_t flac_layout(ExportInfo *info, size_t n) {
    uint64_t at = 0, end = 0;
    for (size_t i = 0; i < n; i++) {
        info[i].offset = at;
        info[i].pad = 0;
        end = at + info[i].n_bytes;
        at = (end + 15) & ~(uint64_t)15;
    }
    return (size_t)end;
}

namespace {
struct FlacProgress {  // per request: the file's length so far, its smallest and largest frame
    uint64_t at = FLAC_STREAM_HEADER;
    uint32_t mn = 0xffffffffu, mx = 0;
};
int flac_run_pieces(th_tm *tm, FlacPlan &pl, const std::vector<FlacPlanRequest> &prs, const std::vector<const float *> &chan, ExportInfo *info,
                    uint8_t *out, std::vector<FlacProgress> &prog) {
    const size_t n = prs.size();
    const std::vector<FlacPiece> &pieces = pl.pieces;
    TH_HIP(hipSetDevice(tm->ctx->device));
    SlotLease lease{tm, nullptr};
    int rc = acquire_slot(tm, &lease.slot);
    if (rc != TH_OK) return rc;
    ReaderSlot &sl = *lease.slot;
    if (!sl.exp_copy) {
        TH_HIP(hipStreamCreateWithFlags(&sl.exp_copy, hipStreamNonBlocking));
        for (int b = 0; b < 2; b++) {
            TH_HIP(hipEventCreateWithFlags(&sl.exp_done[b], hipEventDisableTiming));
            TH_HIP(hipEventCreateWithFlags(&sl.exp_copied[b], hipEventDisableTiming));
        }
    }
    std::vector<FlacJobResult> res(pl.runs.size());  // (behind the drain: alive until the copies are done)
    ExportDrain drain{&sl};
    for (int b = 0; b < 2; b++)
        TH_CHECK(grow_export_buf(sl, sl.exp_stage[b], sl.exp_stage_cap[b], pl.stage_need[b], 1 << 20, EXPORT_STAGE_MAX, sl.exp_copy));
    // (words) powers of two from 1 MiB, never above a piece's bound and a word per unit (a slot is its subframe's verbatim size
    // rounded up to a word: the planner cannot ask for more); a stereo block's four units of bps + 1 bits are at most 4 x 17 / (2 x 16)
    // of the block's bound: three pieces' worth
    bool four_units = false;
    for (const FlacPlanRequest &r : prs) four_units |= flac_units_per_block(r.n_ch, r.flags) != r.n_ch;
    const size_t slot_ceil = (size_t)TH_EXPORT_PIECE_BYTES / 4 * (four_units ? 3 : 1) + 2 * (size_t)FLAC_PIECE_MAX_UNITS;
    if (pl.slot_need > slot_ceil || pl.stage_need[0] > EXPORT_STAGE_MAX || pl.stage_need[1] > EXPORT_STAGE_MAX)
        return fail(TH_ERR_INTERNAL, "a FLAC piece of %llu slot words and %llu / %llu staged bytes is beyond the slot's bounds",
                    (unsigned long long)pl.slot_need, (unsigned long long)pl.stage_need[0], (unsigned long long)pl.stage_need[1]);
    TH_CHECK(grow_export_buf(sl, sl.flac_slots, sl.flac_slots_cap, pl.slot_need, 1 << 18, slot_ceil, nullptr));
    const size_t o_foff = (size_t)pl.unit_need * 4, o_res = (o_foff + (size_t)pl.block_need * 4 + 15) & ~(size_t)15;
    TH_CHECK(sl.flac_aux.ensure(o_res + pl.runs.size() * sizeof(FlacJobResult)));
    TH_CHECK(sl.flac_tab.ensure(pl.tab_bytes));
    TH_CHECK(sl.exp_cnt.ensure(n * 2 * sizeof(unsigned long long)));
    unsigned char *d_tab = static_cast<unsigned char *>(sl.flac_tab.dptr), *d_aux = static_cast<unsigned char *>(sl.flac_aux.dptr);
    unsigned long long *d_cnt = static_cast<unsigned long long *>(sl.exp_cnt.dptr);
    FlacJobResult *d_res = reinterpret_cast<FlacJobResult *>(d_aux + o_res);
    const std::vector<unsigned char> tab =
        bind_flac(pl, FlacBases{{sl.exp_stage[0].get(), sl.exp_stage[1].get()}, sl.flac_slots.get(), reinterpret_cast<uint32_t *>(d_aux),
                                reinterpret_cast<uint32_t *>(d_aux + o_foff), d_res, d_tab, d_cnt}, prs.data(), n, chan.data());
    TH_CHECK(sl.flac_tab.upload(sl.stream, tab.data(), tab.size()));
    TH_HIP(hipMemsetAsync(d_cnt, 0, n * 2 * sizeof(unsigned long long), sl.stream));
    const FlacJob *d_jobs = reinterpret_cast<const FlacJob *>(d_tab);
    auto launch_piece = [&](size_t p) -> int {
        const FlacPiece &pc = pieces[p];
        const uint32_t nj = (uint32_t)(pc.run1 - pc.run0);
        if (p >= 2) TH_HIP(hipStreamWaitEvent(sl.stream, sl.exp_copied[p & 1], 0));  // (the buffer's last piece has left it)
        TH_HIP(launch_flac_subframes(d_jobs + pc.run0, nj, pc.n_units, prs[0].flags, sl.stream));  // (one call, one flags value)
        TH_HIP(launch_flac_scan(d_jobs + pc.run0, nj, sl.stream));
        TH_HIP(launch_flac_frames(d_jobs + pc.run0, nj, pc.n_blocks, sl.stream));
        TH_HIP(hipEventRecord(sl.exp_done[p & 1], sl.stream));
        return TH_OK;
    };
    TH_CHECK(launch_piece(0));
    for (size_t p = 0; p < pieces.size(); p++) {
        const FlacPiece &pc = pieces[p];
        if (p + 1 < pieces.size()) TH_CHECK(launch_piece(p + 1));  // (ahead of the read-back, which holds the host)
        TH_HIP(hipStreamWaitEvent(sl.exp_copy, sl.exp_done[p & 1], 0));
        TH_HIP(hipMemcpyAsync(res.data() + pc.run0, d_res + pc.run0, (pc.run1 - pc.run0) * sizeof(FlacJobResult), hipMemcpyDeviceToHost, sl.exp_copy));
        TH_HIP(hipStreamSynchronize(sl.exp_copy));
        for (size_t k = pc.run0; k < pc.run1; k++) {
            const FlacRun &run = pl.runs[k];
            FlacProgress &pg = prog[run.req];
            if (res[k].bytes > run.bound || pg.at + res[k].bytes > info[run.req].n_bytes)
                return fail(TH_ERR_INTERNAL, "request %zu: a FLAC job of %llu bytes against a bound of %llu", run.req, res[k].bytes,
                            (unsigned long long)run.bound);
            TH_HIP(hipMemcpyAsync(out + info[run.req].offset + pg.at, sl.exp_stage[p & 1].get() + run.stage_at, res[k].bytes, hipMemcpyDeviceToHost,
                                  sl.exp_copy));
            pg.at += res[k].bytes;
            pg.mn = std::min(pg.mn, res[k].min_frame);
            pg.mx = std::max(pg.mx, res[k].max_frame);
        }
        TH_HIP(hipEventRecord(sl.exp_copied[p & 1], sl.exp_copy));
    }
    std::vector<unsigned long long> cnt(n * 2);
    TH_HIP(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, sl.stream));
    TH_HIP(hipStreamSynchronize(sl.stream));
    TH_HIP(hipStreamSynchronize(sl.exp_copy));
    for (size_t i = 0; i < n; i++) {
        info[i].n_clamped = cnt[2 * i];
        info[i].n_nan = cnt[2 * i + 1];
    }
    return TH_OK;
}
}  // namespace

int flac_run(th_tm *tm, size_t n, ExportInfo *info, uint8_t *out) {
    std::vector<FlacPlanRequest> prs(n);
    std::vector<const float *> chan;
    for (size_t i = 0; i < n; i++) {
        const th_export_request &r = info[i].req;
        const Track &tr = *static_cast<const Track *>(info[i].track);
        prs[i] = FlacPlanRequest{info[i].n_channels, r.format, r.dither, r.seed, tr.sr, info[i].sample_start, info[i].sample_end, info[i].offset,
                                 info[i].flac_flags};
        for (const Channel &c : tr.ch) chan.push_back(r.which == 0 ? c.d_wav : r.which == 1 ? c.d_draw : c.d_orig);
        info[i].n_clamped = info[i].n_nan = 0;
    }
    FlacPlan pl = plan_flac(prs.data(), n, TH_EXPORT_PIECE_BYTES);
    if (pl.err != TH_OK) return fail(pl.err, "%s", pl.err_text.c_str());
    std::vector<FlacProgress> prog(n);
    if (!pl.pieces.empty()) TH_CHECK(flac_run_pieces(tm, pl, prs, chan, info, out, prog));
    for (size_t i = 0; i < n; i++) {  // (the frames are in place: their sizes are known)
        flac_stream_header(prs[i].sr, prs[i].n_ch, flac_bps(prs[i].format), prs[i].s1 - prs[i].s0, prog[i].mx ? prog[i].mn : 0u, prog[i].mx,
                           out + info[i].offset);
        info[i].n_bytes = prog[i].at;
    }
    return TH_OK;
}
}  // namespace tmi
}  // namespace th

TH_API int th_tm_export_flac(th_tm *tm, const th_export_request *reqs, size_t n, uint8_t *out, size_t cap, th_export_info *info,
                             size_t *out_len) {
    TH_TRY
    return tmi::flac_read(TmReaders{tm}, reqs, n, 0u, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_export_flac_ex(th_tm *tm, const th_export_request *reqs, size_t n, uint32_t flags, uint8_t *out, size_t cap,
                                th_export_info *info, size_t *out_len) {
    TH_TRY
    return tmi::flac_read(TmReaders{tm}, reqs, n, flags, out, cap, info, out_len);
    TH_CATCH
}

// ---------------------------------------------------------------------------------------------- figures
// th_tm_render_figures: a reader.  plan_figures (figure_plan.h) checks the requests, builds the tap tables and cuts the call into
// pieces; bind_figures gives the jobs their addresses; what is left here is the slot, its buffers, the upload and the pipeline of the
// two streams: per piece the two launches of kernels_figure.hip into staging buffer p & 1 and one copy per part into the caller's
// buffer on the slot's copy stream, while the next piece is computed.
namespace th {
namespace tmi {
int figure_request_info(th_tm *tm, const th_figure_request &r, size_t i, FigureInfo *info) {
    auto it = tm->tracks.find(r.id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "request %zu: Track %zu does not exist", i, r.id);
    TH_REQUIRE(r.ch < it->second.ch.size(), "request %zu: Track %zu has no channel %u", i, r.id, r.ch);
    const Channel &c = it->second.ch[r.ch];
    if (!c.d_img) return fail(TH_ERR_NOT_FOUND, "request %zu: Spectrogram %zu_%u does not exist", i, r.id, r.ch);
    *info = FigureInfo{};
    info->plan = FigurePlanRequest{c.d_img, (uint32_t)c.img_w, (uint32_t)c.img_h, (uint32_t)c.img_pitch, r.kind, r.out_w, r.out_h,
                                   r.left, r.top, r.width, r.height, 0};
    const FigureStatus st = check_figure(info->plan, i);
    if (st.err != TH_OK) return fail(st.err, "%s", st.err_text.c_str());
    info->bytes = (uint64_t)r.out_w * r.out_h * figure_bytes_per_pixel(r.kind);
    info->out_w = r.out_w;
    info->out_h = r.out_h;
    return TH_OK;
}

int figures_run(th_tm *tm, size_t n, FigureInfo *info, uint8_t *out) {
    std::vector<FigurePlanRequest> prs(n);
    for (size_t i = 0; i < n; i++) prs[i] = info[i].plan;
    FigurePlan pl = plan_figures(prs.data(), n);
    if (pl.err != TH_OK) return fail(pl.err, "%s", pl.err_text.c_str());
    const std::vector<FigurePiece> &pieces = pl.pieces;
    if (pieces.empty()) return TH_OK;

    TH_HIP(hipSetDevice(tm->ctx->device));
    SlotLease lease{tm, nullptr};
    int rc = acquire_slot(tm, &lease.slot);
    if (rc != TH_OK) return rc;
    ReaderSlot &sl = *lease.slot;
    if (!sl.exp_copy) {
        TH_HIP(hipStreamCreateWithFlags(&sl.exp_copy, hipStreamNonBlocking));
        for (int b = 0; b < 2; b++) {
            TH_HIP(hipEventCreateWithFlags(&sl.exp_done[b], hipEventDisableTiming));
            TH_HIP(hipEventCreateWithFlags(&sl.exp_copied[b], hipEventDisableTiming));
        }
    }
    std::vector<unsigned char> tab;  // (behind the drain: alive until the upload is done)
    ExportDrain drain{&sl};
    for (int b = 0; b < 2; b++)  // powers of two from 1 MiB, never above one piece; the copy stream reads them too
        TH_CHECK(grow_export_buf(sl, sl.fig_stage[b], sl.fig_stage_cap[b], pl.stage_need[b], 1 << 20, TH_FIGURE_PIECE_BYTES, sl.exp_copy));
    // (elements) powers of two from 1 MiB up to the bound; a single output row that needs more gets exactly what it needs
    TH_CHECK(grow_export_buf(sl, sl.fig_tmp, sl.fig_tmp_cap, pl.tmp_need, 1 << 19,
                             std::max<size_t>(TH_FIGURE_TMP_BYTES / sizeof(uint16_t), pl.tmp_need), nullptr));
    TH_CHECK(sl.fig_tab.ensure(pl.tab_bytes));
    unsigned char *d_tab = static_cast<unsigned char *>(sl.fig_tab.dptr);
    tab = bind_figures(pl, FigureBases{{sl.fig_stage[0].get(), sl.fig_stage[1].get()}, sl.fig_tmp.get(), d_tab}, prs.data());
    TH_CHECK(sl.fig_tab.upload(sl.stream, tab.data(), tab.size()));
    const FigHJob *d_hjobs = reinterpret_cast<const FigHJob *>(d_tab + pl.o_hjobs);
    const FigVJob *d_vjobs = reinterpret_cast<const FigVJob *>(d_tab + pl.o_vjobs);
    const uint32_t n_colors = (uint32_t)(tm->colormap_rgba.size() / 4);
    auto launch_piece = [&](size_t p) -> int {
        const FigurePiece &pc = pieces[p];
        const uint32_t nj = (uint32_t)(pc.part1 - pc.part0);
        // (the stream's order keeps the intermediate from the last piece's vertical pass)
        TH_HIP(launch_figure_hpass(d_hjobs + pc.part0, nj, pc.n_hblocks, sl.stream));
        if (p >= 2) TH_HIP(hipStreamWaitEvent(sl.stream, sl.exp_copied[p & 1], 0));  // (the buffer's last piece has left it)
        TH_HIP(launch_figure_vpass(d_vjobs + pc.part0, nj, pc.n_vblocks, tm->d_colormap, n_colors, sl.stream));
        TH_HIP(hipEventRecord(sl.exp_done[p & 1], sl.stream));
        return TH_OK;
    };
    TH_CHECK(launch_piece(0));
    for (size_t p = 0; p < pieces.size(); p++) {
        if (p + 1 < pieces.size()) TH_CHECK(launch_piece(p + 1));  // (ahead of the copy: a copy into pageable memory holds the host)
        TH_HIP(hipStreamWaitEvent(sl.exp_copy, sl.exp_done[p & 1], 0));
        for (size_t k = pieces[p].part0; k < pieces[p].part1; k++) {
            const FigurePart &pt = pl.parts[k];
            TH_HIP(hipMemcpyAsync(out + pt.out_at, sl.fig_stage[p & 1].get() + pt.stage_at, pt.bytes, hipMemcpyDeviceToHost, sl.exp_copy));
        }
        TH_HIP(hipEventRecord(sl.exp_copied[p & 1], sl.exp_copy));
    }
    TH_HIP(hipStreamSynchronize(sl.stream));
    TH_HIP(hipStreamSynchronize(sl.exp_copy));
    return TH_OK;
}

int figure_box_of(th_tm *tm, size_t id, uint32_t ch, double start_sec, double end_sec, double hz_min, double hz_max, double box[4]) {
    auto it = tm->tracks.find(id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", id);
    TH_REQUIRE(ch < it->second.ch.size(), "Track %zu has no channel %u", id, ch);
    const Channel &c = it->second.ch[ch];
    if (!c.d_img) return fail(TH_ERR_NOT_FOUND, "Spectrogram %zu_%u does not exist", id, ch);
    TH_REQUIRE(figure_box(start_sec, end_sec, hz_min, hz_max, it->second.sr, c.n, c.img_w, c.H, c.img_h, tm->freq_scale, box) == 0,
               "bad figure range: [%g, %g) s, [%g, %g) Hz", start_sec, end_sec, hz_min, hz_max);
    return TH_OK;
}
}  // namespace tmi
}  // namespace th

TH_API int th_figure_axis(double origin, double extent, uint32_t n_out, uint32_t n_in, int32_t *start, int32_t *count, double *weights,
                          size_t cap_weights, uint32_t *max_taps) {
    TH_TRY
    TH_REQUIRE(start && count && max_taps, "NULL argument");
    TH_REQUIRE(n_out > 0 && n_in > 0 && n_in <= 0x7fffffffu, "an axis needs source and output pixels");
    TH_REQUIRE(std::isfinite(origin) && std::isfinite(extent) && extent > 0.0, "the extent must be finite and positive");
    LodAxisHost ax;
    build_lod_axis(origin, extent, n_out, 0, (long)n_in, ax);
    std::memcpy(start, ax.start.data(), (size_t)n_out * sizeof(int32_t));
    std::memcpy(count, ax.count.data(), (size_t)n_out * sizeof(int32_t));
    *max_taps = ax.max_taps;
    if (!weights || cap_weights < ax.w.size()) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu weights", ax.w.size());
    std::memcpy(weights, ax.w.data(), ax.w.size() * sizeof(double));
    return TH_OK;
    TH_CATCH
}

TH_API int th_figure_box(double start_sec, double end_sec, double hz_min, double hz_max, uint32_t sr, size_t n_samples, size_t img_width,
                         size_t spec_height, size_t img_height, int freq_scale, double *left, double *top, double *width, double *height) {
    TH_TRY
    TH_REQUIRE(left && top && width && height, "NULL argument");
    double box[4];
    TH_REQUIRE(figure_box(start_sec, end_sec, hz_min, hz_max, sr, n_samples, img_width, spec_height, img_height, freq_scale, box) == 0,
               "bad figure range: [%g, %g) s, [%g, %g) Hz of %zu samples at %u Hz, image %zu x %zu over %zu rows", start_sec, end_sec, hz_min,
               hz_max, n_samples, sr, img_width, img_height, spec_height);
    *left = box[0];
    *top = box[1];
    *width = box[2];
    *height = box[3];
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_figure_box(th_tm *tm, size_t id, uint32_t ch, double start_sec, double end_sec, double hz_min, double hz_max, double *left,
                            double *top, double *width, double *height) {
    TH_TRY
    TH_REQUIRE(tm && left && top && width && height, "NULL argument");
    std::shared_lock<std::shared_mutex> rl(tm->rw);
    double box[4];
    TH_CHECK(tmi::figure_box_of(tm, id, ch, start_sec, end_sec, hz_min, hz_max, box));
    *left = box[0];
    *top = box[1];
    *width = box[2];
    *height = box[3];
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_render_figures(th_tm *tm, const th_figure_request *reqs, size_t n, uint8_t *out, size_t cap, th_figure_info *info,
                                size_t *out_len) {
    TH_TRY
    return br::batched_read<tmi::FigureReader>(TmReaders{tm}, reqs, n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_render_figure(th_tm *tm, const th_figure_request *req, uint8_t *out, size_t cap, th_figure_info *info) {
    TH_TRY
    TH_REQUIRE(tm && req, "NULL argument");
    return br::single_read(info, [&](th_figure_info *one, size_t *len) { return th_tm_render_figures(tm, req, 1, out, cap, one, len); });
    TH_CATCH
}

// ---------------------------------------------------------------------------------------------- waveform envelopes and lanes
// th_tm_get_envelopes / th_tm_render_waveform_figures: readers.  plan_envelopes / plan_lanes (envelope_plan.h) check the requests,
// build the edge tables and cut the call into pieces; the bind functions give the jobs their addresses; what is left here is the
// slot, its buffers, the upload and the launches of kernels_envelope.hip.  An envelope piece is two launches and one copy per run of
// adjacent records (a call of one piece of at most the slot's pinned staging is written there by the kernels); a lane piece is one
// raster launch into staging buffer p & 1 and one copy per part on the slot's copy stream while the next piece is computed, with
// the envelopes and spans of its group computed once in front of the group's first piece.
namespace th {
namespace tmi {
namespace {
int envelope_channel(th_tm *tm, const th_envelope_request &r, size_t i, EnvelopePlanRequest *pr) {
    auto it = tm->tracks.find(r.id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "request %zu: Track %zu does not exist", i, r.id);
    TH_REQUIRE(r.ch < it->second.ch.size(), "request %zu: Track %zu has no channel %u", i, r.id, r.ch);
    TH_REQUIRE(r.which <= 2, "request %zu: which must be 0 (audio), 1 (drawn) or 2 (original)", i);
    const Channel &c = it->second.ch[r.ch];
    const float *src = r.which == 0 ? c.d_wav : r.which == 1 ? c.d_draw : c.d_orig;
    *pr = EnvelopePlanRequest{src, c.n, it->second.sr, r.n_cols, r.start_sec, r.end_sec, 0};
    return TH_OK;
}
}  // namespace

int envelope_request_info(th_tm *tm, const th_envelope_request &r, size_t i, EnvelopeInfo *info) {
    *info = EnvelopeInfo{};
    TH_CHECK(envelope_channel(tm, r, i, &info->plan));
    const EnvelopeStatus st = check_envelope(info->plan, i, &info->sample_start, &info->sample_end);
    if (st.err != TH_OK) return fail(st.err, "%s", st.err_text.c_str());
    info->length = (uint64_t)r.n_cols * 4;
    return TH_OK;
}

int envelopes_run(th_tm *tm, size_t n, EnvelopeInfo *info, float *out) {
    std::vector<EnvelopePlanRequest> prs(n);
    for (size_t i = 0; i < n; i++) prs[i] = info[i].plan;
    EnvelopePlan pl = plan_envelopes(prs.data(), n);
    if (pl.err != TH_OK) return fail(pl.err, "%s", pl.err_text.c_str());
    if (pl.pieces.empty()) return TH_OK;

    TH_HIP(hipSetDevice(tm->ctx->device));
    SlotLease lease{tm, nullptr};
    int rc = acquire_slot(tm, &lease.slot);
    if (rc != TH_OK) return rc;
    ReaderSlot &sl = *lease.slot;
    std::vector<unsigned char> tab(pl.tab_bytes);  // (behind the drain: alive until the upload is done)
    ExportDrain drain{&sl};
    const bool pinned = pl.pieces.size() == 1 && pl.out_need * sizeof(float) <= TILE_BYTES_MAX;
    if (!pinned) TH_CHECK(sl.env_out.ensure(pl.out_need * sizeof(float)));
    TH_CHECK(sl.env_part.ensure(std::max<size_t>(pl.part_need, 1) * sizeof(EnvPartial)));
    TH_CHECK(sl.env_tab.ensure(pl.tab_bytes));
    float *res = pinned ? reinterpret_cast<float *>(sl.h_tile_dev) : static_cast<float *>(sl.env_out.dptr);
    unsigned char *d_tab = static_cast<unsigned char *>(sl.env_tab.dptr);
    bind_envelopes(pl, EnvelopeBases{res, static_cast<EnvPartial *>(sl.env_part.dptr), d_tab}, prs.data(), tab.data());
    TH_CHECK(sl.env_tab.upload(sl.stream, tab.data(), tab.size()));
    const EnvJob *d_jobs = reinterpret_cast<const EnvJob *>(d_tab + pl.o_jobs);
    for (const EnvelopePiece &pc : pl.pieces) {
        const uint32_t nj = (uint32_t)(pc.req1 - pc.req0);
        TH_HIP(launch_envelope_reduce(d_jobs + pc.req0, nj, pc.n_units, sl.stream));
        TH_HIP(launch_envelope_columns(d_jobs + pc.req0, nj, pc.n_cblocks, sl.stream));
        if (pinned) TH_HIP(hipStreamSynchronize(sl.stream));
        // one copy per maximal run of adjacent destinations (the piece's results are adjacent in the slot's area)
        for (size_t i = pc.req0, k; i < pc.req1; i = k) {
            k = i + 1;
            while (k < pc.req1 && info[k].offset == info[k - 1].offset + info[k - 1].length) k++;
            const size_t bytes = (pl.out_at[k - 1] + (size_t)info[k - 1].length - pl.out_at[i]) * sizeof(float);
            if (pinned)
                std::memcpy(out + info[i].offset, reinterpret_cast<const float *>(sl.h_tile) + pl.out_at[i], bytes);
            else
                TH_HIP(hipMemcpyAsync(out + info[i].offset, res + pl.out_at[i], bytes, hipMemcpyDeviceToHost, sl.stream));
        }
    }
    TH_HIP(hipStreamSynchronize(sl.stream));
    return TH_OK;
}

int waveform_figure_request_info(th_tm *tm, const th_waveform_figure_request &r, size_t i, WaveformFigureInfo *info) {
    *info = WaveformFigureInfo{};
    EnvelopePlanRequest er;
    TH_CHECK(envelope_channel(tm, r.env, i, &er));
    static_cast<EnvelopePlanRequest &>(info->plan) = er;
    info->plan.out_h = r.out_h;
    info->plan.amp_lo = r.amp_lo;
    info->plan.amp_hi = r.amp_hi;
    info->plan.thickness = r.thickness;
    std::memcpy(info->plan.fill, r.fill, 4);
    std::memcpy(info->plan.background, r.background, 4);
    const EnvelopeStatus st = check_lane(info->plan, i, &info->sample_start, &info->sample_end);
    if (st.err != TH_OK) return fail(st.err, "%s", st.err_text.c_str());
    info->bytes = (uint64_t)r.env.n_cols * r.out_h * 4;
    info->out_w = r.env.n_cols;
    info->out_h = r.out_h;
    return TH_OK;
}

int waveform_figures_run(th_tm *tm, size_t n, WaveformFigureInfo *info, uint8_t *out) {
    std::vector<LanePlanRequest> prs(n);
    for (size_t i = 0; i < n; i++) prs[i] = info[i].plan;
    LanePlan pl = plan_lanes(prs.data(), n);
    if (pl.err != TH_OK) return fail(pl.err, "%s", pl.err_text.c_str());
    const std::vector<LanePiece> &pieces = pl.pieces;
    if (pieces.empty()) return TH_OK;

    TH_HIP(hipSetDevice(tm->ctx->device));
    SlotLease lease{tm, nullptr};
    int rc = acquire_slot(tm, &lease.slot);
    if (rc != TH_OK) return rc;
    ReaderSlot &sl = *lease.slot;
    if (!sl.exp_copy) {
        TH_HIP(hipStreamCreateWithFlags(&sl.exp_copy, hipStreamNonBlocking));
        for (int b = 0; b < 2; b++) {
            TH_HIP(hipEventCreateWithFlags(&sl.exp_done[b], hipEventDisableTiming));
            TH_HIP(hipEventCreateWithFlags(&sl.exp_copied[b], hipEventDisableTiming));
        }
    }
    std::vector<unsigned char> tab(pl.tab_bytes);  // (behind the drain: alive until the upload is done)
    ExportDrain drain{&sl};
    for (int b = 0; b < 2; b++)  // the figures' staging buffers: powers of two from 1 MiB, never above one piece
        TH_CHECK(grow_export_buf(sl, sl.fig_stage[b], sl.fig_stage_cap[b], pl.stage_need[b], 1 << 20, TH_FIGURE_PIECE_BYTES, sl.exp_copy));
    TH_CHECK(sl.env_out.ensure(pl.env.out_need * sizeof(float)));
    TH_CHECK(sl.env_part.ensure(std::max<size_t>(pl.env.part_need, 1) * sizeof(EnvPartial)));
    TH_CHECK(sl.lane_span.ensure(pl.span_need * sizeof(int32_t)));
    TH_CHECK(sl.env_tab.ensure(pl.tab_bytes));
    unsigned char *d_tab = static_cast<unsigned char *>(sl.env_tab.dptr);
    LaneBases bases{};
    bases.env = EnvelopeBases{static_cast<float *>(sl.env_out.dptr), static_cast<EnvPartial *>(sl.env_part.dptr), d_tab};
    bases.span = static_cast<int32_t *>(sl.lane_span.dptr);
    bases.stage[0] = sl.fig_stage[0].get();
    bases.stage[1] = sl.fig_stage[1].get();
    bind_lanes(pl, bases, prs.data(), tab.data());
    TH_CHECK(sl.env_tab.upload(sl.stream, tab.data(), tab.size()));
    const EnvJob *d_ejobs = reinterpret_cast<const EnvJob *>(d_tab + pl.env.o_jobs);
    const LaneSpanJob *d_sjobs = reinterpret_cast<const LaneSpanJob *>(d_tab + pl.o_sjobs);
    const LaneRasterJob *d_rjobs = reinterpret_cast<const LaneRasterJob *>(d_tab + pl.o_rjobs);
    auto launch_piece = [&](size_t p) -> int {
        const LanePiece &pc = pieces[p];
        if (pc.first_of_group) {  // (the stream's order keeps the envelopes and spans from the last group's rasters)
            const EnvelopePiece &g = pl.env.pieces[pc.group];
            const uint32_t nj = (uint32_t)(g.req1 - g.req0);
            TH_HIP(launch_envelope_reduce(d_ejobs + g.req0, nj, g.n_units, sl.stream));
            TH_HIP(launch_envelope_columns(d_ejobs + g.req0, nj, g.n_cblocks, sl.stream));
            TH_HIP(launch_lane_spans(d_sjobs + g.req0, nj, pl.group_sblocks[pc.group], sl.stream));
        }
        if (p >= 2) TH_HIP(hipStreamWaitEvent(sl.stream, sl.exp_copied[p & 1], 0));  // (the buffer's last piece has left it)
        TH_HIP(launch_lane_raster(d_rjobs + pc.part0, (uint32_t)(pc.part1 - pc.part0), pc.n_blocks, sl.stream));
        TH_HIP(hipEventRecord(sl.exp_done[p & 1], sl.stream));
        return TH_OK;
    };
    TH_CHECK(launch_piece(0));
    for (size_t p = 0; p < pieces.size(); p++) {
        if (p + 1 < pieces.size()) TH_CHECK(launch_piece(p + 1));  // (ahead of the copy: a copy into pageable memory holds the host)
        TH_HIP(hipStreamWaitEvent(sl.exp_copy, sl.exp_done[p & 1], 0));
        for (size_t k = pieces[p].part0; k < pieces[p].part1; k++) {
            const LanePart &pt = pl.parts[k];
            TH_HIP(hipMemcpyAsync(out + pt.out_at, sl.fig_stage[p & 1].get() + pt.stage_at, pt.bytes, hipMemcpyDeviceToHost, sl.exp_copy));
        }
        TH_HIP(hipEventRecord(sl.exp_copied[p & 1], sl.exp_copy));
    }
    TH_HIP(hipStreamSynchronize(sl.stream));
    TH_HIP(hipStreamSynchronize(sl.exp_copy));
    return TH_OK;
}

// ---------------------------------------------------------------------------------------------- formant candidates
// th_tm_get_formants: a reader.  formant_plan_for checks a request and makes its numbers; plan_formants (formant_plan.h) cuts the call
// into pieces of runs of frames and bind_formants gives the jobs their addresses; what is left here is the slot, its buffers, the
// upload, and per piece the resampler's launch for the resampled runs (export's resample_kernel and the slot's table, unchanged),
// the formant kernel's launch into record buffer p & 1, one copy on the slot's copy stream, and step 6 with the packing on the host
// while the next piece computes.
int formant_request_info(th_tm *tm, const th_formant_request &r, size_t i, FormantInfo *info) {
    *info = FormantInfo{};
    auto it = tm->tracks.find(r.id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "request %zu: Track %zu does not exist", i, r.id);
    TH_REQUIRE(r.ch < it->second.ch.size(), "request %zu: Track %zu has no channel %u", i, r.id, r.ch);
    TH_REQUIRE(r.which <= 2, "request %zu: which must be 0 (audio), 1 (drawn) or 2 (original)", i);
    const Channel &c = it->second.ch[r.ch];
    const uint32_t sr = it->second.sr;
    const int rc = formant_plan_for(sr, c.n, r, &info->plan.pl);
    TH_REQUIRE(rc != 1,
               "request %zu: bad formant request: [%g, %g) s at %u Hz, analysis at %u Hz, %u poles (even, 2 .. %u), window %g s (%u .. %u "
               "samples), step %g s (at most %u samples), pre-emphasis from %g Hz, window %u, kind %u",
               i, r.start_sec, r.end_sec, sr, r.sr_analysis, r.n_poles, TH_FORMANT_MAX_POLES, r.win_sec, r.n_poles + 2, TH_FORMANT_MAX_WIN,
               r.step_sec, TH_FORMANT_MAX_HOP, r.preemph_hz, r.window, r.kind);
    if (rc != 0)
        return fail(TH_ERR_UNSUPPORTED, "request %zu: %u -> %u Hz is beyond the resampler's limits (%u taps, %u coefficients, 64-bit indices)",
                    i, sr, r.sr_analysis, TH_RESAMPLE_MAX_TAPS, TH_RESAMPLE_MAX_COEFS);
    const th_formant_plan &pl = info->plan.pl;
    info->plan.src = r.which == 0 ? c.d_wav : r.which == 1 ? c.d_draw : c.d_orig;
    info->plan.n_in = c.n;
    info->frame_first = pl.frame_first;
    info->frame_end = pl.frame_end;
    info->length = (pl.frame_end - pl.frame_first) * (2 + pl.n_poles);
    info->sr_analysis = pl.sr_analysis;
    info->win = pl.win;
    info->hop = pl.hop;
    return TH_OK;
}

int formants_run(th_tm *tm, size_t n, FormantInfo *info, double *out) {
    std::vector<FormantPlanRequest> prs(n);
    for (size_t i = 0; i < n; i++) {
        prs[i] = info[i].plan;
        info[i].n_invalid = info[i].n_unconverged = 0;
    }
    FormantPlan pl = plan_formants(prs.data(), n);
    if (pl.err != TH_OK) return fail(pl.err, "%s", pl.err_text.c_str());
    const std::vector<FormantPiece> &pieces = pl.pieces;
    if (pieces.empty()) return TH_OK;

    TH_HIP(hipSetDevice(tm->ctx->device));
    SlotLease lease{tm, nullptr};
    int rc = acquire_slot(tm, &lease.slot);
    if (rc != TH_OK) return rc;
    ReaderSlot &sl = *lease.slot;
    if (!sl.exp_copy) {
        TH_HIP(hipStreamCreateWithFlags(&sl.exp_copy, hipStreamNonBlocking));
        for (int b = 0; b < 2; b++) {
            TH_HIP(hipEventCreateWithFlags(&sl.exp_done[b], hipEventDisableTiming));
            TH_HIP(hipEventCreateWithFlags(&sl.exp_copied[b], hipEventDisableTiming));
        }
    }
    std::vector<std::vector<float>> host_tables(pieces.size());  // (behind the drain: alive until the uploads are done)
    std::vector<double> host_rec[2];
    ExportDrain drain{&sl};
    const size_t rec_ceil = (size_t)TH_FORMANT_PIECE_FRAMES * formant_rec_doubles(TH_FORMANT_MAX_POLES);
    for (int b = 0; b < 2; b++) {  // (doubles) powers of two from 64 Ki, never above one piece; the copy stream reads them too
        if ((size_t)b < pieces.size()) TH_CHECK(grow_export_buf(sl, sl.fm_rec[b], sl.fm_rec_cap[b], (size_t)pl.rec_need, 1 << 16, rec_ceil, sl.exp_copy));
        host_rec[b].resize((size_t)pl.rec_need);
    }
    if (pl.scratch_need)
        TH_CHECK(grow_export_buf(sl, sl.rs_scratch, sl.rs_scratch_cap, (size_t)pl.scratch_need, 1 << 18, RESAMPLE_SCRATCH_MAX / sizeof(float), nullptr));
    TH_CHECK(sl.fm_tab.ensure(pl.tab_bytes));
    unsigned char *d_tab = static_cast<unsigned char *>(sl.fm_tab.dptr);
    const std::vector<unsigned char> tab =
        bind_formants(pl, FormantBases{{sl.fm_rec[0].get(), sl.fm_rec[1].get()}, sl.rs_scratch.get(), d_tab}, prs.data(), n);
    TH_CHECK(sl.fm_tab.upload(sl.stream, tab.data(), tab.size()));
    const FormantJob *d_jobs = reinterpret_cast<const FormantJob *>(d_tab + pl.o_jobs);
    const ResampleJob *d_rjobs = reinterpret_cast<const ResampleJob *>(d_tab + pl.o_rjobs);
    auto launch_piece = [&](size_t p) -> int {
        const FormantPiece &pc = pieces[p];
        if (pc.n_rblocks) {  // (the stream's order keeps the scratch and the table from the last piece's readers)
            TH_CHECK(ensure_resample_table(sl, pc.sr_in, pc.sr_out, pc.rs, &host_tables[p]));
            TH_HIP(launch_resample(d_rjobs + pc.rjob0, (uint32_t)(pc.rjob1 - pc.rjob0), pc.n_rblocks, sl.rs_table.get(), resample_tiling(pc.rs), sl.stream));
        }
        TH_HIP(launch_formants(d_jobs + pc.run0, (uint32_t)(pc.run1 - pc.run0), pc.n_blocks, pc.max_W, pc.max_p, sl.stream));
        TH_HIP(hipEventRecord(sl.exp_done[p & 1], sl.stream));
        return TH_OK;
    };
    TH_CHECK(launch_piece(0));
    for (size_t p = 0; p < pieces.size(); p++) {
        // (piece p + 1 goes into the other buffer; the copy of piece p - 1 out of it has been waited for below)
        if (p + 1 < pieces.size()) TH_CHECK(launch_piece(p + 1));
        const FormantPiece &pc = pieces[p];
        double *h = host_rec[p & 1].data();
        TH_HIP(hipStreamWaitEvent(sl.exp_copy, sl.exp_done[p & 1], 0));
        TH_HIP(hipMemcpyAsync(h, sl.fm_rec[p & 1].get(), (size_t)pc.rec_doubles * sizeof(double), hipMemcpyDeviceToHost, sl.exp_copy));
        TH_HIP(hipStreamSynchronize(sl.exp_copy));
        for (size_t j = pc.run0; j < pc.run1; j++) {  // step 6 and the packing, while the next piece computes
            const FormantRun &run = pl.runs[j];
            FormantInfo &fi = info[run.req];
            const th_formant_plan &fp = fi.plan.pl;
            const uint32_t stride = formant_rec_doubles(fp.n_poles), per = 2 + fp.n_poles;
            double *dst = out + fi.offset + (run.f0 - fp.frame_first) * per;
            uint64_t cnt[2] = {0, 0};
            for (uint32_t k = 0; k < run.n_frames; k++) formant_pack(h + run.rec_at + (uint64_t)k * stride, fp, dst + (uint64_t)k * per, cnt);
            fi.n_invalid += cnt[0];
            fi.n_unconverged += cnt[1];
        }
    }
    TH_HIP(hipStreamSynchronize(sl.stream));
    return TH_OK;
}

// ---------------------------------------------------------------------------------------------- alignment of two tracks
// th_tm_align_tracks: a reader.  align_plan_for checks a request and makes its numbers; plan_align (align_plan.h) cuts a request into
// pieces of lags; what is left here is the slot, its buffers and, request after request: the reference's energy, per piece the
// correlation kernel and its fold into record buffer p & 1 and one copy on the slot's copy stream while the next piece computes, then
// the host's step on the curve, the probe's energy at the lag it found, and the summary.
int align_request_info(th_tm *tm, const AlignReq &ar, size_t i, AlignInfo *info) {
    const th_align_request &r = ar.r;
    *info = AlignInfo{};
    auto it = tm->tracks.find(r.id);
    if (it == tm->tracks.end()) return fail(TH_ERR_NOT_FOUND, "request %zu: Track %zu does not exist", i, r.id);
    th_tm *home = ar.home_of ? ar.home_of(ar.who, r.ref_id) : tm;
    const Track *rt = nullptr;
    if (home) {
        auto ir = home->tracks.find(r.ref_id);
        if (ir != home->tracks.end()) rt = &ir->second;
    }
    if (!rt) return fail(TH_ERR_NOT_FOUND, "request %zu: reference Track %zu does not exist", i, r.ref_id);
    const Track &pt = it->second;
    TH_REQUIRE(r.ch < pt.ch.size(), "request %zu: Track %zu has no channel %u", i, r.id, r.ch);
    TH_REQUIRE(r.ref_ch < rt->ch.size(), "request %zu: reference Track %zu has no channel %u", i, r.ref_id, r.ref_ch);
    TH_REQUIRE(r.which <= 2 && r.ref_which <= 2, "request %zu: which must be 0 (audio), 1 (drawn) or 2 (original)", i);
    const Channel &pc = pt.ch[r.ch], &rc = rt->ch[r.ref_ch];
    const int rcode = align_plan_for(rt->sr, rc.n, pt.sr, pc.n, r, &info->pl);
    TH_REQUIRE(rcode != 1, "request %zu: bad alignment request: [%g, %g) s of the reference at %u Hz, lags up to %g s, kind %u, flags %u", i,
               r.start_sec, r.end_sec, rt->sr, r.max_lag_sec, r.kind, r.flags);
    if (rcode != 0)
        return fail(TH_ERR_UNSUPPORTED,
                    "request %zu: [%g, %g) s at %u Hz against %u Hz over %g s of lag: the rates must be equal, the range at most %u samples, "
                    "the lag at most %u samples, their product at most 2^40",
                    i, r.start_sec, r.end_sec, rt->sr, pt.sr, r.max_lag_sec, TH_ALIGN_MAX_REF, TH_ALIGN_MAX_LAG);
    const th_align_plan &pl = info->pl;
    info->ref = r.ref_which == 0 ? rc.d_wav : r.ref_which == 1 ? rc.d_draw : rc.d_orig;
    info->probe = r.which == 0 ? pc.d_wav : r.which == 1 ? pc.d_draw : pc.d_orig;
    info->n_probe = pc.n;
    info->ref_home = home;
    info->length = pl.length;
    info->sr = pl.sr;
    info->max_lag = pl.max_lag;
    info->sample_start = pl.sample_start;
    info->sample_end = pl.sample_end;
    info->waveform_revision = tm->waveform_revision();
    return TH_OK;
}

namespace {
// the calling thread's device goes back to the slot's own when the reference's manager has been read
struct DeviceBack {
    int device;
    ~DeviceBack() { (void)hipSetDevice(device); }
};

// n samples at src, in manager `home` (another one than the slot's: a slot of the same th_tmg, whose lock the caller holds, so no writer
// is in either), into the slot's al_ref: by home's device into pinned host memory, from there up on the slot's stream
int align_stage_ref(th_tm *tm, ReaderSlot &sl, th_tm *home, const float *src, size_t n) {
    if (sl.al_ref_host_cap < n) {
        size_t want = 1 << 16;
        while (want < n) want <<= 1;
        if (sl.al_ref_host) TH_HIP(hipHostFree(sl.al_ref_host));
        sl.al_ref_host = nullptr;
        sl.al_ref_host_cap = 0;
        TH_HIP(hipHostMalloc((void **)&sl.al_ref_host, want * sizeof(float), hipHostMallocPortable));
        sl.al_ref_host_cap = want;
    }
    TH_CHECK(grow_export_buf(sl, sl.al_ref, sl.al_ref_cap, n, 1 << 16, TH_ALIGN_MAX_REF, nullptr));
    {
        std::shared_lock<std::shared_mutex> hl(home->rw);
        DeviceBack back{tm->ctx->device};
        TH_HIP(hipSetDevice(home->ctx->device));
        TH_HIP(hipMemcpy(sl.al_ref_host, src, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    TH_HIP(hipMemcpyAsync(sl.al_ref.get(), sl.al_ref_host, n * sizeof(float), hipMemcpyHostToDevice, sl.stream));
    TH_HIP(hipStreamSynchronize(sl.stream));  // (the pinned buffer is the next staged request's too)
    return TH_OK;
}
}  // namespace

int align_run(th_tm *tm, size_t n, AlignInfo *info, double *out) {
    TH_HIP(hipSetDevice(tm->ctx->device));
    SlotLease lease{tm, nullptr};
    int rc = acquire_slot(tm, &lease.slot);
    if (rc != TH_OK) return rc;
    ReaderSlot &sl = *lease.slot;
    if (!sl.exp_copy) {
        TH_HIP(hipStreamCreateWithFlags(&sl.exp_copy, hipStreamNonBlocking));
        for (int b = 0; b < 2; b++) {
            TH_HIP(hipEventCreateWithFlags(&sl.exp_done[b], hipEventDisableTiming));
            TH_HIP(hipEventCreateWithFlags(&sl.exp_copied[b], hipEventDisableTiming));
        }
    }
    std::vector<double> curve;  // (behind the drain: alive until the copies are done)
    double h_en[2 * ALIGN_GROUP_BLOCKS];
    ExportDrain drain{&sl};
    if (!sl.al_en.get()) TH_HIP(sl.al_en.alloc(sizeof h_en));
    for (size_t i = 0; i < n; i++) {
        const th_align_plan &pl = info[i].pl;
        const uint64_t s0 = pl.sample_start, N = pl.sample_end - pl.sample_start;
        const uint32_t D = pl.max_lag, n_groups = (uint32_t)align_n_groups(N);
        double *dst = out + info[i].offset;
        AlignPeak pk{1u, 0, 0.0, 1.0};
        if (pl.n_lags == 0) {  // (an empty range: nothing to launch)
            align_summary(pk, nullptr, D, 0.0, 0.0, dst);
            continue;
        }
        double *r = dst + TH_ALIGN_SUMMARY_DOUBLES;
        if (pl.kind != TH_ALIGN_OUT_CURVE) {
            curve.resize((size_t)pl.n_lags);
            r = curve.data();
        }
        const float *a = info[i].ref + s0;
        if (info[i].ref_home != tm) {
            TH_CHECK(align_stage_ref(tm, sl, info[i].ref_home, a, (size_t)N));
            a = sl.al_ref.get();
        }
        const AlignPieces ap = plan_align(N, pl.n_lags);
        const std::vector<AlignPiece> &pieces = ap.pieces;
        TH_CHECK(grow_export_buf(sl, sl.al_scratch, sl.al_scratch_cap, (size_t)ap.scratch_doubles, 1 << 16,
                                 (size_t)ALIGN_GROUP_BLOCKS * TH_ALIGN_PIECE_LAGS, nullptr));
        for (int b = 0; b < 2; b++)  // (the copy stream reads them too)
            if ((size_t)b < pieces.size())
                TH_CHECK(grow_export_buf(sl, sl.al_rec[b], sl.al_rec_cap[b], (size_t)ap.rec_doubles, 1 << 12, TH_ALIGN_PIECE_LAGS, sl.exp_copy));
        TH_HIP(launch_align_energy(a, N, 0, N, sl.al_en.get(), sl.stream));
        auto launch_piece = [&](size_t p) -> int {
            const AlignPiece &pc = pieces[p];
            AlignJob job{};
            job.a = a;
            job.b = info[i].probe;
            job.scratch = sl.al_scratch.get();
            job.N = N;
            job.n_b = info[i].n_probe;
            job.first = (int64_t)s0 - (int64_t)D + (int64_t)pc.lag0;
            job.n_lags = pc.n_lags;
            job.n_tiles = pc.n_tiles;
            job.n_groups = pc.n_groups;
            TH_HIP(launch_align_xcorr(job, sl.al_rec[p & 1].get(), sl.stream));
            TH_HIP(hipEventRecord(sl.exp_done[p & 1], sl.stream));
            return TH_OK;
        };
        TH_CHECK(launch_piece(0));
        for (size_t p = 0; p < pieces.size(); p++) {
            // (piece p + 1 goes into the other buffer; the copy of piece p - 1 out of it has been waited for below)
            if (p + 1 < pieces.size()) TH_CHECK(launch_piece(p + 1));
            TH_HIP(hipStreamWaitEvent(sl.exp_copy, sl.exp_done[p & 1], 0));
            TH_HIP(hipMemcpyAsync(r + pieces[p].lag0, sl.al_rec[p & 1].get(), (size_t)pieces[p].n_lags * sizeof(double), hipMemcpyDeviceToHost,
                                  sl.exp_copy));
            TH_HIP(hipStreamSynchronize(sl.exp_copy));
        }
        TH_HIP(hipMemcpyAsync(h_en, sl.al_en.get(), n_groups * sizeof(double), hipMemcpyDeviceToHost, sl.stream));
        TH_HIP(hipStreamSynchronize(sl.stream));
        const double e_ref = align_fold(h_en, n_groups, 1);
        pk = align_peak(r, pl.n_lags, pl.flags, e_ref);
        double e_probe = 0.0;
        if (pk.status == 0) {  // (the probe's energy where the peak was found)
            double *d_en = sl.al_en.get() + ALIGN_GROUP_BLOCKS, *h = h_en + ALIGN_GROUP_BLOCKS;
            TH_HIP(launch_align_energy(info[i].probe, info[i].n_probe, (int64_t)s0 + (int64_t)pk.index - (int64_t)D, N, d_en, sl.stream));
            TH_HIP(hipMemcpyAsync(h, d_en, n_groups * sizeof(double), hipMemcpyDeviceToHost, sl.stream));
            TH_HIP(hipStreamSynchronize(sl.stream));
            e_probe = align_fold(h, n_groups, 1);
        }
        align_summary(pk, r, D, e_ref, e_probe, dst);
    }
    return TH_OK;
}
}  // namespace tmi
}  // namespace th

TH_API int th_envelope_edges(uint32_t sr, size_t n_samples, double start_sec, double end_sec, uint32_t n_cols, uint64_t *edges) {
    TH_TRY
    TH_REQUIRE(edges, "NULL argument");
    TH_REQUIRE(envelope_edges(sr, n_samples, start_sec, end_sec, n_cols, edges) == 0,
               "bad envelope: [%g, %g) s of %zu samples at %u Hz in %u columns (1 .. %u)", start_sec, end_sec, n_samples, sr, n_cols,
               TH_ENVELOPE_MAX_COLS);
    return TH_OK;
    TH_CATCH
}

TH_API int th_waveform_figure_span(const float *col, const float *left, uint32_t out_h, float amp_lo, float amp_hi, uint32_t thickness,
                                   int32_t *y_top, int32_t *y_bot, int *draws) {
    TH_TRY
    TH_REQUIRE(col && y_top && y_bot && draws, "NULL argument");
    TH_REQUIRE(waveform_figure_span(col, left, out_h, amp_lo, amp_hi, thickness, y_top, y_bot, draws) == 0,
               "bad lane: %u rows, amplitudes [%g, %g], thickness %u / 256", out_h, (double)amp_lo, (double)amp_hi, thickness);
    return TH_OK;
    TH_CATCH
}

TH_API int th_tm_get_envelopes(th_tm *tm, const th_envelope_request *reqs, size_t n, float *out, size_t cap, th_envelope_info *info,
                               size_t *out_len) {
    TH_TRY
    return br::batched_read<tmi::EnvelopeReader>(TmReaders{tm}, reqs, n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_get_envelope(th_tm *tm, const th_envelope_request *req, float *out, size_t cap, th_envelope_info *info) {
    TH_TRY
    TH_REQUIRE(tm && req, "NULL argument");
    return br::single_read(info, [&](th_envelope_info *one, size_t *len) { return th_tm_get_envelopes(tm, req, 1, out, cap, one, len); });
    TH_CATCH
}

TH_API int th_tm_get_formants(th_tm *tm, const th_formant_request *reqs, size_t n, double *out, size_t cap, th_formant_info *info,
                              size_t *out_len) {
    TH_TRY
    return br::batched_read<tmi::FormantReader>(TmReaders{tm}, reqs, n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_get_formant_track(th_tm *tm, const th_formant_request *req, double *out, size_t cap, th_formant_info *info) {
    TH_TRY
    TH_REQUIRE(tm && req, "NULL argument");
    return br::single_read(info, [&](th_formant_info *one, size_t *len) { return th_tm_get_formants(tm, req, 1, out, cap, one, len); });
    TH_CATCH
}

TH_API int th_tm_align_tracks(th_tm *tm, const th_align_request *reqs, size_t n, double *out, size_t cap, th_align_info *info, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(n == 0 || reqs, "NULL argument");
    return br::batched_read<tmi::AlignReader>(TmReaders{tm}, tmi::align_requests(reqs, n, nullptr, nullptr).data(), n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_align_track(th_tm *tm, const th_align_request *req, double *out, size_t cap, th_align_info *info) {
    TH_TRY
    TH_REQUIRE(tm && req, "NULL argument");
    return br::single_read(info, [&](th_align_info *one, size_t *len) { return th_tm_align_tracks(tm, req, 1, out, cap, one, len); });
    TH_CATCH
}

TH_API int th_tm_render_waveform_figures(th_tm *tm, const th_waveform_figure_request *reqs, size_t n, uint8_t *out, size_t cap,
                                         th_waveform_figure_info *info, size_t *out_len) {
    TH_TRY
    return br::batched_read<tmi::WaveformFigureReader>(TmReaders{tm}, reqs, n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tm_render_waveform_figure(th_tm *tm, const th_waveform_figure_request *req, uint8_t *out, size_t cap,
                                        th_waveform_figure_info *info) {
    TH_TRY
    TH_REQUIRE(tm && req, "NULL argument");
    return br::single_read(info,
                           [&](th_waveform_figure_info *one, size_t *len) { return th_tm_render_waveform_figures(tm, req, 1, out, cap, one, len); });
    TH_CATCH
}
