// track_manager_multi.hip — th_tmg: one TrackManager whose tracks live on several devices of one process.
//
// A slot = one th_ctx + one th_tm on one device (duplicates allowed).  A track lives whole on one slot.  The only coupling
// between slots is the reference's global dB range and max_sr (core/mod.rs:169-185): the channels' (min, max) are already on
// the host (finish_specs read them back), so the manager folds them here in the order one th_tm would and hands the result to
// every slot's image step.  The per-slot work of a mutator runs on one host thread per slot, so N devices work at once.
// Revisions are the manager's own and every slot's tile cache carries them, so tiles are stamped as one th_tm would stamp them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <shared_mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "common.h"
#include "host_math.h"
#include "tile_cache.h"
#include "track_manager_internal.h"

using namespace th;

struct th_tmg {
    struct Slot {
        int device = 0;
        th_ctx *ctx = nullptr;
        th_tm *tm = nullptr;
    };
    std::vector<Slot> slots;
    struct Placement {
        uint32_t slot;
        uint64_t weight;  // n_samples x n_channels
    };
    std::map<size_t, Placement> where;  // every resident track
    float dB_range = 100.f;             // TrackManager::new, core/mod.rs:46-60
    int lod_source = 0;
    // the revision pair of the whole manager (only the counters of this cache are used: it never holds a tile); every
    // slot's own cache is set to it after each mutator (sync_revisions)
    th_tile_cache revs{0};
    // writers take it exclusively, tile readers share it (th_tm::rw one level up): a reader never sees one slot re-made
    // while another is not
    mutable std::shared_mutex rw;
};

namespace {

// the manager's (waveform, spectrogram) revisions
std::pair<uint64_t, uint64_t> revisions(const th_tmg *g) {
    std::lock_guard<std::mutex> lk(g->revs.mu);
    return {g->revs.waveform_revision, g->revs.spectrogram_revision};
}

void sync_revisions(th_tmg *g) {
    const auto [w, s] = revisions(g);
    for (auto &sl : g->slots) {
        th_tile_cache *c = nullptr;
        if (th_tm_tile_cache(sl.tm, &c) == TH_OK) c->set_revisions(w, s);
    }
}

std::vector<uint32_t> all_slots(const th_tmg *g) {
    std::vector<uint32_t> v(g->slots.size());
    for (size_t i = 0; i < v.size(); i++) v[i] = (uint32_t)i;
    return v;
}

// fn(slot) for every slot of `which`, each on a thread of its own (the caller's thread takes the first).  th_last_error is
// thread-local: a failure is re-raised on the caller's thread with its slot and device (the first failing slot in `which`
// order; every slot has finished by then).
template <class F>
int for_slots(th_tmg *g, const std::vector<uint32_t> &which, F fn) {
    const size_t n = which.size();
    std::vector<int> rc(n, TH_OK);
    std::vector<std::string> msg(n);
    auto run = [&](size_t i) {
        try {
            rc[i] = fn(which[i]);
        } catch (const std::bad_alloc &) {
            rc[i] = fail(TH_ERR_OOM, "host allocation failed");
        } catch (...) {
            rc[i] = fail(TH_ERR_INTERNAL, "exception in slot work");
        }
        if (rc[i] != TH_OK) msg[i] = get_error();
    };
    std::vector<std::thread> thr;
    size_t spawned = 1;
    try {
        for (; spawned < n; spawned++) thr.emplace_back(run, spawned);
    } catch (...) {  // (no more threads: this one runs the rest)
    }
    if (n) run(0);
    for (size_t i = spawned; i < n; i++) run(i);
    for (auto &t : thr) t.join();
    for (size_t i = 0; i < n; i++)
        if (rc[i] != TH_OK) return fail(rc[i], "slot %u (device %d): %s", which[i], g->slots[which[i]].device, msg[i].c_str());
    return TH_OK;
}

// The one coupling: every resident channel's (mn, mx) and every track's sr from all slots, folded in ascending (id, ch) —
// the order one th_tm iterates — by the same global_db_range (so that even a NaN lands where it would there)
tmi::DbRange global_range(th_tmg *g) {
    std::vector<tmi::ChanExtremum> ext;
    std::vector<uint32_t> rates;
    for (auto &sl : g->slots) {
        tmi::list_extrema(sl.tm, &ext);
        tmi::list_rates(sl.tm, &rates);
    }
    std::sort(ext.begin(), ext.end(), [](const tmi::ChanExtremum &a, const tmi::ChanExtremum &b) {
        return std::tie(a.id, a.ch) < std::tie(b.id, b.ch);
    });
    std::vector<float> mins(ext.size()), maxs(ext.size());
    for (size_t i = 0; i < ext.size(); i++) {
        mins[i] = ext[i].mn;
        maxs[i] = ext[i].mx;
    }
    tmi::DbRange r{INFINITY, -INFINITY, 0};
    global_db_range(mins.data(), maxs.data(), mins.size(), g->dB_range, &r.min_dB, &r.max_dB);
    for (uint32_t sr : rates) r.max_sr = std::max(r.max_sr, sr);
    return r;
}

// update_spec_imgs on every slot against the global values; *updated = the ascending union of the slots' ids
int requantise_all(th_tmg *g, bool force_update_all, bool images_only, std::vector<size_t> *updated) {
    const tmi::DbRange r = global_range(g);
    std::vector<std::vector<size_t>> upd(g->slots.size());
    const int rc = for_slots(g, all_slots(g), [&](uint32_t s) -> int {
        std::unique_lock<std::shared_mutex> wl(tmi::rw_of(g->slots[s].tm));
        return tmi::requantise(g->slots[s].tm, &r, force_update_all, images_only, &upd[s]);
    });
    if (updated) {
        std::set<size_t> u;
        for (auto &v : upd) u.insert(v.begin(), v.end());
        updated->assign(u.begin(), u.end());
    }
    return rc;
}

// the slot of a resident track, or NULL
const th_tmg::Placement *find_track(const th_tmg *g, size_t id) {
    auto it = g->where.find(id);
    return it == g->where.end() ? nullptr : &it->second;
}

// th_tmg as the manager of a batched reader (batched_reader.h): every track has one owning slot.  The caller's lock is g->rw; a slot's
// default colormap is uploaded after the short-buffer report, for the busy slots only
struct TmgReaders {
    static constexpr bool single_owner = false;
    th_tmg *g;
    bool null() const { return !g; }
    int before_lock(bool) const { return TH_OK; }
    std::shared_lock<std::shared_mutex> lock() const { return std::shared_lock<std::shared_mutex>(g->rw); }
    uint64_t revision(br::Revision which) const { return which == br::Revision::waveform ? revisions(g).first : revisions(g).second; }
    size_t n_slots() const { return g->slots.size(); }
    bool find(size_t id, uint32_t *slot) const {
        const th_tmg::Placement *p = find_track(g, id);
        if (p) *slot = p->slot;
        return p != nullptr;
    }
    th_tm *owner(uint32_t s) const { return g->slots[s].tm; }
    std::shared_lock<std::shared_mutex> lock_owner(uint32_t s) const { return std::shared_lock<std::shared_mutex>(tmi::rw_of(owner(s))); }
    int before_run(bool colormap, const std::vector<uint32_t> &busy) const {
        if (colormap)
            for (uint32_t s : busy) TH_CHECK(tmi::ensure_colormap(owner(s)));
        return TH_OK;
    }
    template <class F>
    int for_slots(const std::vector<uint32_t> &which, F fn) const { return ::for_slots(g, which, fn); }
};

// Every slot of `which` prepares into a StagedPtr under its write lock (prepare(slot, &staged)); a failure returns with all of them
// discarded, otherwise every one is committed
template <class Prepare>
int prepare_and_commit(th_tmg *g, const std::vector<uint32_t> &which, Prepare prepare) {
    std::vector<tmi::StagedPtr> staged(g->slots.size());
    TH_CHECK(for_slots(g, which, [&](uint32_t s) -> int {
        std::unique_lock<std::shared_mutex> sl(tmi::rw_of(g->slots[s].tm));
        return prepare(s, &staged[s]);
    }));
    for (uint32_t s : which) {
        std::unique_lock<std::shared_mutex> sl(tmi::rw_of(g->slots[s].tm));
        tmi::commit(g->slots[s].tm, std::move(staged[s]));
    }
    return TH_OK;
}

}  // namespace

TH_API int th_tmg_destroy(th_tmg *g) {
    TH_TRY
    if (!g) return TH_OK;
    for (auto &sl : g->slots) {
        if (sl.tm) (void)th_tm_destroy(sl.tm);
        if (sl.ctx) (void)th_ctx_destroy(sl.ctx);
    }
    delete g;
    return TH_OK;
    TH_CATCH
}

TH_API int th_tmg_create(const int *devices, size_t n_devices, th_tmg **out) {
    TH_TRY
    TH_REQUIRE(devices && out, "NULL argument");
    TH_REQUIRE(n_devices >= 1 && n_devices <= 64, "n_devices must be 1 .. 64 (got %zu)", n_devices);
    for (size_t i = 0; i < n_devices; i++) TH_REQUIRE(devices[i] >= 0, "devices[%zu] = %d is negative", i, devices[i]);
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(TH_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    for (size_t i = 0; i < n_devices; i++)
        TH_REQUIRE(devices[i] < n, "devices[%zu] = %d out of range (have %d)", i, devices[i], n);
    std::unique_ptr<th_tmg, int (*)(th_tmg *)> g(new th_tmg(), th_tmg_destroy);
    g->slots.resize(n_devices);
    for (size_t i = 0; i < n_devices; i++) {
        th_tmg::Slot &sl = g->slots[i];
        sl.device = devices[i];
        int rc = th_ctx_create(devices[i], nullptr, &sl.ctx);
        if (rc == TH_OK) rc = th_tm_create(sl.ctx, &sl.tm);
        if (rc != TH_OK) return fail(rc, "slot %zu (device %d): %s", i, devices[i], th_last_error());
    }
    sync_revisions(g.get());
    *out = g.release();
    return TH_OK;
    TH_CATCH
}

TH_API int th_tmg_n_devices(const th_tmg *g, size_t *n) {
    TH_TRY
    TH_REQUIRE(g && n, "NULL argument");
    *n = g->slots.size();
    return TH_OK;
    TH_CATCH
}

TH_API int th_tmg_track_device(const th_tmg *g, size_t id, uint32_t *slot) {
    TH_TRY
    TH_REQUIRE(g && slot, "NULL argument");
    std::shared_lock<std::shared_mutex> rl(g->rw);
    const th_tmg::Placement *p = find_track(g, id);
    if (!p) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", id);
    *slot = p->slot;
    return TH_OK;
    TH_CATCH
}

TH_API int th_tmg_set_colormap(th_tmg *g, const uint8_t *rgba, size_t bytes) {
    TH_TRY
    TH_REQUIRE(g && rgba, "NULL argument");
    std::unique_lock<std::shared_mutex> wl(g->rw);
    int rc = for_slots(g, all_slots(g), [&](uint32_t s) -> int {
        std::unique_lock<std::shared_mutex> sl(tmi::rw_of(g->slots[s].tm));
        return tmi::set_colormap_only(g->slots[s].tm, rgba, bytes);
    });
    if (rc != TH_OK) return rc;
    g->revs.invalidate_spectrogram();
    sync_revisions(g);
    return requantise_all(g, true, false, nullptr);
    TH_CATCH
}

TH_API int th_tmg_set_setting(th_tmg *g, double win_ms, uint32_t t_overlap, uint32_t f_overlap, int freq_scale) {
    TH_TRY
    TH_REQUIRE(g, "tmg is NULL");
    TH_REQUIRE(win_ms > 0. && t_overlap >= 1 && f_overlap >= 1, "invalid SpecSetting (lib.rs:275-277)");
    TH_REQUIRE(freq_scale == TH_FREQ_LINEAR || freq_scale == TH_FREQ_MEL, "bad freq_scale");
    std::unique_lock<std::shared_mutex> wl(g->rw);
    // every slot prepares (new plans and specs beside the resident ones); all commit, or all discard
    TH_CHECK(prepare_and_commit(g, all_slots(g), [&](uint32_t s, tmi::StagedPtr *staged) {
        return tmi::prepare_setting(g->slots[s].tm, win_ms, t_overlap, f_overlap, freq_scale, staged);
    }));
    const int rc = requantise_all(g, true, false, nullptr);
    g->revs.invalidate_spectrogram();  // lib.rs:284
    sync_revisions(g);
    return rc;
    TH_CATCH
}

TH_API int th_tmg_set_dB_range(th_tmg *g, float dB_range) {
    TH_TRY
    TH_REQUIRE(g, "tmg is NULL");
    TH_REQUIRE(dB_range > 0.f, "dB_range must be > 0 (lib.rs:259)");
    std::unique_lock<std::shared_mutex> wl(g->rw);
    g->dB_range = dB_range;
    const int rc = requantise_all(g, true, true, nullptr);
    g->revs.invalidate_spectrogram();  // lib.rs:265
    sync_revisions(g);
    return rc;
    TH_CATCH
}

TH_API int th_tmg_add_tracks(th_tmg *g, size_t n_tracks, const size_t *ids, const uint32_t *srs, const uint32_t *n_channels,
                             const float *const *channels_flat, const size_t *n_samples) {
    TH_TRY
    TH_REQUIRE(g && ids && srs && n_channels && channels_flat && n_samples, "NULL argument");
    TH_REQUIRE(n_tracks >= 1, "no tracks (lib.rs:182)");
    std::vector<size_t> flat0(n_tracks, 0);
    {   // validate everything before anything is allocated (th_tm_add_tracks)
        size_t flat = 0;
        for (size_t t = 0; t < n_tracks; t++) {
            TH_REQUIRE(srs[t] > 0 && n_channels[t] >= 1 && n_samples[t] >= 1, "track %zu: empty or invalid", ids[t]);
            flat0[t] = flat;
            for (uint32_t k = 0; k < n_channels[t]; k++, flat++)
                TH_REQUIRE(channels_flat[flat], "track %zu channel %u: NULL data", ids[t], k);
        }
    }
    std::unique_lock<std::shared_mutex> wl(g->rw);
    const uint32_t n_slots = (uint32_t)g->slots.size();
    // the same id twice in one call: the later one wins, as in th_tm_add_tracks — only it goes to a slot
    std::map<size_t, size_t> last_of;
    for (size_t t = 0; t < n_tracks; t++) last_of[ids[t]] = t;
    // placement: a resident id stays on its slot; new ids longest-first (weight = n_samples x n_channels, ties in input
    // order) to the slot with the least resident weight (ties: the lowest slot) — shard_assign from the resident loads
    std::vector<uint64_t> load(n_slots, 0);
    for (auto &kv : g->where) load[kv.second.slot] += kv.second.weight;
    std::vector<size_t> fresh;  // input indices of the new ids
    std::vector<uint64_t> weight(n_tracks, 0);
    for (size_t t = 0; t < n_tracks; t++) {
        weight[t] = (uint64_t)n_samples[t] * n_channels[t];
        if (last_of[ids[t]] == t && !find_track(g, ids[t])) fresh.push_back(t);
    }
    std::vector<uint64_t> fw(fresh.size());
    for (size_t i = 0; i < fresh.size(); i++) fw[i] = weight[fresh[i]];
    std::vector<uint32_t> owner(fresh.size(), 0);
    shard_assign(fw.data(), fw.size(), n_slots, owner.data(), load.data());
    std::vector<uint32_t> slot_of(n_tracks, 0);
    for (size_t i = 0; i < fresh.size(); i++) slot_of[fresh[i]] = owner[i];
    // each slot's share of the batch, in input order
    struct Batch {
        std::vector<size_t> ids, ns;
        std::vector<uint32_t> srs, nch;
        std::vector<const float *> chans;
    };
    std::vector<Batch> batch(n_slots);
    for (size_t t = 0; t < n_tracks; t++) {
        if (last_of[ids[t]] != t) continue;
        const th_tmg::Placement *p = find_track(g, ids[t]);
        if (p) slot_of[t] = p->slot;
        Batch &b = batch[slot_of[t]];
        b.ids.push_back(ids[t]);
        b.srs.push_back(srs[t]);
        b.nch.push_back(n_channels[t]);
        b.ns.push_back(n_samples[t]);
        for (uint32_t k = 0; k < n_channels[t]; k++) b.chans.push_back(channels_flat[flat0[t] + k]);
    }
    std::vector<uint32_t> busy;
    for (uint32_t s = 0; s < n_slots; s++)
        if (!batch[s].ids.empty()) busy.push_back(s);
    // every slot stages its tracks (upload, waveform pyramids, STFT); all commit, or all discard
    TH_CHECK(prepare_and_commit(g, busy, [&](uint32_t s, tmi::StagedPtr *staged) {
        const Batch &b = batch[s];
        return tmi::prepare_add(g->slots[s].tm, b.ids.size(), b.ids.data(), b.srs.data(), b.nch.data(), b.chans.data(), b.ns.data(), staged);
    }));
    for (size_t t = 0; t < n_tracks; t++)
        if (last_of[ids[t]] == t) g->where[ids[t]] = th_tmg::Placement{slot_of[t], weight[t]};
    g->revs.invalidate_all();  // lib.rs:192
    sync_revisions(g);
    for (uint32_t s : busy) {
        const int rc = tmi::settle(g->slots[s].tm);
        if (rc != TH_OK) return fail(rc, "slot %u (device %d): %s", s, g->slots[s].device, get_error());
    }
    return TH_OK;
    TH_CATCH
}

TH_API int th_tmg_remove_track(th_tmg *g, size_t id) {
    TH_TRY
    TH_REQUIRE(g, "tmg is NULL");
    std::unique_lock<std::shared_mutex> wl(g->rw);
    const th_tmg::Placement *p = find_track(g, id);
    if (!p) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", id);
    const uint32_t s = p->slot;
    const int rc = th_tm_remove_track(g->slots[s].tm, id);
    if (rc != TH_OK) return fail(rc, "slot %u (device %d): %s", s, g->slots[s].device, get_error());
    g->where.erase(id);
    g->revs.invalidate_all();  // lib.rs:221
    sync_revisions(g);
    return TH_OK;
    TH_CATCH
}

TH_API int th_tmg_apply_track_list_changes(th_tmg *g, size_t *updated_ids, size_t cap, size_t *n_updated, uint32_t *max_sr) {
    TH_TRY
    TH_REQUIRE(g, "tmg is NULL");
    std::unique_lock<std::shared_mutex> wl(g->rw);
    std::vector<size_t> upd;
    const int rc = requantise_all(g, false, true, &upd);
    if (rc != TH_OK) return rc;
    if (n_updated) *n_updated = upd.size();
    if (updated_ids)
        for (size_t i = 0; i < upd.size() && i < cap; i++) updated_ids[i] = upd[i];
    if (max_sr) {
        float lo, hi;
        (void)th_tm_get_db_state(g->slots[0].tm, &lo, &hi, max_sr);  // (every slot holds the global values)
    }
    if (!upd.empty()) {  // lib.rs:243-245
        g->revs.invalidate_spectrogram();
        sync_revisions(g);
    }
    return TH_OK;
    TH_CATCH
}

TH_API int th_tmg_get_db_state(const th_tmg *g, float *min_dB, float *max_dB, uint32_t *max_sr) {
    TH_TRY
    TH_REQUIRE(g, "tmg is NULL");
    std::shared_lock<std::shared_mutex> rl(g->rw);
    return th_tm_get_db_state(g->slots[0].tm, min_dB, max_dB, max_sr);  // (every slot holds the global values)
    TH_CATCH
}

// ---------------------------------------------------------------------------------------------- readers: the owning slot
#define TMG_OWNER(g, id, what, ...)                                                        \
    TH_REQUIRE(g, "tmg is NULL");                                                          \
    std::shared_lock<std::shared_mutex> rl((g)->rw);                                       \
    const th_tmg::Placement *p_ = find_track(g, id);                                       \
    if (!p_) return fail(TH_ERR_NOT_FOUND, what " does not exist", __VA_ARGS__);          \
    th_tm *tm_ = (g)->slots[p_->slot].tm

TH_API int th_tmg_spec_shape(const th_tmg *g, size_t id, uint32_t ch, size_t *n_frames, size_t *height) {
    TH_TRY
    TMG_OWNER(g, id, "Spectrogram %zu_%u", id, ch);
    return th_tm_spec_shape(tm_, id, ch, n_frames, height);
    TH_CATCH
}

TH_API int th_tmg_img_shape(const th_tmg *g, size_t id, uint32_t ch, size_t *img_height, size_t *img_width) {
    TH_TRY
    TMG_OWNER(g, id, "Spectrogram %zu_%u", id, ch);
    return th_tm_img_shape(tm_, id, ch, img_height, img_width);
    TH_CATCH
}

TH_API int th_tmg_copy_spec(th_tmg *g, size_t id, uint32_t ch, float *out, size_t capacity_floats) {
    TH_TRY
    TMG_OWNER(g, id, "Spectrogram %zu_%u", id, ch);
    return th_tm_copy_spec(tm_, id, ch, out, capacity_floats);
    TH_CATCH
}

TH_API int th_tmg_copy_img(th_tmg *g, size_t id, uint32_t ch, uint16_t *out, size_t capacity_px) {
    TH_TRY
    TMG_OWNER(g, id, "Spectrogram %zu_%u", id, ch);
    return th_tm_copy_img(tm_, id, ch, out, capacity_px);
    TH_CATCH
}

TH_API int th_tmg_revisions(const th_tmg *g, uint64_t *waveform_revision, uint64_t *spectrogram_revision) {
    TH_TRY
    TH_REQUIRE(g, "tmg is NULL");
    const auto [w, s] = revisions(g);
    if (waveform_revision) *waveform_revision = w;
    if (spectrogram_revision) *spectrogram_revision = s;
    return TH_OK;
    TH_CATCH
}

TH_API int th_tmg_get_spectrogram_tile(th_tmg *g, size_t id, uint32_t ch, uint32_t level_x, uint32_t level_y, uint32_t tile_x,
                                       uint32_t tile_y, uint8_t *out, size_t out_capacity, size_t *out_len) {
    TH_TRY
    TMG_OWNER(g, id, "Spectrogram %zu_%u", id, ch);
    return th_tm_get_spectrogram_tile(tm_, id, ch, level_x, level_y, tile_x, tile_y, out, out_capacity, out_len);
    TH_CATCH
}

TH_API int th_tmg_get_waveform_tile(th_tmg *g, size_t id, uint32_t ch, uint32_t level, uint32_t tile_index, uint8_t *out,
                                    size_t out_capacity, size_t *out_len) {
    TH_TRY
    TMG_OWNER(g, id, "Track %zu", id);
    return th_tm_get_waveform_tile(tm_, id, ch, level, tile_index, out, out_capacity, out_len);
    TH_CATCH
}

TH_API int th_tmg_get_audio_stats(th_tmg *g, size_t id, th_audio_stats *out) {
    TH_TRY
    TMG_OWNER(g, id, "Track %zu", id);
    return th_tm_get_audio_stats(tm_, id, out);
    TH_CATCH
}

TH_API int th_tmg_get_audio_render_metadata(th_tmg *g, size_t id, uint32_t ch, double track_sec, int is_clipped,
                                            th_render_metadata *out) {
    TH_TRY
    TMG_OWNER(g, id, "Track %zu", id);
    return th_tm_get_audio_render_metadata(tm_, id, ch, track_sec, is_clipped, out);
    TH_CATCH
}

// The batched readers go through br::batched_read (batched_reader.h) with TmgReaders: every owning slot runs its subset side by side and
// writes its results straight to their places in the caller's buffer.  The tiles return offsets instead of infos and stamp nothing
// (the headers' revision: every slot carries the manager's), so their entry is written out with the same pieces.
TH_API int th_tmg_get_spectrogram_tiles(th_tmg *g, const th_tile_request *reqs, size_t n, uint8_t *out, size_t out_capacity,
                                        size_t *offsets, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(g && out_len && (n == 0 || (reqs && offsets)), "NULL argument");
    *out_len = 0;
    if (n == 0) {
        if (offsets) offsets[0] = 0;
        return TH_OK;
    }
    TmgReaders m{g};
    const auto rl = m.lock();
    std::vector<tmi::TileInfo> infos(n);
    br::Split sp;
    TH_CHECK(br::check_and_split(m, n, [&](size_t i) { return reqs[i].id; },
                                 [&](th_tm *tm, size_t i) { return tmi::tile_request_info(tm, reqs[i], &infos[i]); }, &sp));
    const size_t total = tmi::tiles_layout(infos.data(), n, offsets);
    *out_len = total;
    if (out_capacity < total || !out) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu bytes", total);
    TH_CHECK(m.before_run(true, sp.busy));
    return br::run_on_owners(m, sp, [&](th_tm *tm, const std::vector<size_t> &idx) -> int {
        std::vector<tmi::TileInfo> sub(idx.size());
        for (size_t j = 0; j < idx.size(); j++) sub[j] = infos[idx[j]];
        return tmi::tiles_run(tm, idx.size(), sub.data(), out);
    });
    TH_CATCH
}

TH_API int th_tmg_get_spectra(th_tmg *g, const th_spectrum_request *reqs, size_t n, float *out, size_t cap, th_spectrum_info *info,
                              size_t *out_len) {
    TH_TRY
    return br::batched_read<tmi::SpectrumReader>(TmgReaders{g}, reqs, n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tmg_get_spectrum(th_tmg *g, size_t id, uint32_t ch, int kind, double start_sec, double end_sec, float *out, size_t cap,
                               th_spectrum_info *info) {
    TH_TRY
    TH_REQUIRE(g, "tmg is NULL");
    TH_REQUIRE(kind >= 0, "unknown spectrum kind %d", kind);
    const th_spectrum_request r{id, ch, (uint32_t)kind, start_sec, end_sec};
    return br::single_read(info, [&](th_spectrum_info *one, size_t *len) { return th_tmg_get_spectra(g, &r, 1, out, cap, one, len); });
    TH_CATCH
}

TH_API int th_tmg_get_loudness_meters(th_tmg *g, const size_t *ids, size_t n, th_loudness_meter *meters, double *series, size_t cap,
                                      size_t *out_len) {
    TH_TRY
    TH_REQUIRE(meters, "NULL argument");  // (also for n == 0)
    return br::batched_read<tmi::MeterReader>(TmgReaders{g}, ids, n, series, cap, meters, out_len);
    TH_CATCH
}

TH_API int th_tmg_get_loudness_meter(th_tmg *g, size_t id, th_loudness_meter *meter, double *series, size_t cap) {
    TH_TRY
    TH_REQUIRE(g && meter, "NULL argument");
    size_t len = 0;
    return th_tmg_get_loudness_meters(g, &id, 1, meter, series, cap, &len);
    TH_CATCH
}

// Export: a slot also writes the zero padding behind each of its requests, and its two counts come back into infos.  The WAV form is
// one request behind a header: checked, stamped and run with the same pieces
namespace {
int tmg_export_pcm_any(th_tmg *g, const tmi::ExportReq *reqs, size_t n, uint8_t *out, size_t cap, th_export_info *info, size_t *out_len) {
    return br::batched_read<tmi::ExportReader>(TmgReaders{g}, reqs, n, out, cap, info, out_len);
}

int tmg_export_wav_any(th_tmg *g, const tmi::ExportReq *req, uint8_t *out, size_t cap, th_export_info *info, size_t *out_len) {
    TH_REQUIRE(g && req && out_len, "NULL argument");
    *out_len = 0;
    TmgReaders m{g};
    const auto rl = m.lock();
    tmi::ExportInfo one{};
    br::Split sp;
    TH_CHECK(br::check_and_split(m, 1, [&](size_t) { return req->base.id; },
                                 [&](th_tm *tm, size_t i) { return tmi::export_request_info(tm, *req, i, &one); }, &sp));
    one.waveform_revision = m.revision(br::Revision::waveform);
    uint8_t hdr[TH_WAV_HEADER_MAX];
    size_t hl = 0, pl = 0;
    TH_CHECK(tmi::wav_header_checked(req->base.format, one.sr, one.n_channels, one.sample_end - one.sample_start, hdr, &hl, &pl));
    one.offset = hl;
    const size_t total = hl + (size_t)one.n_bytes + pl;
    if (info) *info = one;
    *out_len = total;
    if (cap < total || !out) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu bytes", total);
    TH_CHECK(br::run_on_owners(m, sp, [&](th_tm *tm, const std::vector<size_t> &) { return tmi::export_run(tm, 1, &one, out); }));
    std::memcpy(out, hdr, hl);
    if (pl) out[hl + one.n_bytes] = 0;
    if (info) *info = one;
    return TH_OK;
}
}  // namespace

TH_API int th_tmg_export_pcm(th_tmg *g, const th_export_request *reqs, size_t n, uint8_t *out, size_t cap, th_export_info *info,
                             size_t *out_len) {
    TH_TRY
    TH_REQUIRE(n == 0 || reqs, "NULL argument");
    return tmg_export_pcm_any(g, tmi::export_requests(reqs, n).data(), n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tmg_export_wav(th_tmg *g, const th_export_request *req, uint8_t *out, size_t cap, th_export_info *info, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(req, "NULL argument");
    const tmi::ExportReq one = tmi::export_req(*req);
    return tmg_export_wav_any(g, &one, out, cap, info, out_len);
    TH_CATCH
}

// FLAC: a slot writes its requests' files at the batch's offsets; the actual lengths and the counts come back into infos
TH_API int th_tmg_export_flac(th_tmg *g, const th_export_request *reqs, size_t n, uint8_t *out, size_t cap, th_export_info *info,
                              size_t *out_len) {
    TH_TRY
    return tmi::flac_read(TmgReaders{g}, reqs, n, 0u, out, cap, info, out_len);
    TH_CATCH
}
TH_API int th_tmg_export_flac_ex(th_tmg *g, const th_export_request *reqs, size_t n, uint32_t flags, uint8_t *out, size_t cap,
                                 th_export_info *info, size_t *out_len) {
    TH_TRY
    return tmi::flac_read(TmgReaders{g}, reqs, n, flags, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tmg_export_pcm_at(th_tmg *g, const th_export_at_request *reqs, size_t n, uint8_t *out, size_t cap, th_export_info *info,
                                size_t *out_len) {
    TH_TRY
    TH_REQUIRE(n == 0 || reqs, "NULL argument");
    return tmg_export_pcm_any(g, tmi::export_requests(reqs, n).data(), n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tmg_export_wav_at(th_tmg *g, const th_export_at_request *req, uint8_t *out, size_t cap, th_export_info *info, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(req, "NULL argument");
    const tmi::ExportReq one = tmi::export_req(*req);
    return tmg_export_wav_any(g, &one, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tmg_export_pcm_band(th_tmg *g, const th_export_band_request *reqs, size_t n, uint8_t *out, size_t cap, th_export_info *info,
                                  size_t *out_len) {
    TH_TRY
    TH_REQUIRE(n == 0 || reqs, "NULL argument");
    return tmg_export_pcm_any(g, tmi::export_requests(reqs, n).data(), n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tmg_export_wav_band(th_tmg *g, const th_export_band_request *req, uint8_t *out, size_t cap, th_export_info *info,
                                  size_t *out_len) {
    TH_TRY
    TH_REQUIRE(req, "NULL argument");
    const tmi::ExportReq one = tmi::export_req(*req);
    return tmg_export_wav_any(g, &one, out, cap, info, out_len);
    TH_CATCH
}

// Figures: every busy slot needs its device colormap first, as for the tiles
TH_API int th_tmg_render_figures(th_tmg *g, const th_figure_request *reqs, size_t n, uint8_t *out, size_t cap, th_figure_info *info,
                                 size_t *out_len) {
    TH_TRY
    return br::batched_read<tmi::FigureReader>(TmgReaders{g}, reqs, n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tmg_render_figure(th_tmg *g, const th_figure_request *req, uint8_t *out, size_t cap, th_figure_info *info) {
    TH_TRY
    TH_REQUIRE(g && req, "NULL argument");
    return br::single_read(info, [&](th_figure_info *one, size_t *len) { return th_tmg_render_figures(g, req, 1, out, cap, one, len); });
    TH_CATCH
}

TH_API int th_tmg_figure_box(th_tmg *g, size_t id, uint32_t ch, double start_sec, double end_sec, double hz_min, double hz_max,
                             double *left, double *top, double *width, double *height) {
    TH_TRY
    TH_REQUIRE(left && top && width && height, "NULL argument");
    TMG_OWNER(g, id, "Track %zu", id);
    return th_tm_figure_box(tm_, id, ch, start_sec, end_sec, hz_min, hz_max, left, top, width, height);
    TH_CATCH
}

// set_common_normalize / set_common_guard_clipping: every slot re-derives its tracks into staged buffers; all commit, or all discard
namespace {
int set_common_dynamics_all(th_tmg *g, int kind, float target, int mode) {
    TH_CHECK(prepare_and_commit(g, all_slots(g), [&](uint32_t s, tmi::StagedPtr *staged) {
        return tmi::prepare_dynamics(g->slots[s].tm, kind, target, mode, staged);
    }));
    const int rc = requantise_all(g, true, false, nullptr);
    g->revs.invalidate_all();
    sync_revisions(g);
    return rc;
}
}  // namespace

TH_API int th_tmg_set_common_normalize(th_tmg *g, int kind, float target) {
    TH_TRY
    TH_REQUIRE(g, "tmg is NULL");
    std::unique_lock<std::shared_mutex> wl(g->rw);
    int mode = 0;
    tmi::get_common_dynamics(g->slots[0].tm, nullptr, nullptr, &mode);  // (every slot holds the common settings)
    return set_common_dynamics_all(g, kind, target, mode);
    TH_CATCH
}

TH_API int th_tmg_set_common_guard_clipping(th_tmg *g, int mode) {
    TH_TRY
    TH_REQUIRE(g, "tmg is NULL");
    std::unique_lock<std::shared_mutex> wl(g->rw);
    int kind = 0;
    float target = 0.0f;
    tmi::get_common_dynamics(g->slots[0].tm, &kind, &target, nullptr);
    return set_common_dynamics_all(g, kind, target, mode);
    TH_CATCH
}

TH_API int th_tmg_get_common_dynamics(th_tmg *g, int *kind, float *target, int *mode) {
    TH_TRY
    TH_REQUIRE(g, "tmg is NULL");
    std::shared_lock<std::shared_mutex> rl(g->rw);
    return th_tm_get_common_dynamics(g->slots[0].tm, kind, target, mode);
    TH_CATCH
}

TH_API int th_tmg_get_track_dynamics(th_tmg *g, size_t id, th_track_dynamics *out) {
    TH_TRY
    TMG_OWNER(g, id, "Track %zu", id);
    return th_tm_get_track_dynamics(tm_, id, out);
    TH_CATCH
}

TH_API int th_tmg_get_guard_clip_stats(th_tmg *g, size_t id, th_guard_clip_stats *out, size_t cap, size_t *n) {
    TH_TRY
    TMG_OWNER(g, id, "Track %zu", id);
    return th_tm_get_guard_clip_stats(tm_, id, out, cap, n);
    TH_CATCH
}

TH_API int th_tmg_get_limiter_gain(th_tmg *g, size_t id, float *out, size_t cap, size_t *n) {
    TH_TRY
    TMG_OWNER(g, id, "Track %zu", id);
    return th_tm_get_limiter_gain(tm_, id, out, cap, n);
    TH_CATCH
}

TH_API int th_tmg_copy_audio(th_tmg *g, size_t id, uint32_t ch, int which, float *out, size_t cap) {
    TH_TRY
    TMG_OWNER(g, id, "Track %zu", id);
    return th_tm_copy_audio(tm_, id, ch, which, out, cap);
    TH_CATCH
}

TH_API int th_tmg_set_lod_source(th_tmg *g, int per_request) {
    TH_TRY
    TH_REQUIRE(g, "tmg is NULL");
    std::unique_lock<std::shared_mutex> wl(g->rw);
    const int want = per_request ? 1 : 0;
    if (want == g->lod_source) return TH_OK;
    std::vector<int> done(g->slots.size(), 0);
    const int rc = for_slots(g, all_slots(g), [&](uint32_t s) -> int {
        const int r = th_tm_set_lod_source(g->slots[s].tm, want);
        done[s] = r == TH_OK;
        return r;
    });
    if (rc != TH_OK) {  // failure-atomic like th_tm_set_lod_source: the slots that switched go back
        const std::string msg = get_error();
        for (size_t s = 0; s < done.size(); s++)
            if (done[s]) (void)th_tm_set_lod_source(g->slots[s].tm, g->lod_source);
        return fail(rc, "%s", msg.c_str());
    }
    g->lod_source = want;
    return TH_OK;
    TH_CATCH
}

// Waveform envelopes and lanes
TH_API int th_tmg_get_envelopes(th_tmg *g, const th_envelope_request *reqs, size_t n, float *out, size_t cap, th_envelope_info *info,
                                size_t *out_len) {
    TH_TRY
    return br::batched_read<tmi::EnvelopeReader>(TmgReaders{g}, reqs, n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tmg_get_envelope(th_tmg *g, const th_envelope_request *req, float *out, size_t cap, th_envelope_info *info) {
    TH_TRY
    TH_REQUIRE(g && req, "NULL argument");
    return br::single_read(info, [&](th_envelope_info *one, size_t *len) { return th_tmg_get_envelopes(g, req, 1, out, cap, one, len); });
    TH_CATCH
}

// Formant candidates: a slot's two counts come back into infos
TH_API int th_tmg_get_formants(th_tmg *g, const th_formant_request *reqs, size_t n, double *out, size_t cap, th_formant_info *info,
                               size_t *out_len) {
    TH_TRY
    return br::batched_read<tmi::FormantReader>(TmgReaders{g}, reqs, n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tmg_get_formant_track(th_tmg *g, const th_formant_request *req, double *out, size_t cap, th_formant_info *info) {
    TH_TRY
    TH_REQUIRE(g && req, "NULL argument");
    return br::single_read(info, [&](th_formant_info *one, size_t *len) { return th_tmg_get_formants(g, req, 1, out, cap, one, len); });
    TH_CATCH
}

// Alignment: the probe's slot owns a request; the reference is found in the manager's track table (under g->rw, which the driver
// holds from the check to the run) and, where it lives on another slot, staged by the run
namespace {
th_tm *align_home_of(void *who, size_t id) {
    const th_tmg *g = static_cast<const th_tmg *>(who);
    const th_tmg::Placement *p = find_track(g, id);
    return p ? g->slots[p->slot].tm : nullptr;
}
}  // namespace

TH_API int th_tmg_align_tracks(th_tmg *g, const th_align_request *reqs, size_t n, double *out, size_t cap, th_align_info *info, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(n == 0 || reqs, "NULL argument");
    return br::batched_read<tmi::AlignReader>(TmgReaders{g}, tmi::align_requests(reqs, n, align_home_of, g).data(), n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tmg_align_track(th_tmg *g, const th_align_request *req, double *out, size_t cap, th_align_info *info) {
    TH_TRY
    TH_REQUIRE(g && req, "NULL argument");
    return br::single_read(info, [&](th_align_info *one, size_t *len) { return th_tmg_align_tracks(g, req, 1, out, cap, one, len); });
    TH_CATCH
}

TH_API int th_tmg_render_waveform_figures(th_tmg *g, const th_waveform_figure_request *reqs, size_t n, uint8_t *out, size_t cap,
                                          th_waveform_figure_info *info, size_t *out_len) {
    TH_TRY
    return br::batched_read<tmi::WaveformFigureReader>(TmgReaders{g}, reqs, n, out, cap, info, out_len);
    TH_CATCH
}

TH_API int th_tmg_render_waveform_figure(th_tmg *g, const th_waveform_figure_request *req, uint8_t *out, size_t cap,
                                         th_waveform_figure_info *info) {
    TH_TRY
    TH_REQUIRE(g && req, "NULL argument");
    return br::single_read(info,
                           [&](th_waveform_figure_info *one, size_t *len) { return th_tmg_render_waveform_figures(g, req, 1, out, cap, one, len); });
    TH_CATCH
}
