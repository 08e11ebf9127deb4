// track_manager_internal.h — what th_tmg (track_manager_multi.hip) drives inside each slot's th_tm (track_manager.hip).
// Not part of the C ABI.  None of these functions takes the manager's lock: the caller holds rw_of(tm) (or has the only
// reference to the manager), exactly as the th_tm_* entry points do around the same steps.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <shared_mutex>
#include <vector>

#include "common.h"

namespace th {
namespace tmi {

std::shared_mutex &rw_of(th_tm *tm);

// The global values the image step quantises against (update_spec_imgs, core/mod.rs:169-185)
struct DbRange {
    float min_dB, max_dB;
    uint32_t max_sr;
};

// (mn, mx) of every channel that has a spec, in ascending (id, ch) — the order update_spec_imgs folds them in
struct ChanExtremum {
    size_t id;
    uint32_t ch;
    float mn, mx;
};
void list_extrema(th_tm *tm, std::vector<ChanExtremum> *out);
// sample rate of every resident track (TrackList::max_sr folds these)
void list_rates(th_tm *tm, std::vector<uint32_t> *out);

// Work staged beside the manager by a prepare step (plans, specs and, for add_tracks, whole tracks), not yet visible to it.
// commit() swaps it in and cannot fail; destroying a Staged that was not committed frees all of it (the discard).
struct Staged;
struct StagedDeleter {
    void operator()(Staged *s) const;
};
using StagedPtr = std::unique_ptr<Staged, StagedDeleter>;

// set_setting (core/mod.rs:107-115): the plans and specs of the new setting for every resident channel
int prepare_setting(th_tm *tm, double win_ms, uint32_t t_overlap, uint32_t f_overlap, int freq_scale, StagedPtr *out);
// add_tracks (core/mod.rs:62-71): arguments as th_tm_add_tracks, already validated
int prepare_add(th_tm *tm, size_t n_tracks, const size_t *ids, const uint32_t *srs, const uint32_t *n_channels,
                const float *const *channels_flat, const size_t *n_samples, StagedPtr *out);
// set_common_normalize / set_common_guard_clipping: every track's audio re-derived from its original, and the specs of the channels
// it changes; TH_ERR_INVALID_ARG for an unknown kind or mode
int prepare_dynamics(th_tm *tm, int kind, float target, int mode, StagedPtr *out);
void get_common_dynamics(th_tm *tm, int *kind, float *target, int *mode);
void commit(th_tm *tm, StagedPtr staged);

// th_tm_get_spectra's check of ONE request (i: its index in the caller's batch, for the message), with the codes and in the order
// th_tm_get_spectra reports them; *info: offset 0, the spec's height, the frame range and the slot's spectrogram revision
int spectrum_request_info(th_tm *tm, const th_spectrum_request &r, size_t i, th_spectrum_info *info);

// th_tm_get_loudness_meters' check of ONE id: TH_ERR_NOT_FOUND, else the meter's oversampling, counts (offsets 0) and the slot's
// waveform revision, everything else zero
int loudness_meter_info(th_tm *tm, size_t id, th_loudness_meter *m);

// th_tm_export_pcm in three steps (th_tmg runs them per owning slot).  export_request_info: the check of ONE request with the codes
// and in the order th_tm_export_pcm reports them; *info: offset 0, the byte count, the sample range, rate, channels, counts 0 and the
// slot's waveform revision.  export_layout: the offsets (multiples of 16 in request order), the zero bytes behind every request
// (pad[i]: up to the next offset; 0 behind the last) and the bytes of the whole image.  export_run: the device work for requests
// that were checked and laid out: request i's bytes, then pad[i] zero bytes, to out + info[i].offset (ascending in i; they need not
// be adjacent), and its two counts into info[i].  Takes a reader slot; the caller holds the lock (shared)
// Every request carries its output rate (th_export_at_request; sr_out 0: the track's own, which is all th_tm_export_pcm asks for:
// export_at_requests); info->sr is the rate the request comes out at, and a request whose info->sr is not the track's is resampled
// by export_run (kernels_resample.hip into the slot's planar scratch, then the same export kernel)
int export_request_info(th_tm *tm, const th_export_at_request &r, size_t i, th_export_info *info);
void export_layout(th_export_info *info, size_t n, uint32_t *pad, size_t *out_len);
int export_run(th_tm *tm, const th_export_at_request *reqs, size_t n, th_export_info *info, const uint32_t *pad, uint8_t *out);
std::vector<th_export_at_request> export_at_requests(const th_export_request *reqs, size_t n);
// th_wav_header with the status reported (host_math.h wav_header)
int wav_header_checked(uint32_t format, uint32_t sr, uint32_t n_ch, uint64_t n_frames, uint8_t out[TH_WAV_HEADER_MAX], size_t *header_len,
                       size_t *pad_len);

// update_spec_imgs against `global` (NULL: the manager's own tracks, as th_tm_* does), then the writer's final wait:
// for the images only (apply_track_list_changes, set_dB_range) or for everything (set_setting, set_colormap)
int requantise(th_tm *tm, const DbRange *global, bool force_update_all, bool images_only, std::vector<size_t> *updated);
// set_colormap without its image step: the LUT (kept when malformed, render_tiles.rs:80-85) and colormap_length
int set_colormap_only(th_tm *tm, const uint8_t *rgba, size_t bytes);
// the writer's final wait (the context stream idle, host copies of uploads released)
int settle(th_tm *tm);

}  // namespace tmi
}  // namespace th
