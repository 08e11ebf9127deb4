// track_manager_internal.h — what th_tmg (track_manager_multi.hip) drives inside each slot's th_tm (track_manager.hip).
// Not part of the C ABI.  None of these functions takes the manager's lock: the caller holds rw_of(tm) (or has the only
// reference to the manager), exactly as the th_tm_* entry points do around the same steps.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <shared_mutex>
#include <vector>

#include "batched_reader.h"
#include "align_plan.h"
#include "common.h"
#include "envelope_plan.h"
#include "figure_plan.h"
#include "formant_plan.h"
#include "host_math.h"

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

// The batched readers (spectra, loudness meters, export, figures, envelopes, waveform figures, formants, alignment): each is a traits struct,
// beside its Info, that batched_reader.h's br::batched_read drives over either manager: NULL arguments, n == 0, the shared lock, every
// request checked in request order, the layout, the manager's revision stamped, the infos and the length published, a short buffer
// reported, the run, the infos published again where the run updates them.  th_tm is one owner: every request is checked against it
// and the run gets the caller's arrays as they are.  th_tmg checks each request against its owning slot and hands every slot its
// subset for the run.  The spectrogram tiles (an offsets array instead of infos) and the WAV entries (a header in front of one
// request) have entry points of their own that use the same pieces.
//   Locks: none of these takes rw; the caller holds rw_of(tm) shared around each call (ensure_colormap is the exception).
//   check (*_request_info): ONE request, with the codes and in the order the th_tm entry reports them (i: the request's index in the
//     caller's batch, for the message).  *info then holds everything that is known without the GPU, with its offset(s) 0, and what
//     the run needs of the request and of the manager, so that the run looks nothing up again (valid until a writer gets in: th_tm
//     holds rw from the check to the run, th_tmg its own rw, which every writer of its slots takes first).  The revision is the
//     driver's to stamp, its own manager's.
//   layout: the offset of every info, in request order; returns the length of the whole output.
//   run (*_run): the device work for n requests that were checked and laid out.  It takes a reader slot, packs its own n results in
//     the slot's areas and writes request i's to out + info[i].offset and nowhere else: the destinations ascend with i and need not be
//     adjacent (the caller may hold a subset of a larger batch), so whatever lies between them is left alone.  The limits of one
//     launch are checked here (for the meters and the export: by their planners, reader_plan.h, which the run calls).
using br::Revision;
struct SpectrumInfo : th_spectrum_info {  // + the request's kind and the channel's resident rows
    uint32_t kind;
    const float *rows;
    size_t pitch;
};
int spectrum_request_info(th_tm *tm, const th_spectrum_request &r, size_t i, SpectrumInfo *info);
int spectra_run(th_tm *tm, size_t n, SpectrumInfo *info, float *out);
struct SpectrumReader : br::ReaderDefaults {
    using Request = th_spectrum_request;
    using Info = SpectrumInfo;
    using Public = th_spectrum_info;
    using Out = float;
    static constexpr const char *unit = "floats";
    static constexpr Revision revision = Revision::spectrogram;
    static constexpr bool needs_colormap = false, run_updates_infos = false;
    static size_t id_of(const Request &r) { return r.id; }
    static int check(th_tm *tm, const Request &r, size_t i, Info *info) { return spectrum_request_info(tm, r, i, info); }
    static int fit(const Info *, size_t n);  // one launch's job count
    static size_t layout(Info *info, size_t n);
    static int run(th_tm *tm, size_t n, Info *info, Out *out) { return spectra_run(tm, n, info, out); }
};

// *m: the oversampling and the two counts, everything else zero.  meters_run fills meters[i] in place (it keeps the oversampling,
// the counts, the offsets and the revision as the driver set them) and, with series, writes track i's LUFS to
// series + meters[i].momentary_offset (the short-term values follow the momentary ones, as the layout places them)
struct MeterInfo : th_loudness_meter {  // + the track's id, the track (a Track of track_manager.hip) and its channel count
    size_t id;
    const void *track;
    size_t n_channels;
};
int loudness_meter_info(th_tm *tm, size_t id, MeterInfo *m);
int meters_run(th_tm *tm, size_t n, MeterInfo *meters, double *series);
struct MeterReader : br::ReaderDefaults {
    using Request = size_t;
    using Info = MeterInfo;
    using Public = th_loudness_meter;
    using Out = double;
    static constexpr const char *unit = "doubles";
    static constexpr Revision revision = Revision::waveform;
    static constexpr bool needs_colormap = false, run_updates_infos = true, out_optional = true;
    static size_t id_of(const Request &id) { return id; }
    static int check(th_tm *tm, const Request &id, size_t, Info *m) { return loudness_meter_info(tm, id, m); }
    static int fit(const Info *m, size_t n);  // the limits of one launch (its grid: reader_plan.h)
    static size_t layout(Info *m, size_t n);
    static int run(th_tm *tm, size_t n, Info *m, Out *series) { return meters_run(tm, n, m, series); }
};

// Spectrogram tiles: what the run needs of one request (the request, the crop box, the image or mip level it is cut from; single: no
// such level is held, the request goes through the single-tile path) and where its record starts.  Records are 40-byte header + RGBA,
// padded to 64 bytes (tile_record_bytes); tiles_layout also writes the n + 1 offsets the ABI returns.  tiles_run writes headers and
// pixels, never the padding.  It needs the device colormap: ensure_colormap uploads the default one if none was set, taking the
// WRITE lock for that, so callers invoke it before they take the shared lock
struct TileInfo {
    TileGeom g;
    const uint16_t *src;
    uint32_t src_w, src_h, src_pitch;
    bool single;
    size_t offset;
    th_tile_request r;
};
inline size_t tile_record_bytes(const TileGeom &g) { return (40 + g.width * g.height * 4 + 63) / 64 * 64; }
int ensure_colormap(th_tm *tm);
int tile_request_info(th_tm *tm, const th_tile_request &r, TileInfo *info);
size_t tiles_layout(TileInfo *info, size_t n, size_t *offsets);
int tiles_run(th_tm *tm, size_t n, const TileInfo *info, uint8_t *out);

// Export.  Every request carries its output rate (sr_out 0: the track's own, which is all th_tm_export_pcm asks for) and its band
// (none: th_tm_export_pcm and _at; never both a band and another rate): export_requests makes them of each entry's own request type.
// info->sr is the rate the request comes out at, and a request whose info->sr is not the track's is resampled; one whose info->band has
// taps is filtered.
// layout: offsets that are multiples of 16, and in info[i].pad the zero bytes up to the next one (0 behind the last).
// export_run: request i's bytes, then info[i].pad zero bytes, and its two counts into info[i]
struct ExportReq {
    th_export_request base;
    uint32_t sr_out;  // 0 = the track's own
    bool has_band;    // mode, f_lo_hz, f_hi_hz, trans_hz: those of th_export_band_request
    uint32_t mode;
    double f_lo_hz, f_hi_hz, trans_hz;
};
struct ExportInfo : th_export_info {  // + the request, the track (a Track of track_manager.hip), its resampler, its filter, the zero bytes behind the request
    th_export_request req;
    const void *track;
    th_resample_plan plan;  // of (the track's rate, sr) when they differ, and the track's length at sr
    size_t n_out;
    th_band_plan band;      // half_taps == 0: no filter
    uint32_t pad;
    uint32_t flac_flags;    // the FLAC reader's: TH_FLAC_* of the call
};
int export_request_info(th_tm *tm, const ExportReq &r, size_t i, ExportInfo *info);
int export_run(th_tm *tm, size_t n, ExportInfo *info, uint8_t *out);
struct ExportReader : br::ReaderDefaults {
    using Request = ExportReq;
    using Info = ExportInfo;
    using Public = th_export_info;
    using Out = uint8_t;
    static constexpr const char *unit = "bytes";
    static constexpr Revision revision = Revision::waveform;
    static constexpr bool needs_colormap = false, run_updates_infos = true;
    static size_t id_of(const Request &r) { return r.base.id; }
    static int check(th_tm *tm, const Request &r, size_t i, Info *info) { return export_request_info(tm, r, i, info); }
    static size_t layout(Info *info, size_t n);
    static int run(th_tm *tm, size_t n, Info *info, Out *out) { return export_run(tm, n, info, out); }
};
inline ExportReq export_req(const th_export_request &r) { return ExportReq{r, 0u, false, 0u, 0.0, 0.0, 0.0}; }
inline ExportReq export_req(const th_export_at_request &r) { return ExportReq{r.base, r.sr_out, false, 0u, 0.0, 0.0, 0.0}; }
inline ExportReq export_req(const th_export_band_request &r) { return ExportReq{r.base, 0u, true, r.mode, r.f_lo_hz, r.f_hi_hz, r.trans_hz}; }
template <class R>
std::vector<ExportReq> export_requests(const R *reqs, size_t n) {
    std::vector<ExportReq> out(n);
    for (size_t i = 0; i < n; i++) out[i] = export_req(reqs[i]);
    return out;
}
// th_wav_header with the status reported (host_math.h wav_header)
int wav_header_checked(uint32_t format, uint32_t sr, uint32_t n_ch, uint64_t n_frames, uint8_t out[TH_WAV_HEADER_MAX], size_t *header_len,
                       size_t *pad_len);

// FLAC export.  check: the export's own for the same request (F32 refused where the format is checked), then the stream's limits;
// n_bytes = th_flac_bound.  layout: offsets that are multiples of 16, from the bounds; returns the last offset + the last bound.
// flac_run: request i's file image to out + info[i].offset, its actual length into info[i].n_bytes, its two counts into info[i].
// flac_out_len: what *out_len is after a successful call (the last request's offset + its actual length).
// The call's flags (th_tm_export_flac: 0) are checked where the format is.  They are the reader's template argument, so every entry
// hands the caller's requests to the driver as they are: FlacReaderOf<0 .. 3>, and FLAC_FLAGS_UNKNOWN for any other value
int flac_stream_checked(uint32_t sr, uint32_t n_ch, uint32_t format, uint64_t n_frames);
int flac_request_info(th_tm *tm, const th_export_request &r, uint32_t flags, size_t i, ExportInfo *info);
size_t flac_layout(ExportInfo *info, size_t n);
int flac_run(th_tm *tm, size_t n, ExportInfo *info, uint8_t *out);
constexpr uint32_t FLAC_FLAGS_UNKNOWN = ~0u;
template <uint32_t FLAGS>
struct FlacReaderOf : br::ReaderDefaults {
    using Request = th_export_request;
    using Info = ExportInfo;
    using Public = th_export_info;
    using Out = uint8_t;
    static constexpr const char *unit = "bytes";
    static constexpr Revision revision = Revision::waveform;
    static constexpr bool needs_colormap = false, run_updates_infos = true;
    static size_t id_of(const Request &r) { return r.id; }
    static int check(th_tm *tm, const Request &r, size_t i, Info *info) { return flac_request_info(tm, r, FLAGS, i, info); }
    static size_t layout(Info *info, size_t n) { return flac_layout(info, n); }
    static int run(th_tm *tm, size_t n, Info *info, Out *out) { return flac_run(tm, n, info, out); }
};
using FlacReader = FlacReaderOf<0u>;
inline void flac_out_len(int rc, const th_export_info *info, size_t n, size_t *out_len) {
    if (rc == TH_OK && n) *out_len = (size_t)(info[n - 1].offset + info[n - 1].n_bytes);
}
// the entry of either manager (m: its adaptor for batched_read)
template <class M>
int flac_read(M m, const th_export_request *reqs, size_t n, uint32_t flags, uint8_t *out, size_t cap, th_export_info *info, size_t *out_len) {
    int rc;
    switch (flags) {
        case 0u: rc = br::batched_read<FlacReaderOf<0u>>(m, reqs, n, out, cap, info, out_len); break;
        case 1u: rc = br::batched_read<FlacReaderOf<1u>>(m, reqs, n, out, cap, info, out_len); break;
        case 2u: rc = br::batched_read<FlacReaderOf<2u>>(m, reqs, n, out, cap, info, out_len); break;
        case 3u: rc = br::batched_read<FlacReaderOf<3u>>(m, reqs, n, out, cap, info, out_len); break;
        default: rc = br::batched_read<FlacReaderOf<FLAC_FLAGS_UNKNOWN>>(m, reqs, n, out, cap, info, out_len); break;
    }
    flac_out_len(rc, info, n, out_len);
    return rc;
}

// Figures.  *info: the record's size and what the plan needs of the request (the resident image; its offset is the layout's to set).
// layout: offsets that are multiples of 64; returns the last record's end.  figures_run: request i's record to
// out + info[i].offset, nothing between the records.  The device colormap must exist (ensure_colormap, before the shared lock)
struct FigureInfo : th_figure_info {
    FigurePlanRequest plan;
};
int figure_request_info(th_tm *tm, const th_figure_request &r, size_t i, FigureInfo *info);
int figures_run(th_tm *tm, size_t n, FigureInfo *info, uint8_t *out);
struct FigureReader : br::ReaderDefaults {
    using Request = th_figure_request;
    using Info = FigureInfo;
    using Public = th_figure_info;
    using Out = uint8_t;
    static constexpr const char *unit = "bytes";
    static constexpr Revision revision = Revision::spectrogram;
    static constexpr bool needs_colormap = true, run_updates_infos = false;
    static size_t id_of(const Request &r) { return r.id; }
    static int check(th_tm *tm, const Request &r, size_t i, Info *info) { return figure_request_info(tm, r, i, info); }
    static size_t layout(Info *info, size_t n) { return br::layout_aligned_64(info, n); }
    static int run(th_tm *tm, size_t n, Info *info, Out *out) { return figures_run(tm, n, info, out); }
};
// th_tm_figure_box without the lock
int figure_box_of(th_tm *tm, size_t id, uint32_t ch, double start_sec, double end_sec, double hz_min, double hz_max, double box[4]);

// Waveform envelopes and lanes.  *info: the record's size, edges[0] and edges[n_cols], and what the plan needs of the request (the
// resident channel `which` names; its offset is the layout's to set).  Envelopes: requests back to back, in floats; waveform
// figures: offsets that are multiples of 64, the last record's end.  *_run: request i's record to out + info[i].offset, nothing
// between the records
struct EnvelopeInfo : th_envelope_info {
    EnvelopePlanRequest plan;
};
int envelope_request_info(th_tm *tm, const th_envelope_request &r, size_t i, EnvelopeInfo *info);
int envelopes_run(th_tm *tm, size_t n, EnvelopeInfo *info, float *out);
struct EnvelopeReader : br::ReaderDefaults {
    using Request = th_envelope_request;
    using Info = EnvelopeInfo;
    using Public = th_envelope_info;
    using Out = float;
    static constexpr const char *unit = "floats";
    static constexpr Revision revision = Revision::waveform;
    static constexpr bool needs_colormap = false, run_updates_infos = false;
    static size_t id_of(const Request &r) { return r.id; }
    static int check(th_tm *tm, const Request &r, size_t i, Info *info) { return envelope_request_info(tm, r, i, info); }
    static size_t layout(Info *info, size_t n) { return br::layout_back_to_back(info, n, &Info::length); }
    static int run(th_tm *tm, size_t n, Info *info, Out *out) { return envelopes_run(tm, n, info, out); }
};
struct WaveformFigureInfo : th_waveform_figure_info {
    LanePlanRequest plan;
};
int waveform_figure_request_info(th_tm *tm, const th_waveform_figure_request &r, size_t i, WaveformFigureInfo *info);
int waveform_figures_run(th_tm *tm, size_t n, WaveformFigureInfo *info, uint8_t *out);
struct WaveformFigureReader : br::ReaderDefaults {
    using Request = th_waveform_figure_request;
    using Info = WaveformFigureInfo;
    using Public = th_waveform_figure_info;
    using Out = uint8_t;
    static constexpr const char *unit = "bytes";
    static constexpr Revision revision = Revision::waveform;
    static constexpr bool needs_colormap = false, run_updates_infos = false;
    static size_t id_of(const Request &r) { return r.env.id; }
    static int check(th_tm *tm, const Request &r, size_t i, Info *info) { return waveform_figure_request_info(tm, r, i, info); }
    static size_t layout(Info *info, size_t n) { return br::layout_aligned_64(info, n); }
    static int run(th_tm *tm, size_t n, Info *info, Out *out) { return waveform_figures_run(tm, n, info, out); }
};

// Formant candidates.  *info: the frames, the record's length and the request's plan with its resident channel (its offset is the
// layout's to set).  Requests back to back, in doubles.  formants_run: request i's doubles to out + info[i].offset and its two counts
// into info[i]
struct FormantInfo : th_formant_info {
    FormantPlanRequest plan;
};
int formant_request_info(th_tm *tm, const th_formant_request &r, size_t i, FormantInfo *info);
int formants_run(th_tm *tm, size_t n, FormantInfo *info, double *out);
struct FormantReader : br::ReaderDefaults {
    using Request = th_formant_request;
    using Info = FormantInfo;
    using Public = th_formant_info;
    using Out = double;
    static constexpr const char *unit = "doubles";
    static constexpr Revision revision = Revision::waveform;
    static constexpr bool needs_colormap = false, run_updates_infos = true;
    static size_t id_of(const Request &r) { return r.id; }
    static int check(th_tm *tm, const Request &r, size_t i, Info *info) { return formant_request_info(tm, r, i, info); }
    static size_t layout(Info *info, size_t n) { return br::layout_back_to_back(info, n, &Info::length); }
    static int run(th_tm *tm, size_t n, Info *info, Out *out) { return formants_run(tm, n, info, out); }
};

// Alignment of two tracks.  A request names two tracks; the probe's decides the owner, and the reference is looked for in the manager
// home_of(who, ref_id) returns (NULL: no manager holds it), or, with home_of == NULL, in the owner itself: th_tm passes none, th_tmg
// its own track table, so that check reports one request's faults in one order for both.  *info: the plan, the two resident channels
// and the reference's manager; where that is not the run's own manager the run stages the reference's range (it takes that manager's
// shared lock for the copy; the caller holds the lock that keeps writers out of both).  Requests back to back, in doubles.
// align_run: request i's doubles to out + info[i].offset
struct AlignReq {
    th_align_request r;
    th_tm *(*home_of)(void *who, size_t id);
    void *who;
};
struct AlignInfo : th_align_info {
    th_align_plan pl;
    const float *ref, *probe;  // the whole channels (ref: in ref_home's device memory)
    uint64_t n_probe;
    th_tm *ref_home;
};
int align_request_info(th_tm *tm, const AlignReq &r, size_t i, AlignInfo *info);
int align_run(th_tm *tm, size_t n, AlignInfo *info, double *out);
struct AlignReader : br::ReaderDefaults {
    using Request = AlignReq;
    using Info = AlignInfo;
    using Public = th_align_info;
    using Out = double;
    static constexpr const char *unit = "doubles";
    static constexpr Revision revision = Revision::waveform;
    static constexpr bool needs_colormap = false, run_updates_infos = false;
    static size_t id_of(const Request &r) { return r.r.id; }
    static int check(th_tm *tm, const Request &r, size_t i, Info *info) { return align_request_info(tm, r, i, info); }
    static size_t layout(Info *info, size_t n) {
        uint64_t at = 0;
        for (size_t i = 0; i < n; i++) {
            info[i].offset = at;
            at += info[i].length;
        }
        return (size_t)at;
    }
    static int run(th_tm *tm, size_t n, Info *info, Out *out) { return align_run(tm, n, info, out); }
};
inline std::vector<AlignReq> align_requests(const th_align_request *reqs, size_t n, th_tm *(*home_of)(void *, size_t), void *who) {
    std::vector<AlignReq> out(n);
    for (size_t i = 0; i < n; i++) out[i] = AlignReq{reqs[i], home_of, who};
    return out;
}

// update_spec_imgs against `global` (NULL: the manager's own tracks, as th_tm_* does), then the writer's final wait:
// for the images only (apply_track_list_changes, set_dB_range) or for everything (set_setting, set_colormap)
int requantise(th_tm *tm, const DbRange *global, bool force_update_all, bool images_only, std::vector<size_t> *updated);
// set_colormap without its image step: the LUT (kept when malformed, render_tiles.rs:80-85) and colormap_length
int set_colormap_only(th_tm *tm, const uint8_t *rgba, size_t bytes);
// the writer's final wait (the context stream idle, host copies of uploads released)
int settle(th_tm *tm);

}  // namespace tmi
}  // namespace th
