// reader_plan.cpp — the export and loudness-meter readers' host planning (reader_plan.h).  Plain C++: compiled into the library
// and, by g++, into the emulator library of tests/emu/.
#include "reader_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>

#include "export_core.h"  // export_bytes_per_sample
#include "plan_error.h"

namespace th {

namespace {
size_t up256(size_t x) { return (x + 255) / 256 * 256; }

template <class T>
void put(std::vector<unsigned char> &tab, size_t at, const std::vector<T> &v) {
    if (!v.empty()) std::memcpy(tab.data() + at, v.data(), v.size() * sizeof(T));
}

// The next span of a request, as it would lie in the open piece.
struct ExportSpan {
    bool fits = false;
    uint64_t take = 0;      // frames
    uint64_t out_at = 0;    // of its first byte in the caller's buffer
    size_t stage_at = 0;
    bool contiguous = false;  // with the piece's last run
    uint64_t hull0 = 0, stride = 0;
};

// Frames [f, ...) of request r, as many as the open piece `cur` takes (out_end: where the piece's last run ends in the caller's
// buffer).  !fits: the piece has to be closed first; an empty piece takes a span of every request unless its scratch alone exceeds
// the bound (take then says of how many frames).
ExportSpan next_span(const ExportPiece &cur, uint64_t out_end, const ExportPlanRequest &r, uint64_t f) {
    ExportSpan s;
    const bool resampled = r.sr_out != r.sr_in, filtered = r.band.half_taps != 0;
    if (resampled && cur.sr_out != 0 && (cur.sr_in != r.sr_in || cur.sr_out != r.sr_out)) return s;  // (one table per launch)
    if (filtered && cur.band.half_taps != 0 && (cur.band_sr != r.sr_in || !same_band(cur.band, r.band))) return s;  // (and one row)
    const uint64_t fbytes = (uint64_t)r.n_ch * export_bytes_per_sample(r.format);
    s.out_at = r.offset + (f - r.s0) * fbytes;
    s.contiguous = !cur.runs.empty() && s.out_at == out_end;
    s.stage_at = s.contiguous ? cur.stage_bytes : ((cur.stage_bytes + 15) & ~(size_t)15) + (size_t)(s.out_at & 15);
    const uint64_t room = s.stage_at < TH_EXPORT_PIECE_BYTES ? (TH_EXPORT_PIECE_BYTES - s.stage_at) / fbytes : 0;
    if (room == 0) return s;  // (a frame is at most 4 KiB: an empty piece always has room)
    s.take = std::min<uint64_t>(room, r.s1 - f);
    // a resampled or filtered request is cut on the export kernel's chunk grid, and its hull on the grid of 4 frames is what the
    // resampler or the band filter makes: the export kernel's 16-byte loads then stay aligned and inside what was written
    if (resampled || filtered) {
        if (f + s.take < r.s1) {
            const uint64_t F = export_chunk_frames(r.n_ch);
            const uint64_t cut = (f + s.take) / F * F;
            if (cut <= f) return s;  // (an empty piece has room for a whole chunk: at most 16 KiB)
            s.take = cut - f;
        }
        s.hull0 = f & ~(uint64_t)3;
        const uint64_t hull1 = std::min<uint64_t>((f + s.take + 3) & ~(uint64_t)3, resampled ? r.n_out : r.n_in);
        s.stride = (hull1 - s.hull0 + 3) & ~(uint64_t)3;
        if ((cur.scratch_floats + s.stride * r.n_ch) * sizeof(float) > RESAMPLE_SCRATCH_MAX) return s;
    }
    s.fits = true;
    return s;
}
}  // namespace

ExportPlan plan_export(const ExportPlanRequest *reqs, size_t n) {
    if (n > UINT32_MAX) return plan_error<ExportPlan>(TH_ERR_INVALID_ARG, "too many requests");
    ExportPlan p;
    p.ptr0.resize(n);
    p.req_ch.resize(n);
    ExportPiece cur;
    uint64_t out_end = 0;
    auto close_piece = [&]() {
        cur.job1 = p.jobs.size();
        cur.rjob1 = p.rjobs.size();
        cur.bjob1 = p.bjobs.size();
        p.pieces.push_back(std::move(cur));
        cur = ExportPiece{};
        cur.job0 = p.jobs.size();
        cur.rjob0 = p.rjobs.size();
        cur.bjob0 = p.bjobs.size();
    };
    for (size_t i = 0; i < n; i++) {
        const ExportPlanRequest &r = reqs[i];
        const bool resampled = r.sr_out != r.sr_in, filtered = r.band.half_taps != 0;
        if (resampled && filtered) return plan_error<ExportPlan>(TH_ERR_INTERNAL, "request %zu: a band and a rate conversion in one request", i);
        const ResampleTiling tiling = resampled ? resample_tiling(r.plan) : ResampleTiling{};
        const uint64_t fbytes = (uint64_t)r.n_ch * export_bytes_per_sample(r.format);
        p.ptr0[i] = p.n_ptrs;
        p.req_ch[i] = r.n_ch;
        p.n_ptrs += r.n_ch;
        for (uint64_t f = r.s0; f < r.s1;) {
            ExportSpan s = next_span(cur, out_end, r, f);
            if (!s.fits && p.jobs.size() != cur.job0) {
                close_piece();
                s = next_span(cur, out_end, r, f);
            }
            if (!s.fits)
                return plan_error<ExportPlan>(TH_ERR_INTERNAL, "request %zu: a piece of %llu frames exceeds the resampler's scratch", i,
                                              (unsigned long long)s.take);
            const uint32_t pd = f + s.take == r.s1 ? r.pad : 0u;
            const size_t bytes = (size_t)(s.take * fbytes) + pd;
            ExportJob j{};
            j.f0 = f;
            j.f1 = f + s.take;
            j.n = resampled ? r.n_out : r.n_in;
            j.n_ch = r.n_ch;
            j.format = r.format;
            j.dither = r.dither;
            j.seed = r.seed;
            j.first_chunk = cur.n_chunks;
            j.pad = pd;
            const uint64_t chunks = (uint64_t)cur.n_chunks + export_n_chunks(j.f0, j.f1, r.n_ch);
            if (chunks > INT32_MAX) return plan_error<ExportPlan>(TH_ERR_UNSUPPORTED, "request %zu: too many chunks in one piece", i);
            ExportPlace place{i, s.stage_at, 0, 0, s.hull0, s.stride, resampled, filtered};
            if (resampled) {
                ResampleJob rj{};
                rj.ja = s.hull0;
                rj.jb = std::min<uint64_t>(s.hull0 + s.stride, r.n_out);
                rj.n_in = r.n_in;
                rj.ch_stride = s.stride;
                rj.n_ch = r.n_ch;
                const uint64_t n_sb = resample_n_sb(rj.ja, rj.jb, tiling);
                const uint64_t blocks = (uint64_t)cur.n_rblocks + n_sb * r.n_ch * tiling.S;
                if (n_sb > UINT32_MAX || blocks > INT32_MAX)
                    return plan_error<ExportPlan>(TH_ERR_UNSUPPORTED, "request %zu: too many resampler tiles in one piece", i);
                rj.n_sb = (uint32_t)n_sb;
                rj.first_block = cur.n_rblocks;
                cur.n_rblocks = (uint32_t)blocks;
                place.scratch_at = cur.scratch_floats;
                place.ptr_at = p.n_ptrs;
                p.n_ptrs += r.n_ch;
                cur.scratch_floats += s.stride * r.n_ch;
                cur.sr_in = r.sr_in;
                cur.sr_out = r.sr_out;
                cur.plan = r.plan;
                p.rjobs.push_back(rj);
            }
            if (filtered) {
                BandJob bj{};
                bj.ja = s.hull0;
                bj.jb = std::min<uint64_t>(s.hull0 + s.stride, r.n_in);
                bj.n_in = r.n_in;
                bj.ch_stride = s.stride;
                bj.n_ch = r.n_ch;
                const uint64_t n_tiles = band_n_tiles(bj.ja, bj.jb);
                const uint64_t blocks = (uint64_t)cur.n_bblocks + n_tiles * r.n_ch;
                if (n_tiles > UINT32_MAX || blocks > INT32_MAX)
                    return plan_error<ExportPlan>(TH_ERR_UNSUPPORTED, "request %zu: too many filter tiles in one piece", i);
                bj.n_tiles = (uint32_t)n_tiles;
                bj.first_block = cur.n_bblocks;
                cur.n_bblocks = (uint32_t)blocks;
                place.scratch_at = cur.scratch_floats;
                place.ptr_at = p.n_ptrs;
                p.n_ptrs += r.n_ch;
                cur.scratch_floats += s.stride * r.n_ch;
                cur.band_sr = r.sr_in;
                cur.band = r.band;
                p.bjobs.push_back(bj);
            }
            cur.n_chunks = (uint32_t)chunks;
            p.jobs.push_back(j);
            p.places.push_back(place);
            if (s.contiguous)
                cur.runs.back().bytes += bytes;
            else
                cur.runs.push_back(ExportRun{s.stage_at, s.out_at, bytes});
            cur.stage_bytes = s.stage_at + bytes;
            out_end = s.out_at + bytes;
            f += s.take;
        }
    }
    if (cur.n_chunks) close_piece();
    for (size_t k = 0; k < p.pieces.size(); k++) {
        p.stage_need[k & 1] = std::max(p.stage_need[k & 1], p.pieces[k].stage_bytes);
        p.scratch_need = std::max(p.scratch_need, p.pieces[k].scratch_floats);
    }
    p.o_rjobs = p.jobs.size() * sizeof(ExportJob);
    p.o_bjobs = p.o_rjobs + p.rjobs.size() * sizeof(ResampleJob);
    p.o_ptrs = p.o_bjobs + p.bjobs.size() * sizeof(BandJob);
    p.tab_bytes = p.o_ptrs + p.n_ptrs * sizeof(const float *);
    return p;
}

std::vector<unsigned char> bind_export(ExportPlan &p, const ExportBases &b, const float *const *chan) {
    std::vector<const float *> ptrs(p.n_ptrs, nullptr);
    const float *const *d_ptrs = reinterpret_cast<const float *const *>(b.tab + p.o_ptrs);
    for (size_t i = 0; i < p.ptr0.size(); i++) {
        std::copy(chan, chan + p.req_ch[i], ptrs.begin() + p.ptr0[i]);
        chan += p.req_ch[i];
    }
    for (size_t k = 0; k < p.pieces.size(); k++) {
        size_t rj = p.pieces[k].rjob0, bj = p.pieces[k].bjob0;
        for (size_t j = p.pieces[k].job0; j < p.pieces[k].job1; j++) {
            const ExportPlace &pl = p.places[j];
            p.jobs[j].chan = d_ptrs + p.ptr0[pl.req];
            p.jobs[j].dst = b.stage[k & 1] + pl.stage_at;
            p.jobs[j].cnt = b.cnt + 2 * pl.req;
            if (!pl.resampled && !pl.filtered) continue;
            float *run = b.scratch + pl.scratch_at;
            for (uint32_t c = 0; c < p.jobs[j].n_ch; c++)
                ptrs[pl.ptr_at + c] = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(run + (size_t)c * pl.stride) -
                                                                      (uintptr_t)pl.hull0 * sizeof(float));
            p.jobs[j].chan = d_ptrs + pl.ptr_at;
            if (pl.resampled) {
                p.rjobs[rj].chan = d_ptrs + p.ptr0[pl.req];
                p.rjobs[rj].dst = run;
                rj++;
            } else {
                p.bjobs[bj].chan = d_ptrs + p.ptr0[pl.req];
                p.bjobs[bj].dst = run;
                bj++;
            }
        }
    }
    std::vector<unsigned char> tab(p.tab_bytes);
    put(tab, 0, p.jobs);
    put(tab, p.o_rjobs, p.rjobs);
    put(tab, p.o_bjobs, p.bjobs);
    put(tab, p.o_ptrs, ptrs);
    return tab;
}

const char *meter_limits_text(size_t n_tracks, size_t n_channels) {
    if (n_tracks > 65535) return "at most 65535 tracks per call";
    if (n_channels > 65535) return "at most 65535 channels per call";
    return nullptr;
}

MeterPlan plan_meters(const MeterPlanTrack *tracks, size_t n) {
    MeterPlan p;
    for (size_t i = 0; i < n; i++) p.n_ch += tracks[i].n_ch;
    if (const char *text = meter_limits_text(n, p.n_ch)) return plan_error<MeterPlan>(TH_ERR_INVALID_ARG, "%s", text);
    p.tracks.assign(tracks, tracks + n);
    p.rate_ok.resize(n);
    p.tj_m.resize(n);
    p.tj_s.resize(n);
    p.ch0.resize(n);
    p.e0.resize(n);
    for (size_t i = 0; i < n; i++) {
        const MeterPlanTrack &tr = tracks[i];
        const bool ok = p.rate_ok[i] = loudness_rate_ok(tr.sr);
        const LoudnessRate &R = loudness_rate(ok ? tr.sr : 48000);  // (a refused rate: the peaks only, over chunks of a 48 kHz geometry)
        size_t ri = 0;
        while (ri < p.rates.size() && p.rates[ri] != &R) ri++;
        if (ri == p.rates.size()) p.rates.push_back(&R);
        const uint64_t ns = tr.n_samples;
        const uint64_t nseg_any = (ns + R.s100 - 1) / R.s100, nseg = ns / R.s100;
        if (!(ns < (1ull << 40) && nseg_any * R.n_sub < (1ull << 31)))
            return plan_error<MeterPlan>(TH_ERR_INVALID_ARG, "track %zu: too many samples", tr.id);
        const uint32_t nf = ok && nseg >= 4 ? (uint32_t)(nseg * R.n_sub) : 0u;
        p.ch0[i] = p.jobs.size();
        p.e0[i] = p.n_energies;
        p.n_energies += tr.n_momentary + tr.n_short_term;
        for (uint32_t k = 0; k < tr.n_ch; k++) {
            LoudJob j{};
            j.n = ns;
            j.rate = (uint32_t)ri;
            j.n_chunks = (uint32_t)(nseg_any * R.n_sub);
            j.n_fchunks = nf;
            if (tr.oversampling > 1 && ns) {
                const int f = tr.oversampling == 4 ? 0 : 1;
                TruePeakJob t{};
                t.n = ns;
                t.n_chunks = (uint32_t)((ns + TP_CHUNK - 1) / TP_CHUNK);
                p.tp[f].push_back(t);
                p.tp_ch[f].push_back(p.jobs.size());
                p.tp_chunks[f] = std::max(p.tp_chunks[f], t.n_chunks);
            }
            p.jobs.push_back(j);
            p.n_states += nf;
        }
        for (int v = 0; v < 2; v++) {
            LoudTrackJob &t = v ? p.tj_s[i] : p.tj_m[i];
            t = LoudTrackJob{};
            t.n_blocks = v ? tr.n_short_term : tr.n_momentary;
            for (uint32_t k = 0; k < 8; k++) t.w[k] = loudness_channel_weight(k, tr.n_ch);
            t.n_ch = tr.n_ch;
            t.n_sub = R.n_sub;
            t.n_fchunks = nf;
            t.L = (v ? 30u : 4u) * R.s100;
        }
        p.max_chunks = std::max(p.max_chunks, (uint32_t)(nseg_any * R.n_sub));
        p.max_fchunks = std::max(p.max_fchunks, nf);
        p.max_m = std::max<uint64_t>(p.max_m, tr.n_momentary);
        p.max_s = std::max<uint64_t>(p.max_s, tr.n_short_term);
        p.lds_floats = std::max(p.lds_floats, R.cl + 4);
    }
    const size_t pk_bytes = (p.n_ch * 4 + 7) / 8 * 8;
    p.o_sums = p.n_energies * 8;
    p.o_pka = p.o_sums + p.n_ch * 8;
    p.o_pkt = p.o_pka + pk_bytes;
    p.res_bytes = p.o_pkt + pk_bytes;
    p.o_z = up256(p.res_bytes);
    p.o_q = p.o_z + p.n_states * 64;
    p.mem_bytes = p.o_q + p.n_states * 8 + 8;
    p.t_rates = up256(p.jobs.size() * sizeof(LoudJob));
    p.t_m = p.t_rates + up256(p.rates.size() * sizeof(LoudnessRate));
    p.t_s = p.t_m + up256(n * sizeof(LoudTrackJob));
    p.t_tp4 = p.t_s + up256(n * sizeof(LoudTrackJob));
    p.t_tp2 = p.t_tp4 + up256(p.tp[0].size() * sizeof(TruePeakJob));
    p.tab_bytes = p.t_tp2 + up256(p.tp[1].size() * sizeof(TruePeakJob));
    return p;
}

std::vector<unsigned char> bind_meters(MeterPlan &p, unsigned char *mem, const float *const *wav) {
    double *d_res = reinterpret_cast<double *>(mem), *d_sums = reinterpret_cast<double *>(mem + p.o_sums);
    uint32_t *d_pka = reinterpret_cast<uint32_t *>(mem + p.o_pka), *d_pkt = reinterpret_cast<uint32_t *>(mem + p.o_pkt);
    double *d_z = reinterpret_cast<double *>(mem + p.o_z), *d_q = reinterpret_cast<double *>(mem + p.o_q);
    size_t si = 0;
    for (size_t i = 0; i < p.tracks.size(); i++) {
        const size_t q0 = si;
        for (size_t c = p.ch0[i]; c < p.ch0[i] + p.tracks[i].n_ch; c++) {
            LoudJob &j = p.jobs[c];
            j.wav = wav[c];
            j.aligned16 = (reinterpret_cast<uintptr_t>(wav[c]) & 15u) == 0;
            j.z = d_z + 8 * si;
            j.q = d_q + si;
            j.sumsq = d_sums + c;
            j.peak = d_pka + c;
            si += j.n_fchunks;
        }
        p.tj_m[i].q = p.tj_s[i].q = d_q + q0;
        p.tj_m[i].out = d_res + p.e0[i];
        p.tj_s[i].out = d_res + p.e0[i] + p.tracks[i].n_momentary;
    }
    for (int f = 0; f < 2; f++)
        for (size_t k = 0; k < p.tp[f].size(); k++) {
            const size_t c = p.tp_ch[f][k];
            p.tp[f][k].wav = wav[c];
            p.tp[f][k].aligned16 = p.jobs[c].aligned16;
            p.tp[f][k].peak = d_pkt + c;
        }
    std::vector<unsigned char> tab(p.tab_bytes, 0);
    put(tab, 0, p.jobs);
    for (size_t r = 0; r < p.rates.size(); r++) std::memcpy(tab.data() + p.t_rates + r * sizeof(LoudnessRate), p.rates[r], sizeof(LoudnessRate));
    put(tab, p.t_m, p.tj_m);
    put(tab, p.t_s, p.tj_s);
    put(tab, p.t_tp4, p.tp[0]);
    put(tab, p.t_tp2, p.tp[1]);
    return tab;
}

void meter_results(const unsigned char *res, const MeterPlan &p, th_loudness_meter *const *ms, double *series) {
    const double *energies = reinterpret_cast<const double *>(res);
    std::vector<double> lufs, sub;
    for (size_t i = 0; i < p.tracks.size(); i++) {
        th_loudness_meter &m = *ms[i];
        if (p.rate_ok[i]) {
            lufs.resize(m.n_momentary + m.n_short_term);
            const double *e = energies + p.e0[i];
            for (size_t k = 0; k < lufs.size(); k++) lufs[k] = loudness_lufs(e[k]);
            if (series && !lufs.empty()) std::memcpy(series + m.momentary_offset, lufs.data(), lufs.size() * sizeof(double));
            m.max_momentary_lufs = loudness_series_max(lufs.data(), m.n_momentary);
            m.max_short_term_lufs = loudness_series_max(lufs.data() + m.n_momentary, m.n_short_term);
            sub.clear();
            for (size_t k = 0; k < m.n_short_term; k += 10) sub.push_back(e[m.n_momentary + k]);
            m.loudness_range = loudness_range(sub.data(), sub.size());
        } else {
            m.loudness_range = m.max_momentary_lufs = m.max_short_term_lufs = NAN;
        }
        const uint32_t *pk = reinterpret_cast<const uint32_t *>(res + (m.oversampling > 1 ? p.o_pkt : p.o_pka));
        float peak = 0.0f;
        uint32_t at = 0;
        for (uint32_t k = 0; k < p.tracks[i].n_ch; k++) {
            float v;
            std::memcpy(&v, &pk[p.ch0[i] + k], 4);
            if (v > peak) {
                peak = v;
                at = k;
            }
        }
        m.true_peak = peak;
        m.true_peak_dB = peak == 0.0f ? -INFINITY : (float)(20.0 * std::log10((double)peak));
        m.true_peak_channel = at;
    }
}

}  // namespace th
