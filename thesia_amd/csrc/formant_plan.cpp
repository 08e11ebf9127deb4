// formant_plan.cpp — the host side of the formant reader (formant_plan.h): the plan of a request, the tables, the cut of a call into
// pieces, step 6, and the host entries th_formant_* / th_formants_f64, which run the kernel's phase functions (formant_block.h) a
// thread after the other.  No HIP.  -ffp-contract=off, as every unit that includes formant_core.h.
#include "formant_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <utility>

#include "common.h"
#include "formant_block.h"
#include "host_math.h"
#include "plan_error.h"

namespace th {

int formant_plan_for(uint32_t sr, size_t n_samples, const th_formant_request &req, th_formant_plan *plan) {
    th_formant_plan pl{};
    if (sr == 0) return 1;
    if (req.which > 2 || req.window > TH_FORMANT_WIN_RECT || req.kind > TH_FORMANT_OUT_LPC) return 1;
    const uint32_t p = req.n_poles;
    if (p < 2 || p > TH_FORMANT_MAX_POLES || (p & 1u)) return 1;
    if (std::isnan(req.start_sec) || std::isnan(req.end_sec) || std::isnan(req.preemph_hz)) return 1;
    if (!std::isfinite(req.win_sec) || !std::isfinite(req.step_sec) || !(req.win_sec > 0.0) || !(req.step_sec >= 0.0)) return 1;
    if (!(req.preemph_hz >= 0.0)) return 1;
    const uint32_t sr_a = req.sr_analysis ? req.sr_analysis : sr;
    const double w = std::rint(req.win_sec * (double)sr_a), h = std::max(1.0, std::rint(req.step_sec * (double)sr_a));
    if (!(w >= (double)(p + 2)) || !(w <= (double)TH_FORMANT_MAX_WIN) || !(h <= (double)TH_FORMANT_MAX_HOP)) return 1;
    pl.sr = sr;
    pl.sr_analysis = sr_a;
    pl.n_poles = p;
    pl.win = (uint32_t)w;
    pl.hop = (uint32_t)h;
    pl.window = req.window;
    pl.kind = req.kind;
    pl.alpha = std::isinf(req.preemph_hz) ? 0.0 : std::exp(-2.0 * M_PI * req.preemph_hz / (double)sr_a);
    size_t n_a = n_samples;
    if (sr_a != sr) {
        if (resample_plan(sr, sr_a, &pl.rs) != 0 || !resample_n_out(n_samples, pl.rs, &n_a)) return 2;
        pl.resampled = 1;
    }
    pl.n_analysis = n_a;
    pl.n_frames_total = ((uint64_t)n_a + pl.hop - 1) / pl.hop;
    size_t s0 = 0, s1 = 0;
    if (!spectrum_frame_range(sr_a, 1, n_a, req.start_sec, req.end_sec, &s0, &s1)) return 1;
    pl.frame_first = ((uint64_t)s0 + pl.hop - 1) / pl.hop;
    pl.frame_end = ((uint64_t)s1 + pl.hop - 1) / pl.hop;
    *plan = pl;
    return 0;
}

void formant_window(uint32_t window, uint32_t W, double *g) {
    const double c = 0.5 * ((double)W - 1.0), d = ((double)W + 1.0) * ((double)W + 1.0), e12 = std::exp(-12.0);
    for (uint32_t k = 0; k < W; k++) {
        const double x = (double)k - c;
        g[k] = window == TH_FORMANT_WIN_RECT ? 1.0 : (std::exp(-48.0 * x * x / d) - e12) / (1.0 - e12);
    }
}

void formant_start_points(uint32_t p, double *z) {
    for (uint32_t i = 0; i < p; i++) {
        const double t = 2.0 * M_PI * ((double)i + 0.25) / (double)p;
        z[i] = 0.9 * std::cos(t);
        z[p + i] = 0.9 * std::sin(t);
    }
}

void formant_hull(const th_formant_plan &pl, uint64_t f0, uint64_t f1, uint64_t *h0, uint64_t *h1) {
    *h0 = *h1 = 0;
    if (f1 <= f0) return;
    const int64_t first = (int64_t)(f0 * pl.hop) - (int64_t)(pl.win / 2) - 1;
    const uint64_t end = (f1 - 1) * pl.hop - pl.win / 2 + pl.win;  // (W - floor(W / 2) >= 1: no wrap)
    *h0 = first > 0 ? (uint64_t)first : 0;
    *h1 = std::min<uint64_t>(end, pl.n_analysis);
    if (*h1 < *h0) *h1 = *h0;
}

void formant_pack(const double *rec, const th_formant_plan &pl, double *out, uint64_t *counts) {
    const uint32_t p = pl.n_poles;
    const double nan = std::nan("");
    const int status = (int)rec[0];
    if (status != 0) {
        for (uint32_t i = 0; i < 2 + p; i++) out[i] = nan;
        if (counts) {
            counts[0]++;
            if (status == 2) counts[1]++;
        }
        return;
    }
    if (pl.kind == TH_FORMANT_OUT_LPC) {
        out[0] = rec[2];
        out[1] = rec[3];
        for (uint32_t i = 0; i < p; i++) out[2 + i] = rec[4 + i];
        return;
    }
    const double sr_a = (double)pl.sr_analysis, lo = 50.0, hi = sr_a / 2.0 - 50.0;
    std::pair<double, double> found[TH_FORMANT_MAX_POLES];
    uint32_t n = 0;
    for (uint32_t i = 0; i < p; i++) {
        const double re = rec[4 + p + i], im = rec[4 + 2 * p + i];
        if (!(im > 0.0)) continue;
        const double f = std::atan2(im, re) * sr_a / (2.0 * M_PI);
        const double bw = -std::log(re * re + im * im) * sr_a / (2.0 * M_PI);
        if (f >= lo && f <= hi) found[n++] = {f, bw};
    }
    std::sort(found, found + n);
    n = std::min(n, p / 2);
    out[0] = (double)n;
    out[1] = rec[3] / rec[2];
    for (uint32_t i = 0; i < p / 2; i++) {
        out[2 + i] = i < n ? found[i].first : nan;
        out[2 + p / 2 + i] = i < n ? found[i].second : nan;
    }
}

void formant_frame_host(const float *u, const th_formant_plan &pl, const double *win, const double *start, uint64_t f, double *rec, double *r) {
    FormantJob job{};
    job.u = u;
    job.rec = rec;
    job.win = win;
    job.start = start;
    job.n_a = pl.n_analysis;
    job.f0 = f;
    job.alpha = pl.alpha;
    job.n_frames = 1;
    job.W = pl.win;
    job.H = pl.hop;
    job.p = pl.n_poles;
    job.kind = pl.kind;
    std::vector<double> lds(formant_lds_doubles(job.W, job.p));
    const FormantLds l = formant_carve(lds.data(), job.W, job.p);
    formant_block_serial<TH_FORMANT_MAX_POLES + 1>(job, 0, l);
    if (r) std::copy(l.r, l.r + job.p + 1, r);
}

FormantPlan plan_formants(const FormantPlanRequest *reqs, size_t n) {
    FormantPlan p;
    p.tabs.resize(n);
    std::map<std::pair<uint32_t, uint32_t>, size_t> wins;  // (window, W) -> where
    std::map<uint32_t, size_t> starts;
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const th_formant_plan &pl = reqs[i].pl;
        auto w = wins.find({pl.window, pl.win});
        if (w == wins.end()) {
            w = wins.emplace(std::make_pair(pl.window, pl.win), at).first;
            at += (size_t)pl.win * sizeof(double);
        }
        auto s = starts.find(pl.n_poles);
        if (s == starts.end()) {
            s = starts.emplace(pl.n_poles, at).first;
            at += 2 * (size_t)pl.n_poles * sizeof(double);
        }
        p.tabs[i] = FormantTab{w->second, s->second};
    }
    FormantPiece cur;
    auto close = [&]() {
        if (cur.run1 == cur.run0) return;
        cur.rjob1 = p.rjobs.size();
        p.rec_need = std::max(p.rec_need, cur.rec_doubles);
        p.scratch_need = std::max(p.scratch_need, cur.scratch_floats);
        p.pieces.push_back(cur);
        FormantPiece next;
        next.run0 = next.run1 = cur.run1;
        next.rjob0 = next.rjob1 = p.rjobs.size();
        cur = next;
    };
    for (size_t i = 0; i < n; i++) {
        const th_formant_plan &pl = reqs[i].pl;
        const uint32_t stride = formant_rec_doubles(pl.n_poles);
        const ResampleTiling tiling = pl.resampled ? resample_tiling(pl.rs) : ResampleTiling{};
        for (uint64_t f = pl.frame_first; f < pl.frame_end;) {
            if (pl.resampled && cur.sr_out != 0 && (cur.sr_in != pl.sr || cur.sr_out != pl.sr_analysis)) close();  // (one table per launch)
            uint64_t take = std::min<uint64_t>(pl.frame_end - f, TH_FORMANT_PIECE_FRAMES - cur.n_blocks);
            if (pl.resampled) {  // the run's hull is at most (take - 1) H + W + 1 samples
                const uint64_t room = TH_FORMANT_PIECE_SAMPLES - cur.scratch_floats, one = (uint64_t)pl.win + 1;
                take = room < one ? 0 : std::min<uint64_t>(take, (room - one) / pl.hop + 1);
            }
            if (take == 0) {
                close();
                continue;  // (an empty piece takes at least one frame: TH_FORMANT_PIECE_SAMPLES > TH_FORMANT_MAX_WIN + 1)
            }
            FormantRun run{};
            run.req = i;
            run.f0 = f;
            run.n_frames = (uint32_t)take;
            run.rec_at = cur.rec_doubles;
            run.rjob = -1;
            formant_hull(pl, f, f + take, &run.hull0, &run.hull1);
            FormantJob job{};
            job.n_a = pl.n_analysis;
            job.f0 = f;
            job.alpha = pl.alpha;
            job.n_frames = run.n_frames;
            job.first_block = cur.n_blocks;
            job.W = pl.win;
            job.H = pl.hop;
            job.p = pl.n_poles;
            job.kind = pl.kind;
            if (pl.resampled) {
                ResampleJob rj{};
                rj.ja = run.hull0;
                rj.jb = run.hull1;
                rj.n_in = reqs[i].n_in;
                rj.ch_stride = run.hull1 - run.hull0;
                rj.n_ch = 1;
                const uint64_t n_sb = resample_n_sb(rj.ja, rj.jb, tiling);
                const uint64_t blocks = (uint64_t)cur.n_rblocks + n_sb * tiling.S;
                if (n_sb > UINT32_MAX || blocks > INT32_MAX)
                    return plan_error<FormantPlan>(TH_ERR_UNSUPPORTED, "request %zu: too many resampler tiles in one piece", i);
                rj.n_sb = (uint32_t)n_sb;
                rj.first_block = cur.n_rblocks;
                cur.n_rblocks = (uint32_t)blocks;
                run.scratch_at = cur.scratch_floats;
                run.rjob = (int32_t)p.rjobs.size();
                cur.scratch_floats += (rj.ch_stride + 3) & ~(uint64_t)3;
                cur.sr_in = pl.sr;
                cur.sr_out = pl.sr_analysis;
                cur.rs = pl.rs;
                p.rjobs.push_back(rj);
            }
            cur.n_blocks += run.n_frames;
            cur.rec_doubles += (uint64_t)run.n_frames * stride;
            cur.max_p = std::max(cur.max_p, pl.n_poles);
            cur.max_W = std::max(cur.max_W, pl.win);
            cur.run1++;
            p.runs.push_back(run);
            p.jobs.push_back(job);
            f += take;
            if (cur.n_blocks == TH_FORMANT_PIECE_FRAMES) close();
        }
    }
    close();
    p.o_jobs = (at + 15) & ~(size_t)15;
    p.o_rjobs = p.o_jobs + p.jobs.size() * sizeof(FormantJob);
    p.o_ptrs = p.o_rjobs + p.rjobs.size() * sizeof(ResampleJob);
    p.tab_bytes = p.o_ptrs + n * sizeof(const float *);
    return p;
}

std::vector<unsigned char> bind_formants(FormantPlan &p, const FormantBases &b, const FormantPlanRequest *reqs, size_t n) {
    std::vector<unsigned char> tab(p.tab_bytes);
    std::vector<const float *> ptrs(n);
    for (size_t i = 0; i < n; i++) {
        ptrs[i] = reqs[i].src;
        const th_formant_plan &pl = reqs[i].pl;
        // (a table shared by several requests is written once per request that names it: the same bytes)
        formant_window(pl.window, pl.win, reinterpret_cast<double *>(tab.data() + p.tabs[i].win_at));
        formant_start_points(pl.n_poles, reinterpret_cast<double *>(tab.data() + p.tabs[i].start_at));
    }
    const float *const *d_ptrs = reinterpret_cast<const float *const *>(b.tab + p.o_ptrs);
    for (size_t k = 0; k < p.pieces.size(); k++) {
        for (size_t j = p.pieces[k].run0; j < p.pieces[k].run1; j++) {
            const FormantRun &run = p.runs[j];
            FormantJob &job = p.jobs[j];
            job.rec = b.rec[k & 1] + run.rec_at;
            job.win = reinterpret_cast<const double *>(b.tab + p.tabs[run.req].win_at);
            job.start = reinterpret_cast<const double *>(b.tab + p.tabs[run.req].start_at);
            job.u = reqs[run.req].src;
            if (run.rjob >= 0) {  // analysis sample n of the run is scratch[scratch_at + n - hull0]
                float *dst = b.scratch + run.scratch_at;
                job.u = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(dst) - (uintptr_t)run.hull0 * sizeof(float));
                p.rjobs[run.rjob].chan = d_ptrs + run.req;
                p.rjobs[run.rjob].dst = dst;
            }
        }
    }
    if (!p.jobs.empty()) std::memcpy(tab.data() + p.o_jobs, p.jobs.data(), p.jobs.size() * sizeof(FormantJob));
    if (!p.rjobs.empty()) std::memcpy(tab.data() + p.o_rjobs, p.rjobs.data(), p.rjobs.size() * sizeof(ResampleJob));
    if (n) std::memcpy(tab.data() + p.o_ptrs, ptrs.data(), n * sizeof(const float *));
    return tab;
}

}  // namespace th

using namespace th;

namespace {
int plan_checked(uint32_t sr, size_t n, const th_formant_request *req, th_formant_plan *pl) {
    const int rc = formant_plan_for(sr, n, *req, pl);
    TH_REQUIRE(rc != 1,
               "bad formant request: [%g, %g) s of %zu samples at %u Hz, analysis at %u Hz, %u poles (even, 2 .. %u), window %g s (%u .. %u "
               "samples), step %g s (at most %u samples), pre-emphasis from %g Hz, window %u, kind %u, which %u",
               req->start_sec, req->end_sec, n, sr, req->sr_analysis, req->n_poles, TH_FORMANT_MAX_POLES, req->win_sec, req->n_poles + 2,
               TH_FORMANT_MAX_WIN, req->step_sec, TH_FORMANT_MAX_HOP, req->preemph_hz, req->window, req->kind, req->which);
    if (rc != 0)
        return fail(TH_ERR_UNSUPPORTED, "%u -> %u Hz is beyond the resampler's limits (%u taps, %u coefficients, 64-bit indices)", sr,
                    req->sr_analysis, TH_RESAMPLE_MAX_TAPS, TH_RESAMPLE_MAX_COEFS);
    return TH_OK;
}

// the analysis signal that frames [f0, f1) read, as FormantJob::u: the channel itself, or the resampler's output over the hull in *keep
int analysis_signal(const float *x, size_t n, const th_formant_plan &pl, uint64_t f0, uint64_t f1, std::vector<float> *keep, const float **u) {
    *u = x;
    if (!pl.resampled) return TH_OK;
    uint64_t h0, h1;
    formant_hull(pl, f0, f1, &h0, &h1);
    keep->assign((size_t)(h1 - h0) + 1, 0.0f);
    TH_CHECK(th_resample_f32(x, n, pl.sr, pl.sr_analysis, h0, (size_t)(h1 - h0), keep->data()));
    *u = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(keep->data()) - (uintptr_t)h0 * sizeof(float));
    return TH_OK;
}
}  // namespace

TH_API int th_formant_defaults(th_formant_request *req) {
    TH_TRY
    TH_REQUIRE(req, "NULL argument");
    *req = th_formant_request{};
    req->start_sec = 0.0;
    req->end_sec = INFINITY;
    req->sr_analysis = 11000;
    req->n_poles = 10;
    req->win_sec = 0.05;
    req->step_sec = 0.0125;
    req->preemph_hz = 50.0;
    req->window = TH_FORMANT_WIN_GAUSS;
    req->kind = TH_FORMANT_OUT_FORMANTS;
    return TH_OK;
    TH_CATCH
}

TH_API int th_formant_plan_for(uint32_t sr, size_t n_samples, const th_formant_request *req, th_formant_plan *plan) {
    TH_TRY
    TH_REQUIRE(req && plan, "NULL argument");
    return plan_checked(sr, n_samples, req, plan);
    TH_CATCH
}

TH_API int th_formant_window(uint32_t window, uint32_t win, double *g) {
    TH_TRY
    TH_REQUIRE(g, "NULL argument");
    TH_REQUIRE(window <= TH_FORMANT_WIN_RECT && win >= 1 && win <= TH_FORMANT_MAX_WIN, "window %u of %u samples (1 .. %u)", window, win,
               TH_FORMANT_MAX_WIN);
    formant_window(window, win, g);
    return TH_OK;
    TH_CATCH
}

TH_API int th_formant_start_points(uint32_t n_poles, double *z) {
    TH_TRY
    TH_REQUIRE(z, "NULL argument");
    TH_REQUIRE(n_poles >= 1 && n_poles <= TH_FORMANT_MAX_POLES, "%u poles (1 .. %u)", n_poles, TH_FORMANT_MAX_POLES);
    formant_start_points(n_poles, z);
    return TH_OK;
    TH_CATCH
}

TH_API int th_formants_f64(const float *x, size_t n, uint32_t sr, const th_formant_request *req, uint64_t frame0, size_t n_frames, double *out,
                           uint64_t *counts) {
    TH_TRY
    TH_REQUIRE(req && (n == 0 || x) && (n_frames == 0 || out), "NULL argument");
    th_formant_plan pl;
    TH_CHECK(plan_checked(sr, n, req, &pl));
    TH_REQUIRE(frame0 <= pl.n_frames_total && n_frames <= pl.n_frames_total - frame0, "frames [%llu, +%zu) of %llu",
               (unsigned long long)frame0, n_frames, (unsigned long long)pl.n_frames_total);
    uint64_t cnt[2] = {0, 0};
    std::vector<float> keep;
    const float *u = nullptr;
    TH_CHECK(analysis_signal(x, n, pl, frame0, frame0 + n_frames, &keep, &u));
    std::vector<double> win(pl.win), start(2 * pl.n_poles), rec(formant_rec_doubles(pl.n_poles));
    formant_window(pl.window, pl.win, win.data());
    formant_start_points(pl.n_poles, start.data());
    for (size_t i = 0; i < n_frames; i++) {
        formant_frame_host(u, pl, win.data(), start.data(), frame0 + i, rec.data(), nullptr);
        formant_pack(rec.data(), pl, out + i * (2 + pl.n_poles), cnt);
    }
    if (counts) {
        counts[0] = cnt[0];
        counts[1] = cnt[1];
    }
    return TH_OK;
    TH_CATCH
}

TH_API int th_formant_frame_f64(const float *x, size_t n, uint32_t sr, const th_formant_request *req, uint64_t frame, double *r, double *a,
                                double *r0e, double *roots, uint32_t *sweeps, uint32_t *status) {
    TH_TRY
    TH_REQUIRE(req && (n == 0 || x) && r && a && r0e && roots && sweeps && status, "NULL argument");
    th_formant_plan pl;
    TH_CHECK(plan_checked(sr, n, req, &pl));
    TH_REQUIRE(frame < pl.n_frames_total, "frame %llu of %llu", (unsigned long long)frame, (unsigned long long)pl.n_frames_total);
    pl.kind = TH_FORMANT_OUT_FORMANTS;  // (step 5 runs for either kind)
    std::vector<float> keep;
    const float *u = nullptr;
    TH_CHECK(analysis_signal(x, n, pl, frame, frame + 1, &keep, &u));
    const uint32_t p = pl.n_poles;
    std::vector<double> win(pl.win), start(2 * p), rec(formant_rec_doubles(p));
    formant_window(pl.window, pl.win, win.data());
    formant_start_points(p, start.data());
    formant_frame_host(u, pl, win.data(), start.data(), frame, rec.data(), r);
    *status = (uint32_t)rec[0];
    *sweeps = (uint32_t)rec[1];
    r0e[0] = rec[2];
    r0e[1] = rec[3];
    a[0] = 1.0;
    std::copy(rec.begin() + 4, rec.begin() + 4 + p, a + 1);
    std::copy(rec.begin() + 4 + p, rec.begin() + 4 + 3 * p, roots);
    return TH_OK;
    TH_CATCH
}
