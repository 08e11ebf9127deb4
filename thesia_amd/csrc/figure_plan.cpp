// figure_plan.cpp — the host plan of th_tm_render_figures (figure_plan.h)
#include "figure_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "plan_error.h"

namespace th {

namespace {
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the Slaney mel scale of host_math.cpp mel_from_hz, in double
double mel_from_hz_f64(double hz) {
    if (hz < 1000.0) return hz / (200.0 / 3.0);
    return 15.0 + std::log(hz / 1000.0) / 0.06875177742094912;
}
}  // namespace

int figure_box(double start_sec, double end_sec, double hz_min, double hz_max, uint32_t sr, size_t n_samples, size_t img_w, size_t spec_h,
               size_t img_h, int freq_scale, double box[4]) {
    if (std::isnan(start_sec) || std::isnan(end_sec) || std::isnan(hz_min) || std::isnan(hz_max)) return 1;
    if (start_sec < 0.0 || std::isinf(start_sec) || hz_min < 0.0 || std::isinf(hz_min)) return 1;
    if (sr == 0 || n_samples == 0 || img_w == 0 || spec_h == 0 || img_h == 0) return 1;
    if (freq_scale != TH_FREQ_LINEAR && freq_scale != TH_FREQ_MEL) return 1;
    const double W = (double)img_w, Hs = (double)spec_h, Hi = (double)img_h, half = (double)sr / 2.0;
    auto x_of = [&](double sec) { return sec * (double)sr / (double)n_samples * W; };
    auto y_of = [&](double hz) { return (freq_scale == TH_FREQ_MEL ? mel_from_hz_f64(hz) / mel_from_hz_f64(half) : hz / half) * Hs; };
    auto clamp = [](double v, double hi) { return v < 0.0 ? 0.0 : (v > hi ? hi : v); };
    const double x0 = clamp(x_of(start_sec), W), x1 = end_sec == INFINITY ? W : clamp(x_of(end_sec), W);
    const double y0 = clamp(y_of(hz_min), Hi), y1 = hz_max == INFINITY ? Hi : clamp(y_of(hz_max), Hi);
    if (!(x1 > x0) || !(y1 > y0)) return 1;
    box[0] = x0;
    box[1] = y0;
    box[2] = x1 - x0;
    box[3] = y1 - y0;
    return 0;
}

FigureStatus check_figure(const FigurePlanRequest &r, size_t i) {
    using S = FigureStatus;
    if (r.kind > TH_FIGURE_GREY16) return plan_error<S>(TH_ERR_INVALID_ARG, "request %zu: unknown figure kind %u", i, r.kind);
    if (r.out_w == 0 || r.out_h == 0 || r.out_w > TH_FIGURE_MAX_DIM || r.out_h > TH_FIGURE_MAX_DIM)
        return plan_error<S>(TH_ERR_INVALID_ARG, "request %zu: a figure is 1 .. %u pixels wide and high (%u x %u)", i, TH_FIGURE_MAX_DIM, r.out_w,
                             r.out_h);
    if (!std::isfinite(r.left) || !std::isfinite(r.top) || !std::isfinite(r.width) || !std::isfinite(r.height) || !(r.width > 0.0) ||
        !(r.height > 0.0))
        return plan_error<S>(TH_ERR_INVALID_ARG, "request %zu: the box (%g, %g, %g, %g) has no finite positive extent", i, r.left, r.top,
                             r.width, r.height);
    const double W = (double)r.img_w, Hh = (double)r.img_h;
    if (r.left < 0.0 || r.top < 0.0 || r.left + r.width > W * (1.0 + 1e-12) || r.top + r.height > Hh * (1.0 + 1e-12))
        return plan_error<S>(TH_ERR_INVALID_ARG, "request %zu: the box (%g, %g, %g, %g) is not inside the %u x %u image", i, r.left, r.top,
                             r.width, r.height, r.img_w, r.img_h);
    // (plan_lod_tile's rule, word for word)
    const double est_taps = 6.0 * std::max(r.width / (double)r.out_w, r.height / (double)r.out_h) + 4.0;
    if (est_taps * 8.0 * (double)std::max(r.out_w, r.out_h) > 256.0 * 1024 * 1024)
        return plan_error<S>(TH_ERR_UNSUPPORTED, "request %zu: %u x %u pixels of a %g x %g box need a tap table beyond 256 MB", i, r.out_w,
                             r.out_h, r.width, r.height);
    if (r.img_pitch < r.img_w || r.img_pitch % 4 != 0 || (reinterpret_cast<uintptr_t>(r.img) & 7) != 0)
        return plan_error<S>(TH_ERR_INTERNAL, "request %zu: image rows must start on 8-byte boundaries (pitch %u)", i, r.img_pitch);
    return S{};
}

uint32_t figure_pick_oc(const int32_t *start, const int32_t *count, uint32_t n_out) {
    for (uint32_t oc = FIG_OC_MAX; oc > FIG_PASS; oc >>= 1) {
        bool fits = true;
        for (uint32_t o0 = 0; o0 < n_out && fits; o0 += oc) {
            const uint32_t o1 = std::min(n_out, o0 + oc) - 1;
            fits = (int64_t)start[o1] + count[o1] - (start[o0] & ~3) <= (int64_t)FIG_SPAN;
        }
        if (fits) return oc;
    }
    return FIG_PASS;
}

namespace {
// the table of (n_in, origin, extent, n_out): the one already made, or a new one appended to the blob
size_t axis_table(FigurePlan &p, uint32_t n_in, double origin, double extent, uint32_t n_out) {
    for (size_t k = 0; k < p.axes.size(); k++) {
        const FigureAxisTable &t = p.axes[k];
        if (t.n_in == n_in && t.n_out == n_out && t.origin == origin && t.extent == extent) return k;
    }
    LodAxisHost ax;
    build_lod_axis(origin, extent, n_out, 0, (long)n_in, ax);
    FigureAxisTable t;
    t.n_in = n_in;
    t.n_out = n_out;
    t.origin = origin;
    t.extent = extent;
    t.max_taps = ax.max_taps;
    t.oc = figure_pick_oc(ax.start.data(), ax.count.data(), n_out);
    t.at = align_up(p.axis_blob.size(), 8);
    const size_t n = n_out, wbytes = ax.w.size() * sizeof(double);
    p.axis_blob.resize(t.at + align_up(n * 8, 8) + wbytes);
    unsigned char *b = p.axis_blob.data() + t.at;
    std::memcpy(b, ax.start.data(), n * 4);
    std::memcpy(b + n * 4, ax.count.data(), n * 4);
    std::memcpy(b + n * 8, ax.w.data(), wbytes);
    t.start = std::move(ax.start);
    t.count = std::move(ax.count);
    p.axes.push_back(std::move(t));
    return p.axes.size() - 1;
}
}  // namespace

FigurePlan plan_figures(const FigurePlanRequest *reqs, size_t n) {
    FigurePlan p;
    for (size_t i = 0; i < n; i++) {
        const FigureStatus st = check_figure(reqs[i], i);
        if (st.err != TH_OK) return plan_error<FigurePlan>(st.err, "%s", st.err_text.c_str());
    }
    p.ax_of.resize(n);
    p.ay_of.resize(n);
    for (size_t i = 0; i < n; i++) {
        const FigurePlanRequest &r = reqs[i];
        p.ax_of[i] = axis_table(p, r.img_w, r.left, r.width, r.out_w);
        p.ay_of[i] = axis_table(p, r.img_h, r.top, r.height, r.out_h);
    }
    constexpr size_t TMP_ELEMS = (size_t)TH_FIGURE_TMP_BYTES / sizeof(uint16_t);
    FigurePiece pc;
    auto close_piece = [&]() {
        if (pc.part1 == pc.part0) return;
        const size_t b = p.pieces.size() & 1;
        p.stage_need[b] = std::max(p.stage_need[b], pc.stage_bytes);
        p.tmp_need = std::max(p.tmp_need, pc.tmp_elems);
        p.pieces.push_back(pc);
        pc = FigurePiece{};
        pc.part0 = pc.part1 = p.parts.size();
    };
    for (size_t i = 0; i < n; i++) {
        const FigurePlanRequest &r = reqs[i];
        const FigureAxisTable &ay = p.axes[p.ay_of[i]];
        const FigureAxisTable &ax = p.axes[p.ax_of[i]];
        const size_t row_bytes = (size_t)r.out_w * figure_bytes_per_pixel(r.kind);
        const size_t tmp_pitch = align_up(r.out_w, 8);
        // output rows [j0, j1) are the vertical outputs out_h - j1 .. out_h - 1 - j0: their windows' first and last source rows
        auto span = [&](uint32_t j0, uint32_t j1, uint32_t *y_lo, uint32_t *y_hi) {
            const uint32_t o_lo = r.out_h - j1, o_hi = r.out_h - 1 - j0;
            *y_lo = (uint32_t)ay.start[o_lo];
            *y_hi = std::max(*y_lo, (uint32_t)(ay.start[o_hi] + ay.count[o_hi]));
        };
        auto tmp_of = [&](uint32_t j0, uint32_t j1) {
            uint32_t a, b;
            span(j0, j1, &a, &b);
            return (size_t)(b - a) * tmp_pitch;
        };
        uint32_t j0 = 0;
        while (j0 < r.out_h) {
            const size_t stage_at = align_up(pc.stage_bytes, 64), tmp_at = align_up(pc.tmp_elems, 8);
            const size_t room = stage_at < TH_FIGURE_PIECE_BYTES ? (TH_FIGURE_PIECE_BYTES - stage_at) / row_bytes : 0;
            uint32_t lo = 0, hi = (uint32_t)std::min<size_t>(room, r.out_h - j0);  // the most rows whose intermediate still fits
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo + 1) / 2;
                if (tmp_at + tmp_of(j0, j0 + mid) <= TMP_ELEMS)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            uint32_t rows = lo;
            if (rows == 0) {
                if (pc.part1 != pc.part0) {  // a fresh piece has more room
                    close_piece();
                    continue;
                }
                rows = 1;  // (one output row alone is beyond TH_FIGURE_TMP_BYTES: it is its own piece)
            }
            FigurePart pt;
            pt.req = i;
            pt.j0 = j0;
            pt.j1 = j0 + rows;
            span(pt.j0, pt.j1, &pt.y_lo, &pt.y_hi);
            pt.tmp_at = tmp_at;
            pt.stage_at = stage_at;
            pt.out_at = r.offset + (uint64_t)j0 * row_bytes;
            pt.bytes = (size_t)rows * row_bytes;
            FigHJob h{};
            h.src_pitch = r.img_pitch;
            h.tmp_pitch = (uint32_t)tmp_pitch;
            h.y_lo = pt.y_lo;
            h.n_rows = pt.y_hi - pt.y_lo;
            h.oc = ax.oc;
            h.n_cblocks = (r.out_w + ax.oc - 1) / ax.oc;
            h.first_block = pc.n_hblocks;
            FigVJob v{};
            v.tmp_pitch = (uint32_t)tmp_pitch;
            v.y_lo = pt.y_lo;
            v.out_w = r.out_w;
            v.out_h = r.out_h;
            v.j0 = pt.j0;
            v.n_rows = rows;
            v.kind = r.kind;
            v.first_block = pc.n_vblocks;
            const uint64_t hb = (uint64_t)h.n_cblocks * ((h.n_rows + FIG_ROWS - 1) / FIG_ROWS);
            const uint64_t vb = ((pt.bytes + 15) / 16 + FIG_THREADS - 1) / FIG_THREADS;
            if (pc.n_hblocks + hb > 0x7fffffffull || pc.n_vblocks + vb > 0x7fffffffull)
                return plan_error<FigurePlan>(TH_ERR_UNSUPPORTED, "request %zu: a piece beyond 2^31 blocks", i);
            pc.n_hblocks += (uint32_t)hb;
            pc.n_vblocks += (uint32_t)vb;
            pc.stage_bytes = stage_at + pt.bytes;
            pc.tmp_elems = tmp_at + (size_t)h.n_rows * tmp_pitch;
            p.parts.push_back(pt);
            p.hjobs.push_back(h);
            p.vjobs.push_back(v);
            pc.part1 = p.parts.size();
            j0 += rows;
            if (j0 < r.out_h) close_piece();  // (the request did not fit: nothing else will)
        }
    }
    close_piece();
    p.o_hjobs = align_up(p.axis_blob.size(), 16);
    p.o_vjobs = p.o_hjobs + p.hjobs.size() * sizeof(FigHJob);
    p.tab_bytes = p.o_vjobs + p.vjobs.size() * sizeof(FigVJob);
    return p;
}

std::vector<unsigned char> bind_figures(FigurePlan &p, const FigureBases &b, const FigurePlanRequest *reqs) {
    auto axis = [&](size_t k) {
        const FigureAxisTable &t = p.axes[k];
        const unsigned char *at = b.tab + t.at;
        FigAxis a;
        a.start = reinterpret_cast<const int32_t *>(at);
        a.count = reinterpret_cast<const int32_t *>(at + (size_t)t.n_out * 4);
        a.w = reinterpret_cast<const double *>(at + (size_t)t.n_out * 8);
        a.n_out = t.n_out;
        a.max_taps = t.max_taps;
        return a;
    };
    for (size_t pi = 0; pi < p.pieces.size(); pi++)
        for (size_t k = p.pieces[pi].part0; k < p.pieces[pi].part1; k++) {
            const FigurePart &pt = p.parts[k];
            p.hjobs[k].src = reqs[pt.req].img;
            p.hjobs[k].tmp = b.tmp + pt.tmp_at;
            p.hjobs[k].ax = axis(p.ax_of[pt.req]);
            p.vjobs[k].tmp = b.tmp + pt.tmp_at;
            p.vjobs[k].dst = b.stage[pi & 1] + pt.stage_at;
            p.vjobs[k].ay = axis(p.ay_of[pt.req]);
        }
    std::vector<unsigned char> tab(p.tab_bytes, 0);
    if (!p.axis_blob.empty()) std::memcpy(tab.data(), p.axis_blob.data(), p.axis_blob.size());
    if (!p.hjobs.empty()) std::memcpy(tab.data() + p.o_hjobs, p.hjobs.data(), p.hjobs.size() * sizeof(FigHJob));
    if (!p.vjobs.empty()) std::memcpy(tab.data() + p.o_vjobs, p.vjobs.data(), p.vjobs.size() * sizeof(FigVJob));
    return tab;
}

}  // namespace th
