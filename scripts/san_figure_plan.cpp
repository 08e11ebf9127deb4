// san_figure_plan.cpp — plan_figures and bind_figures of thesia_amd/csrc/figure_plan.h under AddressSanitizer and UBSan, on a table of
// cases (single figures at the limits, ragged batches, requests that share axes, figures cut by the output bound and by the
// intermediate's bound, refused requests).  Image pointers are made-up addresses (a planner that read through one would fault here).
// Every plan is checked for what the run relies on: every output row of every request lies in exactly one part, a piece is never
// larger than its bounds, the regions of a piece's scratch and staging never overlap and are aligned, the job tables agree with the
// parts, identical tap tables are made once, and the bound table's pointers lie inside it.  A stand-alone program, never loaded into
// python.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined scripts/san_figure_plan.cpp
//       thesia_amd/csrc/figure_plan.cpp thesia_amd/csrc/host_math.cpp -o build/san_figure_plan && build/san_figure_plan   (one line)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "../thesia_amd/csrc/figure_plan.h"

using namespace th;

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            std::exit(2);                                                             \
        }                                                                             \
    } while (0)

static const uint16_t *const IMG = reinterpret_cast<const uint16_t *>(uintptr_t(0x7f0000000000ull));

static FigurePlanRequest req(uint32_t img_w, uint32_t img_h, uint32_t kind, uint32_t out_w, uint32_t out_h, double l, double t, double w, double h) {
    return FigurePlanRequest{IMG, img_w, img_h, (img_w + 63) / 64 * 64, kind, out_w, out_h, l, t, w, h, 0};
}

static void layout(std::vector<FigurePlanRequest> &rs) {
    uint64_t at = 0;
    for (auto &r : rs) {
        r.offset = at;
        at = (at + (uint64_t)r.out_w * r.out_h * figure_bytes_per_pixel(r.kind) + 63) & ~uint64_t(63);
    }
}

struct Totals {
    size_t plans = 0, pieces = 0, parts = 0, refused = 0, shared_axes = 0;
};

static void check_plan(std::vector<FigurePlanRequest> rs, Totals &tot, size_t want_pieces_at_least = 1) {
    layout(rs);
    FigurePlan p = plan_figures(rs.data(), rs.size());
    if (p.err != TH_OK) std::fprintf(stderr, "refused (%d): %s\n", p.err, p.err_text.c_str());
    EXPECT(p.err == TH_OK);
    const size_t n = rs.size();
    EXPECT(p.ax_of.size() == n && p.ay_of.size() == n);
    EXPECT(p.hjobs.size() == p.parts.size() && p.vjobs.size() == p.parts.size());
    EXPECT(p.pieces.size() >= want_pieces_at_least);
    // tables are deduplicated: no two axes with one key, and every request's axis has its key
    std::set<std::tuple<uint32_t, uint32_t, double, double>> keys;
    for (const FigureAxisTable &t : p.axes) {
        EXPECT(keys.insert({t.n_in, t.n_out, t.origin, t.extent}).second);
        EXPECT(t.at % 8 == 0 && t.at + (size_t)t.n_out * 8 + (size_t)t.n_out * t.max_taps * 8 <= p.axis_blob.size());
        EXPECT(t.oc % FIG_PASS == 0 && t.oc >= FIG_PASS && t.oc <= FIG_OC_MAX);
        EXPECT(t.oc == figure_pick_oc(t.start.data(), t.count.data(), t.n_out));
        if (t.oc > FIG_PASS)  // every run's span is staged at once
            for (uint32_t o0 = 0; o0 < t.n_out; o0 += t.oc) {
                const uint32_t o1 = std::min(t.n_out, o0 + t.oc) - 1;
                EXPECT(t.start[o1] + t.count[o1] - (t.start[o0] & ~3) <= (int32_t)FIG_SPAN);
            }
        for (uint32_t o = 0; o < t.n_out; o++) {
            EXPECT(t.start[o] >= 0 && t.count[o] >= 0 && (uint32_t)(t.start[o] + t.count[o]) <= t.n_in && (uint32_t)t.count[o] <= t.max_taps);
            if (o) EXPECT(t.start[o] >= t.start[o - 1] && t.start[o] + t.count[o] >= t.start[o - 1] + t.count[o - 1]);
        }
    }
    tot.shared_axes += 2 * n - p.axes.size();
    for (size_t i = 0; i < n; i++) {
        const FigureAxisTable &x = p.axes[p.ax_of[i]], &y = p.axes[p.ay_of[i]];
        EXPECT(x.n_in == rs[i].img_w && x.n_out == rs[i].out_w && x.origin == rs[i].left && x.extent == rs[i].width);
        EXPECT(y.n_in == rs[i].img_h && y.n_out == rs[i].out_h && y.origin == rs[i].top && y.extent == rs[i].height);
    }
    // every output row in exactly one part, in order; the pieces partition the parts
    std::vector<uint32_t> next_row(n, 0);
    size_t part = 0, last_req = 0;
    size_t need[2] = {0, 0}, tmp_need = 0;
    for (size_t pi = 0; pi < p.pieces.size(); pi++) {
        const FigurePiece &pc = p.pieces[pi];
        EXPECT(pc.part0 == part && pc.part1 > pc.part0 && pc.part1 <= p.parts.size());
        EXPECT(pc.stage_bytes <= TH_FIGURE_PIECE_BYTES);
        const bool one_row = pc.part1 - pc.part0 == 1 && p.parts[pc.part0].j1 - p.parts[pc.part0].j0 == 1;
        EXPECT(pc.tmp_elems * sizeof(uint16_t) <= TH_FIGURE_TMP_BYTES || one_row);
        size_t stage_end = 0, tmp_end = 0;
        uint32_t hb = 0, vb = 0;
        for (size_t k = pc.part0; k < pc.part1; k++) {
            const FigurePart &pt = p.parts[k];
            const FigurePlanRequest &r = rs[pt.req];
            const FigureAxisTable &y = p.axes[p.ay_of[pt.req]];
            EXPECT(pt.req >= last_req);
            last_req = pt.req;
            EXPECT(pt.j0 == next_row[pt.req] && pt.j1 > pt.j0 && pt.j1 <= r.out_h);
            next_row[pt.req] = pt.j1;
            const size_t row_bytes = (size_t)r.out_w * figure_bytes_per_pixel(r.kind);
            EXPECT(pt.bytes == (size_t)(pt.j1 - pt.j0) * row_bytes && pt.out_at == r.offset + (uint64_t)pt.j0 * row_bytes);
            // the band's windows lie inside [y_lo, y_hi)
            for (uint32_t j = pt.j0; j < pt.j1; j++) {
                const uint32_t oy = r.out_h - 1 - j;
                EXPECT((uint32_t)y.start[oy] >= pt.y_lo && (uint32_t)(y.start[oy] + y.count[oy]) <= pt.y_hi);
            }
            EXPECT(pt.y_hi <= r.img_h && pt.y_hi >= pt.y_lo);
            // staging and scratch: aligned, ascending, disjoint, inside the piece
            EXPECT(pt.stage_at % 64 == 0 && pt.stage_at >= stage_end);
            stage_end = pt.stage_at + pt.bytes;
            EXPECT(stage_end <= pc.stage_bytes);
            const FigHJob &h = p.hjobs[k];
            const FigVJob &v = p.vjobs[k];
            EXPECT(pt.tmp_at % 8 == 0 && pt.tmp_at >= tmp_end && h.tmp_pitch % 8 == 0 && h.tmp_pitch >= r.out_w);
            tmp_end = pt.tmp_at + (size_t)(pt.y_hi - pt.y_lo) * h.tmp_pitch;
            EXPECT(tmp_end <= pc.tmp_elems);
            EXPECT(h.y_lo == pt.y_lo && h.n_rows == pt.y_hi - pt.y_lo && h.src_pitch == r.img_pitch && h.first_block == hb);
            EXPECT(h.oc == p.axes[p.ax_of[pt.req]].oc && h.n_cblocks == (r.out_w + h.oc - 1) / h.oc);
            hb += h.n_cblocks * ((h.n_rows + FIG_ROWS - 1) / FIG_ROWS);
            EXPECT(v.y_lo == pt.y_lo && v.tmp_pitch == h.tmp_pitch && v.out_w == r.out_w && v.out_h == r.out_h && v.j0 == pt.j0 &&
                   v.n_rows == pt.j1 - pt.j0 && v.kind == r.kind && v.first_block == vb);
            vb += (uint32_t)(((pt.bytes + 15) / 16 + FIG_THREADS - 1) / FIG_THREADS);
        }
        EXPECT(hb == pc.n_hblocks && vb == pc.n_vblocks);
        need[pi & 1] = std::max(need[pi & 1], pc.stage_bytes);
        tmp_need = std::max(tmp_need, pc.tmp_elems);
        part = pc.part1;
    }
    EXPECT(part == p.parts.size());
    for (size_t i = 0; i < n; i++) EXPECT(next_row[i] == rs[i].out_h);
    EXPECT(need[0] == p.stage_need[0] && need[1] == p.stage_need[1] && tmp_need == p.tmp_need);
    // bind: every pointer inside its buffer
    std::vector<uint8_t> st0(std::max<size_t>(p.stage_need[0], 1)), st1(std::max<size_t>(p.stage_need[1], 1));
    std::vector<uint16_t> tmp(std::max<size_t>(p.tmp_need, 1));
    std::vector<unsigned char> dev(p.tab_bytes);
    const std::vector<unsigned char> tab = bind_figures(p, FigureBases{{st0.data(), st1.data()}, tmp.data(), dev.data()}, rs.data());
    EXPECT(tab.size() == p.tab_bytes && p.o_hjobs % 16 == 0 && p.o_vjobs == p.o_hjobs + p.hjobs.size() * sizeof(FigHJob));
    std::memcpy(dev.data(), tab.data(), tab.size());
    for (size_t pi = 0; pi < p.pieces.size(); pi++)
        for (size_t k = p.pieces[pi].part0; k < p.pieces[pi].part1; k++) {
            FigHJob h;
            FigVJob v;
            std::memcpy(&h, dev.data() + p.o_hjobs + k * sizeof(FigHJob), sizeof h);
            std::memcpy(&v, dev.data() + p.o_vjobs + k * sizeof(FigVJob), sizeof v);
            const std::vector<uint8_t> &st = pi & 1 ? st1 : st0;
            EXPECT(h.src == IMG && h.tmp == tmp.data() + p.parts[k].tmp_at && v.tmp == h.tmp);
            EXPECT(v.dst == st.data() + p.parts[k].stage_at && v.dst + p.parts[k].bytes <= st.data() + st.size());
            EXPECT(h.tmp + (size_t)h.n_rows * h.tmp_pitch <= tmp.data() + tmp.size());
            for (const FigAxis *a : {&h.ax, &v.ay}) {
                const unsigned char *s = reinterpret_cast<const unsigned char *>(a->start), *w = reinterpret_cast<const unsigned char *>(a->w);
                EXPECT(s >= dev.data() && w + (size_t)a->n_out * a->max_taps * 8 <= dev.data() + p.o_hjobs);
                EXPECT(reinterpret_cast<const unsigned char *>(a->count) == s + (size_t)a->n_out * 4 && w == s + (size_t)a->n_out * 8);
                // (the table reads back as the axis: the first start and the weights of output 0 sum to 1)
                int32_t s0, c0;
                std::memcpy(&s0, s, 4);
                std::memcpy(&c0, a->count, 4);
                double sum = 0;
                for (int32_t t = 0; t < c0; t++) {
                    double wv;
                    std::memcpy(&wv, w + (size_t)t * 8, 8);
                    sum += wv;
                }
                EXPECT(s0 >= 0 && c0 > 0 && sum > 0.999999 && sum < 1.000001);
            }
        }
    tot.plans++;
    tot.pieces += p.pieces.size();
    tot.parts += p.parts.size();
}

static void check_refused(FigurePlanRequest r, int code, Totals &tot) {
    std::vector<FigurePlanRequest> rs{req(300, 129, TH_FIGURE_RGBA, 8, 4, 0, 0, 16, 8), r};
    layout(rs);
    const FigurePlan p = plan_figures(rs.data(), rs.size());
    EXPECT(p.err == code && !p.err_text.empty() && p.pieces.empty());
    EXPECT(check_figure(r, 1).err == code);
    tot.refused++;
}

int main() {
    Totals tot;
    const uint32_t R = TH_FIGURE_RGBA, G = TH_FIGURE_GREY16;
    // single figures
    check_plan({req(300, 129, R, 1, 1, 0, 0, 300, 129)}, tot);
    check_plan({req(300, 129, G, 64, 3, 150.25, 64.5, 0.75, 0.5)}, tot);
    check_plan({req(300, 129, R, 300, 129, 0, 0, 300, 129)}, tot);
    check_plan({req(6000, 33, G, 3, 33, 0, 0, 6000, 33)}, tot);          // the stepped walk: oc 16
    check_plan({req(1025, 129, R, 512, 129, 0, 0, 1025, 129)}, tot);
    check_plan({req(180000, 1025, R, 2000, 800, 0, 0, 180000, 1025)}, tot);  // a 30-minute overview
    check_plan({req(1, 1, R, 5, 7, 0, 0, 1, 1)}, tot);
    // just above the output bound: 1025 rows of 2048 RGBA pixels; and exactly at it
    check_plan({req(300, 129, R, 2048, 1025, 20.25, 30.5, 40, 20)}, tot, 2);
    check_plan({req(300, 129, R, 2048, 1024, 20.25, 30.5, 40, 20)}, tot);
    check_plan({req(300, 129, G, 16384, 300, 0, 0, 300, 129)}, tot, 2);
    // the intermediate's bound cuts the band; and one output row alone is beyond it
    check_plan({req(2600, 1300, G, 8192, 40, 100, 0, 2048, 1300)}, tot, 2);
    check_plan({req(20000, 4096, G, 16384, 2, 0, 0, 20000, 600)}, tot, 2);  // 1800 source rows x 16384 x 2 bytes per output row
    check_plan({req(300, 129, R, 16384, 16384, 0, 0, 300, 129)}, tot, 128);
    // batches: ragged sizes, shared axes, both kinds, many small requests in one piece, a batch over several pieces
    check_plan({req(300, 129, R, 64, 48, 10, 5, 128, 96), req(1025, 129, G, 64, 7, 10, 2.5, 128, 100), req(300, 129, G, 64, 31, 10, 7, 128, 31),
                req(77, 129, R, 3, 5, 0, 0, 77, 129), req(300, 129, R, 1, 1, 1, 1, 2, 2), req(1025, 129, R, 257, 129, 0, 0, 1025, 129)}, tot);
    {
        std::vector<FigurePlanRequest> many;
        for (int k = 0; k < 128; k++) many.push_back(req(3000, 401, k & 1 ? G : R, 1024, 256, 0, 0, 3000, 401));
        const size_t before = tot.shared_axes;
        check_plan(many, tot, 8);
        EXPECT(tot.shared_axes - before == 254);  // 256 axes asked for, 2 made
    }
    {
        std::vector<FigurePlanRequest> mix;
        for (int k = 0; k < 40; k++) mix.push_back(req(500 + 37 * k, 200 + k, k % 3 ? R : G, 100 + 171 * k, 1 + 53 * k, 0.5 * k, 0.25 * k, 300 + k, 150));
        check_plan(mix, tot, 2);
    }
    // refused
    check_refused(req(300, 129, 2, 8, 4, 0, 0, 16, 8), TH_ERR_INVALID_ARG, tot);
    check_refused(req(300, 129, R, 0, 4, 0, 0, 16, 8), TH_ERR_INVALID_ARG, tot);
    check_refused(req(300, 129, R, 8, 16385, 0, 0, 16, 8), TH_ERR_INVALID_ARG, tot);
    check_refused(req(300, 129, R, 8, 4, 0, 0, 0, 8), TH_ERR_INVALID_ARG, tot);
    check_refused(req(300, 129, R, 8, 4, 0, 0, -3, 8), TH_ERR_INVALID_ARG, tot);
    check_refused(req(300, 129, R, 8, 4, 0, 0, 16, __builtin_inf()), TH_ERR_INVALID_ARG, tot);
    check_refused(req(300, 129, R, 8, 4, __builtin_nan(""), 0, 16, 8), TH_ERR_INVALID_ARG, tot);
    check_refused(req(300, 129, R, 8, 4, -0.5, 0, 16, 8), TH_ERR_INVALID_ARG, tot);
    check_refused(req(300, 129, R, 8, 4, 290, 0, 16, 8), TH_ERR_INVALID_ARG, tot);
    check_refused(req(300, 129, R, 8, 4, 0, 122, 16, 8), TH_ERR_INVALID_ARG, tot);
    check_refused(req(0, 0, R, 8, 4, 0, 0, 16, 8), TH_ERR_INVALID_ARG, tot);
    check_refused(req(1025, 129, G, 1, 16384, 0, 0, 1025, 129), TH_ERR_UNSUPPORTED, tot);
    std::printf("san_figure_plan: %zu plans (%zu pieces, %zu parts, %zu tap tables shared), %zu refused, nothing reported\n", tot.plans, tot.pieces,
                tot.parts, tot.shared_axes, tot.refused);
    return 0;
}
