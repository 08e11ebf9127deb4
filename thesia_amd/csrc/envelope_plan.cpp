// envelope_plan.cpp — the host plans of th_tm_get_envelopes and th_tm_render_waveform_figures (envelope_plan.h)
#include "envelope_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "host_math.h"
#include "plan_error.h"

namespace th {

namespace {
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
}  // namespace

EnvelopeStatus check_envelope(const EnvelopePlanRequest &r, size_t i, uint64_t *e0, uint64_t *eW) {
    using S = EnvelopeStatus;
    double A = 0.0, B = 0.0;
    if (envelope_range(r.sr, r.n, r.start_sec, r.end_sec, r.n_cols, &A, &B) != 0)
        return plan_error<S>(TH_ERR_INVALID_ARG, "request %zu: bad envelope: [%g, %g) s of %llu samples at %u Hz in %u columns (1 .. %u)", i,
                             r.start_sec, r.end_sec, (unsigned long long)r.n, r.sr, r.n_cols, TH_ENVELOPE_MAX_COLS);
    if (r.n >= (1ull << 53)) return plan_error<S>(TH_ERR_UNSUPPORTED, "request %zu: a channel of 2^53 samples or more", i);
    if (!r.x || (reinterpret_cast<uintptr_t>(r.x) & 15) != 0)
        return plan_error<S>(TH_ERR_INTERNAL, "request %zu: the channel must start on a 16-byte boundary", i);
    *eW = (uint64_t)std::ceil(B);
    *e0 = std::min((uint64_t)std::ceil(A), *eW);
    return S{};
}

EnvelopeStatus check_lane(const LanePlanRequest &r, size_t i, uint64_t *e0, uint64_t *eW) {
    using S = EnvelopeStatus;
    if (r.n_cols == 0 || r.out_h == 0 || r.n_cols > TH_FIGURE_MAX_DIM || r.out_h > TH_FIGURE_MAX_DIM)
        return plan_error<S>(TH_ERR_INVALID_ARG, "request %zu: a waveform figure is 1 .. %u pixels wide and high (%u x %u)", i, TH_FIGURE_MAX_DIM,
                             r.n_cols, r.out_h);
    if (!std::isfinite(r.amp_lo) || !std::isfinite(r.amp_hi) || !(r.amp_lo < r.amp_hi))
        return plan_error<S>(TH_ERR_INVALID_ARG, "request %zu: the amplitude range [%g, %g] is not finite and ascending", i, (double)r.amp_lo,
                             (double)r.amp_hi);
    if (r.thickness > 256u * r.out_h)
        return plan_error<S>(TH_ERR_INVALID_ARG, "request %zu: a thickness of %u / 256 pixel in %u rows", i, r.thickness, r.out_h);
    return check_envelope(r, i, e0, eW);
}

EnvelopePlan plan_envelopes(const EnvelopePlanRequest *reqs, size_t n, size_t piece_bytes) {
    EnvelopePlan p;
    for (size_t i = 0; i < n; i++) {
        uint64_t e0, eW;
        const EnvelopeStatus st = check_envelope(reqs[i], i, &e0, &eW);
        if (st.err != TH_OK) return plan_error<EnvelopePlan>(st.err, "%s", st.err_text.c_str());
    }
    p.edge_at.resize(n);
    p.out_at.resize(n);
    p.part_at.resize(n);
    p.jobs.resize(n);
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        p.edge_at[i] = total;
        total += (size_t)reqs[i].n_cols + 1;
    }
    p.edges.resize(total);
    constexpr size_t PART_ELEMS = (size_t)TH_ENVELOPE_PART_BYTES / sizeof(EnvPartial);
    const size_t piece_floats = piece_bytes / sizeof(float);
    EnvelopePiece pc;
    auto close_piece = [&]() {
        if (pc.req1 == pc.req0) return;
        p.out_need = std::max(p.out_need, pc.out_floats);
        p.part_need = std::max(p.part_need, pc.part_elems);
        p.pieces.push_back(pc);
        const size_t at = pc.req1;
        pc = EnvelopePiece{};
        pc.req0 = pc.req1 = at;
    };
    for (size_t i = 0; i < n; i++) {
        const EnvelopePlanRequest &r = reqs[i];
        uint64_t *e = p.edges.data() + p.edge_at[i];
        if (envelope_edges(r.sr, r.n, r.start_sec, r.end_sec, r.n_cols, e) != 0)
            return plan_error<EnvelopePlan>(TH_ERR_INTERNAL, "request %zu: no edges for a checked request", i);
        const uint32_t W = r.n_cols;
        for (uint32_t j = 0; j < W; j++)  // (what keeps every read of the kernels inside the channel)
            if (e[j] > e[j + 1]) return plan_error<EnvelopePlan>(TH_ERR_INTERNAL, "request %zu: edge %u decreases", i, j);
        // (e[0] == e[W]: a range between two samples; every column holds sample max(e[0], 1) - 1, which is below n)
        if (e[W] > r.n) return plan_error<EnvelopePlan>(TH_ERR_INTERNAL, "request %zu: edges beyond the channel", i);
        EnvJob j{};
        j.W = W;
        j.e0 = e[0];
        j.eW = e[W];
        uint64_t chunks = 0;
        if (e[W] - e[0] >= (uint64_t)ENV_DENSE_MIN * W) {
            j.k0 = e[0] / ENV_CHUNK;
            chunks = (e[W] - 1) / ENV_CHUNK - j.k0 + 1;
        }
        const size_t floats = (size_t)W * 4, slots = (size_t)chunks * 2;
        if (pc.req1 != pc.req0 && (pc.out_floats + floats > piece_floats || pc.part_elems + slots > PART_ELEMS)) close_piece();
        const uint64_t cblocks = (W + ENV_THREADS - 1) / ENV_THREADS;
        if (pc.n_units + chunks > 0x7fffffffull || pc.n_cblocks + cblocks > 0x7fffffffull)
            return plan_error<EnvelopePlan>(TH_ERR_UNSUPPORTED, "request %zu: a piece beyond 2^31 blocks", i);
        j.n_chunks = (uint32_t)chunks;
        j.first_unit = pc.n_units;
        j.first_cblock = pc.n_cblocks;
        p.out_at[i] = pc.out_floats;
        p.part_at[i] = pc.part_elems;
        pc.n_units += (uint32_t)chunks;
        pc.n_cblocks += (uint32_t)cblocks;
        pc.out_floats += floats;
        pc.part_elems += slots;
        pc.req1 = i + 1;
        p.jobs[i] = j;
    }
    close_piece();
    p.o_jobs = align_up(p.edges.size() * sizeof(uint64_t), 16);
    p.tab_bytes = p.o_jobs + p.jobs.size() * sizeof(EnvJob);
    return p;
}

void bind_envelopes(EnvelopePlan &p, const EnvelopeBases &b, const EnvelopePlanRequest *reqs, unsigned char *tab) {
    for (size_t i = 0; i < p.jobs.size(); i++) {
        EnvJob &j = p.jobs[i];
        j.x = reqs[i].x;
        j.edges = reinterpret_cast<const uint64_t *>(b.tab) + p.edge_at[i];
        j.out = b.out + p.out_at[i];
        j.part = b.part + p.part_at[i];
    }
    std::memset(tab, 0, p.tab_bytes);
    if (!p.edges.empty()) std::memcpy(tab, p.edges.data(), p.edges.size() * sizeof(uint64_t));
    if (!p.jobs.empty()) std::memcpy(tab + p.o_jobs, p.jobs.data(), p.jobs.size() * sizeof(EnvJob));
}

LanePlan plan_lanes(const LanePlanRequest *reqs, size_t n) {
    LanePlan p;
    std::vector<EnvelopePlanRequest> er(n);
    for (size_t i = 0; i < n; i++) {
        uint64_t e0, eW;
        const EnvelopeStatus st = check_lane(reqs[i], i, &e0, &eW);
        if (st.err != TH_OK) return plan_error<LanePlan>(st.err, "%s", st.err_text.c_str());
        er[i] = reqs[i];
    }
    p.env = plan_envelopes(er.data(), n);
    if (p.env.err != TH_OK) return plan_error<LanePlan>(p.env.err, "%s", p.env.err_text.c_str());
    p.span_need = p.env.out_need / 2;
    p.sjobs.resize(n);
    LanePiece pc;
    auto close_piece = [&]() {
        if (pc.part1 == pc.part0) return;
        const size_t b = p.pieces.size() & 1;
        p.stage_need[b] = std::max(p.stage_need[b], pc.stage_bytes);
        p.pieces.push_back(pc);
        pc = LanePiece{};
        pc.part0 = pc.part1 = p.parts.size();
    };
    for (size_t g = 0; g < p.env.pieces.size(); g++) {
        const EnvelopePiece &grp = p.env.pieces[g];
        close_piece();  // (a piece reads one group's spans)
        pc.group = g;
        pc.first_of_group = true;
        uint32_t sblocks = 0;
        for (size_t i = grp.req0; i < grp.req1; i++) {
            const LanePlanRequest &r = reqs[i];
            LaneSpanJob s{};
            s.W = r.n_cols;
            s.out_h = r.out_h;
            s.amp_lo = r.amp_lo;
            s.amp_hi = r.amp_hi;
            s.thickness = r.thickness;
            s.first_block = sblocks;
            sblocks += (r.n_cols + ENV_THREADS - 1) / ENV_THREADS;  // (at most 2^31: the group's column blocks were checked)
            p.sjobs[i] = s;
            const size_t row_bytes = (size_t)r.n_cols * 4;
            uint32_t fill, background;
            std::memcpy(&fill, r.fill, 4);
            std::memcpy(&background, r.background, 4);
            uint32_t j0 = 0;
            while (j0 < r.out_h) {
                const size_t stage_at = align_up(pc.stage_bytes, 64);
                const size_t room = stage_at < TH_FIGURE_PIECE_BYTES ? (TH_FIGURE_PIECE_BYTES - stage_at) / row_bytes : 0;
                const uint32_t rows = (uint32_t)std::min<size_t>(room, r.out_h - j0);
                if (rows == 0) {  // (a fresh piece holds 128 rows of the widest request or more)
                    const size_t grp_of = pc.group;
                    close_piece();
                    pc.group = grp_of;
                    continue;
                }
                LanePart pt;
                pt.req = i;
                pt.j0 = j0;
                pt.j1 = j0 + rows;
                pt.stage_at = stage_at;
                pt.out_at = r.offset + (uint64_t)j0 * row_bytes;
                pt.bytes = (size_t)rows * row_bytes;
                LaneRasterJob rj{};
                rj.out_w = r.n_cols;
                rj.j0 = j0;
                rj.n_rows = rows;
                rj.fill = fill;
                rj.background = background;
                rj.first_block = pc.n_blocks;
                const uint64_t blocks = ((pt.bytes + 15) / 16 + ENV_THREADS - 1) / ENV_THREADS;
                if (pc.n_blocks + blocks > 0x7fffffffull) return plan_error<LanePlan>(TH_ERR_UNSUPPORTED, "request %zu: a piece beyond 2^31 blocks", i);
                pc.n_blocks += (uint32_t)blocks;
                pc.stage_bytes = stage_at + pt.bytes;
                p.parts.push_back(pt);
                p.rjobs.push_back(rj);
                pc.part1 = p.parts.size();
                j0 += rows;
            }
        }
        p.group_sblocks.push_back(sblocks);
    }
    close_piece();
    p.o_sjobs = align_up(p.env.tab_bytes, 16);
    p.o_rjobs = p.o_sjobs + align_up(p.sjobs.size() * sizeof(LaneSpanJob), 16);
    p.tab_bytes = p.o_rjobs + p.rjobs.size() * sizeof(LaneRasterJob);
    return p;
}

void bind_lanes(LanePlan &p, const LaneBases &b, const LanePlanRequest *reqs, unsigned char *tab) {
    std::vector<EnvelopePlanRequest> er(p.sjobs.size());
    for (size_t i = 0; i < er.size(); i++) er[i] = reqs[i];
    std::memset(tab, 0, p.tab_bytes);
    bind_envelopes(p.env, b.env, er.data(), tab);
    for (size_t i = 0; i < p.sjobs.size(); i++) {
        p.sjobs[i].env = b.env.out + p.env.out_at[i];
        p.sjobs[i].span = b.span + p.env.out_at[i] / 2;
    }
    for (size_t pi = 0; pi < p.pieces.size(); pi++)
        for (size_t k = p.pieces[pi].part0; k < p.pieces[pi].part1; k++) {
            p.rjobs[k].span = b.span + p.env.out_at[p.parts[k].req] / 2;
            p.rjobs[k].dst = b.stage[pi & 1] + p.parts[k].stage_at;
        }
    if (!p.sjobs.empty()) std::memcpy(tab + p.o_sjobs, p.sjobs.data(), p.sjobs.size() * sizeof(LaneSpanJob));
    if (!p.rjobs.empty()) std::memcpy(tab + p.o_rjobs, p.rjobs.data(), p.rjobs.size() * sizeof(LaneRasterJob));
}

}  // namespace th
