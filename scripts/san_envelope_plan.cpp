// san_envelope_plan.cpp — th_envelope_edges' definition, plan_envelopes / bind_envelopes and plan_lanes / bind_lanes of
// thesia_amd/csrc/envelope_plan.h under AddressSanitizer and UBSan, on a table of adversarial requests (one column across a track, 65536
// columns, views zoomed in past one sample per column, ranges on and off the chunk grid, one-sample channels, batches cut by the
// result bound and by the partials' bound, lanes cut into bands, refused requests).  Channel pointers are made-up addresses (a planner
// that read through one would fault here).  Every plan is checked for what the run relies on: edges that never decrease and end inside
// the channel, pieces within their bounds, result, partial and staging regions that are aligned and never overlap, job tables that
// agree with the requests, and bound pointers inside their areas.  The walk of the two envelope kernels is then repeated on the host,
// index for index: every sample of a request is read exactly once, every column is written exactly once, every partial that is added
// was written exactly once, and no index leaves the channel or the tables.  A stand-alone program, never loaded into python.  From the
// repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined scripts/san_envelope_plan.cpp
//       thesia_amd/csrc/envelope_plan.cpp thesia_amd/csrc/host_math.cpp -o build/san_envelope_plan && build/san_envelope_plan   (one line)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../thesia_amd/csrc/envelope_plan.h"
#include "../thesia_amd/csrc/host_math.h"

using namespace th;

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            std::exit(2);                                                             \
        }                                                                             \
    } while (0)

static const float *const CHAN = reinterpret_cast<const float *>(uintptr_t(0x7f0000000000ull));
static const double INF = __builtin_inf(), NaN = __builtin_nan("");

static EnvelopePlanRequest req(uint32_t sr, uint64_t n, double a, double b, uint32_t W) { return EnvelopePlanRequest{CHAN, n, sr, W, a, b, 0}; }
static LanePlanRequest lane(uint32_t sr, uint64_t n, double a, double b, uint32_t W, uint32_t H, float lo = -1.f, float hi = 1.f,
                            uint32_t th = 256) {
    LanePlanRequest r{};
    static_cast<EnvelopePlanRequest &>(r) = req(sr, n, a, b, W);
    r.out_h = H;
    r.amp_lo = lo;
    r.amp_hi = hi;
    r.thickness = th;
    r.fill[3] = 255;
    return r;
}

struct Totals {
    size_t plans = 0, pieces = 0, refused = 0, walked = 0, lane_parts = 0;
};

// the index walk of envelope_reduce_kernel and envelope_columns_kernel for request i of plan p (kernels_envelope.hip)
static void walk(const EnvelopePlan &p, size_t i, const EnvelopePlanRequest &r, Totals &tot) {
    const EnvJob &job = p.jobs[i];
    const uint64_t *e = p.edges.data() + p.edge_at[i];
    const uint32_t W = job.W;
    const uint64_t first = e[0], last = e[W];
    EXPECT(last <= r.n && first <= last && job.e0 == first && job.eW == last);  // (first == last: a range between two samples, every column held)
    std::vector<uint8_t> read((size_t)(last - first), 0), wrote(W, 0), slot((size_t)job.n_chunks * 2, 0);
    auto touch = [&](uint64_t s0, uint64_t s1) {
        EXPECT(first <= s0 && s0 < s1 && s1 <= last);
        // env_segment: whole quads [qa, qb), a head and a tail of at most 3 samples
        const uint64_t qa = (s0 + 3) >> 2, qb = s1 >> 2, h1 = std::min(qa << 2, s1), t0 = qa < qb ? (qb << 2) : h1;
        EXPECT(h1 - s0 <= 3 && s1 - t0 <= 3 && t0 >= h1);
        for (uint64_t s = s0; s < h1; s++) read[(size_t)(s - first)]++;
        for (uint64_t q = qa; q < qb; q++)
            for (uint64_t s = q << 2; s < (q << 2) + 4; s++) {
                EXPECT(s >= s0 && s < s1);
                read[(size_t)(s - first)]++;
            }
        for (uint64_t s = t0; s < s1; s++) read[(size_t)(s - first)]++;
    };
    for (uint32_t kr = 0; kr < job.n_chunks; kr++) {
        const uint64_t k = job.k0 + kr;
        const uint64_t c0 = std::max(k * ENV_CHUNK, first), c1 = std::min((k + 1) * ENV_CHUNK, last);
        EXPECT(c0 < c1);
        uint32_t j = std::min((uint32_t)((double)(c0 - first) * (double)W / (double)(last - first)), W - 1), steps = 0;
        while (e[j] > c0) {
            EXPECT(j > 0);
            j--;
            steps++;
        }
        while (e[j + 1] <= c0) {
            EXPECT(j + 1 < W);
            j++;
            steps++;
        }
        EXPECT(steps <= 2);  // (the guess from the even spacing is next to the column)
        uint64_t s0 = c0;
        bool head = true;
        while (s0 < c1) {
            EXPECT(j < W && e[j] <= s0 && s0 < e[j + 1]);
            const uint64_t s1 = std::min(e[j + 1], c1);
            touch(s0, s1);
            if (s0 == e[j] && s1 == e[j + 1])
                wrote[j]++;
            else
                slot[(size_t)kr * 2 + (head ? 0 : 1)]++;
            head = false;
            s0 = s1;
            if (s0 >= c1) break;
            j++;
            while (j + 1 < W && e[j + 1] <= s0) j++;
        }
    }
    for (uint32_t j = 0; j < W; j++) {
        const uint64_t e0 = e[j], e1 = e[j + 1];
        if (e1 == e0) {
            EXPECT((e0 > 0 ? e0 : 1) - 1 < r.n);
            wrote[j]++;
        } else if (job.n_chunks == 0) {
            for (uint64_t s = e0; s < e1; s++) read[(size_t)(s - first)]++;
            wrote[j]++;
        } else {
            const uint64_t ka = e0 / ENV_CHUNK, kb = (e1 - 1) / ENV_CHUNK;
            if (ka == kb) continue;
            for (uint64_t k = ka; k <= kb; k++) {
                const uint64_t c0 = std::max(k * ENV_CHUNK, first);
                const size_t at = (size_t)(k - job.k0) * 2 + (e0 <= c0 ? 0 : 1);
                EXPECT(at < slot.size() && slot[at] == 1);
                slot[at] = 2;  // (added once)
            }
            wrote[j]++;
        }
    }
    for (uint8_t v : read) EXPECT(v == 1);
    for (uint8_t v : wrote) EXPECT(v == 1);
    for (uint8_t v : slot) EXPECT(v == 0 || v == 2);
    tot.walked++;
}

static void check_env(const EnvelopePlan &p, const EnvelopePlanRequest *rs, size_t n, size_t piece_bytes, Totals &tot, bool do_walk) {
    EXPECT(p.jobs.size() == n && p.edge_at.size() == n && p.out_at.size() == n && p.part_at.size() == n);
    size_t next = 0;
    for (const EnvelopePiece &pc : p.pieces) {
        EXPECT(pc.req0 == next && pc.req1 > pc.req0 && pc.req1 <= n);
        next = pc.req1;
        size_t floats = 0, slots = 0;
        uint32_t units = 0, cblocks = 0;
        for (size_t i = pc.req0; i < pc.req1; i++) {
            const EnvJob &j = p.jobs[i];
            EXPECT(j.W == rs[i].n_cols && p.out_at[i] == floats && p.out_at[i] % 4 == 0 && p.part_at[i] == slots);
            EXPECT(j.first_unit == units && j.first_cblock == cblocks);
            const uint64_t *e = p.edges.data() + p.edge_at[i];
            for (uint32_t c = 0; c < j.W; c++) EXPECT(e[c] <= e[c + 1]);
            EXPECT(e[j.W] <= rs[i].n && e[0] <= e[j.W] && j.e0 == e[0] && j.eW == e[j.W]);
            const bool dense = e[j.W] - e[0] >= (uint64_t)ENV_DENSE_MIN * j.W;
            EXPECT(dense == (j.n_chunks != 0));
            if (dense) EXPECT(j.k0 == e[0] / ENV_CHUNK && j.k0 + j.n_chunks - 1 == (e[j.W] - 1) / ENV_CHUNK);
            floats += (size_t)j.W * 4;
            slots += (size_t)j.n_chunks * 2;
            units += j.n_chunks;
            cblocks += (j.W + ENV_THREADS - 1) / ENV_THREADS;
        }
        EXPECT(pc.out_floats == floats && pc.part_elems == slots && pc.n_units == units && pc.n_cblocks == cblocks);
        EXPECT(floats <= p.out_need && slots <= p.part_need);
        if (pc.req1 - pc.req0 > 1) EXPECT(floats * 4 <= piece_bytes && slots * sizeof(EnvPartial) <= TH_ENVELOPE_PART_BYTES);
        EXPECT(floats * 4 <= std::max<size_t>(piece_bytes, 1u << 20));
        tot.pieces++;
    }
    EXPECT(next == n);
    EXPECT(p.o_jobs % 16 == 0 && p.o_jobs >= p.edges.size() * 8 && p.tab_bytes == p.o_jobs + n * sizeof(EnvJob));
    if (do_walk)
        for (size_t i = 0; i < n; i++) walk(p, i, rs[i], tot);
}

static void check_bound(const EnvelopePlan &p, const EnvelopeBases &b, const std::vector<unsigned char> &tab, size_t tab0) {
    for (size_t i = 0; i < p.jobs.size(); i++) {
        EnvJob j;
        std::memcpy(&j, tab.data() + tab0 + p.o_jobs + i * sizeof(EnvJob), sizeof j);
        EXPECT(j.x == CHAN);
        EXPECT(reinterpret_cast<const unsigned char *>(j.edges) >= b.tab && reinterpret_cast<const unsigned char *>(j.edges + j.W + 1) <= b.tab + p.o_jobs);
        EXPECT(j.out >= b.out && j.out + (size_t)j.W * 4 <= b.out + p.out_need && (reinterpret_cast<uintptr_t>(j.out) & 15) == 0);
        EXPECT(j.part >= b.part && j.part + (size_t)j.n_chunks * 2 <= b.part + p.part_need);
        uint64_t e0;
        std::memcpy(&e0, tab.data() + tab0 + (reinterpret_cast<const unsigned char *>(j.edges) - b.tab), 8);
        EXPECT(e0 == p.edges[p.edge_at[i]]);
    }
}

static void check_plan(std::vector<EnvelopePlanRequest> rs, Totals &tot, size_t want_pieces = 1, size_t piece_bytes = TH_ENVELOPE_PIECE_BYTES,
                       bool do_walk = true) {
    uint64_t at = 0;
    for (auto &r : rs) {
        r.offset = at;
        at += (uint64_t)r.n_cols * 4;
    }
    EnvelopePlan p = plan_envelopes(rs.data(), rs.size(), piece_bytes);
    if (p.err != TH_OK) std::fprintf(stderr, "refused (%d): %s\n", p.err, p.err_text.c_str());
    EXPECT(p.err == TH_OK && p.pieces.size() == want_pieces);
    check_env(p, rs.data(), rs.size(), piece_bytes, tot, do_walk);
    EnvelopeBases b{reinterpret_cast<float *>(uintptr_t(0x7e0000000000ull)), reinterpret_cast<EnvPartial *>(uintptr_t(0x7d0000000000ull)),
                    reinterpret_cast<unsigned char *>(uintptr_t(0x7c0000000000ull))};
    std::vector<unsigned char> tab(p.tab_bytes);
    bind_envelopes(p, b, rs.data(), tab.data());
    check_bound(p, b, tab, 0);
    tot.plans++;
}

static void check_lanes(std::vector<LanePlanRequest> rs, Totals &tot, size_t want_pieces_at_least = 1) {
    uint64_t at = 0;
    for (auto &r : rs) {
        r.offset = at;
        at = (at + (uint64_t)r.n_cols * r.out_h * 4 + 63) & ~uint64_t(63);
    }
    LanePlan p = plan_lanes(rs.data(), rs.size());
    if (p.err != TH_OK) std::fprintf(stderr, "refused (%d): %s\n", p.err, p.err_text.c_str());
    EXPECT(p.err == TH_OK && p.pieces.size() >= want_pieces_at_least);
    const size_t n = rs.size();
    std::vector<EnvelopePlanRequest> er(rs.begin(), rs.end());
    check_env(p.env, er.data(), n, TH_ENVELOPE_PIECE_BYTES, tot, false);
    EXPECT(p.sjobs.size() == n && p.rjobs.size() == p.parts.size() && p.group_sblocks.size() == p.env.pieces.size());
    EXPECT(p.span_need * 2 == p.env.out_need);
    std::vector<uint32_t> next_row(n, 0);
    size_t next_part = 0, group = 0;
    std::vector<bool> group_started(p.env.pieces.size(), false);
    for (size_t pi = 0; pi < p.pieces.size(); pi++) {
        const LanePiece &pc = p.pieces[pi];
        EXPECT(pc.part0 == next_part && pc.part1 > pc.part0 && pc.stage_bytes <= TH_FIGURE_PIECE_BYTES && pc.stage_bytes <= p.stage_need[pi & 1]);
        EXPECT(pc.group >= group && pc.group < p.env.pieces.size());
        group = pc.group;
        EXPECT(pc.first_of_group == !group_started[group]);
        group_started[group] = true;
        next_part = pc.part1;
        size_t end = 0;
        uint32_t blocks = 0;
        for (size_t k = pc.part0; k < pc.part1; k++) {
            const LanePart &pt = p.parts[k];
            const LaneRasterJob &rj = p.rjobs[k];
            const LanePlanRequest &r = rs[pt.req];
            EXPECT(pt.req >= p.env.pieces[group].req0 && pt.req < p.env.pieces[group].req1);
            EXPECT(pt.j0 == next_row[pt.req] && pt.j1 > pt.j0 && pt.j1 <= r.out_h);
            next_row[pt.req] = pt.j1;
            EXPECT(pt.stage_at % 64 == 0 && pt.stage_at >= end && pt.bytes == (size_t)(pt.j1 - pt.j0) * r.n_cols * 4);
            end = pt.stage_at + pt.bytes;
            EXPECT(end <= pc.stage_bytes && pt.out_at == r.offset + (uint64_t)pt.j0 * r.n_cols * 4);
            EXPECT(rj.out_w == r.n_cols && rj.j0 == pt.j0 && rj.n_rows == pt.j1 - pt.j0 && rj.first_block == blocks);
            blocks += (uint32_t)(((pt.bytes + 15) / 16 + ENV_THREADS - 1) / ENV_THREADS);
            tot.lane_parts++;
        }
        EXPECT(blocks == pc.n_blocks);
        tot.pieces++;
    }
    EXPECT(next_part == p.parts.size());
    for (size_t i = 0; i < n; i++) EXPECT(next_row[i] == rs[i].out_h);
    for (size_t g = 0; g < p.env.pieces.size(); g++) {
        EXPECT(group_started[g]);
        uint32_t sb = 0;
        for (size_t i = p.env.pieces[g].req0; i < p.env.pieces[g].req1; i++) {
            EXPECT(p.sjobs[i].first_block == sb && p.sjobs[i].W == rs[i].n_cols && p.sjobs[i].out_h == rs[i].out_h);
            sb += (rs[i].n_cols + ENV_THREADS - 1) / ENV_THREADS;
        }
        EXPECT(sb == p.group_sblocks[g]);
    }
    LaneBases b{};
    b.env = EnvelopeBases{reinterpret_cast<float *>(uintptr_t(0x7e0000000000ull)), reinterpret_cast<EnvPartial *>(uintptr_t(0x7d0000000000ull)),
                          reinterpret_cast<unsigned char *>(uintptr_t(0x7c0000000000ull))};
    b.span = reinterpret_cast<int32_t *>(uintptr_t(0x7b0000000000ull));
    b.stage[0] = reinterpret_cast<uint8_t *>(uintptr_t(0x7a0000000000ull));
    b.stage[1] = reinterpret_cast<uint8_t *>(uintptr_t(0x790000000000ull));
    std::vector<unsigned char> tab(p.tab_bytes);
    bind_lanes(p, b, rs.data(), tab.data());
    check_bound(p.env, b.env, tab, 0);
    EXPECT(p.o_sjobs % 16 == 0 && p.o_sjobs >= p.env.tab_bytes && p.o_rjobs % 8 == 0 && p.o_rjobs >= p.o_sjobs + n * sizeof(LaneSpanJob));
    EXPECT(p.tab_bytes == p.o_rjobs + p.rjobs.size() * sizeof(LaneRasterJob));
    for (size_t i = 0; i < n; i++) {
        LaneSpanJob s;
        std::memcpy(&s, tab.data() + p.o_sjobs + i * sizeof s, sizeof s);
        EXPECT(s.env == b.env.out + p.env.out_at[i] && s.span == b.span + p.env.out_at[i] / 2 && s.span + (size_t)s.W * 2 <= b.span + p.span_need);
    }
    for (size_t pi = 0; pi < p.pieces.size(); pi++)
        for (size_t k = p.pieces[pi].part0; k < p.pieces[pi].part1; k++) {
            LaneRasterJob rj;
            std::memcpy(&rj, tab.data() + p.o_rjobs + k * sizeof rj, sizeof rj);
            EXPECT(rj.dst == b.stage[pi & 1] + p.parts[k].stage_at && rj.span == b.span + p.env.out_at[p.parts[k].req] / 2);
        }
    tot.plans++;
}

static void check_refused(EnvelopePlanRequest r, int code, Totals &tot) {
    std::vector<EnvelopePlanRequest> rs{req(48000, 100000, 0, INF, 7), r};
    const EnvelopePlan p = plan_envelopes(rs.data(), rs.size());
    EXPECT(p.err == code && !p.err_text.empty() && p.pieces.empty());
    uint64_t a, b;
    EXPECT(check_envelope(r, 1, &a, &b).err == code);
    std::vector<uint64_t> e((size_t)std::min<uint32_t>(r.n_cols, TH_ENVELOPE_MAX_COLS) + 1);
    if (code == TH_ERR_INVALID_ARG) EXPECT(envelope_edges(r.sr, r.n, r.start_sec, r.end_sec, r.n_cols, e.data()) == 1);
    tot.refused++;
}

static void check_lane_refused(LanePlanRequest r, Totals &tot) {
    std::vector<LanePlanRequest> rs{lane(48000, 100000, 0, INF, 7, 5), r};
    const LanePlan p = plan_lanes(rs.data(), rs.size());
    EXPECT(p.err == TH_ERR_INVALID_ARG && !p.err_text.empty() && p.pieces.empty());
    tot.refused++;
}

int main() {
    Totals tot;
    // the issue's cases and the shapes of the GPU tests
    check_plan({req(48000, 100000, 0, INF, 7)}, tot);
    check_plan({req(48000, 100000, 0.5, 0.50625, 1000)}, tot);
    check_plan({req(8000, 40000, 0.0123, 4.2, 333)}, tot);
    check_plan({req(48000, 70001, 0, INF, 16384)}, tot);
    check_plan({req(48000, 1, 0, INF, 4)}, tot);
    for (uint32_t W : {1u, 2u, 3u, 7u, 333u, 1093u, 1094u, 4099u, 16384u, 65536u}) check_plan({req(48000, 70001, 0, INF, W)}, tot);
    check_plan({req(48000, 70001, 1.0 / 48000, INF, 5)}, tot);                              // starts on an odd sample
    check_plan({req(48000, 70001, 4096.0 / 48000, 8192.0 / 48000 * 2, 3)}, tot);            // on the chunk grid
    check_plan({req(48000, 70001, 4100.0 / 48000, 8000.0 / 48000, 9)}, tot);                // inside one chunk
    check_plan({req(48000, 70001, 4095.0 / 48000, 4097.0 / 48000, 1)}, tot);                // two samples across a chunk boundary
    check_plan({req(48000, 70001, 0, 2.5 / 48000, 1)}, tot);                                // three samples
    check_plan({req(1, 5, 0.5, 3.5, 3)}, tot);
    // ranges that hold no sample index (B > A, ceil(A) == ceil(B)): every column is a hold
    check_plan({req(48000, 70001, 0.2 / 48000, 0.7 / 48000, 5)}, tot);
    check_plan({req(48000, 70001, 1000.25 / 48000, 1000.75 / 48000, 1)}, tot);
    check_plan({req(48000, 70001, 70000.5 / 48000, INF, 65536)}, tot);
    check_plan({req(48000, 1, 0.25 / 48000, 0.5 / 48000, 3)}, tot);
    check_plan({req(4000000000u, 1ull << 32, 0.25, 0.9, 640)}, tot, 1, TH_ENVELOPE_PIECE_BYTES, false);
    check_plan({req(48000, 86400000, 12.4, 47.9, 1800)}, tot);                              // 1800 pixels of a 30-minute track
    check_plan({req(48000, 86400000, 0, INF, 1800)}, tot);
    check_plan({req(48000, 86400000, 0, INF, 65536)}, tot);
    // batches: ragged, cut by the result bound, by the partials' bound, by a small bound, one request above the partials' bound
    check_plan({req(48000, 70001, 0, INF, 7), req(48000, 1, 0, INF, 4), req(8000, 40000, 0.0123, 4.2, 333), req(48000, 70001, 0.5, 0.50625, 1000),
                req(48000, 70001, 0, INF, 4099)}, tot);
    {
        std::vector<EnvelopePlanRequest> many;
        for (int k = 0; k < 20; k++) many.push_back(req(48000, 70001, 0, INF, 16384));
        check_plan(many, tot, 2);                                   // 16 requests of 256 KiB fill 4 MiB
        check_plan(many, tot, 20, 1 << 16, false);                  // (a bound below one request: a piece each)
        many.assign(128, req(48000, 86400000, 0, INF, 1800));
        check_plan(many, tot, 4, TH_ENVELOPE_PIECE_BYTES, false);   // 42 188 slots per request, 1 398 101 fit 32 MiB: 33 requests a piece
    }
    check_plan({req(48000, 70001, 0, INF, 7), req(192000, 1ull << 40, 0, INF, 1800), req(48000, 70001, 0, INF, 7)}, tot, 3,
               TH_ENVELOPE_PIECE_BYTES, false);
    // lanes
    check_lanes({lane(48000, 70001, 0, INF, 333, 64)}, tot);
    check_lanes({lane(48000, 70001, 0, INF, 7, 5), lane(48000, 1, 0, INF, 1, 1), lane(48000, 70001, 0.1, 0.9, 2048, 1)}, tot);
    check_lanes({lane(48000, 70001, 1000.25 / 48000, 1000.75 / 48000, 9, 4), lane(48000, 70001, 0, INF, 9, 4)}, tot);
    check_lanes({lane(48000, 70001, 0, INF, 2048, 1025)}, tot, 2);
    check_lanes({lane(48000, 70001, 0, INF, 2048, 1024)}, tot);
    check_lanes({lane(48000, 70001, 0, INF, 16384, 16384, -0.5f, 0.25f, 0)}, tot, 128);
    {
        std::vector<LanePlanRequest> many;
        for (int k = 0; k < 40; k++) many.push_back(lane(48000, 70001 + k, 0.001 * k, INF, 16384 - 100 * k, 3 + 7 * k));
        check_lanes(many, tot, 2);                                  // 40 x 256 KiB of envelopes: three groups
    }
    // refused
    check_refused(req(48000, 100000, NaN, 1, 7), TH_ERR_INVALID_ARG, tot);
    check_refused(req(48000, 100000, 0, NaN, 7), TH_ERR_INVALID_ARG, tot);
    check_refused(req(48000, 100000, -0.1, 1, 7), TH_ERR_INVALID_ARG, tot);
    check_refused(req(48000, 100000, INF, INF, 7), TH_ERR_INVALID_ARG, tot);
    check_refused(req(48000, 100000, 1, 1, 7), TH_ERR_INVALID_ARG, tot);
    check_refused(req(48000, 100000, 1, 0.5, 7), TH_ERR_INVALID_ARG, tot);
    check_refused(req(48000, 100000, 3, 4, 7), TH_ERR_INVALID_ARG, tot);      // both clamp to the end
    check_refused(req(48000, 100000, 0, -INF, 7), TH_ERR_INVALID_ARG, tot);
    check_refused(req(0, 100000, 0, 1, 7), TH_ERR_INVALID_ARG, tot);
    check_refused(req(48000, 0, 0, 1, 7), TH_ERR_INVALID_ARG, tot);
    check_refused(req(48000, 100000, 0, 1, 0), TH_ERR_INVALID_ARG, tot);
    check_refused(req(48000, 100000, 0, 1, 65537), TH_ERR_INVALID_ARG, tot);
    check_refused(req(48000, 1ull << 53, 0, 1, 7), TH_ERR_UNSUPPORTED, tot);
    {
        EnvelopePlanRequest r = req(48000, 100000, 0, 1, 7);
        r.x = CHAN + 1;
        check_refused(r, TH_ERR_INTERNAL, tot);
    }
    check_lane_refused(lane(48000, 100000, 0, INF, 16385, 5), tot);
    check_lane_refused(lane(48000, 100000, 0, INF, 7, 0), tot);
    check_lane_refused(lane(48000, 100000, 0, INF, 7, 16385), tot);
    check_lane_refused(lane(48000, 100000, 0, INF, 7, 5, 1.f, 1.f), tot);
    check_lane_refused(lane(48000, 100000, 0, INF, 7, 5, 1.f, -1.f), tot);
    check_lane_refused(lane(48000, 100000, 0, INF, 7, 5, (float)NaN, 1.f), tot);
    check_lane_refused(lane(48000, 100000, 0, INF, 7, 5, -1.f, (float)INF), tot);
    check_lane_refused(lane(48000, 100000, 0, INF, 7, 5, -1.f, 1.f, 5 * 256 + 1), tot);
    check_lane_refused(lane(48000, 100000, 3, 4, 7, 5), tot);
    std::printf("san_envelope_plan: %zu plans (%zu pieces, %zu requests walked, %zu lane parts), %zu refused, nothing reported\n", tot.plans,
                tot.pieces, tot.walked, tot.lane_parts, tot.refused);
    return 0;
}
