// flac_plan.cpp — see flac_plan.h.  Host only, plain C++.
#include "flac_plan.h"

#include <algorithm>
#include <cstring>

#include "flac_core.h"

namespace th {

FlacPlan plan_flac(const FlacPlanRequest *reqs, size_t n, uint64_t piece_bytes) {
    FlacPlan pl;
    pl.chan0.resize(n);
    size_t n_ptrs = 0;
    FlacPiece cur;
    auto close = [&]() {
        if (cur.run1 == cur.run0) return;
        const size_t p = pl.pieces.size();
        pl.stage_need[p & 1] = std::max(pl.stage_need[p & 1], cur.bound);
        pl.slot_need = std::max(pl.slot_need, cur.slot_words);
        pl.unit_need = std::max(pl.unit_need, cur.n_units);
        pl.block_need = std::max(pl.block_need, cur.n_blocks);
        pl.pieces.push_back(cur);
        cur = FlacPiece{};
        cur.run0 = cur.run1 = pl.runs.size();
    };
    for (size_t i = 0; i < n; i++) {
        const FlacPlanRequest &r = reqs[i];
        pl.chan0[i] = n_ptrs;
        n_ptrs += r.n_ch;
        if (r.n_ch == 0 || r.n_ch > FLAC_MAX_CHANNELS || r.s1 < r.s0 || (r.flags & ~FLAC_FLAGS)) {
            pl.err = TH_ERR_INTERNAL;
            pl.err_text = "a FLAC request reached the planner unchecked";
            return pl;
        }
        const uint32_t bps = flac_bps(r.format);
        // units of a block, and the sample size that sizes their slots: a stereo block's four are all as wide as its side channel
        const uint32_t upb = flac_units_per_block(r.n_ch, r.flags), slot_bps = upb == r.n_ch ? bps : bps + 1u;
        const uint64_t len = r.s1 - r.s0, n_full = len / FLAC_BLOCK;
        const uint32_t rest = (uint32_t)(len % FLAC_BLOCK);
        const uint64_t n_blk = n_full + (rest ? 1 : 0), fb = flac_frame_bound(FLAC_BLOCK, r.n_ch, bps);
        uint64_t b = 0;
        while (b < n_blk) {
            const uint64_t room = piece_bytes > cur.bound ? piece_bytes - cur.bound : 0;
            const uint64_t units = (FLAC_PIECE_MAX_UNITS - cur.n_units) / upb;
            uint64_t full = b < n_full ? std::min({n_full - b, room / fb, units}) : 0;
            uint64_t bound = full * fb;
            uint32_t tail = 0;  // the request's short last block, when it comes next and fits
            if (b + full == n_full && rest && full < units && bound + flac_frame_bound(rest, r.n_ch, bps) <= room) tail = rest;
            if (full == 0 && tail == 0) {
                if (cur.run1 != cur.run0) {
                    close();
                    continue;
                }
                // an empty piece takes one block whatever its size
                if (b < n_full) full = 1, bound = fb;
                else tail = rest;
            }
            // the whole blocks and the short one are runs of their own: a run's slots are all of one size, that of its blocks
            auto push = [&](uint64_t b0, uint32_t nb, uint32_t n_block, uint64_t run_bound) {
                FlacRun run{};
                run.req = i;
                run.b0 = b0;
                run.nb = nb;
                run.first_unit = cur.n_units;
                run.first_block = cur.n_blocks;
                run.slot_words = flac_slot_words(n_block, slot_bps);
                run.slot_at = cur.slot_words;
                run.stage_at = cur.bound;
                run.bound = run_bound;
                pl.runs.push_back(run);
                cur.run1 = pl.runs.size();
                cur.n_units += nb * upb;
                cur.n_blocks += nb;
                cur.slot_words += (uint64_t)nb * upb * run.slot_words;
                cur.bound += run_bound;
            };
            if (full) push(b, (uint32_t)full, FLAC_BLOCK, bound);
            if (tail) push(b + full, 1u, tail, flac_frame_bound(tail, r.n_ch, bps));
            b += full + (tail ? 1 : 0);
        }
    }
    close();
    pl.o_ptrs = pl.runs.size() * sizeof(FlacJob);
    pl.tab_bytes = pl.o_ptrs + n_ptrs * sizeof(const float *);
    return pl;
}

std::vector<unsigned char> bind_flac(FlacPlan &p, const FlacBases &b, const FlacPlanRequest *reqs, size_t n, const float *const *chan) {
    p.jobs.assign(p.runs.size(), FlacJob{});
    for (size_t pi = 0; pi < p.pieces.size(); pi++) {
        for (size_t k = p.pieces[pi].run0; k < p.pieces[pi].run1; k++) {
            const FlacRun &run = p.runs[k];
            const FlacPlanRequest &r = reqs[run.req];
            FlacJob &j = p.jobs[k];
            j.chan = reinterpret_cast<const float *const *>(b.tab + p.o_ptrs) + p.chan0[run.req];
            j.slots = b.slots + run.slot_at;
            j.bits = b.bits + run.first_unit;
            j.foff = b.foff + run.first_block;
            j.dst = b.stage[pi & 1] + run.stage_at;
            j.cnt = b.cnt + 2 * run.req;
            j.res = b.res + k;
            j.s0 = r.s0;
            j.s1 = r.s1;
            j.b0 = run.b0;
            j.nb = run.nb;
            j.first_unit = run.first_unit;
            j.first_block = run.first_block;
            j.n_ch = r.n_ch;
            j.format = r.format;
            j.dither = r.dither;
            j.seed = r.seed;
            j.sr = r.sr;
            j.slot_words = run.slot_words;
            j.flags = r.flags;
        }
    }
    size_t n_ptrs = 0;
    for (size_t i = 0; i < n; i++) n_ptrs += reqs[i].n_ch;
    std::vector<unsigned char> tab(p.tab_bytes);
    if (!p.jobs.empty()) std::memcpy(tab.data(), p.jobs.data(), p.jobs.size() * sizeof(FlacJob));
    if (n_ptrs && chan) std::memcpy(tab.data() + p.o_ptrs, chan, n_ptrs * sizeof(const float *));
    return tab;
}

}  // namespace th
