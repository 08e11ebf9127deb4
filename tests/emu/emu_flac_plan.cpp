// emu_flac_plan.cpp — plan_flac / bind_flac (thesia_amd/csrc/flac_plan.h) behind a C entry, for tests/test_flac_plan_host.py: the
// planner is plain data, so g++ compiles it beside this file and the test reads the plan as numbers.  Test scaffolding only.
#include <cstdint>
#include <vector>

#include "../../thesia_amd/csrc/flac_plan.h"

using namespace th;

// rows: per request n_ch, format, dither, seed, sr, s0, s1, offset.  bases: stage 0, stage 1, slots, bits, foff, res, table, counters.
// out: err, n_pieces, n_runs, stage_need[0], stage_need[1], slot_need, unit_need, block_need, o_ptrs, tab_bytes; per piece run0, run1,
// n_units, n_blocks, bound, slot_words; per run req, b0, nb, first_unit, first_block, slot_words, slot_at, stage_at, bound, and of its
// job chan, slots, bits, foff, dst, cnt, res, s0, s1, b0, nb, n_ch, format, dither, seed, sr.  Returns the numbers written, or -1
extern "C" __attribute__((visibility("default"))) int64_t emu_flac_plan(const uint64_t *rows, uint64_t n, uint64_t piece_bytes, const uint64_t *bases,
                                                                        uint64_t *out, uint64_t cap) {
    std::vector<FlacPlanRequest> reqs(n);
    std::vector<const float *> chan;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *r = rows + 8 * i;
        reqs[i] = FlacPlanRequest{(uint32_t)r[0], (uint32_t)r[1], (uint32_t)r[2], (uint32_t)r[3], (uint32_t)r[4], r[5], r[6], r[7]};
        for (uint32_t c = 0; c < reqs[i].n_ch; c++) chan.push_back(reinterpret_cast<const float *>(0x1000 * (i + 1) + c));
    }
    FlacPlan pl = plan_flac(reqs.data(), n, piece_bytes);
    std::vector<uint64_t> v{(uint64_t)(int64_t)pl.err};
    if (pl.err == 0) {
        const FlacBases b{{reinterpret_cast<uint8_t *>(bases[0]), reinterpret_cast<uint8_t *>(bases[1])},
                          reinterpret_cast<uint32_t *>(bases[2]),
                          reinterpret_cast<uint32_t *>(bases[3]),
                          reinterpret_cast<uint32_t *>(bases[4]),
                          reinterpret_cast<FlacJobResult *>(bases[5]),
                          reinterpret_cast<unsigned char *>(bases[6]),
                          reinterpret_cast<unsigned long long *>(bases[7])};
        const std::vector<unsigned char> tab = bind_flac(pl, b, reqs.data(), n, chan.data());
        if (tab.size() != pl.tab_bytes) return -1;
        v.insert(v.end(), {pl.pieces.size(), pl.runs.size(), pl.stage_need[0], pl.stage_need[1], pl.slot_need, pl.unit_need, pl.block_need,
                           pl.o_ptrs, pl.tab_bytes});
        for (const FlacPiece &p : pl.pieces) v.insert(v.end(), {p.run0, p.run1, p.n_units, p.n_blocks, p.bound, p.slot_words});
        for (size_t k = 0; k < pl.runs.size(); k++) {
            const FlacRun &r = pl.runs[k];
            const FlacJob &j = pl.jobs[k];
            v.insert(v.end(), {r.req, r.b0, r.nb, r.first_unit, r.first_block, r.slot_words, r.slot_at, r.stage_at, r.bound,
                               (uint64_t)(uintptr_t)j.chan, (uint64_t)(uintptr_t)j.slots, (uint64_t)(uintptr_t)j.bits, (uint64_t)(uintptr_t)j.foff,
                               (uint64_t)(uintptr_t)j.dst, (uint64_t)(uintptr_t)j.cnt, (uint64_t)(uintptr_t)j.res, j.s0, j.s1, j.b0, j.nb, j.n_ch,
                               j.format, j.dither, j.seed, j.sr});
        }
        // the channel pointers behind the jobs, as the table carries them
        const uint64_t *ptrs = reinterpret_cast<const uint64_t *>(tab.data() + pl.o_ptrs);
        for (size_t i = 0; i < chan.size(); i++) v.push_back(ptrs[i]);
    }
    if (v.size() > cap) return -1;
    for (size_t i = 0; i < v.size(); i++) out[i] = v[i];
    return (int64_t)v.size();
}
