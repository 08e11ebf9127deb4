// emu_flac_lpc_plan.cpp — plan_flac / bind_flac (thesia_amd/csrc/flac_plan.h) with the _ex entries' flags behind a C entry, for
// tests/test_flac_lpc_plan_host.py (emu_flac_plan.cpp is the flags == 0 one and stays as it is).  Test scaffolding only.
#include <cstdint>
#include <vector>

#include "../../thesia_amd/csrc/flac_plan.h"

using namespace th;

// rows: per request n_ch, format, s0, s1, offset, flags.  out: err, n_pieces, n_runs, stage_need[0], stage_need[1], slot_need,
// unit_need, block_need; per piece run0, run1, n_units, n_blocks, bound, slot_words; per run req, b0, nb, first_unit, first_block,
// slot_words, slot_at, stage_at, bound, and of its job slots, bits, foff (as offsets from their bases, in elements), flags.
// Returns the numbers written, or -1
extern "C" __attribute__((visibility("default"))) int64_t emu_flac_lpc_plan(const uint64_t *rows, uint64_t n, uint64_t piece_bytes, uint64_t *out,
                                                                            uint64_t cap) {
    std::vector<FlacPlanRequest> reqs(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *r = rows + 6 * i;
        reqs[i] = FlacPlanRequest{(uint32_t)r[0], (uint32_t)r[1], 0u, 0u, 48000u, r[2], r[3], r[4], (uint32_t)r[5]};
    }
    FlacPlan pl = plan_flac(reqs.data(), n, piece_bytes);
    std::vector<uint64_t> v{(uint64_t)(int64_t)pl.err};
    if (pl.err == 0) {
        uint32_t *const slots = reinterpret_cast<uint32_t *>(0x10000000), *const bits = reinterpret_cast<uint32_t *>(0x20000000),
                        *const foff = reinterpret_cast<uint32_t *>(0x30000000);
        const FlacBases b{{reinterpret_cast<uint8_t *>(0x40000000), reinterpret_cast<uint8_t *>(0x50000000)}, slots, bits, foff,
                          reinterpret_cast<FlacJobResult *>(0x60000000), reinterpret_cast<unsigned char *>(0x70000000),
                          reinterpret_cast<unsigned long long *>(0x80000000)};
        bind_flac(pl, b, reqs.data(), n, nullptr);
        v.insert(v.end(), {pl.pieces.size(), pl.runs.size(), pl.stage_need[0], pl.stage_need[1], pl.slot_need, pl.unit_need, pl.block_need});
        for (const FlacPiece &p : pl.pieces) v.insert(v.end(), {p.run0, p.run1, p.n_units, p.n_blocks, p.bound, p.slot_words});
        for (size_t k = 0; k < pl.runs.size(); k++) {
            const FlacRun &r = pl.runs[k];
            const FlacJob &j = pl.jobs[k];
            v.insert(v.end(), {r.req, r.b0, r.nb, r.first_unit, r.first_block, r.slot_words, r.slot_at, r.stage_at, r.bound, (uint64_t)(j.slots - slots),
                               (uint64_t)(j.bits - bits), (uint64_t)(j.foff - foff), j.flags});
        }
    }
    if (v.size() > cap) return -1;
    for (size_t i = 0; i < v.size(); i++) out[i] = v[i];
    return (int64_t)v.size();
}
