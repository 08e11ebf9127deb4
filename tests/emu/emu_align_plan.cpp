// emu_align_plan.cpp — plan_align (thesia_amd/csrc/align_plan.h) behind a C entry, for tests/test_align_host.py: the planner is plain
// data, so g++ compiles it beside this file and the test reads the plan as numbers.  Test scaffolding only.
#include <cstdint>
#include <vector>

#include "../../thesia_amd/csrc/align_plan.h"

using namespace th;

// out: n_pieces, scratch_doubles, rec_doubles, the tile, the group; per piece lag0, n_lags, n_tiles, n_groups, n_blocks.  Returns the
// numbers written, or -1
extern "C" __attribute__((visibility("default"))) int64_t emu_align_plan(uint64_t N, uint64_t n_lags, uint64_t *out, uint64_t cap) {
    const AlignPieces pl = plan_align(N, n_lags);
    std::vector<uint64_t> v{pl.pieces.size(), pl.scratch_doubles, pl.rec_doubles, ALIGN_TILE, ALIGN_GROUP};
    for (const AlignPiece &p : pl.pieces) v.insert(v.end(), {p.lag0, p.n_lags, p.n_tiles, p.n_groups, p.n_blocks});
    if (v.size() > cap) return -1;
    for (size_t i = 0; i < v.size(); i++) out[i] = v[i];
    return (int64_t)v.size();
}
