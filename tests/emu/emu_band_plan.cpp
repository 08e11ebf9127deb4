// emu_band_plan.cpp — plan_export and bind_export (thesia_amd/csrc/reader_plan.h) on requests that carry a band filter, for
// tests/test_band_plan_host.py, which compiles this file with g++ beside reader_plan.cpp and host_math.cpp (no GPU, no HIP header).
#include <cstdint>
#include <vector>

#include "../../thesia_amd/csrc/reader_plan.h"

using namespace th;

// rows of 10 per request: {n_ch, n_in, sr, format, dither, seed, s0, s1, offset, pad}; bands of 4 per request: {half_taps, mode,
// f_lo_hz, f_hi_hz} (half_taps 0: no filter).  bases: {stage 0, stage 1, scratch, table, counters} as addresses; request i's channel c
// lies at chan0 + 0x100000 (its index in request order).  Writes u64 values to out (at most cap) and returns how many, or -1:
//   {err, n_jobs, n_rjobs, n_bjobs, n_pieces, o_rjobs, o_bjobs, o_ptrs, tab_bytes, scratch_need, n_ptrs, table length}
//   per request {ptr0}
//   per job {request, f0, f1, n, first_chunk, stage_at, filtered, hull0, stride, scratch_at, ptr_at, chan, dst}
//   per band job {ja, jb, n_in, ch_stride, n_ch, n_tiles, first_block, chan, dst}
//   per piece {job0, job1, bjob0, bjob1, n_bblocks, band half_taps, band_sr, scratch_floats, n_chunks, runs}
//   the pointer table, n_ptrs entries
extern "C" __attribute__((visibility("default"))) int64_t emu_band_plan(const uint64_t *rows, const double *bands, uint64_t n,
                                                                        const uint64_t *bases, uint64_t chan0, uint64_t *out, uint64_t cap) {
    std::vector<ExportPlanRequest> reqs(n);
    std::vector<const float *> chan;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *r = rows + 10 * i;
        ExportPlanRequest &q = reqs[i];
        q = ExportPlanRequest{};
        q.n_ch = (uint32_t)r[0];
        q.n_in = q.n_out = r[1];
        q.sr_in = q.sr_out = (uint32_t)r[2];
        q.format = (uint32_t)r[3];
        q.dither = (uint32_t)r[4];
        q.seed = (uint32_t)r[5];
        q.s0 = r[6];
        q.s1 = r[7];
        q.offset = r[8];
        q.pad = (uint32_t)r[9];
        q.band.half_taps = (uint32_t)bands[4 * i];
        q.band.mode = (uint32_t)bands[4 * i + 1];
        q.band.f_lo_hz = bands[4 * i + 2];
        q.band.f_hi_hz = bands[4 * i + 3];
        for (uint32_t c = 0; c < q.n_ch; c++) chan.push_back(reinterpret_cast<const float *>((uintptr_t)(chan0 + 0x100000ull * chan.size())));
    }
    ExportPlan p = plan_export(reqs.data(), n);
    std::vector<uint64_t> v;
    if (p.err != TH_OK) {
        v = {(uint64_t)(int64_t)p.err};
    } else {
        const ExportBases b{{reinterpret_cast<uint8_t *>((uintptr_t)bases[0]), reinterpret_cast<uint8_t *>((uintptr_t)bases[1])},
                            reinterpret_cast<float *>((uintptr_t)bases[2]), reinterpret_cast<unsigned char *>((uintptr_t)bases[3]),
                            reinterpret_cast<unsigned long long *>((uintptr_t)bases[4])};
        const std::vector<unsigned char> tab = bind_export(p, b, chan.data());
        v = {0, p.jobs.size(), p.rjobs.size(), p.bjobs.size(), p.pieces.size(), p.o_rjobs, p.o_bjobs, p.o_ptrs, p.tab_bytes, p.scratch_need,
             p.n_ptrs, tab.size()};
        for (size_t i = 0; i < n; i++) v.push_back(p.ptr0[i]);
        for (size_t j = 0; j < p.jobs.size(); j++) {
            const ExportJob &x = p.jobs[j];
            const ExportPlace &pl = p.places[j];
            v.insert(v.end(), {pl.req, x.f0, x.f1, x.n, x.first_chunk, pl.stage_at, pl.filtered, pl.hull0, pl.stride, pl.scratch_at, pl.ptr_at,
                               (uint64_t)(uintptr_t)x.chan, (uint64_t)(uintptr_t)x.dst});
        }
        for (const BandJob &x : p.bjobs)
            v.insert(v.end(), {x.ja, x.jb, x.n_in, x.ch_stride, x.n_ch, x.n_tiles, x.first_block, (uint64_t)(uintptr_t)x.chan, (uint64_t)(uintptr_t)x.dst});
        for (const ExportPiece &x : p.pieces)
            v.insert(v.end(), {x.job0, x.job1, x.bjob0, x.bjob1, x.n_bblocks, x.band.half_taps, x.band_sr, x.scratch_floats, x.n_chunks, x.runs.size()});
        const uint64_t *ptrs = reinterpret_cast<const uint64_t *>(tab.data() + p.o_ptrs);
        v.insert(v.end(), ptrs, ptrs + p.n_ptrs);
    }
    if (v.size() > cap) return -1;
    for (size_t i = 0; i < v.size(); i++) out[i] = v[i];
    return (int64_t)v.size();
}
