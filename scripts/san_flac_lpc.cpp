// san_flac_lpc.cpp — the FLAC kernels' bodies (thesia_amd/csrc/flac_block.h) and the planner (flac_plan.cpp) with the _ex entries'
// flags (TH_FLAC_LPC, TH_FLAC_STEREO) on the host under AddressSanitizer and UndefinedBehaviorSanitizer.  A stand-alone program like
// scripts/san_flac.cpp: a workgroup's threads run one after the other between the barriers, and every slot, table, staging buffer and
// track is a heap block of its exact size, so an index one past any of them is reported.  Stereo with pieces cut down to one block,
// the float path at the absolute index inside longer tracks, every flags value; every file is compared byte for byte with
// th_flac_encode_i32_ex of the same integers.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I. scripts/san_flac_lpc.cpp \
//       thesia_amd/csrc/flac_plan.cpp -Lthesia_amd -lthesia_amd -Wl,-rpath,$PWD/thesia_amd -o build/san_flac_lpc && build/san_flac_lpc
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../thesia_amd/csrc/flac_block.h"

using namespace th;

namespace {

uint64_t g_workgroups = 0, g_bytes = 0, g_files = 0, g_lpc = 0, g_side = 0;

template <class T>
std::unique_ptr<T[]> exact(size_t n) {  // (a block of exactly n elements; never n == 0 rounded up)
    return std::unique_ptr<T[]>(new T[n]);
}

uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

// sample i of channel c of a signal, as an integer of the format; channel 1 of the stereo kinds stays near channel 0
int32_t sample(int kind, uint32_t c, uint64_t i, uint32_t bps, uint32_t &rng) {
    const int32_t S = 1 << (bps - 1);
    const double two_pi = 2.0 * 3.14159265358979323846;
    switch (kind) {
        case 0: return (int32_t)std::lrint(0.4 * S * std::sin(two_pi * 1000.0 * (double)i / 48000.0)) + (c ? (int32_t)(lcg(rng) >> 30) : 0);
        case 1: return (int32_t)(3 * (int64_t)i - 1000);
        case 2: return 0;
        case 3: return (int32_t)(lcg(rng) >> (32 - bps)) - S;
        case 4: return ((i & 1) ? S - 1 : -S) * (c ? -1 : 1) - (c ? 1 : 0);  // full scale, R = -L - 1: the side channel needs bps + 1 bits
        case 5: return (int32_t)(lcg(rng) >> 28) - 8;                        // a few counts, whatever the format
        default: return (int32_t)std::lrint(0.3 * S * std::exp(-(double)(i % 3000) / 900.0) * std::sin(two_pi * 220.0 * (double)i / 48000.0) * (c ? 0.9 : 1.0)) +
                        (int32_t)(lcg(rng) >> 29) - 4;
    }
}

// one request [s0, s1) of a track of n_track samples through plan_flac / bind_flac / the kernels' bodies, pieces of piece_bytes
bool run_case(int kind, uint32_t n_ch, uint64_t n, uint64_t lead, uint32_t format, uint32_t sr, uint32_t flags, uint64_t piece_bytes) {
    const uint32_t bps = flac_bps(format);
    const double S = export_scale(format);
    const uint64_t n_track = lead + n + 3;
    uint32_t rng = 12345u + kind;
    std::vector<std::unique_ptr<float[]>> tracks;
    std::vector<std::unique_ptr<int32_t[]>> ints;
    std::vector<const float *> chan;
    std::vector<const int32_t *> ichan;
    for (uint32_t c = 0; c < n_ch; c++) {
        tracks.push_back(exact<float>(n_track));
        ints.push_back(exact<int32_t>(n ? n : 1));
        for (uint64_t i = 0; i < n_track; i++) {
            int32_t q = sample(kind, c, i, bps, rng);
            q = q < -(1 << (bps - 1)) ? -(1 << (bps - 1)) : q > (1 << (bps - 1)) - 1 ? (1 << (bps - 1)) - 1 : q;
            tracks[c][i] = (float)((double)q / S);  // (exact: at most 24 bits)
            if (i >= lead && i < lead + n) ints[c][i - lead] = q;
        }
        chan.push_back(tracks[c].get());
        ichan.push_back(ints[c].get());
    }
    // the library's stream of the same integers
    uint64_t bound = 0;
    if (th_flac_bound(n, n_ch, format, &bound) != TH_OK) return false;
    auto want = exact<uint8_t>(bound);
    size_t want_len = 0;
    if (th_flac_encode_i32_ex(ichan.data(), n_ch, n, format, sr, flags, want.get(), bound, &want_len) != TH_OK) return false;

    const FlacPlanRequest pr{n_ch, format, TH_DITHER_NONE, 0u, sr, lead, lead + n, 0, flags};
    FlacPlan pl = plan_flac(&pr, 1, piece_bytes);
    if (pl.err != 0) return false;
    auto got = exact<uint8_t>(bound);
    auto res = exact<FlacJobResult>(pl.runs.size() ? pl.runs.size() : 1);
    auto cnt = exact<unsigned long long>(2);
    auto tab_mem = exact<unsigned char>(pl.tab_bytes ? pl.tab_bytes : 1);
    uint64_t at = FLAC_STREAM_HEADER;
    uint32_t mn = 0xffffffffu, mx = 0;
    const uint32_t upb = flac_units_per_block(n_ch, flags);
    for (size_t pi = 0; pi < pl.pieces.size(); pi++) {
        const FlacPiece &pc = pl.pieces[pi];
        auto stage = exact<uint8_t>(pc.bound);
        auto slots = exact<uint32_t>(pc.slot_words);
        auto bits = exact<uint32_t>(pc.n_units);
        auto foff = exact<uint32_t>(pc.n_blocks);
        const std::vector<unsigned char> tab =
            bind_flac(pl, FlacBases{{stage.get(), stage.get()}, slots.get(), bits.get(), foff.get(), res.get(), tab_mem.get(), cnt.get()}, &pr, 1, chan.data());
        std::memcpy(tab_mem.get(), tab.data(), tab.size());  // (the jobs read their channel pointers from the table)
        for (size_t k = pc.run0; k < pc.run1; k++) {
            unsigned long long counts[2] = {0, 0};
            flac_run_job_host(pl.jobs[k], nullptr, counts);
            if (counts[0] || counts[1]) return false;
            if (res[k].bytes > pl.runs[k].bound || at + res[k].bytes > bound) return false;
            std::memcpy(got.get() + at, pl.jobs[k].dst, res[k].bytes);
            // what was chosen: a subframe's first byte is its type, byte 3 of a frame holds the assignment
            for (uint32_t u = 0; u < pl.jobs[k].nb * upb; u++) g_lpc += (pl.jobs[k].slots[(uint64_t)u * pl.jobs[k].slot_words] >> 30) == 1u;
            for (uint32_t f = 0; f < pl.jobs[k].nb; f++) g_side += (pl.jobs[k].dst[pl.jobs[k].foff[f] + 3] >> 4) >= 8u;
            at += res[k].bytes;
            mn = res[k].min_frame < mn ? res[k].min_frame : mn;
            mx = res[k].max_frame > mx ? res[k].max_frame : mx;
            g_workgroups += (uint64_t)pl.jobs[k].nb * (upb + 1) + 1;
        }
    }
    flac_stream_header(sr, n_ch, bps, n, mx ? mn : 0u, mx, got.get());
    g_bytes += at;
    g_files++;
    if (at != want_len || std::memcmp(got.get(), want.get(), at) != 0) {
        std::fprintf(stderr, "san_flac_lpc: kind %d, %u channels, %llu samples from %llu, %u bit, flags %u: the file differs from th_flac_encode_i32_ex's\n",
                     kind, n_ch, (unsigned long long)n, (unsigned long long)lead, bps, flags);
        return false;
    }
    return true;
}

}  // namespace

int main() {
    const uint64_t lengths[] = {0, 1, 4, 5, 9, 33, 64, 320, 4095, 4096, 4097, 8192 + 17};
    bool ok = true;
    for (uint32_t format : {(uint32_t)TH_PCM_S16, (uint32_t)TH_PCM_S24}) {
        for (uint32_t flags = 0; flags <= 3; flags++) {
            for (int kind = 0; kind < 7; kind++) ok = ok && run_case(kind, 2, 4096 + 257, 1, format, 48000, flags, 1);  // stereo, every block its own piece
            for (uint64_t n : lengths) ok = ok && run_case(6, 2, n, 3, format, 44100, flags, 1);
            for (uint32_t c : {1u, 3u, 8u}) ok = ok && run_case((int)(c % 7), c, 4097, 2049, format, 12345, flags, 30000);
            ok = ok && run_case(0, 2, 3 * 4096 + 9, 7, format, 200000, flags, TH_EXPORT_PIECE_BYTES);
        }
    }
    ok = ok && g_lpc > 0 && g_side > 0;  // (both tools were taken somewhere)
    std::printf("san_flac_lpc: %s: %llu files, %llu workgroups, %llu bytes, %llu LPC subframes, %llu frames with a side channel\n", ok ? "ok" : "FAILED",
                (unsigned long long)g_files, (unsigned long long)g_workgroups, (unsigned long long)g_bytes, (unsigned long long)g_lpc,
                (unsigned long long)g_side);
    return ok ? 0 : 1;
}
