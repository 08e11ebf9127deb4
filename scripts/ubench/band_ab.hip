// band_ab.hip — the band-filter kernel (thesia_amd/csrc/kernels_band.hip, compiled into this program from its source) beside the
// resample kernel (kernels_resample.hip, likewise) driven with the same row at L = M = 1: the two compute the same contract
// (resample_core.h), so they give the same bits (checked on the first and the last channel).  Both are timed the same way in one
// process: hipEvents around a window of back-to-back launches that lasts 25 ms or more (as many launches as the first, discarded one
// says that takes, at most 32), the time per launch, median of the repetitions.
//   band_ab <half_taps> [seconds 30] [tracks 64] [reps 7]     (stereo tracks at 48 kHz; prints one JSON line)
// Build (scripts/bench_band.py does it when the program is missing or older than its sources), from the repository root:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize scripts/ubench/band_ab.hip \
//         -Lthesia_amd -lthesia_amd -Wl,-rpath,$PWD/thesia_amd -o scripts/ubench/band_ab
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../thesia_amd/csrc/kernels_band.hip"
#include "../../thesia_amd/csrc/kernels_resample.hip"

using namespace th;

#define HIP(call)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            std::fprintf(stderr, "%s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
            std::exit(2);                                                                      \
        }                                                                                      \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 2) return std::fprintf(stderr, "usage: band_ab half_taps [seconds] [tracks] [reps]\n"), 2;
    const uint32_t K = (uint32_t)std::atol(argv[1]), sr = 48000;
    const double seconds = argc > 2 ? std::atof(argv[2]) : 30.0;
    const uint32_t tracks = argc > 3 ? (uint32_t)std::atol(argv[3]) : 64, reps = argc > 4 ? (uint32_t)std::atol(argv[4]) : 7;
    const uint32_t n_ch = 2 * tracks;
    th_band_plan plan{};
    plan.half_taps = K;
    plan.mode = TH_BAND_PASS;
    plan.f_lo_hz = 200.0;
    plan.f_hi_hz = 8000.0;
    plan.trans_hz = 16.0 * sr / (5.0 * K);
    const uint32_t taps = 2 * K;
    std::vector<float> row(taps);
    if (th_band_coefs(sr, &plan, nullptr, row.data()) != TH_OK) return std::fprintf(stderr, "%s\n", th_last_error()), 2;
    const size_t n = (size_t)(seconds * sr), pitch = (n + 3) & ~(size_t)3;
    std::vector<float> h(pitch);
    uint32_t s = 1;
    for (float &v : h) {
        s = s * 1664525u + 1013904223u;
        v = (float)(int32_t)s * (0.9f / 2147483648.0f);
    }
    float *d_x, *d_y, *d_z, *d_row;
    HIP(hipMalloc(&d_x, pitch * n_ch * sizeof(float)));
    HIP(hipMalloc(&d_y, pitch * n_ch * sizeof(float)));
    HIP(hipMalloc(&d_z, pitch * n_ch * sizeof(float)));
    HIP(hipMalloc(&d_row, row.size() * sizeof(float)));
    HIP(hipMemcpy(d_row, row.data(), row.size() * sizeof(float), hipMemcpyHostToDevice));
    for (uint32_t c = 0; c < n_ch; c++) {  // (every channel its own memory; channel c is the noise rotated by 97 c samples)
        const size_t rot = (97 * (size_t)c) % n;
        HIP(hipMemcpy(d_x + c * pitch, h.data() + rot, (n - rot) * sizeof(float), hipMemcpyHostToDevice));
        if (rot) HIP(hipMemcpy(d_x + c * pitch + (n - rot), h.data(), rot * sizeof(float), hipMemcpyHostToDevice));
    }
    // both kernels' tables: one job per stereo track, as the export builds them
    std::vector<const float *> chan(n_ch);
    for (uint32_t c = 0; c < n_ch; c++) chan[c] = d_x + c * pitch;
    const float **d_chan;
    HIP(hipMalloc(&d_chan, n_ch * sizeof(float *)));
    HIP(hipMemcpy(d_chan, chan.data(), n_ch * sizeof(float *), hipMemcpyHostToDevice));
    const BandTiling bt = band_tiling(plan);
    th_resample_plan rp{};  // (L = M = 1: every output has row 0, windows one sample apart; the plan's limits are not the kernel's)
    rp.L = rp.M = 1;
    rp.half_taps = K;
    rp.rho = rp.cutoff = 1.0;
    const ResampleTiling rt = resample_tiling(rp);
    std::vector<BandJob> bjobs(tracks);
    std::vector<ResampleJob> rjobs(tracks);
    uint64_t bblocks = 0, rblocks = 0;
    for (uint32_t t = 0; t < tracks; t++) {
        BandJob &b = bjobs[t];
        b = BandJob{};
        b.chan = d_chan + 2 * t;
        b.dst = d_y + (size_t)2 * t * pitch;
        b.jb = b.n_in = n;
        b.ch_stride = pitch;
        b.n_ch = 2;
        b.n_tiles = (uint32_t)band_n_tiles(0, n);
        b.first_block = (uint32_t)bblocks;
        bblocks += (uint64_t)b.n_tiles * 2;
        ResampleJob &r = rjobs[t];
        r = ResampleJob{};
        r.chan = d_chan + 2 * t;
        r.dst = d_z + (size_t)2 * t * pitch;
        r.jb = r.n_in = n;
        r.ch_stride = pitch;
        r.n_ch = 2;
        r.n_sb = (uint32_t)resample_n_sb(0, n, rt);
        r.first_block = (uint32_t)rblocks;
        rblocks += (uint64_t)r.n_sb * 2 * rt.S;
    }
    if (bblocks > INT32_MAX || rblocks > INT32_MAX) return std::fprintf(stderr, "too many blocks\n"), 2;
    BandJob *d_bjobs;
    ResampleJob *d_rjobs;
    HIP(hipMalloc(&d_bjobs, bjobs.size() * sizeof(BandJob)));
    HIP(hipMalloc(&d_rjobs, rjobs.size() * sizeof(ResampleJob)));
    HIP(hipMemcpy(d_bjobs, bjobs.data(), bjobs.size() * sizeof(BandJob), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_rjobs, rjobs.data(), rjobs.size() * sizeof(ResampleJob), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    HIP(hipEventCreate(&e0));
    HIP(hipEventCreate(&e1));
    auto timed = [&](auto &&launch) {
        std::vector<float> ms;
        uint32_t inner = 1;
        for (uint32_t i = 0; i < reps + 1; i++) {
            HIP(hipEventRecord(e0, nullptr));
            for (uint32_t k = 0; k < inner; k++) launch();
            HIP(hipEventRecord(e1, nullptr));
            HIP(hipEventSynchronize(e1));
            float t = 0;
            HIP(hipEventElapsedTime(&t, e0, e1));
            if (i)
                ms.push_back(t / (float)inner);
            else  // (the first launch loads the code object; it says how many launches fill a window)
                inner = (uint32_t)std::min(32.0f, std::max(1.0f, std::ceil(25.0f / std::max(t, 0.01f))));
        }
        std::sort(ms.begin(), ms.end());
        return ms[ms.size() / 2];
    };
    const float band_ms = timed([&] { HIP(launch_band(d_bjobs, tracks, (uint32_t)bblocks, d_row, bt, nullptr)); });
    const float resample_ms = timed([&] { HIP(launch_resample(d_rjobs, tracks, (uint32_t)rblocks, d_row, rt, nullptr)); });
    HIP(hipDeviceSynchronize());
    bool same = true;
    std::vector<float> a(n), b(n);
    for (uint32_t c : {0u, n_ch - 1}) {
        HIP(hipMemcpy(a.data(), d_y + (size_t)c * pitch, n * sizeof(float), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(b.data(), d_z + (size_t)c * pitch, n * sizeof(float), hipMemcpyDeviceToHost));
        same = same && std::memcmp(a.data(), b.data(), n * sizeof(float)) == 0;
    }
    const double fma = (double)n * n_ch * taps;
    std::printf("{\"sr\": %u, \"channels\": %u, \"n\": %zu, \"taps\": %u, \"band_blocks\": %llu, \"resample_blocks\": %llu, "
                "\"resample_tile\": {\"G\": %u, \"Pt\": %u, \"R\": %u, \"span\": %u}, \"fma\": %.0f, \"band_ms\": %.4f, \"resample_kernel_ms\": %.4f, "
                "\"resample_over_band\": %.2f, \"band_Tfma_per_s\": %.3f, \"band_fraction_of_f32_peak\": %.4f, \"resample_Tfma_per_s\": %.3f, "
                "\"resample_fraction_of_f32_peak\": %.4f, \"bit_identical\": %s}\n",
                sr, n_ch, n, taps, (unsigned long long)bblocks, (unsigned long long)rblocks, rt.G, rt.Pt, rt.R, rt.span, fma, band_ms, resample_ms,
                resample_ms / band_ms, fma / band_ms / 1e9, 2.0 * fma / band_ms / 1e9 / 157.0, fma / resample_ms / 1e9,
                2.0 * fma / resample_ms / 1e9 / 157.0, same ? "true" : "false");
    return same ? 0 : 1;
}
