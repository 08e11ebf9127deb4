// align_time.hip — the correlation kernel of th_tm_align_tracks (with its fold over the groups) timed by hipEvents, compiled from the
// product's source, on the pieces the reader itself makes (plan_align) for a reference range of S seconds at 48 kHz searched over
// +-D seconds.  A child process of scripts/bench_align.py; prints one JSON line per D.  From the repository root (one line):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 scripts/ubench/align_time.hip thesia_amd/csrc/align_plan.cpp
//         thesia_amd/csrc/host_math.cpp -o scripts/ubench/align_time
// Usage: align_time [seconds 30] [reps 5] [max lag in seconds ...  0.1 1]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../thesia_amd/csrc/kernels_align.hip"

using namespace th;

#define HIP(call)                                                                  \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) {                                                    \
            std::fprintf(stderr, "%s failed: %s\n", #call, hipGetErrorString(e_)); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

int main(int argc, char **argv) {
    const double seconds = argc > 1 ? std::atof(argv[1]) : 30.0;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 5;
    std::vector<double> lags;
    for (int i = 3; i < argc; i++) lags.push_back(std::atof(argv[i]));
    if (lags.empty()) lags = {0.1, 1.0};
    const uint32_t sr = 48000;
    const uint64_t N = (uint64_t)(seconds * sr);
    if (N == 0 || N > TH_ALIGN_MAX_REF) {
        std::fprintf(stderr, "%g s: 1 .. %u samples\n", seconds, TH_ALIGN_MAX_REF);
        return 2;
    }
    // the probe: the reference 1234 samples late at half the level, with a margin on either side (random data: the clock under load)
    const uint64_t n_b = N + 2 * sr;
    std::vector<float> ref(N), probe(n_b, 0.0f);
    uint32_t seed = 12345u;
    for (float &v : ref) {
        seed = seed * 1664525u + 1013904223u;
        v = (float)(int32_t)seed * (1.0f / 2147483648.0f);
    }
    for (uint64_t k = 0; k < N; k++) probe[k + 1234] = 0.5f * ref[k];
    float *d_ref = nullptr, *d_probe = nullptr;
    double *d_scratch = nullptr, *d_rec = nullptr;
    HIP(hipMalloc(&d_ref, N * sizeof(float)));
    HIP(hipMalloc(&d_probe, n_b * sizeof(float)));
    HIP(hipMalloc(&d_scratch, (size_t)ALIGN_GROUP_BLOCKS * TH_ALIGN_PIECE_LAGS * sizeof(double)));
    HIP(hipMalloc(&d_rec, (size_t)TH_ALIGN_PIECE_LAGS * sizeof(double)));
    HIP(hipMemcpy(d_ref, ref.data(), N * sizeof(float), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_probe, probe.data(), n_b * sizeof(float), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    HIP(hipEventCreate(&e0));
    HIP(hipEventCreate(&e1));
    for (double max_lag : lags) {
        const uint32_t D = (uint32_t)(max_lag * sr + 0.5);
        const uint64_t n_lags = 2 * (uint64_t)D + 1;
        if (D > TH_ALIGN_MAX_LAG || N * n_lags > TH_ALIGN_MAX_WORK) {
            std::fprintf(stderr, "%g s of lag: beyond the reader's limits\n", max_lag);
            return 2;
        }
        const AlignPieces ap = plan_align(N, n_lags);
        std::vector<float> ms;
        uint32_t blocks = 0;
        double peak_at = 0.0;
        for (int rep = 0; rep < reps + 1; rep++) {  // (the first one warms up)
            blocks = 0;
            HIP(hipEventRecord(e0, nullptr));
            for (const AlignPiece &pc : ap.pieces) {
                AlignJob job{};
                job.a = d_ref;
                job.b = d_probe;
                job.scratch = d_scratch;
                job.N = N;
                job.n_b = n_b;
                job.first = -(int64_t)D + (int64_t)pc.lag0;
                job.n_lags = pc.n_lags;
                job.n_tiles = pc.n_tiles;
                job.n_groups = pc.n_groups;
                HIP(launch_align_xcorr(job, d_rec, nullptr));
                blocks += pc.n_blocks;
            }
            HIP(hipEventRecord(e1, nullptr));
            HIP(hipEventSynchronize(e1));
            float t = 0.0f;
            HIP(hipEventElapsedTime(&t, e0, e1));
            if (rep) ms.push_back(t);
        }
        {  // the last piece's curve: where its largest value lies (D >= 1234: lag 1234 when that piece holds it)
            const AlignPiece &pc = ap.pieces.back();
            std::vector<double> rec(pc.n_lags);
            HIP(hipMemcpy(rec.data(), d_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
            peak_at = (double)(std::max_element(rec.begin(), rec.end()) - rec.begin()) + (double)pc.lag0 - (double)D;
        }
        std::sort(ms.begin(), ms.end());
        const double med = ms[ms.size() / 2], fma = (double)N * (double)n_lags;
        std::printf("{\"seconds\": %g, \"max_lag_sec\": %g, \"N\": %llu, \"n_lags\": %llu, \"pieces\": %zu, \"workgroups\": %u, \"kernel_ms\": %.3f, "
                    "\"kernel_min_ms\": %.3f, \"tfma_per_s\": %.2f, \"of_f64_vector_peak_39_3\": %.3f, \"last_piece_peak_lag\": %.0f}\n",
                    seconds, max_lag, (unsigned long long)N, (unsigned long long)n_lags, ap.pieces.size(), blocks, med, (double)ms.front(),
                    fma / (med * 1e-3) / 1e12, fma / (med * 1e-3) / 1e12 / 39.3, peak_at);
    }
    HIP(hipFree(d_ref));
    HIP(hipFree(d_probe));
    HIP(hipFree(d_scratch));
    HIP(hipFree(d_rec));
    return 0;
}
