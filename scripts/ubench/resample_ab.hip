// resample_ab.hip — the tiled resample kernel (thesia_amd/csrc/kernels_resample.hip, compiled into this program from its source)
// beside the NAIVE form of the same contract: one thread per output sample, its 2K coefficients read from the table and its 2K
// samples from global memory, the same summation (resample_core.h), so the two give the same bits (checked on the first and the
// last channel).  Both are timed the same way in one process: hipEvents around each launch, median of the repetitions.
//   resample_ab <sr_in> <sr_out> [seconds 30] [tracks 64] [reps 5]     (stereo tracks; prints one JSON line)
// Build (scripts/bench_resample.py does it when the program is missing or older than its sources), from the repository root:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize scripts/ubench/resample_ab.hip \
//         -Lthesia_amd -lthesia_amd -Wl,-rpath,$PWD/thesia_amd -o scripts/ubench/resample_ab
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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

// one thread per output of one channel: blockIdx.y = channel
__global__ __launch_bounds__(256) void resample_naive(const float *__restrict__ x, size_t ch_pitch_in, uint64_t n_in, float *__restrict__ y,
                                                      size_t ch_pitch_out, uint64_t n_out, const float *__restrict__ table, uint32_t L, uint32_t M,
                                                      uint32_t taps) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    const float *src = x + (size_t)blockIdx.y * ch_pitch_in;
    uint64_t q;
    uint32_t r;
    resample_phase(j, L, M, &q, &r);
    const float *c = table + (uint64_t)r * taps;
    const int64_t first = (int64_t)q - (int64_t)(taps / 2) + 1;
    auto at = [&](uint32_t k) {
        const int64_t i = first + (int64_t)k;
        return (i >= 0 && (uint64_t)i < n_in) ? src[i] : 0.0f;
    };
    ResampleAcc acc;
    uint32_t k = 0;
    for (; k + 4 <= taps; k += 4) resample_tap4(acc, c[k], c[k + 1], c[k + 2], c[k + 3], at(k), at(k + 1), at(k + 2), at(k + 3));
    if (k < taps) resample_tap2(acc, c[k], c[k + 1], at(k), at(k + 1));
    y[(size_t)blockIdx.y * ch_pitch_out + j] = resample_fold(acc);
}

int main(int argc, char **argv) {
    if (argc < 3) return std::fprintf(stderr, "usage: resample_ab sr_in sr_out [seconds] [tracks] [reps]\n"), 2;
    const uint32_t sr_in = (uint32_t)std::atol(argv[1]), sr_out = (uint32_t)std::atol(argv[2]);
    const double seconds = argc > 3 ? std::atof(argv[3]) : 30.0;
    const uint32_t tracks = argc > 4 ? (uint32_t)std::atol(argv[4]) : 64, reps = argc > 5 ? (uint32_t)std::atol(argv[5]) : 5;
    const uint32_t n_ch = 2 * tracks;
    th_resample_plan plan;
    if (th_resample_plan_for(sr_in, sr_out, &plan) != TH_OK) return std::fprintf(stderr, "%s\n", th_last_error()), 2;
    const size_t n_in = (size_t)(seconds * sr_in);
    size_t n_out = 0;
    th_resample_n_out(n_in, sr_in, sr_out, &n_out);
    const ResampleTiling tl = resample_tiling(plan);
    std::vector<float> table((size_t)plan.L * tl.taps);
    for (uint32_t r = 0; r < plan.L; r++) th_resample_coefs(sr_in, sr_out, r, nullptr, table.data() + (size_t)r * tl.taps);
    const size_t pin = (n_in + 3) & ~(size_t)3, pout = (n_out + 3) & ~(size_t)3;
    std::vector<float> h(pin);
    uint32_t s = 1;
    for (float &v : h) {
        s = s * 1664525u + 1013904223u;
        v = (float)(int32_t)s * (0.9f / 2147483648.0f);
    }
    float *d_x, *d_y, *d_z, *d_tab;
    HIP(hipMalloc(&d_x, pin * n_ch * sizeof(float)));
    HIP(hipMalloc(&d_y, pout * n_ch * sizeof(float)));
    HIP(hipMalloc(&d_z, pout * n_ch * sizeof(float)));
    HIP(hipMalloc(&d_tab, table.size() * sizeof(float)));
    HIP(hipMemcpy(d_tab, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    for (uint32_t c = 0; c < n_ch; c++) {  // (every channel its own memory; channel c is the noise rotated by 97 c samples)
        const size_t rot = (97 * (size_t)c) % n_in;
        HIP(hipMemcpy(d_x + c * pin, h.data() + rot, (n_in - rot) * sizeof(float), hipMemcpyHostToDevice));
        if (rot) HIP(hipMemcpy(d_x + c * pin + (n_in - rot), h.data(), rot * sizeof(float), hipMemcpyHostToDevice));
    }
    // the tiled kernel's tables: one job per stereo track, as the export builds them
    std::vector<const float *> chan(n_ch);
    for (uint32_t c = 0; c < n_ch; c++) chan[c] = d_x + c * pin;
    const float **d_chan;
    HIP(hipMalloc(&d_chan, n_ch * sizeof(float *)));
    HIP(hipMemcpy(d_chan, chan.data(), n_ch * sizeof(float *), hipMemcpyHostToDevice));
    std::vector<ResampleJob> jobs(tracks);
    uint64_t blocks = 0;
    for (uint32_t t = 0; t < tracks; t++) {
        ResampleJob &j = jobs[t];
        j = ResampleJob{};
        j.chan = d_chan + 2 * t;
        j.dst = d_y + (size_t)2 * t * pout;
        j.ja = 0;
        j.jb = n_out;
        j.n_in = n_in;
        j.ch_stride = pout;
        j.n_ch = 2;
        j.n_sb = (uint32_t)resample_n_sb(0, n_out, tl);
        j.first_block = (uint32_t)blocks;
        blocks += (uint64_t)j.n_sb * 2 * tl.S;
    }
    if (blocks > INT32_MAX) return std::fprintf(stderr, "too many blocks\n"), 2;
    ResampleJob *d_jobs;
    HIP(hipMalloc(&d_jobs, jobs.size() * sizeof(ResampleJob)));
    HIP(hipMemcpy(d_jobs, jobs.data(), jobs.size() * sizeof(ResampleJob), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    HIP(hipEventCreate(&e0));
    HIP(hipEventCreate(&e1));
    auto timed = [&](auto &&launch) {
        std::vector<float> ms;
        for (uint32_t i = 0; i < reps + 1; i++) {
            HIP(hipEventRecord(e0, nullptr));
            launch();
            HIP(hipEventRecord(e1, nullptr));
            HIP(hipEventSynchronize(e1));
            float t = 0;
            HIP(hipEventElapsedTime(&t, e0, e1));
            if (i) ms.push_back(t);  // (the first launch loads the code object)
        }
        std::sort(ms.begin(), ms.end());
        return ms[ms.size() / 2];
    };
    const float tiled_ms = timed([&] { HIP(launch_resample(d_jobs, tracks, (uint32_t)blocks, d_tab, tl, nullptr)); });
    const float naive_ms = timed([&] {
        hipLaunchKernelGGL(resample_naive, dim3((uint32_t)((n_out + 255) / 256), n_ch), dim3(256), 0, nullptr, d_x, pin, (uint64_t)n_in, d_z, pout,
                           (uint64_t)n_out, d_tab, plan.L, plan.M, tl.taps);
        HIP(hipGetLastError());
    });
    HIP(hipDeviceSynchronize());
    bool same = true;
    std::vector<float> a(n_out), b(n_out);
    for (uint32_t c : {0u, n_ch - 1}) {
        HIP(hipMemcpy(a.data(), d_y + (size_t)c * pout, n_out * sizeof(float), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(b.data(), d_z + (size_t)c * pout, n_out * sizeof(float), hipMemcpyDeviceToHost));
        same = same && std::memcmp(a.data(), b.data(), n_out * sizeof(float)) == 0;
    }
    const double fma = (double)n_out * n_ch * tl.taps;
    const double bytes = ((double)n_in + (double)n_out) * n_ch * 4.0;  // the algorithmic ones: every input read once, every output written once
    std::printf("{\"sr_in\": %u, \"sr_out\": %u, \"channels\": %u, \"n_in\": %zu, \"n_out\": %zu, \"taps\": %u, \"L\": %u, \"M\": %u, "
                "\"tile\": {\"G\": %u, \"Pt\": %u, \"R\": %u, \"S\": %u, \"span\": %u}, \"blocks\": %llu, \"fma\": %.0f, \"bytes\": %.0f, "
                "\"tiled_ms\": %.4f, \"naive_ms\": %.4f, \"naive_over_tiled\": %.2f, \"tiled_Tfma_per_s\": %.3f, \"tiled_fraction_of_f32_peak\": %.4f, "
                "\"tiled_TBps\": %.3f, \"roofline_ms_at_8TBps\": %.4f, \"bit_identical\": %s}\n",
                sr_in, sr_out, n_ch, n_in, n_out, tl.taps, plan.L, plan.M, tl.G, tl.Pt, tl.R, tl.S, tl.span, (unsigned long long)blocks, fma, bytes,
                tiled_ms, naive_ms, naive_ms / tiled_ms, fma / tiled_ms / 1e9, 2.0 * fma / tiled_ms / 1e9 / 157.0, bytes / tiled_ms / 1e9, bytes / 8.0e12 * 1e3,
                same ? "true" : "false");
    return same ? 0 : 1;
}
