// formant_time.hip — the two kernels of th_tm_get_formants timed apart by hipEvents: resample_kernel (the decimation to the
// analysis rate) and formant_kernel (LPC fit and roots), compiled from the product's sources, on the plan the reader itself makes
// (plan_formants / bind_formants) for C channels x S seconds at 48 kHz with the speech defaults.  A child process of
// scripts/bench_formant.py; prints one JSON line.  From the repository root (one line):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize scripts/ubench/formant_time.hip
//         thesia_amd/csrc/formant_plan.cpp thesia_amd/csrc/host_math.cpp -Lthesia_amd -lthesia_amd -Wl,-rpath,$PWD/thesia_amd
//         -o scripts/ubench/formant_time
// Usage: formant_time [seconds 30] [channels 128] [reps 5]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../thesia_amd/csrc/kernels_formant.hip"
#include "../../thesia_amd/csrc/kernels_resample.hip"

using namespace th;

namespace th {  // (the library keeps these to itself)
static thread_local char last_error[512];
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}
const char *get_error() { return last_error; }
}  // namespace th

#define HIP(call)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            std::fprintf(stderr, "%s failed: %s\n", #call, hipGetErrorString(e_));         \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

int main(int argc, char **argv) {
    const double seconds = argc > 1 ? std::atof(argv[1]) : 30.0;
    const size_t C = argc > 2 ? (size_t)std::atoi(argv[2]) : 128;
    const int reps = argc > 3 ? std::atoi(argv[3]) : 5;
    const uint32_t sr = 48000;
    const size_t n = (size_t)(seconds * sr);
    th_formant_request req;
    if (th_formant_defaults(&req) != TH_OK) return 1;
    th_formant_plan pl;
    if (formant_plan_for(sr, n, req, &pl) != 0) return 1;
    std::vector<float> x(n);
    uint32_t seed = 1;
    for (size_t i = 0; i < n; i++) {
        seed = seed * 1664525u + 1013904223u;
        x[i] = 0.3f * std::sin(0.09f * (float)i) + 0.2f * std::sin(0.31f * (float)i) + 0.05f * (float)(int32_t)seed * (1.0f / 2147483648.0f);
    }
    std::vector<float *> d_ch(C);
    std::vector<FormantPlanRequest> reqs(C);
    uint64_t at = 0;
    for (size_t c = 0; c < C; c++) {
        HIP(hipMalloc((void **)&d_ch[c], n * sizeof(float)));
        HIP(hipMemcpy(d_ch[c], x.data(), n * sizeof(float), hipMemcpyHostToDevice));
        reqs[c] = FormantPlanRequest{d_ch[c], n, pl, at};
        at += (pl.frame_end - pl.frame_first) * (2 + pl.n_poles);
    }
    FormantPlan p = plan_formants(reqs.data(), C);
    if (p.err) return 1;
    double *d_rec[2];
    float *d_scratch, *d_table;
    unsigned char *d_tab;
    for (int b = 0; b < 2; b++) HIP(hipMalloc((void **)&d_rec[b], std::max<uint64_t>(p.rec_need, 1) * sizeof(double)));
    HIP(hipMalloc((void **)&d_scratch, std::max<uint64_t>(p.scratch_need, 1) * sizeof(float)));
    HIP(hipMalloc((void **)&d_tab, p.tab_bytes));
    const std::vector<unsigned char> tab = bind_formants(p, FormantBases{{d_rec[0], d_rec[1]}, d_scratch, d_tab}, reqs.data(), C);
    HIP(hipMemcpy(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice));
    std::vector<float> table((size_t)pl.rs.L * 2 * pl.rs.half_taps);
    resample_table(pl.rs, table.data());
    HIP(hipMalloc((void **)&d_table, table.size() * sizeof(float)));
    HIP(hipMemcpy(d_table, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    const FormantJob *d_jobs = reinterpret_cast<const FormantJob *>(d_tab + p.o_jobs);
    const ResampleJob *d_rjobs = reinterpret_cast<const ResampleJob *>(d_tab + p.o_rjobs);
    hipEvent_t e0, e1, e2;
    HIP(hipEventCreate(&e0));
    HIP(hipEventCreate(&e1));
    HIP(hipEventCreate(&e2));
    std::vector<double> rs_ms, fm_ms;
    uint64_t frames = 0;
    for (int r = 0; r < reps + 1; r++) {  // (the first pass warms up and is not counted)
        double rs = 0, fm = 0;
        frames = 0;
        for (size_t k = 0; k < p.pieces.size(); k++) {
            const FormantPiece &pc = p.pieces[k];
            HIP(hipEventRecord(e0, nullptr));
            HIP(launch_resample(d_rjobs + pc.rjob0, (uint32_t)(pc.rjob1 - pc.rjob0), pc.n_rblocks, d_table, resample_tiling(pc.rs), nullptr));
            HIP(hipEventRecord(e1, nullptr));
            HIP(launch_formants(d_jobs + pc.run0, (uint32_t)(pc.run1 - pc.run0), pc.n_blocks, pc.max_W, pc.max_p, nullptr));
            HIP(hipEventRecord(e2, nullptr));
            HIP(hipEventSynchronize(e2));
            float a = 0, b = 0;
            HIP(hipEventElapsedTime(&a, e0, e1));
            HIP(hipEventElapsedTime(&b, e1, e2));
            rs += a;
            fm += b;
            frames += pc.n_blocks;
        }
        if (r) {
            rs_ms.push_back(rs);
            fm_ms.push_back(fm);
        }
    }
    std::sort(rs_ms.begin(), rs_ms.end());
    std::sort(fm_ms.begin(), fm_ms.end());
    std::printf("{\"channels\": %zu, \"seconds\": %g, \"frames\": %llu, \"pieces\": %zu, \"analysis_samples\": %llu, "
                "\"resample_kernel_ms\": %.3f, \"formant_kernel_ms\": %.3f, \"formant_kernel_us_per_1000_frames\": %.2f}\n",
                C, seconds, (unsigned long long)frames, p.pieces.size(), (unsigned long long)(pl.n_analysis * C), rs_ms[rs_ms.size() / 2],
                fm_ms[fm_ms.size() / 2], 1e6 * fm_ms[fm_ms.size() / 2] / (double)frames);
    return 0;
}
