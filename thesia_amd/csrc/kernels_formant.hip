// kernels_formant.hip — the formant reader's kernel (include/thesia_amd.h "Formant candidates"): per frame the windowed,
// pre-emphasised frame, its autocorrelation, Levinson-Durbin and the Aberth-Ehrlich sweeps, all in f64, one rounded operation per
// written operation (formant_core.h, shared with th_formants_f64: the bits are the host's).  The body is formant_block.h: phase
// functions that a host program runs too, thread by thread (scripts/san_formant.cpp).
//   A workgroup is ONE wave and ONE frame; the grid is the piece's frames.  Dynamic LDS: formant_lds_doubles(W, p) doubles of the
//   launch's largest W and p (4.4 KiB of samples and 5.7 KiB of partial sums at the speech defaults).  NL = 17 or 33 lags of
//   accumulators per lane, by the launch's largest p; a lag above the job's p is never touched, so the bits do not depend on NL.
//   Indices are 64-bit; plain C++ stores; a block past the piece's last frame stores nothing.
// -ffp-contract=off: nothing is fused.
#include <hip/hip_runtime.h>

#include "formant_block.h"
#include "kernels.h"

namespace th {

namespace {

template <uint32_t NL>
__global__ __launch_bounds__(64) void formant_kernel(const FormantJob *__restrict__ jobs, uint32_t n_jobs, uint32_t n_blocks) {
    extern __shared__ __attribute__((aligned(16))) double formant_lds[];
    if (blockIdx.x >= n_blocks) return;
    // the job of this block: the last one whose first_block is at or below the block index
    uint32_t lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (jobs[mid].first_block <= blockIdx.x)
            lo = mid;
        else
            hi = mid;
    }
    const FormantJob job = jobs[lo];
    const uint32_t i = blockIdx.x - job.first_block, tid = threadIdx.x;
    if (i >= job.n_frames) return;  // (the whole workgroup)
    const FormantLds l = formant_carve(formant_lds, job.W, job.p);
    formant_stage(job, job.f0 + i, tid, l);
    __syncthreads();
    formant_autocorr<NL>(job, tid, l);
    __syncthreads();
    formant_reduce(job, tid, l);
    __syncthreads();
    formant_fit(job, tid, l);
    __syncthreads();
    if (formant_wants_roots(job, l)) {
        formant_roots_start(job, tid, l);
        uint32_t sweeps = 0;
        bool stopped = false;
        while (sweeps < TH_FORMANT_MAX_SWEEPS && !stopped) {
            __syncthreads();  // (the roots of the last sweep, or the start points, are written; wm has been read)
            const fm_c w = formant_sweep_w(job, tid, l);
            __syncthreads();
            formant_sweep_move(job, tid, l, w);
            __syncthreads();
            sweeps++;
            stopped = formant_sweep_done(job, l);
        }
        formant_roots_end(tid, l, sweeps, stopped);
    }
    __syncthreads();
    formant_store(job, i, tid, l);
}

}  // namespace

hipError_t launch_formants(const FormantJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, uint32_t max_W, uint32_t max_p, hipStream_t s) {
    if (n_jobs == 0 || n_blocks == 0) return hipSuccess;
    if (max_W > TH_FORMANT_MAX_WIN || max_p > TH_FORMANT_MAX_POLES || max_p < 2 || max_W < max_p + 2) return hipErrorInvalidValue;
    const size_t lds = (size_t)formant_lds_doubles(max_W, max_p) * sizeof(double);  // (at most 51 KiB: below the 64 KiB a launch may ask for)
    const dim3 grid(n_blocks), block(FORMANT_LANES);
    if (max_p <= 16)
        hipLaunchKernelGGL(formant_kernel<17>, grid, block, lds, s, d_jobs, n_jobs, n_blocks);
    else
        hipLaunchKernelGGL(formant_kernel<33>, grid, block, lds, s, d_jobs, n_jobs, n_blocks);
    return hipGetLastError();
}

}  // namespace th
