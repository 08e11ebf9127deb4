// kernels_align.hip — the cross-correlation of th_tm_align_tracks: r_i = sum over k < N of (double)a[k] (double)b[first + i + k] for a
// run of lags, in f64, in the contract's order (include/thesia_amd.h "Align two tracks"; the arithmetic is align_core.h, shared with
// th_xcorr_f64, so the bits are the host's).  The kernel's body is align_block.h: phase functions that a host program runs too,
// thread by thread (scripts/san_align.cpp).
//
//   The shape is band_kernel's (kernels_band.hip), in f64: the reference range is the wave-uniform "row", the probe is the sliding
//   input, the lags are the outputs.  A workgroup of 128 threads takes ALIGN_TILE = 1024 consecutive lags and ONE group of the
//   reference (32 blocks of 4096 samples); a thread takes ALIGN_R = 8 consecutive lags and keeps their 4 x 8 partial sums in f64
//   registers.  The reference is a kernel argument read at an index that depends on the loop alone, which the compiler turns into
//   scalar loads (a step's 64 samples in front of its LDS reads); a sample is converted to f64 once and serves 8 multiply-adds.
//   Per step of ALIGN_STEP = 64 reference samples the workgroup stages the tile's probe span ONCE: 1024 + 63 floats, +0 outside the
//   track, with one float of skew per 8 samples (align_at), so lane t reads float 9 t + const: conflict-free.  A thread slides a
//   window of 11 doubles over its 8 + 63 samples: four ds_read_b32 and four conversions per 32 v_fma_f64.
//   Two staged spans: the global loads of step s + 1 are issued into registers before the multiply-adds of step s and written to the
//   other span behind them; one barrier per step.  Every 64 steps a block ends: (p0 + p1) + (p2 + p3) joins the group's value.
//   The workgroup stores its group's value per lag with plain stores into scratch[g n_lags + i]; align_fold_kernel adds the groups in
//   ascending order.  No atomics; indices are 64-bit.  A thread whose lags lie past n_lags computes on staged samples and stores
//   nothing.
// The energies E(x, first, N) are small launches of the same order: one workgroup per group, thread 4 j + q partial sum q of block j.
#include <hip/hip_runtime.h>

#include "align_block.h"
#include "kernels.h"

namespace th {

namespace {

__global__ __launch_bounds__(ALIGN_THREADS, 2) void align_xcorr_kernel(const AlignJob job, const float *__restrict__ a) {
    __shared__ float xs[2][ALIGN_XS];
    const AlignBlock k = align_block_of(job, blockIdx.x);
    if (!k.any) return;  // (the whole workgroup)
    AlignAcc acc[ALIGN_R];
    double group[ALIGN_R];
#pragma unroll
    for (uint32_t i = 0; i < ALIGN_R; i++) {
        align_zero(acc[i]);
        group[i] = 0.0;
    }
    float pre[ALIGN_PRE];
    align_fetch(job, k, k.k_first, threadIdx.x, pre);
    align_commit(pre, threadIdx.x, xs[0]);
    __syncthreads();
    uint32_t buf = 0;
    for (uint64_t k0 = k.k_first; k0 < k.k_end; k0 += ALIGN_STEP, buf ^= 1u) {
        const bool more = k0 + ALIGN_STEP < k.k_end;
        if (more) align_fetch(job, k, k0 + ALIGN_STEP, threadIdx.x, pre);  // (in flight under the multiply-adds below)
        if (k.k_end - k0 >= ALIGN_STEP)
            align_accumulate<true>(acc, a + k0, ALIGN_STEP, xs[buf], threadIdx.x);
        else
            align_accumulate<false>(acc, a + k0, (uint32_t)(k.k_end - k0), xs[buf], threadIdx.x);
        if (!more || (k0 + ALIGN_STEP) % ALIGN_BLOCK == 0) align_block_end(acc, group);
        if (more) align_commit(pre, threadIdx.x, xs[buf ^ 1u]);  // (its last readers passed the barrier of the step before)
        __syncthreads();
    }
    align_store(job, k, threadIdx.x, group);
}

__global__ __launch_bounds__(256) void align_fold_kernel(const double *__restrict__ scratch, uint32_t n_groups, uint32_t n_lags, double *__restrict__ rec) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_lags) rec[i] = align_fold(scratch + i, n_groups, n_lags);
}

__global__ __launch_bounds__(ALIGN_ENERGY_THREADS) void align_energy_kernel(const float *__restrict__ x, uint64_t n, int64_t first, uint64_t N,
                                                                            double *__restrict__ groups) {
    __shared__ double part[ALIGN_ENERGY_THREADS];
    part[threadIdx.x] = align_energy_thread(x, n, first, N, blockIdx.x, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) groups[blockIdx.x] = align_energy_group(part, N, blockIdx.x);
}

}  // namespace

hipError_t launch_align_xcorr(const AlignJob &job, double *d_rec, hipStream_t s) {
    if (job.n_lags == 0 || job.N == 0) return hipSuccess;
    if (job.n_tiles != align_n_tiles(job.n_lags) || job.n_groups != align_n_groups(job.N) || job.n_lags > TH_ALIGN_PIECE_LAGS ||
        job.N > TH_ALIGN_MAX_REF)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(align_xcorr_kernel, dim3(job.n_tiles * job.n_groups), dim3(ALIGN_THREADS), 0, s, job, job.a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(align_fold_kernel, dim3((job.n_lags + 255u) / 256u), dim3(256), 0, s, job.scratch, job.n_groups, job.n_lags, d_rec);
    return hipGetLastError();
}

hipError_t launch_align_energy(const float *d_x, uint64_t n, int64_t first, uint64_t N, double *d_groups, hipStream_t s) {
    if (N == 0) return hipSuccess;
    if (N > TH_ALIGN_MAX_REF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(align_energy_kernel, dim3((uint32_t)align_n_groups(N)), dim3(ALIGN_ENERGY_THREADS), 0, s, d_x, n, first, N, d_groups);
    return hipGetLastError();
}

}  // namespace th
