// kernels_resample.hip — the polyphase sinc resampler of th_tm_export_pcm_at: planar f32 channels at the track's rate to planar f32
// at the output rate, 2K fmaf per output sample (include/thesia_amd.h "Export at a target sample rate"; the sum is resample_core.h,
// shared with th_resample_f32, so the bits are the host's).  The kernel's body is resample_block.h: phase functions that a host
// program runs too, thread by thread (scripts/san_resample.cpp).
//
//   Tiling (kernels.h ResampleTiling).  Outputs j and j + L share a coefficient row; their windows lie M input samples apart.  A
//   workgroup of G waves takes one channel, R <= 64 consecutive outputs (lane i = output j_first + i, so neighbouring lanes read
//   neighbouring input samples: about M / L apart, whatever the parity of M) and P = G Pt periods of them, Lp outputs apart.  Wave g
//   takes periods g Pt .. g Pt + Pt - 1; a thread keeps 4 coefficients in registers across its Pt periods.  For L < 64 (the octave
//   ratios: L = 1, 2) Lp is the largest multiple of L up to 64 and a row is staged once per lane that uses it: no lane idles.
//   Steps.  The 2K taps are walked in blocks of RESAMPLE_TAP_BLOCK (the contract's order: a tap goes to partial sum k mod 4, and a
//   block starts at a multiple of 4, so cutting the row changes nothing).  Per block the workgroup stages
//     cs: the R rows' taps of the block (gathered by row index from the table in L2; pitch 68 floats: the 16-byte reads of 16 lanes
//         cover the 64 banks once),
//     xa, xb: the input span of the block, zeros outside the track, TWICE: xb[t] = xa[t + 1].  A window starts at any sample; a
//         lane whose start is odd reads xb at the even index below, so every window is read with aligned 8-byte loads (256 B / clk
//         instead of the 128 B / clk of 4-byte reads).
//   LDS reads per fmaf: (1 + 2 Pt) / (4 Pt) instructions, 9 dwords per 8 fmaf at Pt = 8.
//   Indices are 64-bit; a lane without an output (past jb, or past the sub-tile) computes on offset 0 and stores nothing.
// -ffp-contract=off: the only roundings are the explicit fmaf and the three additions of the fold.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "resample_block.h"

namespace th {

namespace {

template <uint32_t PT>
__global__ __launch_bounds__(256) void resample_kernel(const ResampleJob *__restrict__ jobs, uint32_t n_jobs, const float *__restrict__ table,
                                                       const ResampleTiling tl) {
    __shared__ __attribute__((aligned(16))) float xa[RESAMPLE_XS_MAX];
    __shared__ __attribute__((aligned(16))) float xb[RESAMPLE_XS_MAX];
    __shared__ __attribute__((aligned(16))) float cs[RESAMPLE_LANES * RESAMPLE_CS_PITCH];
    __shared__ uint32_t rows[RESAMPLE_LANES];
    // the job of this block: the last one whose first_block is at or below the block index
    uint32_t lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (jobs[mid].first_block <= blockIdx.x)
            lo = mid;
        else
            hi = mid;
    }
    const ResampleJob job = jobs[lo];
    const ResampleBlock k = resample_block_of(job, tl, blockIdx.x - job.first_block);
    if (!k.any) return;  // (the whole workgroup)
    ResampleLane<PT> ln;
    resample_lane_setup<PT>(job, tl, k, threadIdx.x, ln);
    if (threadIdx.x < RESAMPLE_LANES) rows[threadIdx.x] = ln.row;
    for (uint32_t kb = 0; kb < tl.taps; kb += RESAMPLE_TAP_BLOCK) {
        const uint32_t nt = min(RESAMPLE_TAP_BLOCK, tl.taps - kb);
        __syncthreads();  // (the last block's reads are done; rows[] is written)
        resample_stage(job, tl, k, table, rows, kb, nt, threadIdx.x, blockDim.x, xa, xb, cs);
        __syncthreads();
        resample_accumulate<PT>(ln, nt, cs + (threadIdx.x & 63u) * RESAMPLE_CS_PITCH, xa, xb);
    }
    resample_store<PT>(job, tl, k, ln);
}

}  // namespace

hipError_t launch_resample(const ResampleJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, const float *d_table, const ResampleTiling &t,
                           hipStream_t s) {
    if (n_jobs == 0 || n_blocks == 0) return hipSuccess;
    if (t.span > RESAMPLE_XS_MAX || t.R > RESAMPLE_LANES || (t.G != 1 && t.G != 4) || t.taps < 2) return hipErrorInvalidValue;
    const dim3 grid(n_blocks), block(64 * t.G);
    switch (t.Pt) {
        case 8: hipLaunchKernelGGL(resample_kernel<8>, grid, block, 0, s, d_jobs, n_jobs, d_table, t); break;
        case 4: hipLaunchKernelGGL(resample_kernel<4>, grid, block, 0, s, d_jobs, n_jobs, d_table, t); break;
        case 2: hipLaunchKernelGGL(resample_kernel<2>, grid, block, 0, s, d_jobs, n_jobs, d_table, t); break;
        case 1: hipLaunchKernelGGL(resample_kernel<1>, grid, block, 0, s, d_jobs, n_jobs, d_table, t); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace th
