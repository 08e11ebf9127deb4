// kernels_flac.hip — resident planar f32 channels to FLAC frames (th_tm_export_flac): blocks of 4096 samples are independent of each
// other, so the encoder is block-parallel integer work.  Three launches per piece over one table of jobs (a job = blocks [b0, b0 + nb)
// of one request, flac_plan.h); the bodies are flac_block.h, phase functions that the host runs too, thread by thread (that run is
// th_flac_encode_i32, and scripts/san_flac.cpp runs it under the sanitizers).
//
//   1. flac_subframe_kernel: one workgroup per unit = (block, coded channel).  Quantise the block into LDS (export_core.h, the absolute index);
//      per fixed order 0 .. 4 the sums S[q][k] of (u >> k) over every partition q and parameter k (256 >> p threads stride over a
//      partition, a thread keeps its 16 zigzagged residuals in registers and adds one 64-bit LDS atomic per k), the partition's best k
//      and the order's exact cost; then the type.  Only then the bits: the lengths' exclusive scan gives every code's position, the
//      unary zeros are the zeroed buffer's, a code is one LDS atomic OR of k + 1 bits in at most two words.  The words go to the
//      unit's slot, the bit length to a table.
//   2. flac_scan_kernel: one workgroup per job: frame lengths from the table, byte offsets, total, min, max.
//   3. flac_frame_kernel: one workgroup per frame: header, the n_ch subframes joined at their bit offsets (each output word a funnel
//      shift of two source words), padding, CRC-16 (per thread over a run of words, combined by the CRC's linearity), at the frame's
//      dense byte offset, byte-granular.
// With flags (th_tm_export_flac_ex) kernel 1 is its <true> instance: TH_FLAC_LPC adds, in front of the orders, the block's level, the
// integer window and nine autocorrelation lags (per-thread int64 sums, one 64-bit LDS atomic each; the windowed samples share LDS
// with the sums and the output words, which are zeroed afterwards), Levinson-Durbin and the quantiser on one lane, and behind the
// fixed orders one more pass per LPC order of the fit.  TH_FLAC_STEREO makes four units of a 2-channel block (L, R, mid, side; mid and
// side quantise both channels), kernel 2 picks the frame's pair from the four bit lengths and kernel 3 joins that pair.
// -ffp-contract=off: the quantiser's and the LPC fit's f64 steps are one rounded operation each, as on the host.
#include <hip/hip_runtime.h>

#include "flac_block.h"
#include "kernels.h"

namespace th {

namespace {

template <class First>
__device__ __forceinline__ uint32_t find_job(const FlacJob *jobs, uint32_t n_jobs, uint32_t block, First first) {
    uint32_t lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first(jobs[mid]) <= block)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// EX: the _ex entries' kernel (job.flags: LPC candidates, a stereo block's four units); the other one is compiled for flags == 0
template <bool EX>
__global__ __launch_bounds__(FLAC_THREADS) void flac_subframe_kernel(const FlacJob *__restrict__ jobs, uint32_t n_jobs) {
    __shared__ FlacSubLds l;
    const FlacJob job = jobs[find_job(jobs, n_jobs, blockIdx.x, [](const FlacJob &j) { return j.first_unit; })];
    const uint32_t flags = EX ? job.flags : 0u;
    const FlacUnit k = flac_unit_of(job, blockIdx.x - job.first_unit, flags);
    if (!k.any) return;  // (the whole workgroup)
    const uint32_t tid = threadIdx.x;
    flac_sub_clear(k, tid, l);
    __syncthreads();
    flac_sub_quantize(job, k, tid, l);
    __syncthreads();
    const bool fit = EX && (flags & TH_FLAC_LPC) && k.n >= FLAC_MIN_PART;
    if (fit) {
        flac_lpc_level(k, tid, l);
        __syncthreads();
        flac_lpc_window_block(k, tid, l);
        __syncthreads();
        flac_lpc_autocorr(k, tid, l);
        __syncthreads();
        flac_sub_clear_work(k, tid, l);
        flac_lpc_fit_block(k, tid, l);
        __syncthreads();
    }
    for (uint32_t o = 0; o <= FLAC_MAX_ORDER; o++) {
        flac_sub_accumulate(k, o, tid, l);
        __syncthreads();
        flac_sub_pick_k(k, o, tid, l);
        __syncthreads();
    }
    if (fit) {
        const uint32_t ok = l.fit.ok;  // (the same in every thread: the loop's barriers are uniform)
        for (uint32_t m = 1; m <= FLAC_LPC_MAX; m++) {
            if (!((ok >> (m - 1u)) & 1u)) continue;
            flac_sub_accumulate_lpc(k, m, tid, l);
            __syncthreads();
            flac_sub_pick_k(k, FLAC_MAX_ORDER + m, tid, l);
            __syncthreads();
        }
    }
    const FlacChoice ch = flac_sub_choose(k, fit, l);
    flac_sub_lengths(k, ch, tid, l);
    __syncthreads();
    flac_sub_write(k, ch, tid, l);
    __syncthreads();
    flac_sub_store(job, k, ch, tid, l);
}

__global__ __launch_bounds__(FLAC_THREADS) void flac_scan_kernel(const FlacJob *__restrict__ jobs, uint32_t n_jobs) {
    __shared__ FlacScanLds l;
    if (blockIdx.x >= n_jobs) return;
    const FlacJob job = jobs[blockIdx.x];
    flac_scan_sum(job, threadIdx.x, l);
    __syncthreads();
    flac_scan_write(job, threadIdx.x, l);
}

__global__ __launch_bounds__(FLAC_THREADS) void flac_frame_kernel(const FlacJob *__restrict__ jobs, uint32_t n_jobs) {
    __shared__ FlacFrameLds l;
    const FlacJob job = jobs[find_job(jobs, n_jobs, blockIdx.x, [](const FlacJob &j) { return j.first_block; })];
    const uint32_t f = blockIdx.x - job.first_block;
    if (f >= job.nb) return;
    flac_frame_prepare(job, f, threadIdx.x, l);
    __syncthreads();
    const FlacFrame fr = flac_frame_of(job, f, l);
    if (!fr.any) return;
    flac_frame_store(job, fr, threadIdx.x, l);
    flac_frame_crc_part(job, fr, threadIdx.x, l);
    __syncthreads();
    flac_frame_crc_store(job, fr, threadIdx.x, l);
}

}  // namespace

hipError_t launch_flac_subframes(const FlacJob *d_jobs, uint32_t n_jobs, uint32_t n_units, uint32_t flags, hipStream_t s) {
    if (n_jobs == 0 || n_units == 0) return hipSuccess;
    if (flags)
        hipLaunchKernelGGL(flac_subframe_kernel<true>, dim3(n_units), dim3(FLAC_THREADS), 0, s, d_jobs, n_jobs);
    else
        hipLaunchKernelGGL(flac_subframe_kernel<false>, dim3(n_units), dim3(FLAC_THREADS), 0, s, d_jobs, n_jobs);
    return hipGetLastError();
}
hipError_t launch_flac_scan(const FlacJob *d_jobs, uint32_t n_jobs, hipStream_t s) {
    if (n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(flac_scan_kernel, dim3(n_jobs), dim3(FLAC_THREADS), 0, s, d_jobs, n_jobs);
    return hipGetLastError();
}
hipError_t launch_flac_frames(const FlacJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, hipStream_t s) {
    if (n_jobs == 0 || n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(flac_frame_kernel, dim3(n_blocks), dim3(FLAC_THREADS), 0, s, d_jobs, n_jobs);
    return hipGetLastError();
}

}  // namespace th
