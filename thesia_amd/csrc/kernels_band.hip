// kernels_band.hip — the band filter of th_tm_export_pcm_band: planar f32 channels through ONE FIR row of 2K taps, planar f32 out at
// the same rate, 2K fmaf per output sample (include/thesia_amd.h "Export what a spectrogram box holds"; the sum is resample_core.h,
// shared with th_band_f32 and with the resampler, so the bits are the host's).  The kernel's body is band_block.h: phase functions
// that a host program runs too, thread by thread (scripts/san_band.cpp).
//
//   Every output has the same row, so the coefficients are wave-uniform: the row is a kernel argument read at an index that depends
//   on the loop alone, which the compiler turns into scalar loads (s_load_dwordx16, a block's 64 coefficients in front of its LDS
//   reads); each is copied to a VGPR once (band_coef: a v_fmac_f32 with an SGPR source issues in 3.2 clocks, with VGPR sources in
//   2.05) and serves 8 fmaf.  No lane gathers a coefficient and none passes through LDS.
//   Tiling.  A workgroup of 256 threads takes one channel and BAND_TILE = 2048 consecutive outputs; a thread takes BAND_R = 8
//   consecutive ones and keeps their 4 x 8 partial sums in registers.  The taps are walked in blocks of BAND_TAP_BLOCK = 64 (the
//   contract's order: a tap goes to partial sum k mod 4, and a block starts at a multiple of 4, so cutting the row changes nothing).
//   Per block the workgroup stages the tile's input span ONCE: 2048 + 63 samples, zeros outside the track.  A thread slides a window
//   of 11 registers over its 8 + 63 samples: four ds_read_b32 per 32 v_fmac_f32, one LDS dword per 8 fmaf.
//   Banks.  Thread t's window starts 8 t samples into the span; the span is stored with one float of skew per 8 samples
//   (band_at), so lane t reads float 9 t + const: 64 lanes, 64 banks.
//   Pipeline.  Two staged spans: the global loads of block b + 1 are issued into registers before the fmaf of block b; nothing reads
//   a loaded register until band_commit, behind the fmaf, selects the zeros outside the track and writes the other span (the wait
//   for the loads, s_waitcnt vmcnt, stands behind the fmaf block in the compiled loop); one barrier per block.
//   Indices are 64-bit; a thread whose outputs lie past jb computes on staged samples and stores nothing.
// -ffp-contract=off: the only roundings are the explicit fmaf and the three additions of the fold.
#include <hip/hip_runtime.h>

#include "band_block.h"
#include "kernels.h"

namespace th {

namespace {

__global__ __launch_bounds__(BAND_THREADS) void band_kernel(const BandJob *__restrict__ jobs, uint32_t n_jobs, const float *__restrict__ row,
                                                            uint32_t taps) {
    __shared__ float xs[2][BAND_XS];
    // the job of this block: the last one whose first_block is at or below the block index
    uint32_t lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (jobs[mid].first_block <= blockIdx.x)
            lo = mid;
        else
            hi = mid;
    }
    const BandJob job = jobs[lo];
    const BandBlock k = band_block_of(job, blockIdx.x - job.first_block);
    if (!k.any) return;  // (the whole workgroup)
    ResampleAcc acc[BAND_R];
    float pre[BAND_PRE];
    band_fetch(job, k, taps, 0, threadIdx.x, pre);
    band_commit(job, k, taps, 0, pre, threadIdx.x, xs[0]);
    __syncthreads();
    uint32_t buf = 0;
    for (uint32_t kb = 0; kb < taps; kb += BAND_TAP_BLOCK, buf ^= 1u) {
        const bool more = kb + BAND_TAP_BLOCK < taps;
        if (more) band_fetch(job, k, taps, kb + BAND_TAP_BLOCK, threadIdx.x, pre);  // (in flight under the fmaf below)
        if (taps - kb >= BAND_TAP_BLOCK)
            band_accumulate<true>(acc, row + kb, BAND_TAP_BLOCK, xs[buf], threadIdx.x);
        else
            band_accumulate<false>(acc, row + kb, taps - kb, xs[buf], threadIdx.x);
        if (more) band_commit(job, k, taps, kb + BAND_TAP_BLOCK, pre, threadIdx.x, xs[buf ^ 1u]);  // (its last readers passed the barrier of the step before)
        __syncthreads();
    }
    band_store(job, k, threadIdx.x, acc);
}

}  // namespace

hipError_t launch_band(const BandJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, const float *d_row, const BandTiling &t, hipStream_t s) {
    if (n_jobs == 0 || n_blocks == 0) return hipSuccess;
    if (t.tile != BAND_TILE || t.R != BAND_R || t.tap_block != BAND_TAP_BLOCK || t.taps < 2 || (t.taps & 1u) || t.taps > TH_BAND_MAX_TAPS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(band_kernel, dim3(n_blocks), dim3(BAND_THREADS), 0, s, d_jobs, n_jobs, d_row, t.taps);
    return hipGetLastError();
}

}  // namespace th
