// kernels_spectrum.hip — the spectrum of a frame range of resident dB rows (th_tm_get_spectra): per column the mean amplitude, the
// mean power (both back in dB) or the maximum over the frames [f0, f1) of a T x H spec.  One read of the rows.
//
//   pass 1  spectrum_partial_kernel: grid (blocks of the largest job, jobs).  A job's columns are cut into tiles of ct quads (a quad
//           = 4 columns = one 16-byte load; ct = 8 .. 64, SpectrumShape) and its frames into slices of slice_len; block
//           (tile, slice) holds 256 / ct frames side by side, thread (r, q) walks the frames fa + r, fa + r + 256 / ct, ... of its
//           quad and keeps four f64 sums (or f32 maxima).  The block adds its 256 / ct rows in ascending r and writes one f64 partial
//           per column: part[slice][col].  Neighbouring blocks are neighbouring tiles of the same frames.
//   pass 2  spectrum_finish_kernel: one thread per column adds the slices in ascending order, applies 1 / n and the logarithm (f64)
//           and writes the f32 result.
// Every sum has a fixed order that follows from (H, f0, f1) alone: no atomics, so a request's values do not depend on the batch it
// is part of, on the stream or on the call.  The pitch padding behind a row's H columns may be read (the last quad) and is never
// written out: columns are independent.
//
// 10^(s c) = 2^p, p = s c log2(10) in f64; p = i + f, f in [0, 1): 2^f by v_exp_f32 (1 ulp of f32), scaled by 2^i in f64
// (v_ldexp_f64): no overflow or underflow at any dB value an f32 holds, -inf gives 0, NaN stays NaN.  (-ffp-contract=off: the
// sums are plain f64 additions in the stated order.)
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.h"

namespace th {

namespace {

constexpr uint32_t SPECTRUM_THREADS = 256;
constexpr uint32_t SPECTRUM_BLOCKS_PER_JOB = 512;  // what one job alone is cut into (two blocks per CU), where its frames allow

template <int KIND>
__device__ __forceinline__ double pow10_db(float s) {
    constexpr double K = 3.321928094887362 / (KIND == TH_SPECTRUM_MEAN_AMP ? 20.0 : 10.0);
    const double p = fmin(fmax((double)s * K, -1100.0), 1100.0);  // (beyond: 0 or inf either way; a NaN is put back below)
    const double i = floor(p);
    const float e = __builtin_amdgcn_exp2f((float)(p - i));
    const double v = ldexp((double)e, (int)i);
    return s != s ? (double)s : v;
}

template <int KIND>
__device__ __forceinline__ void take(double a[4], const float4 v) {
    if (KIND == TH_SPECTRUM_MAX) {  // a NaN stays: nothing compares greater than it, and it replaces any number
        a[0] = (v.x > a[0] || v.x != v.x) ? (double)v.x : a[0];
        a[1] = (v.y > a[1] || v.y != v.y) ? (double)v.y : a[1];
        a[2] = (v.z > a[2] || v.z != v.z) ? (double)v.z : a[2];
        a[3] = (v.w > a[3] || v.w != v.w) ? (double)v.w : a[3];
    } else {
        a[0] += pow10_db<KIND>(v.x);
        a[1] += pow10_db<KIND>(v.y);
        a[2] += pow10_db<KIND>(v.z);
        a[3] += pow10_db<KIND>(v.w);
    }
}

template <int KIND>
__device__ __forceinline__ double fold(double a, double b) {
    if (KIND == TH_SPECTRUM_MAX) return (b > a || b != b) ? b : a;
    return a + b;
}

template <int KIND>
__device__ __forceinline__ void partial_block(const SpectrumJob &job, double *red) {
    const uint32_t slice = blockIdx.x / job.n_ctiles, ctile = blockIdx.x - slice * job.n_ctiles;
    const uint32_t ct = 1u << job.log_ct, rb = SPECTRUM_THREADS >> job.log_ct;
    const uint32_t t = threadIdx.x, q = t & (ct - 1), r = t >> job.log_ct;
    const uint32_t col0 = (ctile * ct + q) * 4;
    const uint32_t fa = job.f0 + slice * job.slice_len;
    const uint32_t fb = job.f1 - fa < job.slice_len ? job.f1 : fa + job.slice_len;
    const double init = KIND == TH_SPECTRUM_MAX ? -INFINITY : 0.0;
    double a[4] = {init, init, init, init};
    if (col0 < job.H) {  // (col0 + 3 < pitch: the pitch is a multiple of 4 floats and at least H)
        const gptr<const float> p = as_global(job.rows) + col0;  // (global, not flat, loads: stft_core.h)
        const uint64_t pitch = job.pitch;
        uint32_t f = fa + r;
        for (; f < fb && fb - f > 3 * rb; f += 4 * rb) {  // four loads in flight per thread
            const float4 v0 = *reinterpret_cast<gptr<const float4>>(p + (uint64_t)f * pitch);
            const float4 v1 = *reinterpret_cast<gptr<const float4>>(p + (uint64_t)(f + rb) * pitch);
            const float4 v2 = *reinterpret_cast<gptr<const float4>>(p + (uint64_t)(f + 2 * rb) * pitch);
            const float4 v3 = *reinterpret_cast<gptr<const float4>>(p + (uint64_t)(f + 3 * rb) * pitch);
            take<KIND>(a, v0);
            take<KIND>(a, v1);
            take<KIND>(a, v2);
            take<KIND>(a, v3);
        }
        for (; f < fb; f += rb) take<KIND>(a, *reinterpret_cast<gptr<const float4>>(p + (uint64_t)f * pitch));
    }
    const uint32_t w = ct * 4;  // columns of the tile
#pragma unroll
    for (int j = 0; j < 4; j++) red[r * w + q * 4 + j] = a[j];
    __syncthreads();
    if (t < w) {
        const uint32_t col = ctile * w + t;
        double s = red[t];
        for (uint32_t k = 1; k < rb; k++) s = fold<KIND>(s, red[k * w + t]);
        if (col < job.H) as_global(job.part)[(uint64_t)slice * ((uint64_t)job.n_ctiles * w) + col] = s;
    }
}

// the slices of one column in ascending order; eight loads in flight (a thread has nothing else to hide their latency behind)
template <int KIND>
__device__ __forceinline__ double fold_slices(gptr<const double> part, uint64_t hp, uint32_t n_slices) {
    double acc = part[0];
    uint32_t s = 1;
    for (; n_slices - s >= 8; s += 8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = part[(s + k) * hp];
#pragma unroll
        for (int k = 0; k < 8; k++) acc = fold<KIND>(acc, v[k]);
    }
    for (; s < n_slices; s++) acc = fold<KIND>(acc, part[s * hp]);
    return acc;
}

}  // namespace

__global__ __launch_bounds__(SPECTRUM_THREADS) void spectrum_partial_kernel(const SpectrumJob *__restrict__ jobs) {
    __shared__ double red[SPECTRUM_THREADS * 4];
    const SpectrumJob job = jobs[blockIdx.y];
    if (blockIdx.x >= job.n_ctiles * job.n_slices) return;
    switch (job.kind) {
        case TH_SPECTRUM_MEAN_AMP: partial_block<TH_SPECTRUM_MEAN_AMP>(job, red); break;
        case TH_SPECTRUM_MEAN_POWER: partial_block<TH_SPECTRUM_MEAN_POWER>(job, red); break;
        default: partial_block<TH_SPECTRUM_MAX>(job, red); break;
    }
}

__global__ __launch_bounds__(SPECTRUM_THREADS) void spectrum_finish_kernel(const SpectrumJob *__restrict__ jobs) {
    const SpectrumJob job = jobs[blockIdx.y];
    const uint32_t col = blockIdx.x * SPECTRUM_THREADS + threadIdx.x;
    if (col >= job.H) return;
    const uint32_t n = job.f1 - job.f0;
    const uint64_t hp = (uint64_t)job.n_ctiles << (job.log_ct + 2);
    const gptr<const double> part = as_global((const double *)job.part) + col;
    float o;
    if (n == 0) {
        o = __builtin_nanf("");
    } else if (job.kind == TH_SPECTRUM_MAX) {
        o = (float)fold_slices<TH_SPECTRUM_MAX>(part, hp, job.n_slices);  // (exact: every partial is an f32 value)
    } else {
        const double sum = fold_slices<TH_SPECTRUM_MEAN_AMP>(part, hp, job.n_slices);
        o = (float)((job.kind == TH_SPECTRUM_MEAN_AMP ? 20.0 : 10.0) * log10(sum / (double)n));
    }
    as_global(job.out)[col] = o;
}

// The cut of one job, from its own shape alone (the values of a request must not depend on its batch).  Column tile: the widest of
// 64 / 32 / 16 / 8 quads that leaves at most an eighth of the row's quads idle in the last tile, else the one with the least
// padding.  Slices: as many as bring the job to SPECTRUM_BLOCKS_PER_JOB blocks, of whole groups of 256 / ct frames.
SpectrumShape spectrum_shape(uint32_t height, uint32_t n_frames) {
    SpectrumShape s{};
    const uint32_t quads = (height + 3) / 4;
    uint32_t best = 3, best_pad = UINT32_MAX;
    bool found = false;
    for (uint32_t l = 6; l >= 3 && !found; l--) {
        const uint32_t ct = 1u << l, pad = (quads + ct - 1) / ct * ct - quads;
        if (pad <= quads / 8) {
            best = l;
            found = true;
        } else if (pad < best_pad) {
            best = l;
            best_pad = pad;
        }
    }
    s.log_ct = best;
    const uint32_t ct = 1u << best, rb = SPECTRUM_THREADS / ct;
    s.n_ctiles = (quads + ct - 1) / ct;
    if (n_frames == 0) {
        s.n_slices = 0;
        s.slice_len = rb;
        return s;
    }
    const uint32_t wanted = (SPECTRUM_BLOCKS_PER_JOB + s.n_ctiles - 1) / s.n_ctiles;
    const uint32_t len = (n_frames + wanted - 1) / wanted;
    s.slice_len = (len + rb - 1) / rb * rb;
    s.n_slices = (n_frames + s.slice_len - 1) / s.slice_len;
    return s;
}

hipError_t launch_spectrum(const SpectrumJob *d_jobs, uint32_t n_jobs, uint32_t max_blocks, uint32_t max_height, hipStream_t s) {
    for (uint32_t j0 = 0; j0 < n_jobs; j0 += 65535) {  // (grid.y)
        const uint32_t nj = n_jobs - j0 < 65535 ? n_jobs - j0 : 65535;
        if (max_blocks) hipLaunchKernelGGL(spectrum_partial_kernel, dim3(max_blocks, nj), dim3(SPECTRUM_THREADS), 0, s, d_jobs + j0);
        if (max_height)
            hipLaunchKernelGGL(spectrum_finish_kernel, dim3((max_height + SPECTRUM_THREADS - 1) / SPECTRUM_THREADS, nj),
                               dim3(SPECTRUM_THREADS), 0, s, d_jobs + j0);
    }
    return hipGetLastError();
}

}  // namespace th
