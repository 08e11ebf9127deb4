// kernels_dynamics.hip — the normalise gain and the clip guard of a batch of tracks: AudioTrack::apply_gain (track.rs:158-170) ->
// Audio::mutate -> clip / reduce_global_level / limit (audio.rs:50-63,133-179), the limiter being PerfectLimiter::process_inplace
// (dynamics/limiter.rs:110-156) over PeakHold, ExponentialRelease and a BoxStackFilter of three layers (dynamics/envelope.rs).
//
// dyn_apply_kernel: y = gain x in f32, then the clamp (keeping y as the before-clip audio, with every channel's peak and count of
// |y| > 1) or the global gain y <- clamp(f32(f64(y) g)).
//
// The limiter's gain is a function of v[t] = max over the channels of |gain x[t]| on t < N = n + attack (zeros behind the track);
// sample j's gain is the value of step j + attack.  No stage is sequential in more than a short run:
//   lim_absmax   v (f32) and the maximum of every block of LIM_BLOCK values.
//   lim_peak     the peak hold.  raw = v > 1 ? 1 / (v + eps) : 1 falls as v grows, so the sliding minimum of raw over the last `hold`
//                steps is raw of the sliding MAXIMUM of the f32 v: exact, from block maxima and at most 2 (LIM_BLOCK - 1) single values.
//   lim_release  y <- min(p, fma(p - y, slew, y)), y0 = 1.  One step is y -> min(C, A y + D) with A = 1 - slew, D = slew p, C = p, and
//                such maps compose: (A2, D2, C2) o (A1, D1, C1) = (A2 A1, A2 D1 + D2, min(C2, A2 C1 + D2)).  _summary composes a chunk of
//                LIM_CHUNK steps, _carry runs the chunks' maps from y0 serially (one thread per track) for every chunk's start
//                state, _replay runs each chunk from it with the reference's own arithmetic.  A start state is off by the rounding of
//                the composed maps (~1e-16); the recurrence contracts by (1 - slew) per step, so that dies out, and y = p exactly
//                wherever the minimum takes p.
//   lim_box_cum  BoxSum (envelope.rs:10-87) keeps a running sum that restarts every len + 1 steps (buffer length len + 1) and
//                remembers the last period's total (wrap_jump): step t is (k, j) with t + 1 = k (len + 1) + j, and its read is
//                S[t] - S[t - len] when j = len, else (S[t] + W[k - 1]) - S[t - len], S the period's own running sum and W a period's
//                total.  reset(1.) pre-fills period -1 with S = 1, 2, .. and W = len + 1, and S = 0 at t = -1.  The periods start at
//                fixed steps, so one thread per period adds its len + 1 inputs in the sequential order: the sums are those of the
//                sequential filter bit for bit.  A layer's inputs are the reads of the layer below times 1 / len, formed on the fly.
//   lim_apply    gain = min(read of layer 3, 1); y <- f32(clamp(f64(gain x) gain, -1, 1)); the gain as f32; the least gain and
//                the count of gains != 1.
// Built with -ffp-contract=off: every product and sum above is rounded as the scalar reference rounds it; fma() is explicit.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "kernels.h"

namespace th {

namespace {

constexpr uint32_t DYN_THREADS = 256;

__device__ __forceinline__ float clamp1(float y) { return y < -1.0f ? -1.0f : (y > 1.0f ? 1.0f : y); }  // f32::clamp: NaN stays
__device__ __forceinline__ double clamp1(double y) { return y < -1.0 ? -1.0 : (y > 1.0 ? 1.0 : y); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// One (extremum, count) pair per block — a thread runs DYN_ITEMS samples, the waves meet in LDS — so that a track's reduction slot
// takes one atomic per 2048 samples (one per wave of 64 samples kept a 128-track batch waiting on its slots for 15 ms)
constexpr uint32_t DYN_ITEMS = 8;
template <bool MAX>
__device__ __forceinline__ void block_reduce(float ext, uint32_t cnt, uint32_t *slot_bits, unsigned long long *slot_cnt) {
    __shared__ float sh_ext[DYN_THREADS / 64];
    __shared__ uint32_t sh_cnt[DYN_THREADS / 64];
    ext = MAX ? wave_max(ext) : wave_min(ext);
    cnt = wave_sum(cnt);
    __syncthreads();  // (the last use of the arrays is over)
    if ((threadIdx.x & 63) == 0) {
        sh_ext[threadIdx.x / 64] = ext;
        sh_cnt[threadIdx.x / 64] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < DYN_THREADS / 64; w++) {
            ext = MAX ? fmaxf(ext, sh_ext[w]) : fminf(ext, sh_ext[w]);
            cnt += sh_cnt[w];
        }
        // (non-negative floats order as their bits)
        if (MAX) atomicMax(slot_bits, __float_as_uint(ext));
        else atomicMin(slot_bits, __float_as_uint(ext));
        if (cnt) atomicAdd(slot_cnt, (unsigned long long)cnt);
    }
}

__global__ __launch_bounds__(DYN_THREADS) void dyn_apply_kernel(const DynApplyJob *__restrict__ jobs) {
    const DynApplyJob J = jobs[blockIdx.y];
    const uint64_t b0 = (uint64_t)blockIdx.x * (DYN_THREADS * DYN_ITEMS);
    if (b0 >= J.n) return;  // (whole blocks only: the threads below reduce together)
    for (uint32_t c = 0; c < J.n_ch; c++) {
        float pk = 0.0f;
        uint32_t over = 0;
        for (uint32_t k = 0; k < DYN_ITEMS; k++) {
            const uint64_t i = b0 + k * DYN_THREADS + threadIdx.x;
            if (i >= J.n) break;
            const float y = J.gain * J.x[c * J.x_stride + i];
            if (J.clip) {
                J.before[c * J.y_stride + i] = y;
                J.aud[c * J.y_stride + i] = clamp1(y);
                pk = fmaxf(pk, fabsf(y));
                over += fabsf(y) > 1.0f;
            } else {
                J.aud[c * J.y_stride + i] = J.scale ? clamp1((float)((double)y * J.g)) : y;
            }
        }
        if (J.clip) block_reduce<true>(pk, over, &J.peak_bits[c], &J.cnt[c]);
    }
}

__global__ __launch_bounds__(DYN_THREADS) void lim_absmax_kernel(const LimJob *__restrict__ jobs) {
    const LimJob J = jobs[blockIdx.y];
    const uint64_t N = J.n + J.attack, b0 = (uint64_t)blockIdx.x * DYN_THREADS, i = b0 + threadIdx.x;
    if (b0 >= N) return;
    float v = 0.0f;
    if (i < J.n) {
        v = fabsf(J.gain * J.x[i]);
        for (uint32_t c = 1; c < J.n_ch; c++) v = fmaxf(v, fabsf(J.gain * J.x[c * J.x_stride + i]));  // reduce(f32::max)
    }
    if (i < N) J.v[i] = v;
    const float m = wave_max(v);
    if ((threadIdx.x & 63) == 0 && i < N) J.bm[i / LIM_BLOCK] = m;
}

__global__ __launch_bounds__(DYN_THREADS) void lim_peak_kernel(const LimJob *__restrict__ jobs) {
    const LimJob J = jobs[blockIdx.y];
    const uint64_t N = J.n + J.attack, t = (uint64_t)blockIdx.x * DYN_THREADS + threadIdx.x;
    if (t >= N) return;
    const uint64_t lo = t + 1 >= J.hold ? t + 1 - J.hold : 0;  // the window [lo, t]: the last `hold` steps
    const uint64_t blk0 = (lo + LIM_BLOCK - 1) / LIM_BLOCK, blk1 = (t + 1) / LIM_BLOCK;  // whole blocks inside it: [blk0, blk1)
    float m = 0.0f;
    if (blk0 >= blk1) {
        for (uint64_t i = lo; i <= t; i++) m = fmaxf(m, J.v[i]);
    } else {
        for (uint64_t i = lo; i < blk0 * LIM_BLOCK; i++) m = fmaxf(m, J.v[i]);
        for (uint64_t b = blk0; b < blk1; b++) m = fmaxf(m, J.bm[b]);
        for (uint64_t i = blk1 * LIM_BLOCK; i <= t; i++) m = fmaxf(m, J.v[i]);
    }
    J.a[t] = m > 1.0f ? 1.0 / ((double)m + DBL_EPSILON) : 1.0;  // threshold 1 (limiter.rs:148-152)
}

__global__ __launch_bounds__(DYN_THREADS) void lim_release_summary_kernel(const LimJob *__restrict__ jobs) {
    const LimJob J = jobs[blockIdx.y];
    const uint64_t N = J.n + J.attack, c = (uint64_t)blockIdx.x * DYN_THREADS + threadIdx.x, t0 = c * LIM_CHUNK;
    if (t0 >= N) return;
    const uint64_t t1 = t0 + LIM_CHUNK < N ? t0 + LIM_CHUNK : N;
    const double a = 1.0 - J.slew;
    double A = 1.0, D = 0.0, C = INFINITY;
    for (uint64_t t = t0; t < t1; t++) {
        const double p = J.a[t], d = J.slew * p;
        C = fmin(p, a * C + d);
        D = a * D + d;
        A = a * A;
    }
    J.sum[4 * c] = A;
    J.sum[4 * c + 1] = D;
    J.sum[4 * c + 2] = C;
}

__global__ void lim_release_carry_kernel(const LimJob *__restrict__ jobs, uint32_t n_jobs) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_jobs) return;
    const LimJob J = jobs[j];
    const uint64_t N = J.n + J.attack, nc = (N + LIM_CHUNK - 1) / LIM_CHUNK;
    double y = 1.0;  // ExponentialRelease::new: initial_value 1
    for (uint64_t c = 0; c < nc; c++) {
        J.sum[4 * c + 3] = y;
        y = fmin(J.sum[4 * c + 2], J.sum[4 * c] * y + J.sum[4 * c + 1]);
    }
}

__global__ __launch_bounds__(DYN_THREADS) void lim_release_replay_kernel(const LimJob *__restrict__ jobs) {
    const LimJob J = jobs[blockIdx.y];
    const uint64_t N = J.n + J.attack, c = (uint64_t)blockIdx.x * DYN_THREADS + threadIdx.x, t0 = c * LIM_CHUNK;
    if (t0 >= N) return;
    const uint64_t t1 = t0 + LIM_CHUNK < N ? t0 + LIM_CHUNK : N;
    double y = J.sum[4 * c + 3];
    for (uint64_t t = t0; t < t1; t++) {
        const double p = J.a[t];
        y = fmin(p, fma(p - y, J.slew, y));  // ExponentialRelease::step (limiter.rs:38-42)
        J.a[t] = y;
    }
}

// BoxSum::read(len) after the write of step t (envelope.rs:62-70), from the running sums S of every period (see the head comment)
__device__ __forceinline__ double box_read(const double *__restrict__ S, uint32_t t, uint32_t len) {
    const uint32_t P = len + 1, k = (t + 1) / P, j = (t + 1) - k * P;
    const double prev = t >= len ? S[t - len] : (t + 1 == len ? 0.0 : (double)(t + 2));
    if (j == len) return S[t] - prev;
    const double W = k ? S[(size_t)k * P - 2] : (double)P;
    return (S[t] + W) - prev;
}

// layer LAYER's running sums: src = the release output (LAYER 0) or the sums of the layer below
template <int LAYER>
__global__ __launch_bounds__(DYN_THREADS) void lim_box_cum_kernel(const LimJob *__restrict__ jobs) {
    const LimJob J = jobs[blockIdx.y];
    const uint32_t N = (uint32_t)(J.n + J.attack), len = J.box_len[LAYER], P = len + 1;
    const uint64_t k = (uint64_t)blockIdx.x * DYN_THREADS + threadIdx.x;
    if (k * P > (uint64_t)N) return;  // period k starts at step k P - 1 (period 0 at step 0)
    const double *__restrict__ src = (LAYER & 1) ? J.b : J.a;
    double *__restrict__ dst = (LAYER & 1) ? J.a : J.b;
    const uint32_t t0 = k ? (uint32_t)k * P - 1 : 0;
    const uint64_t t1_ = k * P + len;
    const uint32_t t1 = t1_ < N ? (uint32_t)t1_ : N;
    const uint32_t len_in = LAYER ? J.box_len[LAYER ? LAYER - 1 : 0] : 1;
    const double mul = 1.0 / (double)len_in;  // BoxFilter::multiplier
    double s = 0.0;
    for (uint32_t t = t0; t < t1; t++) {
        const double x = LAYER ? box_read(src, t, len_in) * mul : src[t];
        s = s + x;
        dst[t] = s;
    }
}

__global__ __launch_bounds__(DYN_THREADS) void lim_apply_kernel(const LimJob *__restrict__ jobs) {
    const LimJob J = jobs[blockIdx.y];
    const uint64_t b0 = (uint64_t)blockIdx.x * (DYN_THREADS * DYN_ITEMS);
    if (b0 >= J.n) return;
    const uint32_t len = J.box_len[2];
    const double mul = 1.0 / (double)len;
    float mn = 1.0f;
    uint32_t ne = 0;
    for (uint32_t k = 0; k < DYN_ITEMS; k++) {
        const uint64_t i = b0 + k * DYN_THREADS + threadIdx.x;
        if (i >= J.n) break;
        const double g = fmin(box_read(J.b, (uint32_t)i + J.attack, len) * mul, 1.0);
        const float gf = (float)g;
        J.gain_seq[i] = gf;
        for (uint32_t c = 0; c < J.n_ch; c++) {
            const float y = J.gain * J.x[c * J.x_stride + i];
            J.aud[c * J.y_stride + i] = (float)clamp1((double)y * g);
        }
        mn = fminf(mn, gf);
        ne += gf != 1.0f;
    }
    block_reduce<false>(mn, ne, J.min_bits, J.cnt);  // (gains lie in [0, 1])
}

inline uint32_t blocks_for(uint64_t items) { return (uint32_t)((items + DYN_THREADS - 1) / DYN_THREADS); }

}  // namespace

hipError_t launch_dyn_apply(const DynApplyJob *d_jobs, uint32_t n_jobs, uint64_t max_n, hipStream_t s) {
    if (!n_jobs || !max_n) return hipSuccess;
    hipLaunchKernelGGL(dyn_apply_kernel, dim3(blocks_for((max_n + DYN_ITEMS - 1) / DYN_ITEMS), n_jobs), dim3(DYN_THREADS), 0, s, d_jobs);
    return hipGetLastError();
}

hipError_t launch_limiter(const LimJob *h_jobs, const LimJob *d_jobs, uint32_t n_jobs, hipStream_t s) {
    if (!n_jobs) return hipSuccess;
    uint64_t max_N = 0, max_n = 0, max_per[3] = {0, 0, 0};
    for (uint32_t j = 0; j < n_jobs; j++) {
        const uint64_t N = h_jobs[j].n + h_jobs[j].attack;
        max_N = N > max_N ? N : max_N;
        max_n = h_jobs[j].n > max_n ? h_jobs[j].n : max_n;
        for (int l = 0; l < 3; l++) {
            const uint64_t per = N / (h_jobs[j].box_len[l] + 1) + 1;
            max_per[l] = per > max_per[l] ? per : max_per[l];
        }
    }
    const dim3 thr(DYN_THREADS);
    const uint64_t max_chunks = (max_N + LIM_CHUNK - 1) / LIM_CHUNK;
    hipLaunchKernelGGL(lim_absmax_kernel, dim3(blocks_for(max_N), n_jobs), thr, 0, s, d_jobs);
    hipLaunchKernelGGL(lim_peak_kernel, dim3(blocks_for(max_N), n_jobs), thr, 0, s, d_jobs);
    hipLaunchKernelGGL(lim_release_summary_kernel, dim3(blocks_for(max_chunks), n_jobs), thr, 0, s, d_jobs);
    hipLaunchKernelGGL(lim_release_carry_kernel, dim3((n_jobs + 63) / 64), dim3(64), 0, s, d_jobs, n_jobs);
    hipLaunchKernelGGL(lim_release_replay_kernel, dim3(blocks_for(max_chunks), n_jobs), thr, 0, s, d_jobs);
    hipLaunchKernelGGL(lim_box_cum_kernel<0>, dim3(blocks_for(max_per[0]), n_jobs), thr, 0, s, d_jobs);
    hipLaunchKernelGGL(lim_box_cum_kernel<1>, dim3(blocks_for(max_per[1]), n_jobs), thr, 0, s, d_jobs);
    hipLaunchKernelGGL(lim_box_cum_kernel<2>, dim3(blocks_for(max_per[2]), n_jobs), thr, 0, s, d_jobs);
    hipLaunchKernelGGL(lim_apply_kernel, dim3(blocks_for((max_n + DYN_ITEMS - 1) / DYN_ITEMS), n_jobs), thr, 0, s, d_jobs);
    return hipGetLastError();
}

}  // namespace th
