// kernels_meter.hip — the true peak of a batch of channels (th_tm_get_loudness_meters): the largest |y| over the F phases of a
// 49-tap polyphase interpolator (host_math.h true_peak_filter; libebur128's true-peak mode restated), F = 4 below 96 kHz, 2 below
// 192 kHz.  y_f[i] = sum_d c x[i - d] for every sample i of the channel, causal from zero history, nothing behind the last sample.
//
// One workgroup per chunk of TP_CHUNK samples: the chunk and the T - 1 samples in front of it (T = 12 taps per phase at F = 4, 24 at
// F = 2; zeros in front of the channel) go to LDS, by 16-byte loads where the channel is 16-byte aligned.  A thread takes TP_RUN
// consecutive outputs and keeps the last T samples in registers: one LDS read per sample feeds the 36 (24) multiply-adds of that
// sample, the loop over the run is unrolled so that the window is renamed, not moved.  TP_RUN is odd, so the lanes' reads at a
// stride of TP_RUN words hit 32 different banks.  Each phase is one fmaf chain in ascending delay starting from 0, with f32
// coefficients (kernel arguments: scalar registers); the running fmaxf of |y| ignores NaN as abs_max does.  One atomicMax per
// workgroup on the bit pattern (|y| >= 0: the patterns order like unsigned integers).  The tail chunk of a channel runs the same
// step in a rolled loop over the outputs it has.  (Built with -ffp-contract=off: the chains are the explicit fmaf calls only.)
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace th {

void true_peak_coef(uint32_t factor, TruePeakCoef *out) {
    *out = TruePeakCoef{};
    double c[TRUE_PEAK_TAPS];
    uint32_t ph[TRUE_PEAK_TAPS], dl[TRUE_PEAK_TAPS];
    const uint32_t n = true_peak_filter(factor, c, ph, dl), T = factor == 4 ? 12 : 24;
    for (uint32_t k = 0; k < n; k++) {
        if (ph[k] == 0) {
            out->c0 = (float)c[k];
            out->d0 = dl[k];
        } else if (dl[k] < T && (ph[k] - 1) * T + dl[k] < 36) {
            out->c[(ph[k] - 1) * T + dl[k]] = (float)c[k];
        }
    }
}

namespace {

template <int F>
struct TpShape {
    static constexpr int T = F == 4 ? 12 : 24;   // taps of a phase 1 .. F - 1; the halo is T - 1 samples
    static constexpr int D0 = F == 4 ? 6 : 12;   // phase 0: the sample itself, delayed
    static constexpr int HP = T;                 // floats in front of the chunk in LDS (a multiple of 4)
};

// one output: the window moves on by sample x, every phase runs its chain, m takes the largest |y|
template <int F>
__device__ __forceinline__ void tp_step(const TruePeakCoef &K, float (&w)[TpShape<F>::T], float x, float &m) {
    constexpr int T = TpShape<F>::T;
#pragma unroll
    for (int d = T - 1; d > 0; d--) w[d] = w[d - 1];
    w[0] = x;
#pragma unroll
    for (int p = 0; p < F - 1; p++) {
        float a = 0.0f;
#pragma unroll
        for (int d = 0; d < T; d++) a = fmaf(K.c[p * T + d], w[d], a);
        m = fmaxf(m, fabsf(a));
    }
    m = fmaxf(m, fabsf(fmaf(K.c0, w[TpShape<F>::D0], 0.0f)));
}

template <int F>
__global__ __launch_bounds__(TP_THREADS) void true_peak_kernel(const TruePeakJob *__restrict__ jobs, const TruePeakCoef K) {
    extern __shared__ __attribute__((aligned(16))) float tp_buf[];
    constexpr int T = TpShape<F>::T, HP = TpShape<F>::HP;
    const TruePeakJob job = jobs[blockIdx.y];
    if (blockIdx.x >= job.n_chunks) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t s = (uint64_t)blockIdx.x * TP_CHUNK;
    const uint32_t len = job.n - s < TP_CHUNK ? (uint32_t)(job.n - s) : TP_CHUNK;
    const float *__restrict__ wav = job.wav;
    if (tid < (uint32_t)HP) tp_buf[tid] = s ? wav[s - HP + tid] : 0.0f;  // (s > 0: s >= TP_CHUNK > HP)
    float *body = tp_buf + HP;
    if (job.aligned16) {  // s is a multiple of 4
        const uint32_t n4 = len >> 2;
        for (uint32_t q = tid; q < n4; q += TP_THREADS)
            *reinterpret_cast<float4 *>(body + 4 * q) = *reinterpret_cast<const float4 *>(wav + s + 4 * (uint64_t)q);
        if (tid < (len & 3u)) body[4 * n4 + tid] = wav[s + 4 * n4 + tid];
    } else {
        for (uint32_t i = tid; i < len; i += TP_THREADS) body[i] = wav[s + i];
    }
    for (uint32_t i = len + tid; i < TP_CHUNK; i += TP_THREADS) body[i] = 0.0f;
    __syncthreads();
    const float *p = body + tid * TP_RUN;
    float w[T];
#pragma unroll
    for (int k = 0; k < T - 1; k++) w[k] = p[-(k + 1)];
    w[T - 1] = 0.0f;
    float m = 0.0f;
    if (len == TP_CHUNK) {
#pragma unroll
        for (uint32_t r = 0; r < TP_RUN; r++) tp_step<F>(K, w, p[r], m);
    } else {
        const uint32_t first = tid * TP_RUN;
        const uint32_t cnt = first >= len ? 0u : (len - first < TP_RUN ? len - first : TP_RUN);
#pragma unroll 1
        for (uint32_t r = 0; r < cnt; r++) tp_step<F>(K, w, p[r], m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __syncthreads();  // (every read of the chunk is done: its first words carry the waves' maxima)
    if ((tid & 63u) == 0) tp_buf[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (uint32_t v = 1; v < TP_THREADS / 64; v++) m = fmaxf(m, tp_buf[v]);
        atomicMax(job.peak, __float_as_uint(m));
    }
}

}  // namespace

hipError_t launch_true_peak(const TruePeakJob *d_jobs, uint32_t n_jobs, uint32_t max_chunks, uint32_t factor, const TruePeakCoef &K,
                            hipStream_t s) {
    if (!n_jobs || !max_chunks) return hipSuccess;
    if (factor == 4) {
        const size_t lds = (size_t)(TpShape<4>::HP + TP_CHUNK) * sizeof(float);
        hipLaunchKernelGGL(true_peak_kernel<4>, dim3(max_chunks, n_jobs), dim3(TP_THREADS), lds, s, d_jobs, K);
    } else if (factor == 2) {
        const size_t lds = (size_t)(TpShape<2>::HP + TP_CHUNK) * sizeof(float);
        hipLaunchKernelGGL(true_peak_kernel<2>, dim3(max_chunks, n_jobs), dim3(TP_THREADS), lds, s, d_jobs, K);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace th
