// kernels_loudness.hip — K-weighted block energies (the momentary loudness series) and the per-channel sum of squares / peak
// of a batch of tracks: what StatCalculator::calc (dynamics/stats.rs:56-86) needs of the audio.  The gating that turns block
// energies into integrated LUFS is host arithmetic (host_math.cpp gated_loudness).
//
// The K-weighting is one 4th-order direct-form-II recurrence in f64 (libebur128's arithmetic, host_math.cpp k_weighting).  It is
// linear in (state, input): over a run of `len` samples S' = A^len S + z, z = the run from zero state.  So:
//   pass A  one wave per chunk (a 100 ms segment is n_sub chunks, LoudnessRate): the chunk goes to LDS; lane l runs its m samples from
//           zero state; an inclusive scan over the lanes combines them (z_l += A^(m 2^j) z_(l - 2^j)) into the chunk's zero-state
//           end state.  The same pass sums x^2 and max |x| of every sample.
//   pass B  one wave per channel: S_(i+1) = A^len_i S_i + e_i from chunk to chunk, serially; the start state of every chunk.
//   pass C  pass A again, with the chunk's start state folded into its first non-empty lane, so the scan gives every lane its true
//           start state; each lane re-runs its samples from it and sums y^2 (f64); one energy per chunk.
//   pass D  one thread per 400 ms block: E_k = sum_c w_c (the energies of segments k .. k + 3) / L (the loudness meter runs it again
//           over 30 segments: the short-term series, launch_loudness_blocks).
// The lanes' runs and y^2 sums are plain f64, as the sequential filter's.  Everything that multiplies a state by a power of A is
// double-double: A is far from normal (host_math.h), and those products in f64 put errors of 1e-9 .. 1e-5 into the energies of
// DC-heavy audio at 44.1 .. 192 kHz where the sequential filter's own rounding stays near 1e-12.  (Built with -ffp-contract=off:
// the double-double steps rely on exactly rounded products and sums.)
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace th {

namespace {

struct dd {
    double hi, lo;
};

__device__ __forceinline__ dd dd_add(dd a, dd b) {
    const double s = a.hi + b.hi, bb = s - a.hi, e = ((a.hi - (s - bb)) + (b.hi - bb)) + (a.lo + b.lo);
    const double h = s + e;
    return dd{h, e - (h - s)};
}

// acc + M x for a 4x4 double-double matrix M (LoudnessRate layout: [16][2], row-major) and a double-double 4-vector x
__device__ __forceinline__ void dd_matvec_add(const double (*__restrict__ M)[2], const dd x[4], dd acc[4]) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        double s = acc[r].hi, e = acc[r].lo;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const double mh = M[4 * r + c][0], ml = M[4 * r + c][1];
            const double p = mh * x[c].hi, pe = fma(mh, x[c].hi, -p) + (mh * x[c].lo + ml * x[c].hi);
            const double t = s + p, bb = t - s;
            e += ((s - (t - bb)) + (p - bb)) + pe;
            s = t;
        }
        const double h = s + e;
        acc[r] = dd{h, e - (h - s)};
    }
}

__device__ __forceinline__ double shfl_up_d(double v, int d) {
    return __shfl_up(v, (unsigned)d, 64);
}

// The chunk's samples in LDS: buf[off + i] = x[start + i], i < len, off = start & 3 (16-byte loads from 16-byte aligned addresses
// when the channel is 16-byte aligned).  With `stats`, also the wave's sum of x^2 (f64) and max |x| (NaN ignored, abs_max).
template <bool STATS>
__device__ __forceinline__ uint32_t load_chunk(const LoudJob &job, uint64_t start, uint32_t len, float *buf, double *ss, float *pk) {
    const uint32_t lane = threadIdx.x;
    const float *__restrict__ wav = job.wav;
    double acc = 0.0;
    float mx = 0.0f;
    uint32_t off = 0;
    if (job.aligned16) {
        off = (uint32_t)(start & 3);
        const uint64_t a0 = start - off, end = start + len;
        const uint64_t b0 = (start + 3) & ~(uint64_t)3, b1 = end & ~(uint64_t)3;  // whole float4s inside [start, end)
        if (b0 < b1) {
            const uint32_t n4 = (uint32_t)((b1 - b0) >> 2);
            for (uint32_t q = lane; q < n4; q += 64) {
                const float4 t = *reinterpret_cast<const float4 *>(wav + b0 + 4 * (uint64_t)q);
                *reinterpret_cast<float4 *>(buf + (b0 - a0) + 4 * q) = t;
                if (STATS) {
                    acc += ((double)t.x * (double)t.x + (double)t.y * (double)t.y) + ((double)t.z * (double)t.z + (double)t.w * (double)t.w);
                    mx = fmaxf(fmaxf(mx, fmaxf(fabsf(t.x), fabsf(t.y))), fmaxf(fabsf(t.z), fabsf(t.w)));
                }
            }
            // the up to 3 samples in front of b0 and behind b1
            if (lane < 8) {
                const uint64_t g = lane < 4 ? start + lane : b1 + (lane - 4);
                if ((lane < 4 ? g < b0 : g < end)) {
                    const float v = wav[g];
                    buf[g - a0] = v;
                    if (STATS) {
                        acc += (double)v * (double)v;
                        mx = fmaxf(mx, fabsf(v));
                    }
                }
            }
        } else {
            for (uint32_t i = lane; i < len; i += 64) {
                const float v = wav[start + i];
                buf[off + i] = v;
                if (STATS) {
                    acc += (double)v * (double)v;
                    mx = fmaxf(mx, fabsf(v));
                }
            }
        }
    } else {
        for (uint32_t i = lane; i < len; i += 64) {
            const float v = wav[start + i];
            buf[i] = v;
            if (STATS) {
                acc += (double)v * (double)v;
                mx = fmaxf(mx, fabsf(v));
            }
        }
    }
    if (STATS) {
        *ss = acc;
        *pk = mx;
    }
    return off;
}

// chunk i of a channel: [start, start + len) of the samples; len = 0: past the end
__device__ __forceinline__ void chunk_of(const LoudnessRate &R, const LoudJob &job, uint32_t i, uint64_t *start, uint32_t *len, int *w) {
    const uint32_t k = i / R.n_sub, j = i - k * R.n_sub;
    *w = j == R.n_sub - 1;
    *start = (uint64_t)k * R.s100 + (uint64_t)j * R.cl;
    const uint32_t l = *w ? R.cl_last : R.cl;
    *len = *start >= job.n ? 0u : (uint32_t)(job.n - *start < l ? job.n - *start : l);
}

// lane l's run within a chunk of len samples: [lo, lo + cnt)
__device__ __forceinline__ void lane_run(const LoudnessRate &R, int w, uint32_t len, uint32_t lane, uint32_t *lo, uint32_t *cnt) {
    const uint32_t e = R.e_lane[w];
    if (lane < e) {
        *lo = 0;
        *cnt = 0;
    } else if (lane == e) {
        *lo = 0;
        *cnt = R.r[w];
    } else {
        *lo = len - (64 - lane) * R.m;
        *cnt = R.m;
    }
}

// the lane's run from zero state -> (v1, v2, v3, v4)
__device__ __forceinline__ void zero_state_run(const double a[5], const float *x, uint32_t cnt, dd z[4]) {
    double v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
    for (uint32_t i = 0; i < cnt; i++) {
        const double v0 = (double)x[i] - a[1] * v1 - a[2] * v2 - a[3] * v3 - a[4] * v4;
        v4 = v3;
        v3 = v2;
        v2 = v1;
        v1 = v0;
    }
    z[0] = dd{v1, 0.0};
    z[1] = dd{v2, 0.0};
    z[2] = dd{v3, 0.0};
    z[3] = dd{v4, 0.0};
}

// inclusive scan of the lanes' runs: lane l ends with the state after its run, from the chunk's start state (pass C) or zero (pass A).
// Exact for every lane at or past the first non-empty one: a combined right part [l - 2^j + 1, l] holds only full lanes whenever its
// left part can be non-zero (the lanes in front of the first non-empty lane hold 0).
__device__ __forceinline__ void lane_scan(const LoudnessRate &R, dd z[4]) {
    const uint32_t lane = threadIdx.x;
#pragma unroll 1
    for (int j = 0; j < 6; j++) {
        const int d = 1 << j;
        dd y[4];
#pragma unroll
        for (int r = 0; r < 4; r++) y[r] = dd{shfl_up_d(z[r].hi, d), shfl_up_d(z[r].lo, d)};
        if (lane >= (uint32_t)d) dd_matvec_add(R.scan[j], y, z);
    }
}

}  // namespace

__global__ __launch_bounds__(64) void loudness_zero_state_kernel(const LoudJob *__restrict__ jobs, const LoudnessRate *__restrict__ rates) {
    extern __shared__ float lds_buf[];
    const LoudJob job = jobs[blockIdx.y];
    const uint32_t i = blockIdx.x;
    if (i >= job.n_chunks) return;
    const LoudnessRate &R = rates[job.rate];
    uint64_t start;
    uint32_t len;
    int w;
    chunk_of(R, job, i, &start, &len, &w);
    if (!len) return;
    double ss;
    float pk;
    const uint32_t off = load_chunk<true>(job, start, len, lds_buf, &ss, &pk);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ss += __shfl_xor(ss, o, 64);
        pk = fmaxf(pk, __shfl_xor(pk, o, 64));
    }
    if (threadIdx.x == 0) {
        atomicAdd(job.sumsq, ss);
        atomicMax(job.peak, __float_as_uint(pk));  // |x| >= 0: its bit patterns order like unsigned integers
    }
    if (i >= job.n_fchunks) return;  // (only the sums: no 400 ms block reaches this chunk)
    __syncthreads();
    uint32_t lo, cnt;
    lane_run(R, w, len, threadIdx.x, &lo, &cnt);
    dd z[4];
    zero_state_run(R.a, lds_buf + off + lo, cnt, z);
    lane_scan(R, z);
    if (threadIdx.x == 63) {
        double *dst = job.z + 8 * (uint64_t)i;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            dst[r] = z[r].hi;
            dst[4 + r] = z[r].lo;
        }
    }
}

// serial over the chunks of one channel; every lane keeps the same state, lane t of a group of 64 chunks stores chunk t's start state
__global__ __launch_bounds__(64) void loudness_carry_kernel(const LoudJob *__restrict__ jobs, const LoudnessRate *__restrict__ rates) {
    const LoudJob job = jobs[blockIdx.x];
    const LoudnessRate &R = rates[job.rate];
    const uint32_t lane = threadIdx.x;
    dd S[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    for (uint32_t base = 0; base < job.n_fchunks; base += 64) {
        const uint32_t n = job.n_fchunks - base < 64 ? job.n_fchunks - base : 64;
        double e[8];
#pragma unroll
        for (int r = 0; r < 8; r++) e[r] = lane < n ? job.z[8 * (uint64_t)(base + lane) + r] : 0.0;
        dd mine[4];
        for (uint32_t t = 0; t < n; t++) {
            dd et[4];
#pragma unroll
            for (int r = 0; r < 4; r++) et[r] = dd{__shfl(e[r], (int)t, 64), __shfl(e[4 + r], (int)t, 64)};
            if (lane == t) {
#pragma unroll
                for (int r = 0; r < 4; r++) mine[r] = S[r];
            }
            const uint32_t k = base + t;
            const int w = (k % R.n_sub) == R.n_sub - 1;
            dd_matvec_add(R.step[w], S, et);  // et = A^len S + e
#pragma unroll
            for (int r = 0; r < 4; r++) S[r] = et[r];
        }
        if (lane < n) {
            double *dst = job.z + 8 * (uint64_t)(base + lane);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                dst[r] = mine[r].hi;
                dst[4 + r] = mine[r].lo;
            }
        }
    }
}

__global__ __launch_bounds__(64) void loudness_energy_kernel(const LoudJob *__restrict__ jobs, const LoudnessRate *__restrict__ rates) {
    extern __shared__ float lds_buf[];
    const LoudJob job = jobs[blockIdx.y];
    const uint32_t i = blockIdx.x;
    if (i >= job.n_fchunks) return;
    const LoudnessRate &R = rates[job.rate];
    uint64_t start;
    uint32_t len;
    int w;
    chunk_of(R, job, i, &start, &len, &w);
    const uint32_t off = load_chunk<false>(job, start, len, lds_buf, nullptr, nullptr);
    dd S[4];
    const double *src = job.z + 8 * (uint64_t)i;
#pragma unroll
    for (int r = 0; r < 4; r++) S[r] = dd{src[r], src[4 + r]};
    __syncthreads();
    const uint32_t lane = threadIdx.x;
    uint32_t lo, cnt;
    lane_run(R, w, len, lane, &lo, &cnt);
    const float *x = lds_buf + off + lo;
    dd z[4];
    zero_state_run(R.a, x, cnt, z);
    if (lane == R.e_lane[w]) dd_matvec_add(R.rpow[w], S, z);  // the first non-empty lane starts from S
    lane_scan(R, z);
    double v1 = shfl_up_d(z[0].hi, 1), v2 = shfl_up_d(z[1].hi, 1), v3 = shfl_up_d(z[2].hi, 1), v4 = shfl_up_d(z[3].hi, 1);
    if (lane == R.e_lane[w]) {
        v1 = S[0].hi;
        v2 = S[1].hi;
        v3 = S[2].hi;
        v4 = S[3].hi;
    }
    const double *a = R.a, *b = R.b;
    double acc = 0.0;
    for (uint32_t t = 0; t < cnt; t++) {
        const double v0 = (double)x[t] - a[1] * v1 - a[2] * v2 - a[3] * v3 - a[4] * v4;
        const double y = b[0] * v0 + b[1] * v1 + b[2] * v2 + b[3] * v3 + b[4] * v4;
        acc += y * y;
        v4 = v3;
        v3 = v2;
        v2 = v1;
        v1 = v0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) job.q[i] = acc;
}

// span: segments per block (4: momentary, 30: short-term); t.L = span s100
__global__ __launch_bounds__(256) void loudness_blocks_kernel(const LoudTrackJob *__restrict__ tjobs, uint32_t span) {
    const LoudTrackJob t = tjobs[blockIdx.y];
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= t.n_blocks) return;
    double e = 0.0;
    for (uint32_t c = 0; c < t.n_ch; c++) {
        const double wc = t.w[c < 8 ? c : 7];
        if (wc == 0.0) continue;
        const double *q = t.q + (uint64_t)c * t.n_fchunks + k * t.n_sub;
        double s = 0.0;
        for (uint32_t i = 0; i < span * t.n_sub; i++) s += q[i];
        e += wc * s;
    }
    t.out[k] = e / (double)t.L;
}

hipError_t launch_loudness(const LoudJob *d_jobs, uint32_t n_jobs, uint32_t max_chunks, uint32_t max_fchunks, const LoudnessRate *d_rates,
                           uint32_t lds_floats, const LoudTrackJob *d_tjobs, uint32_t n_tracks, uint64_t max_blocks, hipStream_t s) {
    if (!n_jobs) return hipSuccess;
    const size_t lds = (size_t)lds_floats * sizeof(float);
    if (max_chunks) hipLaunchKernelGGL(loudness_zero_state_kernel, dim3(max_chunks, n_jobs), dim3(64), lds, s, d_jobs, d_rates);
    if (max_fchunks) {
        hipLaunchKernelGGL(loudness_carry_kernel, dim3(n_jobs), dim3(64), 0, s, d_jobs, d_rates);
        hipLaunchKernelGGL(loudness_energy_kernel, dim3(max_fchunks, n_jobs), dim3(64), lds, s, d_jobs, d_rates);
    }
    if (max_blocks && n_tracks)
        hipLaunchKernelGGL(loudness_blocks_kernel, dim3((uint32_t)((max_blocks + 255) / 256), n_tracks), dim3(256), 0, s, d_tjobs, 4u);
    return hipGetLastError();
}

hipError_t launch_loudness_blocks(const LoudTrackJob *d_tjobs, uint32_t n_tracks, uint64_t max_blocks, uint32_t span, hipStream_t s) {
    if (max_blocks && n_tracks)
        hipLaunchKernelGGL(loudness_blocks_kernel, dim3((uint32_t)((max_blocks + 255) / 256), n_tracks), dim3(256), 0, s, d_tjobs, span);
    return hipGetLastError();
}

}  // namespace th
