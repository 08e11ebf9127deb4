// kernels_envelope.hip — the exact (min, max, mean, rms) envelope of a time range of resident audio at any pixel width
// (th_tm_get_envelopes) and its raster as a waveform lane (th_tm_render_waveform_figures): a segmented reduction over ragged columns, a
// column holding no sample or millions.  The job tables and the chunk grid are those of envelope_plan.h; -ffp-contract=off: the f64
// sums are plain additions of x and of the rounded product x x, and the lane's row mapping rounds every step (envelope_core.h).
//
//   envelope_reduce_kernel (dense requests).  One WAVE per chunk of ENV_CHUNK samples on the channel's absolute grid, clipped to the
//   request's [e[0], e[W]).  The wave finds the column that holds the chunk's first sample from the even spacing of the edges (a guess and
//   a step or two) and walks the columns that touch the chunk.  A column's samples inside the chunk are a SEGMENT: lane l takes the
//   segment's whole 16-byte quads qa + l, qa + l + 64, ... (aligned loads: the channel starts on a 16-byte boundary and the quads are
//   counted from sample 0; eight loads in flight, alternately into two accumulators that are added at the end), then at most one sample of the segment's ragged head and one of its tail; the 64 lanes' (min, max, sum, sum of squares) are folded
//   by a butterfly over lane distances 32, 16, ... 1, whose sums are the same in every lane.  A column inside the chunk is finished
//   and stored as one 16-byte store; the chunk's first and last column, where they reach beyond it, go to the partials.  No LDS, no
//   barrier, no atomics: the order of every sum is fixed by the edges and the chunk grid.
//   envelope_columns_kernel (every request).  A thread per column: an empty column holds sample max(e[j], 1) - 1; a sparse request's
//   column is walked in ascending order; a dense request's column that spans chunks adds its partials in ascending chunk order.
//   lane_span_kernel: a thread per column, envelope -> (y_top, y_bot) in 1/256 pixel (lane_span, as the host's
//   th_waveform_figure_span).  lane_raster_kernel: a thread per 16 output bytes (4 pixels), integer coverage and blend, one 16-byte
//   store on the staging buffer's 16-byte grid: a store-rate kernel.
// Pointers loaded from the tables are cast to the global address space.
#include <hip/hip_runtime.h>

#include "envelope_core.h"
#include "envelope_plan.h"
#include "kernels.h"

namespace th {

namespace {

struct EnvAcc {
    float mn, mx;
    double s, q;
};

__device__ __forceinline__ void env_add(EnvAcc &a, float x) {
    a.mn = fminf(a.mn, x);
    a.mx = fmaxf(a.mx, x);
    const double d = (double)x;
    a.s += d;
    a.q += d * d;
}

__device__ __forceinline__ void env_add4(EnvAcc &a, const float4 v) {
    env_add(a, v.x);
    env_add(a, v.y);
    env_add(a, v.z);
    env_add(a, v.w);
}

__device__ __forceinline__ void env_store(gptr<float> out, uint32_t j, const float r[4]) {
    *reinterpret_cast<gptr<float4>>(out + (size_t)j * 4) = make_float4(r[0], r[1], r[2], r[3]);
}

// samples [s0, s1) of x, s0 < s1, by the whole wave; every lane returns the same values
__device__ __forceinline__ EnvAcc env_segment(gptr<const float> x, uint64_t s0, uint64_t s1, uint32_t lane) {
    EnvAcc a{INFINITY, -INFINITY, 0.0, 0.0};
    const uint64_t qa = (s0 + 3) >> 2, qb = s1 >> 2;          // whole quads [qa, qb) when qa < qb
    const uint64_t h1 = min(qa << 2, s1);                     // the head: [s0, h1), at most 3 samples (the whole segment when it has no whole quad)
    const uint64_t t0 = qa < qb ? (qb << 2) : h1;             // the tail: [t0, s1), at most 3 samples
    if (qa < qb) {
        const gptr<const float4> x4 = reinterpret_cast<gptr<const float4>>(x);
        EnvAcc b{INFINITY, -INFINITY, 0.0, 0.0};  // the odd loads of a round: a second chain of additions beside the first
        uint64_t q = qa + lane;
        for (; q + 448 < qb; q += 512) {  // (a whole chunk is two such rounds)
            const float4 v0 = x4[q], v1 = x4[q + 64], v2 = x4[q + 128], v3 = x4[q + 192];
            const float4 v4 = x4[q + 256], v5 = x4[q + 320], v6 = x4[q + 384], v7 = x4[q + 448];
            env_add4(a, v0);
            env_add4(b, v1);
            env_add4(a, v2);
            env_add4(b, v3);
            env_add4(a, v4);
            env_add4(b, v5);
            env_add4(a, v6);
            env_add4(b, v7);
        }
        for (; q + 64 < qb; q += 128) {
            const float4 v0 = x4[q], v1 = x4[q + 64];
            env_add4(a, v0);
            env_add4(b, v1);
        }
        if (q < qb) env_add4(a, x4[q]);
        a.mn = fminf(a.mn, b.mn);
        a.mx = fmaxf(a.mx, b.mx);
        a.s += b.s;
        a.q += b.q;
    }
    if (s0 + lane < h1) env_add(a, x[s0 + lane]);
    if (t0 + lane < s1) env_add(a, x[t0 + lane]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a.mn = fminf(a.mn, __shfl_xor(a.mn, off));
        a.mx = fmaxf(a.mx, __shfl_xor(a.mx, off));
        a.s += __shfl_xor(a.s, off);
        a.q += __shfl_xor(a.q, off);
    }
    return a;
}

}  // namespace

__global__ __launch_bounds__(ENV_THREADS) void envelope_reduce_kernel(const EnvJob *__restrict__ jobs, uint32_t n_jobs, uint32_t n_units) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t unit = blockIdx.x * ENV_WAVES + (threadIdx.x >> 6);
    if (unit >= n_units) return;
    // the last job whose first_unit is at or below the unit (sparse jobs own no unit: a dense job behind them shares their first_unit)
    uint32_t jl = 0, jh = n_jobs;
    while (jh - jl > 1) {
        const uint32_t mid = (jl + jh) >> 1;
        if (jobs[mid].first_unit <= unit)
            jl = mid;
        else
            jh = mid;
    }
    const EnvJob job = jobs[jl];
    if (unit - job.first_unit >= job.n_chunks) return;
    const uint32_t kr = unit - job.first_unit;
    const uint64_t k = job.k0 + kr;
    const gptr<const uint64_t> e = as_global(job.edges);
    const gptr<const float> x = as_global(job.x);
    const gptr<float> out = as_global(job.out);
    const gptr<EnvPartial> part = as_global(job.part);
    const uint32_t W = job.W;
    const uint64_t e0 = job.e0, eW = job.eW;
    const uint64_t c0 = max(k * ENV_CHUNK, e0), c1 = min((k + 1) * ENV_CHUNK, eW);
    if (c0 >= c1) return;
    // the (non-empty) column that holds c0: the largest j with e[j] <= c0.  The edges are evenly spaced up to a rounding, so the
    // guess from the spacing is off by a column or two at the most: two dependent loads instead of a bisection's log2 W
    uint32_t j = (uint32_t)((double)(c0 - e0) * (double)W / (double)(eW - e0));
    j = min(j, W - 1);
    while (e[j] > c0) j--;       // (e[0] <= c0)
    while (e[j + 1] <= c0) j++;  // (c0 < e[W])
    uint64_t s0 = c0;
    bool first = true;
    while (s0 < c1) {
        const uint64_t ej = e[j], ej1 = e[j + 1];
        const uint64_t s1 = min(ej1, c1);
        const EnvAcc a = env_segment(x, s0, s1, lane);
        if (lane == 0) {
            if (s0 == ej && s1 == ej1) {  // the whole column
                float r[4];
                envelope_finish(a.mn, a.mx, a.s, a.q, ej1 - ej, r);
                env_store(out, j, r);
            } else {
                EnvPartial p;
                p.sum = a.s;
                p.sumsq = a.q;
                p.mn = a.mn;
                p.mx = a.mx;
                part[(size_t)kr * 2 + (first ? 0 : 1)] = p;
            }
        }
        first = false;
        s0 = s1;
        if (s0 >= c1) break;
        j++;
        while (j + 1 < W && e[j + 1] <= s0) j++;  // (empty columns; s0 < c1 <= e[W], so a non-empty one follows)
    }
}

__global__ __launch_bounds__(ENV_THREADS) void envelope_columns_kernel(const EnvJob *__restrict__ jobs, uint32_t n_jobs) {
    uint32_t jl = 0, jh = n_jobs;
    while (jh - jl > 1) {
        const uint32_t mid = (jl + jh) >> 1;
        if (jobs[mid].first_cblock <= blockIdx.x)
            jl = mid;
        else
            jh = mid;
    }
    const EnvJob job = jobs[jl];
    const uint32_t j = (blockIdx.x - job.first_cblock) * ENV_THREADS + threadIdx.x;
    if (j >= job.W) return;
    const gptr<const uint64_t> e = as_global(job.edges);
    const gptr<const float> x = as_global(job.x);
    const uint64_t e0 = e[j], e1 = e[j + 1];
    float r[4];
    if (e1 == e0) {
        const float v = x[(e0 > 0 ? e0 : 1) - 1];
        r[0] = r[1] = r[2] = v;
        r[3] = fabsf(v);
    } else if (job.n_chunks == 0) {
        EnvAcc a{INFINITY, -INFINITY, 0.0, 0.0};
        for (uint64_t i = e0; i < e1; i++) env_add(a, x[i]);
        envelope_finish(a.mn, a.mx, a.s, a.q, e1 - e0, r);
    } else {
        const uint64_t ka = e0 / ENV_CHUNK, kb = (e1 - 1) / ENV_CHUNK;
        if (ka == kb) return;  // (the reduction finished it)
        const gptr<const EnvPartial> part = as_global(job.part);
        const uint64_t first = job.e0;
        EnvAcc a{INFINITY, -INFINITY, 0.0, 0.0};
        for (uint64_t k = ka; k <= kb; k++) {
            const uint64_t c0 = max(k * ENV_CHUNK, first);
            const EnvPartial p = part[(size_t)(k - job.k0) * 2 + (e0 <= c0 ? 0 : 1)];
            a.mn = fminf(a.mn, p.mn);
            a.mx = fmaxf(a.mx, p.mx);
            a.s += p.sum;
            a.q += p.sumsq;
        }
        envelope_finish(a.mn, a.mx, a.s, a.q, e1 - e0, r);
    }
    env_store(as_global(job.out), j, r);
}

__global__ __launch_bounds__(ENV_THREADS) void lane_span_kernel(const LaneSpanJob *__restrict__ jobs, uint32_t n_jobs) {
    uint32_t jl = 0, jh = n_jobs;
    while (jh - jl > 1) {
        const uint32_t mid = (jl + jh) >> 1;
        if (jobs[mid].first_block <= blockIdx.x)
            jl = mid;
        else
            jh = mid;
    }
    const LaneSpanJob job = jobs[jl];
    const uint32_t j = (blockIdx.x - job.first_block) * ENV_THREADS + threadIdx.x;
    if (j >= job.W) return;
    const gptr<const float4> env = reinterpret_cast<gptr<const float4>>(as_global(job.env));
    const float4 c = env[j];
    const float col[4] = {c.x, c.y, c.z, c.w};
    float left[4] = {0.f, 0.f, 0.f, 0.f};
    if (j > 0) {
        const float4 l = env[j - 1];
        left[0] = l.x;
        left[1] = l.y;
        left[2] = l.z;
        left[3] = l.w;
    }
    int32_t yt = 0, yb = 0;
    if (!lane_span(col, j > 0 ? left : nullptr, job.out_h, job.amp_lo, job.amp_hi, job.thickness, &yt, &yb)) yt = yb = 0;
    *reinterpret_cast<gptr<int2>>(as_global(job.span) + (size_t)j * 2) = make_int2(yt, yb);
}

__global__ __launch_bounds__(ENV_THREADS) void lane_raster_kernel(const LaneRasterJob *__restrict__ jobs, uint32_t n_jobs) {
    uint32_t jl = 0, jh = n_jobs;
    while (jh - jl > 1) {
        const uint32_t mid = (jl + jh) >> 1;
        if (jobs[mid].first_block <= blockIdx.x)
            jl = mid;
        else
            jh = mid;
    }
    const LaneRasterJob job = jobs[jl];
    const uint32_t n_px = job.n_rows * job.out_w;  // (a part is at most TH_FIGURE_PIECE_BYTES)
    const uint32_t g = (blockIdx.x - job.first_block) * ENV_THREADS + threadIdx.x;
    const uint32_t pa = g * 4u;
    if (pa >= n_px) return;
    const uint32_t n_here = min(4u, n_px - pa);
    const gptr<const int2> span = reinterpret_cast<gptr<const int2>>(as_global(job.span));
    uint32_t row = pa / job.out_w, col = pa - row * job.out_w;
    uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        if (k < n_here) {
            const int2 s = span[col];
            const int32_t r0 = (int32_t)((job.j0 + row) * 256u);
            const int32_t cv = min(s.y, r0 + 256) - max(s.x, r0);
            const uint32_t cov = cv > 0 ? (uint32_t)cv : 0u;
            uint32_t px = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4; b++) {
                const uint32_t f = (job.fill >> (8 * b)) & 255u, bg = (job.background >> (8 * b)) & 255u;
                px |= ((f * cov + bg * (256u - cov) + 128u) >> 8) << (8 * b);
            }
            c[k] = px;
            if (++col == job.out_w) {
                col = 0;
                row++;
            }
        }
    }
    const gptr<uint8_t> dst = as_global(job.dst) + (size_t)g * 16;
    if (n_here == 4) {
        *reinterpret_cast<gptr<uint4>>(dst) = make_uint4(c[0], c[1], c[2], c[3]);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (k < n_here) reinterpret_cast<gptr<uint32_t>>(dst)[k] = c[k];
    }
}

hipError_t launch_envelope_reduce(const EnvJob *d_jobs, uint32_t n_jobs, uint32_t n_units, hipStream_t s) {
    if (n_jobs == 0 || n_units == 0) return hipSuccess;
    hipLaunchKernelGGL(envelope_reduce_kernel, dim3((n_units + ENV_WAVES - 1) / ENV_WAVES), dim3(ENV_THREADS), 0, s, d_jobs, n_jobs, n_units);
    return hipGetLastError();
}

hipError_t launch_envelope_columns(const EnvJob *d_jobs, uint32_t n_jobs, uint32_t n_cblocks, hipStream_t s) {
    if (n_jobs == 0 || n_cblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(envelope_columns_kernel, dim3(n_cblocks), dim3(ENV_THREADS), 0, s, d_jobs, n_jobs);
    return hipGetLastError();
}

hipError_t launch_lane_spans(const LaneSpanJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, hipStream_t s) {
    if (n_jobs == 0 || n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(lane_span_kernel, dim3(n_blocks), dim3(ENV_THREADS), 0, s, d_jobs, n_jobs);
    return hipGetLastError();
}

hipError_t launch_lane_raster(const LaneRasterJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, hipStream_t s) {
    if (n_jobs == 0 || n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(lane_raster_kernel, dim3(n_blocks), dim3(ENV_THREADS), 0, s, d_jobs, n_jobs);
    return hipGetLastError();
}

}  // namespace th
