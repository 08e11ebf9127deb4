// kernels_figure.hip — a region of a resident u16 image resampled to any pixel size (th_tm_render_figures): the separable Lanczos3
// of the LOD tiles with host-tabulated, normalised f64 taps (figure_plan.h), two launches per piece whatever the number of requests.
// Every output adds pixel x tap in ascending tap order from 0.0, a multiplication then an addition (-ffp-contract=off), and rounds
// half up once per pass: bit-identical to lod_hpass_kernel / lod_vpass_kernel and to the definition in include/thesia_amd.h.
//
//   figure_hpass_kernel.  One launch over a ragged table of jobs (a job = the source rows one band of one request needs); block b
//   finds its job by first_block.  A block takes FIG_ROWS rows and a run of `oc` output columns.  It stages the columns the run's taps
//   span into LDS with 8-byte loads along the rows (the rows of a resident image start on 128-byte boundaries), [column][row], so a
//   lane owns a ROW: the wave reads one column as 128 contiguous bytes and the tap is a wave-uniform scalar.  A wave walks the union
//   of the windows of FIG_GROUP consecutive outputs once (one LDS read, FIG_GROUP multiply-adds; outside an output's own window the
//   tap is 0.0, and acc + 0.0 * v == acc exactly for a finite pixel; the taps of 64 columns are fetched by the 64 lanes at once
//   and read back by v_readlane), the four waves take four such groups (a pass), and the block
//   takes its run in passes.  Where the run's whole span fits FIG_SPAN columns it is staged once for all passes (upscaling: the span
//   is smaller than the run; moderate reduction: oc shrinks, figure_pick_oc); where it does not (an overview: a thousand taps per
//   output) a pass stages its own span in steps of FIG_SPAN columns with the accumulators carried.  Results go through LDS so that
//   the stores run along the rows of the intermediate.
//   figure_vpass_kernel.  Over the intermediate, fused with the output stage: a thread makes 16 output bytes (4 RGBA pixels through
//   the colormap, or 8 u16) of the part's rows, flipped, and stores them as one 16-byte store on the staging buffer's 16-byte grid;
//   neighbouring lanes read neighbouring columns of the intermediate.  The LUT sits in LDS when it has at most 1024 colours.
// Pointers loaded from the tables are cast to the global address space.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace th {

namespace {

__device__ __forceinline__ uint32_t fig_round(double acc) {
    double v = floor(acc + 0.5);
    if (v < 0.0) v = 0.0;
    if (v > 65535.0) v = 65535.0;
    return (uint32_t)v;
}

// lane j's value of x as a wave-uniform scalar (j wave-uniform)
__device__ __forceinline__ double fig_bcast(double x, uint32_t j) {
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, (int)j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), (int)j);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// the job of this block: the last one whose first_block is at or below the block index
template <class Job>
__device__ __forceinline__ uint32_t fig_find_job(const Job *__restrict__ jobs, uint32_t n_jobs) {
    uint32_t lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (jobs[mid].first_block <= blockIdx.x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t fig_colour_index(uint32_t v, uint32_t cm1) {  // (v (C - 1) + 32767) / 65535, as the tile raster
    const uint32_t x = __umul24(v, cm1) + 32767u;
    return (x + 1u + (x >> 16)) >> 16;
}

}  // namespace

__global__ __launch_bounds__(FIG_THREADS) void figure_hpass_kernel(const FigHJob *__restrict__ jobs, uint32_t n_jobs) {
    __shared__ uint16_t tile[FIG_SPAN * FIG_COL_PITCH];  // [column][row]
    __shared__ uint16_t outt[FIG_ROWS * FIG_OUT_PITCH];  // [row][output of the run]
    const FigHJob job = jobs[fig_find_job(jobs, n_jobs)];
    const uint32_t local = blockIdx.x - job.first_block;
    const uint32_t rb = local / job.n_cblocks, cb = local - rb * job.n_cblocks;
    const uint32_t o0 = cb * job.oc, r0 = rb * FIG_ROWS;
    if (o0 >= job.ax.n_out || r0 >= job.n_rows) return;  // (no such block in a table built by plan_figures)
    const uint32_t n_o = min(job.oc, job.ax.n_out - o0), n_r = min(FIG_ROWS, job.n_rows - r0);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const gptr<const int32_t> a_start = as_global(job.ax.start), a_count = as_global(job.ax.count);
    const gptr<const double> a_w = as_global(job.ax.w);
    const gptr<const uint16_t> src = as_global(job.src) + (size_t)(job.y_lo + r0) * job.src_pitch;

    // columns [c0, c1) of the block's rows into the tile; c0 is a multiple of 4 and c1 <= the image's width <= src_pitch
    auto stage = [&](int32_t c0, int32_t c1) {
        constexpr uint32_t RPW = FIG_ROWS / (FIG_THREADS / 64);  // rows of one wave: all their loads are issued before the first LDS write
        const uint32_t nq = (uint32_t)(c1 - c0 + 3) >> 2;
        for (uint32_t q = lane; q < nq; q += 64) {
            uint2 v[RPW];
#pragma unroll
            for (uint32_t i = 0; i < RPW; i++) {
                const uint32_t row = wv + i * (FIG_THREADS / 64);
                v[i] = make_uint2(0u, 0u);
                if (row < n_r) v[i] = *reinterpret_cast<gptr<const uint2>>(src + (size_t)row * job.src_pitch + (uint32_t)c0 + 4u * q);
            }
#pragma unroll
            for (uint32_t i = 0; i < RPW; i++) {
                uint16_t *t = tile + (4u * q) * FIG_COL_PITCH + wv + i * (FIG_THREADS / 64);
                t[0] = (uint16_t)v[i].x;
                t[FIG_COL_PITCH] = (uint16_t)(v[i].x >> 16);
                t[2 * FIG_COL_PITCH] = (uint16_t)v[i].y;
                t[3 * FIG_COL_PITCH] = (uint16_t)(v[i].y >> 16);
            }
        }
    };

    const int32_t b0 = __builtin_amdgcn_readfirstlane(a_start[o0]) & ~3;
    const int32_t b1 = __builtin_amdgcn_readfirstlane(a_start[o0 + n_o - 1] + a_count[o0 + n_o - 1]);
    const bool whole = b1 - b0 <= (int32_t)FIG_SPAN;
    if (whole) {
        stage(b0, b1);
        __syncthreads();
    }
    for (uint32_t pbase = 0; pbase < n_o; pbase += FIG_PASS) {
        const uint32_t pn = min(FIG_PASS, n_o - pbase);
        int32_t p0 = b0, p1 = b1;
        if (!whole) {
            p0 = __builtin_amdgcn_readfirstlane(a_start[o0 + pbase]) & ~3;
            p1 = __builtin_amdgcn_readfirstlane(a_start[o0 + pbase + pn - 1] + a_count[o0 + pbase + pn - 1]);
        }
        // this wave's group of the pass: outputs og .. og + ng - 1
        const uint32_t gfirst = pbase + FIG_GROUP * wv;
        const uint32_t ng = gfirst < n_o ? min(FIG_GROUP, n_o - gfirst) : 0u;
        const uint32_t og = o0 + gfirst;
        int32_t st[FIG_GROUP], cn[FIG_GROUP];
        gptr<const double> wrow[FIG_GROUP];
        int32_t g_lo = 0, g_hi = 0;
#pragma unroll
        for (uint32_t k = 0; k < FIG_GROUP; k++) {
            const uint32_t o = min(og + k, job.ax.n_out - 1u);
            st[k] = __builtin_amdgcn_readfirstlane(a_start[o]);
            const int32_t n = __builtin_amdgcn_readfirstlane(a_count[o]);
            cn[k] = k < ng ? n : 0;
            wrow[k] = a_w + (size_t)o * job.ax.max_taps;
            if (k == 0) g_lo = st[0];
            g_hi = max(g_hi, st[k] + cn[k]);
        }
        if (ng == 0) g_hi = g_lo;
        double acc[FIG_GROUP];
#pragma unroll
        for (uint32_t k = 0; k < FIG_GROUP; k++) acc[k] = 0.0;
        for (int32_t c0 = p0; c0 < p1; c0 += (int32_t)FIG_SPAN) {
            const int32_t c1 = min(c0 + (int32_t)FIG_SPAN, p1);
            if (!whole) {
                __syncthreads();  // (every wave has left the last step's columns)
                stage(c0, c1);
                __syncthreads();
            }
            const int32_t lo = max(c0, g_lo), hi = min(c1, g_hi);
            // 64 columns at a time: lane l fetches the group's four taps of column cb + l (0.0 outside an output's window) in one
            // round of vector loads, and the walk reads them back lane by lane as wave-uniform scalars (v_readlane).  A tap loaded
            // where it is used, one scalar load per column and output, made the walk wait a memory latency per column.
            for (int32_t cb = lo; cb < hi; cb += 64) {
                double wl[FIG_GROUP];
#pragma unroll
                for (uint32_t k = 0; k < FIG_GROUP; k++) {
                    const int32_t rel = cb + (int32_t)lane - st[k];
                    wl[k] = (uint32_t)rel < (uint32_t)cn[k] ? wrow[k][rel] : 0.0;
                }
                const uint32_t nb = (uint32_t)min(64, hi - cb);
                const uint16_t *col = tile + (uint32_t)(cb - c0) * FIG_COL_PITCH + lane;
                for (uint32_t j = 0; j < nb; j++) {
                    const double v = (double)col[j * FIG_COL_PITCH];
#pragma unroll
                    for (uint32_t k = 0; k < FIG_GROUP; k++) acc[k] += fig_bcast(wl[k], j) * v;
                }
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < FIG_GROUP; k++)
            if (k < ng) outt[lane * FIG_OUT_PITCH + gfirst + k] = (uint16_t)fig_round(acc[k]);
    }
    __syncthreads();
    const gptr<uint16_t> dst = as_global(job.tmp) + (size_t)r0 * job.tmp_pitch + o0;
    for (uint32_t row = wv; row < n_r; row += FIG_THREADS / 64)
        for (uint32_t o = lane; o < n_o; o += 64) dst[(size_t)row * job.tmp_pitch + o] = outt[row * FIG_OUT_PITCH + o];
}

__global__ __launch_bounds__(FIG_THREADS) void figure_vpass_kernel(const FigVJob *__restrict__ jobs, uint32_t n_jobs,
                                                                   const uint32_t *__restrict__ colormap, uint32_t n_colors) {
    __shared__ uint32_t lut[1024];
    const bool use_lds = n_colors <= 1024;
    if (use_lds) {
        for (uint32_t i = threadIdx.x; i < n_colors; i += FIG_THREADS) lut[i] = as_global(colormap)[i];
        __syncthreads();
    }
    const FigVJob job = jobs[fig_find_job(jobs, n_jobs)];
    const bool grey = job.kind == TH_FIGURE_GREY16;
    const uint32_t px = grey ? 8u : 4u;
    const uint32_t n_px = job.n_rows * job.out_w;  // (a part is at most TH_FIGURE_PIECE_BYTES)
    const uint32_t g = (blockIdx.x - job.first_block) * FIG_THREADS + threadIdx.x;
    const uint32_t pa = g * px;
    if (pa >= n_px) return;
    const uint32_t n_here = min(px, n_px - pa);
    const gptr<const int32_t> a_start = as_global(job.ay.start), a_count = as_global(job.ay.count);
    const gptr<const double> a_w = as_global(job.ay.w);
    const gptr<const uint16_t> tmp = as_global(job.tmp);
    const uint32_t ja = pa / job.out_w, xa = pa - ja * job.out_w;
    uint32_t val[8];
    if (n_here == px && xa + px <= job.out_w) {  // one output row: the taps are walked once for all the thread's pixels
        const uint32_t oy = job.out_h - 1u - (job.j0 + ja);
        const int32_t n = a_count[oy];
        const gptr<const double> w = a_w + (size_t)oy * job.ay.max_taps;
        const gptr<const uint16_t> col = tmp + (size_t)(a_start[oy] - (int32_t)job.y_lo) * job.tmp_pitch + xa;
        double acc[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) acc[k] = 0.0;
        if (grey) {
            for (int32_t t = 0; t < n; t++) {
                const double wt = w[t];
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) acc[k] += wt * (double)col[(size_t)t * job.tmp_pitch + k];
            }
        } else {
            for (int32_t t = 0; t < n; t++) {
                const double wt = w[t];
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) acc[k] += wt * (double)col[(size_t)t * job.tmp_pitch + k];
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) val[k] = fig_round(acc[k]);
    } else {  // the group straddles a row end, or is the part's last: pixel by pixel
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            val[k] = 0;
            if (k < n_here) {
                const uint32_t p = pa + k, j = p / job.out_w, x = p - j * job.out_w;
                const uint32_t oy = job.out_h - 1u - (job.j0 + j);
                const int32_t n = a_count[oy];
                const gptr<const double> w = a_w + (size_t)oy * job.ay.max_taps;
                const gptr<const uint16_t> col = tmp + (size_t)(a_start[oy] - (int32_t)job.y_lo) * job.tmp_pitch + x;
                double acc = 0.0;
                for (int32_t t = 0; t < n; t++) acc += w[t] * (double)col[(size_t)t * job.tmp_pitch];
                val[k] = fig_round(acc);
            }
        }
    }
    const gptr<uint8_t> dst = as_global(job.dst) + (size_t)g * 16;
    if (grey) {
        if (n_here == 8) {
            *reinterpret_cast<gptr<uint4>>(dst) =
                make_uint4(val[0] | (val[1] << 16), val[2] | (val[3] << 16), val[4] | (val[5] << 16), val[6] | (val[7] << 16));
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 8; k++)
                if (k < n_here) reinterpret_cast<gptr<uint16_t>>(dst)[k] = (uint16_t)val[k];
        }
    } else {
        const uint32_t cm1 = n_colors > 1u ? n_colors - 1u : 0u;
        uint32_t c[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t idx = fig_colour_index(val[k], cm1);
            c[k] = use_lds ? lut[idx] : as_global(colormap)[idx];
        }
        if (n_here == 4) {
            *reinterpret_cast<gptr<uint4>>(dst) = make_uint4(c[0], c[1], c[2], c[3]);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (k < n_here) reinterpret_cast<gptr<uint32_t>>(dst)[k] = c[k];
        }
    }
}

hipError_t launch_figure_hpass(const FigHJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, hipStream_t s) {
    if (n_jobs == 0 || n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(figure_hpass_kernel, dim3(n_blocks), dim3(FIG_THREADS), 0, s, d_jobs, n_jobs);
    return hipGetLastError();
}

hipError_t launch_figure_vpass(const FigVJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks, const uint8_t *d_colormap, uint32_t n_colors,
                               hipStream_t s) {
    if (n_jobs == 0 || n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(figure_vpass_kernel, dim3(n_blocks), dim3(FIG_THREADS), 0, s, d_jobs, n_jobs,
                       reinterpret_cast<const uint32_t *>(d_colormap), n_colors);
    return hipGetLastError();
}

}  // namespace th
