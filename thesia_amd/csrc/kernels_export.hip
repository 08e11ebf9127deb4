// kernels_export.hip — resident planar f32 channels to file-ready bytes (th_tm_export_pcm / th_tm_export_wav): the channels
// interleaved, each sample quantised to 16- or 24-bit little-endian PCM (export_core.h: the quantiser and the counter-based TPDF
// dither, shared with the host) or copied as float32.  A pure streaming kernel: 4 bytes read per sample, 2 - 4 written.
//
//   One launch over a table of jobs (a job = frames [f0, f1) of one request), block b finds its job by first_chunk and takes chunk
//   b - first_chunk of it.  Chunks lie on the track's ABSOLUTE frame grid (export_chunk_frames(n_ch) frames each, a multiple of 4, at
//   most EXPORT_CHUNK_SAMPLES samples), so the 16-byte loads of a 16-byte aligned channel stay aligned whatever f0 is, and the cut of
//   a request into jobs (the host's pieces) changes only which block makes a byte, never the byte.
//   Load: a unit is 4 consecutive frames of one channel on that grid, one 16-byte load where the channel pointer is 16-byte aligned
//   and the four samples exist, else guarded 4-byte loads; neighbouring lanes take neighbouring units of one channel.
//   Quantise, and write the sample's bytes into LDS IN OUTPUT BYTE ORDER: the LDS image starts at the 16-byte boundary at or below the
//   chunk's first output byte, so LDS byte i is global byte A0 + i.
//   Store: the image goes out in aligned 16-byte pieces; the pieces that hold the chunk's first and last bytes are written byte by
//   byte where they are not wholly the chunk's.  No thread writes outside [dst, dst + bytes + pad) of its job.
//   Counts: per thread, a wave reduction, the four waves through LDS, then one 64-bit vector atomic add per count and workgroup
//   (skipped when zero): integer sums do not depend on the order.
// The destination may start at any byte address (a WAV header is 44 or 58 bytes; 24-bit frames straddle dwords); frame indices and
// byte offsets are 64-bit.  -ffp-contract=off (x S is exact in f64, so a contraction could not change v anyway).
#include <hip/hip_runtime.h>

#include "export_core.h"
#include "kernels.h"

namespace th {

namespace {

// head (< 16) + the chunk's bytes (<= 4 EXPORT_CHUNK_SAMPLES) + pad (< 16), in 16-byte pieces
constexpr uint32_t EXPORT_LDS_BYTES = EXPORT_CHUNK_SAMPLES * 4 + 48;
static_assert(export_chunk_frames(TH_EXPORT_MAX_CHANNELS) * TH_EXPORT_MAX_CHANNELS <= EXPORT_CHUNK_SAMPLES, "a chunk must fit the LDS image");
static_assert(export_chunk_frames(3) * 3 <= EXPORT_CHUNK_SAMPLES && export_chunk_frames(3) % 4 == 0, "chunk frames");

struct Chunk {
    uint64_t fa, fb;   // frames of this chunk
    uint64_t g0;       // first group of 4 frames (absolute)
    uint32_t ng;       // groups
    uint32_t head;     // LDS byte of the chunk's first output byte
};

template <uint32_t FMT>
__device__ __forceinline__ void put_sample(uint8_t *lds, uint32_t at, uint32_t v, bool wide) {
    if (FMT == TH_PCM_S16) {
        if (wide) {
            *reinterpret_cast<uint16_t *>(lds + at) = (uint16_t)v;
        } else {
            lds[at] = (uint8_t)v;
            lds[at + 1] = (uint8_t)(v >> 8);
        }
    } else if (FMT == TH_PCM_S24) {
        lds[at] = (uint8_t)v;
        lds[at + 1] = (uint8_t)(v >> 8);
        lds[at + 2] = (uint8_t)(v >> 16);
    } else {
        if (wide) {
            *reinterpret_cast<uint32_t *>(lds + at) = v;
        } else {
            lds[at] = (uint8_t)v;
            lds[at + 1] = (uint8_t)(v >> 8);
            lds[at + 2] = (uint8_t)(v >> 16);
            lds[at + 3] = (uint8_t)(v >> 24);
        }
    }
}

// the chunk's samples, quantised, into the LDS image
template <uint32_t FMT>
__device__ __forceinline__ void fill_image(const ExportJob &job, const Chunk &ck, uint8_t *lds, ExportCounts *cnt) {
    constexpr uint32_t BPS = FMT == TH_PCM_S16 ? 2 : FMT == TH_PCM_S24 ? 3 : 4;
    const bool wide = FMT == TH_PCM_S16 ? (ck.head & 1) == 0 : (ck.head & 3) == 0;  // (a sample's offset from the head is a multiple of BPS)
    const bool tpdf = job.dither == TH_DITHER_TPDF;
    const double S = export_scale(FMT);
    const uint32_t units = job.n_ch * ck.ng;
    const gptr<const float *const> chan = as_global(job.chan);
    for (uint32_t u = threadIdx.x; u < units; u += EXPORT_THREADS) {
        const uint32_t c = u / ck.ng, gi = u - c * ck.ng;
        const uint64_t f4 = (ck.g0 + gi) * 4;
        const float *flat = chan[c];
        const gptr<const uint32_t> p = reinterpret_cast<gptr<const uint32_t>>(as_global(flat));
        uint32_t w[4];
        if (f4 + 4 <= job.n && (reinterpret_cast<uintptr_t>(flat) & 15) == 0) {
            const uint4 v = *reinterpret_cast<gptr<const uint4>>(p + f4);
            w[0] = v.x;
            w[1] = v.y;
            w[2] = v.z;
            w[3] = v.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) w[j] = (f4 + j >= ck.fa && f4 + j < ck.fb) ? p[f4 + j] : 0u;
        }
        const uint32_t k1 = export_dither_k1(export_dither_k0(job.seed, c), f4);  // (f4 .. f4 + 3 share the index's upper half)
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint64_t f = f4 + j;
            if (f < ck.fa || f >= ck.fb) continue;
            const uint32_t at = ck.head + ((uint32_t)(f - ck.fa) * job.n_ch + c) * BPS;
            uint32_t v;
            if (FMT == TH_PCM_F32) {
                v = w[j];
                cnt->nan += (v & 0x7fffffffu) > 0x7f800000u;
            } else {
                uint32_t a = 0, b = 0;
                if (tpdf) export_dither_ab(k1, f, &a, &b);
                v = (uint32_t)export_quantize_one(__uint_as_float(w[j]), S, tpdf, a, b, cnt);
            }
            put_sample<FMT>(lds, at, v, wide);
        }
    }
}

}  // namespace

__global__ __launch_bounds__(EXPORT_THREADS) void export_kernel(const ExportJob *__restrict__ jobs, uint32_t n_jobs) {
    __shared__ uint4 img[EXPORT_LDS_BYTES / 16];
    __shared__ uint32_t red[2 * (EXPORT_THREADS / 64)];
    uint8_t *lds = reinterpret_cast<uint8_t *>(img);
    // the job of this block: the last one whose first_chunk is at or below the block index
    uint32_t lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (jobs[mid].first_chunk <= blockIdx.x)
            lo = mid;
        else
            hi = mid;
    }
    const ExportJob job = jobs[lo];
    const uint64_t F = export_chunk_frames(job.n_ch);
    const uint64_t k = job.f0 / F + (blockIdx.x - job.first_chunk);
    Chunk ck;
    ck.fa = k * F > job.f0 ? k * F : job.f0;
    ck.fb = (k + 1) * F < job.f1 ? (k + 1) * F : job.f1;
    if (ck.fa >= ck.fb) return;  // (no such block in a table built by export_n_chunks)
    ck.g0 = ck.fa >> 2;
    ck.ng = (uint32_t)(((ck.fb + 3) >> 2) - ck.g0);
    const uint32_t bps = export_bytes_per_sample(job.format);
    const gptr<uint8_t> dst = as_global(job.dst) + (ck.fa - job.f0) * job.n_ch * bps;
    ck.head = (uint32_t)(reinterpret_cast<uintptr_t>(job.dst) + (ck.fa - job.f0) * job.n_ch * bps) & 15u;
    const uint32_t nb = (uint32_t)(ck.fb - ck.fa) * job.n_ch * bps;
    const uint32_t pad = ck.fb == job.f1 ? job.pad : 0u;

    ExportCounts cnt{0, 0};
    switch (job.format) {
        case TH_PCM_S16: fill_image<TH_PCM_S16>(job, ck, lds, &cnt); break;
        case TH_PCM_S24: fill_image<TH_PCM_S24>(job, ck, lds, &cnt); break;
        default: fill_image<TH_PCM_F32>(job, ck, lds, &cnt); break;
    }
    if (threadIdx.x < pad) lds[ck.head + nb + threadIdx.x] = 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        cnt.clamped += __shfl_xor(cnt.clamped, off, 64);
        cnt.nan += __shfl_xor(cnt.nan, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[2 * (threadIdx.x >> 6)] = cnt.clamped;
        red[2 * (threadIdx.x >> 6) + 1] = cnt.nan;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long s = 0;
        for (uint32_t wv = 0; wv < EXPORT_THREADS / 64; wv++) s += red[2 * wv + threadIdx.x];
        if (s) __hip_atomic_fetch_add(as_global(job.cnt) + threadIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // LDS byte i is global byte a0 + i
    const uint32_t total = ck.head + nb + pad;
    const gptr<uint8_t> a0 = dst - ck.head;
    for (uint32_t pc = threadIdx.x; pc * 16 < total; pc += EXPORT_THREADS) {
        const uint32_t b0 = pc * 16;
        if (b0 >= ck.head && b0 + 16 <= total) {
            *reinterpret_cast<gptr<uint4>>(a0 + b0) = img[pc];
        } else {
            const uint32_t from = b0 > ck.head ? b0 : ck.head, to = b0 + 16 < total ? b0 + 16 : total;
            for (uint32_t i = from; i < to; i++) a0[i] = lds[i];
        }
    }
}

hipError_t launch_export(const ExportJob *d_jobs, uint32_t n_jobs, uint32_t n_chunks, hipStream_t s) {
    if (n_jobs == 0 || n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(export_kernel, dim3(n_chunks), dim3(EXPORT_THREADS), 0, s, d_jobs, n_jobs);
    return hipGetLastError();
}

}  // namespace th
