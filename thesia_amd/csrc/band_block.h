// band_block.h — the body of the band-filter kernel (kernels_band.hip) as phase functions over (thread id, registers, LDS arrays),
// host + device: the kernel calls them between its barriers, and a host program can run a workgroup's threads one after the other
// through the same source (scripts/san_band.cpp does, under AddressSanitizer and UBSan, with arrays of the exact sizes).
#pragma once
#include "kernels.h"
#include "resample_core.h"

namespace th {

constexpr uint32_t BAND_SPAN = BAND_TILE + BAND_TAP_BLOCK - 1;  // input samples a step stages: what the tile's outputs meet in one tap block
// where sample p of the span lies in LDS: one float of skew per BAND_R samples, so thread t's window starts at float (BAND_R + 1) t
// and the 64 lanes of a wave, BAND_R samples apart, read 64 different banks (BAND_R + 1 = 9 is odd)
TH_HD constexpr uint32_t band_at(uint32_t p) { return p + p / BAND_R; }
constexpr uint32_t BAND_XS = band_at(BAND_SPAN - 1) + 1;                      // floats of one staged span
constexpr uint32_t BAND_PRE = (BAND_SPAN + BAND_THREADS - 1) / BAND_THREADS;  // samples a thread stages per step
static_assert(BAND_TAP_BLOCK % 4 == 0 && (BAND_R + 1) % 2 == 1, "a tap block starts at a multiple of 4; the skewed pitch is odd");

// what a workgroup works on: outputs [j_first, j_first + BAND_TILE) of channel c (those below the job's jb)
struct BandBlock {
    uint32_t c;
    uint64_t j_first;
    const float *src;  // the channel's samples
    bool any;
};

// b: the block's index within its job (n_ch x n_tiles blocks: the tile fastest, then the channel)
TH_HD BandBlock band_block_of(const BandJob &job, uint32_t b) {
    BandBlock k{};
    if (job.n_tiles == 0) return k;
    k.c = b / job.n_tiles;
    k.j_first = job.ja + (uint64_t)(b % job.n_tiles) * BAND_TILE;
    k.any = k.c < job.n_ch && k.j_first < job.jb;
    if (k.any) k.src = as_global(job.chan)[k.c];
    return k;
}

// sample p of the span of tap block kb is x[j_first - K + 1 + kb + p]; whether the track has it
TH_HD int64_t band_x0(const BandBlock &k, uint32_t taps, uint32_t kb) { return (int64_t)k.j_first - (int64_t)(taps / 2) + 1 + (int64_t)kb; }
TH_HD bool band_in(const BandJob &job, int64_t x0, uint32_t p) {
    const int64_t at = x0 + (int64_t)p;
    return p < BAND_SPAN && at >= 0 && (uint64_t)at < job.n_in;
}

// the span of tap block kb into registers, RAW: a sample the track does not have is loaded from sample 0 (no branch around the load:
// a block has an output, so the track has a sample 0) and nothing here looks at a loaded value, so the loads stay in flight until
// band_commit, which puts the zeros in
TH_HD void band_fetch(const BandJob &job, const BandBlock &k, uint32_t taps, uint32_t kb, uint32_t tid, float (&pre)[BAND_PRE]) {
    const gptr<const float> src = as_global(k.src);
    const int64_t x0 = band_x0(k, taps, kb);
#pragma unroll
    for (uint32_t u = 0; u < BAND_PRE; u++) {
        const uint32_t p = tid + u * BAND_THREADS;
        pre[u] = src[band_in(job, x0, p) ? x0 + (int64_t)p : 0];
    }
}

// ... and from the registers into one of the two staged spans, zeros outside the track
TH_HD void band_commit(const BandJob &job, const BandBlock &k, uint32_t taps, uint32_t kb, const float (&pre)[BAND_PRE], uint32_t tid, float *xs) {
    const int64_t x0 = band_x0(k, taps, kb);
#pragma unroll
    for (uint32_t u = 0; u < BAND_PRE; u++) {
        const uint32_t p = tid + u * BAND_THREADS;
        if (p < BAND_SPAN) xs[band_at(p)] = band_in(job, x0, p) ? pre[u] : 0.0f;
    }
}

// A wave-uniform coefficient as a VGPR operand: a v_fmac_f32 with an SGPR source issues in 3.2 clocks, one with VGPR sources in 2.05
// (profiles/r04_ubench_valu_bank.txt), and a copy serves BAND_R of them
TH_HD float band_coef(float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    float v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(c));
    return v;
#else
    return c;
#endif
}

// nt taps (c: the row from the block's first tap, the same address in every lane) of the thread's BAND_R outputs.  Output i, tap
// kk meets sample BAND_R tid + i + kk of the span: a window of BAND_R + 3 samples in registers slides by four per four taps, so
// four LDS floats are read for 4 BAND_R fmaf.  FULL: nt == BAND_TAP_BLOCK, unrolled; else nt < BAND_TAP_BLOCK, even (the row's end)
template <bool FULL>
TH_HD void band_accumulate(ResampleAcc (&acc)[BAND_R], const float *c, uint32_t nt_in, const float *xs, uint32_t tid) {
    const uint32_t nt = FULL ? BAND_TAP_BLOCK : nt_in;
    const float *w0 = xs + (BAND_R + 1) * tid;  // (= band_at(BAND_R tid))
    float w[BAND_R + 3];
#pragma unroll
    for (uint32_t i = 0; i + 1 < BAND_R; i++) w[i] = w0[band_at(i)];
    uint32_t kk = 0;
    constexpr uint32_t UNROLL = FULL ? BAND_TAP_BLOCK / 4 : 1;
    float cf[FULL ? BAND_TAP_BLOCK : 4];
    if (FULL) {  // (the whole block's coefficients at once: one wait for the scalar loads per block, in front of the LDS reads)
#pragma unroll
        for (uint32_t i = 0; i < BAND_TAP_BLOCK; i++) cf[i] = c[i];
    }
#pragma unroll UNROLL
    for (; kk + 4 <= nt; kk += 4) {
        const float c0 = band_coef(FULL ? cf[kk] : c[kk]), c1 = band_coef(FULL ? cf[kk + 1] : c[kk + 1]);
        const float c2 = band_coef(FULL ? cf[kk + 2] : c[kk + 2]), c3 = band_coef(FULL ? cf[kk + 3] : c[kk + 3]);
#pragma unroll
        for (uint32_t m = 0; m < 4; m++) w[BAND_R - 1 + m] = w0[band_at(kk + BAND_R - 1 + m)];
#pragma unroll
        for (uint32_t i = 0; i < BAND_R; i++) resample_tap4(acc[i], c0, c1, c2, c3, w[i], w[i + 1], w[i + 2], w[i + 3]);
#pragma unroll
        for (uint32_t i = 0; i + 1 < BAND_R; i++) w[i] = w[i + 4];
    }
    if (!FULL && kk < nt) {  // (2K = 2 mod 4: the row's last two taps)
        const float c0 = band_coef(c[kk]), c1 = band_coef(c[kk + 1]);
        w[BAND_R - 1] = w0[band_at(kk + BAND_R - 1)];
        w[BAND_R] = w0[band_at(kk + BAND_R)];
#pragma unroll
        for (uint32_t i = 0; i < BAND_R; i++) resample_tap2(acc[i], c0, c1, w[i], w[i + 1]);
    }
}

TH_HD void band_store(const BandJob &job, const BandBlock &k, uint32_t tid, const ResampleAcc (&acc)[BAND_R]) {
    const gptr<float> dst = as_global(job.dst) + (uint64_t)k.c * job.ch_stride;
    const uint64_t j0 = k.j_first + (uint64_t)tid * BAND_R;
#pragma unroll
    for (uint32_t i = 0; i < BAND_R; i++)
        if (j0 + i < job.jb) dst[j0 + i - job.ja] = resample_fold(acc[i]);
}

}  // namespace th
