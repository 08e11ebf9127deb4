// align_block.h — the body of the correlation kernel (kernels_align.hip) as phase functions over (thread id, registers, LDS arrays),
// host + device: the kernel calls them between its barriers, and a host program can run a workgroup's threads one after the other
// through the same source (scripts/san_align.cpp does, under AddressSanitizer and UBSan, with arrays of the exact sizes).
#pragma once
#include "align_plan.h"

namespace th {

constexpr uint32_t ALIGN_SPAN = ALIGN_TILE + ALIGN_STEP - 1;  // probe samples a step stages: what the tile's lags meet in one step
// where sample p of the span lies in LDS: one float of skew per ALIGN_R samples, so thread t's window starts at float (ALIGN_R + 1) t
// and the lanes of a wave, ALIGN_R samples apart, read different banks (ALIGN_R + 1 = 9 is odd)
TH_HD constexpr uint32_t align_at(uint32_t p) { return p + p / ALIGN_R; }
constexpr uint32_t ALIGN_XS = align_at(ALIGN_SPAN - 1) + 1;                        // floats of one staged span
constexpr uint32_t ALIGN_CHUNK = 32;  // reference samples fetched together inside a step
constexpr uint32_t ALIGN_PRE = (ALIGN_SPAN + ALIGN_THREADS - 1) / ALIGN_THREADS;  // samples a thread stages per step
static_assert((ALIGN_R + 1) % 2 == 1, "the skewed pitch is odd");

// what a workgroup works on: lags [i_first, i_first + ALIGN_TILE) of the piece (those below n_lags) over reference samples [k_first, k_end)
struct AlignBlock {
    uint32_t g, i_first;
    uint64_t k_first, k_end;
    bool any;
};

// b: the block's index in the launch (n_tiles x n_groups blocks: the tile fastest)
TH_HD AlignBlock align_block_of(const AlignJob &job, uint32_t b) {
    AlignBlock k{};
    if (job.n_tiles == 0) return k;
    k.g = b / job.n_tiles;
    k.i_first = (b % job.n_tiles) * ALIGN_TILE;
    k.k_first = (uint64_t)k.g * ALIGN_GROUP;
    k.k_end = k.k_first + ALIGN_GROUP < job.N ? k.k_first + ALIGN_GROUP : job.N;
    k.any = k.g < job.n_groups && k.i_first < job.n_lags && k.k_first < k.k_end;
    return k;
}

// the span of the step at k0 into registers: sample p of it is b[first + i_first + k0 + p], +0 where the track has none (the load is
// predicated, and nothing here waits for it)
TH_HD void align_fetch(const AlignJob &job, const AlignBlock &k, uint64_t k0, uint32_t tid, float (&pre)[ALIGN_PRE]) {
    const gptr<const float> src = as_global(job.b);
    const int64_t x0 = job.first + (int64_t)k.i_first + (int64_t)k0;
#pragma unroll
    for (uint32_t u = 0; u < ALIGN_PRE; u++) {
        const uint32_t p = tid + u * ALIGN_THREADS;
        const int64_t at = x0 + (int64_t)p;
        float v = 0.0f;
        if (p < ALIGN_SPAN && at >= 0 && (uint64_t)at < job.n_b) v = src[at];
        pre[u] = v;
    }
}

// ... and from the registers into one of the two staged spans
TH_HD void align_commit(const float (&pre)[ALIGN_PRE], uint32_t tid, float *xs) {
#pragma unroll
    for (uint32_t u = 0; u < ALIGN_PRE; u++) {
        const uint32_t p = tid + u * ALIGN_THREADS;
        if (p < ALIGN_SPAN) xs[align_at(p)] = pre[u];
    }
}

// nt reference samples (a: from the step's first one, the same address in every lane) against the thread's ALIGN_R lags.  Lag i,
// sample kk meets sample ALIGN_R tid + i + kk of the span: a window of ALIGN_R + 3 doubles in registers slides by four per four
// samples, so four LDS floats are read and converted for 4 ALIGN_R multiply-adds, and a reference sample is converted once for
// ALIGN_R of them.  A step starts at k = 0 mod 4, so sample kk goes to partial sum kk mod 4.  align_four: four samples from kk = 0 mod 4.
// FULL: nt == ALIGN_STEP, unrolled by chunks; else
// nt < ALIGN_STEP (the range's end): whole fours, then the last one to three samples
TH_HD void align_four(AlignAcc (&acc)[ALIGN_R], double (&w)[ALIGN_R + 3], const float *w0, uint32_t kk, double a0, double a1, double a2, double a3) {
#pragma unroll
    for (uint32_t m = 0; m < 4; m++) w[ALIGN_R - 1 + m] = (double)w0[align_at(kk + ALIGN_R - 1 + m)];
#pragma unroll
    for (uint32_t i = 0; i < ALIGN_R; i++) {
        align_term(acc[i].p[0], a0, w[i]);
        align_term(acc[i].p[1], a1, w[i + 1]);
        align_term(acc[i].p[2], a2, w[i + 2]);
        align_term(acc[i].p[3], a3, w[i + 3]);
    }
#pragma unroll
    for (uint32_t i = 0; i + 1 < ALIGN_R; i++) w[i] = w[i + 4];
}
template <bool FULL>
TH_HD void align_accumulate(AlignAcc (&acc)[ALIGN_R], const float *a, uint32_t nt_in, const float *xs, uint32_t tid) {
    const uint32_t nt = FULL ? ALIGN_STEP : nt_in;
    const float *w0 = xs + (ALIGN_R + 1) * tid;  // (= align_at(ALIGN_R tid))
    double w[ALIGN_R + 3];
#pragma unroll
    for (uint32_t i = 0; i + 1 < ALIGN_R; i++) w[i] = (double)w0[align_at(i)];
    uint32_t kk = 0;
    if (FULL) {
        // (ALIGN_CHUNK reference samples at once: one wait for the scalar loads per chunk, in front of its LDS reads)
#pragma unroll 1
        for (uint32_t c = 0; c < ALIGN_STEP; c += ALIGN_CHUNK) {
            float af[ALIGN_CHUNK];
#pragma unroll
            for (uint32_t i = 0; i < ALIGN_CHUNK; i++) af[i] = a[c + i];
#pragma unroll
            for (uint32_t u = 0; u < ALIGN_CHUNK; u += 4) align_four(acc, w, w0, c + u, (double)af[u], (double)af[u + 1], (double)af[u + 2], (double)af[u + 3]);
        }
        kk = ALIGN_STEP;
    } else {
        for (; kk + 4 <= nt; kk += 4) align_four(acc, w, w0, kk, (double)a[kk], (double)a[kk + 1], (double)a[kk + 2], (double)a[kk + 3]);
    }
    if (!FULL && kk < nt) {
        const uint32_t rem = nt - kk;  // 1 .. 3
#pragma unroll
        for (uint32_t m = 0; m < 3; m++)
            if (m < rem) {
                const double am = (double)a[kk + m];
                w[ALIGN_R - 1 + m] = (double)w0[align_at(kk + ALIGN_R - 1 + m)];
#pragma unroll
                for (uint32_t i = 0; i < ALIGN_R; i++) align_term(acc[i].p[m], am, w[i + m]);
            }
    }
}

// a block of the reference ends: its value joins the group's, the partial sums start again from +0
TH_HD void align_block_end(AlignAcc (&acc)[ALIGN_R], double (&group)[ALIGN_R]) {
#pragma unroll
    for (uint32_t i = 0; i < ALIGN_R; i++) {
        group[i] += align_block_value(acc[i]);
        align_zero(acc[i]);
    }
}

TH_HD void align_store(const AlignJob &job, const AlignBlock &k, uint32_t tid, const double (&group)[ALIGN_R]) {
    const gptr<double> dst = as_global(job.scratch) + (uint64_t)k.g * job.n_lags;
    const uint32_t i0 = k.i_first + tid * ALIGN_R;
#pragma unroll
    for (uint32_t i = 0; i < ALIGN_R; i++)
        if (i0 + i < job.n_lags) dst[i0 + i] = group[i];
}

// ---- the energy kernel: thread t of group g's workgroup is partial sum t mod 4 of block 32 g + t div 4 (+0 for a block past the
// last); then one thread folds the group's blocks in ascending order
TH_HD double align_energy_thread(const float *x, uint64_t n, int64_t first, uint64_t N, uint32_t g, uint32_t tid) {
    return align_partial_sq(x, n, first, N, (uint64_t)g * ALIGN_GROUP_BLOCKS + tid / 4, tid % 4);
}
TH_HD double align_energy_group(const double *part /* ALIGN_ENERGY_THREADS */, uint64_t N, uint32_t g) {
    const uint64_t n_blocks = (N + ALIGN_BLOCK - 1) / ALIGN_BLOCK, j0 = (uint64_t)g * ALIGN_GROUP_BLOCKS;
    const uint32_t cnt = (uint32_t)(n_blocks - j0 < ALIGN_GROUP_BLOCKS ? n_blocks - j0 : ALIGN_GROUP_BLOCKS);
    double group = 0.0;
    for (uint32_t j = 0; j < cnt; j++) group += (part[4 * j] + part[4 * j + 1]) + (part[4 * j + 2] + part[4 * j + 3]);
    return group;
}

}  // namespace th
