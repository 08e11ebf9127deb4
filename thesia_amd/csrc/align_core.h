// align_core.h — the arithmetic of the alignment reader (include/thesia_amd.h "Align two tracks"), host + device: one source for
// kernels_align.hip (through align_block.h), for the host functions th_xcorr_f64 / th_align_energy_f64 / th_align_f64 (align_plan.cpp)
// and for scripts/san_align.cpp.
//
// A term is (double)a * (double)b: the product of two f32 has at most 48 significant bits and an exponent far inside f64's range, so
// it is exact, and p + a b rounds once whether the compiler fuses it or not.  The order of the additions is the contract's: block
// k div 4096, in it four partial sums by k mod 4 in ascending k from +0, (p0 + p1) + (p2 + p3), the blocks of a group of 32 in
// ascending order from +0, the groups in ascending order from +0.
#pragma once
#include <cstdint>

#include "../../include/thesia_amd.h"
#include "stft_core.h"  // TH_HD

namespace th {

constexpr uint32_t ALIGN_BLOCK = TH_ALIGN_BLOCK;                 // reference samples of one block
constexpr uint32_t ALIGN_GROUP_BLOCKS = TH_ALIGN_GROUP_BLOCKS;   // blocks of one group
constexpr uint64_t ALIGN_GROUP = (uint64_t)ALIGN_BLOCK * ALIGN_GROUP_BLOCKS;  // reference samples of one group (131 072)
static_assert(ALIGN_BLOCK % 4 == 0, "a block starts at k = 0 mod 4");

TH_HD uint64_t align_n_groups(uint64_t N) { return (N + ALIGN_GROUP - 1) / ALIGN_GROUP; }

// the four partial sums of a block
struct AlignAcc {
    double p[4];
};
TH_HD void align_zero(AlignAcc &s) { s.p[0] = s.p[1] = s.p[2] = s.p[3] = 0.0; }
TH_HD void align_term(double &p, double a, double b) { p += a * b; }
TH_HD double align_block_value(const AlignAcc &s) { return (s.p[0] + s.p[1]) + (s.p[2] + s.p[3]); }

// sample `at` of a track of n samples, +0 outside it
TH_HD float align_sample(const float *x, uint64_t n, int64_t at) { return at >= 0 && (uint64_t)at < n ? x[at] : 0.0f; }

// Partial sum q of block j of sum over k < N of a[k] b[first + k]: the terms k = 4096 j + q, + 4, + 8 .. below N, in ascending k.
// a: N samples; b: a track of n_b samples (+0 outside).  The plain restatement of the contract, and what an energy thread runs
TH_HD double align_partial(const float *a, uint64_t N, const float *b, uint64_t n_b, int64_t first, uint64_t j, uint32_t q) {
    const uint64_t k0 = j * ALIGN_BLOCK, k1 = k0 + ALIGN_BLOCK < N ? k0 + ALIGN_BLOCK : N;
    double p = 0.0;
    for (uint64_t k = k0 + q; k < k1; k += 4) align_term(p, (double)a[k], (double)align_sample(b, n_b, first + (int64_t)k));
    return p;
}
// ... with both factors the same track x (+0 outside): E(x, first, N)'s partial sum
TH_HD double align_partial_sq(const float *x, uint64_t n, int64_t first, uint64_t N, uint64_t j, uint32_t q) {
    const uint64_t k0 = j * ALIGN_BLOCK, k1 = k0 + ALIGN_BLOCK < N ? k0 + ALIGN_BLOCK : N;
    double p = 0.0;
    for (uint64_t k = k0 + q; k < k1; k += 4) {
        const double v = (double)align_sample(x, n, first + (int64_t)k);
        align_term(p, v, v);
    }
    return p;
}

// n values in ascending order from +0 (a group's blocks; a sum's groups)
TH_HD double align_fold(const double *v, uint64_t n, uint64_t stride) {
    double s = 0.0;
    for (uint64_t i = 0; i < n; i++) s += v[i * stride];
    return s;
}

}  // namespace th
