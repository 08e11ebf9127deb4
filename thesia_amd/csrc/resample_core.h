// resample_core.h — the index arithmetic and the summation of the polyphase sinc resampler (th_tm_export_pcm_at), written once for
// the host (th_resample_f32, api.hip) and for the device (kernels_resample.hip): the same integer steps and the same f32 fmaf chain in
// the same order on both, so a resampled sample is reproducible anywhere.  The definitions are those of include/thesia_amd.h
// ("Export at a target sample rate").
//
//   The order of the sum depends on nothing but the tap index: tap k (0 .. 2K - 1, ascending) goes into partial sum k mod 4 with one
//   fmaf, all four start at +0, and the result is (a0 + a1) + (a2 + a3).  A tap whose sample lies outside the track is NOT skipped:
//   it is the fmaf with x = 0 (the kernel's staged zeros do the same).
#pragma once
#include <stdint.h>

#include "../../include/thesia_amd.h"
#include "stft_core.h"  // TH_HD

namespace th {

struct ResampleAcc {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
};

// taps k .. k + 3 with k a multiple of 4
TH_HD void resample_tap4(ResampleAcc &s, float c0, float c1, float c2, float c3, float x0, float x1, float x2, float x3) {
    s.a0 = __builtin_fmaf(c0, x0, s.a0);
    s.a1 = __builtin_fmaf(c1, x1, s.a1);
    s.a2 = __builtin_fmaf(c2, x2, s.a2);
    s.a3 = __builtin_fmaf(c3, x3, s.a3);
}
// the last two taps of a row whose length 2K is not a multiple of 4 (2K is even): k, k + 1 with k a multiple of 4
TH_HD void resample_tap2(ResampleAcc &s, float c0, float c1, float x0, float x1) {
    s.a0 = __builtin_fmaf(c0, x0, s.a0);
    s.a1 = __builtin_fmaf(c1, x1, s.a1);
}
TH_HD float resample_fold(const ResampleAcc &s) { return (s.a0 + s.a1) + (s.a2 + s.a3); }

// taps [k0, k0 + n) of one output: c = the row from tap k0, x = the window from tap k0 (zeros where the track has no sample);
// k0 a multiple of 4, n even
TH_HD void resample_taps(ResampleAcc &s, const float *c, const float *x, uint32_t n) {
    uint32_t k = 0;
    for (; k + 4 <= n; k += 4) resample_tap4(s, c[k], c[k + 1], c[k + 2], c[k + 3], x[k], x[k + 1], x[k + 2], x[k + 3]);
    if (k < n) resample_tap2(s, c[k], c[k + 1], x[k], x[k + 1]);
}

// output j of the ratio L / M: j M = q L + r (the caller has checked that j M fits 64 bits)
TH_HD void resample_phase(uint64_t j, uint32_t L, uint32_t M, uint64_t *q, uint32_t *r) {
    const uint64_t jm = j * M;
    *q = jm / L;
    *r = (uint32_t)(jm - *q * L);
}

}  // namespace th
