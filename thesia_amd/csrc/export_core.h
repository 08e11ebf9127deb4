// export_core.h — the dither generator and the quantiser of the PCM / WAV export (th_tm_export_pcm), written once for the host
// (th_export_dither, th_export_quantize, api.hip) and for the device (kernels_export.hip): the same integer and f64 steps on both,
// so a byte of an export is reproducible anywhere.  The definitions are those of include/thesia_amd.h ("PCM / WAV export").
#pragma once
#include <stdint.h>

#include "../../include/thesia_amd.h"  // TH_PCM_*
#include "stft_core.h"                 // TH_HD

namespace th {

TH_HD uint32_t export_fmix32(uint32_t h) {  // the finaliser of MurmurHash3 (public domain)
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// k0 depends on (seed, ch) alone and k1 on the upper half of the index as well: a run of samples of one channel shares them
TH_HD uint32_t export_dither_k0(uint32_t seed, uint32_t ch) { return export_fmix32(seed + 0x9e3779b9u * (ch + 1u)); }
TH_HD uint32_t export_dither_k1(uint32_t k0, uint64_t i) { return export_fmix32((uint32_t)(i >> 32) ^ k0); }
// the two 24-bit uniform integers of sample i (the ABSOLUTE index in the track)
TH_HD void export_dither_ab(uint32_t k1, uint64_t i, uint32_t *a, uint32_t *b) {
    const uint32_t k = export_fmix32((uint32_t)i ^ k1);
    *a = export_fmix32(k ^ 0x68bc21ebu) >> 8;
    *b = export_fmix32(k ^ 0x02e5be93u) >> 8;
}

struct ExportCounts {
    uint32_t clamped, nan;
};

// One sample to a signed integer of scale S (32768 or 8388608): v = x S + d in f64 (x S is exact, so a contraction of the two
// cannot change v), d = (a - b) 2^-24 (exact) or 0, q = rint(v) to even, clamped to [-S, S - 1].  A NaN gives 0.
TH_HD int32_t export_quantize_one(float x, double S, bool tpdf, uint32_t a, uint32_t b, ExportCounts *cnt) {
    if (x != x) {
        cnt->nan++;
        return 0;
    }
    const double d = tpdf ? ((double)a - (double)b) * (1.0 / 16777216.0) : 0.0;
    const double v = (double)x * S + d;
    double q = __builtin_rint(v);
    if (q > S - 1.0) {
        q = S - 1.0;
        cnt->clamped++;
    } else if (q < -S) {
        q = -S;
        cnt->clamped++;
    }
    return (int32_t)q;
}

TH_HD double export_scale(uint32_t format) { return format == TH_PCM_S16 ? 32768.0 : 8388608.0; }
TH_HD uint32_t export_bytes_per_sample(uint32_t format) { return format == TH_PCM_S16 ? 2u : format == TH_PCM_S24 ? 3u : 4u; }

}  // namespace th
