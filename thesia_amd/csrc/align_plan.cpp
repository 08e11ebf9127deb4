// align_plan.cpp — the host side of the alignment reader (align_plan.h): the plan of a request, its cut into pieces, the host's step
// on the read-back curve and the host restatements of the two sums.  Plain data and C double, no HIP.  -ffp-contract=off: the host's
// step rounds every product and difference on its own (the sums' terms are exact products, which no contraction can change).
#include "align_plan.h"

#include <algorithm>
#include <cmath>
#include <limits>

#include "host_math.h"

namespace th {

int align_plan_for(uint32_t sr_ref, size_t n_ref, uint32_t sr, size_t n, const th_align_request &req, th_align_plan *plan) {
    (void)n;  // (a probe of any length: what the lags do not meet is +0)
    th_align_plan pl{};
    if (sr_ref == 0 || sr == 0) return 1;
    if (req.ref_which > 2 || req.which > 2 || req.kind > TH_ALIGN_OUT_CURVE || (req.flags & ~TH_ALIGN_ABS)) return 1;
    if (std::isnan(req.start_sec) || std::isnan(req.end_sec) || std::isnan(req.max_lag_sec)) return 1;
    if (!(req.max_lag_sec >= 0.0) || std::isinf(req.max_lag_sec)) return 1;
    size_t s0 = 0, s1 = 0;
    if (!spectrum_frame_range(sr_ref, 1, n_ref, req.start_sec, req.end_sec, &s0, &s1)) return 1;
    if (sr_ref != sr) return 2;
    const uint64_t N = (uint64_t)(s1 - s0);
    if (N > TH_ALIGN_MAX_REF) return 2;
    const double d = std::rint(req.max_lag_sec * (double)sr);
    if (!(d <= (double)TH_ALIGN_MAX_LAG)) return 2;
    const uint32_t D = (uint32_t)d;
    const uint64_t n_lags = N ? 2 * (uint64_t)D + 1 : 0;
    if (N * n_lags > TH_ALIGN_MAX_WORK) return 2;  // (2^22 x 2^21 + 2^22: no overflow)
    pl.sr = sr;
    pl.max_lag = D;
    pl.kind = req.kind;
    pl.flags = req.flags;
    pl.sample_start = s0;
    pl.sample_end = s1;
    pl.n_lags = n_lags;
    pl.length = TH_ALIGN_SUMMARY_DOUBLES + (req.kind == TH_ALIGN_OUT_CURVE ? n_lags : 0);
    *plan = pl;
    return 0;
}

AlignPieces plan_align(uint64_t N, uint64_t n_lags) {
    AlignPieces out;
    const uint32_t n_groups = (uint32_t)align_n_groups(N);
    for (uint64_t at = 0; at < n_lags; at += TH_ALIGN_PIECE_LAGS) {
        AlignPiece pc{};
        pc.lag0 = at;
        pc.n_lags = (uint32_t)std::min<uint64_t>(TH_ALIGN_PIECE_LAGS, n_lags - at);
        pc.n_tiles = align_n_tiles(pc.n_lags);
        pc.n_groups = n_groups;
        pc.n_blocks = pc.n_tiles * pc.n_groups;
        out.scratch_doubles = std::max<uint64_t>(out.scratch_doubles, (uint64_t)pc.n_groups * pc.n_lags);
        out.rec_doubles = std::max<uint64_t>(out.rec_doubles, pc.n_lags);
        out.pieces.push_back(pc);
    }
    return out;
}

AlignPeak align_peak(const double *r, uint64_t n_lags, uint32_t flags, double e_ref) {
    AlignPeak pk{1u, 0, 0.0, 1.0};
    if (n_lags == 0 || !std::isfinite(e_ref) || !(e_ref > 0.0)) return pk;
    for (uint64_t i = 0; i < n_lags; i++)
        if (!std::isfinite(r[i])) return pk;
    const bool abs = (flags & TH_ALIGN_ABS) != 0;
    auto m = [&](uint64_t i) { return abs ? std::fabs(r[i]) : r[i]; };
    uint64_t best = 0;
    for (uint64_t i = 1; i < n_lags; i++)
        if (m(i) > m(best)) best = i;
    pk.status = 0;
    pk.index = best;
    pk.polarity = r[best] < 0.0 ? -1.0 : 1.0;
    if (best > 0 && best + 1 < n_lags) {
        const double mm = m(best - 1), m0 = m(best), mp = m(best + 1);
        const double den = (mm - 2.0 * m0) + mp;
        pk.delta = den < 0.0 ? (0.5 * (mm - mp)) / den : 0.0;
    }
    return pk;
}

void align_summary(const AlignPeak &pk, const double *r, uint32_t D, double e_ref, double e_probe, double out[TH_ALIGN_SUMMARY_DOUBLES]) {
    if (pk.status != 0) {
        out[0] = 1.0;
        for (uint32_t i = 1; i < TH_ALIGN_SUMMARY_DOUBLES; i++) out[i] = std::numeric_limits<double>::quiet_NaN();
        return;
    }
    const double rs = r[pk.index];
    const double gain = rs / e_ref;
    const double fit = rs * gain;
    double resid = e_probe - fit;
    if (resid < 0.0) resid = 0.0;
    out[0] = 0.0;
    out[1] = (double)((int64_t)pk.index - (int64_t)D);
    out[2] = pk.delta;
    out[3] = rs;
    out[4] = e_ref;
    out[5] = e_probe;
    out[6] = rs / std::sqrt(e_ref * e_probe);
    out[7] = gain;
    out[8] = 10.0 * std::log10(resid / e_probe);
    out[9] = pk.polarity;
}

void xcorr_f64(const float *a, uint64_t N, const float *b, uint64_t n_b, int64_t first, uint64_t n_lags, double *r) {
    const uint64_t n_blocks = (N + ALIGN_BLOCK - 1) / ALIGN_BLOCK;
    for (uint64_t i = 0; i < n_lags; i++) {
        double sum = 0.0, group = 0.0;
        for (uint64_t j = 0; j < n_blocks; j++) {
            AlignAcc s;
            for (uint32_t q = 0; q < 4; q++) s.p[q] = align_partial(a, N, b, n_b, first + (int64_t)i, j, q);
            group += align_block_value(s);
            if ((j + 1) % ALIGN_GROUP_BLOCKS == 0 || j + 1 == n_blocks) {
                sum += group;
                group = 0.0;
            }
        }
        r[i] = sum;
    }
}

double align_energy_f64(const float *x, uint64_t n, int64_t first, uint64_t N) {
    const uint64_t n_blocks = (N + ALIGN_BLOCK - 1) / ALIGN_BLOCK;
    double sum = 0.0, group = 0.0;
    for (uint64_t j = 0; j < n_blocks; j++) {
        AlignAcc s;
        for (uint32_t q = 0; q < 4; q++) s.p[q] = align_partial_sq(x, n, first, N, j, q);
        group += align_block_value(s);
        if ((j + 1) % ALIGN_GROUP_BLOCKS == 0 || j + 1 == n_blocks) {
            sum += group;
            group = 0.0;
        }
    }
    return sum;
}

void align_f64(const float *ref, const float *probe, uint64_t n_b, const th_align_plan &pl, double *out) {
    const uint64_t s0 = pl.sample_start, N = pl.sample_end - pl.sample_start;
    std::vector<double> keep;
    double *r = out + TH_ALIGN_SUMMARY_DOUBLES;
    if (pl.kind != TH_ALIGN_OUT_CURVE) {
        keep.resize((size_t)pl.n_lags);
        r = keep.data();
    }
    const float *a = N ? ref + s0 : nullptr;
    xcorr_f64(a, N, probe, n_b, (int64_t)s0 - (int64_t)pl.max_lag, pl.n_lags, r);
    const double e_ref = align_energy_f64(a, N, 0, N);
    const AlignPeak pk = align_peak(r, pl.n_lags, pl.flags, e_ref);
    const double e_probe = pk.status == 0 ? align_energy_f64(probe, n_b, (int64_t)s0 + (int64_t)pk.index - (int64_t)pl.max_lag, N) : 0.0;
    align_summary(pk, r, pl.max_lag, e_ref, e_probe, out);
}

}  // namespace th
