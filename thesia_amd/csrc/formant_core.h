// formant_core.h — the arithmetic of the formant reader (include/thesia_amd.h "Formant candidates"), written once for the host
// (th_formants_f64, formant_plan.cpp) and for the device (kernels_formant.hip): every step is one rounded f64 operation per written
// operation, in the contract's order.  Every translation unit that includes this is compiled with -ffp-contract=off; there is no
// fma and no libm call here (the window, the start points and alpha are host-built tables).
#pragma once
#include <cstdint>

#include "stft_core.h"  // TH_HD, as_global

namespace th {

constexpr uint32_t FORMANT_LANES = 64;       // partial sums of a lag: one per lane
constexpr uint32_t FORMANT_PART_PITCH = 65;  // doubles between two lags' partial sums (lane m walks row m: odd pitch, no common bank)
constexpr double FORMANT_LOADING = 1.0 + 0x1p-30;
constexpr double FORMANT_STOP = 0x1p-80;
constexpr double FORMANT_DBL_MAX = 1.7976931348623157e308;

struct fm_c {
    double r, i;
};
TH_HD fm_c fm_add(fm_c a, fm_c b) { return fm_c{a.r + b.r, a.i + b.i}; }
TH_HD fm_c fm_sub(fm_c a, fm_c b) { return fm_c{a.r - b.r, a.i - b.i}; }
TH_HD fm_c fm_mul(fm_c a, fm_c b) { return fm_c{a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
TH_HD fm_c fm_div(fm_c u, fm_c v) {
    const double n = v.r * v.r + v.i * v.i;
    return fm_c{(u.r * v.r + u.i * v.i) / n, (u.i * v.r - u.r * v.i) / n};
}

// step 1 without the window: d[n] of the analysis signal u (u[n] is analysis sample n; only samples of [0, n_a) are read)
TH_HD double formant_d(const float *u, int64_t n, uint64_t n_a, double alpha) {
    if (n < 0 || (uint64_t)n >= n_a) return 0.0;
    const gptr<const float> g = as_global(u);
    const double prev = n > 0 ? (double)g[n - 1] : 0.0;
    return (double)g[n] - alpha * prev;
}

// step 2, partial sum q of every lag m <= p (p < NL): k = q, q + 64, ... while k + m < W
template <uint32_t NL>
TH_HD void formant_autocorr_lane(const double *s, uint32_t W, uint32_t p, uint32_t q, double *part) {
    double acc[NL];
#pragma unroll
    for (uint32_t m = 0; m < NL; m++) acc[m] = 0.0;
    for (uint32_t k = q; k < W; k += FORMANT_LANES) {
        const double sk = s[k];
#pragma unroll
        for (uint32_t m = 0; m < NL; m++)
            if (m <= p && k + m < W) acc[m] = acc[m] + sk * s[k + m];
    }
#pragma unroll
    for (uint32_t m = 0; m < NL; m++)
        if (m <= p) part[m * FORMANT_PART_PITCH + q] = acc[m];
}

// ... and the tree over one lag's 64 partial sums, in place
TH_HD double formant_tree(double *row) {
    for (uint32_t h = FORMANT_LANES / 2; h; h >>= 1)
        for (uint32_t q = 0; q < h; q++) row[q] = row[q] + row[q + h];
    return row[0];
}

// steps 3 and 4.  r: p + 1 lags; a, tmp: p + 1 doubles; a[0] = 1.  Returns 0, or 1 for an invalid frame (then a[1 ..], *r0p, *E are 0)
TH_HD uint32_t formant_levinson(const double *r, uint32_t p, double *a, double *tmp, double *r0p, double *E_out) {
    a[0] = 1.0;
    for (uint32_t j = 1; j <= p; j++) a[j] = 0.0;
    *r0p = 0.0;
    *E_out = 0.0;
    const double r0 = r[0];
    if (!(r0 > 0.0) || !(r0 <= FORMANT_DBL_MAX)) return 1;
    const double loaded = r0 * FORMANT_LOADING;
    double E = loaded;
    for (uint32_t i = 1; i <= p; i++) {
        double acc = r[i];
        for (uint32_t j = 1; j < i; j++) acc = acc + a[j] * r[i - j];
        const double kappa = (-acc) / E;
        for (uint32_t j = 1; j < i; j++) tmp[j] = a[j] + kappa * a[i - j];
        for (uint32_t j = 1; j < i; j++) a[j] = tmp[j];
        a[i] = kappa;
        E = E * (1.0 - kappa * kappa);
        if (!(E > 0.0)) {
            for (uint32_t j = 1; j <= p; j++) a[j] = 0.0;
            return 1;
        }
    }
    *r0p = loaded;
    *E_out = E;
    return 0;
}

// step 5, root i of one sweep: the correction w_i from the OLD roots
TH_HD fm_c formant_aberth_w(const double *a, uint32_t p, const double *zr, const double *zi, uint32_t i) {
    const fm_c z{zr[i], zi[i]};
    fm_c P{1.0, 0.0}, D{0.0, 0.0};
    for (uint32_t k = 1; k <= p; k++) {
        D = fm_add(fm_mul(D, z), P);
        P = fm_mul(P, z);
        P.r = P.r + a[k];
    }
    const fm_c q = fm_div(P, D);
    fm_c sigma{0.0, 0.0};
    for (uint32_t j = 0; j < p; j++) {
        if (j == i) continue;
        sigma = fm_add(sigma, fm_div(fm_c{1.0, 0.0}, fm_sub(z, fm_c{zr[j], zi[j]})));
    }
    return fm_div(q, fm_sub(fm_c{1.0, 0.0}, fm_mul(q, sigma)));
}
TH_HD double formant_w_mag(fm_c w) { return w.r * w.r + w.i * w.i; }
// ... and whether the sweep was the last: every |w_i|^2 at or below 2^-80 (a NaN never stops)
TH_HD bool formant_stop(const double *wm, uint32_t p) {
    bool stop = true;
    for (uint32_t i = 0; i < p; i++) stop = stop && (wm[i] <= FORMANT_STOP);
    return stop;
}

}  // namespace th
