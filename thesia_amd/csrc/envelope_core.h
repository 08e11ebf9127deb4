// envelope_core.h — the two steps of the waveform envelope that the host and the device must do alike, written once: how a column's
// (min, max, sum, sum of squares) become its four floats, and the integer span of a column of a waveform lane (th_waveform_figure_span,
// host_math.cpp; kernels_envelope.hip).  The definitions are those of include/thesia_amd.h ("Waveform envelope").
#pragma once
#include <stdint.h>

#include "stft_core.h"  // TH_HD

namespace th {

// (min, max, mean, rms) of c > 0 samples: the quotients and the root in f64, one rounding to f32 each
TH_HD void envelope_finish(float mn, float mx, double sum, double sumsq, uint64_t c, float out[4]) {
    out[0] = mn;
    out[1] = mx;
    out[2] = (float)(sum / (double)c);
    out[3] = (float)__builtin_sqrt(sumsq / (double)c);
}

// Y(v) = clamp(floor((hi - v) / (hi - lo) out_h 256 + 0.5), 0, 256 out_h): one rounded f64 operation per step, in this order
// (the product with 256 is exact, so a contraction with the sum that follows cannot change it)
TH_HD int32_t lane_row(double hi, double lo, float v, uint32_t out_h) {
    const double top = 256.0 * (double)out_h;
    double t = hi - (double)v;
    t = t / (hi - lo);
    t = t * (double)out_h;
    t = t * 256.0;
    t = __builtin_floor(t + 0.5);
    if (!(t > 0.0)) t = 0.0;
    if (t > top) t = top;
    return (int32_t)t;
}

// The rows [*y_top, *y_bot) in 1/256 pixel that column `col` = (min, max, mean, rms) of a lane draws, joined to its left neighbour
// (left: that column's four values, un-joined; NULL for column 0).  false: the column draws nothing
TH_HD bool lane_span(const float col[4], const float *left, uint32_t out_h, float amp_lo, float amp_hi, uint32_t thickness, int32_t *y_top,
                     int32_t *y_bot) {
    float mn = col[0], mx = col[1];
    if (mx < mn || col[2] != col[2]) return false;
    if (left && !(left[1] < left[0])) {
        if (mx < left[0]) mx = left[0];
        if (mn > left[1]) mn = left[1];
    }
    const int32_t top = (int32_t)(256u * out_h);
    int32_t yt = lane_row((double)amp_hi, (double)amp_lo, mx, out_h), yb = lane_row((double)amp_hi, (double)amp_lo, mn, out_h);
    if (yb - yt < (int32_t)thickness) {
        const int32_t s = yt + yb - (int32_t)thickness;
        yt = s >= 0 ? s / 2 : -((1 - s) / 2);  // floor(s / 2)
        yb = yt + (int32_t)thickness;
        yt = yt < 0 ? 0 : (yt > top ? top : yt);
        yb = yb < 0 ? 0 : (yb > top ? top : yb);
    }
    *y_top = yt;
    *y_bot = yb;
    return true;
}

}  // namespace th
