// host_math.cpp — see host_math.h.  Each function cites the reference code it mirrors
// (paths relative to the reference checkout).
#include "host_math.h"

#include "envelope_core.h"
#include "stft_plan.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

namespace th {

// SpecSetting::calc_framing_params — src-tauri/src/core/spectrogram.rs:56-98
void calc_framing_params(double win_ms, uint32_t t_overlap, uint32_t f_overlap, uint32_t sr, size_t *hop,
                         size_t *win, size_t *n_fft) {
    const double win_float = win_ms * double(sr) / 1000.;                  // calc_win_length_float
    const double h = std::round(win_float / double(t_overlap));           // f64::round: half away from 0
    const size_t hop_length = h > 0. ? size_t(h) : 0;                     // `as usize` saturates
    const size_t win_length = hop_length * size_t(t_overlap);
    size_t p = 1;
    while (p < win_length) p <<= 1;                                       // next_power_of_two
    *hop = hop_length;
    *win = win_length;
    *n_fft = p * size_t(f_overlap);
}

// Frame count of perform_stft — stft.rs:50-97.  The three-segment construction (front / mid /
// back) yields exactly the frames of a win/2 reflect-padded signal: T = (N + 2*(win/2) - win)/hop + 1
// (tests/test_oracle_numpy.py checks this against the literal restatement).
size_t stft_n_frames(size_t n, size_t win, size_t hop) {
    if (!n || !win || !hop) return 0;
    const size_t padded = n + 2 * (win / 2);
    if (padded < win) return 0;
    return (padded - win) / hop + 1;
}

// calc_normalized_win(Hann, size, n_fft) — windows.rs:12-38,68-83, evaluated in f32 in the
// reference's operation order: x = PI*i/size; (0.5 - 0.5*cos(2x)) + (0*cos(4x) - 0*cos(6x)); / n_fft
std::vector<float> normalized_hann(size_t win, size_t n_fft) {
    std::vector<float> w(win);
    const float pi = 3.14159265358979323846f;
    const float norm = float(n_fft);
    for (size_t i = 0; i < win; i++) {
        const float x = pi * float(i) / float(win);  // size2 - 1 == size for the periodic window
        const float b_ = 0.5f * std::cos(2.0f * x);
        const float c_ = 0.0f * std::cos(4.0f * x);
        const float d_ = 0.0f * std::cos(6.0f * x);
        w[i] = ((0.5f - b_) + (c_ - d_)) / norm;
    }
    return w;
}

// Slaney mel scale — src-common/src/lib.rs:11-43 (f32 instantiation)
static const float kMinLogHz = 1000.f;
static const float kMinLogMel = 15.f;
static const float kLogStep = float(0.06875177742094912);
static const float kLinearScale = float(200. / 3.);

float mel_to_hz(float mel) {
    if (mel < kMinLogMel) return kLinearScale * mel;
    return kMinLogHz * std::exp(kLogStep * (mel - kMinLogMel));
}
float mel_from_hz(float hz) {
    if (hz < kMinLogHz) return hz / kLinearScale;
    return kMinLogMel + std::log(hz / kMinLogHz) / kLogStep;
}

static void linspace(float a, float b, size_t n, float *out) {  // ndarray Array::linspace
    const float step = n > 1 ? (b - a) / float(n - 1) : 0.f;
    for (size_t i = 0; i < n; i++) out[i] = a + step * float(i);
}

// the two f32 frequency arrays of calc_mel_fb (src-common/src/lib.rs:61-67): the bins' frequencies and the n_mel + 2 triangle
// points; fmax < 0 = Nyquist
void mel_fb_points(uint32_t sr, size_t n_fft, size_t n_mel, float fmin, float fmax, std::vector<float> &lin, std::vector<float> &mf) {
    const float f_nyquist = float(double(sr) / 2.);
    if (fmax < 0.f) fmax = f_nyquist;
    const size_t n_freq = n_fft / 2 + 1;
    lin.assign(n_freq, 0.f);
    mf.assign(n_mel + 2, 0.f);
    linspace(0.f, f_nyquist, n_freq, lin.data());
    linspace(mel_from_hz(fmin), mel_from_hz(fmax), n_mel + 2, mf.data());
    for (auto &m : mf) m = mel_to_hz(m);
}

// calc_mel_fb::<f32> — src-common/src/lib.rs:46-89; returns (n_fft/2+1) x n_mel, C order
std::vector<float> calc_mel_fb(uint32_t sr, size_t n_fft, size_t n_mel, float fmin, float fmax, bool do_norm) {
    const size_t n_freq = n_fft / 2 + 1;
    std::vector<float> lin, mf, w(n_freq), fb(n_freq * n_mel, 0.f);
    mel_fb_points(sr, n_fft, n_mel, fmin, fmax, lin, mf);
    for (size_t m = 0; m < n_mel; m++) {
        std::fill(w.begin(), w.end(), 0.f);
        for (size_t i = 0; i < n_freq; i++) {
            const float f = lin[i];
            if (f <= mf[m]) continue;
            if (mf[m] < f && f < mf[m + 1]) w[i] = (f - mf[m]) / (mf[m + 1] - mf[m]);
            else if (f == mf[m + 1]) w[i] = 1.f;
            else if (mf[m + 1] < f && f < mf[m + 2]) w[i] = (mf[m + 2] - f) / (mf[m + 2] - mf[m + 1]);
            else break;
        }
        if (do_norm) {
            float s = 0.f;
            for (size_t i = 0; i < n_freq; i++) s += w[i];
            const float d = std::max(s, std::numeric_limits<float>::epsilon());
            for (size_t i = 0; i < n_freq; i++) w[i] /= d;
        }
        for (size_t i = 0; i < n_freq; i++) fb[i * n_mel + m] = w[i];  // weights.t()
    }
    return fb;
}

// calc_mel_fb_default's n_mel search — src-common/src/lib.rs:91-103
size_t mel_default_n_mel(uint32_t sr, size_t n_fft) {
    const float r = mel_from_hz(float(sr) / 2.f) / mel_from_hz(float(sr) / float(n_fft));
    const float v = std::fma(r, 2.f, -1.f);
    size_t n_mel = (v > 0.f) ? size_t(v) : 0;
    const size_t n_freq = n_fft / 2 + 1;
    n_mel = std::min(n_mel, n_freq);
    while (n_mel > 0) {
        const std::vector<float> fb = calc_mel_fb(sr, n_fft, n_mel, 0.f, -1.f, true);
        bool ok = true;
        for (size_t m = 0; m < n_mel && ok; m++) {
            float s = 0.f;
            for (size_t i = 0; i < n_freq; i++) s += fb[i * n_mel + m];
            ok = s > 0.f;
        }
        if (ok) break;
        n_mel--;
    }
    return n_mel;
}

// FreqScale::hz_range_to_idx — src-common/src/lib.rs:134-159
void hz_range_to_idx(int freq_scale, float hz0, float hz1, uint32_t sr, size_t n, size_t *i0, size_t *i1) {
    if (hz0 >= hz1) {
        *i0 = *i1 = 0;
        return;
    }
    const float half_sr = float(sr) / 2.f;
    const float r0 = freq_scale ? mel_from_hz(hz0) / mel_from_hz(half_sr) : hz0 / half_sr;
    const float r1 = freq_scale ? mel_from_hz(hz1) / mel_from_hz(half_sr) : hz1 / half_sr;
    float lo = std::floor(r0 * float(n));
    if (!(lo > 0.f)) lo = 0.f;
    const float hi = std::ceil(r1 * float(n));
    *i0 = size_t(lo);
    *i1 = hi > 0.f ? size_t(hi) : 0;
}

static inline float rs_min(float a, float b) { return std::isnan(a) ? b : (std::isnan(b) ? a : (a < b ? a : b)); }
static inline float rs_max(float a, float b) { return std::isnan(a) ? b : (std::isnan(b) ? a : (a > b ? a : b)); }

// TrackManager::update_spec_imgs range clamp — core/mod.rs:169-180
void global_db_range(const float *mins, const float *maxs, size_t n, float dB_range, float *mn, float *mx) {
    float lo = INFINITY, hi = -INFINITY;
    for (size_t i = 0; i < n; i++) {
        lo = rs_min(lo, mins[i]);
        hi = rs_max(hi, maxs[i]);
    }
    hi = rs_min(hi, 0.f);
    lo = rs_max(lo, hi - dB_range);
    *mn = lo;
    *mx = hi;
}

// Longest-processing-time-first assignment: units sorted by weight (descending, index ascending
// on ties) go to the currently least-loaded rank (lowest rank on ties).  Equal weights reduce to
// round-robin, e.g. 1024 equal tracks on 8 GPUs = 128 per GPU.  With load0 the ranks start from those loads instead of 0.
void shard_assign(const uint64_t *weights, size_t n, uint32_t world, uint32_t *owner, const uint64_t *load0) {
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return weights[a] > weights[b]; });
    std::vector<uint64_t> load(world, 0);
    if (load0) load.assign(load0, load0 + world);
    for (size_t i : order) {
        uint32_t best = 0;
        for (uint32_t r = 1; r < world; r++)
            if (load[r] < load[best]) best = r;
        owner[i] = best;
        load[best] += weights[i];
    }
}

static inline size_t sat_mul(size_t a, size_t b) {
    size_t r;
    return __builtin_mul_overflow(a, b, &r) ? SIZE_MAX : r;
}
static inline size_t sat_add(size_t a, size_t b) {
    size_t r;
    return __builtin_add_overflow(a, b, &r) ? SIZE_MAX : r;
}
static inline size_t shl_or_max(uint32_t level) { return level < 64 ? (size_t(1) << level) : SIZE_MAX; }
static inline size_t div_ceil(size_t a, size_t b) { return a / b + (a % b != 0); }

// encode_spectrogram_tile geometry — render_tiles.rs:290-313
TileGeom spectrogram_tile_geometry(size_t W, size_t Hh, uint32_t lx, uint32_t ly, uint32_t tx, uint32_t ty) {
    const size_t T = 512, G = 4;
    TileGeom g{};
    g.lod_w = div_ceil(W, shl_or_max(lx));
    g.lod_h = div_ceil(Hh, shl_or_max(ly));
    const size_t sx = sat_mul(tx, T), sy = sat_mul(ty, T);
    const size_t cw = std::min(g.lod_w > sx ? g.lod_w - sx : 0, T);
    const size_t ch = std::min(g.lod_h > sy ? g.lod_h - sy : 0, T);
    g.origin_x = sx > G ? sx - G : 0;
    g.origin_y = sy > G ? sy - G : 0;
    if (cw && ch) {
        const size_t rx = std::min(g.lod_w, sx + cw + G), ry = std::min(g.lod_h, sy + ch + G);
        g.width = rx > g.origin_x ? rx - g.origin_x : 0;
        g.height = ry > g.origin_y ? ry - g.origin_y : 0;
    }
    return g;
}

// encode_waveform_tile geometry — render_tiles.rs:233-241
void waveform_tile_geometry(size_t n, uint32_t level, uint32_t tile, size_t *start, size_t *bins, size_t *spb) {
    const size_t s = shl_or_max(level);
    const size_t tile_samples = sat_mul(1024, s);
    const size_t st = sat_mul(size_t(tile), tile_samples);
    const size_t en = std::min(n, sat_add(st, tile_samples));
    *start = st;
    *spb = s;
    *bins = st >= en ? 0 : div_ceil(en - st, s);
}

static void put_words(uint8_t *out, uint64_t revision, const uint32_t *w, size_t n) {  // little-endian host (x86-64)
    std::memcpy(out, &revision, 8);
    std::memcpy(out + 8, w, 4 * n);
}
void put_spectrogram_tile_header(uint8_t *out, uint64_t revision, const TileGeom &g, uint32_t level_x, uint32_t level_y, uint32_t tile_x,
                                 uint32_t tile_y) {
    const uint32_t w[8] = {(uint32_t)g.width, (uint32_t)g.height, level_x, level_y, tile_x, tile_y, (uint32_t)g.origin_x, (uint32_t)g.origin_y};
    put_words(out, revision, w, 8);
}
void put_waveform_tile_header(uint8_t *out, uint64_t revision, size_t bins, size_t samples_per_bin, uint32_t tile_index) {
    const uint32_t w[4] = {(uint32_t)bins, samples_per_bin > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)samples_per_bin, tile_index, 0u};
    put_words(out, revision, w, 4);
}

// Lanczos3 taps in the arithmetic of the convolution fast_image_resize documents itself as following (Pillow's
// ImagingResample, precompute_coeffs): lanczos(t) = sinc(t) sinc(t / 3) on -3 <= t < 3, sinc(t) = sin(pi t) / (pi t).
static double pil_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}
static double pil_lanczos(double x) {
    if (-3.0 <= x && x < 3.0) return pil_sinc(x) * pil_sinc(x / 3);
    return 0.0;
}

// Window [ (int)(center - support + 0.5), (int)(center + support + 0.5) ) clipped at [lo, hi) = the IMAGE, tap k =
// lanczos(((k + xmin) - center + 0.5) * (1 / filterscale)), taps divided by their sum HERE (one division per tap, not per
// pixel): the kernels then add pixel * tap in ascending order from 0.0 and round half up, which makes a level bit-identical
// to Pillow 12.2's 16-bit Lanczos resize (tests/golden/lod_pillow_cases.npz) wherever that does not overflow 65535.
// wsum stays in the table's layout as 1.0 (x / 1.0 == x exactly).
void build_lod_axis(double origin, double extent, size_t n_out, long lo, long hi, LodAxisHost &ax) {
    const double sc = extent / (double)n_out, f = sc < 1.0 ? 1.0 : sc, sup = 3.0 * f, ss = 1.0 / f;
    ax.start.resize(n_out);
    ax.count.resize(n_out);
    ax.wsum.assign(n_out, 1.0);
    ax.max_taps = 0;
    for (size_t o = 0; o < n_out; o++) {
        const double center = origin + ((double)o + 0.5) * sc;
        long i0 = (long)(center - sup + 0.5), i1 = (long)(center + sup + 0.5);  // (truncation, as the C casts of Pillow)
        if (i0 < lo) i0 = lo;
        if (i1 > hi) i1 = hi;
        if (i1 < i0) i1 = i0;
        ax.start[o] = (int32_t)i0;
        ax.count[o] = (int32_t)(i1 - i0);
        ax.max_taps = std::max<uint32_t>(ax.max_taps, (uint32_t)(i1 - i0));
    }
    if (ax.max_taps == 0) ax.max_taps = 1;
    ax.w.assign(n_out * (size_t)ax.max_taps, 0.0);
    for (size_t o = 0; o < n_out; o++) {
        const double center = origin + ((double)o + 0.5) * sc;
        double *const k = &ax.w[o * (size_t)ax.max_taps];
        double ww = 0.0;
        for (int32_t t = 0; t < ax.count[o]; t++) {
            const double wv = pil_lanczos(((double)(t + ax.start[o]) - center + 0.5) * ss);
            k[t] = wv;
            ww += wv;
        }
        if (ww != 0.0)
            for (int32_t t = 0; t < ax.count[o]; t++) k[t] /= ww;
    }
}

void LodAxisHost::pack(unsigned char *p, size_t n_out) const {
    std::memcpy(p, start.data(), n_out * 4);
    std::memcpy(p + n_out * 4, count.data(), n_out * 4);
    std::memcpy(p + n_out * 8, wsum.data(), n_out * 8);
    std::memcpy(p + n_out * 16, w.data(), w.size() * 8);
}


BluesteinTables bluestein_tables(size_t n_fft, size_t M) {
    BluesteinTables t;
    const size_t nc = n_fft / 2, h = M / 2;
    t.chirp.resize(2 * nc);
    for (size_t n = 0; n < nc; n++) {
        const uint64_t r = (uint64_t)n * n % (2 * (uint64_t)nc);  // e^{-i pi n^2 / nc} has period 2 nc in n^2
        const double a = -M_PI * (double)r / (double)nc;
        t.chirp[2 * n] = std::cos(a);
        t.chirp[2 * n + 1] = std::sin(a);
    }
    t.twm.resize(2 * std::max<size_t>(h, 1));
    for (size_t k = 0; k < std::max<size_t>(h, 1); k++) {
        const double a = -2.0 * M_PI * (double)k / (double)M;
        t.twm[2 * k] = std::cos(a);
        t.twm[2 * k + 1] = std::sin(a);
    }
    t.tws.resize(2 * (nc / 2 + 1));
    for (size_t k = 0; k <= nc / 2; k++) {
        const double a = -2.0 * M_PI * (double)k / (double)n_fft;
        t.tws[2 * k] = std::cos(a);
        t.tws[2 * k + 1] = std::sin(a);
    }
    // bhat = FFT_M(b): radix-2 Stockham, the kernel's own pass structure
    std::vector<double> x(2 * M, 0.0), y(2 * M, 0.0);
    for (size_t n = 0; n < nc; n++) {
        x[2 * n] = t.chirp[2 * n];
        x[2 * n + 1] = -t.chirp[2 * n + 1];
        if (n) {
            x[2 * (M - n)] = t.chirp[2 * n];
            x[2 * (M - n) + 1] = -t.chirp[2 * n + 1];
        }
    }
    for (size_t Ns = 1; Ns < M; Ns <<= 1) {
        const size_t step = h / Ns;
        for (size_t j = 0; j < h; j++) {
            const size_t k = j & (Ns - 1), j0 = (j - k) * 2 + k;
            const double wr = t.twm[2 * k * step], wi = t.twm[2 * k * step + 1];
            const double ar = x[2 * j], ai = x[2 * j + 1], br0 = x[2 * (j + h)], bi0 = x[2 * (j + h) + 1];
            const double br = br0 * wr - bi0 * wi, bi = br0 * wi + bi0 * wr;
            y[2 * j0] = ar + br;
            y[2 * j0 + 1] = ai + bi;
            y[2 * (j0 + Ns)] = ar - br;
            y[2 * (j0 + Ns) + 1] = ai - bi;
        }
        x.swap(y);
    }
    t.bhat = std::move(x);
    return t;
}

// ---------------------------------------------------------------------------------------------- integrated loudness
// StatCalculator::calc (dynamics/stats.rs:56-86) is EbuR128::new(n_ch, sr, Mode::all()) + add_frames_planar_f32 +
// loudness_global() of the ebur128 crate 0.1.10 (Cargo.lock:1192), a port of libebur128.  What follows is libebur128's
// arithmetic; the crate's own source is not pinned here.

// ebur128_init_filter: the high shelf and the high-pass of ITU-R BS.1770-4 designed for `sr`, multiplied into one section
void k_weighting(uint32_t sr, double b[5], double a[5]) {
    const double pi = 3.14159265358979323846;
    double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    double K = std::tan(pi * f0 / (double)sr);
    const double Vh = std::pow(10.0, G / 20.0);
    const double Vb = std::pow(Vh, 0.4996667741545416);
    double pb[3], pa[3] = {1.0, 0.0, 0.0};
    const double rb[3] = {1.0, -2.0, 1.0};
    double ra[3] = {1.0, 0.0, 0.0};
    const double a0 = 1.0 + K / Q + K * K;
    pb[0] = (Vh + Vb * K / Q + K * K) / a0;
    pb[1] = 2.0 * (K * K - Vh) / a0;
    pb[2] = (Vh - Vb * K / Q + K * K) / a0;
    pa[1] = 2.0 * (K * K - 1.0) / a0;
    pa[2] = (1.0 - K / Q + K * K) / a0;
    f0 = 38.13547087602444;
    Q = 0.5003270373238773;
    K = std::tan(pi * f0 / (double)sr);
    ra[1] = 2.0 * (K * K - 1.0) / (1.0 + K / Q + K * K);
    ra[2] = (1.0 - K / Q + K * K) / (1.0 + K / Q + K * K);
    b[0] = pb[0] * rb[0];
    b[1] = pb[0] * rb[1] + pb[1] * rb[0];
    b[2] = pb[0] * rb[2] + pb[1] * rb[1] + pb[2] * rb[0];
    b[3] = pb[1] * rb[2] + pb[2] * rb[1];
    b[4] = pb[2] * rb[2];
    a[0] = pa[0] * ra[0];
    a[1] = pa[0] * ra[1] + pa[1] * ra[0];
    a[2] = pa[0] * ra[2] + pa[1] * ra[1] + pa[2] * ra[0];
    a[3] = pa[1] * ra[2] + pa[2] * ra[1];
    a[4] = pa[2] * ra[2];
}

// the first block is complete after 400 ms, every further one 100 ms later
size_t loudness_n_blocks(size_t n, uint32_t sr) {
    const size_t s100 = loudness_s100(sr), L = 4 * s100;
    return (s100 == 0 || n < L) ? 0 : (n - L) / s100 + 1;
}

// ebur128_init_channel_map: 4 channels L R Ls Rs, 5 channels L R C Ls Rs, otherwise L R C unused Ls Rs unused...
double loudness_channel_weight(uint32_t c, uint32_t n_ch) {
    if (n_ch == 4) return c < 2 ? 1.0 : 1.41;
    if (n_ch == 5) return c < 3 ? 1.0 : 1.41;
    if (c < 3) return 1.0;
    if (c == 4 || c == 5) return 1.41;
    return 0.0;
}

namespace {
struct LoudnessHistogram {
    double boundaries[1001], energies[1000];
    LoudnessHistogram() {
        for (int i = 0; i < 1001; i++) boundaries[i] = std::pow(10.0, ((double)i / 10.0 - 70.0 + 0.691) / 10.0);
        for (int i = 0; i < 1000; i++) energies[i] = std::pow(10.0, ((double)i / 10.0 - 69.95 + 0.691) / 10.0);
    }
    // find_histogram_index: the largest j <= 999 with e >= boundaries[j] (e >= boundaries[0])
    size_t index(double e) const {
        size_t lo = 0, hi = 1000;
        do {
            const size_t mid = (lo + hi) / 2;
            if (e >= boundaries[mid]) lo = mid;
            else hi = mid;
        } while (hi - lo != 1);
        return lo;
    }
};
const LoudnessHistogram &loudness_histogram() {
    static const LoudnessHistogram h;
    return h;
}
}  // namespace

// ebur128_calc_gating_block's histogram update + ebur128_gated_loudness (histogram mode)
double gated_loudness(const double *E, size_t n) {
    const LoudnessHistogram &h = loudness_histogram();
    std::vector<uint64_t> hist(1000, 0);
    for (size_t k = 0; k < n; k++)
        if (E[k] >= h.boundaries[0]) hist[h.index(E[k])]++;  // (NaN compares false: never counted)
    double rel = 0.0;
    uint64_t cnt = 0;
    for (size_t j = 0; j < 1000; j++) {
        rel += (double)hist[j] * h.energies[j];
        cnt += hist[j];
    }
    if (!cnt) return -std::numeric_limits<double>::infinity();
    rel /= (double)cnt;
    rel *= std::pow(10.0, -10.0 / 10.0);  // relative_gate_factor
    size_t start = 0;
    if (rel >= h.boundaries[0]) {
        start = h.index(rel);
        if (rel > h.energies[start]) start++;
    }
    double sum = 0.0;
    cnt = 0;
    for (size_t j = start; j < 1000; j++) {
        sum += (double)hist[j] * h.energies[j];
        cnt += hist[j];
    }
    if (!cnt) return -std::numeric_limits<double>::infinity();
    sum /= (double)cnt;
    return 10.0 * std::log10(sum) - 0.691;
}

size_t loudness_n_short_term(size_t n, uint32_t sr) {
    const size_t s100 = loudness_s100(sr);
    const size_t n_seg = s100 ? n / s100 : 0;
    return n_seg < 30 ? 0 : n_seg - 29;
}

double loudness_lufs(double e) { return 10.0 * std::log10(e) - 0.691; }

double loudness_series_max(const double *lufs, size_t n) {
    double m = -std::numeric_limits<double>::infinity();
    for (size_t k = 0; k < n; k++)
        if (lufs[k] > m) m = lufs[k];  // (NaN compares false)
    return m;
}

// ebur128_loudness_range_multiple (histogram mode) for one state
double loudness_range(const double *E, size_t n) {
    const LoudnessHistogram &h = loudness_histogram();
    std::vector<uint64_t> hist(1000, 0);
    for (size_t k = 0; k < n; k++)
        if (E[k] >= h.boundaries[0]) hist[h.index(E[k])]++;  // (NaN compares false: never counted)
    uint64_t size = 0;
    double power = 0.0;
    for (size_t j = 0; j < 1000; j++) {
        size += hist[j];
        power += (double)hist[j] * h.energies[j];
    }
    if (!size) return 0.0;
    power /= (double)size;
    const double integ = 0.01 * power;  // the relative gate: -20 LU
    size_t idx = 0;
    if (!(integ < h.boundaries[0])) {
        idx = h.index(integ);
        if (integ > h.energies[idx]) idx++;
    }
    size = 0;
    for (size_t j = idx; j < 1000; j++) size += hist[j];
    if (!size) return 0.0;
    const uint64_t lo = (uint64_t)((double)(size - 1) * 0.1 + 0.5), hi = (uint64_t)((double)(size - 1) * 0.95 + 0.5);
    uint64_t cnt = 0;
    size_t j = idx;
    while (cnt <= lo) cnt += hist[j++];
    const double l = h.energies[j - 1];
    while (cnt <= hi) cnt += hist[j++];
    const double hh = h.energies[j - 1];
    return 10.0 * std::log10(hh) - 10.0 * std::log10(l);
}

uint32_t true_peak_factor(uint32_t sr) { return sr < 96000 ? 4 : sr < 192000 ? 2 : 1; }

uint32_t true_peak_filter(uint32_t factor, double coef[TRUE_PEAK_TAPS], uint32_t phase[TRUE_PEAK_TAPS], uint32_t delay[TRUE_PEAK_TAPS]) {
    const double pi = 3.14159265358979323846;
    uint32_t n = 0;
    for (uint32_t j = 0; j < TRUE_PEAK_TAPS; j++) {
        const double m = (double)j - 24.0;
        const double t = m * pi / (double)factor;
        const double sinc = m == 0.0 ? 1.0 : std::sin(t) / t;
        const double c = sinc * (0.5 * (1.0 - std::cos(2.0 * pi * (double)j / 48.0)));
        if (!(std::fabs(c) > 1e-6)) continue;
        coef[n] = c;
        phase[n] = j % factor;
        delay[n] = j / factor;
        n++;
    }
    return n;
}

void kw_transition(const double a[5], double A[16]) {
    std::fill(A, A + 16, 0.0);
    for (int j = 0; j < 4; j++) A[j] = -a[j + 1];
    A[4] = A[9] = A[14] = 1.0;
}

void mat4_pow(const double A[16], uint64_t n, double out[16]) {
    double r[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, p[16], t[16];
    std::memcpy(p, A, sizeof p);
    auto mul = [&](const double *x, const double *y, double *z) {
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) z[4 * i + j] = (x[4 * i] * y[j] + x[4 * i + 1] * y[4 + j]) + (x[4 * i + 2] * y[8 + j] + x[4 * i + 3] * y[12 + j]);
    };
    for (; n; n >>= 1) {
        if (n & 1) {
            mul(r, p, t);
            std::memcpy(r, t, sizeof r);
        }
        if (n > 1) {
            mul(p, p, t);
            std::memcpy(p, t, sizeof p);
        }
    }
    std::memcpy(out, r, sizeof r);
}

namespace {
struct DD {
    double hi, lo;
};
DD dd_fold(DD acc, double c, DD w) {  // acc + c * w, c exact
    const double p = c * w.hi, pe = std::fma(c, w.hi, -p) + c * w.lo;
    const double s = acc.hi + p, bb = s - acc.hi, e = (acc.hi - (s - bb)) + (p - bb) + acc.lo + pe;
    const double h = s + e;
    return DD{h, e - (h - s)};
}
}  // namespace

const LoudnessRate &loudness_rate(uint32_t sr) {
    static std::mutex mu;
    static std::map<uint32_t, std::unique_ptr<LoudnessRate>> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(sr);
    if (it != cache.end()) return *it->second;
    std::unique_ptr<LoudnessRate> R(new LoudnessRate{});
    k_weighting(sr, R->b, R->a);
    R->sr = sr;
    R->s100 = (uint32_t)loudness_s100(sr);
    R->n_sub = (R->s100 + LOUDNESS_CHUNK_MAX - 1) / LOUDNESS_CHUNK_MAX;
    R->cl = (R->s100 + R->n_sub - 1) / R->n_sub;
    R->cl_last = R->s100 - (R->n_sub - 1) * R->cl;
    R->m = (R->cl + 63) / 64;
    if (R->m % 2 == 0) R->m++;
    for (int w = 0; w < 2; w++) {
        const uint32_t len = w ? R->cl_last : R->cl, nl = (len + R->m - 1) / R->m;
        R->e_lane[w] = 64 - nl;
        R->r[w] = len - (nl - 1) * R->m;
    }
    // columns of A^k for k = 1, 2, ...: w <- A w, the filter's own recurrence with zero input, in double-double
    DD W[4][4];  // W[col][row]
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) W[c][r] = DD{c == r ? 1.0 : 0.0, 0.0};
    auto put = [&](double (*dst)[2]) {
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                dst[4 * r + c][0] = W[c][r].hi;
                dst[4 * r + c][1] = W[c][r].lo;
            }
    };
    const uint64_t kmax = std::max<uint64_t>((uint64_t)R->m << 5, R->cl);
    for (uint64_t k = 1; k <= kmax; k++) {
        for (int c = 0; c < 4; c++) {
            DD v0{0.0, 0.0};
            for (int j = 0; j < 4; j++) v0 = dd_fold(v0, -R->a[j + 1], W[c][j]);
            W[c][3] = W[c][2];
            W[c][2] = W[c][1];
            W[c][1] = W[c][0];
            W[c][0] = v0;
        }
        for (int j = 0; j < 6; j++)
            if (k == ((uint64_t)R->m << j)) put(R->scan[j]);
        for (int w = 0; w < 2; w++) {
            if (k == R->r[w]) put(R->rpow[w]);
            if (k == (w ? R->cl_last : R->cl)) put(R->step[w]);
        }
    }
    const LoudnessRate &ref = *R;
    cache[sr] = std::move(R);
    return ref;
}

// ------------------------------------------------------------------------------------------ plan tables (stft_plan.h)
StftGeom stft_geom(size_t win, size_t hop, size_t n_fft) {
    size_t odd_part = n_fft;
    while (odd_part > 1 && odd_part % 2 == 0) odd_part /= 2;
    StftGeom g{};
    g.hop = (uint32_t)hop;
    g.win = (uint32_t)win;
    g.n_fft = (uint32_t)n_fft;
    g.pad_left = (uint32_t)((n_fft - win) / 2);
    g.nc = (uint32_t)(n_fft / 2);
    g.odd_m1 = (uint32_t)odd_part - 1u;
    g.log2_nc = ilog2(g.nc / (uint32_t)odd_part);  // log2 of the power-of-two part of nc
    g.n_freq = (uint32_t)(n_fft / 2 + 1);
    g.n_mel = 0;
    g.height = g.n_freq;
    g.frames_per_tile = 8;  // generic kernel; the wave kernel's tile is set at launch
    return g;
}

std::vector<cf32> build_twiddles(size_t n_fft) {
    std::vector<cf32> tw(n_fft);
    for (size_t i = 0; i < n_fft; i++) {
        const double a = -2.0 * M_PI * (double)i / (double)n_fft;
        tw[i].re = (float)std::cos(a);
        tw[i].im = (float)std::sin(a);
    }
    return tw;
}

WaveWindowHost build_wave_window(const float *w, size_t win, size_t n_fft, int phased_mode) {
    WaveWindowHost out;
    const float half = 0.5f * WAVE_PRESCALE;
    const size_t pad_left = (n_fft - win) / 2;
    auto at = [](std::vector<cf32> &v, size_t i) -> float & { return (i & 1) ? v[i / 2].im : v[i / 2].re; };  // float i of the pairs
    out.wtab.assign(n_fft / 2, cf32{0.f, 0.f});
    for (size_t i = 0; i < win; i++) at(out.wtab, pad_left + i) = half * w[i];
    if (phased_mode == 1) {
        out.phased.assign((96 + n_fft) / 2, cf32{0.f, 0.f});
        for (size_t i = 0; i < win; i++) at(out.phased, 96 + i) = half * w[i];
    } else if (phased_mode == 2 || phased_mode == 3) {
        std::vector<float> t0(n_fft + 2, 0.f);
        for (size_t i = 0; i < win; i++) t0[i] = half * w[i];
        out.phased.assign(128 + n_fft, cf32{0.f, 0.f});
        for (size_t i = 0; i < n_fft; i++) {
            at(out.phased, 128 + i) = t0[i];                    // even table: pairs (t0[2n], t0[2n+1])
            at(out.phased, 128 + n_fft + 128 + i) = t0[i + 1];  // odd table:  pairs (t0[2n+1], t0[2n+2])
        }
    }
    return out;
}

MelRangeHost build_mel_ranges(const float *fb, uint32_t n_freq, uint32_t n_mel) {
    MelRangeHost out;
    out.lo.assign(n_mel, 0);
    out.hi.assign(n_mel, 0);
    for (size_t m = 0; m < n_mel; m++) {
        uint32_t a = n_freq, b = 0;
        for (uint32_t f = 0; f < n_freq; f++)
            if (fb[(size_t)f * n_mel + m] != 0.f) {
                a = std::min(a, f);
                b = f + 1;
            }
        out.lo[m] = b ? a : 0;
        out.hi[m] = b;
    }
    return out;
}

MelMfmaHost build_mel_mfma(const float *fb, const MelRangeHost &rg, uint32_t n_freq, uint32_t n_mel) {
    MelMfmaHost out;
    const uint32_t nt = (n_mel + 15) / 16, kb_n = (n_freq + 15) / 16;
    std::vector<uint32_t> &band = out.band;
    std::vector<float> &bt = out.bt;
    band.assign(3 * (size_t)nt, 0);
    auto fbv = [&](uint32_t f, size_t m) { return (f < n_freq && m < n_mel) ? fb[(size_t)f * n_mel + m] : 0.f; };
    for (uint32_t j = 0; j < nt; j++) {
        // the tile's K band from the per-mel non-zero ranges [lo, hi) (the dense scan over every (bin, mel) of
        // every tile was ~90 M filterbank reads at the 5571-mel default of n_fft 32768)
        uint32_t klo = kb_n, khi = 0;
        for (size_t m = 16 * (size_t)j; m < std::min<size_t>(16 * (size_t)j + 16, n_mel); m++)
            if (rg.hi[m]) {
                klo = std::min(klo, rg.lo[m] / 16);
                khi = std::max(khi, (rg.hi[m] + 15) / 16);
            }
        if (!khi) klo = 0;
        band[3 * j] = klo;
        band[3 * j + 1] = khi;
        band[3 * j + 2] = (uint32_t)(bt.size() / 256);
        for (uint32_t kb = klo; kb < khi; kb++)
            for (uint32_t lane = 0; lane < 64; lane++)
                for (uint32_t st = 0; st < 4; st++) bt.push_back(fbv(16 * kb + 4 * (lane >> 4) + st, 16 * (size_t)j + (lane & 15u)));
    }
    out.zero_block = (uint32_t)(bt.size() / 256);
    bt.insert(bt.end(), 256, 0.f);
    out.kblocks = kb_n;
    out.ntiles = nt;
    std::vector<uint32_t> &slice = out.slice;
    slice.assign(1, 0u);
    uint64_t total = 0;
    for (uint32_t j = 0; j < nt; j++) total += (band[3 * j + 1] - band[3 * j] + 3) / 4 + 1;  // + epilogue
    const uint32_t want = std::min<uint32_t>(TH_MEL_SLICES, nt);
    uint64_t acc_g = 0;
    for (uint32_t j = 0; j < nt; j++) {
        acc_g += (band[3 * j + 1] - band[3 * j] + 3) / 4 + 1;
        if (slice.size() < want && acc_g * want >= total * slice.size() && j + 1 < nt) slice.push_back(j + 1);
    }
    slice.push_back(nt);
    out.n_slices = (uint32_t)slice.size() - 1;
    return out;
}

MelRowsHost build_mel_rows(const float *fb, const MelRangeHost &rg, uint32_t n_freq, uint32_t n_mel) {
    MelRowsHost out;
    constexpr uint32_t W = MEL_ROWS_W;
    uint32_t widest = 0;
    for (size_t m = 0; m < n_mel; m++) widest = std::max(widest, rg.hi[m] - rg.lo[m]);
    const uint32_t ng = (n_mel + 63) / 64, kb_n = (n_freq + 15) / 16;
    if (!(kb_n <= (uint32_t)MEL_ROWS_NKB && n_freq - 1 + W <= 16 * MEL_ROWS_NKB + 4 &&  // (reads stay in the LDS row)
          widest <= W && ng <= (uint32_t)MEL_ROWS_MAX_GROUPS))
        return out;
    out.words.assign((size_t)ng * (W + 1) * 64, 0u);
    for (size_t m = 0; m < n_mel; m++) {
        const size_t at = (m / 64) * (W + 1) * 64 + m % 64;
        out.words[at] = rg.lo[m];
        for (uint32_t t = 0; t < W && rg.lo[m] + t < rg.hi[m]; t++)
            std::memcpy(&out.words[at + (1 + t) * 64], &fb[(size_t)(rg.lo[m] + t) * n_mel + m], 4);
    }
    out.n_groups = ng;
    out.ok = true;
    return out;
}

// ------------------------------------------------------------------------------------------ launch plan (stft_plan.h)
static void launch_fail(StftLaunch &l, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static void launch_fail(StftLaunch &l, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    l.err = TH_ERR_INVALID_ARG;
    l.err_text = buf;
}
#define TH_LAUNCH_REQUIRE(cond, ...)      \
    do {                                  \
        if (!(cond)) {                    \
            launch_fail(l, __VA_ARGS__);  \
            return l;                     \
        }                                 \
    } while (0)

StftLaunch plan_stft_launch(const StftGeom &pg, const StftRoute &r, uint32_t n_cu, int wave_chunk, const th_chan_desc *chans, size_t n_chan) {
    StftLaunch l;
    StftGeom &g = l.g, &ge = l.ge;
    g = ge = pg;
    g.phased = (uint32_t)r.phase_mode;
    const bool wave = r.wave(), mel_second = r.mel_second != StftRoute::MelSecond::None, phased = r.phase_mode != 0;
    // wave kernel: chunk of consecutive frames one wave walks (the first frame of a chunk loads
    // n_fft samples, the rest only hop new ones).  32 amortises that well on large batches; small
    // batches (one track) get shorter chunks so that every wave of the chip has work.
    // interior frames [fa, fb) of a channel: the frame's whole n_fft-sample span [e0, e0 + n_fft), e0 = f*hop - win/2 -
    // pad_left, lies inside the channel (the wave kernel loads it unconditionally); the others are boundary frames
    // phased mode: chunks must start on frames that sit exactly on the 128-sample grid (every fourth)
    auto interior = [&g, &r, phased](const th_chan_desc &d, uint64_t T, uint64_t &fa, uint64_t &fb) {
        if (phased) {
            const int64_t N = (int64_t)d.n_samples, half = (int64_t)(g.win / 2);
            auto delta = [&](int64_t f) { return (((f * (int64_t)g.hop - half) % 128) + 128) % 128; };
            auto start = [&](int64_t f) { return f * (int64_t)g.hop - half - delta(f); };
            int64_t a = 0, b = (int64_t)T;
            while (a < b && (start(a) < 0 || (r.phase_mode == 1 && delta(a) != 0))) a++;  // phased chunks start on the grid
            while (b > a && start(b - 1) + (int64_t)g.n_fft > N) b--;
            fa = (uint64_t)a;
            fb = (uint64_t)b;
            return;
        }
        const uint64_t lead = g.win / 2 + g.pad_left, N = d.n_samples > r.tail_guard ? d.n_samples - r.tail_guard : 0;
        fa = (lead + g.hop - 1) / g.hop;                                  // first f with e0 >= 0
        fb = N + lead >= g.n_fft ? (N + lead - g.n_fft) / g.hop + 1 : 0;  // one past the last f with e0 + n_fft <= N
        fa = std::min<uint64_t>(fa, T);
        fb = std::min<uint64_t>(std::max(fb, fa), T);
    };
    if (wave) {
        uint64_t total = 0;
        for (size_t i = 0; i < n_chan; i++) total += chans[i].n_frames;
        // chunks of `len` frames over the batch's interior frames (+ with_edges: one per boundary frame the wave launch takes)
        auto n_chunks = [&](uint64_t len, bool with_edges) {
            uint64_t n = 0;
            for (size_t i = 0; i < n_chan; i++) {
                uint64_t fa, fb;
                interior(chans[i], chans[i].n_frames, fa, fb);
                n += (fb - fa + len - 1) / len;
                if (with_edges && chans[i].n_samples >= g.n_fft) n += chans[i].n_frames - (fb - fa);
            }
            return n;
        };
        // The launch ends when the last chunk does and every slot (wave, or workgroup) walks its chunks one after the other, so
        // what counts is rounds x chunk length: the length around `want` (at least `lo`) whose chunk count fills the last round best
        auto best_chunk = [&](uint64_t want, uint64_t lo, uint64_t slots) {
            uint64_t best = want, best_cost = ~0ull;
            for (uint64_t cand = std::max<uint64_t>(lo, want - want / 4); cand <= want + want / 4; cand++) {
                const uint64_t cost = (n_chunks(cand, false) + slots - 1) / slots * cand;  // frames a slot walks through, at worst
                if (cost < best_cost || (cost == best_cost && cand > best)) {
                    best_cost = cost;
                    best = cand;
                }
            }
            return best;
        };
        const uint64_t n_waves = (uint64_t)n_cu * (uint64_t)r.waves;
        uint64_t chunk;
        if (r.block_plan && g.log2_nc <= 14) {
            // Workgroup-per-frame plans (n_fft 8192 .. 32768): what runs side by side is one workgroup per CU (two at n_fft 8192),
            // not twelve waves, and a chunk start costs a workgroup launch + its set-up (30-50 us: tables / constants, the first
            // frame) or, in the persistent subwave kernel, a full reload of the resident samples.  About two chunks per slot, the
            // length that fills the last round best (round 5, profiles/r05_ab_block_chunks.txt: n_fft 16384 15 -> 44 frames 0.96 ->
            // 0.84-0.92 ms, 32768 8 -> 43 1.26 -> 1.21, 8192 30 -> 60-90 0.70 -> 0.64-0.69; n_fft 65536 measures 5 % slower with
            // longer chunks and keeps the rule below)
            const uint64_t slots = (uint64_t)n_cu * (g.log2_nc == 12 ? 2u : 1u);
            // (a single track: one frame per chunk, every CU busy)
            chunk = best_chunk(std::min<uint64_t>(128, std::max<uint64_t>(1, total / (slots * 2))), 1, slots);
        } else if (total <= n_waves * 32) {
            // small batch (one track ...): one chunk per wave, all of them assigned statically — the kernel then never
            // touches the queue (3072 waves finding it empty is 25 us of serialised atomics on a 20 us job)
            chunk = std::max<uint64_t>(1, (total + n_waves - 1) / n_waves);
            while (chunk < 32 && n_chunks(chunk, r.edges_in_wave) > n_waves) chunk++;
        } else {
            // around total / (waves x TH_CHUNKS_PER_WAVE), 12 to 40 frames.  Bench workload: 29 frames would be 12416 chunks = 4.04
            // rounds of 3072 waves, i.e. a fifth round for 128 stragglers: 0.520 ms; 30-32 frames 0.507 (r02_chunks).
            chunk = best_chunk(std::min<uint64_t>(32, std::max<uint64_t>(12, total / (n_waves * TH_CHUNKS_PER_WAVE))), 12, n_waves);
        }
        g.frames_per_tile = wave_chunk > 0 ? (uint32_t)wave_chunk : (uint32_t)chunk;
        // The sweep schedule (kernels_stft.hip: 4-frame chunks dealt out in order, next chunk prefetched) — round 4, selector 11
        // only: its memory skeleton streams 3-10 % faster (scripts/ubench/stft_skeleton.hip mode 8), the kernel does not: inside
        // bench.py's step 0.492 / 0.497 / 0.496 ms against 0.495 / 0.495 / 0.494 for the default schedule on one box, alternating,
        // and 8 % slower alone with 1 ms gaps (profiles/r04_ab_sweep.txt) — of which the kernel itself is 1 % (rocprofv3 trace:
        // 480 us against 475, profiles/r04_ab_sweep_kernel_level.txt); the rest is this function building and uploading a
        // seven times longer chunk table per call, which a pipelined step hides and a lone call does not.  With the packed-f32
        // pipeline (-39 % VALU instructions, +-0) that makes three independent changes of what the kernel DOES per frame that do
        // not change what a launch TAKES: it runs at the package power cap, where time follows flops + bytes, and neither moved.
        l.sweep = r.sweep && total > n_waves * 32;
        if (l.sweep) g.frames_per_tile = 4;
        if (r.phase_mode == 1) g.frames_per_tile = std::max<uint32_t>(4, (g.frames_per_tile + 3) / 4 * 4);  // chunks start on the grid
    } else {
        g.frames_per_tile = 8;
        // (short transforms — n_fft 256 and below, the generic kernel's only full plans: a tile of 8 frames is one round of its frames-side-by-side
        // loop, and the workgroup's set-up and (min, max) fold then cost as much as the frames; up to 64 frames a tile where the batch still fills the chip)
        if (g.nc <= 256 && g.odd_m1 == 0) {
            uint64_t all = 0;
            for (size_t i = 0; i < n_chan; i++) all += chans[i].n_frames;
            const uint64_t want = all / ((uint64_t)n_cu * 16u);
            g.frames_per_tile = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(8, want / 8 * 8));
        }
    }
    ge.frames_per_tile = 1;
    if (mel_second) l.amp_row0.assign(n_chan, 0);
    auto add = [](std::vector<ChanJob> &v, std::vector<uint32_t> &st, uint64_t &n_tiles, const StftGeom &gg,
                  const th_chan_desc &d, uint32_t T, uint32_t fb0, uint32_t fe0, uint32_t slot, bool wave_edge = false) {
        if (fb0 >= fe0) return;
        const uint32_t pitch = d.spec_pitch ? (uint32_t)d.spec_pitch : gg.height;
        v.push_back(ChanJob{d.wav, d.spec, (uint32_t)d.n_samples, T, fb0, fe0, slot, pitch, wave_edge ? 1u : 0u, 0u});
        st.push_back((uint32_t)n_tiles);
        const uint32_t fpt = wave_edge ? 1u : gg.frames_per_tile;
        n_tiles += (fe0 - fb0 + fpt - 1) / fpt;
    };
    for (size_t i = 0; i < n_chan; i++) {
        const th_chan_desc &d = chans[i];
        TH_LAUNCH_REQUIRE(d.wav && d.spec, "channel %zu: NULL device pointer", i);
        TH_LAUNCH_REQUIRE(d.n_samples >= 1 && d.n_samples < (1ull << 31) - 2 * g.n_fft, "channel %zu: n_samples=%llu out of range",
                          i, (unsigned long long)d.n_samples);
        const size_t T = stft_n_frames(d.n_samples, g.win, g.hop);
        TH_LAUNCH_REQUIRE(d.n_frames == T, "channel %zu: n_frames=%llu but the framing gives %zu", i,
                          (unsigned long long)d.n_frames, T);
        TH_LAUNCH_REQUIRE(d.spec_pitch == 0 || (d.spec_pitch >= g.height && d.spec_pitch < (1ull << 31)),
                          "channel %zu: spec_pitch %llu < height %u", i, (unsigned long long)d.spec_pitch, g.height);
        if (!wave) {
            add(l.jobs, l.tile_start, l.tiles, g, d, (uint32_t)T, 0, (uint32_t)T, (uint32_t)i);
        } else {
            uint64_t fa, fb;
            interior(d, T, fa, fb);
            add(l.jobs, l.tile_start, l.tiles, g, d, (uint32_t)T, (uint32_t)fa, (uint32_t)fb, (uint32_t)i);
            if (mel_second && fa < fb) {
                l.amp_row0[i] = l.amp_rows;
                l.amp_rows += T;
                l.mel_jobs.push_back(MelJob{nullptr, d.spec, (uint32_t)fa, (uint32_t)fb,
                                            (uint32_t)(d.spec_pitch ? d.spec_pitch : g.height), (uint32_t)i});
                l.mel_start.push_back((uint32_t)l.mel_tiles);
                l.mel_tiles += (fb - fa + MEL_TILE_FRAMES - 1) / MEL_TILE_FRAMES;
            }
            // boundary frames of channels with at least n_fft samples also go to the wave kernel where the route says so; a
            // single reflection is not enough for shorter channels
            if (r.edges_in_wave && d.n_samples >= g.n_fft) {
                add(l.jobs, l.tile_start, l.tiles, g, d, (uint32_t)T, 0, (uint32_t)fa, (uint32_t)i, true);
                add(l.jobs, l.tile_start, l.tiles, g, d, (uint32_t)T, (uint32_t)fb, (uint32_t)T, (uint32_t)i, true);
            } else {
                add(l.edge, l.edge_start, l.edge_tiles, ge, d, (uint32_t)T, 0, (uint32_t)fa, (uint32_t)i);
                add(l.edge, l.edge_start, l.edge_tiles, ge, d, (uint32_t)T, (uint32_t)fb, (uint32_t)T, (uint32_t)i);
            }
        }
        TH_LAUNCH_REQUIRE(l.tiles < (1ull << 31) && l.edge_tiles < (1ull << 31), "batch too large for one launch");
    }
    l.tile_start.push_back((uint32_t)l.tiles);
    l.edge_start.push_back((uint32_t)l.edge_tiles);
    l.mel_start.push_back((uint32_t)l.mel_tiles);
    if (wave) {
        l.chunk_tab.resize((size_t)l.tiles * 2);
        for (size_t j = 0; j < l.jobs.size(); j++) {
            const uint32_t fpt = l.jobs[j].edge ? 1u : g.frames_per_tile;
            for (uint32_t t = l.tile_start[j]; t < l.tile_start[j + 1]; t++) {
                l.chunk_tab[2 * (size_t)t] = (uint32_t)j;
                l.chunk_tab[2 * (size_t)t + 1] = l.jobs[j].f_begin + (t - l.tile_start[j]) * fpt;
            }
            if (!l.post.empty() && l.post.back().mm_index == l.jobs[j].mm_index) l.post.back().t1 = l.tile_start[j + 1];
            else l.post.push_back(WavePostJob{l.tile_start[j], l.tile_start[j + 1], l.jobs[j].mm_index, 0u});
        }
    }
    // (min, max) slots: when every frame of every channel is in the wave launch, its last workgroup initialises and fills
    // them (no init launch); otherwise the caller initialises them and every kernel adds with atomics
    l.all_in_wave = wave && !mel_second && l.edge.empty() && l.tiles > 0;
    return l;
}
#undef TH_LAUNCH_REQUIRE

// ---------------------------------------------------------------------------------------------- normalisation, limiter parameters
// Normalize::normalize_default — dynamics/normalize.rs:23-45
bool normalize_gain(int kind, float target, double global_lufs, float rms_dB, float max_peak_dB, float *gain) {
    float stat;
    switch (kind) {
        case TH_NORM_OFF: *gain = 1.0f; return true;
        case TH_NORM_LUFS: stat = (float)global_lufs; break;
        case TH_NORM_RMS_DB: stat = rms_dB; break;
        case TH_NORM_PEAK_DB: stat = max_peak_dB; break;
        default: return false;
    }
    *gain = powf(10.0f, (target - stat) / 20.0f);
    return true;
}

// PerfectLimiter::new(sr, 1., 5., 15., 40.) — limiter.rs:59-77; PeakHold::resize — envelope.rs:374-377;
// BoxStackFilter::with_num_layers(attack, 3) -> set(attack) — envelope.rs:206-265
bool limiter_params(uint32_t sr, LimiterParams *out) {
    const double attack = std::round(5. * (double)sr / 1000.);  // f64::round: half away from zero
    if (!(attack >= 1.)) return false;
    out->attack = (uint32_t)attack;
    out->hold_length = (uint32_t)std::round((double)sr * 20. / 1000.);
    out->release_samples = 40. * (double)sr / 1000.;
    // optimal_ratios(3) = HARDCODED_RATIOS[3..6], normalised by their sum (setup_layers)
    double ratio[3] = {0.404078562416, 0.334851475794, 0.261069961789};
    const double sum = ((0. + ratio[0]) + ratio[1]) + ratio[2];
    for (double &r : ratio) r /= sum;
    const size_t order = out->attack - 1;
    size_t total = 0;
    double err[3];
    for (int i = 0; i < 3; i++) {
        const double frac = ratio[i] * (double)order;
        const size_t lo = (size_t)frac;
        out->box_len[i] = (uint32_t)lo + 1;
        err[i] = (double)lo - frac;
        total += lo;
    }
    for (size_t k = total; k < order; k++) {  // the layer with the least length error grows (the first of equals)
        int i_min = 0;
        double mn = INFINITY;
        for (int i = 0; i < 3; i++)
            if (err[i] < mn) {
                i_min = i;
                mn = err[i];
            }
        out->box_len[i_min] += 1;
        err[i_min] += 1.;
    }
    return true;
}

float db_from_amp(float x) {
    if (std::isnan(x) || std::signbit(x)) return NAN;
    return x == 0.0f ? -INFINITY : (float)(20.0 * std::log10((double)x));
}

bool spectrum_frame_range(uint32_t sr, size_t hop, size_t n_frames, double start_sec, double end_sec, size_t *f0, size_t *f1) {
    if (!(start_sec >= 0.0) || std::isinf(start_sec) || std::isnan(end_sec) || end_sec < start_sec || sr == 0 || hop == 0) return false;
    auto first_at_or_after = [&](double sec) -> size_t {  // (sec >= 0)
        const double x = std::ceil((sec * (double)sr) / (double)hop);
        return x >= (double)n_frames ? n_frames : (size_t)x;
    };
    *f0 = first_at_or_after(start_sec);
    *f1 = std::isinf(end_sec) ? n_frames : std::max(*f0, first_at_or_after(end_sec));
    return true;
}

int envelope_range(uint32_t sr, uint64_t n_samples, double start_sec, double end_sec, uint32_t n_cols, double *A, double *B) {
    if (std::isnan(start_sec) || std::isnan(end_sec) || start_sec < 0.0 || std::isinf(start_sec)) return 1;
    if (sr == 0 || n_samples == 0 || n_cols == 0 || n_cols > TH_ENVELOPE_MAX_COLS) return 1;
    const double N = (double)n_samples;
    auto clamp = [N](double v) { return v < 0.0 ? 0.0 : (v > N ? N : v); };
    *A = clamp(start_sec * (double)sr);
    *B = end_sec == INFINITY ? N : clamp(end_sec * (double)sr);
    return *B > *A ? 0 : 1;
}

int envelope_edges(uint32_t sr, uint64_t n_samples, double start_sec, double end_sec, uint32_t n_cols, uint64_t *edges) {
    double A, B;
    if (envelope_range(sr, n_samples, start_sec, end_sec, n_cols, &A, &B) != 0) return 1;
    const double W = (double)n_cols;
    const uint64_t last = (uint64_t)std::ceil(B);
    for (uint32_t j = 0; j < n_cols; j++) {
        const double t = (B - A) * (double)j;  // (named steps: a product, a quotient, a sum, each rounded once)
        const double q = t / W;
        edges[j] = std::min((uint64_t)std::ceil(A + q), last);
    }
    edges[n_cols] = last;
    return 0;
}

int waveform_figure_span(const float col[4], const float *left, uint32_t out_h, float amp_lo, float amp_hi, uint32_t thickness, int32_t *y_top,
                         int32_t *y_bot, int *draws) {
    if (out_h == 0 || out_h > TH_FIGURE_MAX_DIM || !std::isfinite(amp_lo) || !std::isfinite(amp_hi) || !(amp_lo < amp_hi) ||
        thickness > 256u * out_h)
        return 1;
    *y_top = *y_bot = 0;
    *draws = lane_span(col, left, out_h, amp_lo, amp_hi, thickness, y_top, y_bot) ? 1 : 0;
    return 0;
}

int wav_header(uint32_t bps, uint32_t sr, uint32_t n_ch, uint64_t n_frames, uint8_t out[64], size_t *header_len, size_t *pad_len) {
    if (n_ch == 0 || sr == 0 || bps < 2 || bps > 4) return 1;
    const bool flt = bps == 4;
    const uint64_t block = (uint64_t)n_ch * bps, rate = block * sr;
    if (n_ch > 65535 || block > 65535 || rate > UINT32_MAX) return 2;
    if (n_frames > UINT32_MAX / block) return 2;  // (the data alone)
    const uint64_t data = n_frames * block, pad = data & 1, hl = flt ? 58 : 44;
    const uint64_t riff = hl - 8 + data + pad;
    if (riff > UINT32_MAX) return 2;
    auto u16 = [&](size_t at, uint32_t v) {
        out[at] = (uint8_t)v;
        out[at + 1] = (uint8_t)(v >> 8);
    };
    auto u32 = [&](size_t at, uint64_t v) {
        u16(at, (uint32_t)v & 0xffff);
        u16(at + 2, (uint32_t)(v >> 16) & 0xffff);
    };
    std::memset(out, 0, 64);
    std::memcpy(out, "RIFF", 4);
    u32(4, riff);
    std::memcpy(out + 8, "WAVEfmt ", 8);
    u32(16, flt ? 18 : 16);
    u16(20, flt ? 3 : 1);
    u16(22, n_ch);
    u32(24, sr);
    u32(28, rate);
    u16(32, (uint32_t)block);
    u16(34, bps * 8);
    size_t at = 36;
    if (flt) {
        u16(36, 0);  // cbSize
        std::memcpy(out + 38, "fact", 4);
        u32(42, 4);
        u32(46, n_frames);
        at = 50;
    }
    std::memcpy(out + at, "data", 4);
    u32(at + 4, data);
    *header_len = (size_t)hl;
    *pad_len = (size_t)pad;
    return 0;
}

// ---- polyphase sinc resampler
int resample_plan(uint32_t sr_in, uint32_t sr_out, th_resample_plan *out) {
    if (sr_in == 0 || sr_out == 0) return 1;
    uint32_t a = sr_in, b = sr_out;
    while (b) {
        const uint32_t t = a % b;
        a = b;
        b = t;
    }
    const uint32_t L = sr_out / a, M = sr_in / a;
    const uint64_t Z = 128;
    const uint64_t K = L >= M ? Z : (Z * M + L - 1) / L;
    if (2 * K > TH_RESAMPLE_MAX_TAPS) return 2;
    if ((uint64_t)L * 2 * K > TH_RESAMPLE_MAX_COEFS) return 2;
    out->L = L;
    out->M = M;
    out->half_taps = (uint32_t)K;
    out->rho = L >= M ? 1.0 : (double)L / (double)M;
    out->cutoff = out->rho * 0.95;
    return 0;
}

bool resample_n_out(size_t n_in, const th_resample_plan &p, size_t *n_out) {
    const unsigned __int128 n = ((unsigned __int128)n_in * p.L + p.M - 1) / p.M;
    if (n > (unsigned __int128)UINT64_MAX / p.M) return false;  // (every j M of the track, and n_out M, fit 64 bits)
    *n_out = (size_t)n;
    return true;
}

namespace {
const double RS_PI = 3.14159265358979323846;
double rs_sinc(double x) { return x == 0.0 ? 1.0 : std::sin(RS_PI * x) / (RS_PI * x); }
// the squared 4-term Blackman-Harris window, 0 for |u| >= 1
double rs_window(double u) {
    if (!(std::fabs(u) < 1.0)) return 0.0;
    const double bh = 0.35875 + 0.48829 * std::cos(RS_PI * u) + 0.14128 * std::cos(2.0 * RS_PI * u) + 0.01168 * std::cos(3.0 * RS_PI * u);
    return bh * bh;
}
// work(i) for i in [0, n) on up to max_thr threads (at most 16, at most the machine's), this thread among them
template <class F>
void on_threads(uint32_t n, size_t max_thr, F work_one) {
    const size_t n_thr = std::min<size_t>(std::max<size_t>(1, max_thr), std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
    std::atomic<uint32_t> next{0};
    auto work = [&]() {
        for (uint32_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) work_one(i);
    };
    std::vector<std::thread> thr;
    try {
        for (size_t i = 1; i < n_thr; i++) thr.emplace_back(work);
    } catch (...) {  // (no more threads: the ones that started and this one do all of it)
    }
    work();
    for (auto &t : thr) t.join();
}
}  // namespace

void resample_row(const th_resample_plan &p, uint32_t r, double *h64, float *c32) {
    const double Z = 128.0;
    const int64_t K = p.half_taps;
    const double frac = (double)r / (double)p.L;
    for (int64_t k = 0; k < 2 * K; k++) {
        const double t = (double)(k - K + 1) - frac;
        const double u = p.rho * t / Z;
        double h = 0.0;
        if (std::fabs(u) < 1.0) h = p.cutoff * rs_sinc(p.cutoff * t) * rs_window(u);
        if (h64) h64[k] = h;
        if (c32) c32[k] = (float)h;
    }
}

void resample_table(const th_resample_plan &p, float *table) {
    const size_t taps = 2 * (size_t)p.half_taps;
    on_threads(p.L, (size_t)p.L * taps / 65536, [&](uint32_t r) { resample_row(p, r, nullptr, table + (size_t)r * taps); });
}

// ---- band filter of the export (include/thesia_amd.h "Export what a spectrogram box holds")
int band_plan_for(uint32_t sr, uint32_t mode, double f_lo_hz, double f_hi_hz, double trans_hz, th_band_plan *out) {
    if (sr == 0 || mode > TH_BAND_STOP) return 1;
    const double nyq = (double)sr / 2.0;
    if (f_lo_hz != f_lo_hz || f_hi_hz != f_hi_hz || trans_hz != trans_hz) return 1;
    const double f_hi = std::min(f_hi_hz, nyq), f_lo = f_lo_hz;
    if (f_lo < 0.0 || f_lo >= f_hi || trans_hz < 0.0 || trans_hz > nyq) return 1;
    const bool whole = f_lo == 0.0 && f_hi == nyq;
    if (whole && mode == TH_BAND_STOP) return 1;
    *out = th_band_plan{};
    out->mode = mode;
    out->f_lo_hz = f_lo;
    out->f_hi_hz = f_hi;
    if (whole) return 0;  // (identity: no filter, whatever the width asked for)
    const double K = trans_hz == 0.0 ? (double)TH_BAND_DEFAULT_HALF_TAPS : std::ceil((16.0 * (double)sr) / (5.0 * trans_hz));
    if (!(2.0 * K <= (double)TH_BAND_MAX_TAPS)) return 2;
    out->half_taps = (uint32_t)K;
    out->trans_hz = (16.0 * (double)sr) / (5.0 * K);
    return 0;
}

namespace {
double band_tap(uint32_t sr, const th_band_plan &p, int64_t k) {
    const int64_t K = p.half_taps, ti = k - K + 1;
    const double t = (double)ti, a = 2.0 * p.f_hi_hz / (double)sr, c = 2.0 * p.f_lo_hz / (double)sr;
    const double delta = ti == 0 ? 1.0 : 0.0;
    const double A = a < 1.0 ? a * rs_sinc(a * t) : delta;
    const double pass = (A - c * rs_sinc(c * t)) * rs_window(t / (double)K);
    return p.mode == TH_BAND_STOP ? delta - pass : pass;
}
}  // namespace

void band_row(uint32_t sr, const th_band_plan &p, double *h64, float *c32) {
    const uint32_t taps = 2 * p.half_taps, per = 4096, n_parts = (taps + per - 1) / per;
    on_threads(n_parts, n_parts, [&](uint32_t part) {
        for (uint32_t k = part * per; k < std::min(taps, (part + 1) * per); k++) {
            const double h = band_tap(sr, p, k);
            if (h64) h64[k] = h;
            if (c32) c32[k] = (float)h;
        }
    });
}

void band_response(uint32_t sr, const float *c32, uint32_t half_taps, const double *hz, size_t n, double *db) {
    const int64_t K = half_taps;
    const uint32_t per = 8, n_parts = (uint32_t)((n + per - 1) / per);
    on_threads(n_parts, (size_t)n_parts * half_taps / 32768, [&](uint32_t part) {
        for (size_t i = (size_t)part * per; i < std::min(n, ((size_t)part + 1) * per); i++) {
            const double w = 2.0 * RS_PI * hz[i] / (double)sr;
            double re = 0.0, im = 0.0;
            for (int64_t k = 0; k < 2 * K; k++) {
                const double ph = w * (double)(k - K + 1);
                re += (double)c32[k] * std::cos(ph);
                im -= (double)c32[k] * std::sin(ph);
            }
            db[i] = 20.0 * std::log10(std::sqrt(re * re + im * im));
        }
    });
}

}  // namespace th
