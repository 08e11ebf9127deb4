// host_math.h — plan-preparation arithmetic done once on the host, exactly as the reference's
// SpectrogramAnalyzer::prepare does (spectrogram.rs:116-154): window and mel filterbank tables,
// framing parameters, tile geometry.  These are tables/shape decisions, not the hot path.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/thesia_amd.h"  // th_resample_plan

namespace th {

void calc_framing_params(double win_ms, uint32_t t_overlap, uint32_t f_overlap, uint32_t sr, size_t *hop,
                         size_t *win, size_t *n_fft);
size_t stft_n_frames(size_t n, size_t win, size_t hop);
std::vector<float> normalized_hann(size_t win, size_t n_fft);
float mel_from_hz(float hz);
float mel_to_hz(float mel);
std::vector<float> calc_mel_fb(uint32_t sr, size_t n_fft, size_t n_mel, float fmin, float fmax, bool do_norm);
void mel_fb_points(uint32_t sr, size_t n_fft, size_t n_mel, float fmin, float fmax, std::vector<float> &lin, std::vector<float> &mf);
size_t mel_default_n_mel(uint32_t sr, size_t n_fft);
void hz_range_to_idx(int freq_scale, float hz0, float hz1, uint32_t sr, size_t n, size_t *i0, size_t *i1);
// load0 (world entries, may be NULL = all zero): the ranks' loads before these units (th_tmg: the resident tracks' weights)
void shard_assign(const uint64_t *weights, size_t n, uint32_t world, uint32_t *owner, const uint64_t *load0 = nullptr);
void global_db_range(const float *mins, const float *maxs, size_t n, float dB_range, float *mn, float *mx);

// Tables of a Bluestein plan (stft_bluestein_kernel, kernels_stft.hip): interleaved (re, im) doubles.  nc = n_fft / 2 points,
// M = 2^m >= 2 nc - 1.  chirp[n] = e^{-i pi n^2 / nc} (n^2 reduced mod 2 nc before the angle is formed), bhat = FFT_M of
// b[n] = b[M - n] = conj chirp[n], twm[k] = e^{-2 pi i k / M} (k < M / 2), tws[k] = e^{-2 pi i k / n_fft} (k <= nc / 2).
struct BluesteinTables {
    std::vector<double> chirp, bhat, twm, tws;
};
BluesteinTables bluestein_tables(size_t n_fft, size_t M);

struct TileGeom {
    size_t width, height, origin_x, origin_y, lod_w, lod_h;
};
TileGeom spectrogram_tile_geometry(size_t W, size_t Hh, uint32_t lx, uint32_t ly, uint32_t tx, uint32_t ty);
void waveform_tile_geometry(size_t n, uint32_t level, uint32_t tile, size_t *start, size_t *bins, size_t *spb);
// The little-endian headers in front of a tile's payload (render_tiles.rs:171-188, :232-279): 40 bytes {revision u64, width, height,
// level_x, level_y, tile_x, tile_y, origin_x, origin_y u32} and 24 bytes {revision u64, bins, samples per bin (saturated to u32),
// tile_index, 0 u32}
void put_spectrogram_tile_header(uint8_t *out, uint64_t revision, const TileGeom &g, uint32_t level_x, uint32_t level_y, uint32_t tile_x,
                                 uint32_t tile_y);
void put_waveform_tile_header(uint8_t *out, uint64_t revision, size_t bins, size_t samples_per_bin, uint32_t tile_index);

// Lanczos3 tap table of one axis of resize_spectrogram_tile (render_tiles.rs:354-393; PARITY UNPINNED against
// fast_image_resize 6.0.0, whose source is not vendored: the textbook filter, exactly as oracle/thesia_oracle.c builds
// it).  n_out outputs over the source interval [origin, origin + extent); output o: taps for the source indices
// start[o] .. start[o] + count[o] - 1 (clamped to [lo, hi)), weights w[o * max_taps + t], their sum wsum[o].
struct LodAxisHost {
    std::vector<int32_t> start, count;
    std::vector<double> wsum, w;
    uint32_t max_taps = 0;
    size_t blob_bytes(size_t n_out) const { return n_out * 16 + n_out * (size_t)max_taps * 8; }
    void pack(unsigned char *p, size_t n_out) const;  // [start i32][count i32][wsum f64][w f64], as LodAxis reads it
};
void build_lod_axis(double origin, double extent, size_t n_out, long lo, long hi, LodAxisHost &ax);

// ---- integrated loudness (StatCalculator::calc, dynamics/stats.rs:56-86: the ebur128 crate 0.1.10, a port of libebur128 —
// PARITY UNPINNED) and the momentary block series behind it
constexpr uint32_t LOUDNESS_MIN_SR = 16, LOUDNESS_MAX_SR = 2822400;  // the rates EbuR128::new accepts
inline bool loudness_rate_ok(uint32_t sr) { return sr >= LOUDNESS_MIN_SR && sr <= LOUDNESS_MAX_SR; }
// the K-weighting filter as one 4th-order section (the shelf times the high-pass), in libebur128's arithmetic
void k_weighting(uint32_t sr, double b[5], double a[5]);
inline size_t loudness_s100(uint32_t sr) { return (sr + 5) / 10; }  // samples per 100 ms; a gating block is 4 of them
size_t loudness_n_blocks(size_t n_samples, uint32_t sr);
// weight of channel c of n_ch in a block energy under the default channel map (L R C: 1, Ls Rs: 1.41, unused: 0)
double loudness_channel_weight(uint32_t c, uint32_t n_ch);
// histogram-mode gating of the block energies (absolute gate -70 LUFS, relative gate -10 LU, 0.1 LU bins) -> integrated LUFS
double gated_loudness(const double *block_energies, size_t n);
// The filter's recurrence on its state S = (v1, v2, v3, v4) over a run of samples is S' = A^len S + z, z = the run from zero state.
// A: the 4x4 (row-major) transition of one sample with zero input; mat4_pow: A^n by squaring, in f64.
void kw_transition(const double a[5], double A[16]);
void mat4_pow(const double A[16], uint64_t n, double out[16]);
// What the loudness kernels (kernels_loudness.hip) need of one rate.  A 100 ms segment is cut into n_sub chunks of cl samples (the
// last one cl_last) of at most LOUDNESS_CHUNK_MAX; a chunk is one wave, whose lane l runs samples [len - (64 - l) m, len - (63 - l) m)
// of it (m odd: the lanes' LDS reads hit 32 different banks); lanes below e_lane[w] are empty, lane e_lane[w] runs r[w] samples
// (w = 0: a chunk of cl samples, 1: of cl_last).  The powers of A are double-double (hi, lo) pairs, made by iterating the
// recurrence itself: the DF-II transition is far from normal (|A^75| = 3.2e3 at 48 kHz, 4.7e4 at 192 kHz) and its powers by
// squaring, or products of them with a state in f64, lose up to 6 digits of the state.
constexpr uint32_t LOUDNESS_CHUNK_MAX = 4800;
struct LoudnessRate {
    double b[5], a[5];
    double scan[6][16][2];  // A^(m 2^j): the lane scan's step j
    double rpow[2][16][2];  // A^r[w]: the chunk's start state through the first non-empty lane
    double step[2][16][2];  // A^cl, A^cl_last: the carry from chunk to chunk
    uint32_t sr, s100, n_sub, cl, cl_last, m, e_lane[2], r[2], pad_;
};
const LoudnessRate &loudness_rate(uint32_t sr);  // (cached per rate; sr must satisfy loudness_rate_ok)

// ---- the loudness meter (th_tm_get_loudness_meters): EBU Tech 3342 loudness range, the momentary / short-term series as LUFS and
// the true-peak interpolator, restated from libebur128 (PARITY UNPINNED like the block above)
// 3 s blocks, one per 100 ms segment: n_seg - 29 of them, n_seg = n / s100, or 0 when n_seg < 30
size_t loudness_n_short_term(size_t n_samples, uint32_t sr);
// 10 log10(E) - 0.691 in f64: E = 0 gives -inf, NaN stays NaN
double loudness_lufs(double energy);
// the largest non-NaN value of a LUFS series, -inf when there is none
double loudness_series_max(const double *lufs, size_t n);
// ebur128_loudness_range in histogram mode over the short-term energies taken once per second: the 1000 bins of gated_loudness,
// relative gate -20 LU, the 10th and 95th percentile of what passes -> LU (0 when nothing passes)
double loudness_range(const double *short_term_energies, size_t n);
// The true-peak interpolator: a 49-tap Hann-windowed sinc for an oversampling factor F (4 below 96 kHz, 2 below 192 kHz, else 1),
// c_j = sinc((j - 24) pi / F) 0.5 (1 - cos(2 pi j / 48)); taps with |c_j| <= 1e-6 are dropped; tap j feeds phase j mod F with delay
// j div F.  The kept taps in ascending j; returns their count.
constexpr uint32_t TRUE_PEAK_TAPS = 49;
uint32_t true_peak_factor(uint32_t sr);
uint32_t true_peak_filter(uint32_t factor, double coef[TRUE_PEAK_TAPS], uint32_t phase[TRUE_PEAK_TAPS], uint32_t delay[TRUE_PEAK_TAPS]);

// ---- normalisation and clip guarding (dynamics/normalize.rs, limiter.rs, envelope.rs, stats.rs)
// 10f32.powf((target - stat) / 20) in f32 (normalize.rs:29-43); kind: TH_NORM_* (Off: 1); false for an unknown kind
bool normalize_gain(int kind, float target, double global_lufs, float rms_dB, float max_peak_dB, float *gain);
// PerfectLimiter::with_default(sr) (limiter.rs:59-82): false when the attack would be 0 samples (sr < 100)
struct LimiterParams {
    uint32_t attack, hold_length, box_len[3];
    double release_samples;
};
bool limiter_params(uint32_t sr, LimiterParams *out);
// dB_from_amp_default of an f32 (decibel.rs:66-102, amin = 0): 20 log10 x, the logarithm in f64 and rounded once (as the AudioStats are)
float db_from_amp(float x);

// ---- spectrum of a time range (th_tm_get_spectra): the frames whose centre t hop lies in [start_sec, end_sec), as [f0, f1) of
// n_frames: f0 = clamp(ceil(start_sec sr / hop), 0, T), f1 = T for end_sec = +inf, else max(f0, clamp(ceil(end_sec sr / hop), 0, T)),
// in double.  false: start_sec NaN, negative or infinite, end_sec NaN or below start_sec, sr or hop zero.
bool spectrum_frame_range(uint32_t sr, size_t hop, size_t n_frames, double start_sec, double end_sec, size_t *f0, size_t *f1);

// ---- waveform envelope (th_envelope_edges, th_waveform_figure_span; include/thesia_amd.h "Waveform envelope")
// envelope_range: A and B of the definition, in samples; 0, or 1 for an invalid argument (a NaN, a negative or infinite start, an end
// not above the start after clamping, a zero sr, n_samples or n_cols, n_cols above TH_ENVELOPE_MAX_COLS).  envelope_edges: the n_cols + 1
// edges, the same status.  waveform_figure_span: one column of a lane (envelope_core.h lane_span); 0, or 1 for an invalid argument
int envelope_range(uint32_t sr, uint64_t n_samples, double start_sec, double end_sec, uint32_t n_cols, double *A, double *B);
int envelope_edges(uint32_t sr, uint64_t n_samples, double start_sec, double end_sec, uint32_t n_cols, uint64_t *edges);
int waveform_figure_span(const float col[4], const float *left, uint32_t out_h, float amp_lo, float amp_hi, uint32_t thickness, int32_t *y_top,
                         int32_t *y_bot, int *draws);

// ---- PCM / WAV export (th_wav_header): the RIFF header around n_frames frames of n_ch channels; bytes_per_sample 2 or 3 (PCM, 44
// bytes, tag 1) or 4 (float32, 58 bytes: an 18-byte "fmt " with tag 3 and a "fact" chunk).  *pad_len: the zero byte behind an odd
// data size.  Returns 0, 1 for an invalid argument (no channels, no rate), 2 for a file RIFF cannot describe (a size above
// 2^32 - 1, more than 65535 channels, a block above 65535 bytes, a byte rate above 2^32 - 1)
int wav_header(uint32_t bytes_per_sample, uint32_t sr, uint32_t n_ch, uint64_t n_frames, uint8_t out[64], size_t *header_len,
               size_t *pad_len);

// ---- polyphase sinc resampler (th_resample_plan_for; include/thesia_amd.h "Export at a target sample rate").  resample_plan: 0, 1 for a
// zero rate, 2 for a pair beyond TH_RESAMPLE_MAX_TAPS / TH_RESAMPLE_MAX_COEFS.  resample_n_out: ceil(n_in L / M), false when
// n_out M does not fit 64 bits (then no j M of the track overflows).  resample_row: row r of the table, 2K taps, in f64
// and / or rounded to f32.  resample_table: rows [0, L) as L x 2K floats, built on up to 16 threads
int resample_plan(uint32_t sr_in, uint32_t sr_out, th_resample_plan *out);
bool resample_n_out(size_t n_in, const th_resample_plan &p, size_t *n_out);
void resample_row(const th_resample_plan &p, uint32_t r, double *h64, float *c32);
void resample_table(const th_resample_plan &p, float *table);

// ---- band filter of the export (th_band_plan_for; include/thesia_amd.h "Export what a spectrogram box holds").  band_plan_for: 0, 1
// for a bad argument, 2 for a row beyond TH_BAND_MAX_TAPS; a plan with half_taps == 0 is the identity.  band_row: the 2K taps of a plan
// with half_taps > 0, in f64 and / or rounded to f32, with the resampler's sinc and window, built on up to 16 threads.  band_response:
// the magnitude in dB of the f32 row c32 at n frequencies, summed in f64
int band_plan_for(uint32_t sr, uint32_t mode, double f_lo_hz, double f_hi_hz, double trans_hz, th_band_plan *out);
void band_row(uint32_t sr, const th_band_plan &p, double *h64, float *c32);
void band_response(uint32_t sr, const float *c32, uint32_t half_taps, const double *hz, size_t n, double *db);

inline bool is_pow2(size_t n) { return n && !(n & (n - 1)); }
inline unsigned ilog2(size_t n) {
    unsigned l = 0;
    while ((size_t(1) << (l + 1)) <= n) l++;
    return l;
}

}  // namespace th
