// reader_plan.h — what the export and loudness-meter readers of the TrackManager decide on the host, as plain data: the job structs
// their kernels read, plan_export (requests -> pieces) and plan_meters (tracks -> job tables and one memory layout), the bind functions
// that turn offsets into addresses, and the host's part of a meter.  No HIP header: track_manager.hip uploads and launches what these
// functions return, tests/emu/ compiles the same functions with g++ (implementations: reader_plan.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/thesia_amd.h"
#include "host_math.h"  // LoudnessRate

namespace th {

// ---- kernels_loudness.hip: K-weighted chunk energies, per-channel sum of squares and peak, 400 ms block energies
struct LoudJob {           // one channel
    const float *wav;
    double *z;             // n_fchunks x 8: double-double states (4 hi, 4 lo), the chunks' zero-state end states, then their start states
    double *q;             // n_fchunks chunk energies (sum of y^2)
    double *sumsq;         // += sum of x^2 over all samples (zeroed by the caller)
    uint32_t *peak;        // max |x| as float bits (zeroed by the caller)
    uint64_t n;
    uint32_t rate;         // index into the LoudnessRate table
    uint32_t n_chunks;     // chunks that hold samples (the sums)
    uint32_t n_fchunks;    // chunks the 400 ms blocks cover: (n_blocks + 3) n_sub, or 0
    uint32_t aligned16;
};
struct LoudTrackJob {      // one track
    const double *q;       // channel c's chunk energies at q + c n_fchunks
    double *out;           // n_blocks block energies
    uint64_t n_blocks;
    double w[8];           // channel weights (channel c >= 7: w[7])
    uint32_t n_ch, n_sub, n_fchunks, L;
};

// ---- kernels_meter.hip: the true peak of a batch of channels (th_tm_get_loudness_meters): max |y| of the polyphase interpolator
// of host_math.h true_peak_filter, F = 4 or 2, causal from zero history, nothing behind the last sample
constexpr uint32_t TP_RUN = 33;                 // consecutive outputs of one thread (odd: the lanes' LDS reads hit different banks)
constexpr uint32_t TP_THREADS = 256;
constexpr uint32_t TP_CHUNK = TP_RUN * TP_THREADS;  // samples of one workgroup (a multiple of 4)
struct TruePeakJob {       // one channel
    const float *wav;
    uint32_t *peak;        // max |y| as float bits (zeroed by the caller)
    uint64_t n;
    uint32_t n_chunks;     // ceil(n / TP_CHUNK)
    uint32_t aligned16;
};
static_assert(sizeof(TruePeakJob) == 32, "TruePeakJob must have no implicit padding");

// ---- kernels_export.hip: planar f32 channels to interleaved file bytes (16 / 24-bit PCM with optional TPDF dither, or float32)
constexpr uint32_t EXPORT_CHUNK_SAMPLES = 4096;  // samples (frames x channels) of one workgroup, at most
// frames of one chunk: a multiple of 4, so that a chunk starts on a 16-byte boundary of every 16-byte aligned channel.  Chunks lie on
// the ABSOLUTE grid k F .. (k + 1) F of the track: a range that starts or ends inside one gets a partial chunk
constexpr uint32_t export_chunk_frames(uint32_t n_ch) {
    return (EXPORT_CHUNK_SAMPLES / n_ch) & ~3u ? (EXPORT_CHUNK_SAMPLES / n_ch) & ~3u : 4u;
}
struct ExportJob {             // frames [f0, f1) of one request: a whole request, or the part of it that lies in one piece
    const float *const *chan;  // n_ch channel pointers (device memory), each of n samples, 4-byte aligned
    uint8_t *dst;              // where frame f0's first byte goes: ANY byte address
    unsigned long long *cnt;   // [0] += clamped samples, [1] += NaN samples
    uint64_t f0, f1, n;        // f0 <= f1 <= n
    uint32_t n_ch;             // 1 .. TH_EXPORT_MAX_CHANNELS
    uint32_t format, dither, seed;
    uint32_t first_chunk;      // blocks [first_chunk, first_chunk of the next job) of the grid are this job's chunks
    uint32_t pad;              // zero bytes behind frame f1 - 1's last byte (0 .. 15; written by the job's last chunk)
};
static_assert(sizeof(ExportJob) == 72, "ExportJob must have no implicit padding");
// chunks of the absolute grid that [f0, f1) touches
inline uint32_t export_n_chunks(uint64_t f0, uint64_t f1, uint32_t n_ch) {
    const uint64_t F = export_chunk_frames(n_ch);
    return f1 > f0 ? (uint32_t)((f1 - 1) / F - f0 / F + 1) : 0u;
}

// ---- kernels_resample.hip: polyphase sinc resampler, planar f32 channels at the track's rate to planar f32 at the output rate
// (include/thesia_amd.h "Export at a target sample rate"; the summation is resample_core.h).  Outputs j and j + L share a coefficient
// row and their windows lie M samples apart, so a workgroup takes ONE channel, R consecutive outputs (R <= 64 rows, one per lane) and
// P = G Pt "periods" of them, Lp outputs apart (Lp a multiple of L): wave g of G takes periods g Pt .. g Pt + Pt - 1, a thread keeps
// four coefficients in registers across its Pt periods.
constexpr uint32_t RESAMPLE_LANES = 64;     // rows of a tile, at most
constexpr uint32_t RESAMPLE_TAP_BLOCK = 64; // taps staged per step (a multiple of 4)
constexpr uint32_t RESAMPLE_XS_MAX = 5248;  // input samples staged per step, at most (two copies of them, the second shifted by one)
constexpr uint32_t RESAMPLE_MAX_PT = 8;
struct ResampleTiling {
    uint32_t L, M, taps;  // taps = 2K
    uint32_t Lp;          // outputs between two periods: L (L >= 64) or the largest multiple of L that is at most 64
    uint32_t R, S;        // a period of Lp outputs is cut into S sub-tiles of R outputs (the last one may be shorter); R <= 64
    uint32_t G, Pt;       // waves of a workgroup, periods per thread: a tile is P = G Pt periods
    uint32_t span;        // input samples a step stages: the largest offset of a window in the tile + RESAMPLE_TAP_BLOCK
    uint64_t Mp;          // input samples between two periods: M Lp / L
};
inline ResampleTiling resample_tiling(const th_resample_plan &p) {
    ResampleTiling t{};
    t.L = p.L;
    t.M = p.M;
    t.taps = 2 * p.half_taps;
    if (p.L < RESAMPLE_LANES) {  // (L = 1, 2, 6 ...: a row serves several lanes, no lane idles but the 64 mod L last ones)
        t.Lp = p.L * (RESAMPLE_LANES / p.L);
        t.R = t.Lp;
        t.S = 1;
    } else {
        t.Lp = p.L;
        t.S = (p.L + RESAMPLE_LANES - 1) / RESAMPLE_LANES;
        t.R = (p.L + t.S - 1) / t.S;
    }
    t.Mp = (uint64_t)p.M * (t.Lp / p.L);
    const uint64_t lanes = ((uint64_t)(t.R - 1) * p.M) / p.L + 1 + RESAMPLE_TAP_BLOCK;
    static const uint32_t shapes[6][2] = {{4, 8}, {4, 4}, {4, 2}, {4, 1}, {1, 2}, {1, 1}};
    for (const auto &sh : shapes) {
        t.G = sh[0];
        t.Pt = sh[1];
        const uint64_t span = (uint64_t)(t.G * t.Pt - 1) * t.Mp + lanes;
        t.span = (uint32_t)std::min<uint64_t>(span, UINT32_MAX);
        if (span <= RESAMPLE_XS_MAX) break;
    }
    return t;  // ({1, 1} fits every plan: M / L <= 64 under TH_RESAMPLE_MAX_TAPS, so lanes <= 63 x 64 + 65)
}
struct ResampleJob {           // outputs [ja, jb) of every channel of one request
    const float *const *chan;  // n_ch channel pointers (device memory), each of n_in samples
    float *dst;                // output ja of channel 0; channel c's run starts ch_stride floats further per channel
    uint64_t ja, jb;           // ja <= jb <= n_out
    uint64_t n_in;
    uint64_t ch_stride;
    uint32_t n_ch;
    uint32_t n_sb;             // tiles of P Lp outputs that [ja, jb) takes, counted from ja
    uint32_t first_block;      // blocks [first_block, first_block of the next job) of the grid are this job's: n_ch x n_sb x S
    uint32_t pad;
};
static_assert(sizeof(ResampleJob) == 64, "ResampleJob must have no implicit padding");
inline uint64_t resample_n_sb(uint64_t ja, uint64_t jb, const ResampleTiling &t) {
    const uint64_t per = (uint64_t)t.G * t.Pt * t.Lp;
    return (jb - ja + per - 1) / per;
}

// ---- kernels_band.hip: one FIR row for every output (the band filter of th_tm_export_pcm_band; the summation is resample_core.h).
// A workgroup takes ONE channel and a tile of BAND_TILE consecutive outputs, a thread BAND_R consecutive ones of them; the 2K taps are
// walked in blocks of BAND_TAP_BLOCK, and per block the tile's input span (tile + block - 1 samples) is staged once
constexpr uint32_t BAND_THREADS = 256;
constexpr uint32_t BAND_R = 8;                         // consecutive outputs of one thread (4 partial sums each)
constexpr uint32_t BAND_TILE = BAND_THREADS * BAND_R;  // outputs of one workgroup
constexpr uint32_t BAND_TAP_BLOCK = 64;                // taps per step (a multiple of 4)
struct BandTiling {
    uint32_t taps;       // 2K
    uint32_t tile, R;    // outputs of a workgroup and of a thread
    uint32_t tap_block;
};
static_assert(sizeof(BandTiling) == 16, "BandTiling must have no implicit padding");
inline BandTiling band_tiling(const th_band_plan &p) { return BandTiling{2 * p.half_taps, BAND_TILE, BAND_R, BAND_TAP_BLOCK}; }
struct BandJob {               // outputs [ja, jb) of every channel of one request
    const float *const *chan;  // n_ch channel pointers (device memory), each of n_in samples
    float *dst;                // output ja of channel 0; channel c's run starts ch_stride floats further per channel
    uint64_t ja, jb;           // ja <= jb <= n_in
    uint64_t n_in;
    uint64_t ch_stride;
    uint32_t n_ch;
    uint32_t n_tiles;          // tiles of BAND_TILE outputs that [ja, jb) takes, counted from ja
    uint32_t first_block;      // blocks [first_block, first_block of the next job) of the grid are this job's: n_ch x n_tiles
    uint32_t pad;
};
static_assert(sizeof(BandJob) == 64, "BandJob must have no implicit padding");
inline uint64_t band_n_tiles(uint64_t ja, uint64_t jb) { return (jb - ja + BAND_TILE - 1) / BAND_TILE; }

// ---- the export reader's plan (th_tm_export_pcm / _wav / _at / _band).  The requests are cut into PIECES of at most TH_EXPORT_PIECE_BYTES
// staged bytes, at frame boundaries; a piece is one launch of the export kernel into one of two staging buffers (piece p: buffer
// p & 1), in front of it one launch of the resampler for the piece's resampled jobs and one of the band filter for its filtered ones
// (both write the piece's planar scratch), and one copy per RUN of contiguous output bytes.
// A job's bytes sit in staging at the same address modulo 16 as in the caller's image, so a run is one copy.
constexpr size_t EXPORT_STAGE_MAX = (size_t)TH_EXPORT_PIECE_BYTES + 64;  // a staging buffer: a piece and its alignment slack
// the planar scratch of a piece: frames x channels x 4 bytes, and per job up to 7 frames more (the hull on the grid of 4 frames and
// the channel pitch), so 2 x TH_EXPORT_PIECE_BYTES (16-bit output) + 64 KiB bounds it; a piece is closed before it would need more
constexpr size_t RESAMPLE_SCRATCH_MAX = 2 * (size_t)TH_EXPORT_PIECE_BYTES + (64u << 10);

struct ExportPlanRequest {     // what the check found of one request (export_request_info, export_layout)
    uint32_t n_ch;             // 1 .. TH_EXPORT_MAX_CHANNELS
    uint32_t sr_in, sr_out;    // the track's rate and the one the request comes out at; resampled when they differ
    uint64_t n_in;             // samples of a channel of the track
    th_resample_plan plan;     // resampled requests: the rate pair's plan and the track's length at sr_out
    uint64_t n_out;
    th_band_plan band;         // filtered requests (half_taps != 0; never resampled as well): the filter; all zero: none
    uint32_t format, dither, seed;
    uint64_t s0, s1;           // frames [s0, s1) at sr_out
    uint64_t offset;           // of frame s0's first byte in the caller's buffer
    uint32_t pad;              // zero bytes behind frame s1 - 1
};
struct ExportPlace {           // where one export job lives
    size_t req;
    size_t stage_at;           // byte offset in the piece's staging buffer
    // resampled and filtered jobs: the job's channel runs in the scratch (float offset; channel c's starts c stride further), its own channel
    // pointers in the pointer table, and the hull on the grid of 4 frames that the resampler makes: [hull0, hull0 + stride) holds
    // the job's frames and the 16-byte loads around them
    size_t scratch_at, ptr_at;
    uint64_t hull0, stride;
    bool resampled;
    bool filtered = false;
};
struct ExportRun {             // one copy: bytes from staging offset stage_at to the caller's out + out_at
    size_t stage_at;
    uint64_t out_at;
    size_t bytes;
};
struct ExportPiece {
    size_t job0 = 0, job1 = 0;    // export jobs [job0, job1)
    uint32_t n_chunks = 0;        // the export launch's grid
    size_t stage_bytes = 0;
    std::vector<ExportRun> runs;
    // the resampler's launch in front of the export's: every resampled request of a piece has the piece's rate pair
    size_t rjob0 = 0, rjob1 = 0;
    uint32_t n_rblocks = 0, sr_in = 0, sr_out = 0;
    size_t scratch_floats = 0;
    th_resample_plan plan{};
    // the band filter's launch, also in front of the export's: every filtered request of a piece has the piece's filter
    size_t bjob0 = 0, bjob1 = 0;
    uint32_t n_bblocks = 0, band_sr = 0;
    th_band_plan band{};
};
inline bool same_band(const th_band_plan &a, const th_band_plan &b) {
    return a.half_taps == b.half_taps && a.mode == b.mode && a.f_lo_hz == b.f_lo_hz && a.f_hi_hz == b.f_hi_hz;
}
struct ExportPlan {
    int err = TH_OK;              // (nothing else below is valid then)
    std::string err_text;
    std::vector<ExportJob> jobs;  // pointer fields unset until bind_export
    std::vector<ResampleJob> rjobs;
    std::vector<BandJob> bjobs;
    // places[j]: of jobs[j]; the resampled ones among a piece's jobs are its rjobs, the filtered ones its bjobs, in order
    std::vector<ExportPlace> places;
    std::vector<ExportPiece> pieces;
    // the pointer table: request i's n_ch channel pointers at ptr0[i], a resampled job's at its ptr_at
    std::vector<size_t> ptr0;
    std::vector<uint32_t> req_ch;  // request i's channel count
    size_t n_ptrs = 0;
    // the uploaded table: jobs, then rjobs at o_rjobs, bjobs at o_bjobs, then the pointer table at o_ptrs
    size_t o_rjobs = 0, o_bjobs = 0, o_ptrs = 0, tab_bytes = 0;
    size_t stage_need[2] = {0, 0}, scratch_need = 0;  // the largest piece of either parity (bytes), the largest scratch (floats)
};
ExportPlan plan_export(const ExportPlanRequest *reqs, size_t n);
struct ExportBases {
    uint8_t *stage[2];
    float *scratch;
    unsigned char *tab;        // where the uploaded table will lie
    unsigned long long *cnt;   // two counters per request
};
// Fills the pointer fields of p's jobs and returns the table to upload.  chan: every request's n_ch channel pointers, in request
// order.  A resampled or filtered export job reads channel c at (its run in the scratch) - hull0: the export kernel indexes a channel by the
// absolute output frame, and run and hull both start on 16-byte boundaries, so the biased pointer is 16-byte aligned as well
std::vector<unsigned char> bind_export(ExportPlan &p, const ExportBases &b, const float *const *chan);

// ---- the loudness meters' plan (th_tm_get_loudness_meters).  Per channel one LoudJob (passes A - C of kernels_loudness.hip) and, at
// F > 1, one TruePeakJob; per track two LoudTrackJobs (pass D over 4 and over 30 segments, writing the energies where the series go)
struct MeterPlanTrack {
    size_t id;                 // (for the message)
    uint32_t sr, n_ch, oversampling;
    uint64_t n_samples, n_momentary, n_short_term;
};
struct MeterPlan {
    int err = TH_OK;
    std::string err_text;
    std::vector<MeterPlanTrack> tracks;
    std::vector<bool> rate_ok;             // per track: loudness_rate_ok (else the peaks only, over chunks of a 48 kHz geometry)
    std::vector<const LoudnessRate *> rates;
    std::vector<LoudJob> jobs;             // every channel, track by track
    std::vector<LoudTrackJob> tj_m, tj_s;  // per track: the momentary and the short-term blocks
    std::vector<TruePeakJob> tp[2];        // F = 4, F = 2
    std::vector<size_t> tp_ch[2];          // the channel (index into jobs) of every true-peak job
    std::vector<size_t> ch0, e0;           // per track: its first channel, its first energy (the momentary ones, then the short-term ones)
    size_t n_ch = 0, n_energies = 0, n_states = 0;
    // launch bounds
    uint32_t max_chunks = 0, max_fchunks = 0, lds_floats = 4, tp_chunks[2] = {0, 0};
    uint64_t max_m = 0, max_s = 0;
    // device memory, byte offsets: results [energies at 0][sums of squares: n_ch f64][pass A's peaks: n_ch u32][true peaks: n_ch u32]
    // | states (64 bytes per chunk) | chunk energies
    size_t o_sums = 0, o_pka = 0, o_pkt = 0, res_bytes = 0, o_z = 0, o_q = 0, mem_bytes = 0;
    // the uploaded table, byte offsets: LoudJobs at 0, the LoudnessRates, tj_m, tj_s, tp[0], tp[1]
    size_t t_rates = 0, t_m = 0, t_s = 0, t_tp4 = 0, t_tp2 = 0, tab_bytes = 0;
};
// the limits of one launch's grid: NULL, or the message (TH_ERR_INVALID_ARG)
const char *meter_limits_text(size_t n_tracks, size_t n_channels);
MeterPlan plan_meters(const MeterPlanTrack *tracks, size_t n);
// Fills the pointer fields (mem: the device memory's base; wav: every channel's samples, track by track) and returns the table to upload
std::vector<unsigned char> bind_meters(MeterPlan &p, unsigned char *mem, const float *const *wav);
// The host's part of every track's meter from the res_bytes that came back: LUFS, maxima, the loudness range, the peak and its channel.
// Keeps ms[i]'s oversampling, counts, offsets and revision; with series, writes track i's LUFS to series + ms[i]->momentary_offset
// (the short-term values follow the momentary ones)
void meter_results(const unsigned char *res, const MeterPlan &p, th_loudness_meter *const *ms, double *series);

}  // namespace th
