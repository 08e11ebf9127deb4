// align_plan.h — the host side of the alignment reader (include/thesia_amd.h "Align two tracks") as plain data, no HIP: the tile shape
// and the job of kernels_align.hip, the plan of one request (align_plan_for: the one place where numbers are made from seconds), the cut
// of a request into pieces, the host's step on the read-back curve, and the host restatements th_xcorr_f64 / th_align_f64 stand on.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/thesia_amd.h"
#include "align_core.h"

namespace th {

// ---- kernels_align.hip.  A workgroup of ALIGN_THREADS threads takes a tile of ALIGN_TILE consecutive lags and ONE group of the
// reference; a thread takes ALIGN_R consecutive lags of the tile (4 partial sums each).  The reference is walked in steps of
// ALIGN_STEP samples, and per step the tile's probe span (tile + step - 1 samples) is staged once
constexpr uint32_t ALIGN_THREADS = 128;
constexpr uint32_t ALIGN_R = 8;
constexpr uint32_t ALIGN_TILE = ALIGN_THREADS * ALIGN_R;
constexpr uint32_t ALIGN_STEP = 64;
static_assert(ALIGN_BLOCK % ALIGN_STEP == 0 && ALIGN_STEP % 4 == 0, "a block is whole steps; a step starts at k = 0 mod 4");
// the energy kernel: a workgroup takes one group, thread 4 j + q partial sum q of the group's block j
constexpr uint32_t ALIGN_ENERGY_THREADS = 4 * ALIGN_GROUP_BLOCKS;

// lags [0, n_lags) of one piece: r_i = sum over k < N of a[k] b[first + i + k].  Workgroup (tile t, group g) writes the group's value
// of lag i to scratch[g n_lags + i]
struct AlignJob {
    const float *a;   // the reference's range: N samples
    const float *b;   // the probe: a track of n_b samples, +0 outside
    double *scratch;  // n_groups x n_lags
    uint64_t N, n_b;
    int64_t first;    // s0 + the piece's first lag
    uint32_t n_lags, n_tiles, n_groups, reserved;
};
static_assert(sizeof(AlignJob) == 64, "AlignJob must have no implicit padding");
inline uint32_t align_n_tiles(uint64_t n_lags) { return (uint32_t)((n_lags + ALIGN_TILE - 1) / ALIGN_TILE); }

// ---- one request's plan.  0; 1: TH_ERR_INVALID_ARG; 2: TH_ERR_UNSUPPORTED
int align_plan_for(uint32_t sr_ref, size_t n_ref, uint32_t sr, size_t n, const th_align_request &req, th_align_plan *plan);

// ---- the cut of one request: pieces of at most TH_ALIGN_PIECE_LAGS lags, in order.  lag0: the piece's first lag as an index into
// [0, n_lags) (the lag itself is lag0 - D)
struct AlignPiece {
    uint64_t lag0;
    uint32_t n_lags, n_tiles, n_groups, n_blocks;  // n_blocks = n_tiles x n_groups: the launch's grid
};
struct AlignPieces {
    std::vector<AlignPiece> pieces;
    uint64_t scratch_doubles = 0;  // the largest piece's n_groups x n_lags
    uint64_t rec_doubles = 0;      // the largest piece's n_lags
};
AlignPieces plan_align(uint64_t N, uint64_t n_lags);

// ---- the host's step
struct AlignPeak {
    uint32_t status;  // 0 valid, 1 invalid
    uint64_t index;   // of l* in r (l* = index - D)
    double delta, polarity;
};
AlignPeak align_peak(const double *r, uint64_t n_lags, uint32_t flags, double e_ref);
// the ten doubles of a request from its peak and the two energies (e_probe is not looked at when the peak is invalid)
void align_summary(const AlignPeak &pk, const double *r, uint32_t D, double e_ref, double e_probe, double out[TH_ALIGN_SUMMARY_DOUBLES]);

// ---- the host restatements, in the contract's order (align_core.h)
void xcorr_f64(const float *a, uint64_t N, const float *b, uint64_t n_b, int64_t first, uint64_t n_lags, double *r);
double align_energy_f64(const float *x, uint64_t n, int64_t first, uint64_t N);
// a planned request from two host channels: pl.length doubles
void align_f64(const float *ref, const float *probe, uint64_t n_b, const th_align_plan &pl, double *out);

}  // namespace th
