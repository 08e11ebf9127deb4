// envelope_plan.h — what the envelope and waveform-lane readers of the TrackManager (th_tm_get_envelopes,
// th_tm_render_waveform_figures) decide on the host, as plain data: the checks of a request, the edge tables, the job tables of the
// kernels of kernels_envelope.hip, the pieces a call is cut into and the memory layout of a piece, and the bind functions, which turn
// offsets into addresses.  A planner copies the channel pointer of a request and never reads through it.  No HIP header:
// track_manager.hip uploads, launches and copies what these functions return, and a stand-alone program compiles the same functions
// with g++ (implementations: envelope_plan.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/thesia_amd.h"

namespace th {

// ---- kernels_envelope.hip
// A CHUNK is ENV_CHUNK samples on the absolute grid of the channel (chunk k = samples [k ENV_CHUNK, (k + 1) ENV_CHUNK)), so that the
// 16-byte loads of a chunk are aligned wherever a request starts.  A request whose columns hold ENV_DENSE_MIN samples or more on
// average is DENSE: one wave reduces the part of a chunk the request covers, column by column; a column inside one chunk is
// finished there, the at most two columns of a chunk that reach beyond it leave a partial (slot 2 k' for the chunk's first column, 2 k'
// + 1 for its last; k' counts from the request's first chunk), and the column kernel adds a column's partials in ascending chunk
// order.  Every other request is SPARSE: the column kernel's thread walks its column's samples in ascending order.
constexpr uint32_t ENV_CHUNK = 4096;
constexpr uint32_t ENV_THREADS = 256;
constexpr uint32_t ENV_WAVES = ENV_THREADS / 64;  // chunks of a block of the reduction
constexpr uint32_t ENV_DENSE_MIN = 64;
static_assert(ENV_CHUNK % 4 == 0, "a chunk is whole 16-byte quads");

struct EnvPartial {          // of one column's samples inside one chunk
    double sum, sumsq;
    float mn, mx;
};
static_assert(sizeof(EnvPartial) == 24, "EnvPartial must have no implicit padding");
struct EnvJob {              // one request
    const float *x;          // sample 0 of the channel: 16-byte aligned
    const uint64_t *edges;   // [W + 1], never decreasing, edges[W] <= the channel's length
    float *out;              // [W][4] (min, max, mean, rms): 16-byte aligned
    EnvPartial *part;        // dense: 2 n_chunks slots
    uint64_t k0;             // dense: the chunk that holds sample edges[0]
    uint64_t e0, eW;         // edges[0], edges[W]: what every wave needs before its first load of a sample
    uint32_t W;
    uint32_t n_chunks;       // dense: chunks k0 .. k0 + n_chunks - 1 hold [edges[0], edges[W]); 0: a sparse request
    uint32_t first_unit;     // the reduction: chunks [first_unit, first_unit + n_chunks) of the launch are this job's
    uint32_t first_cblock;   // the column kernel: a block is ENV_THREADS columns
};
static_assert(sizeof(EnvJob) == 72, "EnvJob must have no implicit padding");
struct LaneSpanJob {         // one lane request: its columns' spans from its envelope
    const float *env;        // [W][4]
    int32_t *span;           // [W][2] (y_top, y_bot) in 1/256 pixel; (0, 0): the column draws nothing
    uint32_t W, out_h;
    float amp_lo, amp_hi;
    uint32_t thickness;
    uint32_t first_block;    // a block is ENV_THREADS columns
};
static_assert(sizeof(LaneSpanJob) == 40, "LaneSpanJob must have no implicit padding");
struct LaneRasterJob {       // one part: output rows [j0, j0 + n_rows) of one request
    const int32_t *span;
    uint8_t *dst;            // output row j0's first byte in staging: 64-byte aligned
    uint32_t out_w, j0, n_rows;
    uint32_t fill, background;  // RGBA, the R byte lowest
    uint32_t first_block;    // a block is ENV_THREADS groups of 16 output bytes
};
static_assert(sizeof(LaneRasterJob) == 40, "LaneRasterJob must have no implicit padding");

// ---- the envelope plan
struct EnvelopePlanRequest {  // one request, checked against the manager (the channel exists) and laid out (offset)
    const float *x;           // device memory: the channel's n samples
    uint64_t n;
    uint32_t sr, n_cols;
    double start_sec, end_sec;
    uint64_t offset;          // of the record in the caller's buffer: floats (envelopes) or bytes (lanes)
};
struct EnvelopeStatus {
    int err = TH_OK;          // (nothing else is valid otherwise)
    std::string err_text;
};
// The check of ONE request (i: its index, for the message): the arguments of th_envelope_edges and what the kernels ask of the
// channel (16-byte aligned, below 2^53 samples).  *e0, *eW: edges[0] and edges[n_cols]
EnvelopeStatus check_envelope(const EnvelopePlanRequest &r, size_t i, uint64_t *e0, uint64_t *eW);

struct EnvelopePiece {        // whole requests [req0, req1)
    size_t req0 = 0, req1 = 0;
    uint32_t n_units = 0, n_cblocks = 0;
    size_t out_floats = 0, part_elems = 0;
};
struct EnvelopePlan : EnvelopeStatus {
    std::vector<uint64_t> edges;       // every request's table, back to back
    std::vector<size_t> edge_at;       // per request: its table's first element
    std::vector<EnvJob> jobs;          // per request; pointer fields unset until bind_envelopes
    std::vector<size_t> out_at;        // per request: its first float in the piece's result area (a multiple of 4)
    std::vector<size_t> part_at;       // per request: its first slot in the piece's partials
    std::vector<EnvelopePiece> pieces;
    // the uploaded table: the edges at 0, the EnvJobs at o_jobs
    size_t o_jobs = 0, tab_bytes = 0;
    size_t out_need = 0, part_need = 0;  // the largest piece: floats, slots
};
// Pieces of whole requests: at most piece_bytes of results (one request is at most 1 MiB: TH_ENVELOPE_MAX_COLS columns) and at most
// TH_ENVELOPE_PART_BYTES of partials, or what ONE request needs where that alone is more (48 bytes per chunk of 16 KiB it reads)
EnvelopePlan plan_envelopes(const EnvelopePlanRequest *reqs, size_t n, size_t piece_bytes = TH_ENVELOPE_PIECE_BYTES);
struct EnvelopeBases {
    float *out;
    EnvPartial *part;
    unsigned char *tab;       // where the uploaded table will lie
};
// Fills the pointer fields of p's jobs and writes the table to upload into tab[0, p.tab_bytes)
void bind_envelopes(EnvelopePlan &p, const EnvelopeBases &b, const EnvelopePlanRequest *reqs, unsigned char *tab);

// ---- the lane plan
struct LanePlanRequest : EnvelopePlanRequest {  // n_cols = out_w
    uint32_t out_h;
    float amp_lo, amp_hi;
    uint32_t thickness;
    uint8_t fill[4], background[4];
};
EnvelopeStatus check_lane(const LanePlanRequest &r, size_t i, uint64_t *e0, uint64_t *eW);
struct LanePart {             // rows [j0, j1) of request req: one raster job, one copy
    size_t req;
    uint32_t j0, j1;
    size_t stage_at;          // byte offset in the piece's staging buffer: a multiple of 64
    uint64_t out_at;          // byte offset in the caller's buffer
    size_t bytes;
};
struct LanePiece {
    size_t part0 = 0, part1 = 0;   // parts (= raster jobs) [part0, part1)
    uint32_t n_blocks = 0;
    size_t stage_bytes = 0;
    size_t group = 0;              // the envelope piece its requests belong to
    bool first_of_group = false;   // that piece's envelopes and spans are computed in front of this piece
};
struct LanePlan : EnvelopeStatus {
    EnvelopePlan env;                  // its pieces are the GROUPS: the envelopes that are resident at once
    std::vector<LaneSpanJob> sjobs;    // per request
    std::vector<uint32_t> group_sblocks;  // per group: the blocks of its span launch
    std::vector<LanePart> parts;
    std::vector<LaneRasterJob> rjobs;  // rjobs[k]: of parts[k]
    std::vector<LanePiece> pieces;
    // the uploaded table: the envelope plan's table at 0, the LaneSpanJobs at o_sjobs, the LaneRasterJobs at o_rjobs
    size_t o_sjobs = 0, o_rjobs = 0, tab_bytes = 0;
    size_t stage_need[2] = {0, 0};     // the largest piece of either parity, bytes
    size_t span_need = 0;              // int32 elements: half the envelope floats of the largest group
};
// Groups of whole requests (plan_envelopes); inside a group, pieces of bands of whole output rows, at most TH_FIGURE_PIECE_BYTES each
LanePlan plan_lanes(const LanePlanRequest *reqs, size_t n);
struct LaneBases {
    EnvelopeBases env;
    int32_t *span;
    uint8_t *stage[2];
};
void bind_lanes(LanePlan &p, const LaneBases &b, const LanePlanRequest *reqs, unsigned char *tab);

}  // namespace th
