// figure_plan.h — what the figure reader of the TrackManager (th_tm_render_figures) decides on the host, as plain data: the checks of
// a request, the tap tables (one per distinct axis), the job tables of the two kernels of kernels_figure.hip, the pieces a call is cut
// into and the memory layout of a piece, and bind_figures, which turns offsets into addresses.  A planner copies the image pointer of
// a request and never reads through it.  No HIP header: track_manager.hip uploads, launches and copies what these functions return,
// and a stand-alone program compiles the same functions with g++ (implementations: figure_plan.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/thesia_amd.h"
#include "host_math.h"  // LodAxisHost

namespace th {

// ---- kernels_figure.hip
// The horizontal pass: a block takes FIG_ROWS source rows (a lane owns a row) and a run of `oc` output columns; it stages the column
// span of the run in LDS, [column][row] with FIG_COL_PITCH u16 per column, in steps of at most FIG_SPAN columns.  A wave walks the taps
// of FIG_GROUP consecutive outputs at once; a pass of the block is one group per wave (FIG_PASS outputs).
constexpr uint32_t FIG_THREADS = 256;
constexpr uint32_t FIG_ROWS = 64;
constexpr uint32_t FIG_SPAN = 368;       // columns of one staged step: a multiple of 4
constexpr uint32_t FIG_COL_PITCH = 65;   // u16 per staged column: odd, so that the 8-byte loads' four LDS writes spread over the banks
constexpr uint32_t FIG_GROUP = 4;
constexpr uint32_t FIG_PASS = FIG_GROUP * (FIG_THREADS / 64);
constexpr uint32_t FIG_OC_MAX = 128;     // output columns of a block, at most: a multiple of FIG_PASS
constexpr uint32_t FIG_OUT_PITCH = FIG_OC_MAX + 2;  // u16 per row of the block's results in LDS (65 dwords: a row per bank)
static_assert(FIG_SPAN % 4 == 0 && FIG_OC_MAX % FIG_PASS == 0, "figure tile shape");
// 47 840 + 16 640 bytes: two blocks stay resident in the 160 KiB of a CU
static_assert((FIG_SPAN * FIG_COL_PITCH + FIG_ROWS * FIG_OUT_PITCH) * sizeof(uint16_t) <= 64 * 1024, "figure LDS");

struct FigAxis {             // device pointers into the uploaded table
    const int32_t *start;    // [n_out] first source index, clipped to the image
    const int32_t *count;    // [n_out] taps
    const double *w;         // [n_out][max_taps] normalised weights
    uint32_t n_out, max_taps;
};
static_assert(sizeof(FigAxis) == 32, "FigAxis must have no implicit padding");
struct FigHJob {             // one part: source rows [y_lo, y_lo + n_rows) of one image to n_out columns each
    const uint16_t *src;     // the image's row 0
    uint16_t *tmp;           // row y_lo's outputs; row r's are tmp_pitch elements further per row
    FigAxis ax;
    uint32_t src_pitch, tmp_pitch;
    uint32_t y_lo, n_rows;
    uint32_t oc;             // output columns of a block: a multiple of FIG_PASS, at most FIG_OC_MAX
    uint32_t n_cblocks;      // ceil(n_out / oc); the job's blocks are n_cblocks x ceil(n_rows / FIG_ROWS), the column block fastest
    uint32_t first_block;    // blocks [first_block, first_block of the next job) of the grid are this job's
    uint32_t pad;
};
static_assert(sizeof(FigHJob) == 80, "FigHJob must have no implicit padding");
struct FigVJob {             // one part: output rows [j0, j0 + n_rows) of one request
    const uint16_t *tmp;     // the part's intermediate: source row y_lo's outputs
    uint8_t *dst;            // output row j0's first byte in staging: 64-byte aligned
    FigAxis ay;
    uint32_t tmp_pitch, y_lo;
    uint32_t out_w, out_h;
    uint32_t j0, n_rows;
    uint32_t kind;           // TH_FIGURE_*
    uint32_t first_block;    // a block is FIG_THREADS groups of 16 output bytes
};
static_assert(sizeof(FigVJob) == 80, "FigVJob must have no implicit padding");
inline uint32_t figure_bytes_per_pixel(uint32_t kind) { return kind == TH_FIGURE_GREY16 ? 2u : 4u; }

// ---- the plan
struct FigurePlanRequest {   // one request, checked against the manager (the image exists) and laid out (offset)
    const uint16_t *img;     // device memory: row 0 of img_h rows of img_w pixels, img_pitch elements apart
    uint32_t img_w, img_h, img_pitch;
    uint32_t kind, out_w, out_h;
    double left, top, width, height;
    uint64_t offset;         // of the record in the caller's buffer
};
struct FigureStatus {
    int err = TH_OK;         // (nothing else is valid otherwise)
    std::string err_text;
};
// The check of ONE request (i: its index, for the message): kind, size, box, the 256 MB rule of plan_lod_tile, and what the kernels
// ask of the image (rows that start on 8-byte boundaries).  A box is inside the image when left, top >= 0 and left + width <=
// img_w (1 + 1e-12), likewise for the rows: a box that th_figure_box clamped may exceed the edge by a rounding.
FigureStatus check_figure(const FigurePlanRequest &r, size_t i);

struct FigureAxisTable {     // one distinct axis
    uint32_t n_in, n_out;
    double origin, extent;
    uint32_t max_taps;
    uint32_t oc;             // the horizontal kernel's run for this axis (figure_pick_oc)
    size_t at;               // byte offset of [start][count][w] in the table: a multiple of 8
    std::vector<int32_t> start, count;
};
struct FigurePart {          // rows [j0, j1) of request req: one job of each kernel, one copy
    size_t req;
    uint32_t j0, j1;
    uint32_t y_lo, y_hi;     // the source rows the band's filter windows span
    size_t tmp_at;           // u16 offset of the intermediate in the piece's scratch: a multiple of 8
    size_t stage_at;         // byte offset in the piece's staging buffer: a multiple of 64
    uint64_t out_at;         // byte offset in the caller's buffer
    size_t bytes;
};
struct FigurePiece {
    size_t part0 = 0, part1 = 0;      // parts (= jobs of either table) [part0, part1)
    uint32_t n_hblocks = 0, n_vblocks = 0;
    size_t stage_bytes = 0, tmp_elems = 0;
};
struct FigurePlan : FigureStatus {
    std::vector<FigureAxisTable> axes;
    std::vector<size_t> ax_of, ay_of;  // per request: its axes
    std::vector<FigurePart> parts;
    std::vector<FigurePiece> pieces;
    std::vector<FigHJob> hjobs;        // hjobs[k], vjobs[k]: of parts[k]; pointer fields unset until bind_figures
    std::vector<FigVJob> vjobs;
    std::vector<unsigned char> axis_blob;  // every axis's [start][count][w]
    // the uploaded table: the axis blob at 0, the FigHJobs at o_hjobs, the FigVJobs at o_vjobs
    size_t o_hjobs = 0, o_vjobs = 0, tab_bytes = 0;
    size_t stage_need[2] = {0, 0}, tmp_need = 0;  // the largest piece of either parity (bytes), the largest intermediate (u16 elements)
};
// The run of output columns a block of the horizontal kernel takes on this axis: the largest of 128, 64, 32, 16 whose every run's
// column span (from the 4-aligned start of its first window to the end of its last) fits FIG_SPAN, else 16 (the stepped walk)
uint32_t figure_pick_oc(const int32_t *start, const int32_t *count, uint32_t n_out);
FigurePlan plan_figures(const FigurePlanRequest *reqs, size_t n);
struct FigureBases {
    uint8_t *stage[2];
    uint16_t *tmp;
    unsigned char *tab;      // where the uploaded table will lie
};
// Fills the pointer fields of p's jobs and returns the table to upload
std::vector<unsigned char> bind_figures(FigurePlan &p, const FigureBases &b, const FigurePlanRequest *reqs);

// th_figure_box: 0, or 1 for an invalid argument
int figure_box(double start_sec, double end_sec, double hz_min, double hz_max, uint32_t sr, size_t n_samples, size_t img_w, size_t spec_h,
               size_t img_h, int freq_scale, double box[4]);

}  // namespace th
