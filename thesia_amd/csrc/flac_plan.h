// flac_plan.h — the host side of the FLAC export (include/thesia_amd.h "FLAC export") as plain data, no HIP: the job of
// kernels_flac.hip, the cut of a call into pieces of whole blocks, and the addresses of a piece's jobs.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/thesia_amd.h"

namespace th {

// what the scan kernel leaves per job: the job's frames in bytes, and the smallest and the largest of them
struct FlacJobResult {
    unsigned long long bytes;
    uint32_t min_frame, max_frame;
};
static_assert(sizeof(FlacJobResult) == 16, "FlacJobResult must have no implicit padding");

// ---- kernels_flac.hip.  A job is blocks [b0, b0 + nb) of one request: the whole request, or the part of it that lies in one piece.
// Block b holds samples s0 + 4096 b .. of the range [s0, s1) and is frame b of the stream.  The subframe kernel runs one workgroup per
// unit (block-major: unit = block x units per block + coded channel), the scan kernel one per job, the frame kernel one per block.
// A block has n_ch units, one per channel; with TH_FLAC_STEREO a 2-channel block has four, L R M S, of which the frame joins two.
struct FlacJob {
    const float *const *chan;  // n_ch planar f32 channels, indexed by the track's ABSOLUTE sample
    uint32_t *slots;           // the job's units: slot_words words each (the subframe's bits, big-endian in the word)
    uint32_t *bits;            // the job's units: each subframe's length in bits
    uint32_t *foff;            // the job's frames: each frame's first byte, from dst
    uint8_t *dst;              // the job's frames, dense, at any byte address
    unsigned long long *cnt;   // the request's n_clamped, n_nan
    FlacJobResult *res;
    uint64_t s0, s1;
    uint64_t b0;
    uint32_t nb;
    uint32_t first_unit, first_block;  // the job's first workgroup in the subframe / frame kernel's grid
    uint32_t n_ch, format, dither, seed, sr;
    uint32_t slot_words;
    uint32_t flags;            // TH_FLAC_LPC | TH_FLAC_STEREO (0: th_tm_export_flac's stream)
    uint32_t pad_[2];
};
static_assert(sizeof(FlacJob) == 128, "FlacJob must have no implicit padding");

// ---- the cut of a call.  A request that was checked, and where its file image goes
struct FlacPlanRequest {
    uint32_t n_ch, format, dither, seed, sr;
    uint64_t s0, s1;
    uint64_t offset;  // into out
    uint32_t flags;   // of the call (the _ex entries)
};
struct FlacRun {       // a job before it has addresses
    size_t req;
    uint64_t b0;
    uint32_t nb;
    uint32_t first_unit, first_block;
    uint32_t slot_words;
    uint64_t slot_at;   // words into the slot scratch
    uint64_t stage_at;  // bytes into the piece's staging buffer
    uint64_t bound;     // bytes of staging the run may fill
};
struct FlacPiece {
    size_t run0 = 0, run1 = 0;
    uint32_t n_units = 0, n_blocks = 0;
    uint64_t bound = 0, slot_words = 0;
};
constexpr uint32_t FLAC_PIECE_MAX_UNITS = 1u << 16;  // bounds the two tables (bits, foff) of a piece
struct FlacPlan {
    int err = 0;
    std::string err_text;
    std::vector<FlacRun> runs;
    std::vector<FlacPiece> pieces;
    std::vector<FlacJob> jobs;  // jobs[k]: of runs[k]
    std::vector<size_t> chan0;  // per request: its first channel pointer in the caller's flat list
    size_t o_ptrs = 0, tab_bytes = 0;  // the table: the jobs, then the channel pointers
    uint64_t stage_need[2] = {0, 0};   // bytes, per staging buffer
    uint64_t slot_need = 0;            // words
    uint32_t unit_need = 0, block_need = 0;
};
// piece_bytes: TH_EXPORT_PIECE_BYTES in the product (a test may cut smaller)
FlacPlan plan_flac(const FlacPlanRequest *reqs, size_t n, uint64_t piece_bytes);
struct FlacBases {
    uint8_t *stage[2];
    uint32_t *slots, *bits, *foff;
    FlacJobResult *res;       // one per run of the call
    unsigned char *tab;       // the device address of the table
    unsigned long long *cnt;  // two per request
};
// the addresses into the jobs, and the table's bytes.  chan: every request's channel pointers, flat, in request order
std::vector<unsigned char> bind_flac(FlacPlan &p, const FlacBases &b, const FlacPlanRequest *reqs, size_t n, const float *const *chan);

}  // namespace th
