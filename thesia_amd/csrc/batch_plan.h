// batch_plan.h — what the context-level batch entries of the image, raster and waveform stages decide on the host, as plain data: the
// job structs their kernels read, the constants the jobs are cut with, and one planner per entry (descriptors -> checks, job table,
// block -> job table, launch bounds).  A planner copies and checks the pointers in a descriptor and never reads through them (the one
// HOST array, th_img_tiles_desc.tiles, is read).  No HIP header: api.hip uploads and launches what these functions return, tests/emu/
// compiles the same functions with g++ (implementations: batch_plan.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/thesia_amd.h"
#include "host_math.h"  // TileGeom, LodAxisHost

namespace th {

// ---- kernels_image.hip
struct ImgJob {  // device-visible copy of th_img_desc
    const float *spec;
    uint16_t *img;
    uint32_t n_frames, height, i_start, i_end;
    uint32_t spec_pitch, img_pitch;  // elements per row (>= height / n_frames)
    uint32_t first_tile, n_tiles;    // this job's block range in the launch
};
static_assert(sizeof(ImgJob) == 48, "ImgJob must have no implicit padding");
constexpr uint32_t IMG_TILE_T = 64;   // frames per quantise/transpose tile
constexpr uint32_t IMG_TILE_F = 128;  // frequency rows per tile

// Quantise + level-0 raster in one pass (round 4): one job per image; block b of a job = (tile column tx = local / n_bands,
// band of FUSED_FB image rows = local % n_bands); tiles[tile0 + tx * n_ty + ty] = RGBA array of level-0 tile (tx, ty) or NULL
struct FusedJob {
    const float *spec;
    uint16_t *img;
    uint32_t n_frames, height, i_start, i_end;
    uint32_t spec_pitch, img_pitch;
    uint32_t first_block, n_bands;
    uint32_t n_tx, n_ty;
    uint32_t tile0, reserved;
};
static_assert(sizeof(FusedJob) == 64, "FusedJob must have no implicit padding");
#if !defined(TH_FUSED_FB)
#define TH_FUSED_FB 32
#endif
#if !defined(TH_FUSED_THREADS)
#define TH_FUSED_THREADS 256
#endif
constexpr uint32_t FUSED_FB = TH_FUSED_FB;        // image rows (frequency bins) per block
constexpr uint32_t FUSED_THREADS = TH_FUSED_THREADS;

struct RasterJob {  // device-visible copy of th_raster_desc (+ derived fields)
    const uint16_t *img;
    uint8_t *rgba;
    uint32_t img_width, img_height, origin_x, origin_y, width, height;
    uint32_t img_pitch;      // u16 elements per image row (>= img_width)
    uint32_t quads_per_row;  // ceil(width / 4): a thread rasterises 4 horizontally adjacent pixels
    uint32_t inv_qpr;        // floor(2^32 / quads_per_row) + 1: q / quads_per_row == umulhi(q, inv_qpr)
    uint32_t inv_width;      // floor(2^32 / width) + 1 (flat-quad path of widths that are not multiples of 4)
    uint32_t first_block;    // this job's first block in the launch
};
static_assert(sizeof(RasterJob) == 64, "RasterJob: 60 bytes of fields, 4 of tail padding");
#if !defined(TH_RASTER_THREADS)
#define TH_RASTER_THREADS 256
#endif
#if !defined(TH_RASTER_QPB)
#define TH_RASTER_QPB 1024
#endif
constexpr uint32_t RASTER_THREADS = TH_RASTER_THREADS;
constexpr uint32_t RASTER_QUADS_PER_BLOCK = TH_RASTER_QPB;  // default: 256 threads x 4 quads of 4 pixels

// ---- kernels_waveform.hip
struct WaveJob {  // device-visible copy of th_wave_desc
    const float *wav;
    float *bins;
    uint64_t n_samples, start;
    uint32_t level, bin_count;
};
static_assert(sizeof(WaveJob) == 40, "WaveJob must have no implicit padding");
constexpr uint32_t WAVE_SMALL_MAX_LEVEL = 5;  // spb <= 32: one thread per bin (sequential, like render_tiles.rs:270-278)
inline uint32_t waveform_blocks_for(uint32_t level, uint32_t bin_count) {
    if (!bin_count) return 0;
    if (level <= WAVE_SMALL_MAX_LEVEL) return (bin_count + 255) / 256;
    return (bin_count + 3) / 4;  // one wave per bin, 4 waves per block
}

// waveform pyramid (all levels of a channel in one pass over the audio)
constexpr uint32_t PYR_MAX_LEVELS = 40;
struct PyrJob {
    const float *wav;
    float *out;          // all levels, level L at float offset level_off[L]
    float *sums;         // scratch: 2 * sums_half floats (bin sums of the level being reduced, ping-pong)
    uint64_t n_samples;
    uint64_t sums_half;
    uint64_t level_off[PYR_MAX_LEVELS];
    uint32_t n_levels;
    uint32_t aligned16;  // bit 0: wav is 16-byte aligned (float4 loads); bits 1-2: th_pyramid_desc.first_level (levels below it are not written)
};
static_assert(sizeof(PyrJob) == 48 + 8 * PYR_MAX_LEVELS, "PyrJob must have no implicit padding");
struct StatsJob {
    const float *wav;
    uint64_t n_samples;
    uint32_t aligned16, pad_;
};
static_assert(sizeof(StatsJob) == 24, "StatsJob must have no implicit padding");
inline uint64_t pyramid_bins(uint64_t n, uint32_t level) {
    if (n == 0) return 0;
    if (level >= 63) return 1;
    return (n + (1ull << level) - 1) >> level;
}
// Float offset of a level inside a channel's pyramid.  Every level starts on a 128-byte boundary (and the total is a
// multiple of 32 floats, so channels packed back to back stay aligned): level 0 is written with 16-byte stores laid on the
// output address, and a channel whose base was 4, 8 or 12 bytes off that grid took the dword-store fallback for half of
// all the bytes — with the dense layout three of four packed channels of the 13-level pyramid did (config 3: 2.10 ms;
// the same pass into an aligned 11-level pyramid 1.83 ms).
inline uint64_t pyramid_offset(uint64_t n, uint32_t level) {
    uint64_t off = 0;
    for (uint32_t l = 0; l < level; l++) off += (3 * pyramid_bins(n, l) + 31) / 32 * 32;
    return off;
}

// ---- the plans.  err != TH_OK: err_text is the message, nothing else is valid.  Every message names the first failing descriptor
// in the order the entry has always reported.
struct PlanStatus {
    int err = TH_OK;
    std::string err_text;
};

// th_spec_to_img_batch_dev[_ranged].  check_img is what runs on EVERY call, in front of the key comparison (the alignment of every
// descriptor and the range); plan_img, on a key miss, checks the shapes and builds the tables.
PlanStatus check_img(const th_img_desc *descs, size_t n, float min_dB, float max_dB, const float *d_range);
// the host range that zero-fills the images instead of quantising (drawing.rs:16-18)
bool db_range_all_neg_inf(float min_dB, float max_dB, const float *d_range);
struct ImgPlan : PlanStatus {
    std::vector<ImgJob> jobs;
    std::vector<uint32_t> block_job;  // job index of every block
    uint32_t n_blocks = 0;
};
ImgPlan plan_img(const th_img_desc *descs, size_t n);

// th_spec_to_img_raster_batch_dev.  check_fused: on every call; it also makes the batch's key (the descriptors and every tile
// pointer).  plan_fused: on a key miss.
PlanStatus check_fused(const th_img_tiles_desc *descs, size_t n, float min_dB, float max_dB, const float *d_range,
                       std::vector<unsigned char> *key);
struct FusedPlan : PlanStatus {
    std::vector<FusedJob> jobs;
    std::vector<uint32_t> block_job;
    std::vector<uint8_t *> ptrs;      // every image's tile pointers in (tx, ty) order; one NULL when there is none
    uint32_t n_blocks = 0;
};
FusedPlan plan_fused(const th_img_tiles_desc *descs, size_t n);

// th_raster_tiles_dev (on a key miss: the entry compares the key first)
struct RasterPlan : PlanStatus {
    std::vector<RasterJob> jobs;
    std::vector<uint32_t> block_job;
    uint32_t n_blocks = 0;
};
RasterPlan plan_raster(const th_raster_desc *descs, size_t n);

// th_waveform_tiles_dev
struct WavePlan : PlanStatus {
    std::vector<WaveJob> jobs;
    std::vector<uint32_t> start;      // n + 1: job i's blocks are [start[i], start[i + 1])
    uint32_t n_blocks = 0;
};
WavePlan plan_wave_tiles(const th_wave_desc *descs, size_t n);

// th_channel_stats_dev
struct StatsPlan : PlanStatus {
    std::vector<StatsJob> jobs;
    uint64_t max_samples = 0;
};
StatsPlan plan_stats(const th_stats_desc *descs, size_t n);

// th_waveform_pyramid_dev.  jobs[i].sums is unset until bind_pyramid; sums_at[i] is its float offset in the scratch of
// sums_floats floats.  launch: false when no job has both samples and levels (nothing is uploaded or launched then).
struct PyrPlan : PlanStatus {
    std::vector<PyrJob> jobs;
    std::vector<uint64_t> sums_at;
    uint64_t sums_floats = 0, max_samples = 0;
    uint32_t max_levels = 0;
    bool launch = false;
};
PyrPlan plan_pyramid(const th_pyramid_desc *descs, size_t n);
void bind_pyramid(PyrPlan &p, float *sums);

// The LOD > 0 branch of th_encode_spectrogram_tile_dev: separable Lanczos3 of the tile's crop box (render_tiles.rs:354-393).
// Tap tables are built in f64 exactly as the CPU restatement does, in the arithmetic of Pillow's ImagingResample (bit-identical to
// Pillow on the committed fixtures; formally unpinned against fast_image_resize itself).
struct LodTilePlan : PlanStatus {
    double left = 0, top = 0, crop_w = 0, crop_h = 0;  // the crop box in source coordinates
    long y_lo = 0, y_hi = 0;                           // source rows the vertical taps can reach, clamped to the image
    size_t n_rows = 0, dw = 0, dh = 0;                 // y_hi - y_lo; the tile
    // one blob: [x: start,count,wsum,w][y: start,count,wsum,w], 8-byte aligned sections; y's starts at y_at
    std::vector<unsigned char> blob;
    size_t y_at = 0;
    uint32_t taps_x = 0, taps_y = 0;
    size_t lod_at = 0;         // u16 offset of the resampled tile in the scratch, behind the n_rows x dw intermediate
    size_t scratch_bytes = 0;
};
// g: spectrogram_tile_geometry of the request, with width and height above zero
LodTilePlan plan_lod_tile(size_t img_width, size_t img_height, const TileGeom &g, uint32_t level_x, uint32_t level_y);

}  // namespace th
