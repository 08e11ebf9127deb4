// batch_plan.cpp — the host planning of the image, raster and waveform batch entries (batch_plan.h).  Plain C++: compiled into the
// library and, by g++, into the emulator library of tests/emu/.
#include "batch_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "plan_error.h"

namespace th {

namespace {
#define PLAN_REQUIRE(P, cond, ...)                                         \
    do {                                                                   \
        if (!(cond)) return plan_error<P>(TH_ERR_INVALID_ARG, __VA_ARGS__); \
    } while (0)

bool aligned(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }
// floor(2^32 / d) + 1: x / d == (x * magic) >> 32 for every x with x * d < 2^32 (d = 1 has no such word: the kernels test for it)
uint32_t magic_reciprocal(uint32_t d) { return d > 1 ? (uint32_t)((1ull << 32) / d) + 1u : 0u; }
}  // namespace

// ------------------------------------------------------------------------------------------ spec → img
bool db_range_all_neg_inf(float min_dB, float max_dB, const float *d_range) {
    return !d_range && (min_dB == max_dB) && std::isinf(max_dB) && max_dB < 0;  // drawing.rs:16-18
}

PlanStatus check_img(const th_img_desc *descs, size_t n, float min_dB, float max_dB, const float *d_range) {
    for (size_t i = 0; i < n; i++) {
        PLAN_REQUIRE(PlanStatus, aligned(descs[i].spec, 4), "desc %zu: spec must be 4-byte aligned", i);
        PLAN_REQUIRE(PlanStatus, aligned(descs[i].img, 2), "desc %zu: img must be 2-byte aligned", i);
    }
    if (!db_range_all_neg_inf(min_dB, max_dB, d_range) && !d_range)
        PLAN_REQUIRE(PlanStatus, std::isfinite(min_dB), "min_dB must be finite (drawing.rs:19)");
    return PlanStatus{};
}

ImgPlan plan_img(const th_img_desc *descs, size_t n) {
    ImgPlan p;
    p.jobs.resize(n);
    uint64_t tiles = 0;
    for (size_t i = 0; i < n; i++) {
        const th_img_desc &d = descs[i];
        PLAN_REQUIRE(ImgPlan, d.i_end >= d.i_start, "desc %zu: i_end < i_start", i);
        const uint64_t out_h = d.i_end - d.i_start;
        PLAN_REQUIRE(ImgPlan, d.n_frames < (1ull << 31) && d.height < (1ull << 31) && d.i_end < (1ull << 31), "desc %zu: too large", i);
        PLAN_REQUIRE(ImgPlan, (d.spec && d.img) || out_h * d.n_frames == 0, "desc %zu: NULL device pointer", i);
        PLAN_REQUIRE(ImgPlan, d.spec_pitch == 0 || (d.spec_pitch >= d.height && d.spec_pitch < (1ull << 31)), "desc %zu: bad spec_pitch", i);
        PLAN_REQUIRE(ImgPlan, d.img_pitch == 0 || (d.img_pitch >= d.n_frames && d.img_pitch < (1ull << 31)), "desc %zu: bad img_pitch", i);
        const uint64_t nt = ((d.n_frames + IMG_TILE_T - 1) / IMG_TILE_T) * ((out_h + IMG_TILE_F - 1) / IMG_TILE_F);
        PLAN_REQUIRE(ImgPlan, tiles + nt < (1ull << 27), "batch too large for one launch");
        p.jobs[i] = ImgJob{d.spec, d.img, (uint32_t)d.n_frames, (uint32_t)d.height, (uint32_t)d.i_start, (uint32_t)d.i_end,
                           (uint32_t)(d.spec_pitch ? d.spec_pitch : d.height), (uint32_t)(d.img_pitch ? d.img_pitch : d.n_frames),
                           (uint32_t)tiles, (uint32_t)nt};
        tiles += nt;
        p.block_job.insert(p.block_job.end(), (size_t)nt, (uint32_t)i);
    }
    p.n_blocks = (uint32_t)tiles;
    return p;
}

// ------------------------------------------------------------------------------------------ quantise + level-0 raster
PlanStatus check_fused(const th_img_tiles_desc *descs, size_t n, float min_dB, float max_dB, const float *d_range,
                       std::vector<unsigned char> *key) {
    for (size_t i = 0; i < n; i++) {
        PLAN_REQUIRE(PlanStatus, aligned(descs[i].img.spec, 4), "desc %zu: spec must be 4-byte aligned", i);
        PLAN_REQUIRE(PlanStatus, aligned(descs[i].img.img, 2), "desc %zu: img must be 2-byte aligned", i);
    }
    if (!db_range_all_neg_inf(min_dB, max_dB, d_range) && !d_range)
        PLAN_REQUIRE(PlanStatus, std::isfinite(min_dB), "min_dB must be finite (drawing.rs:19)");
    size_t n_ptrs = 0;
    for (size_t i = 0; i < n; i++) n_ptrs += (size_t)descs[i].n_tiles_x * descs[i].n_tiles_y;
    key->clear();
    key->reserve(n * sizeof(th_img_tiles_desc) + n_ptrs * sizeof(void *));
    for (size_t i = 0; i < n; i++) {
        const th_img_tiles_desc &d = descs[i];
        PLAN_REQUIRE(PlanStatus, d.tiles || (size_t)d.n_tiles_x * d.n_tiles_y == 0, "desc %zu: tiles is NULL", i);
        const unsigned char *p = reinterpret_cast<const unsigned char *>(&d);
        key->insert(key->end(), p, p + sizeof(th_img_tiles_desc));
        const unsigned char *q = reinterpret_cast<const unsigned char *>(d.tiles);
        key->insert(key->end(), q, q + (size_t)d.n_tiles_x * d.n_tiles_y * sizeof(void *));
    }
    return PlanStatus{};
}

FusedPlan plan_fused(const th_img_tiles_desc *descs, size_t n) {
    FusedPlan p;
    p.jobs.resize(n);
    uint64_t blocks = 0;
    for (size_t i = 0; i < n; i++) {
        const th_img_desc &d = descs[i].img;
        PLAN_REQUIRE(FusedPlan, d.i_end >= d.i_start, "desc %zu: i_end < i_start", i);
        const uint64_t out_h = d.i_end - d.i_start;
        PLAN_REQUIRE(FusedPlan, d.n_frames < (1ull << 31) && d.height < (1ull << 31) && d.i_end < (1ull << 31), "desc %zu: too large", i);
        PLAN_REQUIRE(FusedPlan, (d.spec && d.img && d.height >= 1) || out_h * d.n_frames == 0, "desc %zu: NULL device pointer or empty spec", i);
        PLAN_REQUIRE(FusedPlan, d.spec_pitch == 0 || (d.spec_pitch >= d.height && d.spec_pitch < (1ull << 31)), "desc %zu: bad spec_pitch", i);
        PLAN_REQUIRE(FusedPlan, d.img_pitch == 0 || (d.img_pitch >= d.n_frames && d.img_pitch < (1ull << 31)), "desc %zu: bad img_pitch", i);
        const uint64_t n_tx = out_h && d.n_frames ? (d.n_frames + 511) / 512 : 0, n_ty = out_h && d.n_frames ? (out_h + 511) / 512 : 0;
        PLAN_REQUIRE(FusedPlan, descs[i].n_tiles_x == n_tx && descs[i].n_tiles_y == n_ty, "desc %zu: the image has %llu x %llu level-0 tiles, not %u x %u",
                     i, (unsigned long long)n_tx, (unsigned long long)n_ty, descs[i].n_tiles_x, descs[i].n_tiles_y);
        const uint64_t n_bands = (out_h + FUSED_FB - 1) / FUSED_FB, nb = n_tx * n_bands;
        PLAN_REQUIRE(FusedPlan, blocks + nb < (1ull << 27) && p.ptrs.size() + n_tx * n_ty < (1ull << 31), "batch too large for one launch");
        for (uint64_t t = 0; t < n_tx * n_ty; t++) {
            uint8_t *tp = descs[i].tiles[t];
            PLAN_REQUIRE(FusedPlan, aligned(tp, 4), "desc %zu: tile %llu must be 4-byte aligned", i, (unsigned long long)t);
            p.ptrs.push_back(tp);
        }
        p.jobs[i] = FusedJob{d.spec, d.img, (uint32_t)d.n_frames, (uint32_t)d.height, (uint32_t)d.i_start, (uint32_t)d.i_end,
                             (uint32_t)(d.spec_pitch ? d.spec_pitch : d.height), (uint32_t)(d.img_pitch ? d.img_pitch : d.n_frames),
                             (uint32_t)blocks, (uint32_t)std::max<uint64_t>(n_bands, 1), (uint32_t)n_tx, (uint32_t)n_ty,
                             (uint32_t)(p.ptrs.size() - n_tx * n_ty), 0u};
        blocks += nb;
        p.block_job.insert(p.block_job.end(), (size_t)nb, (uint32_t)i);
    }
    if (p.ptrs.empty()) p.ptrs.push_back(nullptr);
    p.n_blocks = (uint32_t)blocks;
    return p;
}

// ------------------------------------------------------------------------------------------ raster
RasterPlan plan_raster(const th_raster_desc *descs, size_t n) {
    RasterPlan p;
    p.jobs.resize(n);
    uint64_t blocks = 0;
    for (size_t i = 0; i < n; i++) {
        const th_raster_desc &d = descs[i];
        PLAN_REQUIRE(RasterPlan, (uint64_t)d.origin_x + d.width <= d.img_width && (uint64_t)d.origin_y + d.height <= d.img_height,
                     "desc %zu: tile rectangle outside the image", i);
        const uint64_t px = (uint64_t)d.width * d.height;
        PLAN_REQUIRE(RasterPlan, px < (1ull << 31), "desc %zu: tile too large", i);
        PLAN_REQUIRE(RasterPlan, px == 0 || (d.img && d.rgba), "desc %zu: NULL device pointer", i);
        PLAN_REQUIRE(RasterPlan, aligned(d.rgba, 4), "desc %zu: rgba must be 4-byte aligned", i);
        PLAN_REQUIRE(RasterPlan, aligned(d.img, 2), "desc %zu: img must be 2-byte aligned", i);
        PLAN_REQUIRE(RasterPlan, d.img_pitch == 0 || d.img_pitch >= d.img_width, "desc %zu: img_pitch < img_width", i);
        const uint32_t qpr = (d.width + 3) / 4;
        // the reciprocals are exact for q * qpr < 2^32 and p * width < 2^32; the kernel forms q < qpr * height and p < px
        PLAN_REQUIRE(RasterPlan, px == 0 || (px + 4) * d.width < (1ull << 32), "desc %zu: tile too large", i);
        // (+1: a tile base off the 16-byte grid shifts the quads by up to 3 pixels, see raster_quads)
        const uint64_t nb = ((uint64_t)qpr * d.height + 1 + RASTER_QUADS_PER_BLOCK - 1) / RASTER_QUADS_PER_BLOCK;
        PLAN_REQUIRE(RasterPlan, blocks + nb < (1ull << 27), "batch too large for one launch");
        p.jobs[i] = RasterJob{d.img, d.rgba, d.img_width, d.img_height, d.origin_x, d.origin_y, d.width, d.height,
                              d.img_pitch ? d.img_pitch : d.img_width, qpr, magic_reciprocal(qpr), magic_reciprocal(d.width), (uint32_t)blocks};
        blocks += nb;
        p.block_job.insert(p.block_job.end(), (size_t)nb, (uint32_t)i);
    }
    p.n_blocks = (uint32_t)blocks;
    return p;
}

// ------------------------------------------------------------------------------------------ waveform
WavePlan plan_wave_tiles(const th_wave_desc *descs, size_t n) {
    WavePlan p;
    p.jobs.resize(n);
    p.start.resize(n + 1);
    uint64_t blocks = 0;
    for (size_t i = 0; i < n; i++) {
        const th_wave_desc &d = descs[i];
        PLAN_REQUIRE(WavePlan, d.bin_count <= TH_WAVEFORM_TILE_BINS, "desc %zu: bin_count > 1024", i);
        PLAN_REQUIRE(WavePlan, d.level < 40, "desc %zu: level %u too large", i, d.level);
        PLAN_REQUIRE(WavePlan, d.bin_count == 0 || (d.wav && d.bins), "desc %zu: NULL device pointer", i);
        PLAN_REQUIRE(WavePlan, aligned(d.wav, 4), "desc %zu: wav must be 4-byte aligned", i);
        PLAN_REQUIRE(WavePlan, aligned(d.bins, 4), "desc %zu: bins must be 4-byte aligned", i);
        if (d.bin_count) {
            const uint64_t spb = 1ull << d.level;
            PLAN_REQUIRE(WavePlan, d.start < d.n_samples && d.start + (uint64_t)(d.bin_count - 1) * spb < d.n_samples,
                         "desc %zu: bins run past the end of the channel", i);
        }
        p.jobs[i] = WaveJob{d.wav, d.bins, d.n_samples, d.start, d.level, d.bin_count};
        p.start[i] = (uint32_t)blocks;
        blocks += waveform_blocks_for(d.level, d.bin_count);
        PLAN_REQUIRE(WavePlan, blocks < (1ull << 31), "batch too large for one launch");
    }
    p.start[n] = p.n_blocks = (uint32_t)blocks;
    return p;
}

// ------------------------------------------------------------------------------------------ channel statistics
StatsPlan plan_stats(const th_stats_desc *descs, size_t n) {
    PLAN_REQUIRE(StatsPlan, n <= 65535, "at most 65535 channels per call");
    StatsPlan p;
    p.jobs.resize(n);
    for (size_t i = 0; i < n; i++) {
        PLAN_REQUIRE(StatsPlan, descs[i].n_samples == 0 || descs[i].wav, "desc %zu: NULL device pointer", i);
        PLAN_REQUIRE(StatsPlan, aligned(descs[i].wav, 4), "desc %zu: wav must be 4-byte aligned", i);
        PLAN_REQUIRE(StatsPlan, descs[i].n_samples < (1ull << 40), "desc %zu: too many samples", i);
        p.jobs[i] = StatsJob{descs[i].wav, descs[i].n_samples, aligned(descs[i].wav, 16), 0};
        p.max_samples = std::max<uint64_t>(p.max_samples, descs[i].n_samples);
    }
    return p;
}

// ------------------------------------------------------------------------------------------ waveform pyramid
PyrPlan plan_pyramid(const th_pyramid_desc *descs, size_t n) {
    PLAN_REQUIRE(PyrPlan, n <= 65535, "at most 65535 channels per call");
    PyrPlan p;
    p.jobs.resize(n);
    p.sums_at.resize(n);
    for (size_t i = 0; i < n; i++) {
        const th_pyramid_desc &d = descs[i];
        PLAN_REQUIRE(PyrPlan, d.n_levels <= PYR_MAX_LEVELS, "desc %zu: more than %u levels", i, PYR_MAX_LEVELS);
        PLAN_REQUIRE(PyrPlan, d.n_samples == 0 || d.n_levels == 0 || (d.wav && d.out), "desc %zu: NULL device pointer", i);
        PLAN_REQUIRE(PyrPlan, aligned(d.wav, 4), "desc %zu: wav must be 4-byte aligned", i);
        PLAN_REQUIRE(PyrPlan, aligned(d.out, 4), "desc %zu: out must be 4-byte aligned", i);
        PLAN_REQUIRE(PyrPlan, d.n_samples < (1ull << 40), "desc %zu: too many samples", i);
        PLAN_REQUIRE(PyrPlan, d.first_level <= 2, "desc %zu: first_level must be 0, 1 or 2", i);
        PyrJob &j = p.jobs[i];
        j = PyrJob{};
        j.wav = d.wav;
        // first_level = 1: the kernels keep addressing level L at out + level_off[L]; shifting `out` back by the extent of the skipped levels
        // (a multiple of 128 bytes) puts level first_level at the start of the caller's buffer; the levels below are never touched
        j.out = d.first_level ? reinterpret_cast<float *>(reinterpret_cast<uintptr_t>(d.out) - pyramid_offset(d.n_samples, d.first_level) * sizeof(float)) : d.out;
        j.n_samples = (d.n_levels > d.first_level) ? d.n_samples : 0;
        j.n_levels = d.n_levels;
        j.aligned16 = (aligned(d.wav, 16) ? 1u : 0u) | (d.first_level << 1);
        for (uint32_t l = 0; l < PYR_MAX_LEVELS; l++) j.level_off[l] = pyramid_offset(d.n_samples, l);
        j.sums_half = pyramid_bins(d.n_samples, 12);
        p.sums_at[i] = p.sums_floats;
        p.sums_floats += 2 * j.sums_half;
        p.max_samples = std::max<uint64_t>(p.max_samples, j.n_samples);
        p.max_levels = std::max(p.max_levels, d.n_levels);
    }
    p.launch = p.max_samples && p.max_levels;
    return p;
}

void bind_pyramid(PyrPlan &p, float *sums) {
    for (size_t i = 0; i < p.jobs.size(); i++) p.jobs[i].sums = sums + p.sums_at[i];
}

// ------------------------------------------------------------------------------------------ one LOD > 0 spectrogram tile
LodTilePlan plan_lod_tile(size_t img_width, size_t img_height, const TileGeom &g, uint32_t level_x, uint32_t level_y) {
    LodTilePlan p;
    const size_t dw = p.dw = g.width, dh = p.dh = g.height;
    const double W = (double)img_width, Hh = (double)img_height;
    p.left = (double)g.origin_x * W / (double)g.lod_w;
    p.top = (double)g.origin_y * Hh / (double)g.lod_h;
    p.crop_w = (double)(g.origin_x + dw) * W / (double)g.lod_w - p.left;
    p.crop_h = (double)(g.origin_y + dh) * Hh / (double)g.lod_h - p.top;
    const double scy = p.crop_h / (double)dh, fy = scy < 1.0 ? 1.0 : scy, supy = 3.0 * fy;
    p.y_lo = (long)std::floor(p.top - supy) - 1;
    p.y_hi = (long)std::ceil(p.top + p.crop_h + supy) + 1;
    if (p.y_lo < 0) p.y_lo = 0;
    if (p.y_hi > (long)img_height) p.y_hi = (long)img_height;
    p.n_rows = (size_t)(p.y_hi - p.y_lo);
    // a tap table beyond this is a level no viewer asks for; refuse instead of allocating GBs
    const double est_taps = 6.0 * std::max(p.crop_w / (double)dw, p.crop_h / (double)dh) + 4.0;
    if (est_taps * 8.0 * (double)std::max(dw, dh) > 256.0 * 1024 * 1024)
        return plan_error<LodTilePlan>(TH_ERR_UNSUPPORTED, "LOD level (%u,%u) needs a tap table beyond 256 MB", level_x, level_y);
    LodAxisHost ax, ay;
    build_lod_axis(p.left, p.crop_w, dw, 0, (long)img_width, ax);
    build_lod_axis(p.top, p.crop_h, dh, p.y_lo, p.y_hi, ay);
    p.y_at = ax.blob_bytes(dw);
    p.blob.resize(p.y_at + ay.blob_bytes(dh));
    ax.pack(p.blob.data(), dw);
    ay.pack(p.blob.data() + p.y_at, dh);
    p.taps_x = ax.max_taps;
    p.taps_y = ay.max_taps;
    p.lod_at = ((p.n_rows * dw + 3) / 4) * 4;
    p.scratch_bytes = (p.n_rows * dw + dw * dh) * sizeof(uint16_t) + 64;
    return p;
}

}  // namespace th
