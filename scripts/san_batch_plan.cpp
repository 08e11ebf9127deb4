// san_batch_plan.cpp — the planners of thesia_amd/csrc/batch_plan.h under AddressSanitizer and UBSan: the fixed batches of
// tests/golden/batch_plan_cases.json (the file's path may be given as the argument), batches at the limits and random batches, valid
// and refused, through every planner.  Device pointers are made-up addresses (a planner that read through one
// would fault here); the one host array a planner reads, th_img_tiles_desc.tiles, has exactly n_tiles_x * n_tiles_y entries, so a read
// past it is reported.  Every plan is checked for the sizes a launch relies on.  Not a pytest test and never loaded into python.
// From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined scripts/san_batch_plan.cpp
//       thesia_amd/csrc/batch_plan.cpp thesia_amd/csrc/host_math.cpp -o build/san_batch_plan && build/san_batch_plan   (one line)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../thesia_amd/csrc/batch_plan.h"

using namespace th;

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            std::exit(2);                                                             \
        }                                                                             \
    } while (0)

static std::mt19937_64 rng(20261019);
static uint64_t r(uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo); }  // [lo, hi)
template <class T>
static T *dev(uint64_t off) { return reinterpret_cast<T *>((uintptr_t)0x7F0000000000ull + off); }  // never read

static th_img_desc random_img(bool may_be_bad) {
    const uint64_t T = r(0, 1400), H = r(1, 1100), i0 = r(0, H), i1 = r(i0, H + 40);
    th_img_desc d{dev<const float>(4 * r(0, 64)), dev<uint16_t>((1ull << 32) + 2 * r(0, 64)), T, H, i0, i1, r(0, 2) * (H + r(0, 70)), r(0, 2) * (T + r(0, 70))};
    if (may_be_bad && r(0, 20) == 0) (r(0, 2) ? d.n_frames : d.spec_pitch) = r(0, 3) << 31;
    if (may_be_bad && r(0, 30) == 0) d.spec = dev<const float>(2);
    return d;
}

static size_t refused = 0, planned = 0;
static bool ok(const PlanStatus &p) {
    EXPECT((p.err == TH_OK) == p.err_text.empty());
    (p.err == TH_OK ? planned : refused)++;
    return p.err == TH_OK;
}

static void img_batch(const std::vector<th_img_desc> &d) {
    if (!ok(check_img(d.data(), d.size(), -100.f, 0.f, nullptr))) return;
    const ImgPlan p = plan_img(d.data(), d.size());
    if (!ok(p)) return;
    EXPECT(p.jobs.size() == d.size() && p.block_job.size() == p.n_blocks);
    for (size_t i = 0; i < d.size(); i++) EXPECT(p.jobs[i].first_tile + p.jobs[i].n_tiles <= p.n_blocks);
}

static void fused_batch(const std::vector<th_img_desc> &imgs, int spoil) {
    std::vector<std::unique_ptr<uint8_t *[]>> arrays;   // one allocation per image, of exactly its tile count
    std::vector<th_img_tiles_desc> d;
    size_t n_ptrs = 0;
    for (const th_img_desc &im : imgs) {
        const uint64_t out_h = im.i_end >= im.i_start ? im.i_end - im.i_start : 0;
        const bool live = out_h && im.n_frames && im.n_frames < (1ull << 31);
        const uint32_t n_tx = live ? (uint32_t)((im.n_frames + 511) / 512) : 0, n_ty = live ? (uint32_t)((out_h + 511) / 512) : 0;
        arrays.emplace_back(new uint8_t *[(size_t)n_tx * n_ty]);
        for (size_t t = 0; t < (size_t)n_tx * n_ty; t++) arrays.back()[t] = r(0, 8) ? dev<uint8_t>((2ull << 32) + 4 * r(0, 1 << 20) + (spoil == 1 && r(0, 9) == 0 ? 2 : 0)) : nullptr;
        d.push_back(th_img_tiles_desc{im, n_tx && n_ty ? arrays.back().get() : nullptr, n_tx, n_ty});
        n_ptrs += (size_t)n_tx * n_ty;
    }
    if (spoil == 2 && !d.empty() && d[0].n_tiles_x) d[0].n_tiles_x--;   // (fewer than the image has: the array still holds what is read)
    std::vector<unsigned char> key;
    if (!ok(check_fused(d.data(), d.size(), -100.f, 0.f, nullptr, &key))) return;
    const FusedPlan p = plan_fused(d.data(), d.size());
    if (!ok(p)) return;
    EXPECT(p.jobs.size() == d.size() && p.block_job.size() == p.n_blocks && p.ptrs.size() == (n_ptrs ? n_ptrs : 1));
    EXPECT(key.size() == d.size() * sizeof(th_img_tiles_desc) + n_ptrs * sizeof(void *));
    for (const FusedJob &j : p.jobs) EXPECT((size_t)j.tile0 + (size_t)j.n_tx * j.n_ty <= n_ptrs && j.n_bands >= 1);
}

static void raster_batch(const std::vector<th_raster_desc> &d) {
    const RasterPlan p = plan_raster(d.data(), d.size());
    if (!ok(p)) return;
    EXPECT(p.jobs.size() == d.size() && p.block_job.size() == p.n_blocks);
    for (const RasterJob &j : p.jobs) {
        // the quads of the job fit its blocks, and the reciprocals divide the largest index the kernel forms
        const uint64_t quads = (uint64_t)j.quads_per_row * j.height, px = (uint64_t)j.width * j.height;
        if (quads > 1 && j.quads_per_row > 1) EXPECT((((quads - 1) * j.inv_qpr) >> 32) == (quads - 1) / j.quads_per_row);
        if (px > 1 && j.width > 1) EXPECT((((px - 1) * j.inv_width) >> 32) == (px - 1) / j.width);
    }
}

// ---- the fixed cases of the CPU test: {"case":{"entry":...,"rows":[[...]],"tiles":[...] | "args":[...]},"want":...}, integers only in
// what is read here (the ranges of the cases are left at their defaults)
static std::vector<uint64_t> int_list(const std::string &js, size_t &at) {  // at: behind the list's '['; leaves at behind its ']'
    std::vector<uint64_t> v;
    while (js[at] != ']') {
        char *end = nullptr;
        v.push_back(std::strtoull(js.c_str() + at, &end, 10));
        EXPECT(end != js.c_str() + at);
        at = (size_t)(end - js.c_str());
        if (js[at] == ',') at++;
    }
    at++;
    return v;
}
static std::vector<uint64_t> field_list(const std::string &c, const char *name) {
    size_t at = c.find(std::string("\"") + name + "\":[");
    if (at == std::string::npos) return {};
    at += std::strlen(name) + 4;
    return int_list(c, at);
}
static size_t fixed_cases(const char *path) {
    std::ifstream f(path);
    EXPECT(f.good());
    const std::string js((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t n_cases = 0;
    for (size_t at = js.find("\"case\":{"); at != std::string::npos; at = js.find("\"case\":{", at + 1), n_cases++) {
        const std::string c = js.substr(at, js.find("\"want\":", at) - at);
        const size_t e = c.find("\"entry\":\"") + 9;
        const std::string entry = c.substr(e, c.find('"', e) - e);
        std::vector<std::vector<uint64_t>> rows;
        size_t r = c.find("\"rows\":[");
        if (r != std::string::npos)
            for (r += 8; c[r] == '[' || c[r] == ','; ) {
                if (c[r] == ',') r++;
                r++;
                rows.push_back(int_list(c, r));
            }
        auto P = [](uint64_t a) { return reinterpret_cast<void *>((uintptr_t)a); };
        if (entry == "img") {
            std::vector<th_img_desc> d;
            for (const auto &w : rows) d.push_back(th_img_desc{(const float *)P(w[0]), (uint16_t *)P(w[1]), w[2], w[3], w[4], w[5], w[6], w[7]});
            img_batch(d);
        } else if (entry == "fused") {
            const std::vector<uint64_t> tiles = field_list(c, "tiles");
            std::vector<std::unique_ptr<uint8_t *[]>> arrays;
            std::vector<th_img_tiles_desc> d;
            for (const auto &w : rows) {
                const size_t n_t = (size_t)(w[9] * w[10]);
                arrays.emplace_back(new uint8_t *[n_t]);
                for (size_t t = 0; t < n_t; t++) arrays.back()[t] = (uint8_t *)P(tiles[w[8] + t]);
                d.push_back(th_img_tiles_desc{th_img_desc{(const float *)P(w[0]), (uint16_t *)P(w[1]), w[2], w[3], w[4], w[5], w[6], w[7]},
                                              n_t ? arrays.back().get() : nullptr, (uint32_t)w[9], (uint32_t)w[10]});
            }
            std::vector<unsigned char> key;
            if (ok(check_fused(d.data(), d.size(), -100.f, 0.f, nullptr, &key))) {
                const FusedPlan p = plan_fused(d.data(), d.size());
                if (ok(p)) EXPECT(p.jobs.size() == d.size() && p.block_job.size() == p.n_blocks);
            }
        } else if (entry == "raster") {
            std::vector<th_raster_desc> d;
            for (const auto &w : rows)
                d.push_back(th_raster_desc{(const uint16_t *)P(w[0]), (uint8_t *)P(w[1]), (uint32_t)w[2], (uint32_t)w[3], (uint32_t)w[4], (uint32_t)w[5],
                                           (uint32_t)w[6], (uint32_t)w[7], (uint32_t)w[8], (uint32_t)w[9]});
            raster_batch(d);
        } else if (entry == "wave") {
            std::vector<th_wave_desc> d;
            for (const auto &w : rows) d.push_back(th_wave_desc{(const float *)P(w[0]), (float *)P(w[1]), w[2], w[3], (uint32_t)w[4], (uint32_t)w[5]});
            const WavePlan p = plan_wave_tiles(d.data(), d.size());
            if (ok(p)) EXPECT(p.start.size() == d.size() + 1 && p.start.back() == p.n_blocks);
        } else if (entry == "stats") {
            std::vector<th_stats_desc> d;
            for (const auto &w : rows) d.push_back(th_stats_desc{(const float *)P(w[0]), w[1]});
            if (ok(plan_stats(d.data(), d.size()))) {}
        } else if (entry == "pyramid") {
            std::vector<th_pyramid_desc> d;
            for (const auto &w : rows) d.push_back(th_pyramid_desc{(const float *)P(w[0]), (float *)P(w[1]), w[2], (uint32_t)w[3], (uint32_t)w[4]});
            PyrPlan p = plan_pyramid(d.data(), d.size());
            if (ok(p)) bind_pyramid(p, dev<float>(6ull << 32));
        } else if (entry == "lod") {
            const std::vector<uint64_t> a = field_list(c, "args");
            EXPECT(a.size() == 6);
            const TileGeom g = spectrogram_tile_geometry(a[0], a[1], (uint32_t)a[2], (uint32_t)a[3], (uint32_t)a[4], (uint32_t)a[5]);
            if (g.width && g.height) (void)ok(plan_lod_tile(a[0], a[1], g, (uint32_t)a[2], (uint32_t)a[3]));
        } else {
            EXPECT(!"a known entry");
        }
    }
    return n_cases;
}

int main(int argc, char **argv) {
    const size_t n_fixed = fixed_cases(argc > 1 ? argv[1] : "tests/golden/batch_plan_cases.json");
    EXPECT(n_fixed >= 10);
    for (int it = 0; it < 400; it++) {
        std::vector<th_img_desc> imgs(r(1, 6));
        for (th_img_desc &d : imgs) d = random_img(it % 3 == 0);
        img_batch(imgs);
        fused_batch(imgs, it % 5 == 0 ? (int)r(1, 3) : 0);

        std::vector<th_raster_desc> ras(r(1, 6));
        for (th_raster_desc &d : ras) {
            const uint32_t W = (uint32_t)r(1, 3000), H = (uint32_t)r(1, 1200), w = (uint32_t)r(0, std::min<uint32_t>(W, 700) + 1), h = (uint32_t)r(0, std::min<uint32_t>(H, 700) + 1);
            d = th_raster_desc{dev<const uint16_t>(2 * r(0, 16)), dev<uint8_t>((3ull << 32) + 4 * r(0, 16)), W, H, (uint32_t)r(0, W - w + 1), (uint32_t)r(0, H - h + 1), w, h,
                               (uint32_t)(r(0, 2) * (W + r(0, 64))), 0};
            if (it % 4 == 0 && r(0, 6) == 0) d.origin_x = W;
        }
        raster_batch(ras);

        std::vector<th_wave_desc> wav(r(1, 6));
        for (th_wave_desc &d : wav) {
            const uint32_t level = (uint32_t)r(0, it % 7 == 0 ? 42 : 20), bins = (uint32_t)r(0, it % 9 == 0 ? 1030 : 1025);
            const uint64_t n = r(1, 1ull << 34), reach = (uint64_t)(bins ? bins - 1 : 0) << std::min<uint32_t>(level, 39);
            d = th_wave_desc{dev<const float>(4 * r(0, 8)), dev<float>((4ull << 32) + 4 * r(0, 8)), n, it % 4 && reach < n ? r(0, n - reach) : r(0, n + 2), level, bins};
        }
        const WavePlan wp = plan_wave_tiles(wav.data(), wav.size());
        if (ok(wp)) EXPECT(wp.jobs.size() == wav.size() && wp.start.size() == wav.size() + 1 && wp.start.back() == wp.n_blocks);

        std::vector<th_stats_desc> sts(r(1, 6));
        for (th_stats_desc &d : sts) d = th_stats_desc{dev<const float>(4 * r(0, 8) + (r(0, 40) == 0 ? 2 : 0)), r(0, r(0, 30) ? 1ull << 30 : 1ull << 41)};
        const StatsPlan sp = plan_stats(sts.data(), sts.size());
        if (ok(sp)) EXPECT(sp.jobs.size() == sts.size());

        std::vector<th_pyramid_desc> pyr(r(1, 6));
        for (th_pyramid_desc &d : pyr)
            d = th_pyramid_desc{dev<const float>(4 * r(0, 8)), dev<float>((5ull << 32) + 4 * r(0, 64)), r(0, 1ull << r(1, 36)), (uint32_t)r(0, 42), (uint32_t)r(0, r(0, 15) ? 3 : 4)};
        PyrPlan pp = plan_pyramid(pyr.data(), pyr.size());
        if (ok(pp)) {
            std::vector<float> sums(pp.sums_floats < (1u << 22) ? pp.sums_floats : 0);   // (bound for real when it is small)
            bind_pyramid(pp, sums.empty() ? dev<float>(6ull << 32) : sums.data());
            EXPECT(pp.jobs.size() == pyr.size() && pp.sums_at.size() == pyr.size());
            for (size_t i = 0; i < pyr.size(); i++) EXPECT(pp.sums_at[i] + 2 * pp.jobs[i].sums_half <= pp.sums_floats);
        }

        const size_t W = r(1, 4000), H = r(1, 1200);
        const uint32_t ly = (uint32_t)r(0, 5), lx = (uint32_t)r(ly ? 0 : 1, 6), tx = (uint32_t)r(0, 3), ty = (uint32_t)r(0, 2);
        const TileGeom g = spectrogram_tile_geometry(W, H, lx, ly, tx, ty);
        if (g.width && g.height) {
            const LodTilePlan lp = plan_lod_tile(W, H, g, lx, ly);
            if (ok(lp)) {
                EXPECT(lp.blob.size() == lp.y_at + 16 * lp.dh + 8 * lp.dh * (size_t)lp.taps_y && lp.y_at == 16 * lp.dw + 8 * lp.dw * (size_t)lp.taps_x);
                EXPECT(lp.y_lo >= 0 && lp.y_hi <= (long)H && (lp.lod_at + lp.dw * lp.dh) * 2 <= lp.scratch_bytes);
            }
        }
    }
    // at the limits: 2^27 blocks in one descriptor (image, fused), the channel counts, a level past the tap-table bound, tile headers
    img_batch({th_img_desc{dev<const float>(0), dev<uint16_t>(64), 64ull << 20, 128ull << 7, 0, 128ull << 7, 0, 0}});
    {
        std::vector<th_stats_desc> many(65536, th_stats_desc{dev<const float>(0), 100});
        EXPECT(!ok(plan_stats(many.data(), many.size())) && ok(plan_stats(many.data(), 65535)));
        std::vector<th_pyramid_desc> pm(65536, th_pyramid_desc{dev<const float>(0), dev<float>(4096), 5000, 13, 2});
        EXPECT(!ok(plan_pyramid(pm.data(), pm.size())) && ok(plan_pyramid(pm.data(), 65535)));
    }
    EXPECT(plan_lod_tile(600, 16384, spectrogram_tile_geometry(600, 16384, 0, 14, 0, 0), 0, 14).err == TH_ERR_UNSUPPORTED);
    EXPECT(plan_lod_tile(600, 16384, spectrogram_tile_geometry(600, 16384, 0, 13, 0, 0), 0, 13).err == TH_OK);
    {
        std::unique_ptr<uint8_t[]> h40(new uint8_t[40]), h24(new uint8_t[24]);   // exactly the headers' sizes
        put_spectrogram_tile_header(h40.get(), 7, spectrogram_tile_geometry(600, 40, 1, 1, 0, 0), 1, 1, 0, 0);
        put_waveform_tile_header(h24.get(), 7, 1, (size_t)1 << 33, 0);
        EXPECT(h40[0] == 7 && h24[12] == 0xFF && h24[15] == 0xFF);
    }
    std::printf("san_batch_plan: %zu fixed cases, %zu plans made, %zu refused, nothing reported\n", n_fixed, planned, refused);
    return 0;
}
