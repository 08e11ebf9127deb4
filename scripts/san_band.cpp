// san_band.cpp — the band-filter kernel's source run on the CPU, a workgroup's threads one after the other between the kernel's
// barriers (thesia_amd/csrc/band_block.h is what kernels_band.hip calls), under AddressSanitizer and UBSan: every staged array, the
// row, every source and destination has exactly the size the host side gives it, so a read or write out of bounds is reported; every
// output is compared bit for bit with th_band_f32.  Not a pytest test and never loaded into python.  From the repository root:
//   hipcc -x hip --cuda-host-only -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         scripts/san_band.cpp -Lthesia_amd -lthesia_amd -Wl,-rpath,$PWD/thesia_amd -o build/san_band && build/san_band
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../thesia_amd/csrc/band_block.h"

using namespace th;

#define CHECK(call)                                                        \
    do {                                                                   \
        if ((call) != TH_OK) {                                             \
            std::fprintf(stderr, "%s failed: %s\n", #call, th_last_error()); \
            std::exit(2);                                                  \
        }                                                                  \
    } while (0)

struct Lane {
    ResampleAcc acc[BAND_R];
    float pre[BAND_PRE];
};

// the kernel's loop: what lies between two barriers runs for every thread before anything behind the barrier does
static void run_block(const BandJob &job, uint32_t b, const float *row, uint32_t taps) {
    const BandBlock k = band_block_of(job, b);
    if (!k.any) return;
    // exact sizes: a read or write past a staged span is reported
    std::unique_ptr<float[]> xs[2] = {std::unique_ptr<float[]>(new float[BAND_XS]), std::unique_ptr<float[]>(new float[BAND_XS])};
    std::vector<Lane> ln(BAND_THREADS);
    for (uint32_t t = 0; t < BAND_THREADS; t++) {
        band_fetch(job, k, taps, 0, t, ln[t].pre);
        band_commit(job, k, taps, 0, ln[t].pre, t, xs[0].get());
    }
    uint32_t buf = 0;
    for (uint32_t kb = 0; kb < taps; kb += BAND_TAP_BLOCK, buf ^= 1u) {
        const bool more = kb + BAND_TAP_BLOCK < taps;
        for (uint32_t t = 0; t < BAND_THREADS; t++) {
            if (more) band_fetch(job, k, taps, kb + BAND_TAP_BLOCK, t, ln[t].pre);
            if (taps - kb >= BAND_TAP_BLOCK)
                band_accumulate<true>(ln[t].acc, row + kb, BAND_TAP_BLOCK, xs[buf].get(), t);
            else
                band_accumulate<false>(ln[t].acc, row + kb, taps - kb, xs[buf].get(), t);
            if (more) band_commit(job, k, taps, kb + BAND_TAP_BLOCK, ln[t].pre, t, xs[buf ^ 1u].get());
        }
    }
    for (uint32_t t = 0; t < BAND_THREADS; t++) band_store(job, k, t, ln[t].acc);
}

static size_t n_checked = 0, n_blocks_run = 0;

static void run_case(uint32_t K, uint32_t mode, double f_lo, double f_hi, size_t n_in, uint64_t ja, uint64_t jb_want, uint32_t n_ch) {
    const uint32_t sr = 8000, taps = 2 * K;
    th_band_plan plan{};
    plan.half_taps = K;  // (a plan as th_band_plan_for fills it; K set directly so that every length is reached)
    plan.mode = mode;
    plan.f_lo_hz = f_lo;
    plan.f_hi_hz = f_hi;
    plan.trans_hz = 16.0 * sr / (5.0 * K);
    std::vector<float> row(taps);
    CHECK(th_band_coefs(sr, &plan, nullptr, row.data()));
    const uint64_t jb = jb_want < n_in ? jb_want : n_in;
    if (ja >= jb) return;
    std::vector<std::vector<float>> src(n_ch, std::vector<float>(n_in));
    std::vector<const float *> chan(n_ch);
    uint32_t seed = 12345u + K + 7u * mode + (uint32_t)n_in;
    for (uint32_t c = 0; c < n_ch; c++) {
        for (float &v : src[c]) {
            seed = seed * 1664525u + 1013904223u;
            v = (float)(int32_t)seed * (1.0f / 2147483648.0f);
        }
        chan[c] = src[c].data();
    }
    const uint64_t stride = jb - ja;  // (exactly: a store past a channel's run lands in the next one and fails the comparison, or past the end)
    std::vector<float> dst(stride * n_ch, -77.0f);
    BandJob job{};
    job.chan = chan.data();
    job.dst = dst.data();
    job.ja = ja;
    job.jb = jb;
    job.n_in = n_in;
    job.ch_stride = stride;
    job.n_ch = n_ch;
    job.n_tiles = (uint32_t)band_n_tiles(ja, jb);
    const uint32_t blocks = job.n_tiles * n_ch;
    for (uint32_t b = 0; b < blocks; b++) run_block(job, b, row.data(), taps);
    n_blocks_run += blocks;
    std::vector<float> want(jb - ja);
    for (uint32_t c = 0; c < n_ch; c++) {
        CHECK(th_band_f32(src[c].data(), n_in, row.data(), K, ja, want.size(), want.data()));
        if (std::memcmp(want.data(), dst.data() + c * stride, want.size() * sizeof(float)) != 0) {
            std::fprintf(stderr, "MISMATCH K %u mode %u, n_in %zu, [%llu, %llu), channel %u\n", K, mode, n_in, (unsigned long long)ja,
                         (unsigned long long)jb, c);
            std::exit(1);
        }
        n_checked += want.size();
    }
    std::printf("ok K %5u mode %u [%6.0f, %6.0f] Hz  n_in %6zu  [%llu, %llu) x %u ch\n", K, mode, f_lo, f_hi, n_in, (unsigned long long)ja,
                (unsigned long long)jb, n_ch);
}

int main() {
    // the K values and track lengths of tests/test_gpu_band.py: 2K = 0 and 2 mod 4, a row shorter than, equal to and just longer than
    // the tap block, several blocks; pass, stop, low-pass, high-pass
    const uint32_t Ks[] = {1, 31, 32, 33, 64, 65, 66, 256, 1024};
    const uint64_t tile = BAND_TILE;
    for (uint32_t K : Ks) {
        const size_t taps = 2 * (size_t)K;
        const uint32_t mode = K & 1u;
        const double f_lo = K % 3 == 0 ? 0.0 : 1000.0, f_hi = K % 3 == 1 ? 4000.0 : 2500.0;
        for (size_t n_in : {(size_t)1, (size_t)100, taps - 1, taps + 1, (size_t)tile - 1, (size_t)tile + 1, 2 * (size_t)tile + 1})
            if (n_in) run_case(K, mode, f_lo, f_hi, n_in, 0, UINT64_MAX, 1);
        const size_t n_in = 2 * tile + taps + 3;
        run_case(K, mode ^ 1u, f_lo, f_hi, n_in, 1, UINT64_MAX, 2);
        run_case(K, mode, f_lo, f_hi, n_in, tile - 1, tile + 70, 3);
        run_case(K, mode, f_lo, f_hi, n_in, tile + 1, 2 * tile - 1, 1);
        run_case(K, mode, f_lo, f_hi, n_in, 4, 9, 2);
    }
    std::printf("san_band: %zu outputs of %zu workgroups bit-identical to th_band_f32\n", n_checked, n_blocks_run);
    return 0;
}
