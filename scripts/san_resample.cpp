// san_resample.cpp — the resample kernel's source run on the CPU, a workgroup's threads one after the other between the kernel's
// barriers (thesia_amd/csrc/resample_block.h is what kernels_resample.hip calls), under AddressSanitizer and UBSan: every staged
// array, table, source and destination has exactly the size the host side gives it, so a read or write out of bounds is reported;
// every output is compared bit for bit with th_resample_f32.  Not a pytest test and never loaded into python.  From the repository root:
//   hipcc -x hip --cuda-host-only -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         scripts/san_resample.cpp -Lthesia_amd -lthesia_amd -Wl,-rpath,$PWD/thesia_amd -o build/san_resample && build/san_resample
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../thesia_amd/csrc/resample_block.h"

using namespace th;

#define CHECK(call)                                                        \
    do {                                                                   \
        if ((call) != TH_OK) {                                             \
            std::fprintf(stderr, "%s failed: %s\n", #call, th_last_error()); \
            std::exit(2);                                                  \
        }                                                                  \
    } while (0)

struct Aligned {  // n floats on a 16-byte boundary, not one more
    float *p = nullptr;
    explicit Aligned(size_t n) {
        void *v = nullptr;
        if (posix_memalign(&v, 16, n * sizeof(float)) != 0) std::exit(3);
        p = static_cast<float *>(v);
    }
    Aligned(const Aligned &) = delete;
    ~Aligned() { std::free(p); }
    float *get() const { return p; }
};

template <uint32_t PT>
static void run_block(const ResampleJob &job, const ResampleTiling &tl, uint32_t b, const float *table) {
    const ResampleBlock k = resample_block_of(job, tl, b);
    if (!k.any) return;
    const uint32_t n_thr = 64 * tl.G;
    // exact sizes: xb's last element is never written or read; the arrays are 16-byte aligned as the kernel's are
    Aligned xa(tl.span), xb(tl.span), cs(RESAMPLE_LANES * RESAMPLE_CS_PITCH);
    uint32_t rows[RESAMPLE_LANES];
    std::vector<ResampleLane<PT>> ln(n_thr);
    for (uint32_t t = 0; t < n_thr; t++) {
        resample_lane_setup<PT>(job, tl, k, t, ln[t]);
        if (t < RESAMPLE_LANES) rows[t] = ln[t].row;
    }
    for (uint32_t kb = 0; kb < tl.taps; kb += RESAMPLE_TAP_BLOCK) {
        const uint32_t nt = tl.taps - kb < RESAMPLE_TAP_BLOCK ? tl.taps - kb : RESAMPLE_TAP_BLOCK;
        for (uint32_t t = 0; t < n_thr; t++) resample_stage(job, tl, k, table, rows, kb, nt, t, n_thr, xa.get(), xb.get(), cs.get());
        for (uint32_t t = 0; t < n_thr; t++) resample_accumulate<PT>(ln[t], nt, cs.get() + (t & 63u) * RESAMPLE_CS_PITCH, xa.get(), xb.get());
    }
    for (uint32_t t = 0; t < n_thr; t++) resample_store<PT>(job, tl, k, ln[t]);
}

static size_t n_checked = 0, n_blocks_run = 0;

static void run_case(uint32_t sr_in, uint32_t sr_out, size_t n_in, uint64_t ja, uint64_t jb_want, uint32_t n_ch) {
    th_resample_plan plan;
    CHECK(th_resample_plan_for(sr_in, sr_out, &plan));
    size_t n_out = 0;
    CHECK(th_resample_n_out(n_in, sr_in, sr_out, &n_out));
    const uint64_t jb = jb_want < n_out ? jb_want : n_out;
    if (ja >= jb) return;
    const ResampleTiling tl = resample_tiling(plan);
    std::vector<float> table((size_t)plan.L * tl.taps);
    for (uint32_t r = 0; r < plan.L; r++) CHECK(th_resample_coefs(sr_in, sr_out, r, nullptr, table.data() + (size_t)r * tl.taps));
    std::vector<std::vector<float>> src(n_ch, std::vector<float>(n_in));
    std::vector<const float *> chan(n_ch);
    uint32_t seed = 12345u + sr_in + 7u * sr_out + (uint32_t)n_in;
    for (uint32_t c = 0; c < n_ch; c++) {
        for (float &v : src[c]) {
            seed = seed * 1664525u + 1013904223u;
            v = (float)(int32_t)seed * (1.0f / 2147483648.0f);
        }
        chan[c] = src[c].data();
    }
    const uint64_t stride = jb - ja;  // (exactly: a store past a channel's run lands in the next one and fails the comparison, or past the end)
    std::vector<float> dst(stride * n_ch, -77.0f);
    ResampleJob job{};
    job.chan = chan.data();
    job.dst = dst.data();
    job.ja = ja;
    job.jb = jb;
    job.n_in = n_in;
    job.ch_stride = stride;
    job.n_ch = n_ch;
    job.n_sb = (uint32_t)resample_n_sb(ja, jb, tl);
    const uint32_t blocks = job.n_sb * n_ch * tl.S;
    for (uint32_t b = 0; b < blocks; b++) {
        switch (tl.Pt) {
            case 8: run_block<8>(job, tl, b, table.data()); break;
            case 4: run_block<4>(job, tl, b, table.data()); break;
            case 2: run_block<2>(job, tl, b, table.data()); break;
            default: run_block<1>(job, tl, b, table.data()); break;
        }
    }
    n_blocks_run += blocks;
    std::vector<float> want(jb - ja);
    for (uint32_t c = 0; c < n_ch; c++) {
        CHECK(th_resample_f32(src[c].data(), n_in, sr_in, sr_out, ja, want.size(), want.data()));
        if (std::memcmp(want.data(), dst.data() + c * stride, want.size() * sizeof(float)) != 0) {
            std::fprintf(stderr, "MISMATCH %u -> %u, n_in %zu, [%llu, %llu), channel %u\n", sr_in, sr_out, n_in, (unsigned long long)ja,
                         (unsigned long long)jb, c);
            std::exit(1);
        }
        n_checked += want.size();
    }
    std::printf("ok %6u -> %6u  n_in %7zu  [%llu, %llu) x %u ch  G %u Pt %u R %u S %u span %u taps %u\n", sr_in, sr_out, n_in, (unsigned long long)ja,
                (unsigned long long)jb, n_ch, tl.G, tl.Pt, tl.R, tl.S, tl.span, tl.taps);
}

int main() {
    // the seven pairs of the tests, and one pair for each remaining shape of the tiling: {4, 2}, {4, 1}, {1, 2}
    const uint32_t pairs[][2] = {{44100, 48000}, {48000, 44100}, {48000, 96000}, {96000, 48000}, {8000, 48000}, {48000, 16000}, {8000, 8001},
                                 {64000, 8000},  {128000, 8000}, {192000, 8000}};
    for (const auto &pr : pairs) {
        th_resample_plan plan;
        CHECK(th_resample_plan_for(pr[0], pr[1], &plan));
        const ResampleTiling tl = resample_tiling(plan);
        const size_t taps = tl.taps, PM = (size_t)tl.G * tl.Pt * tl.Mp;
        const uint64_t tile = (uint64_t)tl.G * tl.Pt * tl.Lp;
        const bool big = plan.L > 4096;  // (8000 -> 8001: the blocks are many and small)
        for (size_t n_in : {(size_t)1, (size_t)100, taps - 1, taps, taps + 1, PM - 1, PM + 1, 2 * PM + 1}) {
            if (big && n_in > 9000) n_in = 9000;
            run_case(pr[0], pr[1], n_in, 0, UINT64_MAX, 1);
        }
        const size_t n_in = big ? 9000 : 2 * PM + taps + 3;
        run_case(pr[0], pr[1], n_in, 1, UINT64_MAX, 2);
        run_case(pr[0], pr[1], n_in, tile - 1, tile + 70, 3);
        run_case(pr[0], pr[1], n_in, tile + 1, 2 * tile - 1, 1);
        run_case(pr[0], pr[1], n_in, 4, 9, 2);
    }
    std::printf("san_resample: %zu outputs of %zu workgroups bit-identical to th_resample_f32\n", n_checked, n_blocks_run);
    return 0;
}
