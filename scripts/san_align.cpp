// san_align.cpp — the correlation kernel's source run on the CPU, a workgroup's threads one after the other between the kernel's
// barriers (thesia_amd/csrc/align_block.h is what kernels_align.hip calls), with the planner's pieces (align_plan.cpp) as the launches,
// under AddressSanitizer and UBSan: the reference range, the probe, every staged span, the scratch of group values and the record have
// exactly the size the host side gives them, so a read or write out of bounds is reported; every lag is compared bit for bit with
// th_xcorr_f64 and every energy with th_align_energy_f64.  Not a pytest test and never loaded into python.  From the repository root:
//   hipcc -x hip --cuda-host-only -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         scripts/san_align.cpp thesia_amd/csrc/align_plan.cpp thesia_amd/csrc/host_math.cpp -o build/san_align && build/san_align
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../thesia_amd/csrc/align_block.h"

using namespace th;

struct Lane {
    AlignAcc acc[ALIGN_R];
    double group[ALIGN_R];
    float pre[ALIGN_PRE];
};

// the kernel's loop: what lies between two barriers runs for every thread before anything behind the barrier does
static void run_block(const AlignJob &job, uint32_t b) {
    const AlignBlock k = align_block_of(job, b);
    if (!k.any) return;
    // exact sizes: a read or write past a staged span is reported
    std::unique_ptr<float[]> xs[2] = {std::unique_ptr<float[]>(new float[ALIGN_XS]), std::unique_ptr<float[]>(new float[ALIGN_XS])};
    std::vector<Lane> ln(ALIGN_THREADS);
    for (uint32_t t = 0; t < ALIGN_THREADS; t++) {
        for (uint32_t i = 0; i < ALIGN_R; i++) {
            align_zero(ln[t].acc[i]);
            ln[t].group[i] = 0.0;
        }
        align_fetch(job, k, k.k_first, t, ln[t].pre);
        align_commit(ln[t].pre, t, xs[0].get());
    }
    uint32_t buf = 0;
    for (uint64_t k0 = k.k_first; k0 < k.k_end; k0 += ALIGN_STEP, buf ^= 1u) {
        const bool more = k0 + ALIGN_STEP < k.k_end;
        for (uint32_t t = 0; t < ALIGN_THREADS; t++) {
            if (more) align_fetch(job, k, k0 + ALIGN_STEP, t, ln[t].pre);
            if (k.k_end - k0 >= ALIGN_STEP)
                align_accumulate<true>(ln[t].acc, job.a + k0, ALIGN_STEP, xs[buf].get(), t);
            else
                align_accumulate<false>(ln[t].acc, job.a + k0, (uint32_t)(k.k_end - k0), xs[buf].get(), t);
            if (!more || (k0 + ALIGN_STEP) % ALIGN_BLOCK == 0) align_block_end(ln[t].acc, ln[t].group);
            if (more) align_commit(ln[t].pre, t, xs[buf ^ 1u].get());
        }
    }
    for (uint32_t t = 0; t < ALIGN_THREADS; t++) align_store(job, k, t, ln[t].group);
}

static size_t n_lags_checked = 0, n_blocks_run = 0, n_energies = 0;

static std::unique_ptr<float[]> noise(size_t n, uint32_t seed) {
    std::unique_ptr<float[]> v(new float[n ? n : 1]);
    for (size_t i = 0; i < n; i++) {
        seed = seed * 1664525u + 1013904223u;
        v[i] = (float)(int32_t)seed * (1.0f / 2147483648.0f);
    }
    return v;
}

// the energy kernel's two phases for every group, folded as the host folds them
static double run_energy(const float *x, uint64_t n, int64_t first, uint64_t N) {
    const uint32_t n_groups = (uint32_t)align_n_groups(N);
    std::unique_ptr<double[]> groups(new double[n_groups ? n_groups : 1]);
    for (uint32_t g = 0; g < n_groups; g++) {
        std::unique_ptr<double[]> part(new double[ALIGN_ENERGY_THREADS]);
        for (uint32_t t = 0; t < ALIGN_ENERGY_THREADS; t++) part[t] = align_energy_thread(x, n, first, N, g, t);
        groups[g] = align_energy_group(part.get(), N, g);
    }
    return align_fold(groups.get(), n_groups, 1);
}

// reference range of N samples (allocated at exactly N), probe of n_b samples, the lags first .. first + n_lags - 1 cut by plan_align
static void run_case(uint64_t N, uint64_t n_b, int64_t first, uint64_t n_lags) {
    const std::unique_ptr<float[]> a = noise(N, 77u + (uint32_t)N), b = noise(n_b, 99u + (uint32_t)n_b + (uint32_t)n_lags);
    const AlignPieces ap = plan_align(N, n_lags);
    std::unique_ptr<double[]> scratch(new double[ap.scratch_doubles ? ap.scratch_doubles : 1]);
    std::vector<double> got(n_lags, -77.0), want(n_lags, -78.0);
    uint64_t covered = 0;
    for (const AlignPiece &pc : ap.pieces) {
        if (pc.lag0 != covered || (uint64_t)pc.n_groups * pc.n_lags > ap.scratch_doubles || pc.n_lags > ap.rec_doubles) {
            std::fprintf(stderr, "BAD PLAN N %llu lags %llu\n", (unsigned long long)N, (unsigned long long)n_lags);
            std::exit(1);
        }
        for (uint64_t i = 0; i < (uint64_t)pc.n_groups * pc.n_lags; i++) scratch[i] = -79.0;
        AlignJob job{};
        job.a = a.get();
        job.b = b.get();
        job.scratch = scratch.get();
        job.N = N;
        job.n_b = n_b;
        job.first = first + (int64_t)pc.lag0;
        job.n_lags = pc.n_lags;
        job.n_tiles = pc.n_tiles;
        job.n_groups = pc.n_groups;
        for (uint32_t blk = 0; blk < pc.n_blocks; blk++) run_block(job, blk);
        n_blocks_run += pc.n_blocks;
        std::unique_ptr<double[]> rec(new double[pc.n_lags]);  // the fold kernel: one thread per lag
        for (uint32_t i = 0; i < pc.n_lags; i++) rec[i] = align_fold(scratch.get() + i, pc.n_groups, pc.n_lags);
        std::memcpy(got.data() + pc.lag0, rec.get(), pc.n_lags * sizeof(double));
        covered += pc.n_lags;
    }
    if (covered != n_lags) {
        std::fprintf(stderr, "PLAN COVERS %llu of %llu lags\n", (unsigned long long)covered, (unsigned long long)n_lags);
        std::exit(1);
    }
    xcorr_f64(a.get(), N, b.get(), n_b, first, n_lags, want.data());
    if (n_lags && std::memcmp(got.data(), want.data(), n_lags * sizeof(double)) != 0) {
        std::fprintf(stderr, "MISMATCH N %llu, probe %llu, first %lld, %llu lags\n", (unsigned long long)N, (unsigned long long)n_b, (long long)first,
                     (unsigned long long)n_lags);
        std::exit(1);
    }
    n_lags_checked += n_lags;
    // the energies of the range and of the probe's windows at the first and the last lag
    const int64_t firsts[3] = {0, first, first + (int64_t)n_lags - 1};
    for (int e = 0; e < 3; e++) {
        const float *x = e == 0 ? a.get() : b.get();
        const uint64_t n = e == 0 ? N : n_b;
        const double ge = run_energy(x, n, firsts[e], N), we = align_energy_f64(x, n, firsts[e], N);
        if (std::memcmp(&ge, &we, sizeof ge) != 0) {
            std::fprintf(stderr, "ENERGY MISMATCH N %llu first %lld\n", (unsigned long long)N, (long long)firsts[e]);
            std::exit(1);
        }
        n_energies++;
    }
    std::printf("ok N %7llu  probe %7llu  first %6lld  %6llu lags in %zu piece(s)\n", (unsigned long long)N, (unsigned long long)n_b, (long long)first,
                (unsigned long long)n_lags, ap.pieces.size());
}

int main() {
    // the reference lengths of tests/test_align_host.py at D <= 8, with the lags leaving the probe at both ends
    const uint64_t Ns[] = {1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 131071, 131072, 131073, 2 * 131072 + 5};
    for (uint64_t N : Ns) {
        const int64_t D = N < 100000 ? 8 : 3;
        run_case(N, N + 5, 3 - D, 2 * (uint64_t)D + 1);
    }
    run_case(1000, 1003, -70, 141);   // N = 1000 at D = 70
    run_case(1000, 400, 3 - 70, 141);  // a probe shorter than the reference
    run_case(1000, 1, -70, 141);
    run_case(1000, 0, -70, 141);      // no probe at all
    run_case(1000, 5000, 501 - 70, 141);
    // lags one below, at and one above the tile, twice the tile, and a bit more
    for (uint64_t n_lags : {(uint64_t)ALIGN_TILE - 1, (uint64_t)ALIGN_TILE, (uint64_t)ALIGN_TILE + 1, 2 * (uint64_t)ALIGN_TILE, 2 * (uint64_t)ALIGN_TILE + 1})
        run_case(200, 1500, -(int64_t)(n_lags / 2), n_lags);
    run_case(4100, 3000, -40, ALIGN_TILE + 7);  // two blocks of the reference, two tiles
    run_case(70, 200000, -66000, 2 * (uint64_t)TH_ALIGN_PIECE_LAGS + 5);  // just over two pieces
    std::printf("san_align: %zu lags of %zu workgroups and %zu energies bit-identical to th_xcorr_f64 / th_align_energy_f64\n", n_lags_checked,
                n_blocks_run, n_energies);
    return 0;
}
