// san_formant.cpp — the formant kernel's source run on the CPU, a workgroup's threads one after the other between the kernel's
// barriers (thesia_amd/csrc/formant_block.h is what kernels_formant.hip calls), under AddressSanitizer and UBSan: the staged frame,
// the partial sums, the lags, the coefficients, the roots, the window and start tables, the analysis signal (for a resampled shape:
// exactly the hull of the run, as the slot's scratch holds it) and the records each have exactly the size the host side gives them,
// so a read or write out of bounds is reported; every frame's packed doubles are compared bit for bit with th_formants_f64.  Then
// plan_formants / bind_formants on adversarial batches (cut by the frame bound, by the scratch bound, by a change of rate pair): every
// piece within its bounds, records and scratch runs that never overlap, hulls that hold every sample the kernel reads, tables inside
// the table.  Not a pytest test and never loaded into python.  From the repository root (one line):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined scripts/san_formant.cpp
//       thesia_amd/csrc/formant_plan.cpp thesia_amd/csrc/host_math.cpp -Lthesia_amd -lthesia_amd
//       -Wl,-rpath,$PWD/thesia_amd -o build/san_formant && build/san_formant
// (the library is linked for th_resample_f32 alone; everything under test is compiled here)
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../thesia_amd/csrc/common.h"
#include "../thesia_amd/csrc/formant_block.h"

using namespace th;

namespace th {  // (the library keeps these to itself)
static thread_local char last_error[512];
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}
const char *get_error() { return last_error; }
}  // namespace th

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            std::exit(2);                                                             \
        }                                                                             \
    } while (0)
#define CHECK(call)                                                      \
    do {                                                                 \
        if ((call) != TH_OK) {                                           \
            std::fprintf(stderr, "%s failed: %s\n", #call, get_error()); \
            std::exit(2);                                                \
        }                                                                \
    } while (0)

static size_t n_frames_checked = 0;

static th_formant_request request(uint32_t sr_a, uint32_t p, uint32_t W, uint32_t H, uint32_t window, double pre, uint32_t kind, uint32_t rate) {
    th_formant_request r{};
    r.start_sec = 0.0;
    r.end_sec = INFINITY;
    r.sr_analysis = sr_a;
    r.n_poles = p;
    r.win_sec = (double)W / rate;
    r.step_sec = (double)H / rate;
    r.preemph_hz = pre;
    r.window = window;
    r.kind = kind;
    return r;
}

// one run of frames [f0, f1) of a channel through the kernel's body, every array of its exact size
static void run_case(uint32_t sr, uint32_t sr_a, size_t n, uint32_t p, uint32_t W, uint32_t H, uint32_t window, double pre, uint32_t kind,
                     int poison) {
    const uint32_t rate = sr_a ? sr_a : sr;
    const th_formant_request req = request(sr_a, p, W, H, window, pre, kind, rate);
    th_formant_plan pl;
    EXPECT(formant_plan_for(sr, n, req, &pl) == 0);
    EXPECT(pl.win == W && pl.hop == H);
    std::vector<float> x(n);
    uint32_t seed = 777u + p + 3u * W + (uint32_t)n;
    for (size_t i = 0; i < n; i++) {
        seed = seed * 1664525u + 1013904223u;
        x[i] = 0.3f * std::sin(0.37f * (float)i) + 0.1f * (float)(int32_t)seed * (1.0f / 2147483648.0f);
    }
    if (poison == 1 && n > 5) x[n / 2] = NAN;
    if (poison == 2) std::fill(x.begin(), x.end(), 0.0f);
    const uint64_t F = pl.n_frames_total;
    // three runs: the first third, the middle, the rest: a run's signal is its own hull
    const uint64_t cuts[4] = {0, F / 3, F / 3 + (F - F / 3) / 2, F};
    std::vector<double> want(F * (2 + p));
    uint64_t want_counts[2];
    CHECK(th_formants_f64(x.data(), n, sr, &req, 0, F, want.data(), want_counts));
    uint64_t counts[2] = {0, 0};
    std::unique_ptr<double[]> win(new double[W]), start(new double[2 * p]);
    formant_window(window, W, win.get());
    formant_start_points(p, start.get());
    for (int c = 0; c < 3; c++) {
        const uint64_t f0 = cuts[c], f1 = cuts[c + 1];
        if (f1 <= f0) continue;
        uint64_t h0 = 0, h1 = n;
        std::unique_ptr<float[]> hull;
        const float *u = x.data();
        if (pl.resampled) {
            formant_hull(pl, f0, f1, &h0, &h1);
            hull.reset(new float[h1 - h0]);
            CHECK(th_resample_f32(x.data(), n, sr, rate, h0, h1 - h0, hull.get()));
            u = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(hull.get()) - (uintptr_t)h0 * sizeof(float));
        }
        const uint32_t stride = formant_rec_doubles(p);
        std::unique_ptr<double[]> rec(new double[(f1 - f0) * stride]);
        FormantJob job{};
        job.u = u;
        job.rec = rec.get();
        job.win = win.get();
        job.start = start.get();
        job.n_a = pl.n_analysis;
        job.f0 = f0;
        job.alpha = pl.alpha;
        job.n_frames = (uint32_t)(f1 - f0);
        job.W = W;
        job.H = H;
        job.p = p;
        job.kind = kind;
        // exact sizes: a read or write past any of the workgroup's arrays is reported
        std::unique_ptr<double[]> s(new double[W]), part(new double[(p + 1) * FORMANT_PART_PITCH]), r(new double[p + 1]), a(new double[p + 1]),
            tmp(new double[p + 1]), zr(new double[p]), zi(new double[p]), wm(new double[p]), fit(new double[4]);
        const FormantLds l{s.get(), part.get(), r.get(), a.get(), tmp.get(), zr.get(), zi.get(), wm.get(), fit.get()};
        for (uint32_t i = 0; i < job.n_frames; i++) {
            if (p <= 16 && (i & 1))
                formant_block_serial<17>(job, i, l);  // (the launch's choice, and the wider one: the same bits)
            else
                formant_block_serial<33>(job, i, l);
        }
        for (uint32_t i = 0; i < job.n_frames; i++) {
            double out[2 + TH_FORMANT_MAX_POLES];
            formant_pack(rec.get() + (size_t)i * stride, pl, out, counts);
            if (std::memcmp(out, want.data() + (f0 + i) * (2 + p), (2 + p) * sizeof(double)) != 0) {
                std::fprintf(stderr, "MISMATCH %u -> %u Hz, n %zu, p %u, W %u, H %u, frame %llu\n", sr, rate, n, p, W, H, (unsigned long long)(f0 + i));
                std::exit(1);
            }
        }
        n_frames_checked += job.n_frames;
    }
    EXPECT(counts[0] == want_counts[0] && counts[1] == want_counts[1]);
    if (poison == 2) EXPECT(counts[0] == F);
    std::printf("ok %5u -> %5u Hz  n %6zu  p %2u  W %4u  H %4u  window %u  kind %u  %llu frames, %llu invalid\n", sr, rate, n, p, W, H, window, kind,
                (unsigned long long)F, (unsigned long long)counts[0]);
}

// ---- the planners
static float *const SCRATCH = reinterpret_cast<float *>(uintptr_t(0x7e0000000000ull));
static double *const REC[2] = {reinterpret_cast<double *>(uintptr_t(0x7d0000000000ull)), reinterpret_cast<double *>(uintptr_t(0x7c0000000000ull))};
static unsigned char *const TAB = reinterpret_cast<unsigned char *>(uintptr_t(0x7b0000000000ull));

static void check_plan(const std::vector<FormantPlanRequest> &reqs, size_t want_pieces_at_least) {
    FormantPlan p = plan_formants(reqs.data(), reqs.size());
    EXPECT(p.err == 0);
    const std::vector<unsigned char> tab = bind_formants(p, FormantBases{{REC[0], REC[1]}, SCRATCH, TAB}, reqs.data(), reqs.size());
    EXPECT(tab.size() == p.tab_bytes && p.jobs.size() == p.runs.size());
    EXPECT(p.pieces.size() >= want_pieces_at_least);
    std::vector<uint64_t> next(reqs.size());
    for (size_t i = 0; i < reqs.size(); i++) next[i] = reqs[i].pl.frame_first;
    size_t run = 0, rjob = 0;
    for (size_t k = 0; k < p.pieces.size(); k++) {
        const FormantPiece &pc = p.pieces[k];
        EXPECT(pc.run0 == run && pc.run1 > pc.run0 && pc.rjob0 == rjob);
        EXPECT(pc.n_blocks <= TH_FORMANT_PIECE_FRAMES && pc.scratch_floats <= TH_FORMANT_PIECE_SAMPLES);
        EXPECT(pc.rec_doubles <= p.rec_need && pc.scratch_floats <= p.scratch_need);
        uint32_t blocks = 0, rblocks = 0;
        uint64_t rec_at = 0, scratch_at = 0;
        for (size_t j = pc.run0; j < pc.run1; j++, run++) {
            const FormantRun &r = p.runs[j];
            const FormantJob &job = p.jobs[j];
            const th_formant_plan &pl = reqs[r.req].pl;
            EXPECT(r.f0 == next[r.req] && r.n_frames >= 1 && r.f0 + r.n_frames <= pl.frame_end);  // every frame once, in order
            next[r.req] += r.n_frames;
            EXPECT(job.first_block == blocks && job.n_frames == r.n_frames && job.f0 == r.f0 && job.W == pl.win && job.H == pl.hop && job.p == pl.n_poles);
            EXPECT(job.W <= pc.max_W && job.p <= pc.max_p);
            blocks += r.n_frames;
            EXPECT(r.rec_at == rec_at && job.rec == REC[k & 1] + rec_at);  // records back to back: no overlap
            rec_at += (uint64_t)r.n_frames * formant_rec_doubles(pl.n_poles);
            EXPECT((size_t)((const unsigned char *)job.win - TAB) + pl.win * sizeof(double) <= p.o_jobs);
            EXPECT((size_t)((const unsigned char *)job.start - TAB) + 2 * pl.n_poles * sizeof(double) <= p.o_jobs);
            // what the kernel reads of the analysis signal: [b - 1, b + W) of every frame, inside [0, n_a)
            const int64_t lo = (int64_t)(r.f0 * pl.hop) - (int64_t)(pl.win / 2) - 1;
            const int64_t hi = (int64_t)((r.f0 + r.n_frames - 1) * pl.hop) - (int64_t)(pl.win / 2) + (int64_t)pl.win;
            const uint64_t need0 = lo > 0 ? (uint64_t)lo : 0, need1 = std::min<uint64_t>((uint64_t)hi, pl.n_analysis);
            EXPECT(r.hull0 <= need0 && need1 <= r.hull1 && r.hull1 <= pl.n_analysis);
            if (pl.resampled) {
                EXPECT(r.rjob == (int32_t)rjob && pc.sr_in == pl.sr && pc.sr_out == pl.sr_analysis);
                const ResampleJob &rj = p.rjobs[rjob++];
                EXPECT(rj.ja == r.hull0 && rj.jb == r.hull1 && rj.n_ch == 1 && rj.n_in == reqs[r.req].n_in && rj.ch_stride == r.hull1 - r.hull0);
                EXPECT(rj.first_block == rblocks && rj.dst == SCRATCH + r.scratch_at && r.scratch_at >= scratch_at);
                EXPECT((const unsigned char *)rj.chan == TAB + p.o_ptrs + r.req * sizeof(const float *));
                const ResampleTiling t = resample_tiling(pl.rs);
                EXPECT(rj.n_sb == resample_n_sb(rj.ja, rj.jb, t));
                rblocks += rj.n_sb * t.S;
                scratch_at = r.scratch_at + (r.hull1 - r.hull0);
                EXPECT(scratch_at <= pc.scratch_floats);
                EXPECT(job.u + r.hull0 == SCRATCH + r.scratch_at);
            } else {
                EXPECT(r.rjob == -1 && job.u == reqs[r.req].src);
            }
        }
        EXPECT(blocks == pc.n_blocks && rblocks == pc.n_rblocks && rec_at == pc.rec_doubles && pc.rjob1 == rjob);
    }
    EXPECT(run == p.runs.size() && rjob == p.rjobs.size());
    for (size_t i = 0; i < reqs.size(); i++) EXPECT(next[i] == reqs[i].pl.frame_end);
    std::printf("ok plan: %zu requests, %zu runs in %zu pieces, %zu resampler jobs, table %zu bytes\n", reqs.size(), p.runs.size(), p.pieces.size(),
                p.rjobs.size(), p.tab_bytes);
}

static FormantPlanRequest planned(uint32_t sr, uint64_t n, uint32_t sr_a, uint32_t p, uint32_t W, uint32_t H, double a = 0.0, double b = INFINITY) {
    th_formant_request r = request(sr_a, p, W, H, 0, 50.0, 0, sr_a ? sr_a : sr);
    r.start_sec = a;
    r.end_sec = b;
    FormantPlanRequest pr{};
    pr.src = reinterpret_cast<const float *>(uintptr_t(0x7f0000000000ull) + (uintptr_t)n * 4);
    pr.n_in = n;
    EXPECT(formant_plan_for(sr, n, r, &pr.pl) == 0);
    return pr;
}

int main() {
    // the shapes of tests/test_gpu_formant.py, then more lengths around the window, a NaN and silence
    const double INF = INFINITY;
    run_case(8000, 0, 300, 2, 4, 1, 0, 50.0, 0, 0);
    run_case(8000, 0, 1, 2, 4, 7, 1, INF, 0, 0);
    run_case(8000, 0, 62, 10, 63, 7, 0, 50.0, 0, 0);
    run_case(8000, 0, 63, 10, 63, 63, 1, 50.0, 1, 0);
    run_case(8000, 0, 64, 10, 63, 126, 0, INF, 0, 0);
    run_case(8000, 0, 900, 16, 64, 7, 0, 50.0, 0, 0);
    run_case(8000, 0, 900, 16, 65, 65, 1, INF, 1, 0);
    run_case(8000, 0, 2000, 32, 129, 7, 0, 50.0, 0, 0);
    run_case(8000, 0, 3000, 32, 34, 68, 0, 50.0, 0, 0);
    run_case(8000, 0, 9000, 10, 4096, 4096, 0, 50.0, 0, 0);
    run_case(8000, 0, 4097, 32, 4096, 8192, 1, INF, 0, 0);
    run_case(44100, 11000, 22050, 10, 550, 138, 0, 50.0, 0, 0);
    run_case(48000, 11000, 4800, 10, 550, 1, 0, 50.0, 1, 0);
    run_case(48000, 11000, 24000, 16, 129, 258, 1, INF, 0, 0);
    run_case(44100, 11000, 5000, 2, 63, 63, 1, 50.0, 0, 0);
    for (size_t n : {(size_t)128, (size_t)129, (size_t)130, (size_t)257}) run_case(8000, 0, n, 10, 129, 129, 0, 50.0, 0, 0);
    run_case(8000, 0, 1500, 6, 65, 20, 0, 50.0, 0, 1);
    run_case(8000, 0, 1500, 6, 65, 20, 0, INF, 1, 1);
    run_case(8000, 0, 1500, 6, 65, 20, 0, 50.0, 0, 2);
    run_case(44100, 11000, 6000, 6, 65, 20, 0, 50.0, 0, 1);

    // the planners: one request, a request just over two pieces, a batch cut by the frame bound in the middle of a request, a long
    // resampled track cut by the scratch bound, two rate pairs, hops far above the window, empty ranges
    check_plan({planned(8000, 900, 0, 16, 64, 7)}, 1);
    check_plan({planned(8000, 2 * TH_FORMANT_PIECE_FRAMES + 5, 0, 2, 4, 1)}, 3);
    check_plan({planned(8000, 20000, 0, 2, 4, 1), planned(48000, 480000, 11000, 10, 550, 138), planned(8000, 20000, 0, 32, 129, 2)}, 2);
    check_plan({planned(48000, (uint64_t)48000 * 1200, 11000, 10, 550, 138), planned(8000, 9000, 0, 10, 4096, 4096)}, 4);
    check_plan({planned(48000, 480000, 11000, 10, 550, 138), planned(44100, 441000, 11000, 10, 550, 138), planned(48000, 48000, 11000, 4, 63, 1)}, 3);
    check_plan({planned(48000, (uint64_t)48000 * 3600, 8000, 4, 4096, 65536), planned(48000, 4800, 11000, 10, 550, 138, 0.2, 0.2)}, 1);
    check_plan({planned(8000, 9000, 0, 10, 100, 50, 0.5, 0.5), planned(8000, 1, 0, 2, 4, 7)}, 1);
    std::printf("san_formant: %zu frames bit-identical to th_formants_f64\n", n_frames_checked);
    return 0;
}
