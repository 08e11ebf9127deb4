// formant_plan.h — the host side of the formant reader (include/thesia_amd.h "Formant candidates") as plain data, no HIP: the job
// of kernels_formant.hip, the plan of one request (formant_plan_for: the one place where numbers are made from seconds), the host
// tables, the cut of a call into pieces, and the host's step 6 and packing of a raw record.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/thesia_amd.h"
#include "reader_plan.h"  // ResampleJob, ResampleTiling

namespace th {

// ---- kernels_formant.hip: a workgroup of one wave takes ONE frame of one run.  A run is frames [f0, f0 + n_frames) of one request.
// The raw record of a frame is 4 + 3 p doubles: status (0 valid, 1 invalid, 2 unconverged), sweeps, r0', E, a_1 .. a_p, p real
// parts, p imaginary parts (zero where step 5 did not run)
struct FormantJob {
    const float *u;       // analysis sample n is u[n], for every n of [0, n_a) that the run's windows and their left neighbours meet
    double *rec;          // the run's first record
    const double *win;    // g[W]
    const double *start;  // 2 p start points: real parts, then imaginary parts
    uint64_t n_a;
    uint64_t f0;
    double alpha;
    uint32_t n_frames;
    uint32_t first_block;  // blocks [first_block, first_block + n_frames) of the grid are this run's
    uint32_t W, H, p, kind;
};
static_assert(sizeof(FormantJob) == 80, "FormantJob must have no implicit padding");
inline uint32_t formant_rec_doubles(uint32_t p) { return 4 + 3 * p; }
// dynamic LDS of a workgroup, in doubles: s[W], part[(p + 1) 65], r[p + 1], a[p + 1], tmp[p + 1], zr[p], zi[p], wm[p], fit[4]
inline uint32_t formant_lds_doubles(uint32_t W, uint32_t p) { return W + (p + 1) * 65 + 3 * (p + 1) + 3 * p + 4; }

// ---- one request's plan.  0; 1: TH_ERR_INVALID_ARG; 2: TH_ERR_UNSUPPORTED (the rate pair or the track's length at sr_a)
int formant_plan_for(uint32_t sr, size_t n_samples, const th_formant_request &req, th_formant_plan *plan);
void formant_window(uint32_t window, uint32_t W, double *g);
void formant_start_points(uint32_t p, double *z);
// first sample and length of the analysis signal that frames [f0, f1) read (the windows and one sample to the left, inside [0, n_a))
void formant_hull(const th_formant_plan &pl, uint64_t f0, uint64_t f1, uint64_t *h0, uint64_t *h1);

// ---- the host's half of a frame: step 6 and the packing.  rec: a raw record; out: 2 + p doubles; counts[0] += invalid, counts[1] +=
// unconverged
void formant_pack(const double *rec, const th_formant_plan &pl, double *out, uint64_t *counts);
// frame f of the analysis signal u (as FormantJob::u) into a raw record, through the kernel's own phase functions (formant_block.h);
// r (p + 1, may be NULL) receives the lags
void formant_frame_host(const float *u, const th_formant_plan &pl, const double *win, const double *start, uint64_t f, double *rec, double *r);

// ---- the cut of a call.  A request that was planned, and where its doubles go
struct FormantPlanRequest {
    const float *src;  // the resident channel (device memory), n_in samples at pl.sr
    uint64_t n_in;
    th_formant_plan pl;
    uint64_t offset;   // into out, doubles
};
struct FormantRun {
    size_t req;
    uint64_t f0;
    uint32_t n_frames;
    uint64_t rec_at;      // doubles into the piece's record buffer
    uint64_t hull0, hull1;
    uint64_t scratch_at;  // floats into the slot's scratch (resampled runs)
    int32_t rjob;         // index into rjobs, or -1
};
struct FormantPiece {
    size_t run0 = 0, run1 = 0, rjob0 = 0, rjob1 = 0;
    uint32_t n_blocks = 0, n_rblocks = 0;
    uint32_t max_p = 0, max_W = 0;
    uint32_t sr_in = 0, sr_out = 0;  // the piece's rate pair (0: nothing resampled)
    th_resample_plan rs{};
    uint64_t rec_doubles = 0, scratch_floats = 0;
};
struct FormantTab {  // where a request's tables lie in the call's table (bytes)
    size_t win_at, start_at;
};
struct FormantPlan {
    int err = 0;
    std::string err_text;
    std::vector<FormantRun> runs;
    std::vector<FormantPiece> pieces;
    std::vector<FormantJob> jobs;      // jobs[k]: of runs[k]
    std::vector<ResampleJob> rjobs;
    std::vector<FormantTab> tabs;      // per request
    size_t o_jobs = 0, o_rjobs = 0, o_ptrs = 0, tab_bytes = 0;  // the table: windows and start points, jobs, resampler jobs, channel pointers
    uint64_t rec_need = 0, scratch_need = 0;
};
FormantPlan plan_formants(const FormantPlanRequest *reqs, size_t n);
struct FormantBases {
    double *rec[2];
    float *scratch;
    unsigned char *tab;  // the device address of the table
};
// the addresses into the jobs, and the table's bytes
std::vector<unsigned char> bind_formants(FormantPlan &p, const FormantBases &b, const FormantPlanRequest *reqs, size_t n);

}  // namespace th
