// formant_block.h — the body of the formant kernel (kernels_formant.hip) as phase functions over (thread id, LDS arrays), host +
// device: the kernel calls them between its barriers, th_formants_f64 runs the same ones thread after thread (formant_plan.cpp), and
// so does a stand-alone program under AddressSanitizer and UBSan with arrays of the exact sizes (scripts/san_formant.cpp).
// A workgroup is one wave and takes one frame: the wave stages the windowed frame s in LDS as f64, lane q is partial sum q of every
// lag (s[k + m] is consecutive across the lanes: no bank conflict), lane m folds lag m's 64 partial sums, lane 0 runs Levinson,
// lane i is root i of the Aberth sweeps (the old roots are read from LDS by every lane), and the stop test is the same loop in every lane.
#pragma once
#include "formant_core.h"
#include "formant_plan.h"

namespace th {

// the arrays of a workgroup (LDS on the device; formant_lds_doubles is their sum)
struct FormantLds {
    double *s;     // W
    double *part;  // (p + 1) x FORMANT_PART_PITCH
    double *r;     // p + 1
    double *a;     // p + 1
    double *tmp;   // p + 1
    double *zr;    // p
    double *zi;    // p
    double *wm;    // p
    double *fit;   // 4: status, sweeps, r0', E
};
TH_HD FormantLds formant_carve(double *base, uint32_t W, uint32_t p) {
    FormantLds l;
    l.s = base;
    l.part = l.s + W;
    l.r = l.part + (p + 1) * FORMANT_PART_PITCH;
    l.a = l.r + (p + 1);
    l.tmp = l.a + (p + 1);
    l.zr = l.tmp + (p + 1);
    l.zi = l.zr + p;
    l.wm = l.zi + p;
    l.fit = l.wm + p;
    return l;
}

// step 1: frame f's windowed samples
TH_HD void formant_stage(const FormantJob &job, uint64_t f, uint32_t tid, const FormantLds &l) {
    const int64_t b = (int64_t)(f * job.H) - (int64_t)(job.W / 2);
    const gptr<const double> g = as_global(job.win);
    for (uint32_t k = tid; k < job.W; k += FORMANT_LANES) l.s[k] = formant_d(job.u, b + (int64_t)k, job.n_a, job.alpha) * g[k];
}

// step 2: the lane's partial sums
template <uint32_t NL>
TH_HD void formant_autocorr(const FormantJob &job, uint32_t tid, const FormantLds &l) {
    formant_autocorr_lane<NL>(l.s, job.W, job.p, tid, l.part);
}

// ... lane m folds lag m
TH_HD void formant_reduce(const FormantJob &job, uint32_t tid, const FormantLds &l) {
    if (tid <= job.p) l.r[tid] = formant_tree(l.part + tid * FORMANT_PART_PITCH);
}

// steps 3 and 4 in lane 0; the other lanes set the roots to zero
TH_HD void formant_fit(const FormantJob &job, uint32_t tid, const FormantLds &l) {
    if (tid == 0) {
        double r0p, E;
        const uint32_t st = formant_levinson(l.r, job.p, l.a, l.tmp, &r0p, &E);
        l.fit[0] = (double)st;
        l.fit[1] = 0.0;
        l.fit[2] = r0p;
        l.fit[3] = E;
    } else if (tid <= job.p) {
        l.zr[tid - 1] = 0.0;
        l.zi[tid - 1] = 0.0;
    }
}
// whether step 5 runs (after formant_fit and a barrier; the same in every lane)
TH_HD bool formant_wants_roots(const FormantJob &job, const FormantLds &l) { return l.fit[0] == 0.0 && job.kind == TH_FORMANT_OUT_FORMANTS; }
TH_HD void formant_roots_start(const FormantJob &job, uint32_t tid, const FormantLds &l) {
    if (tid >= job.p) return;
    const gptr<const double> z0 = as_global(job.start);
    l.zr[tid] = z0[tid];
    l.zi[tid] = z0[job.p + tid];
}
// one sweep in two phases with a barrier between them: the corrections from the old roots, then the new roots
TH_HD fm_c formant_sweep_w(const FormantJob &job, uint32_t tid, const FormantLds &l) {
    if (tid >= job.p) return fm_c{0.0, 0.0};
    return formant_aberth_w(l.a, job.p, l.zr, l.zi, tid);
}
TH_HD void formant_sweep_move(const FormantJob &job, uint32_t tid, const FormantLds &l, fm_c w) {
    if (tid >= job.p) return;
    l.zr[tid] = l.zr[tid] - w.r;
    l.zi[tid] = l.zi[tid] - w.i;
    l.wm[tid] = formant_w_mag(w);
}
// after a sweep and a barrier: whether it was the last, the same in every lane
TH_HD bool formant_sweep_done(const FormantJob &job, const FormantLds &l) { return formant_stop(l.wm, job.p); }
// lane 0 notes how the sweeps ended (before the barrier in front of formant_store)
TH_HD void formant_roots_end(uint32_t tid, const FormantLds &l, uint32_t sweeps, bool stopped) {
    if (tid != 0) return;
    l.fit[1] = (double)sweeps;
    if (!stopped) l.fit[0] = 2.0;
}

// the raw record of frame i of the run
TH_HD void formant_store(const FormantJob &job, uint32_t i, uint32_t tid, const FormantLds &l) {
    if (i >= job.n_frames) return;
    const gptr<double> rec = as_global(job.rec) + (uint64_t)i * (4 + 3 * job.p);
    if (tid < 4) rec[tid] = l.fit[tid];
    if (tid < job.p) {
        rec[4 + tid] = l.a[1 + tid];
        rec[4 + job.p + tid] = l.zr[tid];
        rec[4 + 2 * job.p + tid] = l.zi[tid];
    }
}

// A whole frame, a workgroup's threads one after the other between the kernel's barriers: what th_formants_f64 and the stand-alone
// checker run.  The kernel's body is this sequence with tid = threadIdx.x and a barrier where a loop over the threads ends here
template <uint32_t NL>
inline void formant_block_serial(const FormantJob &job, uint32_t i, const FormantLds &l) {
    const uint64_t f = job.f0 + i;
    for (uint32_t t = 0; t < FORMANT_LANES; t++) formant_stage(job, f, t, l);
    for (uint32_t t = 0; t < FORMANT_LANES; t++) formant_autocorr<NL>(job, t, l);
    for (uint32_t t = 0; t < FORMANT_LANES; t++) formant_reduce(job, t, l);
    for (uint32_t t = 0; t < FORMANT_LANES; t++) formant_fit(job, t, l);
    if (formant_wants_roots(job, l)) {
        for (uint32_t t = 0; t < FORMANT_LANES; t++) formant_roots_start(job, t, l);
        uint32_t sweeps = 0;
        bool stopped = false;
        fm_c w[FORMANT_LANES];
        while (sweeps < TH_FORMANT_MAX_SWEEPS && !stopped) {
            for (uint32_t t = 0; t < FORMANT_LANES; t++) w[t] = formant_sweep_w(job, t, l);
            for (uint32_t t = 0; t < FORMANT_LANES; t++) formant_sweep_move(job, t, l, w[t]);
            sweeps++;
            stopped = formant_sweep_done(job, l);
        }
        for (uint32_t t = 0; t < FORMANT_LANES; t++) formant_roots_end(t, l, sweeps, stopped);
    }
    for (uint32_t t = 0; t < FORMANT_LANES; t++) formant_store(job, i, t, l);
}

}  // namespace th
