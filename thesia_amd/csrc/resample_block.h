// resample_block.h — the body of the resample kernel (kernels_resample.hip) as phase functions over (thread id, registers, LDS
// arrays), host + device: the kernel calls them between its barriers, and a host program can run a workgroup's threads one after the
// other through the same source (scripts/san_resample.cpp does, under AddressSanitizer and UBSan, with arrays of the exact sizes).
#pragma once
#include "kernels.h"
#include "resample_core.h"

namespace th {

constexpr uint32_t RESAMPLE_CS_PITCH = RESAMPLE_TAP_BLOCK + 4;  // floats: the 16-byte reads of 16 lanes cover the 64 banks once
typedef float rs_f2 __attribute__((ext_vector_type(2)));
#if defined(__HIP_DEVICE_COMPILE__)
typedef rs_f2 __attribute__((address_space(3))) rs_lds_f2;
#else
typedef rs_f2 rs_lds_f2;
#endif

// what a workgroup works on: channel c, lanes [0, rs) = outputs j_first .. of each of its periods
struct ResampleBlock {
    uint32_t c, rs;
    uint64_t j_first, q_min;
    bool any;  // false: no output at all (a table built by resample_n_sb has such blocks only behind a range's last sub-tile)
};

// b: the block's index within its job (n_ch x n_sb x S blocks: the sub-tile fastest, then the tile, then the channel)
TH_HD ResampleBlock resample_block_of(const ResampleJob &job, const ResampleTiling &tl, uint32_t b) {
    ResampleBlock k{};
    const uint32_t s = b % tl.S;
    b /= tl.S;
    const uint32_t sb = b % job.n_sb;
    k.c = b / job.n_sb;
    const uint32_t left = tl.Lp - s * tl.R;
    k.rs = tl.R < left ? tl.R : left;
    k.j_first = job.ja + (uint64_t)sb * (tl.G * tl.Pt) * tl.Lp + (uint64_t)s * tl.R;
    k.any = k.c < job.n_ch && k.j_first < job.jb;
    uint32_t r;
    if (k.any) resample_phase(k.j_first, tl.L, tl.M, &k.q_min, &r);
    return k;
}

template <uint32_t PT>
struct ResampleLane {
    bool on;          // this lane has an output in period 0 of its wave (else it computes on offset 0 and stores nothing)
    uint64_t j0;      // its first output; period p is j0 + p Lp
    uint32_t row;     // its coefficient row
    uint32_t off[PT]; // where period p's window starts in the staged span (+ the tap within the block)
    ResampleAcc acc[PT];
};

template <uint32_t PT>
TH_HD void resample_lane_setup(const ResampleJob &job, const ResampleTiling &tl, const ResampleBlock &k, uint32_t tid, ResampleLane<PT> &ln) {
    const uint32_t lane = tid & 63u, g = tid >> 6;
    ln.on = lane < k.rs && k.j_first + lane < job.jb;
    ln.j0 = k.j_first + lane + (uint64_t)(g * PT) * tl.Lp;
    uint64_t q;
    resample_phase(ln.on ? k.j_first + lane : k.j_first, tl.L, tl.M, &q, &ln.row);
    const uint32_t off = (uint32_t)(q - k.q_min) + (uint32_t)((g * PT) * tl.Mp);
    for (uint32_t p = 0; p < PT; p++) {
        ln.off[p] = ln.on ? off + p * (uint32_t)tl.Mp : 0u;
        ln.acc[p] = ResampleAcc{};
    }
}

// taps [kb, kb + nt) of the block's rows into cs, the input span they meet into xa and, shifted by one, xb: xb[t] = xa[t + 1]
TH_HD void resample_stage(const ResampleJob &job, const ResampleTiling &tl, const ResampleBlock &k, const float *table, const uint32_t *rows,
                          uint32_t kb, uint32_t nt, uint32_t tid, uint32_t n_thr, float *xa, float *xb, float *cs) {
    const gptr<const float> src = as_global(as_global(job.chan)[k.c]);
    const gptr<const float> tab = as_global(table);
    const int64_t x0 = (int64_t)k.q_min - (int64_t)(tl.taps / 2) + 1 + (int64_t)kb;  // the track's sample at xa[0]
    for (uint32_t t = tid; t < tl.span; t += n_thr) {
        const int64_t at = x0 + (int64_t)t;
        const float v = (at >= 0 && (uint64_t)at < job.n_in) ? src[at] : 0.0f;
        xa[t] = v;
        if (t) xb[t - 1] = v;
    }
    for (uint32_t u = tid; u < RESAMPLE_LANES * (RESAMPLE_TAP_BLOCK / 2); u += n_thr) {
        const uint32_t row = u / (RESAMPLE_TAP_BLOCK / 2), k2 = 2 * (u % (RESAMPLE_TAP_BLOCK / 2));
        rs_f2 v = {0.0f, 0.0f};
        if (k2 < nt) v = *reinterpret_cast<gptr<const rs_f2>>(tab + (uint64_t)rows[row] * tl.taps + kb + k2);  // (taps, kb, k2 are even)
        *reinterpret_cast<rs_f2 *>(cs + row * RESAMPLE_CS_PITCH + k2) = v;
    }
}

// nt taps of every period of this lane: 4 coefficients stay in registers across the periods; a window that starts at an odd sample
// is read from xb at the even index below, so every read is an aligned 8-byte one
template <uint32_t PT>
TH_HD void resample_accumulate(ResampleLane<PT> &ln, uint32_t nt, const float *cr, const float *xa, const float *xb) {
    // (volatile: two 8-byte reads stay two ds_read_b64; the paired read2 form the compiler would merge them into runs at half their rate)
    const volatile rs_lds_f2 *xp[PT];
#pragma unroll
    for (uint32_t p = 0; p < PT; p++) {
        const uint32_t o = ln.off[p];
        xp[p] = (const volatile rs_lds_f2 *)((o & 1u) ? xb + (o - 1u) : xa + o);
    }
    uint32_t kk = 0;
#pragma unroll 4
    for (; kk + 4 <= nt; kk += 4) {
        const float4 cf = *reinterpret_cast<const float4 *>(cr + kk);
#pragma unroll
        for (uint32_t p = 0; p < PT; p++) {
            const rs_f2 u0 = xp[p][kk / 2], u1 = xp[p][kk / 2 + 1];
            resample_tap4(ln.acc[p], cf.x, cf.y, cf.z, cf.w, u0.x, u0.y, u1.x, u1.y);
        }
    }
    if (kk < nt) {  // (2K = 2 mod 4: the row's last two taps)
        const rs_f2 cf = *reinterpret_cast<const rs_f2 *>(cr + kk);
#pragma unroll
        for (uint32_t p = 0; p < PT; p++) {
            const rs_f2 u0 = xp[p][kk / 2];
            resample_tap2(ln.acc[p], cf.x, cf.y, u0.x, u0.y);
        }
    }
}

template <uint32_t PT>
TH_HD void resample_store(const ResampleJob &job, const ResampleTiling &tl, const ResampleBlock &k, const ResampleLane<PT> &ln) {
    if (!ln.on) return;
    const gptr<float> dst = as_global(job.dst) + (uint64_t)k.c * job.ch_stride;
#pragma unroll
    for (uint32_t p = 0; p < PT; p++) {
        const uint64_t j = ln.j0 + (uint64_t)p * tl.Lp;
        if (j < job.jb) dst[j - job.ja] = resample_fold(ln.acc[p]);
    }
}

}  // namespace th
