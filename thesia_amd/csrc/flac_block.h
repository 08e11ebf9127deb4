// flac_block.h — the bodies of the three FLAC kernels (kernels_flac.hip) as phase functions over (thread id, LDS struct), host +
// device: a kernel calls them between its barriers, and the host runs a workgroup's threads one after the other through the same
// source.  That host run IS th_flac_encode_i32 and th_flac_encode_i32_ex (flac_run_job_host below), and scripts/san_flac.cpp and
// scripts/san_flac_lpc.cpp run it under AddressSanitizer and UBSan with every slot, table and destination at its exact size.
//
// Fault safety.  Every bit position that comes from data is checked against the stream's limit inside flac_put_bits; the Rice path
// runs only when the exact total is below the verbatim size, otherwise the verbatim path, whose size follows from n alone.  No loop's
// trip count depends on a sample: a unary run is never walked, only its length is added.  Indices are 64-bit.  A unit's slot holds
// the verbatim bits of the unit's own sample size (a stereo block's four units: the side channel's, the widest).
#pragma once
#include "export_core.h"
#include "flac_core.h"
#include "flac_plan.h"  // FlacJob, FlacJobResult

namespace th {

constexpr uint32_t FLAC_THREADS = 256;
constexpr uint32_t FLAC_PER_THREAD = FLAC_BLOCK / FLAC_THREADS;  // 16
constexpr uint32_t FLAC_MAX_PARTS = 1u << FLAC_MAX_PART_ORDER;
constexpr uint32_t FLAC_S_ROW = FLAC_MAX_K + 1;
constexpr uint32_t FLAC_OUT_WORDS = (8u + FLAC_BLOCK * 25u + 31u) / 32u;  // a verbatim side subframe of a 24-bit file
static_assert(FLAC_BLOCK % FLAC_THREADS == 0 && FLAC_THREADS % FLAC_MAX_PARTS == 0, "threads per partition");

enum : uint32_t { FLAC_SUB_CONSTANT = 0, FLAC_SUB_VERBATIM = 1, FLAC_SUB_FIXED = 2, FLAC_SUB_LPC = 3 };
enum : uint32_t { FLAC_MIX_NONE = 0, FLAC_MIX_MID = 1, FLAC_MIX_SIDE = 2 };

// ---------------------------------------------------------------------------------------------- the subframe kernel
// one workgroup: n samples of one coded channel of one block
struct FlacSubWork {
    unsigned long long S[FLAC_MAX_PARTS * FLAC_S_ROW];  // of the candidate at hand: S[q][k] = sum of (u >> k) over partition q
    uint32_t out[FLAC_OUT_WORDS];
};
struct FlacSubLds {
    int32_t s[FLAC_BLOCK];
    union {
        FlacSubWork w;
        int32_t x[FLAC_BLOCK];  // the windowed samples: only until the autocorrelation is summed, then w is zeroed
    };
    unsigned long long cost[FLAC_CANDS];
    unsigned long long r[FLAC_LPC_MAX + 1];  // the autocorrelation, int64 in two's complement
    uint8_t bestk[FLAC_CANDS][FLAC_MAX_PARTS];
    uint32_t scan[FLAC_THREADS];
    FlacLpcFit fit;
    uint32_t differ;   // some sample is not s[0]
    uint32_t cnt[2];   // clamped, NaN
    uint32_t amax;     // the largest |s|
    uint32_t lpc_bad;  // bit m - 1: a residual of LPC order m does not fit 32 bits
};

struct FlacUnit {  // what the workgroup works on
    uint32_t c, n;
    uint32_t bps;    // of this unit's samples: the file's, and one more for a side channel
    uint32_t fbps;   // the file's: the Rice method and the coefficients' precision follow it
    uint32_t mix;    // FLAC_MIX_*: channel c as it is, or mid / side of channels 0 and 1
    uint64_t first;  // absolute index of sample 0 of the block
    uint64_t slot;   // the unit's index in its job (block-major)
    bool any;
};
// flags: the job's (a kernel that is compiled for flags == 0 passes the constant)
TH_HD FlacUnit flac_unit_of(const FlacJob &job, uint32_t u, uint32_t flags) {
    FlacUnit k{};
    if (job.n_ch == 0) return k;
    const uint32_t upb = flac_units_per_block(job.n_ch, flags);
    const uint32_t blk = u / upb;
    k.c = u - blk * upb;
    k.fbps = k.bps = flac_bps(job.format);
    if (upb != job.n_ch && k.c >= 2u) {
        k.mix = k.c == 2u ? FLAC_MIX_MID : FLAC_MIX_SIDE;
        k.bps += k.c == 3u ? 1u : 0u;
    }
    k.slot = u;
    const uint64_t at = (job.b0 + blk) * FLAC_BLOCK, len = job.s1 - job.s0;
    k.any = blk < job.nb && at < len;  // a block past the job's end stores nothing
    if (k.any) {
        k.first = job.s0 + at;
        k.n = len - at < FLAC_BLOCK ? (uint32_t)(len - at) : FLAC_BLOCK;
    }
    return k;
}

struct FlacChoice {
    uint32_t type, order, p, bits;  // bits: the whole subframe
    uint32_t cand;                  // FIXED, LPC: the candidate's index (the row of bestk)
};

// the rows of sums and the subframe's words
TH_HD void flac_sub_clear_work(const FlacUnit &k, uint32_t tid, FlacSubLds &l) {
    for (uint32_t i = tid; i < FLAC_MAX_PARTS * FLAC_S_ROW; i += FLAC_THREADS) l.w.S[i] = 0;
    const uint32_t nw = flac_slot_words(k.n, k.bps);
    for (uint32_t i = tid; i < nw; i += FLAC_THREADS) l.w.out[i] = 0;
}
TH_HD void flac_sub_clear(const FlacUnit &k, uint32_t tid, FlacSubLds &l) {
    flac_sub_clear_work(k, tid, l);
    if (tid < FLAC_CANDS) l.cost[tid] = 0;
    if (tid <= FLAC_LPC_MAX) l.r[tid] = 0;
    if (tid == 0) l.differ = l.cnt[0] = l.cnt[1] = l.amax = l.lpc_bad = l.fit.ok = 0;
}

TH_HD int32_t flac_mix(uint32_t mix, int32_t a, int32_t b) { return mix == FLAC_MIX_MID ? (a + b) >> 1 : a - b; }

// the block's samples of planar f32 channel k.c, quantised as th_export_quantize does at the ABSOLUTE index; a mid or side unit
// quantises both channels (their counts are the L and R units' to report)
TH_HD void flac_sub_quantize(const FlacJob &job, const FlacUnit &k, uint32_t tid, FlacSubLds &l) {
    const bool tpdf = job.dither == TH_DITHER_TPDF;
    const double S = export_scale(job.format);
    ExportCounts cnt{0, 0};
    if (k.mix == FLAC_MIX_NONE) {
        const gptr<const float> src = as_global(as_global(job.chan)[k.c]);
        const uint32_t k0 = export_dither_k0(job.seed, k.c);
#pragma unroll 4
        for (uint32_t j = 0; j < FLAC_PER_THREAD; j++) {
            const uint32_t i = tid + j * FLAC_THREADS;
            if (i >= k.n) break;
            const uint64_t f = k.first + i;
            uint32_t a = 0, b = 0;
            if (tpdf) export_dither_ab(export_dither_k1(k0, f), f, &a, &b);
            l.s[i] = export_quantize_one(src[f], S, tpdf, a, b, &cnt);
        }
        if (cnt.clamped) TH_FLAC_ADD32(&l.cnt[0], cnt.clamped);
        if (cnt.nan) TH_FLAC_ADD32(&l.cnt[1], cnt.nan);
        return;
    }
    const gptr<const float> src0 = as_global(as_global(job.chan)[0]), src1 = as_global(as_global(job.chan)[1]);
    const uint32_t k00 = export_dither_k0(job.seed, 0), k01 = export_dither_k0(job.seed, 1);
#pragma unroll 2
    for (uint32_t j = 0; j < FLAC_PER_THREAD; j++) {
        const uint32_t i = tid + j * FLAC_THREADS;
        if (i >= k.n) break;
        const uint64_t f = k.first + i;
        uint32_t a0 = 0, b0 = 0, a1 = 0, b1 = 0;
        if (tpdf) {
            export_dither_ab(export_dither_k1(k00, f), f, &a0, &b0);
            export_dither_ab(export_dither_k1(k01, f), f, &a1, &b1);
        }
        const int32_t left = export_quantize_one(src0[f], S, tpdf, a0, b0, &cnt), right = export_quantize_one(src1[f], S, tpdf, a1, b1, &cnt);
        l.s[i] = flac_mix(k.mix, left, right);
    }
}
// ... or taken as they are (th_flac_encode_i32); chan: the channels from the block's own `first`
TH_HD void flac_sub_load_i32(const int32_t *const *chan, const FlacUnit &k, uint32_t tid, FlacSubLds &l) {
    for (uint32_t i = tid; i < k.n; i += FLAC_THREADS)
        l.s[i] = k.mix == FLAC_MIX_NONE ? chan[k.c][k.first + i] : flac_mix(k.mix, chan[0][k.first + i], chan[1][k.first + i]);
}

// ---- TH_FLAC_LPC: the block's level, the windowed samples, the autocorrelation, the fit (between barriers, in this order)
TH_HD void flac_lpc_level(const FlacUnit &k, uint32_t tid, FlacSubLds &l) {
    uint32_t m = 0;
    for (uint32_t j = 0; j < FLAC_PER_THREAD; j++) {
        const uint32_t i = tid + j * FLAC_THREADS;
        if (i >= k.n) break;
        const int32_t v = l.s[i];
        const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
        m = a > m ? a : m;
    }
    if (m) TH_FLAC_MAX32(&l.amax, m);
}
TH_HD void flac_lpc_window_block(const FlacUnit &k, uint32_t tid, FlacSubLds &l) {
    const uint32_t sh = flac_lpc_level_shift(l.amax);
    for (uint32_t j = 0; j < FLAC_PER_THREAD; j++) {
        const uint32_t i = tid + j * FLAC_THREADS;
        if (i >= k.n) break;
        l.x[i] = flac_lpc_windowed(l.s[i], flac_lpc_window(i, k.n), sh);
    }
}
// nine lags as per-thread int64 partial sums, one 64-bit LDS atomic each (integer sums do not depend on the order)
TH_HD void flac_lpc_autocorr(const FlacUnit &k, uint32_t tid, FlacSubLds &l) {
    long long part[FLAC_LPC_MAX + 1];
#pragma unroll
    for (uint32_t m = 0; m <= FLAC_LPC_MAX; m++) part[m] = 0;
    for (uint32_t j = 0; j < FLAC_PER_THREAD; j++) {
        const uint32_t i = tid + j * FLAC_THREADS;
        if (i >= k.n) break;
        const long long xi = l.x[i];
#pragma unroll
        for (uint32_t m = 0; m <= FLAC_LPC_MAX; m++)
            if (i + m < k.n) part[m] += xi * (long long)l.x[i + m];
    }
#pragma unroll
    for (uint32_t m = 0; m <= FLAC_LPC_MAX; m++)
        if (part[m]) TH_FLAC_ADD64(&l.r[m], (unsigned long long)part[m]);
}
// one lane: Levinson-Durbin and the quantiser (the other lanes zero the work area the windowed samples lay in: flac_sub_clear_work)
TH_HD void flac_lpc_fit_block(const FlacUnit &k, uint32_t tid, FlacSubLds &l) {
    if (tid != 0) return;
    long long r[FLAC_LPC_MAX + 1];
#pragma unroll
    for (uint32_t m = 0; m <= FLAC_LPC_MAX; m++) r[m] = (long long)l.r[m];
    flac_lpc_fit(r, flac_lpc_max_order(k.n), flac_lpc_precision(k.fbps), &l.fit);
}

// S[q][k] of the thread's zigzagged residuals u[] of partition q
TH_HD void flac_sub_add_sums(const FlacUnit &k, const uint32_t *u, uint32_t q, FlacSubLds &l) {
    const uint32_t kmax = flac_kmax(k.fbps);
    for (uint32_t kk = 0; kk <= kmax; kk++) {
        unsigned long long sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < FLAC_PER_THREAD; j++) sum += u[j] >> kk;
        if (sum) TH_FLAC_ADD64(&l.w.S[q * FLAC_S_ROW + kk], sum);
    }
}
// S[q][k] of fixed order o.  Partition q of the 2^p is the work of 256 >> p threads, which stride over its n >> p samples
TH_HD void flac_sub_accumulate(const FlacUnit &k, uint32_t o, uint32_t tid, FlacSubLds &l) {
    if (k.n < FLAC_MIN_PART) return;
    const uint32_t p = flac_part_order(k.n), psz = k.n >> p, T = FLAC_THREADS >> p;
    const uint32_t q = tid / T, r = tid - q * T;
    uint32_t u[FLAC_PER_THREAD];
    bool any = false, differ = false;
#pragma unroll
    for (uint32_t j = 0; j < FLAC_PER_THREAD; j++) {
        const uint32_t at = r + j * T, i = q * psz + at;
        const bool in = at < psz && i >= o;
        u[j] = in ? flac_zigzag(flac_residual(l.s, i, o)) : 0u;
        any |= in;
        if (o == 0 && in) differ |= l.s[i] != l.s[0];
    }
    if (differ) l.differ = 1u;  // (every writer writes the same value)
    if (!any) return;
    flac_sub_add_sums(k, u, q, l);
}
// ... of LPC order m (a candidate of the fit); a residual beyond 32 bits marks the order
TH_HD void flac_sub_accumulate_lpc(const FlacUnit &k, uint32_t m, uint32_t tid, FlacSubLds &l) {
    const uint32_t p = flac_part_order(k.n, m), psz = k.n >> p, T = FLAC_THREADS >> p;
    const uint32_t q = tid / T, r = tid - q * T;
    int32_t coef[FLAC_LPC_MAX];
#pragma unroll
    for (uint32_t j = 0; j < FLAC_LPC_MAX; j++) coef[j] = j < m ? l.fit.q[m - 1][j] : 0;
    const uint32_t shift = l.fit.shift[m - 1];
    uint32_t u[FLAC_PER_THREAD];
    bool any = false, bad = false;
#pragma unroll
    for (uint32_t j = 0; j < FLAC_PER_THREAD; j++) {
        const uint32_t at = r + j * T, i = q * psz + at;
        const bool in = at < psz && i >= m && i < k.n;
        u[j] = 0u;
        if (in) {
            const long long e = flac_lpc_residual(l.s, i, coef, m, shift);
            bad |= !flac_residual_fits(e);
            u[j] = flac_zigzag((int32_t)e);
        }
        any |= in;
    }
    if (bad) TH_FLAC_OR32(&l.lpc_bad, 1u << (m - 1u));
    if (!any) return;
    flac_sub_add_sums(k, u, q, l);
}
// each partition's parameter and bits, the candidate's cost; the rows are zero again for the next candidate
TH_HD void flac_sub_pick_k(const FlacUnit &k, uint32_t cand, uint32_t tid, FlacSubLds &l) {
    if (k.n < FLAC_MIN_PART) return;
    const uint32_t o = flac_cand_order(cand), p = flac_part_order(k.n, o), psz = k.n >> p;
    if (tid >= (1u << p)) return;
    const uint32_t m = psz - (tid == 0 ? o : 0u);
    unsigned long long bits = 0;
    l.bestk[cand][tid] = (uint8_t)flac_best_k(&l.w.S[tid * FLAC_S_ROW], m, flac_kmax(k.fbps), &bits);
    TH_FLAC_ADD64(&l.cost[cand], bits + flac_param_bits(k.fbps));
    for (uint32_t kk = 0; kk < FLAC_S_ROW; kk++) l.w.S[tid * FLAC_S_ROW + kk] = 0;
}
// CONSTANT; else the first candidate of the smallest cost: fixed o at o bps + 6 + the partitions, then (lpc) the fit's LPC orders at
// flac_lpc_head_bits + the partitions; VERBATIM when that is no gain (every thread computes the same)
TH_HD FlacChoice flac_sub_choose(const FlacUnit &k, bool lpc, const FlacSubLds &l) {
    FlacChoice ch{};
    bool differ = l.differ != 0;
    if (k.n < FLAC_MIN_PART) {
        differ = false;
        for (uint32_t i = 1; i < FLAC_MIN_PART - 1; i++) differ |= i < k.n && l.s[i] != l.s[0];
    }
    if (!differ) {
        ch.type = FLAC_SUB_CONSTANT;
        ch.bits = 8u + k.bps;
        return ch;
    }
    ch.type = FLAC_SUB_VERBATIM;
    ch.bits = flac_verbatim_bits(k.n, k.bps);
    if (k.n < FLAC_MIN_PART) return ch;
    unsigned long long best = 0;
    uint32_t bc = 0;
    for (uint32_t o = 0; o <= FLAC_MAX_ORDER; o++) {
        const unsigned long long c = l.cost[o] + o * k.bps + 6u;
        if (o == 0 || c < best) {
            best = c;
            bc = o;
        }
    }
    if (lpc) {
        const uint32_t ok = l.fit.ok & ~l.lpc_bad, P = flac_lpc_precision(k.fbps);
        for (uint32_t m = 1; m <= FLAC_LPC_MAX; m++) {
            if (!((ok >> (m - 1u)) & 1u)) continue;
            const unsigned long long c = l.cost[FLAC_MAX_ORDER + m] + flac_lpc_head_bits(m, k.bps, P);
            if (c < best) {
                best = c;
                bc = FLAC_MAX_ORDER + m;
            }
        }
    }
    if (best >= (unsigned long long)k.n * k.bps) return ch;
    ch.type = flac_cand_is_lpc(bc) ? FLAC_SUB_LPC : FLAC_SUB_FIXED;
    ch.cand = bc;
    ch.order = flac_cand_order(bc);
    ch.p = flac_part_order(k.n, ch.order);
    ch.bits = 8u + (uint32_t)best;
    return ch;
}

// the code of residual i of the chosen candidate: its length, with the partition's parameter in front of a partition's first code
struct FlacCode {
    uint32_t u, k, lead;  // lead: the parameter's bits in front (0 or 4 / 5)
};
TH_HD FlacCode flac_code_at(const FlacUnit &k, const FlacChoice &ch, uint32_t i, const FlacSubLds &l) {
    const uint32_t psz = k.n >> ch.p, q = i / psz;
    FlacCode c;
    if (ch.type == FLAC_SUB_LPC)
        c.u = flac_zigzag((int32_t)flac_lpc_residual(l.s, i, l.fit.q[ch.order - 1u], ch.order, l.fit.shift[ch.order - 1u]));
    else
        c.u = flac_zigzag(flac_residual(l.s, i, ch.order));
    c.k = l.bestk[ch.cand][q];
    c.lead = (i == (q == 0 ? ch.order : q * psz)) ? flac_param_bits(k.fbps) : 0u;
    return c;
}
TH_HD uint32_t flac_code_bits(const FlacCode &c) { return c.lead + (c.u >> c.k) + 1u + c.k; }

// FIXED, LPC: the bits of the thread's 16 consecutive residuals
TH_HD void flac_sub_lengths(const FlacUnit &k, const FlacChoice &ch, uint32_t tid, FlacSubLds &l) {
    if (ch.type != FLAC_SUB_FIXED && ch.type != FLAC_SUB_LPC) return;
    uint32_t sum = 0;
    for (uint32_t j = 0; j < FLAC_PER_THREAD; j++) {
        const uint32_t i = tid * FLAC_PER_THREAD + j;
        if (i >= ch.order && i < k.n) sum += flac_code_bits(flac_code_at(k, ch, i, l));
    }
    l.scan[tid] = sum;
}
// the subframe's bits into l.w.out
TH_HD void flac_sub_write(const FlacUnit &k, const FlacChoice &ch, uint32_t tid, FlacSubLds &l) {
    const uint32_t limit = ch.bits;
    uint32_t *out = l.w.out;
    if (ch.type == FLAC_SUB_CONSTANT) {
        if (tid == 0) {
            flac_put_bits(out, limit, 0, 8, 0u);
            flac_put_bits(out, limit, 8, k.bps, (uint32_t)l.s[0]);
        }
        return;
    }
    if (ch.type == FLAC_SUB_VERBATIM) {
        if (tid == 0) flac_put_bits(out, limit, 0, 8, 1u << 1);
        for (uint32_t i = tid; i < k.n; i += FLAC_THREADS) flac_put_bits(out, limit, 8u + i * k.bps, k.bps, (uint32_t)l.s[i]);
        return;
    }
    const uint32_t method = ((k.fbps == 16 ? 0u : 1u) << 4) | ch.p;
    uint32_t base;
    if (ch.type == FLAC_SUB_LPC) {
        const uint32_t P = flac_lpc_precision(k.fbps), coefs = 8u + ch.order * k.bps + 9u;
        base = 8u + flac_lpc_head_bits(ch.order, k.bps, P);
        if (tid == 0) {
            flac_put_bits(out, limit, 0, 8, (32u | (ch.order - 1u)) << 1);
            flac_put_bits(out, limit, coefs - 9u, 4, P - 1u);
            flac_put_bits(out, limit, coefs - 5u, 5, l.fit.shift[ch.order - 1u]);
            flac_put_bits(out, limit, base - 6u, 6, method);
        }
        if (tid < ch.order) flac_put_bits(out, limit, coefs + tid * P, P, (uint32_t)l.fit.q[ch.order - 1u][tid]);
    } else {
        base = 8u + ch.order * k.bps + 6u;
        if (tid == 0) {
            flac_put_bits(out, limit, 0, 8, (8u | ch.order) << 1);
            flac_put_bits(out, limit, base - 6u, 6, method);
        }
    }
    if (tid < ch.order) flac_put_bits(out, limit, 8u + tid * k.bps, k.bps, (uint32_t)l.s[tid]);
    uint32_t pos = base;
    for (uint32_t t = 0; t < tid; t++) pos += l.scan[t];
    const uint32_t pb = flac_param_bits(k.fbps);
    for (uint32_t j = 0; j < FLAC_PER_THREAD; j++) {
        const uint32_t i = tid * FLAC_PER_THREAD + j;
        if (i < ch.order || i >= k.n) continue;
        const FlacCode c = flac_code_at(k, ch, i, l);
        if (c.lead) flac_put_bits(out, limit, pos, pb, c.k);
        // the unary zeros are the buffer's; the stop bit and the k low bits are one write of k + 1 <= 31 bits
        const uint32_t q = c.u >> c.k;
        if (q <= limit && pos + c.lead <= limit - q)
            flac_put_bits(out, limit, pos + c.lead + q, c.k + 1u, (1u << c.k) | (c.u & ((1u << c.k) - 1u)));
        pos += flac_code_bits(c);
        if (pos > limit) pos = limit;  // (cannot be: the lengths add up to the exact total)
    }
}
// the words to the unit's slot, the length to the table, the counts to the request's
TH_HD void flac_sub_store(const FlacJob &job, const FlacUnit &k, const FlacChoice &ch, uint32_t tid, const FlacSubLds &l) {
    const gptr<uint32_t> slot = as_global(job.slots) + k.slot * job.slot_words;
    uint32_t nw = (ch.bits + 31u) >> 5;
    if (nw > job.slot_words) nw = job.slot_words;
    for (uint32_t i = tid; i < nw; i += FLAC_THREADS) slot[i] = l.w.out[i];
    if (tid == 0) as_global(job.bits)[k.slot] = ch.bits;
#if defined(__HIP_DEVICE_COMPILE__)  // (integer sums do not depend on the order; the host's run adds l.cnt itself)
    if (tid < 2 && l.cnt[tid])
        __hip_atomic_fetch_add(as_global(job.cnt) + tid, (unsigned long long)l.cnt[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// ---------------------------------------------------------------------------------------------- the scan kernel
// one workgroup: the frames of one job.  Lengths from the table, then every frame's byte offset in the job, the total, min and max
struct FlacScanLds {
    unsigned long long sum[FLAC_THREADS];
    uint32_t mn[FLAC_THREADS], mx[FLAC_THREADS];
};
TH_HD uint32_t flac_frame_n(const FlacJob &job, uint32_t f) {
    const uint64_t at = (job.b0 + f) * FLAC_BLOCK, len = job.s1 - job.s0;
    return at >= len ? 0u : len - at < FLAC_BLOCK ? (uint32_t)(len - at) : FLAC_BLOCK;
}
// which of the frame's units are its subframes, and their bits: the n_ch channels, or a stereo block's cheapest pair of L R M S
TH_HD FlacAssign flac_frame_assign(const FlacJob &job, uint32_t f) {
    const uint32_t upb = flac_units_per_block(job.n_ch, job.flags);
    const gptr<const uint32_t> bits = as_global((const uint32_t *)job.bits) + (uint64_t)f * upb;
    if (upb != job.n_ch) return flac_pick_assignment(bits[0], bits[1], bits[2], bits[3]);
    FlacAssign a{job.n_ch - 1u, 0u, 1u, 0u};
    for (uint32_t c = 0; c < job.n_ch; c++) a.bits += bits[c];
    return a;
}
TH_HD uint32_t flac_frame_bytes(const FlacJob &job, uint32_t f) {
    return flac_frame_header_len(job.sr, job.b0 + f, flac_frame_n(job, f)) + (uint32_t)((flac_frame_assign(job, f).bits + 7u) >> 3) + 2u;
}
TH_HD uint32_t flac_scan_per_thread(const FlacJob &job) { return (job.nb + FLAC_THREADS - 1) / FLAC_THREADS; }
TH_HD void flac_scan_sum(const FlacJob &job, uint32_t tid, FlacScanLds &l) {
    const uint32_t per = flac_scan_per_thread(job);
    unsigned long long sum = 0;
    uint32_t mn = 0xffffffffu, mx = 0;
    for (uint32_t j = 0; j < per; j++) {
        const uint64_t f = (uint64_t)tid * per + j;
        if (f >= job.nb) break;
        const uint32_t b = flac_frame_bytes(job, (uint32_t)f);
        sum += b;
        mn = b < mn ? b : mn;
        mx = b > mx ? b : mx;
    }
    l.sum[tid] = sum;
    l.mn[tid] = mn;
    l.mx[tid] = mx;
}
TH_HD void flac_scan_write(const FlacJob &job, uint32_t tid, const FlacScanLds &l) {
    const uint32_t per = flac_scan_per_thread(job);
    unsigned long long at = 0;
    for (uint32_t t = 0; t < tid; t++) at += l.sum[t];
    const gptr<uint32_t> foff = as_global(job.foff);
    for (uint32_t j = 0; j < per; j++) {
        const uint64_t f = (uint64_t)tid * per + j;
        if (f >= job.nb) break;
        foff[f] = (uint32_t)at;
        at += flac_frame_bytes(job, (uint32_t)f);
    }
    if (tid == 0) {
        FlacJobResult r{0, 0xffffffffu, 0};
        for (uint32_t t = 0; t < FLAC_THREADS; t++) {
            r.bytes += l.sum[t];
            r.min_frame = l.mn[t] < r.min_frame ? l.mn[t] : r.min_frame;
            r.max_frame = l.mx[t] > r.max_frame ? l.mx[t] : r.max_frame;
        }
        *as_global(job.res) = r;
    }
}

// ---------------------------------------------------------------------------------------------- the frame kernel
// one workgroup: one frame.  The frame is a bit stream of 1 + n_ch sources (the header, the subframes); byte i of the frame goes to
// dst + off + i, so the IMAGE the workgroup writes is that stream shifted by the destination's offset in its 4-byte word
struct FlacFrameLds {
    uint32_t hdr[FLAC_FRAME_HEADER_MAX / 4];
    uint8_t hdr_bytes[FLAC_FRAME_HEADER_MAX];
    uint16_t crc_tab[256];
    uint32_t crc[FLAC_THREADS];
    uint32_t src_bits[FLAC_MAX_CHANNELS];
    uint32_t src_unit[FLAC_MAX_CHANNELS];  // subframe c of the frame: which of the block's units
};
struct FlacFrame {
    uint32_t f, n, hdr_len;
    uint32_t body;  // bytes in front of the CRC-16
    uint64_t off;   // the frame's first byte in the job
    bool any;
};
TH_HD void flac_frame_prepare(const FlacJob &job, uint32_t f, uint32_t tid, FlacFrameLds &l) {
    l.crc_tab[tid] = (uint16_t)flac_crc16_entry(tid);
    const uint32_t upb = flac_units_per_block(job.n_ch, job.flags);
    if (tid < job.n_ch && tid < FLAC_MAX_CHANNELS) {
        uint32_t unit = tid;
        if (upb != job.n_ch) {
            const FlacAssign a = flac_frame_assign(job, f);
            unit = tid == 0 ? a.u0 : a.u1;
        }
        l.src_unit[tid] = unit;
        l.src_bits[tid] = as_global((const uint32_t *)job.bits)[(uint64_t)f * upb + unit];
    }
    if (tid == 0) {
        for (uint32_t i = 0; i < FLAC_FRAME_HEADER_MAX; i++) l.hdr_bytes[i] = 0;
        const uint32_t n = flac_frame_n(job, f);
        if (n) flac_frame_header_as(job.sr, upb != job.n_ch ? flac_frame_assign(job, f).code : job.n_ch - 1u, flac_bps(job.format), job.b0 + f, n, l.hdr_bytes);
        for (uint32_t i = 0; i < FLAC_FRAME_HEADER_MAX / 4; i++)
            l.hdr[i] = ((uint32_t)l.hdr_bytes[4 * i] << 24) | ((uint32_t)l.hdr_bytes[4 * i + 1] << 16) | ((uint32_t)l.hdr_bytes[4 * i + 2] << 8) |
                       l.hdr_bytes[4 * i + 3];
    }
}
TH_HD FlacFrame flac_frame_of(const FlacJob &job, uint32_t f, const FlacFrameLds &l) {
    FlacFrame fr{};
    fr.f = f;
    fr.n = flac_frame_n(job, f);
    fr.any = f < job.nb && fr.n != 0 && job.n_ch <= FLAC_MAX_CHANNELS;
    if (!fr.any) return fr;
    fr.hdr_len = flac_frame_header_len(job.sr, job.b0 + f, fr.n);
    uint64_t total = 0;
    for (uint32_t c = 0; c < job.n_ch; c++) total += l.src_bits[c];
    fr.body = fr.hdr_len + (uint32_t)((total + 7u) >> 3);
    fr.off = as_global((const uint32_t *)job.foff)[f];
    return fr;
}
// 32 bits of the frame from bit `at` (may be negative): each source is a funnel shift of two of its words
TH_HD uint32_t flac_frame_bits32(const FlacJob &job, const FlacFrame &fr, int64_t at, const FlacFrameLds &l) {
    uint32_t v = flac_get_bits32(l.hdr, fr.hdr_len * 8u, at);
    int64_t start = (int64_t)fr.hdr_len * 8;
    const uint32_t upb = flac_units_per_block(job.n_ch, job.flags);
    for (uint32_t c = 0; c < FLAC_MAX_CHANNELS; c++) {
        if (c >= job.n_ch) break;
        const uint32_t len = l.src_bits[c];
        if (at + 32 > start && at < start + (int64_t)len) {
            const uint32_t *slot =
                (const uint32_t *)(as_global((const uint32_t *)job.slots) + ((uint64_t)fr.f * upb + l.src_unit[c]) * job.slot_words);
            const uint32_t cap = job.slot_words * 32u;
            v |= flac_get_bits32(slot, len < cap ? len : cap, at - start);
        }
        start += len;
    }
    return v;
}
// image word w (the 4 bytes at the destination's aligned address + 4 w) of the frame's body, stored: whole where the body has all
// four bytes, else byte by byte
TH_HD void flac_frame_store(const FlacJob &job, const FlacFrame &fr, uint32_t tid, const FlacFrameLds &l) {
    uint8_t *dst = job.dst + fr.off;
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
    const uint32_t nw = (head + fr.body + 3u) >> 2;
    for (uint32_t w = tid; w < nw; w += FLAC_THREADS) {
        const uint32_t v = flac_frame_bits32(job, fr, (int64_t)w * 32 - (int64_t)head * 8, l);
        const int64_t b0 = (int64_t)w * 4 - head;  // the body's byte of the word's first byte
        if (b0 >= 0 && b0 + 4 <= (int64_t)fr.body) {
            *reinterpret_cast<gptr<uint32_t>>(as_global(dst + b0)) = __builtin_bswap32(v);
        } else {
            for (int j = 0; j < 4; j++)
                if (b0 + j >= 0 && b0 + j < (int64_t)fr.body) as_global(dst)[b0 + j] = (uint8_t)(v >> (24 - 8 * j));
        }
    }
}
// the CRC of the thread's run of body words, moved to the body's end
TH_HD void flac_frame_crc_part(const FlacJob &job, const FlacFrame &fr, uint32_t tid, FlacFrameLds &l) {
    const uint32_t nw = (fr.body + 3u) >> 2, per = (nw + FLAC_THREADS - 1) / FLAC_THREADS;
    uint32_t crc = 0, end = 0;
    for (uint32_t j = 0; j < per; j++) {
        const uint32_t w = tid * per + j;
        if (w >= nw) break;
        const uint32_t v = flac_frame_bits32(job, fr, (int64_t)w * 32, l);
        for (uint32_t b = 0; b < 4; b++)
            if (w * 4 + b < fr.body) {
                crc = flac_crc16_step(crc, (v >> (24 - 8 * b)) & 0xffu, l.crc_tab);
                end = w * 4 + b + 1;
            }
    }
    l.crc[tid] = end ? flac_crc16_shift(crc, fr.body - end) : 0u;
}
TH_HD void flac_frame_crc_store(const FlacJob &job, const FlacFrame &fr, uint32_t tid, const FlacFrameLds &l) {
    if (tid != 0) return;
    uint32_t crc = 0;
    for (uint32_t t = 0; t < FLAC_THREADS; t++) crc ^= l.crc[t];
    const gptr<uint8_t> dst = as_global(job.dst) + fr.off + fr.body;
    dst[0] = (uint8_t)(crc >> 8);
    dst[1] = (uint8_t)crc;
}

// ---------------------------------------------------------------------------------------------- the host's run of the three kernels
// One job whose addresses are host memory.  src: the channels as int32 (chan != NULL) or the job's own planar f32 (job.chan).
// cnt (2, may be NULL) receives the quantiser's counts
inline void flac_run_job_host(const FlacJob &job, const int32_t *const *chan, unsigned long long *cnt) {
    {
        FlacSubLds *l = new FlacSubLds;
        const uint32_t upb = flac_units_per_block(job.n_ch, job.flags);
        const bool lpc = (job.flags & TH_FLAC_LPC) != 0;
        for (uint32_t u = 0; u < job.nb * upb; u++) {
            const FlacUnit k = flac_unit_of(job, u, job.flags);
            if (!k.any) continue;
            for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_sub_clear(k, t, *l);
            for (uint32_t t = 0; t < FLAC_THREADS; t++) {
                if (chan) {
                    FlacUnit rel = k;
                    rel.first = k.first - job.s0;  // (the host's arrays start at the range)
                    flac_sub_load_i32(chan, rel, t, *l);
                } else {
                    flac_sub_quantize(job, k, t, *l);
                }
            }
            const bool fit = lpc && k.n >= FLAC_MIN_PART;
            if (fit) {
                for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_lpc_level(k, t, *l);
                for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_lpc_window_block(k, t, *l);
                for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_lpc_autocorr(k, t, *l);
                for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_sub_clear_work(k, t, *l);
                for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_lpc_fit_block(k, t, *l);
            }
            for (uint32_t o = 0; o <= FLAC_MAX_ORDER; o++) {
                for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_sub_accumulate(k, o, t, *l);
                for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_sub_pick_k(k, o, t, *l);
            }
            for (uint32_t m = 1; fit && m <= FLAC_LPC_MAX; m++) {
                if (!((l->fit.ok >> (m - 1u)) & 1u)) continue;
                for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_sub_accumulate_lpc(k, m, t, *l);
                for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_sub_pick_k(k, FLAC_MAX_ORDER + m, t, *l);
            }
            const FlacChoice ch = flac_sub_choose(k, fit, *l);
            for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_sub_lengths(k, ch, t, *l);
            for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_sub_write(k, ch, t, *l);
            for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_sub_store(job, k, ch, t, *l);
            if (cnt) {
                cnt[0] += l->cnt[0];
                cnt[1] += l->cnt[1];
            }
        }
        delete l;
    }
    {
        FlacScanLds l;
        for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_scan_sum(job, t, l);
        for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_scan_write(job, t, l);
    }
    FlacFrameLds l;
    for (uint32_t f = 0; f < job.nb; f++) {
        for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_frame_prepare(job, f, t, l);
        const FlacFrame fr = flac_frame_of(job, f, l);
        if (!fr.any) continue;
        for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_frame_store(job, fr, t, l);
        for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_frame_crc_part(job, fr, t, l);
        for (uint32_t t = 0; t < FLAC_THREADS; t++) flac_frame_crc_store(job, fr, t, l);
    }
}

}  // namespace th
