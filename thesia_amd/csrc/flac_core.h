// flac_core.h — the arithmetic of the FLAC export (th_tm_export_flac, th_flac_encode_i32), written once for the host and for the
// device (kernels_flac.hip through flac_block.h): the fixed predictors, the zigzag, the Rice cost and argmin rules, the frame header,
// CRC-8 and CRC-16, and the big-endian bit writer; for the _ex entries (TH_FLAC_LPC, TH_FLAC_STEREO) the LPC fit of a block (integer
// window and autocorrelation, Levinson-Durbin and the coefficient quantiser in f64, one operation after the other in the order written
// here) and the rule that picks a stereo frame's channel assignment.  Every translation unit that runs flac_lpc_fit is built with
// -ffp-contract=off: kernels_flac.hip and api.hip in the library, the sanitizer programs by their command lines; a fused
// multiply-add would change the coefficients.  The definitions are those of include/thesia_amd.h ("FLAC export"), a subset of
// RFC 9639 with every choice fixed, so the bytes of a stream are a function of its samples and the flags.
#pragma once
#include <stdint.h>

#include "../../include/thesia_amd.h"  // TH_PCM_*
#include "stft_core.h"                 // TH_HD

namespace th {

constexpr uint32_t FLAC_BLOCK = TH_FLAC_BLOCK;        // samples of every block but a stream's last
constexpr uint32_t FLAC_STREAM_HEADER = 42;           // "fLaC", a metadata block header, STREAMINFO
constexpr uint32_t FLAC_FRAME_HEADER_MAX = 16;        // sync .. CRC-8 with a 7-byte number and both 16-bit tails
constexpr uint32_t FLAC_MAX_CHANNELS = 8;
constexpr uint32_t FLAC_MAX_PART_ORDER = 6;
constexpr uint32_t FLAC_MAX_ORDER = 4;
constexpr uint32_t FLAC_MIN_PART = 5;                 // residuals' samples of the smallest partition; below it no predictor is tried
constexpr uint32_t FLAC_LPC_MAX = TH_FLAC_LPC_MAX_ORDER;
constexpr uint32_t FLAC_CANDS = FLAC_MAX_ORDER + 1 + FLAC_LPC_MAX;  // fixed 0 .. 4, then LPC 1 .. 8
constexpr uint32_t FLAC_FLAGS = TH_FLAC_LPC | TH_FLAC_STEREO;
constexpr uint32_t FLAC_MAX_K = 30;                   // the largest Rice parameter (24 bit; 16 bit stops at 14)
constexpr uint64_t FLAC_MAX_SAMPLES = 1ull << 36;
constexpr uint32_t FLAC_MAX_RATE = 1048575;

TH_HD uint32_t flac_bps(uint32_t format) { return format == TH_PCM_S16 ? 16u : 24u; }
TH_HD uint32_t flac_kmax(uint32_t bps) { return bps == 16 ? 14u : 30u; }
TH_HD uint32_t flac_param_bits(uint32_t bps) { return bps == 16 ? 4u : 5u; }  // coding method 0 / 1
TH_HD uint32_t flac_verbatim_bits(uint32_t n, uint32_t bps) { return 8u + n * bps; }
TH_HD uint32_t flac_slot_words(uint32_t n, uint32_t bps) { return (flac_verbatim_bits(n, bps) + 31u) / 32u; }
// a frame of n samples at most: the header, n_ch verbatim subframes, a byte of padding, CRC-16
TH_HD uint64_t flac_frame_bound(uint32_t n, uint32_t n_ch, uint32_t bps) {
    return FLAC_FRAME_HEADER_MAX + (uint64_t)n_ch * (1u + n * (bps / 8u)) + 1u + 2u;
}
TH_HD uint64_t flac_n_blocks(uint64_t n_frames) { return (n_frames + FLAC_BLOCK - 1) / FLAC_BLOCK; }
// 42 bytes, then every block's frame bound (the formula of th_flac_bound)
TH_HD uint64_t flac_stream_bound(uint64_t n_frames, uint32_t n_ch, uint32_t bps) {
    const uint64_t full = n_frames / FLAC_BLOCK;
    const uint32_t rest = (uint32_t)(n_frames % FLAC_BLOCK);
    return FLAC_STREAM_HEADER + full * flac_frame_bound(FLAC_BLOCK, n_ch, bps) + (rest ? flac_frame_bound(rest, n_ch, bps) : 0u);
}

// ---- CRC-8 (x^8 + x^2 + x + 1) and CRC-16 (x^16 + x^15 + x^2 + 1), both from 0, most significant bit first
TH_HD uint32_t flac_crc8_byte(uint32_t crc, uint32_t b) {
    crc ^= b;
    for (int i = 0; i < 8; i++) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xffu : (crc << 1) & 0xffu;
    return crc;
}
TH_HD uint32_t flac_crc16_byte(uint32_t crc, uint32_t b) {
    crc ^= b << 8;
    for (int i = 0; i < 8; i++) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x8005u) & 0xffffu : (crc << 1) & 0xffffu;
    return crc;
}
// entry i of the byte table (the CRC of the one byte i); with it a byte is one lookup
TH_HD uint32_t flac_crc16_entry(uint32_t i) { return flac_crc16_byte(0, i); }
TH_HD uint32_t flac_crc16_step(uint32_t crc, uint32_t b, const uint16_t *tab) { return ((crc << 8) & 0xffffu) ^ tab[(crc >> 8) ^ b]; }
// The CRC is linear: crc(A || B) = crc(A) x^(8 |B|) + crc(B) over GF(2) modulo the polynomial.  a b mod P:
TH_HD uint32_t flac_gf16_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) & 0xffffu : (r << 1);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
// crc x^(8 n_bytes): the CRC of a message followed by n_bytes zero bytes (n_bytes < 2^24; the loop's length does not depend on it)
TH_HD uint32_t flac_crc16_shift(uint32_t crc, uint32_t n_bytes) {
    uint32_t pw = 0x0100u;  // x^8
    for (int i = 0; i < 24; i++) {
        if ((n_bytes >> i) & 1u) crc = flac_gf16_mul(crc, pw);
        pw = flac_gf16_mul(pw, pw);
    }
    return crc;
}

// ---- the frame header
TH_HD uint32_t flac_rate_code(uint32_t sr) {
    switch (sr) {
        case 88200: return 1;
        case 176400: return 2;
        case 192000: return 3;
        case 8000: return 4;
        case 16000: return 5;
        case 22050: return 6;
        case 24000: return 7;
        case 32000: return 8;
        case 44100: return 9;
        case 48000: return 10;
        case 96000: return 11;
        default: break;
    }
    if (sr <= 65535u) return 13;                          // 16 bits of Hz
    if (sr % 10u == 0 && sr / 10u <= 65535u) return 14;   // 16 bits of tens of Hz
    return 0;                                             // as STREAMINFO says
}
TH_HD uint32_t flac_number_bytes(uint64_t v) {
    return v < 0x80u ? 1u : v < 0x800u ? 2u : v < 0x10000u ? 3u : v < 0x200000u ? 4u : v < 0x4000000u ? 5u : v < 0x80000000ull ? 6u : 7u;
}
// the coded channels of a block: its n_ch channels, or with TH_FLAC_STEREO the four of a 2-channel block (L, R, mid, side)
TH_HD uint32_t flac_units_per_block(uint32_t n_ch, uint32_t flags) { return (flags & TH_FLAC_STEREO) && n_ch == 2u ? 4u : n_ch; }
TH_HD uint32_t flac_frame_header_len(uint32_t sr, uint64_t frame_number, uint32_t n) {
    const uint32_t rc = flac_rate_code(sr);
    return 4u + flac_number_bytes(frame_number) + (n == FLAC_BLOCK ? 0u : n <= 256u ? 1u : 2u) + (rc == 13u || rc == 14u ? 2u : 0u) + 1u;
}
// sync .. CRC-8 into out (at most FLAC_FRAME_HEADER_MAX bytes); 1 <= n <= 65536, frame_number < 2^36.  Returns the length
// (assign: the four channel-assignment bits, n_ch - 1 for independent channels)
TH_HD uint32_t flac_frame_header_as(uint32_t sr, uint32_t assign, uint32_t bps, uint64_t frame_number, uint32_t n, uint8_t *out) {
    const uint32_t rc = flac_rate_code(sr);
    const uint32_t bc = n == FLAC_BLOCK ? 12u : n <= 256u ? 6u : 7u;
    uint32_t at = 0;
    out[at++] = 0xff;
    out[at++] = 0xf8;
    out[at++] = (uint8_t)((bc << 4) | rc);
    out[at++] = (uint8_t)((assign << 4) | ((bps == 16 ? 4u : 6u) << 1));
    const uint32_t nb = flac_number_bytes(frame_number);
    if (nb == 1) {
        out[at++] = (uint8_t)frame_number;
    } else {
        out[at++] = (uint8_t)((0xff00u >> nb) | (uint32_t)(frame_number >> (6u * (nb - 1u))));
        for (uint32_t j = 1; j < nb; j++) out[at++] = (uint8_t)(0x80u | ((uint32_t)(frame_number >> (6u * (nb - 1u - j))) & 0x3fu));
    }
    if (bc == 6u) {
        out[at++] = (uint8_t)(n - 1u);
    } else if (bc == 7u) {
        out[at++] = (uint8_t)((n - 1u) >> 8);
        out[at++] = (uint8_t)(n - 1u);
    }
    if (rc == 13u || rc == 14u) {
        const uint32_t v = rc == 13u ? sr : sr / 10u;
        out[at++] = (uint8_t)(v >> 8);
        out[at++] = (uint8_t)v;
    }
    uint32_t crc = 0;
    for (uint32_t j = 0; j < at; j++) crc = flac_crc8_byte(crc, out[j]);
    out[at++] = (uint8_t)crc;
    return at;
}

TH_HD uint32_t flac_frame_header(uint32_t sr, uint32_t n_ch, uint32_t bps, uint64_t frame_number, uint32_t n, uint8_t *out) {
    return flac_frame_header_as(sr, n_ch - 1u, bps, frame_number, n, out);
}
// A stereo frame's assignment from the bits of its four subframes L, R, M, S: the cheapest of independent (0001), left/side (1000),
// side/right (1001), mid/side (1010), the earlier one on ties.  u0, u1: which of the four is the frame's first and second subframe
struct FlacAssign {
    uint32_t code, u0, u1;
    uint64_t bits;
};
TH_HD FlacAssign flac_pick_assignment(uint32_t bl, uint32_t br, uint32_t bm, uint32_t bs) {
    FlacAssign a{1u, 0u, 1u, (uint64_t)bl + br};
    if ((uint64_t)bl + bs < a.bits) a = FlacAssign{8u, 0u, 3u, (uint64_t)bl + bs};
    if ((uint64_t)bs + br < a.bits) a = FlacAssign{9u, 3u, 1u, (uint64_t)bs + br};
    if ((uint64_t)bm + bs < a.bits) a = FlacAssign{10u, 2u, 3u, (uint64_t)bm + bs};
    return a;
}

// ---- the 42 bytes in front of the frames; min_frame / max_frame: the frames' actual sizes (0 0 for a stream without frames)
TH_HD void flac_stream_header(uint32_t sr, uint32_t n_ch, uint32_t bps, uint64_t n_frames, uint32_t min_frame, uint32_t max_frame,
                              uint8_t *out) {
    const uint8_t head[8] = {'f', 'L', 'a', 'C', 0x80, 0, 0, 34};  // the last metadata block, type 0, 34 bytes
    for (int i = 0; i < 8; i++) out[i] = head[i];
    out[8] = (uint8_t)(FLAC_BLOCK >> 8);
    out[9] = (uint8_t)FLAC_BLOCK;
    out[10] = (uint8_t)(FLAC_BLOCK >> 8);
    out[11] = (uint8_t)FLAC_BLOCK;
    out[12] = (uint8_t)(min_frame >> 16);
    out[13] = (uint8_t)(min_frame >> 8);
    out[14] = (uint8_t)min_frame;
    out[15] = (uint8_t)(max_frame >> 16);
    out[16] = (uint8_t)(max_frame >> 8);
    out[17] = (uint8_t)max_frame;
    const uint64_t x = ((uint64_t)sr << 44) | ((uint64_t)(n_ch - 1u) << 41) | ((uint64_t)(bps - 1u) << 36) | n_frames;
    for (int i = 0; i < 8; i++) out[18 + i] = (uint8_t)(x >> (56 - 8 * i));
    for (int i = 26; i < 42; i++) out[i] = 0;  // MD5: not computed
}

// ---- predictors and Rice rules
// the residual of fixed order o at sample i >= o (|e| < 2^28 for 24-bit samples)
TH_HD int32_t flac_residual(const int32_t *s, uint32_t i, uint32_t o) {
    switch (o) {
        case 0: return s[i];
        case 1: return s[i] - s[i - 1];
        case 2: return s[i] - 2 * s[i - 1] + s[i - 2];
        case 3: return s[i] - 3 * s[i - 1] + 3 * s[i - 2] - s[i - 3];
        default: return s[i] - 4 * s[i - 1] + 6 * s[i - 2] - 4 * s[i - 3] + s[i - 4];
    }
}
TH_HD uint32_t flac_zigzag(int32_t e) { return ((uint32_t)e << 1) ^ (uint32_t)(e >> 31); }
// the largest p <= 6 with 2^p | n and (n >> p) >= max(5, order + 1) (n >= 5, order < n; order <= 4: the fixed predictors' rule)
TH_HD uint32_t flac_part_order(uint32_t n, uint32_t order = 0) {
    const uint32_t least = order + 1u > FLAC_MIN_PART ? order + 1u : FLAC_MIN_PART;
    uint32_t p = 0;
    for (uint32_t q = 1; q <= FLAC_MAX_PART_ORDER; q++)
        if (p + 1 == q && (n & ((1u << q) - 1u)) == 0 && (n >> q) >= least) p = q;
    return p;
}
// The smallest k in 0 .. kmax that minimises S[k] + m (k + 1), S[k] = sum of (u >> k) over the partition's m residuals; *bits: that
// minimum (the residual bits of the partition, without its parameter)
TH_HD uint32_t flac_best_k(const unsigned long long *S, uint32_t m, uint32_t kmax, unsigned long long *bits) {
    uint32_t best = 0;
    unsigned long long bc = S[0] + m;
    for (uint32_t k = 1; k <= FLAC_MAX_K; k++) {
        if (k > kmax) break;
        const unsigned long long c = S[k] + (unsigned long long)m * (k + 1u);
        if (c < bc) {
            bc = c;
            best = k;
        }
    }
    *bits = bc;
    return best;
}

// ---- LPC (TH_FLAC_LPC).  Candidate c of a subframe: the fixed predictor of order c for c <= 4, else LPC of order c - 4
TH_HD bool flac_cand_is_lpc(uint32_t c) { return c > FLAC_MAX_ORDER; }
TH_HD uint32_t flac_cand_order(uint32_t c) { return c > FLAC_MAX_ORDER ? c - FLAC_MAX_ORDER : c; }
TH_HD uint32_t flac_lpc_precision(uint32_t file_bps) { return file_bps == 16 ? 12u : 14u; }
TH_HD uint32_t flac_lpc_max_order(uint32_t n) { return n < FLAC_MIN_PART ? 0u : n - 1u < FLAC_LPC_MAX ? n - 1u : FLAC_LPC_MAX; }
TH_HD uint32_t flac_bit_length(uint32_t v) { return v ? 32u - (uint32_t)__builtin_clz(v) : 0u; }
// the Welch window in 14 fractional bits, 0 <= w <= 2^14; the windowed sample at the block's level (amax: the largest |s| of the
// block): |x| < 2^22, so nine lags of 4096 products stay below 2^56
TH_HD uint32_t flac_lpc_window(uint32_t i, uint32_t n) {
    return (uint32_t)((((uint64_t)(2u * i + 1u) * (uint64_t)(2u * n - 2u * i - 1u)) << 14) / ((uint64_t)n * n));
}
TH_HD uint32_t flac_lpc_level_shift(uint32_t amax) {
    const uint32_t L = flac_bit_length(amax);
    return L > 8u ? L - 8u : 0u;
}
TH_HD int32_t flac_lpc_windowed(int32_t s, uint32_t w, uint32_t sh) { return (int32_t)(((long long)s * (long long)w) >> sh); }

TH_HD uint64_t flac_f64_bits(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return b;
}
TH_HD bool flac_f64_finite(double v) { return ((flac_f64_bits(v) >> 52) & 0x7ffu) != 0x7ffu; }
// Order m's coefficients a[0 .. m) to P-bit integers q and their shift; false: this order is no candidate.  e is the exponent frexp
// gives |a|'s maximum (from the bits; a subnormal's is smaller still and clamps to the same shift), shift = P - e - 1, at most 15;
// the rounding error of one coefficient is fed into the next
TH_HD bool flac_lpc_quantize(const double *a, uint32_t m, uint32_t P, int32_t *q, uint32_t *shift) {
    double cmax = 0.0;
    for (uint32_t j = 0; j < FLAC_LPC_MAX; j++) {
        if (j >= m) break;
        if (!flac_f64_finite(a[j])) return false;
        const double v = a[j] < 0.0 ? -a[j] : a[j];
        if (v > cmax) cmax = v;
    }
    if (!(cmax > 0.0)) return false;
    const int e = (int)((flac_f64_bits(cmax) >> 52) & 0x7ffu) - 1022;
    int sh = (int)P - e - 1;
    if (sh > 15) sh = 15;
    if (sh < 0) return false;
    const double scale = (double)(1u << sh), hi = (double)((1 << (P - 1u)) - 1), lo = -(double)(1 << (P - 1u));
    double fb = 0.0;
    for (uint32_t j = 0; j < FLAC_LPC_MAX; j++) {
        if (j >= m) break;
        fb = fb + a[j] * scale;
        double qd = __builtin_floor(fb + 0.5);
        qd = qd > hi ? hi : qd < lo ? lo : qd;
        q[j] = (int32_t)qd;
        fb = fb - qd;
    }
    *shift = (uint32_t)sh;
    return true;
}
// What one lane makes of the autocorrelation r[0 .. max_order]: per order m the quantised predictor, or no candidate
struct FlacLpcFit {
    int32_t q[FLAC_LPC_MAX][FLAC_LPC_MAX];  // q[m - 1][j - 1] multiplies s[i - j]
    uint32_t shift[FLAC_LPC_MAX];
    uint32_t ok;                            // bit m - 1: order m is a candidate
};
// Levinson-Durbin in f64, every operation in this order.  An order whose error E is not a finite number above 0 ends the recursion:
// it and all higher orders are no candidates
TH_HD void flac_lpc_fit(const long long *r, uint32_t max_order, uint32_t P, FlacLpcFit *fit) {
    fit->ok = 0;
    if (r[0] == 0) return;
    double a[FLAC_LPC_MAX], t[FLAC_LPC_MAX];
    for (uint32_t j = 0; j < FLAC_LPC_MAX; j++) a[j] = t[j] = 0.0;
    double E = (double)r[0];
#pragma unroll
    for (uint32_t m = 1; m <= FLAC_LPC_MAX; m++) {
        if (m > max_order) break;
        double acc = (double)r[m];
#pragma unroll
        for (uint32_t j = 1; j < FLAC_LPC_MAX; j++)
            if (j < m) acc = acc - a[j - 1] * (double)r[m - j];
        const double k = acc / E;
#pragma unroll
        for (uint32_t j = 1; j < FLAC_LPC_MAX; j++)
            if (j < m) t[j - 1] = a[j - 1] - k * a[m - j - 1];
#pragma unroll
        for (uint32_t j = 1; j < FLAC_LPC_MAX; j++)
            if (j < m) a[j - 1] = t[j - 1];
        a[m - 1] = k;
        E = E * (1.0 - k * k);
        if (!(E > 0.0) || !flac_f64_finite(E)) break;
        if (flac_lpc_quantize(a, m, P, fit->q[m - 1], &fit->shift[m - 1])) fit->ok |= 1u << (m - 1u);
    }
}
// the residual of LPC order m at sample i >= m, exact in 64 bits (|q| < 2^13, |s| < 2^25, eight products)
TH_HD long long flac_lpc_residual(const int32_t *s, uint32_t i, const int32_t *q, uint32_t m, uint32_t shift) {
    long long pred = 0;
#pragma unroll
    for (uint32_t j = 1; j <= FLAC_LPC_MAX; j++)
        if (j <= m) pred += (long long)q[j - 1] * (long long)s[i - j];
    return (long long)s[i] - (pred >> shift);
}
TH_HD bool flac_residual_fits(long long e) { return e >= -2147483647ll && e <= 2147483647ll; }
// the bits of an LPC subframe of order m in front of its partitions, without the 8 of the subframe header: warm-up, precision, shift,
// coefficients, coding method and partition order
TH_HD uint32_t flac_lpc_head_bits(uint32_t m, uint32_t unit_bps, uint32_t P) { return m * unit_bps + 4u + 5u + m * P + 6u; }

// ---- the bit writer.  A stream is 32-bit words, bit b of the stream is bit 31 - (b & 31) of word b >> 5, so a word's bytes go out
// most significant first.  The words are zero before the first write and every write ORs: writers need no order among themselves.
#if defined(__HIP_DEVICE_COMPILE__)
#define TH_FLAC_OR32(p, v) ((void)__hip_atomic_fetch_or((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#define TH_FLAC_ADD32(p, v) ((void)__hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#define TH_FLAC_ADD64(p, v) ((void)__hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#define TH_FLAC_MAX32(p, v) ((void)__hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#else
#define TH_FLAC_OR32(p, v) ((void)(*(p) |= (v)))
#define TH_FLAC_ADD32(p, v) ((void)(*(p) += (v)))
#define TH_FLAC_ADD64(p, v) ((void)(*(p) += (v)))
#define TH_FLAC_MAX32(p, v) ((void)(*(p) = *(p) < (v) ? (v) : *(p)))
#endif
// the low nbits (1 .. 32) of v at bit pos; nothing is written unless [pos, pos + nbits) lies inside the stream's limit bits
TH_HD void flac_put_bits(uint32_t *w, uint32_t limit, uint32_t pos, uint32_t nbits, uint32_t v) {
    if (nbits == 0 || nbits > 32u || pos > limit || limit - pos < nbits) return;
    if (nbits < 32u) v &= (1u << nbits) - 1u;
    const uint32_t sh = pos & 31u;
    const unsigned long long x = (unsigned long long)v << (64u - nbits - sh);
    const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
    if (hi) TH_FLAC_OR32(w + (pos >> 5), hi);
    if (lo) TH_FLAC_OR32(w + (pos >> 5) + 1, lo);  // (then the write's last bit lies in that word, which the stream has)
}
// 32 bits of a stream of len bits from bit off (off may be negative or beyond the end: zeros there)
TH_HD uint32_t flac_get_bits32(const uint32_t *w, uint32_t len, int64_t off) {
    if (off <= -32 || off >= (int64_t)len) return 0;
    const uint32_t nw = (len + 31u) >> 5;
    uint32_t v;
    if (off < 0) {
        v = w[0] >> (uint32_t)(-off);
    } else {
        const uint32_t wi = (uint32_t)(off >> 5), sh = (uint32_t)off & 31u;
        const uint32_t a = w[wi], b = wi + 1u < nw ? w[wi + 1u] : 0u;
        v = sh ? (a << sh) | (b >> (32u - sh)) : a;
    }
    // the bits behind the stream's end
    const int64_t end = (int64_t)len - off;  // valid bits of the window, from its top
    if (end < 32) v &= ~(0xffffffffu >> (uint32_t)end);
    return v;
}

}  // namespace th
