// flac_core.h — the arithmetic of the FLAC export (th_tm_export_flac, th_flac_encode_i32), written once for the host and for the
// device (kernels_flac.hip through flac_block.h): the fixed predictors, the zigzag, the Rice cost and argmin rules, the frame header,
// CRC-8 and CRC-16, and the big-endian bit writer.  Integers only; the definitions are those of include/thesia_amd.h ("FLAC export"),
// a subset of RFC 9639 with every choice fixed, so the bytes of a stream are a function of its samples.
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
TH_HD uint32_t flac_frame_header_len(uint32_t sr, uint64_t frame_number, uint32_t n) {
    const uint32_t rc = flac_rate_code(sr);
    return 4u + flac_number_bytes(frame_number) + (n == FLAC_BLOCK ? 0u : n <= 256u ? 1u : 2u) + (rc == 13u || rc == 14u ? 2u : 0u) + 1u;
}
// sync .. CRC-8 into out (at most FLAC_FRAME_HEADER_MAX bytes); 1 <= n <= 65536, frame_number < 2^36.  Returns the length
TH_HD uint32_t flac_frame_header(uint32_t sr, uint32_t n_ch, uint32_t bps, uint64_t frame_number, uint32_t n, uint8_t *out) {
    const uint32_t rc = flac_rate_code(sr);
    const uint32_t bc = n == FLAC_BLOCK ? 12u : n <= 256u ? 6u : 7u;
    uint32_t at = 0;
    out[at++] = 0xff;
    out[at++] = 0xf8;
    out[at++] = (uint8_t)((bc << 4) | rc);
    out[at++] = (uint8_t)(((n_ch - 1u) << 4) | ((bps == 16 ? 4u : 6u) << 1));
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
// the largest p <= 6 with 2^p | n and (n >> p) >= 5 (n >= 5)
TH_HD uint32_t flac_part_order(uint32_t n) {
    uint32_t p = 0;
    for (uint32_t q = 1; q <= FLAC_MAX_PART_ORDER; q++)
        if (p + 1 == q && (n & ((1u << q) - 1u)) == 0 && (n >> q) >= FLAC_MIN_PART) p = q;
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

// ---- the bit writer.  A stream is 32-bit words, bit b of the stream is bit 31 - (b & 31) of word b >> 5, so a word's bytes go out
// most significant first.  The words are zero before the first write and every write ORs: writers need no order among themselves.
#if defined(__HIP_DEVICE_COMPILE__)
#define TH_FLAC_OR32(p, v) ((void)__hip_atomic_fetch_or((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#define TH_FLAC_ADD32(p, v) ((void)__hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#define TH_FLAC_ADD64(p, v) ((void)__hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#else
#define TH_FLAC_OR32(p, v) ((void)(*(p) |= (v)))
#define TH_FLAC_ADD32(p, v) ((void)(*(p) += (v)))
#define TH_FLAC_ADD64(p, v) ((void)(*(p) += (v)))
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
