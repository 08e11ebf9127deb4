// emu_stft.cpp — CPU lane emulator of the wave STFT kernel (TEST SCAFFOLDING, never shipped):
// compiles thesia_amd/csrc/stft_wave.h with g++ and walks the 64 lanes sequentially through the
// same phase functions the gfx950 kernel runs, so the index arithmetic (Stockham passes, LDS
// swizzle, mirror exchange, split pass) can be checked against the oracle without a GPU.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../thesia_amd/csrc/stft_wave.h"
#include "../../thesia_amd/csrc/stft_wave_multi.h"
#include <type_traits>

#include "../../thesia_amd/csrc/stft_block.h"
#include "../../thesia_amd/csrc/mel_fuse.h"
#include "../../thesia_amd/csrc/host_math.h"  // bluestein_tables (host_math.cpp is compiled into the emulator)
#include "../../thesia_amd/csrc/stft_plan.h"  // the plan tables and the launch planner, as th_plan_create / th_calc_spec_batch_dev call them
#include "../../thesia_amd/csrc/reader_plan.h"  // the export and meter readers' planners, as export_run / meters_run call them (reader_plan.cpp is compiled in)

using namespace th;

template <int LOG2_NC>
static void emu_frame(const float *wav, uint32_t n_samples, uint32_t frame, const StftGeom &g, const cf32 *wtab,
                      const cf32 *tw, float *row) {
    using W = WaveFft<LOG2_NC>;
    constexpr int P = W::P, NC = W::NC;
    std::vector<cf32> slab(W::SLAB_LEN);
    static cf32 x[64][P], z[64][P];
    std::vector<cf32> t2(W::T2_LEN), t3(W::T3_LEN);
    const int64_t e0 = (int64_t)frame * g.hop - (int64_t)(g.win / 2) - (int64_t)g.pad_left;
    for (uint32_t t = 0; t < 256; t++) W::fill_tables(t, 256, tw, t2.data(), t3.data());
    // (a lane's column of the frame is W::lane_col(lane): the plane exchanges of n_fft = 2048 deal the columns out permuted)
    for (uint32_t l = 0; l < 64; l++) wave_fetch<P, 0>(W::lane_col(l), x[l], wav, e0);
    for (uint32_t l = 0; l < 64; l++) wave_window<P>(W::lane_col(l), z[l], x[l], wtab);
    for (uint32_t l = 0; l < 64; l++) W::pass1(l, z[l], slab.data());
    for (uint32_t l = 0; l < 64; l++) W::read1(l, z[l], slab.data());
    for (uint32_t l = 0; l < 64; l++) W::pass2(l, z[l], t2.data(), slab.data());
    if (W::PAIRED) {  // mirror-local last pass: no third exchange
        static cf32 za[64][W::NQ][W::R3], zb[64][W::NQ][W::R3];
        for (uint32_t l = 0; l < 64; l++) W::read2_paired(l, za[l], zb[l], slab.data());
        for (uint32_t l = 0; l < 64; l++) W::pass3_paired(l, za[l], zb[l], t3.data());
        std::vector<int> hits(NC + 1, 0);
        for (uint32_t l = 0; l < 64; l++)
            W::split_paired(l, za[l], zb[l], tw, [&](uint32_t kb, int kc, float p) {
                const uint32_t k = kb + (uint32_t)kc;
                row[k] = power_to_dB(p);
                hits[k]++;
            });
        for (int k = 0; k <= NC; k++)
            if (hits[k] != 1) row[k] = NAN;  // every bin must be emitted exactly once
        return;
    }
    if constexpr (W::SWAP8) {  // n_fft 1024: the wave's halves swap registers for the split pass (v_permlane32_swap on the GPU)
        static cf32 z256[64];
        typename W::Swap8Lane sl[64];
        for (uint32_t l = 0; l < 64; l++) sl[l] = W::swap8_lane(l);
        for (uint32_t l = 0; l < 64; l++) W::read2_sw(sl[l], z[l], slab.data());
        for (uint32_t l = 0; l < 64; l++) {
            cf32 w3[4];
            W::load_t3_sw(sl[l], w3, t3.data());
            W::pass3_sw(sl[l], z[l], w3, z256[l]);
        }
        // swap(a = z[i], b = z[7 - i]): lanes 32..63 of a <-> lanes 0..31 of b, lanes 0 and 32 masked out
        for (uint32_t l = 1; l < 32; l++)
            for (int i = 0; i < 4; i++) std::swap(z[32 + l][i % P], z[l][(7 - i) % P]);
        std::vector<int> hits(NC + 1, 0);
        for (uint32_t l = 0; l < 64; l++)
            W::split_sw(sl[l], z[l], z256[l], tw, [&](uint32_t kb, int kc, float p) {
                const uint32_t k = kb + (uint32_t)kc;
                row[k] = power_to_dB(p);
                hits[k]++;
            });
        for (int k = 0; k <= NC; k++)
            if (hits[k] != 1) row[k] = NAN;  // every bin must be emitted exactly once
    }
}

// The packed-f32 pipeline of the n_fft 2048 plan (WaveFft<10>::*_pk, stft_pk.h): the same phases on register pairs, with
// the pair-ordered split-twiddle table.  On the CPU the pair helpers are plain structs: this checks the pair bookkeeping
// (which point sits in which half of which pair after every level), the lane-0 selects and the table layout.
static void emu_frame_pk(const float *wav, uint32_t n_samples, uint32_t frame, const StftGeom &g, const cf32 *wtab,
                         const cf32 *tw, float *row) {
    using W = WaveFft<10>;
    constexpr int P = W::P, NC = W::NC;
    static_assert(W::PK, "packed pipeline");
    std::vector<cf32> slab(W::SLAB_LEN), t2(W::T2_LEN), t3(W::T3_LEN), stwp(W::STWP_LEN);
    static cf32 x[64][P], z[64][P];
    static v2f zp[64][16], zr[64][8], zi[64][8];
    const int64_t e0 = (int64_t)frame * g.hop - (int64_t)(g.win / 2) - (int64_t)g.pad_left;
    for (uint32_t t = 0; t < 256; t++) {
        W::fill_tables(t, 256, tw, t2.data(), t3.data());
        W::fill_stwp(t, 256, tw, stwp.data());
    }
    for (uint32_t l = 0; l < 64; l++) wave_fetch<P, 0>(W::lane_col(l), x[l], wav, e0);
    for (uint32_t l = 0; l < 64; l++) wave_window<P>(W::lane_col(l), z[l], x[l], wtab);
    for (uint32_t l = 0; l < 64; l++)
        for (int m = 0; m < P; m++) zp[l][m] = mk2(z[l][m].re, z[l][m].im);
    for (uint32_t l = 0; l < 64; l++) W::pass1_pk(l, zp[l], slab.data());
    for (uint32_t l = 0; l < 64; l++) W::read1_pk(l, zr[l], zi[l], slab.data());
    for (uint32_t l = 0; l < 64; l++) {
        v2f w2[W::NT2];
        W::load_t2_pk(l, w2, t2.data());
        W::pass2_pk(l, zr[l], zi[l], w2, slab.data());
    }
    static typename W::PkPairs za[64][W::NQ], zb[64][W::NQ];
    for (uint32_t l = 0; l < 64; l++) W::read2_paired_pk(W::pair_base(l), za[l], zb[l], slab.data());
    for (uint32_t l = 0; l < 64; l++) {
        v2f wa[W::NQ][W::NT3], wb[W::NQ][W::NT3];
        W::load_t3_paired_pk(W::pair_base(l), wa, wb, t3.data());
        W::pass3_paired_pk(za[l], zb[l], wa, wb);
    }
    std::vector<int> hits(NC + 1, 0);
    for (uint32_t l = 0; l < 64; l++) {
        v2f wsr[W::NQ][2], wsi[W::NQ][2];
        W::load_stw_paired_pk(l, wsr, wsi, stwp.data());
        W::split_paired_pk(l, za[l], zb[l], wsr, wsi, tw[NC / 2], [&](uint32_t kb, int kc, float p) {
            const uint32_t k = kb + (uint32_t)kc;
            row[k] = power_to_dB(p);
            hits[k]++;
        });
    }
    for (int k = 0; k <= NC; k++)
        if (hits[k] != 1) row[k] = NAN;  // every bin must be emitted exactly once
}

// One frame of the workgroup-per-frame plan (stft_block.h): the T threads run every phase one after the other, a phase
// boundary stands for the workgroup barrier.
template <int LOG2_NC>
static void emu_frame_block(const float *wav, uint32_t frame, const StftGeom &g, const cf32 *wtab, const cf32 *tw, float *row) {
    using B = BlockFft<LOG2_NC>;
    constexpr int T = B::T, NC = B::NC;
    std::vector<cf32> buf(B::BUF_LEN);
    static cf32 z[T][16];
    const int64_t e0 = (int64_t)frame * g.hop - (int64_t)(g.win / 2) - (int64_t)g.pad_left;
    for (uint32_t t = 0; t < (uint32_t)T; t++)
        for (int m = 0; m < 16; m++) {
            const uint32_t n = t + (uint32_t)T * m;
            z[t][m] = {wav[e0 + 2 * n] * wtab[n].re, wav[e0 + 2 * n + 1] * wtab[n].im};
        }
    // an exchange: every thread stores, (barrier), every thread reads; planar plans (n_fft 65536) run it per part
    auto exchange = [&](auto store, auto read) {
        if constexpr (B::PLANAR) {
            for (uint32_t t = 0; t < (uint32_t)T; t++) store(t, std::integral_constant<int, 0>{});
            for (uint32_t t = 0; t < (uint32_t)T; t++) read(t, std::integral_constant<int, 0>{});
            for (uint32_t t = 0; t < (uint32_t)T; t++) store(t, std::integral_constant<int, 1>{});
            for (uint32_t t = 0; t < (uint32_t)T; t++) read(t, std::integral_constant<int, 1>{});
        } else {
            for (uint32_t t = 0; t < (uint32_t)T; t++) store(t, std::integral_constant<int, -1>{});
            for (uint32_t t = 0; t < (uint32_t)T; t++) read(t, std::integral_constant<int, -1>{});
        }
    };
    for (uint32_t t = 0; t < (uint32_t)T; t++) B::pass_first_compute(z[t]);
    exchange([&](uint32_t t, auto part) { B::template pass_first_store<decltype(part)::value>(t, z[t], buf.data()); },
             [&](uint32_t t, auto part) { B::template read_in<B::FIRST_LAYOUT, decltype(part)::value>(t, z[t], buf.data()); });
    if (B::R2_FIRST) {
        for (uint32_t t = 0; t < (uint32_t)T; t++) {
            cf32 w[B::NTW];
            B::template load_tw<B::NS_A>(t, w, tw);
            B::template pass_mid_compute<B::NS_A>(z[t], w);
        }
        exchange([&](uint32_t t, auto part) { B::template pass_mid_store<B::NS_A, decltype(part)::value>(t, z[t], buf.data()); },
                 [&](uint32_t t, auto part) { B::template read_in<B::NS_A, decltype(part)::value>(t, z[t], buf.data()); });
    }
    for (uint32_t t = 0; t < (uint32_t)T; t++) {
        cf32 w[B::NTW];
        B::template load_tw<B::NS_B>(t, w, tw);
        B::template pass_mid_compute<B::NS_B>(z[t], w);
    }
    exchange([&](uint32_t t, auto part) { B::template pass_mid_store<B::NS_B, decltype(part)::value>(t, z[t], buf.data()); },
             [&](uint32_t t, auto part) { B::template read_in<B::NS_B, decltype(part)::value>(t, z[t], buf.data()); });
    for (uint32_t t = 0; t < (uint32_t)T; t++) {
        cf32 w[B::NTW];
        B::template load_tw<B::NS_C>(t, w, tw);
        B::pass_last(z[t], w);
    }
    static cf32 zm[T][8];
    exchange([&](uint32_t t, auto part) { B::template write_z<decltype(part)::value>(t, z[t], buf.data()); },
             [&](uint32_t t, auto part) { B::template split_read<decltype(part)::value>(t, buf.data(), zm[t]); });
    std::vector<int> hits(NC + 1, 0);
    for (uint32_t t = 0; t < (uint32_t)T; t++)
        B::split_compute(t, z[t], zm[t], tw[t], [&](uint32_t k, float p) {
            row[k] = power_to_dB(p);
            hits[k]++;
        });
    for (int k = 0; k <= NC; k++)
        if (hits[k] != 1) row[k] = NAN;  // every bin exactly once
}

// G frames of one wave of the multi-frame plan (stft_wave_multi.h): group g of the lanes computes frame frames[g]
template <int LOG2_NC>
static void emu_frames_multi(const float *wav, const uint32_t *frames, const StftGeom &g, const cf32 *wtab, const cf32 *tw,
                             float *const *rows) {
    using W = WaveFftM<LOG2_NC>;
    constexpr int P = W::P, NC = W::NC;
    std::vector<cf32> slab(W::SLAB_LEN);
    static cf32 x[64][P], z[64][P];
    std::vector<cf32> t2(W::T2_LEN), t3(W::T3_LEN + 1);
    for (uint32_t t = 0; t < 256; t++) W::fill_tables(t, 256, tw, t2.data(), t3.data());
    for (uint32_t l = 0; l < 64; l++) {
        const int64_t e0 = (int64_t)frames[W::grp(l)] * g.hop - (int64_t)(g.win / 2) - (int64_t)g.pad_left;
        // slot m of a lane = complex point col + L m of its frame
        for (int m = 0; m < P; m++) {
            const uint32_t n = W::lane_col(l) + (uint32_t)W::L * m;
            x[l][m] = {wav[e0 + 2 * n], wav[e0 + 2 * n + 1]};
            const cf32 w = wtab[n];
            z[l][m] = {x[l][m].re * w.re, x[l][m].im * w.im};
        }
    }
    for (uint32_t l = 0; l < 64; l++) W::pass1(l, z[l], slab.data());
    for (uint32_t l = 0; l < 64; l++) W::read1(l, z[l], slab.data());
    {
        static cf32 w2[64][W::NT2];
        for (uint32_t l = 0; l < 64; l++) W::load_t2(l, w2[l], t2.data());
        for (uint32_t l = 0; l < 64; l++) W::pass2_w(l, z[l], w2[l], slab.data());
    }
    static cf32 za[64][W::NQ][W::R3], zb[64][W::NQ][W::R3];
    for (uint32_t l = 0; l < 64; l++) W::read2_paired(l, za[l], zb[l], slab.data());
    for (uint32_t l = 0; l < 64; l++) {
        cf32 wa[W::NW3], wb[W::NW3];
        W::load_t3_paired(l, wa, wb, t3.data());
        W::pass3_paired_w(za[l], zb[l], wa, wb);
    }
    std::vector<int> hits((size_t)W::G * (NC + 1), 0);
    for (uint32_t l = 0; l < 64; l++) {
        cf32 ws[W::NQ][W::R3];
        W::load_stw_paired(l, ws, tw);
        const uint32_t gi = W::grp(l);
        W::split_paired_w(l, za[l], zb[l], ws, tw[NC / 2], [&](uint32_t kb, int kc, float p) {
            const uint32_t k = kb + (uint32_t)kc;
            rows[gi][k] = power_to_dB(p);
            hits[gi * (NC + 1) + k]++;
        });
    }
    for (int gi = 0; gi < W::G; gi++)
        for (int k = 0; k <= NC; k++)
            if (hits[gi * (NC + 1) + k] != 1) rows[gi][k] = NAN;  // every bin exactly once per frame
}

// the multi-frame plan (n_fft = 512, 1024): out as emu_stft_wave
extern "C" __attribute__((visibility("default"))) int emu_stft_wave_multi(const float *wav, uint32_t n_samples, uint32_t win,
                                                                           uint32_t hop, uint32_t n_fft, const float *window,
                                                                           uint32_t n_frames, float *out) {
    if (n_fft != 512 && n_fft != 1024) return -1;
    StftGeom g{};
    g.hop = hop;
    g.win = win;
    g.n_fft = n_fft;
    g.pad_left = (n_fft - win) / 2;
    g.nc = n_fft / 2;
    g.n_freq = n_fft / 2 + 1;
    g.height = g.n_freq;
    const std::vector<cf32> tw = build_twiddles(n_fft), wtab = build_wave_window(window, win, n_fft, 0).wtab;  // the plan's own tables
    std::vector<uint32_t> interior;
    for (uint32_t f = 0; f < n_frames; f++) {
        const int64_t e0 = (int64_t)f * hop - (int64_t)(win / 2) - (int64_t)g.pad_left;
        if (e0 < 0 || e0 + (int64_t)n_fft > (int64_t)n_samples)
            for (uint32_t k = 0; k < g.n_freq; k++) out[(size_t)f * g.n_freq + k] = NAN;
        else interior.push_back(f);
    }
    const uint32_t G = 1024 / g.nc;
    std::vector<float> scratch(g.n_freq);
    for (size_t i = 0; i < interior.size(); i += G) {
        uint32_t fr[4];
        float *rows[4];
        for (uint32_t k = 0; k < G; k++) {
            const bool valid = i + k < interior.size();
            fr[k] = interior[valid ? i + k : interior.size() - 1];  // the kernel clamps: a duplicate frame, computed again
            rows[k] = valid ? out + (size_t)fr[k] * g.n_freq : scratch.data();
        }
        if (n_fft == 1024) emu_frames_multi<9>(wav, fr, g, wtab.data(), tw.data(), rows);
        else emu_frames_multi<8>(wav, fr, g, wtab.data(), tw.data(), rows);
    }
    return 0;
}

// out: n_frames x (n_fft/2+1).  window: normalised window (len win).  Returns 0 on success.
static int emu_stft_wave_impl(const float *wav, uint32_t n_samples, uint32_t win, uint32_t hop, uint32_t n_fft,
                              const float *window, uint32_t n_frames, float *out, bool packed);
extern "C" __attribute__((visibility("default"))) int emu_stft_wave(const float *wav, uint32_t n_samples,
                                                                     uint32_t win, uint32_t hop, uint32_t n_fft,
                                                                     const float *window, uint32_t n_frames,
                                                                     float *out) {
    return emu_stft_wave_impl(wav, n_samples, win, hop, n_fft, window, n_frames, out, false);
}
// the packed-f32 pipeline (n_fft 2048 only)
extern "C" __attribute__((visibility("default"))) int emu_stft_wave_pk(const float *wav, uint32_t n_samples,
                                                                        uint32_t win, uint32_t hop, uint32_t n_fft,
                                                                        const float *window, uint32_t n_frames,
                                                                        float *out) {
    if (n_fft != 2048) return -1;
    return emu_stft_wave_impl(wav, n_samples, win, hop, n_fft, window, n_frames, out, true);
}
static int emu_stft_wave_impl(const float *wav, uint32_t n_samples, uint32_t win, uint32_t hop, uint32_t n_fft,
                              const float *window, uint32_t n_frames, float *out, bool packed) {
    StftGeom g{};
    g.hop = hop;
    g.win = win;
    g.n_fft = n_fft;
    g.pad_left = (n_fft - win) / 2;
    g.nc = n_fft / 2;
    g.n_freq = n_fft / 2 + 1;
    g.height = g.n_freq;
    const std::vector<cf32> tw = build_twiddles(n_fft), wtab = build_wave_window(window, win, n_fft, 0).wtab;  // the plan's own tables
    for (uint32_t f = 0; f < n_frames; f++) {
        float *row = out + (size_t)f * g.n_freq;
        const int64_t e0 = (int64_t)f * hop - (int64_t)(win / 2) - (int64_t)g.pad_left;
        if (e0 < 0 || e0 + (int64_t)n_fft > (int64_t)n_samples) {  // boundary frame: not the wave kernel's job
            for (uint32_t k = 0; k < g.n_freq; k++) row[k] = NAN;
            continue;
        }
        switch (n_fft) {
            case 1024: emu_frame<9>(wav, n_samples, f, g, wtab.data(), tw.data(), row); break;
            case 2048:
                if (packed) emu_frame_pk(wav, n_samples, f, g, wtab.data(), tw.data(), row);
                else emu_frame<10>(wav, n_samples, f, g, wtab.data(), tw.data(), row);
                break;
            case 4096: emu_frame<11>(wav, n_samples, f, g, wtab.data(), tw.data(), row); break;
            case 8192: emu_frame_block<12>(wav, f, g, wtab.data(), tw.data(), row); break;
            case 16384: emu_frame_block<13>(wav, f, g, wtab.data(), tw.data(), row); break;
            case 32768: emu_frame_block<14>(wav, f, g, wtab.data(), tw.data(), row); break;
            case 65536: emu_frame_block<15>(wav, f, g, wtab.data(), tw.data(), row); break;
            default: return -1;
        }
    }
    return 0;
}

// Check of the quotient the quantise kernel uses (kernels_image.hip: quantise): q0 = a*r, e = fma(-q0, b, a),
// q = fma(e, r, q0) with r = RN(1/b) against the IEEE quotient a / b.  Returns the number of mismatches (signed
// zeros compare equal).  fmaf is the correctly rounded C library / hardware operation.
extern "C" __attribute__((visibility("default"))) uint64_t emu_fma_div_mismatches(const float *a, uint64_t n, float b) {
    const float r = 1.0f / b;
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; i++) {
        const float want = a[i] / b;
        const float q0 = a[i] * r;
        const float e = std::fmaf(-q0, b, a[i]);
        const float q = std::fmaf(e, r, q0);
        if (std::memcmp(&q, &want, 4) != 0 && !(q == 0.0f && want == 0.0f)) bad++;
    }
    return bad;
}

// Fused mel epilogue (mel_fuse.h tables + stft_wave.h lane functions) on one amplitude row: out[m] = the filter outputs
// (linear, before dB).  info[0..2] = pieces, slots, groups.  Returns 0, or 1 when the filterbank is not fusable.
extern "C" __attribute__((visibility("default"))) int emu_mel_fuse(const float *amp, const float *fb, uint32_t n_freq,
                                                                    uint32_t n_mel, uint32_t max_pieces, float *out,
                                                                    uint32_t *info) {
    const MelFuseHost h = build_mel_fuse(fb, n_freq, n_mel, max_pieces);
    if (!h.ok) return 1;
    info[0] = h.n_pieces;
    info[1] = h.n_slots;
    info[2] = h.n_groups;
    if (h.words.size() != mel_fuse_words(h.n_slots, h.n_groups)) return -1;
    const MelFuseTab t = mel_fuse_view(h.words.data(), h.n_slots, h.n_groups);
    std::vector<cf32> prf(64 * (size_t)h.n_slots);
    for (uint32_t m = 0; m < n_mel; m++) out[m] = NAN;
    for (uint32_t l = 0; l < 64; l++) mel_pieces(l, amp, prf.data(), t);
    for (uint32_t l = 0; l < 64; l++)
        mel_gather(l, prf.data(), t, [&](uint32_t m, float v) {
            if (m < n_mel) out[m] = v;
        });
    return 0;
}

// Frame pairs (mel_banded_pair, round 5): two amplitude rows RB floats apart, one pass over the paired table; out_a / out_b[m] and
// (every lane's result, also those past the last mel) the extremes over all lanes in mm[0..3] = min a, max a, min b, max b — the
// kernel folds every lane into its min / max because lanes past the last mel repeat the last filter.  reach = MelBandHost::reach.
extern "C" __attribute__((visibility("default"))) int emu_mel_band_pair(const float *amp_a, const float *amp_b, const float *fb, uint32_t n_freq,
                                                                         uint32_t n_mel, float *out_a, float *out_b, float *mm, uint32_t *reach) {
    constexpr int RB = 1092;
    const MelBandHost h = build_mel_band(fb, n_freq, n_mel, 1u << 16, true, true);
    if (!h.ok) return 1;
    *reach = h.reach;
    if (n_freq > RB - 64 || h.reach > n_freq + 59) return 2;
    std::vector<float> a(2 * RB + 64, NAN);  // (NaN wherever the kernel guarantees nothing)
    for (uint32_t k = 0; k < n_freq; k++) {
        a[k] = amp_a[k];
        a[RB + k] = amp_b[k];
    }
    for (uint32_t k = 0; k < 64; k++) a[n_freq + k] = 0.0f;   // the zeros wave_frame writes behind the rows
    for (uint32_t k = 0; k < 59; k++) a[RB + n_freq + k] = 0.0f;
    uint32_t off[8] = {0, 0, 0, 0, 0, 0, 0, 0}, nt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t g = 0; g < h.n_groups; g++) {
        off[g] = h.words[2 * g];
        nt[g] = h.words[2 * g + 1];
    }
    mm[0] = mm[2] = INFINITY;
    mm[1] = mm[3] = -INFINITY;
    for (uint32_t l = 0; l < 64; l++)
        mel_banded_pair<RB>(
            l, a.data(), h.words.data(), h.n_groups, off, nt,
            [&](uint32_t m, float v) {
                mm[0] = std::fmin(mm[0], v);
                mm[1] = std::fmax(mm[1], v);
                if (m < n_mel) out_a[m] = v;
            },
            [&](uint32_t m, float v) {
                mm[2] = std::fmin(mm[2], v);
                mm[3] = std::fmax(mm[3], v);
                if (m < n_mel) out_b[m] = v;
            });
    return 0;
}

// The same product as banded sums, lane = mel (build_mel_band + mel_banded): out[m] = the filter outputs (linear).
// layout: 0 = first bins as the filters start, 1 = spread over the LDS banks, 2 = the paired layout (even first bins, weights
// in quads).  info[0..4] = table words, groups, widest group's taps, all groups' taps, LDS cycles of one frame's amplitude reads
// by the bank rule (mel_fuse.h).  amp must be followed by 128 readable zeros (the kernel zeroes them).
extern "C" __attribute__((visibility("default"))) int emu_mel_band(const float *amp, const float *fb, uint32_t n_freq,
                                                                    uint32_t n_mel, uint32_t max_words, uint32_t layout, float *out,
                                                                    uint32_t *info) {
    const MelBandHost h = build_mel_band(fb, n_freq, n_mel, max_words, layout >= 1, layout == 2);
    if (!h.ok) return 1;
    info[0] = (uint32_t)h.words.size();
    info[1] = h.n_groups;
    info[2] = h.max_taps;
    info[3] = info[4] = 0;
    std::vector<float> a(n_freq + MEL_BAND_MAX_TAPS, 0.0f);
    std::memcpy(a.data(), amp, n_freq * sizeof(float));
    for (uint32_t m = 0; m < n_mel; m++) out[m] = NAN;
    uint32_t off[8] = {0, 0, 0, 0, 0, 0, 0, 0}, nt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t g = 0; g < h.n_groups; g++) {
        off[g] = h.words[2 * g];
        nt[g] = h.words[2 * g + 1];
        info[3] += nt[g];
        uint32_t first[64];
        for (uint32_t l = 0; l < 64; l++) {
            first[l] = h.words[off[g] + l];
            if (layout == 2) {
                if (first[l] & 1u) return 2;  // 8-byte reads need even first bins
                first[l] /= 2;
            }
        }
        const uint32_t cyc = mel_band_half_cycles(first, 32) + mel_band_half_cycles(first + 32, 32);
        info[4] += layout == 2 ? nt[g] / 2 * cyc : nt[g] * cyc;
    }
    for (uint32_t l = 0; l < 64; l++) {
        auto emit = [&](uint32_t m, float v) {
            if (m < n_mel) out[m] = v;
        };
        if (layout == 2) mel_banded<true>(l, a.data(), h.words.data(), h.n_groups, off, nt, emit);
        else mel_banded<false>(l, a.data(), h.words.data(), h.n_groups, off, nt, emit);
    }
    return 0;
}

// Moment form of the mel filterbank (round 6: build_mel_moments + mel_mom_lane / mel_mom_w_lane / mel_mom_combine, lane = segment):
// out[m] = the filter outputs (linear).  amp_slab: the amplitude row followed by whatever the slab holds behind it (the caller
// passes NaN there: the masks must keep it out).  info[0..5] = table words, groups, all groups' taps, widest group's taps, reach,
// groups in the W form; dev[0..1] = MelMomHost::max_dev, max_amp.  Returns 0, 1 when the filterbank has no moment form.
extern "C" __attribute__((visibility("default"))) int emu_mel_moments(const float *amp_slab, uint32_t slab_len, const float *fb, const float *lin,
                                                                       const float *mf, uint32_t n_freq, uint32_t n_mel, uint32_t spread, float *out,
                                                                       uint32_t *info, double *dev) {
    const MelMomHost h = build_mel_moments(fb, lin, mf, n_freq, n_mel, slab_len, spread != 0);
    dev[0] = h.max_dev;
    dev[1] = h.max_amp;
    if (!h.ok) return 1;
    info[0] = (uint32_t)h.words.size();
    info[1] = h.n_groups;
    info[2] = h.taps;
    info[3] = h.max_taps;
    info[4] = h.reach;
    info[5] = h.w_groups;
    dev[0] = h.max_dev;
    dev[1] = h.max_amp;
    if (h.words[0] != h.n_groups || h.reach > slab_len) return -1;
    for (uint32_t m = 0; m < n_mel; m++) out[m] = NAN;
    float carry = 0.0f;  // F of lane 0 of the group above (the kernel walks the groups downwards)
    for (uint32_t g = h.n_groups; g-- != 0;) {
        const uint32_t nw = h.words[MEL_MOM_HDR0 + 2 * g], n = nw & 0xffffu, off = h.words[MEL_MOM_HDR0 + 1 + 2 * g];
        const bool wform = (nw & MEL_MOM_FORM_W) != 0;
        if (off % 4 != 0 || (wform ? (n < 1 || n > 2) : n % MEL_MOM_UNROLL != 0)) return -2;
        const uint64_t *masks = reinterpret_cast<const uint64_t *>(h.words.data() + off + 256);
        MelMomLane s[64];
        for (uint32_t l = 0; l < 64; l++) {
            float prm[3], w1[2];
            std::memcpy(prm, &h.words[off + 4 * l + 1], 12);
            std::memcpy(w1, &h.words[off + 256 + 2 * l], 8);
            s[l] = wform ? mel_mom_w_lane(amp_slab, h.words[off + 4 * l], n, prm[0], prm[1], w1[0], w1[1])
                         : mel_mom_lane_any(l, amp_slab, h.words[off + 4 * l], prm[0], prm[1], masks, n);
        }
        if (!wform) {  // the window words say what the masks say: the lockstep walk of the workgroup-per-frame kernels, bit for bit
            const uint32_t *win = h.words.data() + off + 256 + mel_mom_mask_words(n);
            uint32_t n_run = n;  // (the widest M group of the batch of MEL_MOM_BATCH groups this one is walked with)
            for (uint32_t gg = g / MEL_MOM_BATCH * MEL_MOM_BATCH; gg < std::min(h.n_groups, (g / MEL_MOM_BATCH + 1) * MEL_MOM_BATCH); gg++) {
                const uint32_t nw2 = h.words[MEL_MOM_HDR0 + 2 * gg];
                if (!(nw2 & MEL_MOM_FORM_W)) n_run = std::max(n_run, nw2 & 0xffffu);
            }
            for (uint32_t l = 0; l < 64; l++) {
                float prm[2];
                std::memcpy(prm, &h.words[off + 4 * l + 1], 8);
                const uint32_t first = h.words[off + 4 * l];
                // (the wave kernel's slab ends closer behind the row than a workgroup's exchange buffer)
                const MelMomLane w = mel_mom_lane_win(amp_slab, first, prm[0], prm[1], win[l], first + n_run <= slab_len ? n_run : n);
                if (std::memcmp(&w, &s[l], sizeof w) != 0) return -4;
            }
        }
        for (uint32_t l = 0; l < 64; l++) {
            float inv_d;
            std::memcpy(&inv_d, &h.words[off + 4 * l + 3], 4);
            const float v = mel_mom_combine(inv_d, s[l].R, l == 63 ? carry : s[l + 1].F);
            const uint32_t m = 64 * g + l;
            if (m < n_mel) out[m] = v;
            else if (v != 0.0f) return -3;  // lanes past the last mel hold 1 / d = 0
        }
        carry = s[0].F;
    }
    // The workgroup-per-frame kernels' lane table (made without spreading: a lane's window starts at its first bin): walked as
    // mel_moments_range_lockstep walks it — batches of MEL_MOM_BATCH groups counted from 0, every M group of a batch over the taps
    // of the widest — the same numbers bit for bit.
    if (spread == 0) {
        const std::vector<uint32_t> lt = build_mel_mom_lanes(h);
        if (lt.size() != MEL_LANE_BLK0 + (size_t)MEL_LANE_STRIDE * (h.n_groups + MEL_MOM_BATCH)) return -6;
        for (uint32_t i = 0; i < MEL_LANE_BLK0; i++)
            if (lt[i] != h.words[i]) return -6;
        float carry2 = 0.0f;
        for (uint32_t g = h.n_groups; g-- != 0;) {
            const uint32_t *blk = &lt[MEL_LANE_BLK0 + (size_t)MEL_LANE_STRIDE * g];
            const uint32_t nw = blk[256 + 2], n = nw & 0xffffu;
            uint32_t n_run = 0;
            for (uint32_t gg = g / MEL_MOM_BATCH * MEL_MOM_BATCH; gg < std::min(h.n_groups, (g / MEL_MOM_BATCH + 1) * MEL_MOM_BATCH); gg++) {
                const uint32_t nw2 = lt[MEL_LANE_BLK0 + (size_t)MEL_LANE_STRIDE * gg + 256 + 2];
                if (!(nw2 & MEL_MOM_FORM_W)) n_run = std::max(n_run, nw2 & 0xffffu);
            }
            MelMomLane s[64];
            for (uint32_t l = 0; l < 64; l++) {
                if (blk[256 + 4 * l + 2] != nw) return -7;
                float p[4], q[2];
                std::memcpy(p, &blk[4 * l], 16);
                std::memcpy(q, &blk[256 + 4 * l], 8);
                const uint32_t first = blk[4 * l], win = blk[256 + 4 * l];
                if (nw & MEL_MOM_FORM_W) {
                    s[l] = mel_mom_w_lane(amp_slab, first, n, p[1], p[2], q[0], q[1]);
                } else {
                    if ((win & 0xffffu) != 0) return -7;
                    s[l] = mel_mom_lane_win(amp_slab, first, p[1], p[2], win, first + n_run <= slab_len ? n_run : n);
                }
            }
            for (uint32_t l = 0; l < 64; l++) {
                float inv_d;
                std::memcpy(&inv_d, &blk[4 * l + 3], 4);
                const float v = mel_mom_combine(inv_d, s[l].R, l == 63 ? carry2 : s[l + 1].F);
                const uint32_t m = 64 * g + l;
                if (m < n_mel && std::memcmp(&v, &out[m], 4) != 0) return -8;
            }
            carry2 = s[0].F;
        }
        // the waves' ranges: ascending, from 0 to the last group
        if (lt[3] == 1) {
            auto byte = [&](uint32_t b) { return (lt[b / 4] >> (8 * (b % 4))) & 255u; };
            for (uint32_t pass = 0; pass < 2; pass++) {
                const uint32_t b0 = pass ? MEL_MOM_SPLIT4_BYTE : MEL_MOM_SPLIT8_BYTE, nw = pass ? 4 : 8;
                if (byte(b0) != 0 || byte(b0 + nw) != h.n_groups) return -9;
                for (uint32_t w = 0; w < nw; w++)
                    if (byte(b0 + w) > byte(b0 + w + 1)) return -9;
            }
        } else if (h.n_groups <= 255) {
            return -9;
        }
    }
    return 0;
}

// The chirp-z plan (an odd factor of n_fft above 63; stft_bluestein_kernel): the kernel's phases (stft_core.h) run by one
// "thread" over the tables the plan uploads (bluestein_tables, host_math.cpp).  Every frame incl. the reflected boundary
// frames; out[f][k] = amplitude (not dB).  Returns M.
extern "C" __attribute__((visibility("default"))) int emu_stft_bluestein(const float *wav, uint32_t n_samples, uint32_t win, uint32_t hop,
                                                                          uint32_t n_fft, const float *window, uint32_t n_frames, float *out) {
    if (n_fft < 2 || n_fft % 2) return -1;
    StftGeom g{};
    g.hop = hop;
    g.win = win;
    g.n_fft = n_fft;
    g.pad_left = (n_fft - win) / 2;
    g.nc = n_fft / 2;
    g.n_freq = n_fft / 2 + 1;
    g.height = g.n_freq;
    uint32_t M = 1;
    while (M < 2 * g.nc - 1) M <<= 1;
    const BluesteinTables bt = bluestein_tables(n_fft, M);
    if (bt.chirp.size() != 2 * (size_t)g.nc || bt.bhat.size() != 2 * (size_t)M || bt.tws.size() != 2 * (size_t)(g.nc / 2 + 1)) return -2;
    const cf64 *chirp = reinterpret_cast<const cf64 *>(bt.chirp.data()), *bhat = reinterpret_cast<const cf64 *>(bt.bhat.data());
    const cf64 *twm = reinterpret_cast<const cf64 *>(bt.twm.data()), *tws = reinterpret_cast<const cf64 *>(bt.tws.data());
    std::vector<cf64> a(M), b(M);
    for (uint32_t f = 0; f < n_frames; f++) {
        const int64_t s0 = (int64_t)f * hop - (int64_t)(win / 2);
        bluestein_load(0, 1, g, M, wav, n_samples, s0, window, chirp, a.data());
        cf64 *in = a.data(), *o = b.data();
        for (int pass = 0; pass < 2; pass++) {
            for (uint32_t Ns = 1; Ns < M; Ns <<= 1) {
                bluestein_pass(0, 1, M, Ns, twm, in, o);
                std::swap(in, o);
            }
            if (pass == 0) bluestein_product(0, 1, M, bhat, in);
        }
        bluestein_unchirp(0, 1, g, M, chirp, in, o);
        bluestein_split(0, 1, g, tws, o, out + (size_t)f * g.n_freq);
    }
    return (int)M;
}


// ---- the plan's host tables and the launch planner (stft_plan.h), for tests/test_plan_host.py.  A call builds the product's
// structures and keeps them as byte blobs behind a handle; emu_blob copies one out (returns its size; copies when cap suffices).
struct EmuBlobs {
    std::vector<std::vector<unsigned char>> b;
    template <class T>
    void add(const std::vector<T> &v) {
        const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
        b.emplace_back(p, p + v.size() * sizeof(T));
    }
};
extern "C" __attribute__((visibility("default"))) uint64_t emu_blob(const void *h, uint32_t which, void *out, uint64_t cap) {
    const EmuBlobs *e = static_cast<const EmuBlobs *>(h);
    if (!e || which >= e->b.size()) return ~0ull;
    const std::vector<unsigned char> &v = e->b[which];
    if (out && cap >= v.size() && !v.empty()) std::memcpy(out, v.data(), v.size());
    return v.size();
}
extern "C" __attribute__((visibility("default"))) void emu_blob_free(void *h) { delete static_cast<EmuBlobs *>(h); }

// plan_stft_launch on channels of n_samples[i] samples (frame counts as th_stft_n_frames gives them; dense spec rows).
// route: {main, mel_fused, mel_second, phase_mode, waves, tail_guard, edges_in_wave, block_plan, sweep} (StftRoute's values).
// Blobs (u64 unless said): 0 {err, frames_per_tile, phased, sweep, tiles, edge_tiles, mel_tiles, amp_rows, all_in_wave, edge
// frames_per_tile}; 1 jobs and 2 edge jobs, rows of {n_samples, n_frames, f_begin, f_end, mm_index, edge}; 3 tile_start (u32);
// 4 edge_start (u32); 5 chunk_tab (u32); 6 mel jobs, rows of {f_begin, f_end, mm_index}; 7 mel_start (u32); 8 amp_row0;
// 9 post jobs, rows of {t0, t1, mm_index}
extern "C" __attribute__((visibility("default"))) void *emu_plan_launch(uint32_t win, uint32_t hop, uint32_t n_fft, uint32_t n_mel, const int32_t *route,
                                                                        uint32_t n_cu, int32_t wave_chunk, const uint64_t *n_samples, uint64_t n_chan) {
    StftGeom g = stft_geom(win, hop, n_fft);
    if (n_mel) g.n_mel = g.height = n_mel;
    StftRoute r;
    r.main = (StftRoute::Main)route[0];
    r.mel_fused = (StftRoute::MelFused)route[1];
    r.mel_second = (StftRoute::MelSecond)route[2];
    r.phase_mode = route[3];
    r.waves = route[4];
    r.tail_guard = (uint32_t)route[5];
    r.edges_in_wave = route[6] != 0;
    r.block_plan = route[7] != 0;
    r.sweep = route[8] != 0;
    static float dummy[2];  // (the planner copies the pointers and reads nothing through them)
    std::vector<th_chan_desc> ch(n_chan);
    for (uint64_t i = 0; i < n_chan; i++) ch[i] = th_chan_desc{dummy, dummy, n_samples[i], stft_n_frames(n_samples[i], win, hop), 0};
    const StftLaunch l = plan_stft_launch(g, r, n_cu, wave_chunk, ch.data(), ch.size());
    EmuBlobs *e = new EmuBlobs;
    e->add(std::vector<uint64_t>{(uint64_t)l.err, l.g.frames_per_tile, l.g.phased, l.sweep, l.tiles, l.edge_tiles, l.mel_tiles, l.amp_rows,
                                 l.all_in_wave, l.ge.frames_per_tile});
    for (const std::vector<ChanJob> *v : {&l.jobs, &l.edge}) {
        std::vector<uint64_t> rows;
        for (const ChanJob &j : *v) rows.insert(rows.end(), {j.n_samples, j.n_frames, j.f_begin, j.f_end, j.mm_index, j.edge});
        e->add(rows);
    }
    e->add(l.tile_start);
    e->add(l.edge_start);
    e->add(l.chunk_tab);
    std::vector<uint64_t> mj, pj;
    for (const MelJob &j : l.mel_jobs) mj.insert(mj.end(), {j.f_begin, j.f_end, j.mm_index});
    for (const WavePostJob &j : l.post) pj.insert(pj.end(), {j.t0, j.t1, j.mm_index});
    e->add(mj);
    e->add(l.mel_start);
    e->add(l.amp_row0);
    e->add(pj);
    return e;
}

// The mel tables th_plan_create builds from calc_mel_fb(sr, n_fft, n_mel) (n_mel = 0: the default count).  Blobs: 0 the dense
// filterbank (f32, [n_freq][n_mel]); 1 {n_mel, kblocks, ntiles, zero_block, n_slices, mel_rows ok, mel_rows groups} (u32);
// 2 lo, 3 hi, 4 band, 5 slice (u32); 6 the operand-order blocks (f32); 7 the mel_rows table (u32)
extern "C" __attribute__((visibility("default"))) void *emu_mel_tables(uint32_t sr, uint32_t n_fft, uint32_t n_mel) {
    if (n_mel == 0) n_mel = (uint32_t)mel_default_n_mel(sr, n_fft);
    const uint32_t n_freq = n_fft / 2 + 1;
    const std::vector<float> fb = calc_mel_fb(sr, n_fft, n_mel, 0.f, -1.f, true);
    const MelRangeHost rg = build_mel_ranges(fb.data(), n_freq, n_mel);
    const MelMfmaHost mt = build_mel_mfma(fb.data(), rg, n_freq, n_mel);
    const MelRowsHost mr = build_mel_rows(fb.data(), rg, n_freq, n_mel);
    EmuBlobs *e = new EmuBlobs;
    e->add(fb);
    e->add(std::vector<uint32_t>{n_mel, mt.kblocks, mt.ntiles, mt.zero_block, mt.n_slices, mr.ok ? 1u : 0u, mr.n_groups});
    e->add(rg.lo);
    e->add(rg.hi);
    e->add(mt.band);
    e->add(mt.slice);
    e->add(mt.bt);
    e->add(mr.words);
    return e;
}

// The wave kernels' window tables from a normalised window.  Blobs (f32): 0 wtab, 1 the phased / dynamic table (empty in mode 0)
extern "C" __attribute__((visibility("default"))) void *emu_wave_window(const float *window, uint32_t win, uint32_t n_fft, int32_t phased_mode) {
    const WaveWindowHost ww = build_wave_window(window, win, n_fft, phased_mode);
    EmuBlobs *e = new EmuBlobs;
    e->add(ww.wtab);
    e->add(ww.phased);
    return e;
}

// ---- the export and loudness-meter readers' plans (reader_plan.h), for tests/test_reader_plan_host.py
#define EMU_API extern "C" __attribute__((visibility("default")))
// rows of 11: {n_ch, n_in, sr_in, sr_out, format, dither, seed, s0, s1, offset, pad}; the resampler's plan and n_out as the check makes them
static bool emu_export_requests(const uint64_t *rows, uint64_t n, std::vector<ExportPlanRequest> *out) {
    out->assign(n, ExportPlanRequest{});
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *r = rows + 11 * i;
        ExportPlanRequest &q = (*out)[i];
        q.n_ch = (uint32_t)r[0];
        q.n_in = r[1];
        q.sr_in = (uint32_t)r[2];
        q.sr_out = (uint32_t)r[3];
        q.format = (uint32_t)r[4];
        q.dither = (uint32_t)r[5];
        q.seed = (uint32_t)r[6];
        q.s0 = r[7];
        q.s1 = r[8];
        q.offset = r[9];
        q.pad = (uint32_t)r[10];
        if (q.sr_out == q.sr_in) continue;
        size_t n_out = 0;
        if (resample_plan(q.sr_in, q.sr_out, &q.plan) != 0 || !resample_n_out(q.n_in, q.plan, &n_out)) return false;
        q.n_out = n_out;
    }
    return true;
}
// Blobs (u64 unless said): 0 {err, n_ptrs, o_rjobs, o_ptrs, tab_bytes, stage_need[0], stage_need[1], scratch_need}; 1 the error text
// (bytes); 2 jobs, rows of {request, f0, f1, n, n_ch, format, dither, seed, first_chunk, pad, stage_at, resampled, hull0, stride,
// scratch_at, ptr_at}; 3 resample jobs, rows of {ja, jb, n_in, ch_stride, n_ch, n_sb, first_block}; 4 pieces, rows of {job0, job1,
// n_chunks, stage_bytes, run0, run1, rjob0, rjob1, n_rblocks, sr_in, sr_out, scratch_floats}; 5 runs, rows of {stage_at, out_at,
// bytes}; 6 ptr0; 7 per request {n_out, S, outputs per tile (G Pt Lp)} of its resampler (zeros: not resampled)
EMU_API void *emu_plan_export(const uint64_t *rows, uint64_t n) {
    std::vector<ExportPlanRequest> reqs;
    if (!emu_export_requests(rows, n, &reqs)) return nullptr;
    const ExportPlan p = plan_export(reqs.data(), reqs.size());
    EmuBlobs *e = new EmuBlobs;
    e->add(std::vector<uint64_t>{(uint64_t)p.err, p.n_ptrs, p.o_rjobs, p.o_ptrs, p.tab_bytes, p.stage_need[0], p.stage_need[1], p.scratch_need});
    e->add(std::vector<char>(p.err_text.begin(), p.err_text.end()));
    std::vector<uint64_t> jobs, rjobs, pieces, runs, per_req;
    for (size_t j = 0; j < p.jobs.size(); j++) {
        const ExportJob &x = p.jobs[j];
        const ExportPlace &pl = p.places[j];
        jobs.insert(jobs.end(), {pl.req, x.f0, x.f1, x.n, x.n_ch, x.format, x.dither, x.seed, x.first_chunk, x.pad, pl.stage_at, pl.resampled,
                                 pl.hull0, pl.stride, pl.scratch_at, pl.ptr_at});
    }
    for (const ResampleJob &x : p.rjobs) rjobs.insert(rjobs.end(), {x.ja, x.jb, x.n_in, x.ch_stride, x.n_ch, x.n_sb, x.first_block});
    for (const ExportPiece &x : p.pieces) {
        const uint64_t run0 = runs.size() / 3;
        for (const ExportRun &r : x.runs) runs.insert(runs.end(), {r.stage_at, r.out_at, r.bytes});
        pieces.insert(pieces.end(), {x.job0, x.job1, x.n_chunks, x.stage_bytes, run0, runs.size() / 3, x.rjob0, x.rjob1, x.n_rblocks, x.sr_in,
                                     x.sr_out, x.scratch_floats});
    }
    for (const ExportPlanRequest &q : reqs) {
        const ResampleTiling t = q.sr_out != q.sr_in ? resample_tiling(q.plan) : ResampleTiling{};
        per_req.insert(per_req.end(), {q.n_out, t.S, (uint64_t)t.G * t.Pt * t.Lp});
    }
    e->add(jobs);
    e->add(rjobs);
    e->add(pieces);
    e->add(runs);
    e->add(std::vector<uint64_t>(p.ptr0.begin(), p.ptr0.end()));
    e->add(per_req);
    return e;
}
// bind_export on the plan of the same rows.  bases: {stage 0, stage 1, scratch, table, counters} as addresses; chan: every
// request's channel addresses in request order.  Blobs (u64): 0 jobs, rows of {chan, dst, cnt}; 1 resample jobs, rows of {chan, dst};
// 2 the table as it would be uploaded (bytes)
EMU_API void *emu_bind_export(const uint64_t *rows, uint64_t n, const uint64_t *bases, const uint64_t *chan, uint64_t n_chan) {
    std::vector<ExportPlanRequest> reqs;
    if (!emu_export_requests(rows, n, &reqs)) return nullptr;
    ExportPlan p = plan_export(reqs.data(), reqs.size());
    if (p.err != TH_OK) return nullptr;
    std::vector<const float *> ch(n_chan);
    for (uint64_t i = 0; i < n_chan; i++) ch[i] = reinterpret_cast<const float *>((uintptr_t)chan[i]);
    const ExportBases b{{reinterpret_cast<uint8_t *>((uintptr_t)bases[0]), reinterpret_cast<uint8_t *>((uintptr_t)bases[1])},
                        reinterpret_cast<float *>((uintptr_t)bases[2]), reinterpret_cast<unsigned char *>((uintptr_t)bases[3]),
                        reinterpret_cast<unsigned long long *>((uintptr_t)bases[4])};
    const std::vector<unsigned char> tab = bind_export(p, b, ch.data());
    EmuBlobs *e = new EmuBlobs;
    std::vector<uint64_t> jobs, rjobs;
    for (const ExportJob &x : p.jobs) jobs.insert(jobs.end(), {(uint64_t)(uintptr_t)x.chan, (uint64_t)(uintptr_t)x.dst, (uint64_t)(uintptr_t)x.cnt});
    for (const ResampleJob &x : p.rjobs) rjobs.insert(rjobs.end(), {(uint64_t)(uintptr_t)x.chan, (uint64_t)(uintptr_t)x.dst});
    e->add(jobs);
    e->add(rjobs);
    e->add(tab);
    return e;
}

// rows of 4: {id, sr, n_ch, n_samples}; the oversampling and the two counts as loudness_meter_info makes them
static std::vector<MeterPlanTrack> emu_meter_tracks(const uint64_t *rows, uint64_t n) {
    std::vector<MeterPlanTrack> out(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *r = rows + 4 * i;
        const uint32_t sr = (uint32_t)r[1];
        const bool ok = loudness_rate_ok(sr);
        out[i] = MeterPlanTrack{(size_t)r[0], sr, (uint32_t)r[2], true_peak_factor(sr), r[3], ok ? loudness_n_blocks(r[3], sr) : 0,
                                ok ? loudness_n_short_term(r[3], sr) : 0};
    }
    return out;
}
// Blobs (u64 unless said): 0 {err, n_ch, n_energies, n_states, max_chunks, max_fchunks, lds_floats, tp_chunks[0], tp_chunks[1], max_m,
// max_s, o_sums, o_pka, o_pkt, res_bytes, o_z, o_q, mem_bytes, t_rates, t_m, t_s, t_tp4, t_tp2, tab_bytes, sizeof LoudJob, LoudnessRate,
// LoudTrackJob, TruePeakJob}; 1 the error text (bytes); 2 rates, rows of {sr, s100, n_sub, cl}; 3 jobs, rows of {n, rate, n_chunks,
// n_fchunks}; 4 momentary and 5 short-term track jobs, rows of {n_blocks, n_ch, n_sub, n_fchunks, L}; 6 the track jobs' weights (f64,
// 8 per track); 7 F = 4 and 8 F = 2 true-peak jobs, rows of {n, n_chunks, channel}; 9 per track {ch0, e0, rate_ok, oversampling,
// n_momentary, n_short_term}
EMU_API void *emu_plan_meters(const uint64_t *rows, uint64_t n) {
    const std::vector<MeterPlanTrack> trs = emu_meter_tracks(rows, n);
    const MeterPlan p = plan_meters(trs.data(), trs.size());
    EmuBlobs *e = new EmuBlobs;
    e->add(std::vector<uint64_t>{(uint64_t)p.err, p.n_ch, p.n_energies, p.n_states, p.max_chunks, p.max_fchunks, p.lds_floats, p.tp_chunks[0],
                                 p.tp_chunks[1], p.max_m, p.max_s, p.o_sums, p.o_pka, p.o_pkt, p.res_bytes, p.o_z, p.o_q, p.mem_bytes, p.t_rates,
                                 p.t_m, p.t_s, p.t_tp4, p.t_tp2, p.tab_bytes, sizeof(LoudJob), sizeof(LoudnessRate), sizeof(LoudTrackJob),
                                 sizeof(TruePeakJob)});
    e->add(std::vector<char>(p.err_text.begin(), p.err_text.end()));
    std::vector<uint64_t> rates, jobs, tj[2], tp[2], per;
    std::vector<double> w;
    for (const LoudnessRate *r : p.rates) rates.insert(rates.end(), {r->sr, r->s100, r->n_sub, r->cl});
    for (const LoudJob &j : p.jobs) jobs.insert(jobs.end(), {j.n, j.rate, j.n_chunks, j.n_fchunks});
    for (int v = 0; v < 2; v++)
        for (const LoudTrackJob &t : v ? p.tj_s : p.tj_m) tj[v].insert(tj[v].end(), {t.n_blocks, t.n_ch, t.n_sub, t.n_fchunks, t.L});
    for (const LoudTrackJob &t : p.tj_m) w.insert(w.end(), t.w, t.w + 8);
    for (int f = 0; f < 2; f++)
        for (size_t k = 0; k < p.tp[f].size(); k++) tp[f].insert(tp[f].end(), {p.tp[f][k].n, p.tp[f][k].n_chunks, p.tp_ch[f][k]});
    for (size_t i = 0; i < p.tracks.size(); i++)
        per.insert(per.end(), {p.ch0[i], p.e0[i], p.rate_ok[i], trs[i].oversampling, trs[i].n_momentary, trs[i].n_short_term});
    e->add(rates);
    e->add(jobs);
    e->add(tj[0]);
    e->add(tj[1]);
    e->add(w);
    e->add(tp[0]);
    e->add(tp[1]);
    e->add(per);
    return e;
}
// bind_meters on the plan of the same rows (mem: the memory's address; wav: every channel's address).  Blobs (u64): 0 jobs, rows of
// {wav, z, q, sumsq, peak, aligned16}; 1 momentary and 2 short-term track jobs, rows of {q, out}; 3 F = 4 and 4 F = 2 true-peak
// jobs, rows of {wav, peak, aligned16}; 5 the table as it would be uploaded (bytes)
EMU_API void *emu_bind_meters(const uint64_t *rows, uint64_t n, uint64_t mem, const uint64_t *wav, uint64_t n_wav) {
    const std::vector<MeterPlanTrack> trs = emu_meter_tracks(rows, n);
    MeterPlan p = plan_meters(trs.data(), trs.size());
    if (p.err != TH_OK || n_wav != p.n_ch) return nullptr;
    std::vector<const float *> w(n_wav);
    for (uint64_t i = 0; i < n_wav; i++) w[i] = reinterpret_cast<const float *>((uintptr_t)wav[i]);
    const std::vector<unsigned char> tab = bind_meters(p, reinterpret_cast<unsigned char *>((uintptr_t)mem), w.data());
    auto a = [](const void *q) { return (uint64_t)(uintptr_t)q; };
    std::vector<uint64_t> jobs, tj[2], tp[2];
    for (const LoudJob &j : p.jobs) jobs.insert(jobs.end(), {a(j.wav), a(j.z), a(j.q), a(j.sumsq), a(j.peak), j.aligned16});
    for (int v = 0; v < 2; v++)
        for (const LoudTrackJob &t : v ? p.tj_s : p.tj_m) tj[v].insert(tj[v].end(), {a(t.q), a(t.out)});
    for (int f = 0; f < 2; f++)
        for (const TruePeakJob &t : p.tp[f]) tp[f].insert(tp[f].end(), {a(t.wav), a(t.peak), t.aligned16});
    EmuBlobs *e = new EmuBlobs;
    e->add(jobs);
    e->add(tj[0]);
    e->add(tj[1]);
    e->add(tp[0]);
    e->add(tp[1]);
    e->add(tab);
    return e;
}
// meter_results from a result area of res_bytes (the series laid out as meters_layout does: track by track, the momentary values,
// then the short-term ones).  Blobs (f64): 0 rows of {max_momentary_lufs, max_short_term_lufs, loudness_range, true_peak,
// true_peak_dB, true_peak_channel}; 1 the series
EMU_API void *emu_meter_results(const uint64_t *rows, uint64_t n, const unsigned char *res, uint64_t res_bytes) {
    const std::vector<MeterPlanTrack> trs = emu_meter_tracks(rows, n);
    const MeterPlan p = plan_meters(trs.data(), trs.size());
    if (p.err != TH_OK || res_bytes != p.res_bytes) return nullptr;
    std::vector<th_loudness_meter> ms(trs.size());
    std::vector<th_loudness_meter *> mp(trs.size());
    for (size_t i = 0; i < trs.size(); i++) {
        ms[i] = th_loudness_meter{};
        ms[i].oversampling = trs[i].oversampling;
        ms[i].n_momentary = trs[i].n_momentary;
        ms[i].n_short_term = trs[i].n_short_term;
        ms[i].momentary_offset = p.e0[i];
        ms[i].short_term_offset = p.e0[i] + trs[i].n_momentary;
        mp[i] = &ms[i];
    }
    std::vector<double> out, series(p.n_energies, -1.0);
    meter_results(res, p, mp.data(), series.data());
    for (const th_loudness_meter &m : ms)
        out.insert(out.end(), {m.max_momentary_lufs, m.max_short_term_lufs, m.loudness_range, (double)m.true_peak, (double)m.true_peak_dB,
                               (double)m.true_peak_channel});
    EmuBlobs *e = new EmuBlobs;
    e->add(out);
    e->add(series);
    return e;
}

// ---- the image, raster and waveform batch entries' plans (batch_plan.h), for tests/test_batch_plan_host.py.  Descriptors come as rows
// of u64 in the order of their struct's fields, pointers as addresses (a planner never reads through them).  Blob 0 of every plan
// starts with the error code, blob 1 is the error text (bytes).
#include "../../thesia_amd/csrc/batch_plan.h"  // (batch_plan.cpp is compiled in)
template <class T>
static T *emu_ptr(uint64_t a) { return reinterpret_cast<T *>((uintptr_t)a); }
static uint64_t emu_addr(const void *p) { return (uint64_t)(uintptr_t)p; }
static EmuBlobs *emu_status(const PlanStatus &p, std::initializer_list<uint64_t> more) {
    EmuBlobs *e = new EmuBlobs;
    std::vector<uint64_t> head{(uint64_t)(int64_t)p.err};
    head.insert(head.end(), more.begin(), more.end());
    e->add(head);
    e->add(std::vector<char>(p.err_text.begin(), p.err_text.end()));
    return e;
}
static th_img_desc emu_img_desc(const uint64_t *r) {
    return th_img_desc{emu_ptr<const float>(r[0]), emu_ptr<uint16_t>(r[1]), r[2], r[3], r[4], r[5], r[6], r[7]};
}
static float emu_f32(uint32_t bits) {
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
// check_img.  rows of 8: th_img_desc; the range as float bits.  Blobs: 0 {err, all_neg_inf}
EMU_API void *emu_check_img(const uint64_t *rows, uint64_t n, uint32_t min_bits, uint32_t max_bits, uint64_t d_range) {
    std::vector<th_img_desc> d(n);
    for (uint64_t i = 0; i < n; i++) d[i] = emu_img_desc(rows + 8 * i);
    const float lo = emu_f32(min_bits), hi = emu_f32(max_bits);
    return emu_status(check_img(d.data(), n, lo, hi, emu_ptr<const float>(d_range)), {db_range_all_neg_inf(lo, hi, emu_ptr<const float>(d_range))});
}
// plan_img.  Blobs: 0 {err, n_blocks}; 2 jobs, rows of {spec, img, n_frames, height, i_start, i_end, spec_pitch, img_pitch, first_tile,
// n_tiles}; 3 the block -> job table (u32)
EMU_API void *emu_plan_img(const uint64_t *rows, uint64_t n) {
    std::vector<th_img_desc> d(n);
    for (uint64_t i = 0; i < n; i++) d[i] = emu_img_desc(rows + 8 * i);
    const ImgPlan p = plan_img(d.data(), n);
    EmuBlobs *e = emu_status(p, {p.n_blocks});
    std::vector<uint64_t> jobs;
    for (const ImgJob &j : p.jobs)
        jobs.insert(jobs.end(), {emu_addr(j.spec), emu_addr(j.img), j.n_frames, j.height, j.i_start, j.i_end, j.spec_pitch, j.img_pitch, j.first_tile, j.n_tiles});
    e->add(jobs);
    e->add(p.block_job);
    return e;
}
// check_fused, then plan_fused.  rows of 11: th_img_desc, then {index of the image's first tile pointer in `tiles` (~0: tiles is NULL),
// n_tiles_x, n_tiles_y}.  Blobs: 0 {err of the first of the two that failed, n_blocks, sizeof(th_img_tiles_desc)}; 2 the key
// (bytes); 3 jobs, rows of {spec, img, n_frames, height, i_start, i_end, spec_pitch, img_pitch, first_block, n_bands, n_tx, n_ty,
// tile0}; 4 the block -> job table (u32); 5 the pointer table
EMU_API void *emu_plan_fused(const uint64_t *rows, uint64_t n, const uint64_t *tiles, uint32_t min_bits, uint32_t max_bits, uint64_t d_range) {
    std::vector<th_img_tiles_desc> d(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *r = rows + 11 * i;
        d[i] = th_img_tiles_desc{emu_img_desc(r), r[8] == ~0ull ? nullptr : reinterpret_cast<uint8_t *const *>(tiles + r[8]), (uint32_t)r[9], (uint32_t)r[10]};
    }
    std::vector<unsigned char> key;
    const PlanStatus ok = check_fused(d.data(), n, emu_f32(min_bits), emu_f32(max_bits), emu_ptr<const float>(d_range), &key);
    const FusedPlan p = ok.err == TH_OK ? plan_fused(d.data(), n) : FusedPlan{};
    EmuBlobs *e = emu_status(ok.err != TH_OK ? ok : p, {p.n_blocks, sizeof(th_img_tiles_desc)});
    e->add(key);
    std::vector<uint64_t> jobs, ptrs;
    for (const FusedJob &j : p.jobs)
        jobs.insert(jobs.end(), {emu_addr(j.spec), emu_addr(j.img), j.n_frames, j.height, j.i_start, j.i_end, j.spec_pitch, j.img_pitch, j.first_block,
                                 j.n_bands, j.n_tx, j.n_ty, j.tile0});
    for (const uint8_t *t : p.ptrs) ptrs.push_back(emu_addr(t));
    e->add(jobs);
    e->add(p.block_job);
    e->add(ptrs);
    return e;
}
// plan_raster.  rows of 10: th_raster_desc.  Blobs: 0 {err, n_blocks}; 2 jobs, rows of {img, rgba, img_width, img_height, origin_x,
// origin_y, width, height, img_pitch, quads_per_row, inv_qpr, inv_width, first_block}; 3 the block -> job table (u32)
EMU_API void *emu_plan_raster(const uint64_t *rows, uint64_t n) {
    std::vector<th_raster_desc> d(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *r = rows + 10 * i;
        d[i] = th_raster_desc{emu_ptr<const uint16_t>(r[0]), emu_ptr<uint8_t>(r[1]), (uint32_t)r[2], (uint32_t)r[3], (uint32_t)r[4], (uint32_t)r[5],
                              (uint32_t)r[6], (uint32_t)r[7], (uint32_t)r[8], (uint32_t)r[9]};
    }
    const RasterPlan p = plan_raster(d.data(), n);
    EmuBlobs *e = emu_status(p, {p.n_blocks});
    std::vector<uint64_t> jobs;
    for (const RasterJob &j : p.jobs)
        jobs.insert(jobs.end(), {emu_addr(j.img), emu_addr(j.rgba), j.img_width, j.img_height, j.origin_x, j.origin_y, j.width, j.height, j.img_pitch,
                                 j.quads_per_row, j.inv_qpr, j.inv_width, j.first_block});
    e->add(jobs);
    e->add(p.block_job);
    return e;
}
// plan_wave_tiles.  rows of 6: th_wave_desc.  Blobs: 0 {err, n_blocks}; 2 jobs, rows of 6 as the descriptor; 3 the n + 1 starts (u32)
EMU_API void *emu_plan_wave_tiles(const uint64_t *rows, uint64_t n) {
    std::vector<th_wave_desc> d(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *r = rows + 6 * i;
        d[i] = th_wave_desc{emu_ptr<const float>(r[0]), emu_ptr<float>(r[1]), r[2], r[3], (uint32_t)r[4], (uint32_t)r[5]};
    }
    const WavePlan p = plan_wave_tiles(d.data(), n);
    EmuBlobs *e = emu_status(p, {p.n_blocks});
    std::vector<uint64_t> jobs;
    for (const WaveJob &j : p.jobs) jobs.insert(jobs.end(), {emu_addr(j.wav), emu_addr(j.bins), j.n_samples, j.start, j.level, j.bin_count});
    e->add(jobs);
    e->add(p.start);
    return e;
}
// plan_stats.  rows of 2: th_stats_desc.  Blobs: 0 {err, max_samples}; 2 jobs, rows of {wav, n_samples, aligned16}
EMU_API void *emu_plan_stats(const uint64_t *rows, uint64_t n) {
    std::vector<th_stats_desc> d(n);
    for (uint64_t i = 0; i < n; i++) d[i] = th_stats_desc{emu_ptr<const float>(rows[2 * i]), rows[2 * i + 1]};
    const StatsPlan p = plan_stats(d.data(), n);
    EmuBlobs *e = emu_status(p, {p.max_samples});
    std::vector<uint64_t> jobs;
    for (const StatsJob &j : p.jobs) jobs.insert(jobs.end(), {emu_addr(j.wav), j.n_samples, j.aligned16});
    e->add(jobs);
    return e;
}
// plan_pyramid, then bind_pyramid(sums).  rows of 5: th_pyramid_desc.  Blobs: 0 {err, sums_floats, max_samples, max_levels, launch};
// 2 jobs, rows of 47: {wav, out, sums, n_samples, sums_half, n_levels, aligned16, level_off[40]}; 3 sums_at
EMU_API void *emu_plan_pyramid(const uint64_t *rows, uint64_t n, uint64_t sums) {
    std::vector<th_pyramid_desc> d(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *r = rows + 5 * i;
        d[i] = th_pyramid_desc{emu_ptr<const float>(r[0]), emu_ptr<float>(r[1]), r[2], (uint32_t)r[3], (uint32_t)r[4]};
    }
    PyrPlan p = plan_pyramid(d.data(), n);
    if (p.err == TH_OK) bind_pyramid(p, emu_ptr<float>(sums));
    EmuBlobs *e = emu_status(p, {p.sums_floats, p.max_samples, p.max_levels, p.launch});
    std::vector<uint64_t> jobs;
    for (const PyrJob &j : p.jobs) {
        jobs.insert(jobs.end(), {emu_addr(j.wav), emu_addr(j.out), emu_addr(j.sums), j.n_samples, j.sums_half, j.n_levels, j.aligned16});
        jobs.insert(jobs.end(), j.level_off, j.level_off + PYR_MAX_LEVELS);
    }
    e->add(jobs);
    e->add(p.sums_at);
    return e;
}
// plan_lod_tile of tile (tx, ty) of level (lx, ly) of a W x H image (NULL: the tile is empty).  Blobs: 0 {err, y_lo, y_hi, n_rows, dw,
// dh, y_at, taps_x, taps_y, lod_at, scratch_bytes, origin_x, origin_y, lod_w, lod_h}; 2 {left, top, crop_w, crop_h} (f64); 3 the tap blob
EMU_API void *emu_plan_lod_tile(uint64_t W, uint64_t H, uint32_t lx, uint32_t ly, uint32_t tx, uint32_t ty) {
    const TileGeom g = spectrogram_tile_geometry(W, H, lx, ly, tx, ty);
    if (!g.width || !g.height) return nullptr;
    const LodTilePlan p = plan_lod_tile(W, H, g, lx, ly);
    EmuBlobs *e = emu_status(p, {(uint64_t)p.y_lo, (uint64_t)p.y_hi, p.n_rows, p.dw, p.dh, p.y_at, p.taps_x, p.taps_y, p.lod_at, p.scratch_bytes,
                                 g.origin_x, g.origin_y, g.lod_w, g.lod_h});
    e->add(std::vector<double>{p.left, p.top, p.crop_w, p.crop_h});
    e->add(p.blob);
    return e;
}
// the tile headers (host_math.h): 40 and 24 bytes into out; return the pixels / the bins of the tile
EMU_API uint64_t emu_spectrogram_tile_header(uint8_t *out, uint64_t revision, uint64_t W, uint64_t H, uint32_t lx, uint32_t ly, uint32_t tx, uint32_t ty) {
    const TileGeom g = spectrogram_tile_geometry(W, H, lx, ly, tx, ty);
    put_spectrogram_tile_header(out, revision, g, lx, ly, tx, ty);
    return g.width * g.height;
}
EMU_API uint64_t emu_waveform_tile_header(uint8_t *out, uint64_t revision, uint64_t n_samples, uint32_t level, uint32_t tile) {
    size_t start, bins, spb;
    waveform_tile_geometry(n_samples, level, tile, &start, &bins, &spb);
    put_waveform_tile_header(out, revision, bins, spb, tile);
    return bins;
}
