// stft_plan.h — the host side of an STFT plan as plain data: which kernels it runs (StftRoute), the tables it holds
// (build_wave_window .. build_mel_rows) and what one launch is made of (plan_stft_launch).  No HIP header: api.hip uploads
// and launches what these functions return, tests/emu/ compiles the same functions with g++ (implementations: host_math.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/thesia_amd.h"
#include "stft_core.h"

// ---- build-time constants (TH_MEL_SLICES, TH_CHUNKS_PER_WAVE: read by host_math.cpp — scripts/build_variant.sh with VARIANT_SOURCES=host_math.cpp)
#if !defined(TH_MEL_MT)
#define TH_MEL_MT 2
#endif
#if !defined(TH_MEL_SLICES)
#define TH_MEL_SLICES 6  // slices of mel_mfma_kernel's tile range (grid y)
#endif
// about TH_CHUNKS_PER_WAVE chunks per wave (at most 32 frames each): the launch ends when the last chunk does,
// so a chunk is the granularity of the load balance, while every chunk costs one full fetch and one atomic on the
// queue head (served at ~8 ns each device-wide).  Measured inside bench.py's step: 4 per wave (29 frames)
// 0.50-0.515 ms, 6 (19) 0.52, 8 (14) 0.54, 12 (9) 0.69; 32-frame chunks 0.53.
#if !defined(TH_CHUNKS_PER_WAVE)
#define TH_CHUNKS_PER_WAVE 4
#endif

namespace th {

// th_plan_set_kernel's selectors (bits 0-7), described in include/thesia_amd_testing.h.  Product builds refuse the A/B-only
// ones there (9, 11, 14 at n_fft 32768 / 65536, 15 at n_fft 8192, and wave counts other than a size's own).
enum StftSelector : int {
    SEL_AUTO = 0,
    SEL_GENERIC = 1,
    SEL_WAVE = 2,              // every selector from here on asks for a wave kernel
    SEL_MEL_AMP = 3,           // amplitude rows + a second mel kernel
    SEL_NO_PHASE = 4,
    SEL_PHASE_FUSED = 5,
    SEL_MULTI_1024 = 6,
    SEL_MEL_MFMA = 7,          // as 3, the matrix-core kernel also where 3 runs mel_rows / mel_band_rows
    SEL_MEL_PIECES = 8,
    SEL_PACKED = 9,
    SEL_RESERVED = 10,         // as 2
    SEL_SWEEP = 11,
    SEL_MEL_TWO_KERNELS = 12,
    SEL_MEL_ONE_FRAME = 13,
    SEL_BLOCK = 14,
    SEL_SUBWAVE = 15,
};

// Which kernels a plan launches, and how: everything about a th_calc_spec_batch_dev launch that the batch does not change.
// resolve_route (api.hip) fills it from the plan's geometry, its tables and its kernel selector — at th_plan_create and at every
// th_plan_set_kernel — and nothing else reads the selector.
struct StftRoute {
    enum class Main : uint8_t { Generic, Bluestein, Wave, WaveMulti, Block, Subwave };
    // the mel filterbank in the main kernel's epilogue (mel_fuse.h): moment form with its table in global memory, the same as
    // per-lane constants of the block kernel, mel_rows_kernel's table (n_fft 512), banded sums one frame or two at a time, pieces / gather
    enum class MelFused : uint8_t { None, Moment, MomentLanes, Rows, Banded, BandedPairs, Pieces };
    enum class MelSecond : uint8_t { None, Rows, BandRows, Mfma };  // the mel kernel behind amplitude rows
    Main main = Main::Generic;
    MelFused mel_fused = MelFused::None;
    MelSecond mel_second = MelSecond::None;
    bool no_wave_kernel = false;   // a selector >= 2 asked for a wave kernel this plan has none of: th_calc_spec_batch_dev fails
    int phase_mode = 0;            // StftGeom::phased of the launch (grid-aligned frame loop; window table d_wtab_phased when != 0)
    int waves = 0;                 // waves per workgroup of the wave kernels
    uint32_t tail_guard = 0;       // stft_wave_multi_tail_guard, or 0
    bool edges_in_wave = false;    // boundary frames of channels of at least n_fft samples run inside the wave launch
    bool block_plan = false;       // stft_is_block_plan: launch_stft_wave runs a workgroup-per-frame kernel (n_fft 8192 and above)
    int long_plan = 1;             // WaveOut::long_plan: 1 stft_block_kernel, 2 stft_subwave_kernel (read at n_fft 8192 and above)
    bool sweep = false;            // selector 11's sweep schedule exists for this plan (the launch adds: the batch is large enough)
    bool packed = false;           // selector 9: WaveOut::packed
    char name[48] = "";            // th_plan_kernel_name
    bool wave() const { return main != Main::Generic && main != Main::Bluestein; }
    int out_mode() const { return mel_second != MelSecond::None ? 1 : mel_fused != MelFused::None ? 2 : 0; }  // WaveOut::mode
};

// per-channel tile range [t0, t1) of a wave launch for wave_post_kernel (kernels.h: launch_wave_post)
struct WavePostJob {
    uint32_t t0, t1, mm_index, reserved;
};

// ---- kernels_mel.hip: mel filterbank contraction on the matrix cores (spectrogram.rs:207)
struct MelJob {
    const float *amp;  // n_frames x amp_pitch linear amplitudes |X| (columns >= n_freq are zero)
    float *spec;       // n_frames x spec_pitch dB mel spectrogram
    uint32_t f_begin, f_end, spec_pitch, mm_index;
};
constexpr int MEL_MT = TH_MEL_MT;                         // 16-frame row tiles per wave
constexpr uint32_t MEL_TILE_FRAMES = 64 * MEL_MT;         // 4 waves x MEL_MT x 16 frames per workgroup
// short rows (at most MEL_ROWS_NKB * 16 bins: n_fft 512) under narrow filters (at most MEL_ROWS_W bins each, at most
// 64 * MEL_ROWS_MAX_GROUPS mels): banded sums, lane = mel.  d_tab: [n_groups][1 + MEL_ROWS_W][64] words — the first bin of
// mel 64 g + lane, then its weights (float bits, zero past the filter's end and for mels >= n_mel)
constexpr int MEL_ROWS_NKB = 17, MEL_ROWS_W = 8, MEL_ROWS_MAX_GROUPS = 8;

// The geometry of a plan (n_fft even; linear height, the generic kernel's tile: th_plan_create adds the mel count, a launch its own tile)
StftGeom stft_geom(size_t win, size_t hop, size_t n_fft);

// ---- plan tables (th_plan_create uploads them as they are)
std::vector<cf32> build_twiddles(size_t n_fft);  // W_{n_fft}^i, i < n_fft (double -> f32)
// Wave-kernel window tables from the normalised window w[win] (normalized_hann).  wtab[n] = 0.5 * 2^32 * (wpad[2n], wpad[2n+1]),
// wpad = the window zero-padded to n_fft (pad_left = (n_fft - win) / 2 zeros in front): the 1/2 of the real-FFT split pass and
// the kernel's 2^32 pre-scale (WAVE_PRESCALE, undone in the dB conversion) are folded in; exact, powers of two.
// phased: the grid-aligned modes of the wave kernel (kernels_stft.hip) read the window at offset 0 instead of pad_left —
//   phased_mode 1 (hop 480): behind 48 zero pairs (read 0, 96, 64 or 32 samples lower): 96 + n_fft floats;
//   2 / 3 (dynamic, e.g. hop 441): behind 64 zero pairs, followed by the same with every pair shifted by one sample (odd
//   offsets): 2 (128 + n_fft) floats (3 reads the even table only: the same buffer);  0: empty.
struct WaveWindowHost {
    std::vector<cf32> wtab, phased;
};
WaveWindowHost build_wave_window(const float *w, size_t win, size_t n_fft, int phased_mode);
// the non-zero bin range [lo, hi) of every mel of fb[n_freq][n_mel] (calc_mel_fb's layout); lo = hi = 0 for an empty filter
struct MelRangeHost {
    std::vector<uint32_t> lo, hi;
};
MelRangeHost build_mel_ranges(const float *fb, uint32_t n_freq, uint32_t n_mel);
// MFMA mel path tables (kernels_mel.hip): for every N tile j of 16 mels the band of K blocks (16 bins each) that hold
// non-zeros — band[3 j ..] = {klo, khi, first block} — and the filterbank of those blocks in operand order (256 floats per
// block): lane (kq = lane / 16, li = lane % 16), step s -> fb[16 kb + 4 kq + s][16 j + li]; one all-zero block behind them
// (zero_block); slices of the tile range (grid y): contiguous, about equal numbers of 4-K-block groups, slice[n_slices + 1]
struct MelMfmaHost {
    std::vector<float> bt;
    std::vector<uint32_t> band, slice;
    uint32_t kblocks = 0, ntiles = 0, zero_block = 0, n_slices = 0;
};
MelMfmaHost build_mel_mfma(const float *fb, const MelRangeHost &rg, uint32_t n_freq, uint32_t n_mel);
// mel_rows_kernel's per-mel table (layout: MEL_ROWS_* above).  ok: the bank has the shape the kernel takes — rows of at most
// MEL_ROWS_NKB K blocks whose reads stay in the LDS row, filters of at most MEL_ROWS_W bins, at most MEL_ROWS_MAX_GROUPS groups
struct MelRowsHost {
    std::vector<uint32_t> words;
    uint32_t n_groups = 0;
    bool ok = false;
};
MelRowsHost build_mel_rows(const float *fb, const MelRangeHost &rg, uint32_t n_freq, uint32_t n_mel);

// ---- one launch of th_calc_spec_batch_dev: everything that is decided before the context is locked
struct StftLaunch {
    int err = TH_OK;       // a per-channel argument error found while walking the channels (nothing else below is valid then)
    std::string err_text;
    StftGeom g{}, ge{};    // main launch (phased and frames_per_tile set) and edge launch (generic kernel, one frame per tile)
    bool sweep = false;    // the sweep chunk schedule runs (StftRoute::sweep and the batch is large enough)
    // main jobs: the wave kernel takes the interior frames [fa, fb) of every channel (all windowed samples inside the signal)
    // and, with StftRoute::edges_in_wave, the boundary frames as one-frame chunks; the generic kernel takes the boundary
    // frames (reflect padding, stft.rs:50-95) — or every frame when the wave kernel does not cover this plan.
    std::vector<ChanJob> jobs, edge;
    std::vector<uint32_t> tile_start, edge_start;  // first tile of every job, then the tile count
    std::vector<uint32_t> chunk_tab;               // wave kernels: (job, first frame) per chunk (cursor_at, kernels_stft.hip)
    uint64_t tiles = 0, edge_tiles = 0;
    // a second mel kernel: one job per channel with interior frames; the channel's amplitude rows start at row amp_row0[channel]
    std::vector<MelJob> mel_jobs;  // (amp: filled in by the caller, who owns the amplitude buffer)
    std::vector<uint32_t> mel_start;
    std::vector<uint64_t> amp_row0;
    uint64_t mel_tiles = 0, amp_rows = 0;
    std::vector<WavePostJob> post;  // wave kernels: a channel's jobs (interior, head, tail) are consecutive
    bool all_in_wave = false;       // every frame of every channel is in the wave launch: its follow-up stores the (min, max) slots
};
// g: the plan's geometry (StftGeom::phased and frames_per_tile are the launch's to set); wave_chunk: th_plan_set_kernel's
// frames-per-chunk tuning (0 = choose)
StftLaunch plan_stft_launch(const StftGeom &g, const StftRoute &r, uint32_t n_cu, int wave_chunk, const th_chan_desc *chans, size_t n_chan);

}  // namespace th
