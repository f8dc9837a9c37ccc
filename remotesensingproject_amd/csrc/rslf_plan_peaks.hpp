// The host-side decisions of the score-row peaks (rslf_score_peaks, rslf_depth_epi_peaks; rslf_peaks.hip, k8_peaks.hpp):
// how a row is cut into LDS blocks, the kernel's LDS and grid, the scanlines per pass of the composed entries.  Host-only
// like rslf_plan.hpp, which it continues (that header is at the length limit of a library source); pure functions, tested
// by tests/cpp/test_plan_peaks.cpp.  The per-row rule itself is k8_peak_rule.hpp, shared with the kernel.
#pragma once

#include "rslf_plan.hpp"

namespace rslf {
namespace plan {

// k8_score_peaks: a wave owns a tile of 64 consecutive pixels (rows are [pixel][dim_d], so a tile's rows are one contiguous
// piece of memory) and brings it into LDS block by block: at most kPeakBlock hypotheses of all 64 pixels, at a pitch of
// kPeakBlock + 1 floats -- odd, so that lane = pixel reads its own row without bank conflicts.  32: 8.25 KiB per wave, so
// a CU's 160 KiB hold four workgroups of four waves; a block row of 32 floats is one 128-byte line.
constexpr int kPeakBlock = 32;
constexpr int kPeakPitch = kPeakBlock + 1;
constexpr int kPeakWaves = 4;                       // waves (tiles) per workgroup; they share nothing
constexpr int kPeakTile = 64;                       // pixels per wave
constexpr int kPeakMinRunBytes = 64;                // every load covers contiguous runs at least this long ...
constexpr int kPeakMaxDimD = 1 << 24;               // ... and a tile's 64 * dim_d floats are indexed in 32 bits
constexpr size_t kPeakLdsLimit = (size_t)64 << 10;  // static LDS of one workgroup
constexpr size_t peaks_lds_bytes() { return (size_t)kPeakWaves * kPeakTile * kPeakPitch * sizeof(float); }

// Blocks of a row of dim_d hypotheses: as few as hold kPeakBlock each, of equal width within one.  Block k is
// [peak_block_begin(k), peak_block_begin(k + 1)).  A row that fits one block is loaded whole (the tile is contiguous);
// otherwise every block is at least kPeakBlock / 2 = 16 floats = 64 B wide, whatever dim_d: no sliver at the end.
inline int peak_blocks(int dim_d) { return (std::max(1, dim_d) + kPeakBlock - 1) / kPeakBlock; }
// The first dim_d % n_blocks blocks are one wider than the rest.  (`width`, `wider`: dim_d / n_blocks and dim_d % n_blocks,
// which the kernel takes once per wave.)
constexpr int peak_block_at(int k, int width, int wider) { return k * width + (k < wider ? k : wider); }
constexpr int peak_block_begin(int k, int dim_d, int n_blocks) { return peak_block_at(k, dim_d / n_blocks, dim_d % n_blocks); }

// One wave per tile of the n_pixels = n_rows * U pixels; 0: more workgroups than a grid holds
inline long long peaks_tiles(long long n_pixels) { return (n_pixels + kPeakTile - 1) / kPeakTile; }
inline unsigned peaks_grid(long long n_pixels)
{
    const long long groups = (peaks_tiles(n_pixels) + kPeakWaves - 1) / kPeakWaves;
    return groups >= 1 && groups <= (long long)INT32_MAX ? (unsigned)groups : 0u;
}

// rslf_depth_epi_peaks: the rows of a pass go through the staging buffer, as the host form of the score rows sends them
// (score_window_rows); the five result planes of a pass of the host form follow them in the same buffer.
inline int peaks_window_rows(int U, int dim_d, size_t budget_bytes) { return score_window_rows(U, dim_d, budget_bytes); }
constexpr size_t kPeakPlaneBytes = 5 * sizeof(float);   // per pixel: idx, score, disp, runner_idx, runner_score
inline size_t peaks_staging_bytes(int pass_rows, int U, int dim_d, bool host_planes)
{
    const size_t px = (size_t)pass_rows * (size_t)U;
    return px * (size_t)dim_d * sizeof(float) + (host_planes ? px * kPeakPlaneBytes : 0);
}

}  // namespace plan
}  // namespace rslf
