// K8, score-row peaks (k8_score_peaks): winner, sub-grid disparity and runner-up of every pixel's score row.
//
// The reader of what the score rows write (k2_scores.hpp): rows [pixel][dim_d], d fastest, pixels of a window of scanlines
// in order, so the rows of 64 consecutive pixels are ONE contiguous piece of memory.  The rule per row is k8_peak_rule.hpp
// (one pass in ascending d, a window of three values); the work here is getting the rows to the lanes.  Lane = pixel
// reading its own row would put every lane on a cache line of its own (rows are dim_d floats apart) -- what ScoreRows
// transposes on the way out.  This is ScoreRows in reverse: a wave brings a block of at most kPeakBlock hypotheses x its
// 64 pixels into LDS with loads whose lanes walk the block's floats in memory order (runs of a whole block row, at least
// 64 B, a whole tile when dim_d fits one block), at an odd pitch; then lane = pixel walks its row of the block in
// ascending d through PeakScan, whose state stays in registers across blocks.  One pass over the row, no cross-lane
// reduction, no atomics, nothing that depends on the launch shape; the waves of a workgroup share nothing.
//
// A pixel whose mask byte is 0, or past the window's end, is neither read nor written: the loads of its share of a block
// go to the tile's first live pixel instead (a line the wave reads anyway), which keeps the load loop free of branches.
#pragma once

#include <hip/hip_runtime.h>

#include "k8_peak_rule.hpp"
#include "rslf_plan_peaks.hpp"

namespace rslf {

struct PeakArgs {
    const float* scores;      // [n_pixels][dim_d]
    const uint8_t* mask;      // nullable; [first + pixel]
    const float* dmin_vu;     // both or neither; [first + pixel]
    const float* dmax_vu;
    float dmin, dmax;
    long long first;          // v_first * U: the window's first pixel within the [V][U] planes
    long long n_pixels;       // n_rows * U
    int dim_d, n_blocks;      // plan::peak_blocks(dim_d)
    int32_t* idx;             // the five planes [n_pixels], each nullable
    float* score;
    float* disp;
    int32_t* runner_idx;
    float* runner_score;
};

__global__ __launch_bounds__(64 * plan::kPeakWaves) void k8_score_peaks(PeakArgs a)
{
    constexpr int kPitch = plan::kPeakPitch;
    __shared__ float s_park[plan::kPeakWaves][plan::kPeakTile * kPitch];
    static_assert(sizeof(s_park) == plan::peaks_lds_bytes() && plan::peaks_lds_bytes() <= plan::kPeakLdsLimit,
                  "rslf_plan_peaks.hpp states this kernel's LDS");
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long long p0 = ((long long)blockIdx.x * plan::kPeakWaves + wave) * plan::kPeakTile;
    if (p0 >= a.n_pixels)
        return;   // (wave-uniform; no workgroup barrier below)
    const long long p = p0 + lane;
    const bool alive = p < a.n_pixels && (!a.mask || a.mask[a.first + p] != 0);
    const unsigned long long live = __ballot(alive);
    if (live == 0)
        return;
    const unsigned first_live = (unsigned)(__ffsll((long long)live) - 1);
    float* park = s_park[wave];
    const float* tile = a.scores + (size_t)p0 * (size_t)a.dim_d;
    const unsigned D = (unsigned)a.dim_d;

    PeakScan scan;
    scan.init();
    const int width = a.dim_d / a.n_blocks, wider = a.dim_d % a.n_blocks;
    for (int k = 0; k < a.n_blocks; k++) {
        const unsigned d0 = (unsigned)plan::peak_block_at(k, width, wider);
        const unsigned W = (unsigned)plan::peak_block_at(k + 1, width, wider) - d0;   // 1 .. kPeakBlock
        // the block's 64 * W floats in memory order, 64 per step: float g = i * 64 + lane is (pixel g / W, hypothesis g % W)
        const unsigned q_step = 64u / W, r_step = 64u % W;
        unsigned px = (unsigned)lane / W, j = (unsigned)lane % W;
#pragma unroll 16
        for (unsigned i = 0; i < W; i++) {   // (16 loads in flight per lane before the first parking store waits)
            const unsigned from = ((live >> px) & 1ull) ? px : first_live;
            park[px * kPitch + j] = tile[from * D + d0 + j];   // (64 * dim_d < 2^32: plan::kPeakMaxDimD)
            j += r_step;
            px += q_step;
            if (j >= W)
                j -= W, px++;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (alive) {
            // eight LDS reads ahead of their use (past the block's end the last value again, not offered)
            for (unsigned j0 = 0; j0 < W; j0 += 8) {
                float s[8];
#pragma unroll
                for (unsigned e = 0; e < 8; e++)
                    s[e] = park[lane * kPitch + min(j0 + e, W - 1)];
#pragma unroll
                for (unsigned e = 0; e < 8; e++)
                    if (j0 + e < W)   // (wave-uniform)
                        scan.offer(s[e], (int)(d0 + j0 + e));
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (!alive)
        return;
    const float lo = a.dmin_vu ? a.dmin_vu[a.first + p] : a.dmin;
    const float hi = a.dmax_vu ? a.dmax_vu[a.first + p] : a.dmax;
    const PeakResult r = scan.finish(a.dim_d, lo, hi);
    if (a.idx)
        a.idx[p] = r.idx;
    if (a.score)
        a.score[p] = r.score;
    if (a.disp)
        a.disp[p] = r.disp;
    if (a.runner_idx)
        a.runner_idx[p] = r.runner_idx;
    if (a.runner_score)
        a.runner_score[p] = r.runner_score;
}

}  // namespace rslf
