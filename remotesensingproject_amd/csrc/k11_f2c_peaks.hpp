// K11: the peak planes of a fine-to-coarse pyramid (include/rslf_hip.h, "peaks per level and validity by uniqueness") -- the
// uniqueness predicate on a level's validity plane, and the fused peaks: for every pixel of the fused map the level that
// decided it and that level's peaks.  The rules are k11_f2c_peak_rule.hpp's, which g++ compiles too.
#pragma once

#include <hip/hip_runtime.h>

#include "k11_f2c_peak_rule.hpp"

namespace rslf {

// In place on a level's validity plane, lanes along u: a valid pixel whose runner-up is within `ratio` of its winner becomes
// invalid; every other byte is left as the validity rule wrote it.  The peaks are read where the byte is non-zero only.
__global__ __launch_bounds__(256) void k11_unique_mask(uint8_t* __restrict__ valid, const int32_t* __restrict__ idx,
                                                      const float* __restrict__ score, const int32_t* __restrict__ runner_idx,
                                                      const float* __restrict__ runner_score, float ratio, long long n)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (valid[i] == 0)
            continue;
        if (f2c_peak_ambiguous(idx[i], runner_idx[i], score[i], runner_score[i], ratio))
            valid[i] = 0;
    }
}

// The whole pyramid as one by-value argument: wave-uniform, so every member is read with scalar loads.  Finest level first.
constexpr int kF2cPeakLevels = 32;   // RSLF_F2C_MAX_LEVELS
struct FusePeaksArgs {
    const uint8_t* valid[kF2cPeakLevels];          // [S][V_p][U_p] each
    const int32_t* idx[kF2cPeakLevels];
    const float* score[kF2cPeakLevels];
    const int32_t* runner_idx[kF2cPeakLevels];
    const float* runner_score[kF2cPeakLevels];
    double scale_v[kF2cPeakLevels];                // f2c_walk_scale(V_p, V_{p+1}), f2c_walk_scale(U_p, U_{p+1}); unused at P - 1
    double scale_u[kF2cPeakLevels];
    int V[kF2cPeakLevels], U[kF2cPeakLevels];
    int P, S;
    int32_t* out_idx;                              // [S][V_0][U_0], each nullable
    float* out_score;
    int32_t* out_runner_idx;
    float* out_runner_score;
    uint8_t* out_level;
};

// One launch for the pyramid, lane = pixel of the finest plane (x along u; blockIdx.y the scanline, blockIdx.z the view).
// The lane walks down the fusion's mask chain (k5_fuse_step's INTER_NEAREST): at level p and pixel (y, x), a non-zero validity
// byte makes this pixel the origin; else the walk goes on at level p + 1, pixel (f2c_walk_index(y), f2c_walk_index(x)).  One
// validity byte is read per level walked, then the origin's four values; no origin: level 255, idx = runner_idx = -1, scores 0.
// The level counter is uniform inside the loop (lanes leave it, none runs ahead), so the level's pointers and sizes stay
// scalar; the gather sits inside the loop for that reason.  Every index is inside its plane: 0 <= f2c_walk_index < coarse.
__global__ __launch_bounds__(256) void k11_fuse_peaks(const FusePeaksArgs a)
{
    const int x0 = blockIdx.x * blockDim.x + threadIdx.x;
    const int y0 = blockIdx.y, s = blockIdx.z;
    if (x0 >= a.U[0])
        return;
    int x = x0, y = y0;
    int level = 255;
    int32_t i1 = -1, i2 = -1;
    float s1 = 0.0f, s2 = 0.0f;
    for (int p = 0; p < a.P; p++) {
        const long long o = ((long long)s * a.V[p] + y) * a.U[p] + x;
        if (a.valid[p][o] != 0) {
            level = p;
            i1 = a.idx[p][o];
            s1 = a.score[p][o];
            i2 = a.runner_idx[p][o];
            s2 = a.runner_score[p][o];
            break;
        }
        if (p + 1 < a.P) {
            y = f2c_walk_index(y, a.scale_v[p], a.V[p + 1]);
            x = f2c_walk_index(x, a.scale_u[p], a.U[p + 1]);
        }
    }
    const long long o0 = ((long long)s * a.V[0] + y0) * a.U[0] + x0;
    if (a.out_idx)
        a.out_idx[o0] = i1;
    if (a.out_score)
        a.out_score[o0] = s1;
    if (a.out_runner_idx)
        a.out_runner_idx[o0] = i2;
    if (a.out_runner_score)
        a.out_runner_score[o0] = s2;
    if (a.out_level)
        a.out_level[o0] = (uint8_t)level;
}

}  // namespace rslf
