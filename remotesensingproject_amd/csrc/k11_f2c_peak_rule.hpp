// The two rules of the pyramid's peak planes, stated once for the device (k11_f2c_peaks.hpp) and for the host
// (tests/cpp/test_plan_f2c_peaks.cpp).  No HIP include: g++ compiles it alone.
//
// The WALK: where the fusion's mask chain looks one level down.  k5_fuse_step (k5_f2c.hpp) upscales the running mask from
// level p + 1 to level p with cv::resize's INTER_NEAREST: pixel x of a side of `fine` pixels reads pixel
// min(floor(x * (1 / (fine / coarse))), coarse - 1) of the side of `coarse` pixels, the scale and the product in double.
// f2c_walk_scale is that scale, f2c_walk_index the index; the same two serve rows and columns.
//
// The UNIQUENESS predicate: a pixel whose winner has a runner-up within the ratio r of it is ambiguous.  A pixel without a
// winner (idx < 0: no visit scanned or painted it) or without a runner-up (runner_idx < 0: one candidate) never is.
//
// Arithmetic contract: every float operation is one IEEE operation in the order written: the product r * score
// is one binary32 multiply.  Host code that includes this header is built with -ffp-contract=off.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RSLF_F2C_PEAK_FN __host__ __device__ __forceinline__
#else
#define RSLF_F2C_PEAK_FN inline
#endif

namespace rslf {

RSLF_F2C_PEAK_FN double f2c_walk_scale(int fine, int coarse) { return 1.0 / ((double)fine / coarse); }

RSLF_F2C_PEAK_FN int f2c_walk_index(int x, double scale, int coarse)
{
    const int n = (int)floor(x * scale);
    return n < coarse - 1 ? n : coarse - 1;
}

RSLF_F2C_PEAK_FN bool f2c_peak_ambiguous(int32_t idx, int32_t runner_idx, float score, float runner_score, float r)
{
    if (idx < 0 || runner_idx < 0)
        return false;
    const float bound = r * score;
    return runner_score > bound;
}

}  // namespace rslf
