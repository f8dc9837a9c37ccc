// The rule of the derivative channels (K17, rslf_volume_derivative_channels, rslf_derivative_channels_dense), stated once
// for the host and the device.  No HIP in here; g++ compiles it alone (tests/cpp/derivative_rule_main.cpp restates a whole
// field with it, tests/derivative_ref.py says the same in numpy).
//
// A one-channel field x[v][s][u] becomes three channels per pixel, (x, fu, fv):
//     h  = 0.5f * weight                                  (binary32, once, on the host: derivative_half_weight)
//     fu = cap(fabsf(x[v][s][min(u+1, U-1)] - x[v][s][max(u-1, 0)]) * h, hi)
//     fv = cap(fabsf(x[min(v+1, V-1)][s][u] - x[max(v-1, 0)][s][u]) * h, hi)
// one binary32 subtraction, fabsf, one binary32 multiplication -- nothing that can contract -- and cap(f, hi) = f > hi ? hi : f
// (a NaN stays one).  Channel 0 is the source's bits.  U == 1 gives fu = 0 and V == 1 gives fv = 0: both neighbours are the
// pixel itself.  The neighbour along v is another EPI: the image's second spatial axis.
// Integer elements (the raw levels of CV_8U and CV_16U fields, held as floats with integer values) round the product with
// rintf, ties to even, as cv::saturate_cast does, and hi is the type's 255 or 65535.  For float elements hi is
// max(m, 0) with m the source's maximum, so the field's maximum stays the intensity's.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RSLF_DERIV_HD __host__ __device__
#else
#define RSLF_DERIV_HD
#endif

namespace rslf {

constexpr int kDerivativeChannels = 3;   // (x, fu, fv)

// h of a weight; the entries refuse a weight that is not finite or not > 0 (plan::derivative_weight_ok).
inline float derivative_half_weight(float weight) { return 0.5f * weight; }
// hi of a float source whose maximum is m.
inline float derivative_hi_f32(float m) { return m > 0.0f ? m : 0.0f; }
// hi of an integer element type of `bytes` bytes (1 or 2).
inline float derivative_hi_int(int bytes) { return bytes == 1 ? 255.0f : 65535.0f; }

RSLF_DERIV_HD inline int derivative_left(int u) { return u > 0 ? u - 1 : 0; }
RSLF_DERIV_HD inline int derivative_right(int u, int U) { return u + 1 < U ? u + 1 : U - 1; }

// One feature from its two neighbours: `after` at the larger index.  INTEGER: the product goes through rintf.
template <bool INTEGER>
RSLF_DERIV_HD inline float derivative_feature(float after, float before, float h, float hi)
{
    const float d = after - before;
    float f = fabsf(d) * h;
    if (INTEGER)
        f = rintf(f);
    return f > hi ? hi : f;
}

}  // namespace rslf
