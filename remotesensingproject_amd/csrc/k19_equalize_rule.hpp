// The rule of the per-view equalisation (K19, rslf_volume_view_stats, rslf_equalize_coefficients, rslf_volume_equalize_views,
// rslf_equalize_views_dense), stated once for the host and the device.  No HIP in here; g++ compiles it alone
// (tests/cpp/equalize_rule_main.cpp restates whole fields with it, tests/equalize_ref.py says the same in numpy).
//
// Three parts, each stated so that any correct implementation gives the same bits.
//
// 1. Quantised statistics.  Floating-point sums depend on their order, so a view's statistic is defined on integers.
//    hi > 0 is the field's cap (a volume: its max_value; a raw integer level: 255 or 65535; a raw float level: its maximum),
//    k = 65535.0f / hi one binary32 division on the host (eq_quant_scale), and per sample
//        q(x) = (uint32) min(rintf(fminf(fmaxf(x, 0.f), hi) * k), 65535.f)
//    A NaN sample is not counted.  Per view s and channel c, over all v and u < U: n = #counted, s1 = sum q, s2 = sum q^2,
//    all uint64, exact while V * U <= 2^31 - 1 (q^2 < 2^32).  A u16 field has q == x, a u8 field q == 257 x.
// 2. Coefficients: eq_coefficients, a pure host function in double.  m = s1 / n / 65535 * hi,
//    var = max(s2 / n / 65535^2 * hi^2 - m^2, 0), sd = sqrt(var) per view and channel; `joint` (C == 3) adds the three
//    channels' n, s1, s2 first (as uint64: exact while 3 * V * U * 65535^2 < 2^64, that is V * U <= kEqMaxSamplesJoint; the
//    entries refuse a joint field beyond it) and writes the one pair to all three, so hue is kept.  The target (mt, sdt) is the reference view's (m, sd), or with ref_view == -1 the arithmetic mean of m and
//    of sd over the views with n > 0, in view order.  GAIN: a = m > 0 ? mt / m : 1, b = 0.  AFFINE: a = sd > 0 ? sdt / sd : 1,
//    b = mt - a m.  a is clamped to [1 / max_gain, max_gain] and b computed after the clamp.  A view with n == 0 and the
//    reference view itself get exactly (1, 0); so does every view when the target has no sample (the reference view's n == 0,
//    or no view's n > 0).  a and b are rounded to binary32 once, at the end.
// 3. Apply: y = x * a + b, one binary32 multiplication, then one addition, never contracted; integer elements then rintf
//    (ties to even, as K17); then y < 0 ? 0 : (y > hi ? hi : y).  A NaN stays that NaN; a pair (1, 0) copies the source's bits.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RSLF_EQ_HD __host__ __device__
#else
#define RSLF_EQ_HD
#endif

// (the values of include/rslf_hip.h's RSLF_EQUALIZE_*)
#define RSLF_EQ_MODE_GAIN   1
#define RSLF_EQ_MODE_AFFINE 2

namespace rslf {

constexpr int kEqStats = 3;                       // (n, s1, s2) per view and channel
constexpr long long kEqMaxSamples = 2147483647;   // V * U beyond this: the sums are no longer exact
constexpr long long kEqMaxSamplesJoint = (long long)(UINT64_MAX / (3ull * 65535ull * 65535ull));   // ... of the joint statistic: three channels' s2 in one uint64

constexpr bool eq_mode_ok(int mode) { return mode == RSLF_EQ_MODE_GAIN || mode == RSLF_EQ_MODE_AFFINE; }
// a cap: finite and > 0 (x - x == 0: finite, without <cmath>'s overloads)
constexpr bool eq_hi_ok(float hi) { return hi == hi && hi - hi == 0.0f && hi > 0.0f; }
constexpr bool eq_max_gain_ok(float g) { return g == g && g - g == 0.0f && g >= 1.0f; }
// hi of an integer element type of `bytes` bytes (1 or 2)
inline float eq_hi_int(int bytes) { return bytes == 1 ? 255.0f : 65535.0f; }
// k of a cap: once, on the host
inline float eq_quant_scale(float hi) { return 65535.0f / hi; }

// q(x) of a sample that is not a NaN (the caller skips those: x != x)
RSLF_EQ_HD inline uint32_t eq_quantise(float x, float hi, float k)
{
    const float c = fminf(fmaxf(x, 0.0f), hi);
    const float p = c * k;
    const float r = fminf(rintf(p), 65535.0f);
    return (uint32_t)r;
}

// One sample into (n, s1, s2).
RSLF_EQ_HD inline void eq_count(float x, float hi, float k, uint64_t* n, uint64_t* s1, uint64_t* s2)
{
    if (x != x)
        return;
    const uint64_t q = eq_quantise(x, hi, k);
    *n += 1;
    *s1 += q;
    *s2 += q * q;
}

// The apply rule for one sample.
template <bool INTEGER>
RSLF_EQ_HD inline float eq_apply(float x, float a, float b, float hi)
{
    if (x != x || (a == 1.0f && b == 0.0f))
        return x;
    const float p = x * a;
    float y = p + b;
    if (INTEGER)
        y = rintf(y);
    return y < 0.0f ? 0.0f : (y > hi ? hi : y);
}

struct EqMoments {
    double m, sd;
    bool counted;
};
inline EqMoments eq_moments(uint64_t n, uint64_t s1, uint64_t s2, double hi)
{
    EqMoments r = {0.0, 0.0, n > 0};
    if (!r.counted)
        return r;
    const double dn = (double)n;
    r.m = (double)s1 / dn / 65535.0 * hi;
    const double e2 = (double)s2 / dn / (65535.0 * 65535.0) * (hi * hi);
    const double mm = r.m * r.m;
    const double var = e2 - mm;
    r.sd = sqrt(var > 0.0 ? var : 0.0);
    return r;
}

// stats [S][C][3] -> a_b [S][C][2].  The caller has checked the arguments (eq_mode_ok, ref_view in [-1, S), joint only with
// C == 3, eq_max_gain_ok, eq_hi_ok).
inline void eq_coefficients(const uint64_t* stats, int S, int C, float hi_f, int mode, int ref_view, int joint, float max_gain, float* a_b)
{
    const double hi = (double)hi_f, gmax = (double)max_gain, gmin = 1.0 / gmax;
    const int G = joint ? 1 : C;   // groups of channels that share a pair
    for (int g = 0; g < G; g++) {
        // the views' moments (view order), then the target
        double mt = 0.0, sdt = 0.0;
        bool target = false;
        if (ref_view < 0) {
            double sum_m = 0.0, sum_sd = 0.0;
            int views = 0;
            for (int s = 0; s < S; s++) {
                uint64_t t[kEqStats] = {0, 0, 0};
                for (int c = joint ? 0 : g; c < (joint ? C : g + 1); c++)
                    for (int i = 0; i < kEqStats; i++)
                        t[i] += stats[((size_t)s * C + c) * kEqStats + i];
                const EqMoments v = eq_moments(t[0], t[1], t[2], hi);
                if (v.counted) {
                    sum_m += v.m;
                    sum_sd += v.sd;
                    views++;
                }
            }
            if (views > 0) {
                mt = sum_m / (double)views;
                sdt = sum_sd / (double)views;
                target = true;
            }
        } else {
            uint64_t r[kEqStats] = {0, 0, 0};
            for (int c = joint ? 0 : g; c < (joint ? C : g + 1); c++)
                for (int i = 0; i < kEqStats; i++)
                    r[i] += stats[((size_t)ref_view * C + c) * kEqStats + i];
            const EqMoments v = eq_moments(r[0], r[1], r[2], hi);
            mt = v.m, sdt = v.sd, target = v.counted;
        }
        for (int s = 0; s < S; s++) {
            uint64_t t[kEqStats] = {0, 0, 0};
            for (int c = joint ? 0 : g; c < (joint ? C : g + 1); c++)
                for (int i = 0; i < kEqStats; i++)
                    t[i] += stats[((size_t)s * C + c) * kEqStats + i];
            const EqMoments v = eq_moments(t[0], t[1], t[2], hi);
            double a = 1.0, b = 0.0;
            if (target && v.counted && s != ref_view) {
                if (mode == RSLF_EQ_MODE_GAIN)
                    a = v.m > 0.0 ? mt / v.m : 1.0;
                else
                    a = v.sd > 0.0 ? sdt / v.sd : 1.0;
                a = a < gmin ? gmin : (a > gmax ? gmax : a);
                if (mode == RSLF_EQ_MODE_AFFINE) {
                    const double am = a * v.m;
                    b = mt - am;
                }
            }
            for (int c = joint ? 0 : g; c < (joint ? C : g + 1); c++) {
                a_b[((size_t)s * C + c) * 2] = (float)a;
                a_b[((size_t)s * C + c) * 2 + 1] = (float)b;
            }
        }
    }
}

}  // namespace rslf
