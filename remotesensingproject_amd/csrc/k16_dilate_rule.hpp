// The rule of the dilation along u (K16, rslf_volume_dilate_u), stated once for the host and the device: the kinds and
// their taps, the output width, the weight rows and the per-sample arithmetic.  No HIP in here; g++ compiles it alone
// (tests/cpp/dilate_rule_main.cpp restates a whole volume with it, tests/dilate_ref.py says the same in numpy).
//
// A row of U source columns becomes U' = f * (U - 1) + 1 columns; output column j = i * f + p (phase p in [0, f)) lies at
// the source coordinate i + p / f.  Phase 0 copies source column i bit for bit.  Every other phase is
//     acc = w[0] * x[clamp(i - R + 1)];  acc = acc + w[m] * x[clamp(i - R + 1 + m)]  for m = 1 .. T - 1, ascending,
// a binary32 multiply, then a binary32 add (no contraction), indices clamped to [0, U - 1], and out = min(max(acc, lo), hi)
// with the source volume's min and max: nothing leaves [lo, hi], so the dilated volume's range IS the source's.
// The weights are made in double on the host -- w_m = h(p / f - (m - R + 1)), divided by their double sum -- and rounded
// to float: the kernel only reads the table.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RSLF_DILATE_HD __host__ __device__
#else
#define RSLF_DILATE_HD
#endif

#ifndef RSLF_DILATE_LINEAR   // (include/rslf_hip.h defines the same three)
#define RSLF_DILATE_LINEAR 0
#define RSLF_DILATE_CUBIC 1
#define RSLF_DILATE_LANCZOS3 2
#endif

namespace rslf {

constexpr int kDilateMaxFactor = 8;
constexpr int kDilateMaxTaps = 6;

// The weight rows of a call, [phase][tap]; row 0 is never read (phase 0 is a copy) and holds the unit vector.
struct DilateWeights {
    float w[kDilateMaxFactor][kDilateMaxTaps];
};

RSLF_DILATE_HD inline bool dilate_kind_ok(int kind) { return kind == RSLF_DILATE_LINEAR || kind == RSLF_DILATE_CUBIC || kind == RSLF_DILATE_LANCZOS3; }
RSLF_DILATE_HD inline bool dilate_factor_ok(int f) { return f >= 1 && f <= kDilateMaxFactor; }
// The radius R of a kind (0: no such kind); a kind has T = 2 R taps.
RSLF_DILATE_HD inline int dilate_radius(int kind) { return dilate_kind_ok(kind) ? kind + 1 : 0; }
RSLF_DILATE_HD inline int dilate_taps(int kind) { return 2 * dilate_radius(kind); }

// U' = f * (U - 1) + 1 as a 64-bit value (the caller decides what is too wide).
RSLF_DILATE_HD inline long long dilate_width(int U, int f) { return (long long)f * ((long long)U - 1) + 1; }

RSLF_DILATE_HD inline int dilate_clamp(int i, int U) { return i < 0 ? 0 : (i > U - 1 ? U - 1 : i); }

// One output sample of a phase != 0 before the range clamp: column k of the row is x[k * stride + off] (stride: the channel
// count; off: the channel, less where x starts in the row), i the source column the sample follows, w the phase's weight row.
template <int TAPS>
RSLF_DILATE_HD inline float dilate_sum(const float* x, int stride, int off, int i, int U, const float* w)
{
    constexpr int R = TAPS / 2;
    float acc = w[0] * x[dilate_clamp(i - R + 1, U) * stride + off];
    for (int m = 1; m < TAPS; m++) {
        const float prod = w[m] * x[dilate_clamp(i - R + 1 + m, U) * stride + off];
        acc = acc + prod;
    }
    return acc;
}
RSLF_DILATE_HD inline float dilate_range(float acc, float lo, float hi) { return fminf(fmaxf(acc, lo), hi); }

// The source segment a tile of the flattened output row reads.  The tile is the `tile` floats from float e0 of the row
// (float e is column e / C, channel e % C); the segment is the floats [first, first + count) of the source row (row_in floats,
// a multiple of 4), both ends at 16-byte boundaries, and holds the source columns col_lo .. col_hi: every column a sample of
// the tile reads after clamping.  count = 0: the tile lies in the pad and reads nothing.  The kernel stages exactly this
// (k16_dilate.hpp); tests/cpp/test_plan_dilate.cpp holds it to the taps.
struct DilateStage {
    int col_lo, col_hi;   // source columns, inclusive
    int first, count;     // floats of the source row
};
RSLF_DILATE_HD inline DilateStage dilate_stage(int e0, int tile, int U, int U_out, int C, int f, int taps, int row_in)
{
    DilateStage s = {0, -1, 0, 0};
    const int R = taps / 2;
    const int j0 = e0 / C;
    if (j0 >= U_out)
        return s;
    int j1 = (e0 + tile - 1) / C;
    j1 = j1 > U_out - 1 ? U_out - 1 : j1;
    s.col_lo = dilate_clamp(j0 / f - R + 1, U);
    s.col_hi = dilate_clamp(j1 / f + R, U);
    s.first = (s.col_lo * C) & ~3;
    int end = ((s.col_hi + 1) * C + 3) & ~3;
    end = end > row_in ? row_in : end;   // (row_in is a multiple of 64: rounding up stays inside the row)
    s.count = end - s.first;
    return s;
}

// ---- host only from here: the weights and a row as the host restates it ----

// The kernels h, in double.
inline double dilate_sinc(double x)
{
    if (x == 0.0)
        return 1.0;
    const double px = 3.14159265358979323846 * x;
    return sin(px) / px;
}
inline double dilate_kernel(int kind, double x)
{
    const double a = fabs(x);
    switch (kind) {
    case RSLF_DILATE_LINEAR:
        return a < 1.0 ? 1.0 - a : 0.0;
    case RSLF_DILATE_CUBIC:   // Keys, a = -0.5
        if (a <= 1.0)
            return (1.5 * a - 2.5) * a * a + 1.0;
        if (a < 2.0)
            return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0;
        return 0.0;
    case RSLF_DILATE_LANCZOS3:
        return a < 3.0 ? dilate_sinc(x) * dilate_sinc(x / 3.0) : 0.0;
    default:
        return 0.0;
    }
}

// The weight row of phase p of factor f: T floats (the rest of the row zero).
inline void dilate_weight_row(int kind, int f, int p, float* w)
{
    const int R = dilate_radius(kind), T = 2 * R;
    double d[kDilateMaxTaps] = {0, 0, 0, 0, 0, 0}, sum = 0.0;
    for (int m = 0; m < T; m++) {
        d[m] = dilate_kernel(kind, (double)p / (double)f - (double)(m - R + 1));
        sum += d[m];
    }
    for (int m = 0; m < kDilateMaxTaps; m++)
        w[m] = m < T ? (float)(d[m] / sum) : 0.0f;
    if (p == 0)   // the column itself (sin(k pi) is not 0 in double: said, not computed)
        for (int m = 0; m < kDilateMaxTaps; m++)
            w[m] = m == R - 1 ? 1.0f : 0.0f;
}
inline DilateWeights dilate_weights(int kind, int f)
{
    DilateWeights t = {};
    for (int p = 0; p < f && p < kDilateMaxFactor; p++)
        dilate_weight_row(kind, f, p, t.w[p]);
    return t;
}

// A whole row on the host (the yardstick of the stand-alone program): x [U][C] -> out [U'][C].
template <int TAPS>
inline void dilate_row_host(const float* x, int U, int C, int f, const DilateWeights& t, float lo, float hi, float* out, float* unclamped)
{
    const long long Uo = dilate_width(U, f);
    for (long long j = 0; j < Uo; j++) {
        const int i = (int)(j / f), p = (int)(j % f);
        for (int c = 0; c < C; c++) {
            float v, raw;
            if (p == 0)
                v = raw = x[(long long)i * C + c];
            else {
                raw = dilate_sum<TAPS>(x, C, c, i, U, t.w[p]);
                v = dilate_range(raw, lo, hi);
            }
            out[j * C + c] = v;
            if (unclamped)
                unclamped[j * C + c] = raw;
        }
    }
}

}  // namespace rslf
