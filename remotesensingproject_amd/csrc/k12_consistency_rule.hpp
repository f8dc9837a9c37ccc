// The rule of the cross-view consistency check (K12), stated once for the device (k12_consistency.hpp) and for the host
// (tests/cpp/test_plan_consistency.cpp, tests/cpp/consistency_rule_main.cpp).  No HIP include: g++ compiles it alone.
//
// A sweep ends with one disparity plane per view, depth[S][V][U].  A pixel (s, v, u) of disparity d lies, in view t, at
// column u + round(d * (s - t) * slope) of the same scanline -- the propagation's column rule (k4_propagate.hpp, core.hpp:1109)
// with the pixel's own view where the propagation has s_hat.  The check asks every other view t (ascending; with a radius
// only |t - s| <= radius) what it holds there:
//
//   out of field   the offset is not below 1e9 in magnitude (a NaN included; the propagation has no such guard, and the
//                  conversion to int must not be undefined here), or the column is outside [0, U)
//   seen           every other view that is in field
//   agree          ... whose pixel is ok and within tol of d: its disparity joins the running sum
//   above          ... whose pixel is ok and holds MORE than d + tol
//   below          ... whose pixel is ok and holds less (a NaN difference cannot occur: both values are finite)
//
// ok(s, v, u): the validity plane is absent or non-zero there, and the disparity is finite.  A pixel that is not ok has
// four counts of 0, fused 0 and valid_out 0, and is nobody's agreeing, above or below neighbour -- but a view that shows
// such a pixel at the target column still counts as seen.
//
// `above` and `below` are kept apart because what they mean depends on the sign convention of the field.  With
// disparities that GROW towards the camera, a neighbour above is a legitimate occluder (something nearer hides the point in
// that view) and a neighbour below is a free-space violation (that view looks through the point).  With the opposite
// convention the two swap.  The rule counts; the caller decides.
//
// fused = (d + the agreeing views' disparities, added in ascending t) / (1 + agree): the order of the additions is part of
// the definition, so the value is the same bits wherever it is computed.  valid_out = 255 where agree >= min_agree.
//
// Arithmetic contract: every float operation is one IEEE binary32 operation in the order written: the two
// products of the offset are taken one after the other, unfused.  Host code that includes this header is built with
// -ffp-contract=off.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RSLF_K12_FN __host__ __device__ __forceinline__
#else
#define RSLF_K12_FN inline
#endif

namespace rslf {

constexpr float kConsistencyMaxOffset = 1e9f;   // an offset at or past it (or a NaN) is out of field

// What one pixel accumulates over the other views, and what it ends with.
struct ConsistencyAcc {
    int32_t seen, agree, above, below;
    float sum;
};
struct ConsistencyResult {
    int32_t seen, agree, above, below;
    float fused;
    uint8_t valid;
};

RSLF_K12_FN bool consistency_finite(float d) { return fabsf(d) <= 3.402823466e+38f; }   // false for a NaN and for +-inf
RSLF_K12_FN bool consistency_ok(float d, uint8_t valid_byte) { return valid_byte != 0 && consistency_finite(d); }

RSLF_K12_FN ConsistencyAcc consistency_start(float d)
{
    ConsistencyAcc a;
    a.seen = a.agree = a.above = a.below = 0;
    a.sum = d;
    return a;
}

// The views a pixel of view s asks: [*t0, *t1], s itself among them (the loop skips it); radius <= 0: every view.
RSLF_K12_FN void consistency_window(int s, int S, int radius, int* t0, int* t1)
{
    if (radius <= 0 || radius >= S) {
        *t0 = 0;
        *t1 = S - 1;
        return;
    }
    *t0 = s - radius > 0 ? s - radius : 0;
    *t1 = s + radius < S - 1 ? s + radius : S - 1;
}

// off = fl(fl(d * float(s - t)) * slope)
RSLF_K12_FN float consistency_offset(float d, int s, int t, float slope)
{
    float off = d * (float)(s - t);
    off = off * slope;
    return off;
}

// The column of view t that the offset points at; false: out of field (*x untouched).  Written without a branch -- the kernel
// has eight of these ahead of its loads --: an offset out of range is never converted, 0 is in its place.
RSLF_K12_FN bool consistency_column(float off, int u, int U, int* x)
{
    const bool in_range = fabsf(off) < kConsistencyMaxOffset;   // false for a NaN
    const int c = u + (int)roundf(in_range ? off : 0.0f);
    const bool in_field = in_range & (c >= 0) & (c < U);
    *x = in_field ? c : *x;
    return in_field;
}

// One view: in_field says whether it counts at all (the kernel calls this for every view of a batch, without a branch); dt
// and ok_t are what the view holds at the target column.  The first line that matches: agree, above, below.
RSLF_K12_FN void consistency_visit(ConsistencyAcc* a, bool in_field, float d, float dt, bool ok_t, float tol)
{
    const float diff = dt - d;
    const bool there = in_field & ok_t;
    const bool agree = there & (fabsf(diff) <= tol);
    const bool above = there & !agree & (diff > tol);
    const bool below = there & !agree & !above;
    a->seen += in_field ? 1 : 0;
    a->agree += agree ? 1 : 0;
    a->above += above ? 1 : 0;
    a->below += below ? 1 : 0;
    a->sum = agree ? a->sum + dt : a->sum;
}

RSLF_K12_FN ConsistencyResult consistency_finish(const ConsistencyAcc& a, int min_agree)
{
    ConsistencyResult r;
    r.seen = a.seen, r.agree = a.agree, r.above = a.above, r.below = a.below;
    r.fused = a.sum / (float)(1 + a.agree);
    r.valid = a.agree >= min_agree ? 255 : 0;
    return r;
}

// The gate a kept fine-to-coarse run puts on a level's validity (k13_f2c_consistency.hpp): a pixel keeps its
// validity if at least min_agree of the views that can see it agree with it -- and, where fewer than min_agree views can see
// it, if all of them do.  seen == 0 (the pixel's line leaves the field in every view asked): kept.  Unlike valid_out above
// (agree >= min_agree) the rule does not drop a pixel for lying near the field's border or in an outer view of a radius.
RSLF_K12_FN bool consistency_gate(int32_t seen, int32_t agree, int32_t min_agree)
{
    return agree >= (seen < min_agree ? seen : min_agree);
}

// What the gate accumulates: consistency_visit's `seen` and `agree`, the same tests, nothing else.
RSLF_K12_FN void consistency_gate_visit(int32_t* seen, int32_t* agree, bool in_field, float d, float dt, bool ok_t, float tol)
{
    const float diff = dt - d;
    *seen += in_field ? 1 : 0;
    *agree += (in_field & ok_t & (fabsf(diff) <= tol)) ? 1 : 0;
}

RSLF_K12_FN ConsistencyResult consistency_nothing()
{
    ConsistencyResult r;
    r.seen = r.agree = r.above = r.below = 0;
    r.fused = 0.0f;
    r.valid = 0;
    return r;
}

// The whole rule for one pixel, one view after the other: what the kernel computes in batches of views, and what the host
// tests compare it with.  valid: nullable.
RSLF_K12_FN ConsistencyResult consistency_pixel(const float* depth, const uint8_t* valid, int S, int V, int U, int s, int v, int u,
                                                float slope, float tol, int radius, int min_agree)
{
    const long long plane = (long long)V * U, row = (long long)v * U;
    const long long o = (long long)s * plane + row + u;
    const float d = depth[o];
    if (!consistency_ok(d, valid ? valid[o] : (uint8_t)255))
        return consistency_nothing();
    ConsistencyAcc a = consistency_start(d);
    int t0, t1;
    consistency_window(s, S, radius, &t0, &t1);
    for (int t = t0; t <= t1; t++) {
        if (t == s)
            continue;
        int x = u;
        if (!consistency_column(consistency_offset(d, s, t, slope), u, U, &x))
            continue;
        const long long q = (long long)t * plane + row + x;
        const float dt = depth[q];
        consistency_visit(&a, true, d, dt, consistency_ok(dt, valid ? valid[q] : (uint8_t)255), tol);
    }
    return consistency_finish(a, min_agree);
}

}  // namespace rslf
