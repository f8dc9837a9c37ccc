// The rule of the view warp (K14), stated once for the device (k14_view_warp.hpp) and for the host
// (tests/cpp/test_plan_warp.cpp).  No HIP include: g++ compiles it alone.
//
// K12 looks along a pixel's own EPI line: a gather.  This is the opposite question: what does a view POSITION t look like, given
// what every other view holds?  A scatter with an occlusion order.  A source pixel (s, v, u) of disparity d lands, in a view at
// position t (a float: it need not be integral and need not lie inside [0, S - 1]), at column
//     x = u + (int)roundf(fl(fl(d * fl((float)s - t)) * slope))
// of the same scanline -- K12's column rule (consistency_offset, consistency_column) with a float view distance; for an
// integral t the two are the same bits.  The pixel is a CANDIDATE for (v, x) when
//     consistency_ok(d, valid byte)                       finite and not masked out
//     s != exclude                                         (the leave-one-out; -1: nobody)
//     radius <= 0 || fabsf((float)s - t) <= (float)radius
//     consistency_column(off, u, U, &x)                    |off| < 1e9 (a NaN is never converted) and x in [0, U)
//
// Among the candidates of one (v, x) the WINNER is
//     the greatest z = nearer >= 0 ? d : -d                (-0.0f and +0.0f are equal)
//     then the smaller view distance fabsf((float)s - t)
//     then the smaller s
// Two candidates of one view with equal d have equal offsets and cannot meet in a column, so the order is total and the winner
// does not depend on the order in which the sources are visited.
//
// The encoding (the device's; the order above is the rule): the views are WALKED in the order (distance, s) -- warp_walk_* below,
// two pointers that leave t to either side -- and a view's place in the walk is its rank.  A candidate's 64-bit key is
//     warp_order_bits(z) << 32 | (~rank & 0xffff) << 16 | s
// whose unsigned maximum is the winner; s and z come back out of the key, and the source column is recomputed from them
// (warp_source_column: the same offset, so the same column).  S and |t| are at most 65536 (kWarpMaxViews, kWarpMaxTarget): a
// rank and a view fit their 16 bits, and (float)s - t is exact to 1/64, so two views never share a distance on one side of t.
// A key of 0 is no candidate (the smallest z, -FLT_MAX, has order bits 0x00800000).
//
// Arithmetic contract as k12_consistency_rule.hpp: every float operation is one IEEE binary32 operation in the order written;
// host code that includes this header is built with -ffp-contract=off.
#pragma once

#include "k12_consistency_rule.hpp"

namespace rslf {

constexpr int kWarpMaxViews = 65536;         // S: a view index and a rank fit 16 bits of the key
constexpr float kWarpMaxTarget = 65536.0f;   // |t|

RSLF_K12_FN bool warp_target_ok(float t) { return fabsf(t) <= kWarpMaxTarget; }   // false for a NaN and for +-inf
RSLF_K12_FN bool warp_target_integral(float t, int S) { return t >= 0.0f && t < (float)S && t == (float)(int)t; }   // (after warp_target_ok)

RSLF_K12_FN float warp_distance(int s, float t) { return fabsf((float)s - t); }
RSLF_K12_FN bool warp_in_window(int s, float t, int radius) { return radius <= 0 || warp_distance(s, t) <= (float)radius; }

// off = fl(fl(d * fl((float)s - t)) * slope)
RSLF_K12_FN float warp_offset(float d, int s, float t, float slope)
{
    const float dist = (float)s - t;
    float off = d * dist;
    off = off * slope;
    return off;
}

// Is (s, v, u) with disparity d and validity byte vb a candidate of the target t, and for which column?  (*x untouched if not.)
RSLF_K12_FN bool warp_candidate(float d, uint8_t vb, int s, int u, int U, float t, int exclude, int radius, float slope, int* x)
{
    const bool asked = consistency_ok(d, vb) & (s != exclude) & warp_in_window(s, t, radius);
    int c = *x;
    const bool in_field = consistency_column(warp_offset(d, s, t, slope), u, U, &c);
    *x = asked & in_field ? c : *x;
    return asked & in_field;
}

RSLF_K12_FN float warp_z(float d, int nearer)
{
    const float z = nearer >= 0 ? d : -d;
    return z == 0.0f ? 0.0f : z;   // -0.0f and +0.0f are one depth
}

RSLF_K12_FN uint32_t warp_float_bits(float x)
{
    union { float f; uint32_t u; } c;
    c.f = x;
    return c.u;
}
RSLF_K12_FN float warp_bits_float(uint32_t b)
{
    union { float f; uint32_t u; } c;
    c.u = b;
    return c.f;
}
// A float's bits as a key whose UNSIGNED order is the float order (plan::radix_key, stated here for both sides).
RSLF_K12_FN uint32_t warp_order_bits(float z)
{
    const uint32_t b = warp_float_bits(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
RSLF_K12_FN float warp_order_bits_inverse(uint32_t key) { return warp_bits_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

RSLF_K12_FN unsigned long long warp_key(float z, int rank, int s)
{
    return ((unsigned long long)warp_order_bits(z) << 32) | ((unsigned long long)(~(uint32_t)rank & 0xffffu) << 16) | (uint32_t)s;
}
RSLF_K12_FN int warp_key_view(unsigned long long key) { return (int)(key & 0xffffu); }
RSLF_K12_FN float warp_key_z(unsigned long long key) { return warp_order_bits_inverse((uint32_t)(key >> 32)); }
// The winner's source column, from what its key holds: the candidate's own offset again (z is d or -d; a zero of either sign
// gives an offset that rounds to 0), clamped into the row whatever the key.
RSLF_K12_FN int warp_source_column(unsigned long long key, int x, int U, float t, int nearer, float slope)
{
    const float z = warp_key_z(key);
    const float off = warp_offset(nearer >= 0 ? z : -z, warp_key_view(key), t, slope);
    const bool in_range = fabsf(off) < kConsistencyMaxOffset;   // consistency_column's guard: true for every candidate's key
    const int moved = (int)roundf(in_range ? off : 0.0f);
    const int c = x - moved;   // (moved = x - u of a candidate in field: |moved| < U; of anything else the clamp holds)
    return c < 0 ? 0 : c >= U ? U - 1 : c;
}

// The views in the order (distance to t, s): two pointers that start either side of t and leave it.  S in [1, kWarpMaxViews],
// warp_target_ok(t).  warp_walk_next: false when no view is left; else *s, and its place is the number of calls before.
struct WarpWalk {
    int lo, hi;   // the next view below t (-1: none left) and the next at or above it (S: none left)
};
RSLF_K12_FN WarpWalk warp_walk_start(float t, int S)
{
    WarpWalk w;
    const float c = ceilf(t);   // |c| <= 65536: converts
    w.hi = c <= 0.0f ? 0 : c >= (float)S ? S : (int)c;
    w.lo = w.hi - 1;
    return w;
}
RSLF_K12_FN bool warp_walk_next(WarpWalk* w, float t, int S, int* s)
{
    const bool has_lo = w->lo >= 0, has_hi = w->hi < S;
    if (!has_lo && !has_hi)
        return false;
    // of equal distances the smaller s: lo
    const bool take_lo = has_lo && (!has_hi || warp_distance(w->lo, t) <= warp_distance(w->hi, t));
    *s = take_lo ? w->lo-- : w->hi++;
    return true;
}

// Is candidate a (z, distance, s) ahead of candidate b?  The rule's order, as the brute-force forms state it.
RSLF_K12_FN bool warp_ahead(float za, float dist_a, int sa, float zb, float dist_b, int sb)
{
    if (za != zb)
        return za > zb;
    if (dist_a != dist_b)
        return dist_a < dist_b;
    return sa < sb;
}

// The leave-one-out residual of one pixel: acc = 0; for c ascending: acc = acc + |colour[c] - L[c]|; acc / (float)C.
RSLF_K12_FN float warp_residual(const float* colour, const float* L, int C)
{
    float acc = 0.0f;
    for (int c = 0; c < C; c++)
        acc = acc + fabsf(colour[c] - L[c]);
    return acc / (float)C;
}

}  // namespace rslf
