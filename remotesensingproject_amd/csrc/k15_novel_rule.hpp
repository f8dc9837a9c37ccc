// The rule of the novel view (K15), stated once for the device (k15_novel_view.hpp) and for the host
// (rslf_plan_novel.hpp, tests/cpp/test_plan_novel.cpp).  No HIP include: g++ compiles it alone.
//
// K14 (k14_warp_rule.hpp) stops at one source pixel per target pixel, or nothing.  This is the second half of depth-image-based
// rendering: every target pixel gets a disparity (cracks and disocclusions are filled from the background side), and the
// colour is gathered BACKWARDS along that disparity from the views that really see the point, blended at sub-pixel positions.
// Per target t and scanline v, three stages:
//
// A. z-buffer.  K14's rule unchanged (warp_candidate, the order warp_ahead; exclude, radius, nearer): per column x a `hit` and
//    the winner's stored disparity dw(x), its own bits.
//
// B. fill.  A RUN is a maximal stretch of columns without a hit, of length n; its left bound L is the column before it (none
//    at the row's start), its right bound R the column after it (none at the row's end).  The run stays a hole when it has no
//    bound at all or when max_gap > 0 && n > max_gap.  Otherwise every column of it takes the disparity of ONE bound: the only
//    one, or of two the FARTHER -- the smaller warp_z(dw, nearer): a disocclusion belongs to the background --, the left one on
//    equal z (novel_fill_choice).  fill: 0 hole, 1 hit, 2 filled from the left bound, 3 from the right; depth: dw at hits, the
//    bound's bits at filled pixels, 0 at holes.
//
// C. gather and blend.  For a pixel with fill != 0 and disparity d the views are walked in warp_walk_* order; the walk stops
//    at the first view outside the radius and skips `exclude`.  For view s (novel_tap):
//        off = warp_offset(d, s, t, slope)           out of field unless fabsf(off) < 1e9f (nothing else is converted)
//        p   = (float)x - off
//        ur  = (int)roundf(p)                        out of field unless in [0, U)
//    The view AGREES when consistency_ok(depth[s][v][ur], valid byte) and fabsf(depth[s][v][ur] - d) <= tol (tol >= 0; +inf
//    accepts every ok pixel).  Its sample is the reference's linear interpolation (rslf_interpolation.hpp):
//        i0 = floorf(p), i1 = ceilf(p), w = p - (float)i0, both taps clamped into [0, U - 1],
//        sample[c] = (1 - w) * E[i0][c] + w * E[i1][c]         two products and one sum, no FMA
//    An agreeing view joins the blend with weight g = 1.0f / (1.0f + warp_distance(s, t)), in walk order:
//        acc[c] = acc[c] + g * sample[c], wsum = wsum + g
//    and the walk ends after `sources` (>= 1) agreeing views.  n_src is their number.  With n_src > 0 colour[c] = acc[c] /
//    wsum; with n_src == 0 colour is the sample of the FIRST view of the walk that was in field, unverified, and 0 if none
//    was; a hole has 0.  err = warp_residual(colour, L[x], C) against the slab's own row (v, t) (t integral, in [0, S))
//    wherever a colour was taken from a view (n_src > 0 or a first view in field), else 0.  row_err (double, order open) and
//    row_cov sum err over, and count, only the pixels with n_src > 0.
//
// The encoding (the device's): after stage A a column's 64-bit LDS key is decoded in place to an ENTRY, fill code << 32 |
// disparity bits; a thread owns a contiguous chunk of columns (novel_chunk_partials, novel_chunk_fill), the chunks' "last hit
// at or before" / "first hit at or after" are a scan over the threads.  A filled column's entry is written by its chunk's
// owner only, and bounds are hit columns, which nobody rewrites.
//
// Arithmetic contract as k12_consistency_rule.hpp: every float operation is one IEEE binary32 operation in the order written;
// host code that includes this header is built with -ffp-contract=off.
#pragma once

#include "k14_warp_rule.hpp"

namespace rslf {

constexpr int kNovelHole = 0, kNovelHit = 1, kNovelLeft = 2, kNovelRight = 3;

RSLF_K12_FN bool novel_tol_ok(float tol) { return tol >= 0.0f; }   // false for a NaN; +inf passes

// Stage B: what a run of n columns becomes.  dl / dr: the bounds' disparities (read only where the bound exists).
RSLF_K12_FN int novel_fill_choice(bool has_l, bool has_r, int n, int max_gap, float dl, float dr, int nearer)
{
    if ((!has_l && !has_r) || (max_gap > 0 && n > max_gap))
        return kNovelHole;
    if (!has_r)
        return kNovelLeft;
    if (!has_l)
        return kNovelRight;
    return warp_z(dr, nearer) < warp_z(dl, nearer) ? kNovelRight : kNovelLeft;
}

RSLF_K12_FN unsigned long long novel_entry(int code, uint32_t depth_bits) { return ((unsigned long long)(uint32_t)code << 32) | depth_bits; }
RSLF_K12_FN int novel_entry_code(unsigned long long e) { return (int)(e >> 32) & 3; }
RSLF_K12_FN float novel_entry_depth(unsigned long long e) { return warp_bits_float((uint32_t)e); }

// A chunk [x0, x1) of a row of entries (codes 0 / 1): its last hit column (-1: none) and its first (U: none).
RSLF_K12_FN void novel_chunk_partials(const unsigned long long* e, int x0, int x1, int U, int* last, int* first)
{
    int l = -1, f = U;
    for (int x = x0; x < x1; x++)
        if (novel_entry_code(e[x]) == kNovelHit) {
            l = x;
            f = f == U ? x : f;
        }
    *last = l, *first = f;
}

// The second pass over a chunk: before: the last hit column of the row before x0 (-1: none), after: the first at or after x1
// (U: none).  Every no-hit column of the chunk gets its entry; the bounds' entries, wherever they lie, are only read.
RSLF_K12_FN void novel_chunk_fill(unsigned long long* e, int x0, int x1, int U, int before, int after, int max_gap, int nearer)
{
    int l = before;
    int x = x0;
    while (x < x1) {
        if (novel_entry_code(e[x]) == kNovelHit) {
            l = x++;
            continue;
        }
        int end = x + 1;   // the run's end within the chunk
        while (end < x1 && novel_entry_code(e[end]) != kNovelHit)
            end++;
        const int r = end < x1 ? end : after;
        const bool has_l = l >= 0, has_r = r < U;
        const float dl = has_l ? novel_entry_depth(e[l]) : 0.0f, dr = has_r ? novel_entry_depth(e[r]) : 0.0f;
        const int code = novel_fill_choice(has_l, has_r, r - l - 1, max_gap, dl, dr, nearer);   // the whole run's length: L + 1 .. R - 1
        const unsigned long long fill =
            code == kNovelHole ? novel_entry(kNovelHole, 0u) : novel_entry(code, warp_float_bits(code == kNovelLeft ? dl : dr));
        for (; x < end; x++)
            e[x] = fill;
    }
}

// Stage C, one view of one pixel: where the pixel's line meets view s.  Written without a branch: an offset out of range is
// never converted, 0 is in its place.  ur, i0 and i1 are in [0, U) whatever the inputs (clamped): loads may be issued before
// in_field is looked at.
struct NovelTap {
    bool in_field;
    int ur, i0, i1;
    float w;
};
RSLF_K12_FN int novel_clamp(int c, int U) { return c < 0 ? 0 : c >= U ? U - 1 : c; }
RSLF_K12_FN NovelTap novel_tap(float d, int s, int x, int U, float t, float slope)
{
    NovelTap k;
    const float off = warp_offset(d, s, t, slope);
    const bool in_range = fabsf(off) < kConsistencyMaxOffset;   // false for a NaN
    const float p = (float)x - (in_range ? off : 0.0f);         // |p| < 1e9 + 8192: converts
    const int ur = (int)roundf(p);
    k.in_field = in_range & (ur >= 0) & (ur < U);
    k.ur = novel_clamp(ur, U);
    const float f0 = floorf(p);
    k.w = p - f0;
    k.i0 = novel_clamp((int)f0, U);
    k.i1 = novel_clamp((int)ceilf(p), U);
    return k;
}

RSLF_K12_FN bool novel_agrees(float dt, uint8_t vb, float d, float tol) { return consistency_ok(dt, vb) & (fabsf(dt - d) <= tol); }
RSLF_K12_FN float novel_weight(int s, float t) { return 1.0f / (1.0f + warp_distance(s, t)); }
RSLF_K12_FN float novel_lerp(float w, float e0, float e1)
{
    const float a = (1.0f - w) * e0;
    const float b = w * e1;
    return a + b;
}

}  // namespace rslf
