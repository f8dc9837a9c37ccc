// Host test of the consistency check's pure decisions (rslf_plan_consistency.hpp) and of its per-pixel rule
// (k12_consistency_rule.hpp).  Stand-alone: built by tests/test_consistency_cpu.py with g++ -fsanitize=address,undefined
// -ffp-contract=off.  No HIP.
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "rslf_plan_consistency.hpp"

using namespace rslf;
using namespace rslf::plan;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

static const float kNan = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

static void arguments()
{
    CHECK(consistency_args(3, 2, 5, 0.0f, 0, true, false) == kConsistencyOk);
    CHECK(consistency_args(1, 1, 1, 0.125f, 7, true, false) == kConsistencyOk);
    CHECK(consistency_args(0, 2, 5, 0.1f, 0, true, false) == kConsistencyBadShape);
    CHECK(consistency_args(3, 0, 5, 0.1f, 0, true, false) == kConsistencyBadShape);
    CHECK(consistency_args(3, 2, -1, 0.1f, 0, true, false) == kConsistencyBadShape);
    CHECK(consistency_args(3, 2, 5, -0.1f, 0, true, false) == kConsistencyBadTol);
    CHECK(consistency_args(3, 2, 5, kNan, 0, true, false) == kConsistencyBadTol);
    CHECK(consistency_args(3, 2, 5, kInf, 0, true, false) == kConsistencyBadTol);
    CHECK(consistency_args(3, 2, 5, -0.0f, 0, true, false) == kConsistencyOk);
    CHECK(consistency_args(3, 2, 5, 0.1f, -1, true, false) == kConsistencyBadMinAgree);
    CHECK(consistency_args(3, 2, 5, 0.1f, 0, false, false) == kConsistencyNoOutput);
    CHECK(consistency_args(3, 2, 5, 0.1f, 0, true, true) == kConsistencyAlias);
    // the order of the refusals: shape, tol, min_agree, outputs, alias
    CHECK(consistency_args(0, 2, 5, kNan, -1, false, true) == kConsistencyBadShape);
    CHECK(consistency_args(3, 2, 5, kNan, -1, false, true) == kConsistencyBadTol);
    CHECK(consistency_args(3, 2, 5, 0.1f, -1, false, true) == kConsistencyBadMinAgree);
    CHECK(consistency_args(3, 2, 5, 0.1f, 0, false, true) == kConsistencyNoOutput);
}

static void grid_and_bytes()
{
    CHECK(consistency_segments(1) == 1 && consistency_segments(256) == 1 && consistency_segments(257) == 2);
    CHECK(consistency_segments(kConsistencyMaxU) == kConsistencyMaxU / 256 && consistency_segments(INT_MAX) == (1 << 23));
    // 8 * ceil(V / 8) scanlines of S * segments workgroups
    CHECK(consistency_grid(9, 3, 300) == 8u * 9 * 2);
    CHECK(consistency_grid(1, 8, 70) == 8u && consistency_grid(1, 9, 70) == 16u);
    CHECK(consistency_grid(101, 1080, 1920) == 1080u * 101 * 8);
    CHECK(consistency_grid(0, 3, 300) == 0 && consistency_grid(9, 0, 300) == 0 && consistency_grid(9, 3, 0) == 0);
    CHECK(consistency_grid(1, 1, kConsistencyMaxU) == 8u * (kConsistencyMaxU / 256));
    CHECK(consistency_grid(1, 1, kConsistencyMaxU + 1) == 0);
    // the limit itself: the largest grid that fits, and the first that does not
    CHECK(consistency_grid(INT_MAX / 8, 8, 1) == (unsigned)(INT_MAX / 8) * 8u);
    CHECK(consistency_grid(INT_MAX / 8 + 1, 8, 1) == 0);
    CHECK(consistency_grid(INT_MAX, INT_MAX, 1) == 0 && consistency_grid(INT_MAX, 1, kConsistencyMaxU) == 0);
    CHECK(consistency_out_bytes_per_cell(4, true, true) == kConsistencyStageOutBytes);
    CHECK(consistency_out_bytes_per_cell(0, false, true) == 1 && consistency_out_bytes_per_cell(2, true, false) == 12);
    CHECK(consistency_bytes(101, 1080, 1920, true, 4, true, true) == (size_t)101 * 1080 * 1920 * 26);
    CHECK(consistency_bytes(2, 3, 5, false, 0, false, true) == 30u * 5);
}

static void windows()
{
    int t0, t1;
    consistency_window(4, 9, 0, &t0, &t1);
    CHECK(t0 == 0 && t1 == 8);
    consistency_window(4, 9, -3, &t0, &t1);
    CHECK(t0 == 0 && t1 == 8);
    consistency_window(4, 9, 2, &t0, &t1);
    CHECK(t0 == 2 && t1 == 6);
    consistency_window(0, 9, 2, &t0, &t1);
    CHECK(t0 == 0 && t1 == 2);
    consistency_window(8, 9, 2, &t0, &t1);
    CHECK(t0 == 6 && t1 == 8);
    consistency_window(8, 9, INT_MAX, &t0, &t1);   // no overflow of s + radius
    CHECK(t0 == 0 && t1 == 8);
    consistency_window(0, 1, 5, &t0, &t1);
    CHECK(t0 == 0 && t1 == 0);
    CHECK(consistency_window_rows(4, 9, 2) == 5 && consistency_window_rows(0, 9, 2) == 3 && consistency_window_rows(3, 9, 0) == 9);
    CHECK(consistency_window_rows(0, 1, 0) == 1);
}

static void rule_pieces()
{
    CHECK(consistency_finite(0.0f) && consistency_finite(-3.4e38f) && consistency_finite(FLT_MAX));
    CHECK(!consistency_finite(kNan) && !consistency_finite(kInf) && !consistency_finite(-kInf));
    CHECK(consistency_ok(1.0f, 255) && consistency_ok(1.0f, 1) && !consistency_ok(1.0f, 0) && !consistency_ok(kNan, 255));
    // the offset: two products, the first rounded before the second
    const float d = 0.1f, slope = 3.0f;
    const float first = d * 7.0f;
    CHECK(consistency_offset(d, 9, 2, slope) == first * slope);
    CHECK(consistency_offset(2.0f, 1, 4, 0.5f) == -3.0f);
    // the column: ties away from zero, out of field past either end, and nothing converted at or past 1e9 or for a NaN
    int x = -7;
    CHECK(consistency_column(0.5f, 10, 20, &x) && x == 11);
    CHECK(consistency_column(-0.5f, 10, 20, &x) && x == 9);
    CHECK(consistency_column(0.49999997f, 10, 20, &x) && x == 10);
    CHECK(consistency_column(2.5f, 10, 20, &x) && x == 13);
    CHECK(consistency_column(9.4f, 10, 20, &x) && x == 19);
    x = -7;
    CHECK(!consistency_column(9.5f, 10, 20, &x) && x == -7);
    CHECK(!consistency_column(-10.5f, 10, 20, &x) && x == -7);
    CHECK(consistency_column(-10.4f, 10, 20, &x) && x == 0);
    x = -7;
    CHECK(!consistency_column(1e9f, 0, kConsistencyMaxU, &x) && !consistency_column(-1e9f, 0, kConsistencyMaxU, &x));
    CHECK(!consistency_column(1e30f, 5, 20, &x) && !consistency_column(-kInf, 5, 20, &x) && !consistency_column(kNan, 5, 20, &x));
    CHECK(x == -7);
    // the largest offset that is converted, at the widest row: u + offset stays an int (UBSan watches the addition)
    const float big = nextafterf(1e9f, 0.0f);
    CHECK(!consistency_column(big, kConsistencyMaxU - 1, kConsistencyMaxU, &x));
    CHECK(consistency_column(-big, kConsistencyMaxU - 1, kConsistencyMaxU, &x) && x == kConsistencyMaxU - 1 - 999999936);
    CHECK(!consistency_column(-big, 0, kConsistencyMaxU, &x));
    // the classification: the first line that matches
    ConsistencyAcc a = consistency_start(1.0f);
    consistency_visit(&a, true, 1.0f, 1.125f, true, 0.125f);     // |diff| == tol: agrees
    CHECK(a.seen == 1 && a.agree == 1 && a.above == 0 && a.below == 0 && a.sum == 2.125f);
    consistency_visit(&a, true, 1.0f, 1.25f, true, 0.125f);      // above
    CHECK(a.seen == 2 && a.agree == 1 && a.above == 1 && a.below == 0 && a.sum == 2.125f);
    consistency_visit(&a, true, 1.0f, 0.5f, true, 0.125f);       // below
    CHECK(a.seen == 3 && a.agree == 1 && a.above == 1 && a.below == 1);
    consistency_visit(&a, true, 1.0f, 1.0f, false, 0.125f);      // in field, its pixel not ok: seen only
    CHECK(a.seen == 4 && a.agree == 1 && a.above == 1 && a.below == 1 && a.sum == 2.125f);
    consistency_visit(&a, false, 1.0f, 1.0f, true, 0.125f);      // out of field: nothing
    CHECK(a.seen == 4 && a.agree == 1 && a.sum == 2.125f);
    consistency_visit(&a, true, -3e38f, 3e38f, true, 0.125f);    // the difference overflows to +inf: above, not a NaN
    CHECK(a.above == 2);
    ConsistencyResult r = consistency_finish(a, 1);
    CHECK(r.seen == 5 && r.agree == 1 && r.fused == 2.125f / 2.0f && r.valid == 255);
    CHECK(consistency_finish(a, 2).valid == 0 && consistency_finish(a, 0).valid == 255);
    r = consistency_nothing();
    CHECK(r.seen == 0 && r.agree == 0 && r.above == 0 && r.below == 0 && r.fused == 0.0f && r.valid == 0);
    ConsistencyAcc z = consistency_start(0.75f);
    CHECK(consistency_finish(z, 0).fused == 0.75f);   // nobody agrees: the pixel's own value
}

// One scanline, three views, followed by hand (slope 1, tol 0.125).
static void rule_pixel()
{
    const int S = 3, V = 1, U = 6;
    //                      u: 0     1     2     3     4     5
    const float depth[S * U] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f,      // view 0
                                1.0f, 1.0f, 1.0f, kNan, 2.0f, 1.0f,      // view 1
                                1.0f, 1.0f, 1.1f, 0.0f, 1.0f, 1.0f};     // view 2
    const uint8_t valid[S * U] = {255, 255, 255, 255, 255, 255, 255, 0, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255};
    // (1, 0, 2), d = 1: view 0 at column 2 + 1 = 3 holds 1 (agree); view 2 at column 2 - 1 = 1 holds 1 (agree)
    ConsistencyResult r = consistency_pixel(depth, valid, S, V, U, 1, 0, 2, 1.0f, 0.125f, 0, 2);
    CHECK(r.seen == 2 && r.agree == 2 && r.above == 0 && r.below == 0 && r.fused == 1.0f && r.valid == 255);
    // (0, 0, 3), d = 1: view 1 at column 2 holds 1 (agree), view 2 at column 1 holds 1 (agree)
    r = consistency_pixel(depth, valid, S, V, U, 0, 0, 3, 1.0f, 0.125f, 0, 0);
    CHECK(r.seen == 2 && r.agree == 2);
    // (0, 0, 5), d = 1: view 1 at column 4 holds 2 (above), view 2 at column 3 holds 0 (below)
    r = consistency_pixel(depth, valid, S, V, U, 0, 0, 5, 1.0f, 0.125f, 0, 1);
    CHECK(r.seen == 2 && r.agree == 0 && r.above == 1 && r.below == 1 && r.fused == 1.0f && r.valid == 0);
    // (0, 0, 4), d = 1: view 1 at column 3 holds a NaN (seen only), view 2 at column 2 holds 1.1 (agree): fused (1 + 1.1) / 2
    r = consistency_pixel(depth, valid, S, V, U, 0, 0, 4, 1.0f, 0.125f, 0, 1);
    CHECK(r.seen == 2 && r.agree == 1 && r.above == 0 && r.below == 0 && r.fused == (1.0f + 1.1f) / 2.0f && r.valid == 255);
    // (0, 0, 2), d = 1: view 1 at column 1 is invalid (seen only), view 2 at column 0 agrees
    r = consistency_pixel(depth, valid, S, V, U, 0, 0, 2, 1.0f, 0.125f, 0, 0);
    CHECK(r.seen == 2 && r.agree == 1);
    // (0, 0, 0), d = 1: view 1 at column -1 and view 2 at column -2 are out of field
    r = consistency_pixel(depth, valid, S, V, U, 0, 0, 0, 1.0f, 0.125f, 0, 0);
    CHECK(r.seen == 0 && r.agree == 0 && r.fused == 1.0f && r.valid == 255);
    // (1, 0, 3) is a NaN and (1, 0, 1) is invalid: nothing
    r = consistency_pixel(depth, valid, S, V, U, 1, 0, 3, 1.0f, 0.125f, 0, 0);
    CHECK(r.seen == 0 && r.fused == 0.0f && r.valid == 0);
    r = consistency_pixel(depth, valid, S, V, U, 1, 0, 1, 1.0f, 0.125f, 0, 0);
    CHECK(r.seen == 0 && r.fused == 0.0f && r.valid == 0);
    // ... and valid again without the plane
    r = consistency_pixel(depth, nullptr, S, V, U, 1, 0, 1, 1.0f, 0.125f, 0, 0);
    CHECK(r.seen == 2 && r.agree == 2 && r.valid == 255);
    // radius 1 from view 0: view 2 is not asked
    r = consistency_pixel(depth, valid, S, V, U, 0, 0, 5, 1.0f, 0.125f, 1, 0);
    CHECK(r.seen == 1 && r.above == 1 && r.below == 0);
    // slope 0.5 from (2, 0, 2), d = 1.1: view 0 at 2 + round(1.1) = 3 holds 1 (agree), view 1 at 2 + round(0.55) = 3 holds the NaN
    r = consistency_pixel(depth, valid, S, V, U, 2, 0, 2, 0.5f, 0.125f, 0, 0);
    CHECK(r.seen == 2 && r.agree == 1 && r.fused == (1.1f + 1.0f) / 2.0f);
    // one view: nobody to ask
    r = consistency_pixel(depth, valid, 1, V, U, 0, 0, 2, 1.0f, 0.125f, 0, 0);
    CHECK(r.seen == 0 && r.fused == 1.0f && r.valid == 255);
}

int main()
{
    arguments();
    grid_and_bytes();
    windows();
    rule_pieces();
    rule_pixel();
    printf("consistency plan tests ok\n");
    return 0;
}
