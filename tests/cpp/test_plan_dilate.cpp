// Host test of the dilation's pure decisions (rslf_plan_dilate.hpp) and of its weight rows (k16_dilate_rule.hpp).
// Stand-alone: built by tests/test_dilate_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off.  No HIP.
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rslf_plan_dilate.hpp"

using namespace rslf;
using namespace rslf::plan;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

static int pitch_of(int U) { return ((U + 1 + 63) / 64) * 64; }   // plan::volume_pitch (rslf_plan.hpp)

static void widths()
{
    int w = -7;
    CHECK(dilated_width(1, 1, &w) == kDilateOk && w == 1);
    CHECK(dilated_width(1, 8, &w) == kDilateOk && w == 1);
    CHECK(dilated_width(2, 4, &w) == kDilateOk && w == 5);
    CHECK(dilated_width(33, 2, &w) == kDilateOk && w == 65);
    CHECK(dilated_width(22, 3, &w) == kDilateOk && w == 64);
    CHECK(dilated_width(1920, 8, &w) == kDilateOk && w == 15353);
    CHECK(dilated_width(96, 1, nullptr) == kDilateOk);
    w = -7;
    CHECK(dilated_width(0, 2, &w) == kDilateBadWidth && dilated_width(-5, 2, &w) == kDilateBadWidth);
    CHECK(dilated_width(10, 0, &w) == kDilateBadFactor && dilated_width(10, 9, &w) == kDilateBadFactor);
    CHECK(dilated_width(10, -1, &w) == kDilateBadFactor && dilated_width(0, 0, &w) == kDilateBadWidth);   // (the order)
    CHECK(dilated_width(INT_MAX, 8, &w) == kDilateTooWide && dilated_width(INT_MAX, 1, &w) == kDilateTooWide);
    CHECK(dilated_width(INT_MAX / 8 - 16, 8, &w) == kDilateOk);
    CHECK(w == 8 * (INT_MAX / 8 - 17) + 1);
    CHECK(dilated_width(INT_MAX / 8, 8, &w) == kDilateTooWide);   // U' + 64 must fit an int: the pitch
    w = -7;
    CHECK(dilate_args(10, 2, 3, &w) == kDilateBadKind && dilate_args(10, 2, -1, &w) == kDilateBadKind);
    CHECK(dilate_args(10, 9, 7, &w) == kDilateBadFactor);
    CHECK(dilate_args(10, 2, RSLF_DILATE_LANCZOS3, &w) == kDilateOk && w == 19);
    for (int f = 1; f <= 8; f++)
        for (int U = 1; U <= 70; U++) {
            CHECK(dilated_width(U, f, &w) == kDilateOk && w == f * (U - 1) + 1);
            CHECK(undilated_width(w, f) == U);
            for (int k = 1; k < f; k++)
                CHECK(undilated_width(w + k, f) == 0);
        }
    CHECK(undilated_width(0, 2) == 0 && undilated_width(-3, 2) == 0 && undilated_width(5, 0) == 0 && undilated_width(5, 9) == 0);
    CHECK(dilate_radius(RSLF_DILATE_LINEAR) == 1 && dilate_radius(RSLF_DILATE_CUBIC) == 2 && dilate_radius(RSLF_DILATE_LANCZOS3) == 3);
    CHECK(dilate_radius(3) == 0 && dilate_taps(RSLF_DILATE_LANCZOS3) == 6 && kDilateMaxTaps == 6 && kDilateMaxFactor == 8);
}

static void weight_rows()
{
    for (int kind = 0; kind < 3; kind++) {
        const int R = dilate_radius(kind), T = 2 * R;
        for (int f = 1; f <= 8; f++) {
            const DilateWeights t = dilate_weights(kind, f);
            // phase 0: the unit vector at tap R - 1 (the column itself)
            for (int m = 0; m < kDilateMaxTaps; m++)
                CHECK(t.w[0][m] == (m == R - 1 ? 1.0f : 0.0f));
            for (int p = 0; p < f; p++) {
                double sum = 0.0;
                for (int m = 0; m < T; m++)
                    sum += (double)t.w[p][m];
                CHECK(fabs(sum - 1.0) <= T * (double)FLT_EPSILON);   // 1 ulp (of 1) per tap
                for (int m = T; m < kDilateMaxTaps; m++)
                    CHECK(t.w[p][m] == 0.0f);
                // phase p mirrors phase f - p: w_p[m] == w_{f-p}[T - 1 - m]
                if (p > 0)
                    for (int m = 0; m < T; m++)
                        CHECK(fabsf(t.w[p][m] - t.w[f - p][T - 1 - m]) <= FLT_EPSILON);
            }
            for (int p = f; p < kDilateMaxFactor; p++)
                for (int m = 0; m < kDilateMaxTaps; m++)
                    CHECK(t.w[p][m] == 0.0f);
        }
    }
    // the values everybody knows
    DilateWeights t = dilate_weights(RSLF_DILATE_LINEAR, 4);
    CHECK(t.w[1][0] == 0.75f && t.w[1][1] == 0.25f && t.w[2][0] == 0.5f && t.w[3][1] == 0.75f);
    t = dilate_weights(RSLF_DILATE_CUBIC, 2);
    CHECK(t.w[1][0] == -0.0625f && t.w[1][1] == 0.5625f && t.w[1][2] == 0.5625f && t.w[1][3] == -0.0625f);
    t = dilate_weights(RSLF_DILATE_LANCZOS3, 2);
    CHECK(t.w[1][2] > 0.6f && t.w[1][2] == t.w[1][3] && t.w[1][1] == t.w[1][4] && t.w[1][0] > 0.0f && t.w[1][0] < 0.03f && t.w[1][4] < -0.1f);
}

// Every output column is covered exactly once, every staged index lies inside the clamped range and the stage fits.
static void tiles_of(int U, int f, int C, int taps)
{
    int Uo = 0;
    CHECK(dilated_width(U, f, &Uo) == kDilateOk);
    const int R = taps / 2, pitch_in = pitch_of(U), pitch_out = pitch_of(Uo);
    const long long row = dilate_row_floats(pitch_out, C), tiles = dilate_tiles_per_row(pitch_out, C);
    CHECK(row % kDilateLane == 0 && tiles * kDilateTile >= row && (tiles - 1) * kDilateTile < row);
    std::vector<int> covered((size_t)Uo * C, 0);
    for (long long t = 0; t < tiles; t++) {
        const DilateStage s = dilate_tile_stage(t, U, Uo, C, f, taps, pitch_in);
        const long long e0 = t * kDilateTile;
        if (e0 / C >= Uo) {
            CHECK(s.count == 0);
            continue;
        }
        CHECK(s.count > 0 && s.count <= kDilateStage && s.first % 4 == 0 && s.count % 4 == 0);
        CHECK(s.first >= 0 && (long long)s.first + s.count <= (long long)pitch_in * C);
        CHECK(s.col_lo >= 0 && s.col_hi <= U - 1 && s.col_lo <= s.col_hi);
        for (long long e = e0; e < e0 + kDilateTile && e < row; e++) {
            const long long j = e / C;
            const int c = (int)(e % C);
            if (j >= Uo)
                continue;
            covered[(size_t)e]++;
            const int i = (int)(j / f);
            for (int m = 0; m < taps; m++) {
                const int col = dilate_clamp(i - R + 1 + m, U);
                const long long at = (long long)col * C + c - s.first;
                CHECK(col >= s.col_lo && col <= s.col_hi && at >= 0 && at < s.count);
            }
        }
    }
    for (int v : covered)
        CHECK(v == 1);
}

static void tiles()
{
    CHECK(kDilateTile == 1024 && kDilateBlock * kDilateLane == kDilateTile && kDilateStage % 4 == 0);
    for (int f = 1; f <= 8; f++)
        for (int Uo = 1; Uo <= 300; Uo++) {
            const int U = undilated_width(Uo, f);
            if (!U)
                continue;
            for (int C : {1, 3})
                for (int taps : {2, 4, 6})
                    tiles_of(U, f, C, taps);
        }
    // several tiles per row, and the widest stage: f = 1, three channels, six taps
    for (int U : {700, 1023, 1024, 1025, 1920, 2731, 4096})
        for (int f : {1, 2, 3, 8})
            for (int C : {1, 3})
                tiles_of(U, f, C, 6);
    int worst = 0;
    for (int f = 1; f <= 8; f++)
        for (int C : {1, 3})
            for (int U = 3000; U < 3012; U++) {
                int Uo = 0;
                CHECK(dilated_width(U, f, &Uo) == kDilateOk);
                for (long long t = 0; t < dilate_tiles_per_row(pitch_of(Uo), C); t++) {
                    const int n = dilate_tile_stage(t, U, Uo, C, f, 6, pitch_of(U)).count;
                    worst = n > worst ? n : worst;
                }
            }
    printf("widest stage %d of %d floats\n", worst, kDilateStage);
    CHECK(worst <= kDilateStage && worst > kDilateTile);
}

static void grids()
{
    CHECK(dilate_grid(0) == 0 && dilate_grid(-1) == 0 && dilate_grid(1) == 1 && dilate_grid(2047) == 2047);
    CHECK(dilate_grid(2048) == kDilateGridCap && dilate_grid(1LL << 40) == kDilateGridCap && kDilateGridCap == 2048);
    CHECK(dilate_tiles(6, 128, 1) == 6 && dilate_tiles(6, 128, 3) == 6 && dilate_tiles(4, 2816, 1) == 12 && dilate_tiles(4, 2816, 3) == 36);
    CHECK(dilate_tiles(65535LL * 65535LL, 64, 1) == 65535LL * 65535LL);
    CHECK(undilate_grid_x(0) == 0 && undilate_grid_x(1) == 1 && undilate_grid_x(256) == 1 && undilate_grid_x(257) == 2);
    CHECK(undilate_grid_y(0) == 0 && undilate_grid_y(7) == 7 && undilate_grid_y(65535) == 65535 && undilate_grid_y((size_t)1 << 33) == 65535);
}

int main()
{
    widths();
    weight_rows();
    tiles();
    grids();
    printf("dilate plan tests ok\n");
    return 0;
}
