// The host-side pieces of a kept fine-to-coarse run's peak planes, compiled with g++ alone and run under AddressSanitizer /
// UBSan (tests/test_f2c_peaks_cpu.py): k11_f2c_peak_rule.hpp -- the index function of the fused peaks' walk and the
// uniqueness predicate, the very functions k11_f2c_peaks.hpp's kernels call -- and rslf_plan_f2c_peaks.hpp: the argument
// checks and the byte counts.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "k11_f2c_peak_rule.hpp"
#include "rslf_plan_f2c_peaks.hpp"

using namespace rslf;
using namespace rslf::plan;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

// cv::resize's INTER_NEAREST as k5_fuse_step states it, every step a named double: sx = min(floor(dx * (1 / (W2 / W))), W - 1)
static int nearest_brute(int x, int fine, int coarse)
{
    volatile double ratio = (double)fine / (double)coarse;
    volatile double inv = 1.0 / ratio;
    volatile double pos = (double)x * inv;
    int n = (int)std::floor(pos);
    if (n > coarse - 1)
        n = coarse - 1;
    return n;
}

static void test_walk()
{
    int pairs = 0, odd = 0, clamped = 0;
    for (int R = 1; R <= 40; R++)
        for (int W = 1; W <= 40; W++) {
            int R2 = 0, W2 = 0;
            f2c_level_dims(R, W, &R2, &W2);
            if (R2 < 1 || W2 < 1)
                continue;   // no level below
            pairs++;
            odd += (R % 2) + (W % 2) > 0;
            const double sv = f2c_walk_scale(R, R2), su = f2c_walk_scale(W, W2);
            int last = -1;
            for (int y = 0; y < R; y++) {
                const int n = f2c_walk_index(y, sv, R2);
                CHECK(n == nearest_brute(y, R, R2));
                CHECK(n >= 0 && n < R2);
                CHECK(n >= last && n <= last + 1);   // monotone, no pixel of the coarse side skipped
                last = n;
                // against the exact rational floor(y * R2 / R): the double product never lands on the wrong side of an integer
                // for these sizes, and where the rational index would reach R2 the minimum holds it at R2 - 1
                const int exact = (int)(((long long)y * R2) / R);
                CHECK(n == (exact < R2 - 1 ? exact : R2 - 1));
            }
            CHECK(last == R2 - 1);                    // the last pixel looks at the last pixel
            for (int x = 0; x < W; x++)
                CHECK(f2c_walk_index(x, su, W2) == nearest_brute(x, W, W2));
        }
    CHECK(pairs > 1400 && odd > 1000);
    // where min(..., coarse - 1) bites: a coarse side smaller than the halving gives (any sizes >= 1 are safe in the kernel)
    for (int fine = 1; fine <= 40; fine++)
        for (int coarse = 1; coarse <= fine; coarse++) {
            const double s = f2c_walk_scale(fine, coarse);
            for (int x = 0; x < fine + 3; x++) {   // (past the side too: still inside the coarse side)
                const int n = f2c_walk_index(x, s, coarse);
                CHECK(n >= 0 && n <= coarse - 1);
                clamped += (int)std::floor(x * s) > coarse - 1;
            }
        }
    CHECK(clamped > 0);
    // the hand-made chain of the GPU test: cvRound ties to even, so 11 x 17 halves to 6 x 8 (not 6 x 9) and that to 3 x 4
    int a = 0, b = 0;
    f2c_level_dims(11, 17, &a, &b);
    CHECK(a == 6 && b == 8);
    f2c_level_dims(6, 8, &a, &b);
    CHECK(a == 3 && b == 4);
    CHECK(f2c_walk_index(10, f2c_walk_scale(11, 6), 6) == 5);
    CHECK(f2c_walk_index(16, f2c_walk_scale(17, 8), 8) == 7);
}

static void test_predicate()
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // ties: runner_score == score is kept at r = 1, dropped below it
    CHECK(!f2c_peak_ambiguous(3, 5, 0.8f, 0.8f, 1.0f));
    CHECK(f2c_peak_ambiguous(3, 5, 0.8f, 0.8f, 0.999f));
    CHECK(f2c_peak_ambiguous(3, 5, 0.8f, 0.81f, 1.0f));    // (a later candidate as high as the winner cannot score more; a caller's planes can)
    // r at its other end: the smallest ratio drops every pixel with a positive runner-up
    const float tiny = std::numeric_limits<float>::denorm_min();
    CHECK(f2c_peak_ambiguous(0, 1, 1.0f, 1e-30f, tiny));
    CHECK(!f2c_peak_ambiguous(0, 1, 1.0f, 0.0f, tiny));
    // no winner, no runner-up: never ambiguous, whatever the scores say
    CHECK(!f2c_peak_ambiguous(-1, 5, 0.1f, 0.9f, 0.5f));
    CHECK(!f2c_peak_ambiguous(3, -1, 0.1f, 0.9f, 0.5f));
    CHECK(!f2c_peak_ambiguous(-1, -1, 0.0f, 0.0f, 0.5f));
    // the bound is one binary32 product: 0.7f * 0.3f rounds to 0.21000001f, and a runner-up of exactly that is not above it
    const float bound = 0.7f * 0.3f;
    CHECK(!f2c_peak_ambiguous(1, 2, 0.3f, bound, 0.7f));
    CHECK(f2c_peak_ambiguous(1, 2, 0.3f, std::nextafter(bound, 1.0f), 0.7f));
    CHECK((double)bound != 0.7 * 0.3);   // (the double product differs: the float one is what counts)
    // a NaN score compares false: kept
    CHECK(!f2c_peak_ambiguous(1, 2, nan, 0.5f, 0.7f));
    CHECK(!f2c_peak_ambiguous(1, 2, 0.5f, nan, 0.7f));
}

static void test_args()
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(f2c_peaks_args(0, 0.0f, 9) == kF2cPeaksOk);
    CHECK(f2c_peaks_args(1, 0.0f, 9) == kF2cPeaksOk);
    CHECK(f2c_peaks_args(1, 0.7f, 9) == kF2cPeaksOk);
    CHECK(f2c_peaks_args(1, 1.0f, 9) == kF2cPeaksOk);
    CHECK(f2c_peaks_args(2, 0.0f, 9) == kF2cPeaksBadFlag);
    CHECK(f2c_peaks_args(-1, 0.5f, 9) == kF2cPeaksBadFlag);
    CHECK(f2c_peaks_args(1, -0.1f, 9) == kF2cPeaksBadRatio);
    CHECK(f2c_peaks_args(1, 1.0001f, 9) == kF2cPeaksBadRatio);
    CHECK(f2c_peaks_args(1, nan, 9) == kF2cPeaksBadRatio);
    CHECK(f2c_peaks_args(0, nan, 9) == kF2cPeaksBadRatio);
    CHECK(f2c_peaks_args(0, 0.7f, 9) == kF2cPeaksRatioAlone);
    CHECK(f2c_peaks_args(1, 0.7f, kPeakMaxDimD) == kF2cPeaksOk);
    CHECK(f2c_peaks_args(1, 0.0f, kPeakMaxDimD + 1) == kF2cPeaksBadDimD);
    CHECK(f2c_peaks_args(0, 0.0f, kPeakMaxDimD + 1) == kF2cPeaksOk);   // without peaks the sweeps take what they always took
    CHECK(f2c_uniqueness_ok(0.0f) && f2c_uniqueness_ok(1.0f) && !f2c_uniqueness_ok(nan) && !f2c_uniqueness_ok(-0.5f));
    // the level accepted whole is not touched; an off ratio touches nothing
    CHECK(!f2c_unique_applies(0.7f, kValidAll));
    CHECK(f2c_unique_applies(0.7f, kValidEdgeConf) && f2c_unique_applies(0.7f, kValidLineConf) && f2c_unique_applies(1.0f, kValidDispConf));
    CHECK(!f2c_unique_applies(0.0f, kValidEdgeConf));
    // the validity rule keeps its two values: the ratio is no third one
    CHECK(f2c_validity_rule_ok(0) && f2c_validity_rule_ok(1) && !f2c_validity_rule_ok(2));
    CHECK(f2c_fuse_peaks_grid_ok(5, 44, 64) && !f2c_fuse_peaks_grid_ok(0, 44, 64) && !f2c_fuse_peaks_grid_ok(5, 65536, 64));
}

static void test_bytes()
{
    const std::vector<LevelDims> dims = f2c_pyramid(44, 64, -1);
    CHECK(dims.size() == 3 && dims[1].V == 22 && dims[2].U == 16);
    const int S = 5;
    CHECK(f2c_peaks_level_bytes(true, S, dims[0]) == (size_t)S * 44 * 64 * 16);
    CHECK(f2c_peaks_level_bytes(false, S, dims[0]) == 0);
    CHECK(f2c_peaks_level_bytes(true, 0, dims[0]) == 0);
    CHECK(f2c_peaks_level_bytes(true, S, LevelDims{0, 4}) == 0);
    size_t want = (size_t)S * 44 * 64 * 17;   // the fused four and fused_level
    for (const LevelDims& d : dims)
        want += (size_t)S * d.V * d.U * 16;
    CHECK(f2c_peaks_bytes(true, S, dims) == want);
    CHECK(f2c_peaks_bytes(false, S, dims) == 0);
    CHECK(f2c_peaks_bytes(true, S, std::vector<LevelDims>()) == 0);
    // the kept run's own counts keep their values: three float planes and the validity per level, the fused map and validity
    CHECK(f2c_kept_level_bytes(S, 1, dims[0], kLineConfOff, false) == (size_t)S * 44 * 64 * 13);
    size_t kept = (size_t)S * 44 * 64 * 5;
    for (const LevelDims& d : dims)
        kept += (size_t)S * d.V * d.U * 13;
    CHECK(f2c_kept_bytes(S, 1, dims, kLineConfOff, false) == kept);
}

int main()
{
    test_walk();
    test_predicate();
    test_args();
    test_bytes();
    std::printf("f2c peaks plan tests ok\n");
    return 0;
}
