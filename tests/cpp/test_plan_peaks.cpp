// The score-row peaks on the host: the per-row rule of k8_peak_rule.hpp -- the text the kernel k8_score_peaks compiles --
// held to rows worked by hand (argv[1]: the file tests/test_peaks_cpu.py writes from tests/peaks_ref.py's table, bit
// patterns in hex) and, on seeded rows full of ties, to the rule restated here from its definition over the whole row;
// and the plan functions of rslf_plan_peaks.hpp held to their LDS and grid limits.
// Built with g++ -ffp-contract=off under AddressSanitizer + UBSan and run directly (tests/test_peaks_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "k8_peak_rule.hpp"
#include "rslf_plan_peaks.hpp"

using namespace rslf;
using namespace rslf::plan;

static int g_checks = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        g_checks++;                                                             \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static uint32_t bits(float x)
{
    uint32_t b;
    std::memcpy(&b, &x, sizeof(b));
    return b;
}
static float from_bits(uint32_t b)
{
    float x;
    std::memcpy(&x, &b, sizeof(x));
    return x;
}

// The rule from its definition: the candidate list first, then the two picks, the row indexed at the winner
static PeakResult by_definition(const std::vector<float>& s, float lo, float hi)
{
    const int D = (int)s.size();
    std::vector<int> cand;
    for (int j = 0; j < D; j++)
        if ((j == 0 || s[j] > s[j - 1]) && (j == D - 1 || s[j] >= s[j + 1]))
            cand.push_back(j);
    int i1 = cand[0];
    for (int j : cand)
        if (s[j] > s[i1])
            i1 = j;
    int i2 = -1;
    for (int j : cand)
        if (j != i1 && (i2 < 0 || s[j] > s[i2]))
            i2 = j;
    PeakResult r;
    r.idx = i1, r.score = s[i1], r.runner_idx = i2, r.runner_score = i2 < 0 ? 0.0f : s[i2];
    const float range = hi - lo, denom = (float)(D - 1);
    const float num_d = (float)i1 * range;
    const float quo = num_d / denom;
    const float Dd = lo + quo;
    float delta = 0.0f;
    if (i1 != 0 && i1 != D - 1) {
        const float a = s[i1 - 1], c = s[i1 + 1];
        const float num = a - c;
        const float t = a + c;
        const float bb = s[i1] + s[i1];
        const float den = t - bb;
        const float den2 = den + den;
        delta = den2 == 0.0f ? 0.0f : num / den2;
        delta = delta < -0.5f ? -0.5f : delta > 0.5f ? 0.5f : delta;
    }
    const float step = range / denom;
    const float move = delta * step;
    r.disp = Dd + move;
    return r;
}

static bool same(const PeakResult& x, const PeakResult& y)
{
    return x.idx == y.idx && bits(x.score) == bits(y.score) && bits(x.disp) == bits(y.disp) && x.runner_idx == y.runner_idx &&
           bits(x.runner_score) == bits(y.runner_score);
}

static int test_hand_rows(const char* path)
{
    FILE* f = std::fopen(path, "r");
    CHECK(f != nullptr);
    int rows = 0, D = 0, i1 = 0, i2 = 0;
    unsigned lo = 0, hi = 0, s1 = 0, disp = 0, s2 = 0;
    char name[64];
    while (std::fscanf(f, "%63s %d %x %x %d %x %x %d %x", name, &D, &lo, &hi, &i1, &s1, &disp, &i2, &s2) == 9) {
        std::vector<float> s((size_t)D);
        for (int d = 0; d < D; d++) {
            unsigned b = 0;
            CHECK(std::fscanf(f, "%x", &b) == 1);
            s[(size_t)d] = from_bits(b);
        }
        const PeakResult got = peak_row(s.data(), D, from_bits(lo), from_bits(hi));
        const PeakResult want = {i1, from_bits(s1), from_bits(disp), i2, from_bits(s2)};
        if (!same(got, want))
            std::printf("row %s: got (%d, %g, %.9g, %d, %g) want (%d, %g, %.9g, %d, %g)\n", name, got.idx, got.score, got.disp,
                        got.runner_idx, got.runner_score, want.idx, want.score, want.disp, want.runner_idx, want.runner_score);
        CHECK(same(got, want));
        CHECK(same(by_definition(s, from_bits(lo), from_bits(hi)), want));
        rows++;
    }
    std::fclose(f);
    CHECK(rows >= 10);
    return rows;
}

static void test_built_in_rows()
{
    // winner in the interior: a = 1, s1 = 4, c = 3 -> num = -2, den2 = -8, delta = 0.25; Dd = 2, step = 1
    const float r0[] = {0, 1, 4, 3, 2};
    PeakResult r = peak_row(r0, 5, 0.0f, 4.0f);
    CHECK(r.idx == 2 && r.score == 4.0f && r.disp == 2.25f && r.runner_idx == -1 && r.runner_score == 0.0f);
    // D = 2, a plateau: the first element wins, no runner-up, disp is lo
    const float r1[] = {1, 1};
    r = peak_row(r1, 2, 0.5f, 0.75f);
    CHECK(r.idx == 0 && r.disp == 0.5f && r.runner_idx == -1);
    // a tie between two peaks: the first wins, the later one is the runner-up
    const float r2[] = {1, 5, 1, 5, 0};
    r = peak_row(r2, 5, 0.0f, 4.0f);
    CHECK(r.idx == 1 && r.runner_idx == 3 && r.runner_score == 5.0f && r.disp == 1.0f);
    // NaNs: unspecified values, but nothing is indexed
    const float nan = from_bits(0x7fc00000u);
    const float r3[] = {nan, nan, nan};
    r = peak_row(r3, 3, 0.0f, 1.0f);
    CHECK(r.idx >= -1 && r.idx < 3 && r.runner_idx >= -1 && r.runner_idx < 3);
}

static void test_seeded_rows()
{
    // scores on 8 levels: ties, plateaus and tied runners-up everywhere; every D up to 70 and a few beyond the blocks
    uint32_t state = 12345u;
    auto next = [&]() { return state = state * 1664525u + 1013904223u; };
    int fitted = 0, ends = 0, flat = 0, clamped = 0, lone = 0, tied = 0;
    for (int D = 2; D <= 300; D += (D < 70 ? 1 : 23))
        for (int rep = 0; rep < 200; rep++) {
            std::vector<float> s((size_t)D);
            const unsigned levels = rep % 3 == 0 ? 2u : 8u;
            for (float& x : s)
                x = (float)((next() >> 16) % levels) * 0.125f + (rep % 5 == 0 ? 0.0f : (float)((next() >> 20) % 3) * 0.001f);
            const float lo = -2.0f + (float)(next() % 1000) * 0.003f, hi = rep % 7 == 0 ? lo : lo + (float)(next() % 1000) * 0.004f;
            const PeakResult got = peak_row(s.data(), D, lo, hi), want = by_definition(s, lo, hi);
            CHECK(same(got, want));
            CHECK(got.idx >= 0 && got.idx < D && got.runner_idx >= -1 && got.runner_idx < D && got.runner_idx != got.idx);
            const float grid = lo + ((float)got.idx * (hi - lo)) / (float)(D - 1), half = ((hi - lo) / (float)(D - 1)) * 0.5f;
            CHECK(got.disp >= grid - half * 1.0001f - 1e-6f && got.disp <= grid + half * 1.0001f + 1e-6f);
            const bool end = got.idx == 0 || got.idx == D - 1;
            ends += end, fitted += !end && got.disp != grid, flat += !end && got.disp == grid;
            clamped += !end && s[(size_t)got.idx + 1] == got.score;   // c == s1: delta = +0.5 exactly
            lone += got.runner_idx < 0, tied += got.runner_idx >= 0 && got.runner_score == got.score;
        }
    CHECK(fitted > 100 && ends > 100 && flat > 100 && clamped > 10 && lone > 100 && tied > 100);
}

static void test_plan()
{
    const size_t device_lds = (size_t)160 << 10;
    CHECK(kPeakPitch % 2 == 1 && kPeakPitch > kPeakBlock);   // the odd pitch
    CHECK(peaks_lds_bytes() == (size_t)kPeakWaves * 64 * (kPeakBlock + 1) * 4);
    CHECK(peaks_lds_bytes() <= kPeakLdsLimit && kPeakLdsLimit <= device_lds);
    CHECK(4 * peaks_lds_bytes() <= device_lds);   // four workgroups, sixteen waves a CU
    for (int D = 1; D <= 5000; D++) {
        const int nb = peak_blocks(D);
        CHECK(nb >= 1 && (long long)nb * kPeakBlock >= D && (long long)(nb - 1) * kPeakBlock < D);
        CHECK(peak_block_begin(0, D, nb) == 0 && peak_block_begin(nb, D, nb) == D);
        for (int k = 0; k < nb; k++) {
            const int w = peak_block_begin(k + 1, D, nb) - peak_block_begin(k, D, nb);
            CHECK(w >= 1 && w <= kPeakBlock);                                 // a block fits its LDS rows ...
            CHECK(nb == 1 || w * (int)sizeof(float) >= kPeakMinRunBytes);     // ... and no load is a sliver
            CHECK(63 * kPeakPitch + w <= 64 * kPeakPitch);                    // the last pixel's row ends inside the wave's LDS
        }
    }
    for (int D : {kPeakMaxDimD - 1, kPeakMaxDimD}) {
        const int nb = peak_blocks(D);
        CHECK(peak_block_begin(nb, D, nb) == D && peak_block_begin(nb - 1, D, nb) >= D - kPeakBlock);
        CHECK(64ull * (unsigned long long)D <= 0xffffffffull);   // a tile's floats in 32 bits
    }
    CHECK(peak_blocks(2) == 1 && peak_blocks(32) == 1 && peak_blocks(33) == 2 && peak_blocks(64) == 2 && peak_blocks(65) == 3 &&
          peak_blocks(256) == 8 && peak_blocks(257) == 9);
    // grid: one wave per 64 pixels, kPeakWaves per workgroup; 0 = refused
    CHECK(peaks_tiles(1) == 1 && peaks_tiles(64) == 1 && peaks_tiles(65) == 2 && peaks_tiles(210) == 4);
    CHECK(peaks_grid(0) == 0 && peaks_grid(1) == 1 && peaks_grid(256) == 1 && peaks_grid(257) == 2 && peaks_grid(245760) == 960);
    for (long long n : {1LL, 63LL, 64LL, 210LL, 245760LL, 1920LL * 1080, (1LL << 31) + 5}) {
        const unsigned g = peaks_grid(n);
        CHECK(g >= 1 && (long long)g * kPeakWaves * kPeakTile >= n && ((long long)g - 1) * kPeakWaves * kPeakTile < n);
    }
    CHECK(peaks_grid((long long)INT32_MAX * kPeakWaves * kPeakTile) == (unsigned)INT32_MAX);
    CHECK(peaks_grid((long long)INT32_MAX * kPeakWaves * kPeakTile + 1) == 0);
    // passes: the score rows' rule; the host form's planes ride behind the rows
    for (int U : {1, 130, 1920})
        for (int D : {2, 33, 256})
            for (size_t budget : {(size_t)0, (size_t)17 << 10, (size_t)256 << 20}) {
                const int rows = peaks_window_rows(U, D, budget);
                CHECK(rows == score_window_rows(U, D, budget) && rows >= 1);
                CHECK(peaks_staging_bytes(rows, U, D, false) == (size_t)rows * U * D * 4);
                CHECK(peaks_staging_bytes(rows, U, D, true) == (size_t)rows * U * (D + 5) * 4);
            }
    CHECK(peaks_window_rows(130, 33, (size_t)17 << 10) == 1);   // the GPU test's three passes of one scanline
}

int main(int argc, char** argv)
{
    int rows = 0;
    if (argc > 1)
        rows = test_hand_rows(argv[1]);
    test_built_in_rows();
    test_seeded_rows();
    test_plan();
    std::printf("plan peaks tests ok: %d checks, %d hand-worked rows\n", g_checks, rows);
    return 0;
}
