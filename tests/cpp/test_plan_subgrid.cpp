// The sub-grid rule on the host: peak_disp of k8_peak_rule.hpp -- the one function k8_score_peaks (through PeakScan::finish)
// and k9_subgrid_refine call -- held to the rows worked by hand (argv[1]: the file tests/test_subgrid_cpu.py writes from
// tests/peaks_ref.py's table, bit patterns in hex) through its three-score form, to the rule restated here, and to
// peak_row on seeded rows: the two kernels' paths to a disparity give the same bits.
// Built with g++ -ffp-contract=off under AddressSanitizer + UBSan and run directly (tests/test_subgrid_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "k8_peak_rule.hpp"

using namespace rslf;

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

// The rule from its text (include/rslf_hip.h, rslf_peaks::disp)
static float by_definition(int i1, int D, float lo, float hi, float a, float s1, float c)
{
    const float range = hi - lo, denom = (float)(D - 1);
    const float Dd = lo + ((float)i1 * range) / denom;
    float delta = 0.0f;
    if (i1 != 0 && i1 != D - 1) {
        const float den = (a + c) - (s1 + s1);
        const float den2 = den + den;
        delta = den2 == 0.0f ? 0.0f : (a - c) / den2;
        delta = delta < -0.5f ? -0.5f : delta > 0.5f ? 0.5f : delta;
    }
    return Dd + delta * (range / denom);
}

// what k9_subgrid_refine hands the rule for winner i of a row: 0 stands for the neighbour an end of the grid lacks
static float three_scores(const std::vector<float>& s, int i, float lo, float hi)
{
    const int D = (int)s.size();
    const float a = i > 0 ? s[(size_t)i - 1] : 0.0f, c = i < D - 1 ? s[(size_t)i + 1] : 0.0f;
    CHECK(bits(peak_disp(i, D, lo, hi, a, s[(size_t)i], c)) == bits(by_definition(i, D, lo, hi, a, s[(size_t)i], c)));
    return peak_disp(i, D, lo, hi, a, s[(size_t)i], c);
}

static int test_hand_rows(const char* path)
{
    FILE* f = std::fopen(path, "r");
    CHECK(f != nullptr);
    int rows = 0, D = 0, i1 = 0;
    unsigned lo = 0, hi = 0, disp = 0;
    char name[64];
    while (std::fscanf(f, "%63s %d %x %x %d %x", name, &D, &lo, &hi, &i1, &disp) == 6) {
        std::vector<float> s((size_t)D);
        for (int d = 0; d < D; d++) {
            unsigned b = 0;
            CHECK(std::fscanf(f, "%x", &b) == 1);
            s[(size_t)d] = from_bits(b);
        }
        const float got = three_scores(s, i1, from_bits(lo), from_bits(hi));
        if (bits(got) != disp)
            std::printf("row %s: got %.9g want %.9g\n", name, got, from_bits(disp));
        CHECK(bits(got) == disp);
        rows++;
    }
    std::fclose(f);
    CHECK(rows >= 10);
    return rows;
}

static void test_seeded_rows()
{
    // scores on 8 levels, ties everywhere: the winner of a whole row through peak_row, then the same winner through the
    // three-score form; and every OTHER index of the row as a forced winner, within half a step of its grid value
    uint32_t state = 777u;
    auto next = [&]() { return state = state * 1664525u + 1013904223u; };
    int fitted = 0, ends = 0, flat = 0;
    for (int D = 2; D <= 70; D++)
        for (int rep = 0; rep < 100; rep++) {
            std::vector<float> s((size_t)D);
            for (float& x : s)
                x = (float)((next() >> 16) % 8u) * 0.125f + (rep % 5 == 0 ? 0.0f : (float)((next() >> 20) % 3) * 0.001f);
            const float lo = -2.0f + (float)(next() % 1000) * 0.003f, hi = rep % 7 == 0 ? lo : lo + (float)(next() % 1000) * 0.004f;
            const PeakResult whole = peak_row(s.data(), D, lo, hi);
            CHECK(whole.idx >= 0 && whole.idx < D);
            CHECK(bits(three_scores(s, whole.idx, lo, hi)) == bits(whole.disp));
            const float step = (hi - lo) / (float)(D - 1);
            for (int i = 0; i < D; i++) {
                const float grid = lo + ((float)i * (hi - lo)) / (float)(D - 1);
                const float d = three_scores(s, i, lo, hi);
                CHECK(d >= grid - step * 0.50001f - 1e-6f && d <= grid + step * 0.50001f + 1e-6f);
                if (i == 0 || i == D - 1)
                    CHECK(bits(d) == bits(grid + 0.0f * step));
            }
            const bool end = whole.idx == 0 || whole.idx == D - 1;
            const float grid = lo + ((float)whole.idx * (hi - lo)) / (float)(D - 1);
            ends += end, fitted += !end && whole.disp != grid, flat += !end && whole.disp == grid;
        }
    CHECK(fitted > 100 && ends > 100 && flat > 100);
}

int main(int argc, char** argv)
{
    int rows = 0;
    if (argc > 1)
        rows = test_hand_rows(argv[1]);
    // D = 2: both winners are ends of the grid, the scores are not read
    const float nan = from_bits(0x7fc00000u);
    CHECK(peak_disp(0, 2, 0.5f, 0.75f, nan, 1.0f, nan) == 0.5f && peak_disp(1, 2, 0.5f, 0.75f, nan, 1.0f, nan) == 0.75f);
    // interior, a = 1, s1 = 4, c = 3: delta = 0.25, Dd = 2, step = 1
    CHECK(peak_disp(2, 5, 0.0f, 4.0f, 1.0f, 4.0f, 3.0f) == 2.25f);
    test_seeded_rows();
    std::printf("plan subgrid tests ok: %d checks, %d hand-worked rows\n", g_checks, rows);
    return 0;
}
