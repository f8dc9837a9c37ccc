// CPU unit tests of the renderers' host-side rules (remotesensingproject_amd/csrc/rslf_plan.hpp, "K6, the renderers"):
// built with g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_render_cpu.py.
// The constexpr functions here are the ones the kernels call (k6_render.hpp).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "rslf_plan.hpp"

using namespace rslf::plan;

static int g_checks = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        g_checks++;                                                             \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static uint32_t bits_of(float f)
{
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
static float float_of(uint32_t b)
{
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// The radix select as the library runs it: kRadixPasses passes, each counting the digits of the keys that share the
// prefix found so far and narrowing the rank to one bin.
static float radix_select(const std::vector<float>& v, uint32_t rank)
{
    uint32_t prefix = 0;
    for (int pass = 0; pass < kRadixPasses; pass++) {
        uint32_t hist[kRadixBins] = {0};
        for (float f : v) {
            const uint32_t key = radix_key(bits_of(f));
            if (radix_prefix(key, pass) == prefix)
                hist[radix_digit(key, pass)]++;
        }
        uint32_t within = 0;
        const int bin = radix_narrow(hist, rank, &within);
        CHECK(bin >= 0 && bin < kRadixBins);
        // exactly one bin holds the rank
        uint32_t before = 0;
        int holders = 0;
        for (int b = 0; b < kRadixBins; b++) {
            holders += radix_bin_holds(before, hist[b], rank) ? 1 : 0;
            before += hist[b];
        }
        CHECK(holders == 1);
        prefix = (prefix << kRadixBits) | (uint32_t)bin;
        rank = within;
    }
    return float_of(radix_key_inverse(prefix));
}

static void check_select(std::vector<float> v, uint32_t rank)
{
    const float got = radix_select(v, rank);
    std::nth_element(v.begin(), v.begin() + rank, v.end());
    CHECK(got == v[rank]);   // == : -0.0f and +0.0f are the same element of a sort
}

static void test_key_transform()
{
    // monotone over a sweep of bit patterns: negative floats descending in magnitude, -0, +0, positive ascending
    std::vector<float> sweep;
    for (uint32_t b = 0xff800000u; b > 0x80000001u; b -= 0x00013579u)   // -inf towards -0
        sweep.push_back(float_of(b));
    sweep.push_back(-std::numeric_limits<float>::denorm_min());
    sweep.push_back(-0.0f);
    sweep.push_back(0.0f);
    sweep.push_back(std::numeric_limits<float>::denorm_min());
    for (uint32_t b = 2; b < 0x7f800000u; b += 0x00013579u)
        sweep.push_back(float_of(b));
    sweep.push_back(std::numeric_limits<float>::infinity());
    for (size_t i = 0; i + 1 < sweep.size(); i++) {
        CHECK(sweep[i] <= sweep[i + 1]);
        CHECK(radix_key(bits_of(sweep[i])) < radix_key(bits_of(sweep[i + 1])));
    }
    for (float f : sweep)
        CHECK(radix_key_inverse(radix_key(bits_of(f))) == bits_of(f));
    CHECK(radix_key(bits_of(-0.0f)) + 1 == radix_key(bits_of(0.0f)));
    // NaNs lie beyond the infinities
    CHECK(radix_key(0x7fc00000u) > radix_key(0x7f800000u) && radix_key(0xffc00000u) < radix_key(0xff800000u));
    // digits and prefixes cut the key into kRadixPasses pieces
    const uint32_t k = 0xa1b2c3d4u;
    CHECK(kRadixPasses == 4 && radix_digit(k, 0) == 0xa1 && radix_digit(k, 1) == 0xb2 && radix_digit(k, 2) == 0xc3 && radix_digit(k, 3) == 0xd4);
    CHECK(radix_prefix(k, 0) == 0 && radix_prefix(k, 1) == 0xa1 && radix_prefix(k, 2) == 0xa1b2 && radix_prefix(k, 3) == 0xa1b2c3);
}

static void test_select()
{
    std::mt19937 rng(20260601);
    // N from 1 to 70: every rank
    for (int n = 1; n <= 70; n++) {
        std::vector<float> v(n);
        std::normal_distribution<float> g(0.0f, 3.0f);
        for (float& f : v)
            f = g(rng);
        if (n > 3) {
            v[0] = -0.0f;
            v[1] = 0.0f;
            v[2] = -v[3];
        }
        for (int r = 0; r < n; r++)
            check_select(v, (uint32_t)r);
        check_select(v, (uint32_t)quantile_index(0.02, n));
        check_select(v, (uint32_t)quantile_index(0.98, n));
    }
    // heavy ties: at most 16 distinct values among 10^5 keys, negative ones and both zeros among them
    for (int trial = 0; trial < 6; trial++) {
        const int n = 100000, distinct = 1 + (int)(rng() % 16);
        std::vector<float> values(distinct);
        for (int i = 0; i < distinct; i++)
            values[i] = -2.0f + 0.5f * (float)(int)(rng() % 17) - (i == 0 ? 0.0f : 0.03125f * (float)(rng() % 3));
        values[0] = 0.0f;
        if (distinct > 1)
            values[1] = -0.0f;
        std::vector<float> v(n);
        for (float& f : v)
            f = (rng() % 3 == 0) ? values[0] : values[rng() % distinct];   // a large share of exact zeros
        const uint32_t ranks[] = {0u, (uint32_t)quantile_index(0.02, n), (uint32_t)n / 2, (uint32_t)quantile_index(0.98, n), (uint32_t)n - 1};
        for (uint32_t r : ranks)
            check_select(v, r);
    }
    uint32_t hist[kRadixBins] = {0}, within = 7;
    hist[3] = 2;
    CHECK(radix_narrow(hist, 2, &within) == -1 && radix_narrow(hist, 1, &within) == 3 && within == 1);
}

static void test_fit_rules()
{
    CHECK(quantile_index(0.02, 20) == 0 && quantile_index(0.98, 20) == 19);
    CHECK(quantile_index(0.02, 50) == 1 && quantile_index(0.98, 50) == 49);
    CHECK(quantile_index(0.02, 1) == 0 && quantile_index(0.98, 1) == 0);
    CHECK(quantile_index(0.98, 1080 * 1920) == (int)std::floor(0.98 * 2073600));
    // mean 2, variance 1 over {1, 3}: mean + 12 std = 14, capped by the true max
    CHECK(meanstd_max(4.0, 10.0, 2, 100.0) == 14.0 && meanstd_max(4.0, 10.0, 2, 3.0) == 3.0);
    CHECK(meanstd_max(6.0, 12.0, 3, 9.0) == 2.0);   // a constant plane: variance 0 (never negative under the sqrt)
    CHECK(fit_blocks(1) == 1 && fit_blocks(1024) == 1 && fit_blocks(1025) == 2 && fit_blocks(1 << 30) == kFitMaxBlocks);
}

static void test_render_rules()
{
    const RenderConsts s = render_consts(0, 1.0, 3.0), a = render_consts(1, 1.0, 3.0);
    CHECK(s.a == 1.0f && s.b == 127.5f && a.a == 127.5f && a.b == -127.5f);
    const RenderConsts c = render_consts(0, 2.0, 2.0);   // a constant plane: 255 / 0
    CHECK(std::isinf(c.b) && std::isnan((2.0f - c.a) * c.b) && render_level(std::rint((2.0f - c.a) * c.b)) == 0);
    // cvRound is nearest-even: x.5 goes both ways
    CHECK(render_level(std::rint(0.5f)) == 0 && render_level(std::rint(1.5f)) == 2 && render_level(std::rint(2.5f)) == 2);
    CHECK(render_level(std::rint(254.5f)) == 254 && render_level(std::rint(255.5f)) == 255 && render_level(-3.0f) == 0 && render_level(300.0f) == 255);
    const float inf = std::numeric_limits<float>::infinity();
    CHECK(render_level(inf) == 0 && render_level(-inf) == 0 && render_level(3.0e9f) == 0 && render_level(std::nanf("")) == 0);
    alignas(16) static float buf[8];
    CHECK(render_vec4_ok(1920, 1920, 1920 * 1080, buf, nullptr, buf) && !render_vec4_ok(1919, 1919, 0, buf, nullptr, buf));
    CHECK(!render_vec4_ok(1920, 1921, 0, buf, nullptr, buf) && !render_vec4_ok(4, 4, 0, buf + 1, nullptr, buf));
    CHECK(!render_vec4_ok(4, 4, 0, buf, (const char*)buf + 1, buf) && !render_vec4_ok(4, 4, 6, buf, nullptr, buf));
    CHECK(render_quads(1080, 1920) == 1080ll * 480 && render_quads(3, 5) == 6 && render_quads(2, 1) == 2);
    CHECK(epi_lines_lds_bytes(kEpiLinesMaxU) <= (size_t)64 << 10);
}

static void test_index_rules()
{
    // (int)std::round(n / 2.0): halves away from zero; n itself for n = 1
    CHECK(centre_plane_index(1) == -1 && centre_plane_index(0) == -1);
    CHECK(centre_plane_index(2) == 1 && centre_plane_index(3) == 2 && centre_plane_index(4) == 2 && centre_plane_index(5) == 3);
    CHECK(centre_plane_index(101) == 51);
    // (int)std::round(1.0 * v * dim_v / dim_v_orig)
    CHECK(scaled_row_index(0, 1, 1) == 0 && scaled_row_index(1, 1, 1) == -1 && scaled_row_index(-1, 4, 8) == -1);
    CHECK(scaled_row_index(12, 24, 24) == 12 && scaled_row_index(12, 12, 24) == 6 && scaled_row_index(12, 6, 24) == 3);
    CHECK(scaled_row_index(23, 12, 24) == -1);   // 11.5 rounds up to dim_v
    CHECK(scaled_row_index(22, 12, 24) == 11 && scaled_row_index(1, 12, 24) == 1);   // 0.5 rounds away from zero
    CHECK(scaled_row_index(24, 12, 24) == -1);
    for (int v0 = 1; v0 <= 40; v0++)
        for (int vp = 1; vp <= v0; vp++)
            for (int v = 0; v < v0; v++) {
                const int i = scaled_row_index(v, vp, v0);
                CHECK(i == -1 || (i >= 0 && i < vp));
            }
}

int main()
{
    test_key_transform();
    test_select();
    test_fit_rules();
    test_render_rules();
    test_index_rules();
    std::printf("render plan tests ok: %d checks\n", g_checks);
    return 0;
}
