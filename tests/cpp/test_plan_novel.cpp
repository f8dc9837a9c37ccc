// Host test of the novel view's pure decisions (rslf_plan_novel.hpp) and of its per-pixel rule (k15_novel_rule.hpp).
// Stand-alone: built by tests/test_novel_view_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off.  No HIP.
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "rslf_plan_novel.hpp"

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

static uint32_t lcg(uint32_t* x) { return *x = *x * 1664525u + 1013904223u; }
static float unit(uint32_t* x) { return (float)(lcg(x) >> 8) * (1.0f / 16777216.0f); }

static void arguments()
{
    CHECK(novel_args(true, 1, 0.0f) == kNovelOk && novel_args(true, 4, 0.1f) == kNovelOk && novel_args(true, INT_MAX, kInf) == kNovelOk);
    CHECK(novel_args(false, 1, 0.0f) == kNovelNoParams);
    CHECK(novel_args(true, 0, 0.0f) == kNovelBadSources && novel_args(true, -3, 0.0f) == kNovelBadSources);
    CHECK(novel_args(true, 1, -0.0f) == kNovelOk);
    CHECK(novel_args(true, 1, -1e-30f) == kNovelBadTol && novel_args(true, 1, kNan) == kNovelBadTol && novel_args(true, 1, -kInf) == kNovelBadTol);
    CHECK(novel_args(false, 0, kNan) == kNovelNoParams && novel_args(true, 0, kNan) == kNovelBadSources);   // the order
    // the warp's own list is the novel view's too
    CHECK(warp_args(3, 2, 5, 1, 0, true, false, false, false, 0, 0, 0) == kWarpBadNearer);
    CHECK(warp_args(3, 2, 5, 1, 1, false, false, false, false, 0, 0, 0) == kWarpNoOutput);
    CHECK(warp_args(3, 2, 5, 1, 1, true, true, false, false, 0, 0, 0) == kWarpAlias);
    CHECK(warp_args(3, 2, 5, 1, 1, true, false, true, false, 0, 0, 0) == kWarpNoVolume);
}

static void lds_cap_and_grid()
{
    CHECK(novel_lds_bytes(1) == 8 && novel_lds_bytes(1920) == 15360 && novel_lds_bytes(kWarpMaxU) == ((size_t)64 << 10));
    CHECK(novel_lds_bytes(kWarpMaxU) <= kWarpLdsBudget / 2);   // two workgroups share a CU at the cap
    CHECK(warp_limits(9, 4, kWarpMaxU, 1) == kWarpFits && warp_limits(9, 4, kWarpMaxU + 1, 1) == kWarpTooWide);
    CHECK(warp_limits(kWarpMaxViews + 1, 4, 100, 1) == kWarpTooManyViews && warp_limits(9, 1 << 28, 100, 8) == kWarpGridLimit);
    CHECK(warp_grid(11, 3) == 48u && warp_launches(300) == 2 && warp_launch_targets(300, 1) == 44);
    CHECK(novel_chunk(1) == 1 && novel_chunk(256) == 1 && novel_chunk(257) == 2 && novel_chunk(kWarpMaxU) == 32);
    for (int U : {1, 2, 255, 256, 257, 1920, 8191, 8192})   // the chunks tile the row
        CHECK((long long)novel_chunk(U) * kWarpBlock >= U && (long long)(novel_chunk(U) - 1) * kWarpBlock < U);
    NovelPlanes all = {true, true, true, true, true, true};
    CHECK(novel_out_bytes_per_cell(all, 3) == 1 + 12 + 12);
    CHECK(novel_bytes(3, 2, 10, 1, 1, true, 0.0, all) == (size_t)3 * 20 * 5 + 20 * 4 + 20 * 17 + 2 * 12);
}

// Stage B by the rule's words, column by column: the nearest hit to either side.
static void fill_brute(const std::vector<unsigned long long>& in, std::vector<unsigned long long>& out, int max_gap, int nearer)
{
    const int U = (int)in.size();
    out = in;
    for (int x = 0; x < U; x++) {
        if (novel_entry_code(in[(size_t)x]) == kNovelHit)
            continue;
        int l = x, r = x;
        while (l >= 0 && novel_entry_code(in[(size_t)l]) != kNovelHit)
            l--;
        while (r < U && novel_entry_code(in[(size_t)r]) != kNovelHit)
            r++;
        const int n = r - l - 1;
        int code = kNovelHole;
        if ((l >= 0 || r < U) && !(max_gap > 0 && n > max_gap)) {
            if (l >= 0 && r < U) {
                const float zl = warp_z(novel_entry_depth(in[(size_t)l]), nearer), zr = warp_z(novel_entry_depth(in[(size_t)r]), nearer);
                code = zr < zl ? kNovelRight : kNovelLeft;
            } else {
                code = l >= 0 ? kNovelLeft : kNovelRight;
            }
        }
        out[(size_t)x] = code == kNovelHole ? 0ull : novel_entry(code, (uint32_t)in[(size_t)(code == kNovelLeft ? l : r)]);
    }
}

static void check_fill(const std::vector<unsigned long long>& row)
{
    const int U = (int)row.size();
    for (int nearer : {1, -1})
        for (int max_gap : {0, 1, 3, 40}) {
            std::vector<unsigned long long> want, a = row, b = row;
            fill_brute(row, want, max_gap, nearer);
            novel_fill_chunked(a.data(), U, max_gap, nearer);
            novel_fill_runs(b.data(), U, max_gap, nearer);
            CHECK(a == want);
            CHECK(b == want);
        }
}

static void fill_scan()
{
    CHECK(novel_fill_choice(false, false, 3, 0, 0.0f, 0.0f, 1) == kNovelHole);
    CHECK(novel_fill_choice(true, false, 3, 0, 1.0f, 0.0f, 1) == kNovelLeft && novel_fill_choice(false, true, 3, 0, 0.0f, 1.0f, 1) == kNovelRight);
    CHECK(novel_fill_choice(true, true, 3, 3, 2.0f, 0.5f, 1) == kNovelRight && novel_fill_choice(true, true, 3, 3, 2.0f, 0.5f, -1) == kNovelLeft);
    CHECK(novel_fill_choice(true, true, 4, 3, 2.0f, 0.5f, 1) == kNovelHole && novel_fill_choice(true, false, 4, 3, 2.0f, 0.0f, 1) == kNovelHole);
    CHECK(novel_fill_choice(true, true, 1, 0, 0.0f, -0.0f, 1) == kNovelLeft && novel_fill_choice(true, true, 1, 0, -0.0f, 0.0f, -1) == kNovelLeft);
    uint32_t seed = 7;
    for (int U : {1, 2, 255, 256, 257, 8192}) {
        const float values[5] = {0.5f, 2.0f, -0.0f, 0.0f, -1.25f};
        for (int per_mille : {0, 2, 100, 500, 900, 1000}) {   // no-hit and all-hit rows among them
            std::vector<unsigned long long> row((size_t)U, 0ull);
            for (int x = 0; x < U; x++)
                if ((int)(lcg(&seed) >> 8) % 1000 < per_mille)
                    row[(size_t)x] = novel_entry(kNovelHit, warp_float_bits(values[(lcg(&seed) >> 8) % 5]));
            check_fill(row);
        }
        // one hit only, at either end and in the middle: runs that span every other thread's chunk
        for (int at : {0, U / 2, U - 1}) {
            std::vector<unsigned long long> row((size_t)U, 0ull);
            row[(size_t)at] = novel_entry(kNovelHit, warp_float_bits(2.0f));
            check_fill(row);
        }
        // two hits a long run apart, the run's ends on chunk boundaries and one column off them
        const int chunk = novel_chunk(U);
        for (int off : {-1, 0, 1}) {
            const int a = chunk * 3 + off, b = chunk * 200 + off;
            if (a < 0 || b >= U || a >= b)
                continue;
            std::vector<unsigned long long> row((size_t)U, 0ull);
            row[(size_t)a] = novel_entry(kNovelHit, warp_float_bits(2.0f));
            row[(size_t)b] = novel_entry(kNovelHit, warp_float_bits(0.5f));
            check_fill(row);
        }
    }
}

static void taps()
{
    // integral positions: both taps the pixel, w = 0; between two pixels: the neighbours; at the row's ends: clamped
    NovelTap k = novel_tap(1.0f, 2, 10, 20, 1.0f, 1.0f);   // off = 1: p = 9
    CHECK(k.in_field && k.ur == 9 && k.i0 == 9 && k.i1 == 9 && k.w == 0.0f);
    k = novel_tap(0.5f, 2, 10, 20, 1.0f, 1.0f);            // p = 9.5: roundf away from zero
    CHECK(k.in_field && k.ur == 10 && k.i0 == 9 && k.i1 == 10 && k.w == 0.5f);
    k = novel_tap(0.25f, 0, 0, 20, 1.0f, 1.0f);            // off = -0.25: p = 0.25
    CHECK(k.in_field && k.ur == 0 && k.i0 == 0 && k.i1 == 1 && k.w == 0.25f);
    k = novel_tap(-0.25f, 0, 0, 20, 1.0f, 1.0f);           // p = -0.25: rounds to -0 -> column 0, the left tap clamped
    CHECK(k.in_field && k.ur == 0 && k.i0 == 0 && k.i1 == 0 && k.w == 0.75f);
    k = novel_tap(-0.25f, 2, 19, 20, 1.0f, 1.0f);          // p = 19.25: the right tap clamped
    CHECK(k.in_field && k.ur == 19 && k.i0 == 19 && k.i1 == 19);
    k = novel_tap(-0.5f, 2, 19, 20, 1.0f, 1.0f);           // p = 19.5 -> 20: out of field
    CHECK(!k.in_field && k.ur == 19);
    for (float d : {kNan, kInf, -kInf, 1e30f, -1e30f, 1e9f, -1e9f}) {
        k = novel_tap(d, 3, 5, 20, 1.0f, 1.0f);
        CHECK(!k.in_field && k.ur >= 0 && k.ur < 20 && k.i0 >= 0 && k.i0 < 20 && k.i1 >= 0 && k.i1 < 20);
        k = novel_tap(1.0f, 3, 5, 20, 1.0f, d);
        CHECK(!k.in_field && k.ur >= 0 && k.ur < 20 && k.i0 >= 0 && k.i0 < 20 && k.i1 >= 0 && k.i1 < 20);
    }
    k = novel_tap(0.0f, 3, 5, 20, 1.0f, 1e30f);            // a zero offset stays in field
    CHECK(k.in_field && k.ur == 5);
    CHECK(novel_agrees(1.0f, 255, 1.1f, 0.125f) && !novel_agrees(1.0f, 0, 1.0f, 0.125f) && !novel_agrees(kNan, 255, 1.0f, kInf));
    CHECK(novel_agrees(-3e38f, 255, 3e38f, kInf) && !novel_agrees(kInf, 255, 1.0f, kInf) && novel_agrees(1.0f, 1, 1.0f, 0.0f));
    CHECK(novel_weight(3, 3.0f) == 1.0f && novel_weight(2, 3.0f) == 0.5f && novel_weight(4, 2.5f) == 1.0f / 2.5f);
    CHECK(novel_lerp(0.0f, 0.3f, 0.9f) == 0.3f && novel_lerp(0.5f, 0.25f, 0.75f) == 0.5f);
}

// One row by brute force, with nothing of the walk: the views sorted by (distance, s), the z-buffer by warp_ahead over all
// pairs, the fill column by column.
static void row_brute(const std::vector<float>& depth, const std::vector<uint8_t>& valid, int S, int V, int U, int v, float t, int exclude,
                      int radius, int nearer, int max_gap, int sources, float tol, float slope, const NovelVolume& vol,
                      std::vector<uint8_t>& fill, std::vector<float>& dout, std::vector<int32_t>& nsrc, std::vector<float>& colour,
                      std::vector<float>& err, double* row_err, int32_t* row_cov)
{
    const int C = vol.C;
    std::vector<unsigned long long> e((size_t)U, 0ull), f;
    for (int x = 0; x < U; x++) {
        int bs = -1, bu = -1;
        for (int s = 0; s < S; s++)
            for (int u = 0; u < U; u++) {
                const size_t q = ((size_t)s * V + v) * U + u;
                int c = -1;
                if (!warp_candidate(depth[q], valid[q], s, u, U, t, exclude, radius, slope, &c) || c != x)
                    continue;
                const size_t b = bs < 0 ? 0 : ((size_t)bs * V + v) * U + bu;
                if (bs < 0 || warp_ahead(warp_z(depth[q], nearer), warp_distance(s, t), s, warp_z(depth[b], nearer), warp_distance(bs, t), bs))
                    bs = s, bu = u;
            }
        if (bs >= 0)
            e[(size_t)x] = novel_entry(kNovelHit, warp_float_bits(depth[((size_t)bs * V + v) * U + bu]));
    }
    fill_brute(e, f, max_gap, nearer);
    std::vector<int> order;
    for (int s = 0; s < S; s++)
        if (s != exclude && warp_in_window(s, t, radius))
            order.push_back(s);
    std::stable_sort(order.begin(), order.end(), [t](int a, int b) { return warp_distance(a, t) < warp_distance(b, t); });
    *row_err = 0.0, *row_cov = 0;
    for (int x = 0; x < U; x++) {
        fill[(size_t)x] = (uint8_t)novel_entry_code(f[(size_t)x]);
        const float d = dout[(size_t)x] = fill[(size_t)x] ? novel_entry_depth(f[(size_t)x]) : 0.0f;
        nsrc[(size_t)x] = 0, err[(size_t)x] = 0.0f;
        std::vector<float> acc((size_t)C, 0.0f), first((size_t)C, 0.0f);
        float wsum = 0.0f;
        bool seen = false;
        for (size_t i = 0; fill[(size_t)x] && i < order.size() && nsrc[(size_t)x] < sources; i++) {
            const int s = order[i];
            float off = d * ((float)s - t);
            off = off * slope;
            if (!(fabsf(off) < 1e9f))
                continue;
            const float p = (float)x - off;
            const long ur = lroundf(p);
            if (ur < 0 || ur >= U)
                continue;
            const size_t q = ((size_t)s * V + v) * U + (size_t)ur;
            const bool agrees = valid[q] != 0 && std::isfinite(depth[q]) && fabsf(depth[q] - d) <= tol;
            const long i0 = std::min<long>(std::max<long>((long)floorf(p), 0), U - 1), i1 = std::min<long>(std::max<long>((long)ceilf(p), 0), U - 1);
            const float w = p - floorf(p), g = 1.0f / (1.0f + fabsf((float)s - t));
            for (int c = 0; c < C; c++) {
                const float a = (1.0f - w) * vol.row(v, s)[i0 * C + c], b = w * vol.row(v, s)[i1 * C + c];
                const float sample = a + b;
                if (!seen)
                    first[(size_t)c] = sample;
                if (agrees) {
                    const float gs = g * sample;
                    acc[(size_t)c] = acc[(size_t)c] + gs;
                }
            }
            seen = true;
            if (agrees) {
                wsum = wsum + g;
                nsrc[(size_t)x]++;
            }
        }
        for (int c = 0; c < C; c++)
            colour[(size_t)x * C + c] = nsrc[(size_t)x] > 0 ? acc[(size_t)c] / wsum : first[(size_t)c];
        if (seen) {
            float a = 0.0f;
            for (int c = 0; c < C; c++)
                a = a + fabsf(colour[(size_t)x * C + c] - vol.row(v, (int)t)[(size_t)x * C + c]);
            err[(size_t)x] = a / (float)C;
        }
        if (nsrc[(size_t)x] > 0) {
            *row_err += (double)err[(size_t)x];
            ++*row_cov;
        }
    }
}

static void rows()
{
    uint32_t seed = 99;
    const float wild[6] = {kNan, kInf, -kInf, 1e30f, -1e30f, -0.0f};
    int filled = 0, blended = 0, unverified = 0;
    for (int round = 0; round < 24; round++) {
        const int S = 1 + (int)(lcg(&seed) >> 8) % 6, V = 2, U = 1 + (int)(lcg(&seed) >> 8) % 40, C = round % 3 + 1, v = round % 2;
        std::vector<float> depth((size_t)S * V * U), vol((size_t)V * S * (U + 3) * C);
        std::vector<uint8_t> valid((size_t)S * V * U);
        for (size_t i = 0; i < depth.size(); i++) {
            const float r = unit(&seed);
            depth[i] = r < 0.5f ? 0.5f : r < 0.8f ? 2.0f : r < 0.95f ? 4.0f * unit(&seed) - 1.0f : wild[(lcg(&seed) >> 8) % 6];
            valid[i] = unit(&seed) < 0.35f ? 0 : 255;
        }
        for (float& x : vol)
            x = unit(&seed);
        const NovelVolume nv = {vol.data(), (long long)S * (U + 3) * C, (long long)(U + 3) * C, C};
        const float slopes[4] = {1.0f, -0.5f, 1e30f, 0.75f};
        const float slope = slopes[round % 4], tol = round % 5 == 0 ? kInf : 0.1f;
        const int exclude = round % 3 == 0 ? -1 : (int)(lcg(&seed) >> 8) % S, radius = round % 4 == 1 ? 2 : 0, nearer = round % 2 ? 1 : -1;
        const int max_gap = round % 3 == 2 ? 2 : 0, sources = 1 + round % 3;
        const float t = (float)((int)(lcg(&seed) >> 8) % S);
        std::vector<uint8_t> f1((size_t)U), f2((size_t)U);
        std::vector<float> d1((size_t)U), d2((size_t)U), c1((size_t)U * C), c2((size_t)U * C), e1((size_t)U), e2((size_t)U);
        std::vector<int32_t> n1((size_t)U), n2((size_t)U);
        double r1, r2;
        int32_t k1, k2;
        novel_row(depth.data(), valid.data(), S, V, U, v, t, exclude, radius, nearer, max_gap, sources, tol, slope, nv, true, f1.data(), d1.data(),
                  n1.data(), c1.data(), e1.data(), &r1, &k1);
        row_brute(depth, valid, S, V, U, v, t, exclude, radius, nearer, max_gap, sources, tol, slope, nv, f2, d2, n2, c2, e2, &r2, &k2);
        CHECK(f1 == f2 && n1 == n2 && k1 == k2);
        CHECK(memcmp(d1.data(), d2.data(), d1.size() * 4) == 0 && memcmp(c1.data(), c2.data(), c1.size() * 4) == 0);
        CHECK(memcmp(e1.data(), e2.data(), e1.size() * 4) == 0 && r1 == r2);
        for (int x = 0; x < U; x++) {
            filled += f1[(size_t)x] >= 2;
            blended += n1[(size_t)x] >= 2;
            unverified += f1[(size_t)x] != 0 && n1[(size_t)x] == 0;
            CHECK(std::isfinite(d1[(size_t)x]));   // (1e30 does arrive: from the target's own view, at distance 0)
        }
        // without a volume: the same fill, depth and n_src
        const NovelVolume none = {nullptr, 0, 0, 0};
        novel_row(depth.data(), valid.data(), S, V, U, v, t + 0.5f, exclude, radius, nearer, max_gap, sources, tol, slope, none, false, f1.data(),
                  d1.data(), n1.data(), nullptr, nullptr, &r1, &k1);
        CHECK(r1 == 0.0);
    }
    CHECK(filled > 20 && blended > 20 && unverified > 5);   // the rows are working ones
}

int main()
{
    arguments();
    lds_cap_and_grid();
    fill_scan();
    taps();
    rows();
    printf("novel plan tests ok\n");
    return 0;
}
