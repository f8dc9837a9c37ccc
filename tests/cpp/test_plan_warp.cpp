// Host test of the view warp's pure decisions (rslf_plan_warp.hpp) and of its per-pixel rule (k14_warp_rule.hpp).
// Stand-alone: built by tests/test_view_warp_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off.  No HIP.
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "rslf_plan_warp.hpp"

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

static void arguments()
{
    CHECK(warp_args(3, 2, 5, 1, 1, true, false, false, false, 0, 0, 0) == kWarpOk);
    CHECK(warp_args(3, 2, 5, 4, -1, true, false, true, true, 2, 3, 5) == kWarpOk);
    CHECK(warp_args(0, 2, 5, 1, 1, true, false, false, false, 0, 0, 0) == kWarpBadShape);
    CHECK(warp_args(3, 0, 5, 1, 1, true, false, false, false, 0, 0, 0) == kWarpBadShape);
    CHECK(warp_args(3, 2, -1, 1, 1, true, false, false, false, 0, 0, 0) == kWarpBadShape);
    CHECK(warp_args(3, 2, 5, 0, 1, true, false, false, false, 0, 0, 0) == kWarpBadTargets);
    CHECK(warp_args(3, 2, 5, -3, 1, true, false, false, false, 0, 0, 0) == kWarpBadTargets);
    CHECK(warp_args(3, 2, 5, 1, 0, true, false, false, false, 0, 0, 0) == kWarpBadNearer);
    CHECK(warp_args(3, 2, 5, 1, 1, false, false, false, false, 0, 0, 0) == kWarpNoOutput);
    CHECK(warp_args(3, 2, 5, 1, 1, true, true, false, false, 0, 0, 0) == kWarpAlias);
    CHECK(warp_args(3, 2, 5, 1, 1, true, false, true, false, 0, 0, 0) == kWarpNoVolume);
    CHECK(warp_args(3, 2, 5, 1, 1, true, false, true, true, 2, 3, 6) == kWarpVolumeShape);
    CHECK(warp_args(3, 2, 5, 1, 1, true, false, true, true, 3, 2, 5) == kWarpVolumeShape);   // (V and S swapped)
    CHECK(warp_args(3, 2, 5, 1, 1, true, false, false, true, 9, 9, 9) == kWarpOk);           // a volume nobody reads
    // the order of the refusals
    CHECK(warp_args(0, 2, 5, 0, 0, false, true, true, false, 0, 0, 0) == kWarpBadShape);
    CHECK(warp_args(3, 2, 5, 0, 0, false, true, true, false, 0, 0, 0) == kWarpBadTargets);
    CHECK(warp_args(3, 2, 5, 1, 0, false, true, true, false, 0, 0, 0) == kWarpBadNearer);
    CHECK(warp_args(3, 2, 5, 1, 1, false, true, true, false, 0, 0, 0) == kWarpNoOutput);
    CHECK(warp_args(3, 2, 5, 1, 1, true, true, true, false, 0, 0, 0) == kWarpAlias);

    CHECK(warp_target_arg(0.0f, 5, true) == kWarpTargetOk && warp_target_arg(4.0f, 5, true) == kWarpTargetOk);
    CHECK(warp_target_arg(-0.0f, 5, true) == kWarpTargetOk);
    CHECK(warp_target_arg(5.0f, 5, true) == kWarpTargetNotAView && warp_target_arg(-1.0f, 5, true) == kWarpTargetNotAView);
    CHECK(warp_target_arg(2.5f, 5, true) == kWarpTargetNotAView && warp_target_arg(2.5f, 5, false) == kWarpTargetOk);
    CHECK(warp_target_arg(-1.0f, 5, false) == kWarpTargetOk && warp_target_arg(65536.0f, 5, false) == kWarpTargetOk);
    CHECK(warp_target_arg(-65536.0f, 5, false) == kWarpTargetOk);
    CHECK(warp_target_arg(65536.01f, 5, false) == kWarpTargetRange && warp_target_arg(kNan, 5, false) == kWarpTargetRange);
    CHECK(warp_target_arg(kInf, 5, false) == kWarpTargetRange && warp_target_arg(-kInf, 5, true) == kWarpTargetRange);
    CHECK(warp_target_arg(1e30f, 5, true) == kWarpTargetRange);
}

static void lds_grid_and_bytes()
{
    CHECK(kWarpMaxU >= 8000);   // plan::kEpiLinesMaxU
    CHECK(warp_lds_bytes(1920, false) == 15360 && warp_lds_bytes(1920, true) == 23040);
    CHECK(warp_lds_bytes(kWarpMaxU, true) + 64 <= kWarpLdsBudget);
    CHECK(2 * (warp_lds_bytes(kWarpMaxU, false) + 64) <= kWarpLdsBudget);   // two workgroups a CU at the cap
    CHECK(warp_grid(3, 9) == 8u * 9 && warp_grid(8, 1) == 8u && warp_grid(9, 1) == 16u && warp_grid(1080, 101) == 1080u * 101);
    CHECK(warp_grid(0, 1) == 0 && warp_grid(1, 0) == 0);
    CHECK(warp_grid(INT_MAX / 8 * 8, 1) == (unsigned)(INT_MAX / 8 * 8));
    CHECK(warp_grid(1 << 28, 8) == 0 && warp_grid(1 << 28, 7) == 7u << 28 && warp_grid(INT_MAX, 1) == 0);
    CHECK(warp_limits(101, 1080, 1920, 101) == kWarpFits && warp_limits(2, 1, kWarpMaxU, 1) == kWarpFits);
    CHECK(warp_limits(2, 1, kWarpMaxU + 1, 1) == kWarpTooWide);
    CHECK(warp_limits(kWarpMaxViews, 1, 8, 1) == kWarpFits && warp_limits(kWarpMaxViews + 1, 1, 8, 1) == kWarpTooManyViews);
    CHECK(warp_limits(2, 1 << 28, 8, 8) == kWarpGridLimit);
    CHECK(warp_limits(1 << 20, 1 << 30, 1 << 20, 8) == kWarpTooWide);   // the order: width, views, grid
    CHECK(warp_launches(1) == 1 && warp_launches(kWarpLaunchTargets) == 1 && warp_launches(kWarpLaunchTargets + 1) == 2);
    CHECK(warp_launch_targets(kWarpLaunchTargets + 3, 0) == kWarpLaunchTargets && warp_launch_targets(kWarpLaunchTargets + 3, 1) == 3);
    CHECK(warp_launch_targets(5, 0) == 5);
    CHECK(sizeof(float) * kWarpLaunchTargets + sizeof(int) * kWarpLaunchTargets <= 2048);

    int s0, s1;
    CHECK(warp_window(4.0f, 9, 0, &s0, &s1) && s0 == 0 && s1 == 8);
    CHECK(warp_window(4.0f, 9, 2, &s0, &s1) && s0 == 2 && s1 == 6);
    CHECK(warp_window(4.5f, 9, 2, &s0, &s1) && s0 == 3 && s1 == 6);
    CHECK(warp_window(-1.0f, 9, 2, &s0, &s1) && s0 == 0 && s1 == 1);
    CHECK(warp_window(9.0f, 9, 1, &s0, &s1) && s0 == 8 && s1 == 8);
    CHECK(!warp_window(20.0f, 9, 2, &s0, &s1) && s0 == -1);
    CHECK(warp_window(20.0f, 9, 0, &s0, &s1) && s0 == 0 && s1 == 8);

    WarpPlanes none = {}, all = {true, true, true, true, true, true, true, true};
    CHECK(warp_out_bytes_per_cell(none, 3) == 0 && warp_out_bytes_per_cell(all, 3) == 1 + 5 * 4 + 12);
    CHECK(warp_bytes(9, 3, 300, 9, 1, true, none) == (size_t)9 * 900 * 5);
    CHECK(warp_bytes(9, 3, 300, 9, 1, false, none) == (size_t)9 * 900 * 4);
    CHECK(warp_bytes(9, 3, 300, 2, 3, true, all) == (size_t)9 * 900 * 5 + (size_t)2 * 900 * 24 + (size_t)2 * 900 * 33 + 2 * 3 * 12);
}

// The rank order against a sort by (distance, s); the distance tie at t = c + 0.5 goes to the smaller s.
static void rank_order()
{
    int order[9];
    warp_rank_order(4.0f, 9, order);
    const int want_mid[9] = {4, 3, 5, 2, 6, 1, 7, 0, 8};
    CHECK(!memcmp(order, want_mid, sizeof order));
    warp_rank_order(4.5f, 9, order);
    const int want_half[9] = {4, 5, 3, 6, 2, 7, 1, 8, 0};
    CHECK(!memcmp(order, want_half, sizeof order));
    warp_rank_order(-1.0f, 9, order);
    for (int k = 0; k < 9; k++)
        CHECK(order[k] == k);
    warp_rank_order(9.0f, 9, order);
    for (int k = 0; k < 9; k++)
        CHECK(order[k] == 8 - k);
    warp_rank_order(0.25f, 3, order);
    CHECK(order[0] == 0 && order[1] == 1 && order[2] == 2);
    const float ts[] = {0.0f, -0.0f, 3.75f, 7.5f, 100.0f, -100.0f, 65536.0f, -65536.0f, 12.000001f, 1e-30f, 16.5f, 33.0f, 32.5f};
    for (float t : ts)
        for (int S : {1, 2, 17, 34}) {
            std::vector<int> got((size_t)S), want((size_t)S);
            warp_rank_order(t, S, got.data());
            for (int s = 0; s < S; s++)
                want[(size_t)s] = s;
            std::stable_sort(want.begin(), want.end(), [t](int a, int b) {
                return warp_distance(a, t) != warp_distance(b, t) ? warp_distance(a, t) < warp_distance(b, t) : a < b;
            });
            CHECK(got == want);
        }
    // the largest case the key holds: every rank and view in 16 bits, the walk complete
    std::vector<int> big((size_t)kWarpMaxViews);
    warp_rank_order(65535.5f, kWarpMaxViews, big.data());
    CHECK(big[0] == 65535 && big[1] == 65534 && big[(size_t)kWarpMaxViews - 1] == 0);
    warp_rank_order(-65536.0f, kWarpMaxViews, big.data());
    CHECK(big[0] == 0 && big[(size_t)kWarpMaxViews - 1] == kWarpMaxViews - 1);
    for (int s = 1; s < kWarpMaxViews; s++)   // one side of t: no two views share a distance
        CHECK(warp_distance(s, -65536.0f) > warp_distance(s - 1, -65536.0f));
}

// For an integral t the offset is consistency_offset's, bit for bit.
static void integral_identity()
{
    const float ds[] = {0.0f, -0.0f, 0.5f, -0.5f, 2.0f, 1.37f, -3.3f, 1e30f, -1e30f, kInf, -kInf, 3e38f, 1e-40f, 123456.78f};
    const float slopes[] = {1.0f, 0.5f, -1.0f, 1e30f, 2e-38f, 0.333f};
    for (float d : ds)
        for (float slope : slopes)
            for (int s = 0; s < 20; s += 3)
                for (int t = -3; t < 24; t += 2) {
                    const float a = warp_offset(d, s, (float)t, slope), b = consistency_offset(d, s, t, slope);
                    CHECK(warp_float_bits(a) == warp_float_bits(b));
                }
    const float nan_off = warp_offset(kNan, 3, 1.0f, 1.0f);
    CHECK(nan_off != nan_off);
    CHECK(warp_target_integral(3.0f, 4) && !warp_target_integral(4.0f, 4) && !warp_target_integral(3.5f, 4) && !warp_target_integral(-1.0f, 4));
}

// The key's order is the rule's order, and what went in comes out.
static void key_order()
{
    const float zs[] = {-FLT_MAX, -2.0f, -1e-40f, 0.0f, 1e-40f, 0.5f, 2.0f, FLT_MAX};
    const int n = (int)(sizeof zs / sizeof zs[0]);
    CHECK(warp_key(-FLT_MAX, kWarpMaxViews - 1, 0) != 0ull);   // 0 is "no candidate"
    CHECK(warp_z(-0.0f, 1) == 0.0f && !signbit(warp_z(-0.0f, 1)) && !signbit(warp_z(0.0f, -1)) && warp_z(2.0f, -1) == -2.0f);
    CHECK(warp_key(warp_z(-0.0f, 1), 3, 7) == warp_key(warp_z(0.0f, 1), 3, 7));
    int order[9];
    const float t = 4.5f;
    warp_rank_order(t, 9, order);
    int rank_of[9];
    for (int k = 0; k < 9; k++)
        rank_of[order[k]] = k;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++)
            for (int sa = 0; sa < 9; sa++)
                for (int sb = 0; sb < 9; sb++) {
                    if (i == j && sa == sb)
                        continue;
                    const bool ahead = warp_ahead(zs[i], warp_distance(sa, t), sa, zs[j], warp_distance(sb, t), sb);
                    CHECK(ahead == (warp_key(zs[i], rank_of[sa], sa) > warp_key(zs[j], rank_of[sb], sb)));
                }
    for (int i = 0; i < n; i++) {
        const unsigned long long key = warp_key(zs[i], 65535, 65535);
        CHECK(warp_key_view(key) == 65535 && warp_float_bits(warp_key_z(key)) == warp_float_bits(zs[i]));
        CHECK(warp_key_view(warp_key(zs[i], 0, 12)) == 12);
    }
}

// The rule header against a brute-force loop that knows no keys: every target column's winner and count.
struct Best {
    bool any;
    float z, dist, d;
    int s, u, count;
};

static void rule_against_brute_force()
{
    const int S = 7, V = 2, U = 53;
    uint32_t seed = 12345u;
    std::vector<float> depth((size_t)S * V * U);
    std::vector<uint8_t> valid(depth.size());
    for (size_t i = 0; i < depth.size(); i++) {
        const uint32_t r = lcg(&seed) >> 8;
        depth[i] = (r % 9 == 0) ? 2.0f : (r % 7 == 0) ? -0.0f : (r % 11 == 0) ? 0.0f : (float)(r % 4001) / 1000.0f - 1.5f;
        if (r % 53 == 0)
            depth[i] = kNan;
        if (r % 59 == 0)
            depth[i] = kInf;
        if (r % 61 == 0)
            depth[i] = 1e30f;
        valid[i] = (lcg(&seed) >> 8) % 10 == 0 ? 0 : 255;
    }
    const float ts[] = {3.0f, 0.0f, 3.5f, -1.0f, 7.0f, 2.25f};
    const int excl[] = {3, 0, -1, -1, -1, 2};
    const float slopes[] = {1.0f, -0.5f, 1e30f};
    for (int nearer : {1, -1})
        for (int radius : {0, 2})
            for (float slope : slopes)
                for (int k = 0; k < 6; k++) {
                    const float t = ts[k];
                    std::vector<int> order((size_t)S), rank_of((size_t)S);
                    warp_rank_order(t, S, order.data());
                    for (int r = 0; r < S; r++)
                        rank_of[(size_t)order[(size_t)r]] = r;
                    for (int v = 0; v < V; v++) {
                        std::vector<Best> best((size_t)U, Best{false, 0, 0, 0, 0, 0, 0});
                        std::vector<unsigned long long> keys((size_t)U, 0ull);
                        for (int s = 0; s < S; s++)
                            for (int u = 0; u < U; u++) {
                                const size_t o = ((size_t)s * V + v) * U + u;
                                const float d = depth[o];
                                // the candidate test, spelt out
                                bool cand = valid[o] != 0 && isfinite(d) && s != excl[k] && (radius <= 0 || fabsf((float)s - t) <= (float)radius);
                                float off = d * ((float)s - t);
                                off = off * slope;
                                long long x = -1;
                                if (cand && fabsf(off) < 1e9f)
                                    x = u + (long long)roundf(off);
                                cand = cand && x >= 0 && x < U;
                                int xr = -7;
                                CHECK(warp_candidate(d, valid[o], s, u, U, t, excl[k], radius, slope, &xr) == cand);
                                CHECK(cand ? xr == (int)x : xr == -7);
                                if (!cand)
                                    continue;
                                const float z = warp_z(d, nearer), dist = fabsf((float)s - t);
                                Best& b = best[(size_t)x];
                                b.count++;
                                if (!b.any || warp_ahead(z, dist, s, b.z, b.dist, b.s))
                                    b = Best{true, z, dist, d, s, u, b.count};
                                const unsigned long long key = warp_key(z, rank_of[(size_t)s], s);
                                keys[(size_t)x] = key > keys[(size_t)x] ? key : keys[(size_t)x];
                            }
                        for (int x = 0; x < U; x++) {
                            const Best& b = best[(size_t)x];
                            CHECK(b.any == (keys[(size_t)x] != 0ull));
                            if (!b.any)
                                continue;
                            CHECK(warp_key_view(keys[(size_t)x]) == b.s);
                            CHECK(warp_source_column(keys[(size_t)x], x, U, t, nearer, slope) == b.u);
                            CHECK(warp_key_z(keys[(size_t)x]) == b.z);
                        }
                    }
                }
    // a key that no candidate made still gives a column inside the row
    CHECK(warp_source_column(warp_key(FLT_MAX, 0, 5), 3, U, 0.0f, 1, 1e30f) >= 0);
    CHECK(warp_source_column(~0ull, 3, U, 0.0f, 1, 1.0f) < U && warp_source_column(~0ull, 3, U, 0.0f, 1, 1.0f) >= 0);
    const float col[3] = {0.5f, 0.25f, 1.0f}, L[3] = {0.25f, 0.5f, 0.0f};
    CHECK(warp_residual(col, L, 3) == ((0.0f + 0.25f) + 0.25f + 1.0f) / 3.0f && warp_residual(col, L, 1) == 0.25f);
}

int main()
{
    arguments();
    lds_grid_and_bytes();
    rank_order();
    integral_identity();
    key_order();
    rule_against_brute_force();
    printf("warp plan tests ok\n");
    return 0;
}
