// tap_entry (remotesensingproject_amd/csrc/k2_taps.hpp) on the host: whenever it says `fast`, its {t, floor - u, 1 - t} are
// the per-lane arithmetic of scan_reg_body in EVERY pixel of the tile, and every sample lies inside the row.  Built by
// tests/test_taps_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "k2_taps.hpp"

using rslf::TapEntry;
using rslf::tap_entry;

static long long g_cases = 0, g_fast = 0, g_failures = 0;

static uint32_t bits(float x) { return rslf::tap_float_bits(x); }

// One (offset, tile, row width): compare the entry with what each lane computes for itself.  Returns `fast`.
static bool check(float off, int u_first, int width, int U, const char* family)
{
    const int C = 1, row = 1000;
    const int u_last = u_first + width - 1;
    if (u_first < 0 || width < 1 || width > 64 || u_last > U - 1)
        return false;
    const TapEntry e = tap_entry(off, u_first, u_last, U, C, row);
    g_cases++;
    if (!e.fast)
        return false;
    g_fast++;
    const int rel = e.byteoff / 4 - row - u_first;   // floor(x) - u of the first lane
    for (int u = u_first; u <= u_last; u++) {
        // scan_reg_body, line for line
        const float uf = (float)u;
        const float x = off + uf;                    // core.hpp:552
        const float fl = floorf(x);
        const float t = x - fl;                      // = v_fract_f32 for x > 0
        const int i0 = (int)fl;                      // = v_cvt_flr_i32_f32
        const float omt = 1.0f - t;
        const bool inside = bits(x) <= bits((float)(U - 1));   // the BORDER form's validity test
        if (bits(t) != bits(e.t) || bits(omt) != bits(e.omt) || i0 - u != rel || !inside || i0 < 0 || i0 + 1 > U) {
            if (g_failures++ < 20)
                printf("FAIL %s: off=%.9g (0x%08x) tile [%d, %d] U=%d lane u=%d: t %.9g / %.9g, floor-u %d / %d, 1-t %.9g / %.9g, inside %d\n",
                       family, off, bits(off), u_first, u_last, U, u, t, e.t, i0 - u, rel, omt, e.omt, (int)inside);
            return true;
        }
    }
    return true;
}

struct Family {
    const char* name;
    long long cases, fast;
};
static std::vector<Family> g_families;
static void close_family(const char* name)
{
    long long c = g_cases, f = g_fast;
    for (const Family& x : g_families)
        c -= x.cases, f -= x.fast;
    g_families.push_back({name, c, f});
}

// ---- the fast-batch share of a whole frame, from tap_entry and the row kernel's interior rule --------------------------
// scan_reg_rows: a hypothesis is interior for a tile when every lane keeps reach = max|s_hat - s| * |D| * |slope| + 2
// pixels to both row ends.  Batches of eight samples; two ways of counting the batch that reaches past S:
//   whole_only = false: it counts when its samples are all fast (its padding slots would stay sentinels) -- the share
//                       the table could serve at most, and the figure the round's model was made with;
//   whole_only = true:  it never counts -- what scan_reg_body does (the batch with padding slots takes the per-lane form).
// Shares are of ALL batches, ceil(S / 8) per (tile, hypothesis), in the interior form and in the border form.
static void shares(int U, int S, int D, float dmin, float dmax, float slope, bool whole_only, double* interior_share, double* border_share)
{
    const int s_hat = S / 2, batch = 8;
    const float range = dmax - dmin, denom = (float)(D - 1);
    const float max_ds = (float)std::max(s_hat, S - 1 - s_hat), Um1 = (float)(U - 1);
    long long total = 0, fast_in = 0, fast_border = 0;
    for (int d = 0; d < D; d++) {
        const float num = (float)d * range;          // k2_scan.hpp, hypothesis()
        const float quo = num / denom;
        const float Dd = dmin + quo;
        const float r0 = max_ds * fabsf(Dd);
        const float r1 = r0 * fabsf(slope);
        const float reach = r1 + 2.0f;
        for (int u0 = 0; u0 < U; u0 += 64) {
            const int u1 = std::min(u0 + 63, U - 1);
            const bool interior = (float)u0 - reach >= 0.0f && (float)u1 + reach <= Um1;
            for (int s0 = 0; s0 < S; s0 += batch) {
                bool all = !(whole_only && s0 + batch > S);
                for (int s = s0; s < std::min(s0 + batch, S); s++) {
                    float off = (float)(s_hat - s) * Dd;   // core.hpp:542,550
                    off = off * slope;                     // core.hpp:551
                    all = all && tap_entry(off, u0, u1, U, 1, 0).fast;
                }
                total++;
                fast_in += all && interior;
                fast_border += all && !interior;
            }
        }
    }
    *interior_share = (double)fast_in / (double)total;
    *border_share = (double)fast_border / (double)total;
}

int main()
{
    std::mt19937 rng(20261018);
    auto uni = [&](int lo, int hi) { return (int)(lo + (int)(rng() % (unsigned)(hi - lo + 1))); };
    auto unif = [&](double lo, double hi) { return (float)(lo + (hi - lo) * ((double)rng() / 4294967296.0)); };

    // random offsets in +-600, any tile of a 4096-pixel row
    for (int i = 0; i < 200000; i++)
        check(unif(-600.0, 600.0), uni(0, 4096 - 64), 64, 4096, "random");
    close_family("random");

    // odd multiples of half a quantum for every binade 2..2048: x = off + u sits on a tie in the binade [2^b, 2^(b+1))
    for (int b = 1; b <= 11; b++) {
        const float q = ldexpf(1.0f, b - 23);   // quantum of [2^b, 2^(b+1))
        for (int i = 0; i < 400; i++) {
            const int u0 = std::max(0, (1 << b) - 64 + uni(0, 70));
            const float frac = (float)(2 * uni(0, 1 << 20) + 1) * (0.5f * q);   // odd multiple of q / 2
            for (int whole = -3; whole <= 40; whole += 7)
                check((float)whole + frac, u0, 64, 8192, "half-quantum ties");
            check(-(float)uni(0, 60) + frac, u0, 64, 8192, "half-quantum ties");
        }
    }
    close_family("half-quantum ties");

    // tiles starting at 2^b - 64 .. 2^b + 1: the tile crosses, touches or just clears the binade edge
    for (int b = 1; b <= 11; b++)
        for (int du = -64; du <= 1; du++) {
            const int u0 = (1 << b) + du;
            if (u0 < 0)
                continue;
            for (int i = 0; i < 24; i++) {
                check(unif(-40.0, 40.0), u0, 64, 8192, "binade edges");
                check((float)uni(-1280, 1280) / 32.0f, u0, 64, 8192, "binade edges");
            }
        }
    close_family("binade edges");

    // dyadic grids: multiples of 1/32 (the c3 grid), 1/64 and 1/4
    for (int i = 0; i < 100000; i++) {
        const float den = i % 3 == 0 ? 32.0f : i % 3 == 1 ? 64.0f : 4.0f;
        check((float)uni(-600 * 32, 600 * 32) / den, uni(0, 4096 - 64), 64, 4096, "dyadic");
    }
    close_family("dyadic");

    // offsets that round a lane up to exactly 2^b: off + u = 2^b - eps for some lane of the tile
    for (int b = 1; b <= 11; b++)
        for (int i = 0; i < 600; i++) {
            const int u0 = std::max(0, (1 << b) - uni(1, 200));
            const int lane = uni(0, 63);
            const float target = (float)(1 << b) - ldexpf((float)uni(1, 3), b - 25);   // within half a quantum below 2^b
            check(target - (float)(u0 + lane), u0, 64, 8192, "round up to 2^b");
            check(nextafterf(target - (float)(u0 + lane), 1.0e9f), u0, 64, 8192, "round up to 2^b");
        }
    close_family("round up to 2^b");

    // ragged tiles: 1..63 pixels, anywhere
    for (int i = 0; i < 100000; i++) {
        const int w = uni(1, 63);
        const float off = i & 1 ? unif(-600.0, 600.0) : (float)uni(-600 * 32, 600 * 32) / 32.0f;
        check(off, uni(0, 4096 - w), w, 4096, "ragged");
    }
    close_family("ragged");

    // x_last equal to U - 1 (inside) and one ulp above it (outside: never fast)
    for (int i = 0; i < 20000; i++) {
        const int U = uni(130, 5000), w = uni(1, 64), u_last = uni(w - 1 + 64, U - 1), u0 = u_last - w + 1;
        const float off = (float)(U - 1) - (float)u_last;   // an integer: x_last == U - 1 exactly
        if (!check(off, u0, w, U, "row end") && (float)u0 + off > 0.0f) {
            if (g_failures++ < 20)
                printf("FAIL row end: off=%g tile [%d, %d] U=%d: x_last == U - 1 with an exact sum must be fast\n", off, u0, u_last, U);
        }
        const float above = nextafterf((float)(U - 1), 1.0e9f) - (float)u_last;
        if ((above + (float)u_last) > (float)(U - 1) && tap_entry(above, u0, u_last, U, 1, 0).fast) {
            if (g_failures++ < 20)
                printf("FAIL row end: off=%.9g tile [%d, %d] U=%d: x_last above U - 1 is fast\n", above, u0, u_last, U);
        }
        // and the row's start: x_first <= 0 is never fast
        if (tap_entry(-(float)u0, u0, u_last, U, 1, 0).fast) {
            if (g_failures++ < 20)
                printf("FAIL row start: tile [%d, %d]: x_first == 0 is fast\n", u0, u_last);
        }
    }
    close_family("row end");

    for (const Family& f : g_families) {
        printf("%-20s %8lld cases, %8lld fast\n", f.name, f.cases, f.fast);
        if (f.fast * 20 < f.cases) {   // every family must exercise the comparison, not only the refusal
            printf("FAIL %s: under 5 %% of the cases are fast\n", f.name);
            g_failures++;
        }
    }

    // fast-batch shares of whole frames.  The first two are asserted here, both ways of counting; every line is printed
    // for tests/test_taps_cpu.py, which holds the kernel's shares to the numpy restatement the GPU tests use.
    struct Frame {
        const char* name;
        int U, S, D;
        float dmin, dmax, slope;
        double most, kernel;   // expected interior-form shares (+- 0.005), < 0: printed only
    };
    const Frame frames[] = {
        {"c3", 1920, 101, 256, -2.0f, 5.96875f, 1.0f, 0.833, 0.769},
        {"skysat_lr", 960, 100, 120, -1.0f, 4.0f, 1.0f, 0.546, 0.504},
        {"c2", 512, 33, 128, -1.0f, 2.96875f, 1.0f, -1.0, -1.0},
        {"test_nondyadic", 320, 101, 16, -0.37f, 1.13f, 1.0f, -1.0, -1.0},
        {"test_nondyadic_07", 320, 101, 16, -0.37f, 1.13f, 0.7f, -1.0, -1.0},
        {"test_dyadic", 320, 101, 16, -0.5f, 1.375f, 1.0f, -1.0, -1.0},
        {"test_short_tile", 200, 101, 16, -0.5f, 1.375f, 1.0f, -1.0, -1.0},
    };
    for (const Frame& f : frames) {
        double most = 0.0, most_b = 0.0, kern = 0.0, kern_b = 0.0;
        shares(f.U, f.S, f.D, f.dmin, f.dmax, f.slope, false, &most, &most_b);
        shares(f.U, f.S, f.D, f.dmin, f.dmax, f.slope, true, &kern, &kern_b);
        printf("share %s U %d S %d D %d dmin %.9g dmax %.9g slope %.9g : padded %.6f %.6f kernel %.6f %.6f\n", f.name, f.U, f.S, f.D,
               f.dmin, f.dmax, f.slope, most, most_b, kern, kern_b);
        if (f.most >= 0.0 && (fabs(most - f.most) > 0.005 || fabs(kern - f.kernel) > 0.005)) {
            printf("FAIL %s: interior-form fast share %.4f (padded batch counted) / %.4f (whole batches, the kernel), expected %.3f / %.3f +- 0.005\n",
                   f.name, most, kern, f.most, f.kernel);
            g_failures++;
        }
    }

    if (g_failures) {
        printf("%lld failures\n", g_failures);
        return 1;
    }
    printf("tap tests ok: %lld cases, %lld fast\n", g_cases, g_fast);
    return 0;
}
