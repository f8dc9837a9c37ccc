// row_exact_entry (remotesensingproject_amd/csrc/k2_taps.hpp) on the host: whenever it says `exact`, its {tap offset, t, 1 - t}
// are the per-lane arithmetic of scan_reg_body in EVERY pixel 0 <= u < U whose sample lies inside the row -- and so, wherever
// some pixel's per-lane values differ from the entry, the flag is false.  Whole hypothesis grids, every (d, s), every pixel.
// Built by tests/test_row_exact_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "k2_taps.hpp"

using rslf::row_exact_entry;
using rslf::RowExactEntry;

static long long g_failures = 0, g_entries = 0, g_exact = 0, g_pixels = 0;

static uint32_t bits(float x) { return rslf::tap_float_bits(x); }

// Does the entry reproduce every in-row pixel's per-lane values?  (scan_reg_body, line for line)
static bool reproduces(const RowExactEntry& e, float off, int U, int C, int row, int* first_bad)
{
    const uint32_t um1 = bits((float)(U - 1));
    for (int u = 0; u < U; u++) {
        const float uf = (float)u;
        const float x = off + uf;                    // core.hpp:552
        if (!(bits(x) <= um1))                       // the BORDER form's validity test: outside the row
            continue;
        g_pixels++;
        const float fl = floorf(x);
        const float t = x - fl;                      // = v_fract_f32 for x >= 0
        const int i0 = (int)fl;                      // = v_cvt_flr_i32_f32
        const float omt = 1.0f - t;
        const long long byteoff = ((long long)i0 * C + row) * 4;   // of this pixel's left tap
        if (bits(t) != bits(e.t) || bits(omt) != bits(e.omt) || byteoff != (long long)e.byteoff + (long long)u * C * 4) {
            *first_bad = u;
            return false;
        }
    }
    return true;
}

struct Grid {
    const char* name;
    int U, S, D;
    float dmin, dmax, slope;
    int s_hat;          // -1: the centre view
    int want_exact;     // row-exact hypotheses expected, -1: printed only
};

// Returns the number of row-exact hypotheses (every view offset s < S exact).
static int run_grid(const Grid& g, bool print_which)
{
    const int C = 1, pitch = g.U + 3;
    const int s_hat = g.s_hat < 0 ? g.S / 2 : g.s_hat;
    const float range = g.dmax - g.dmin, denom = (float)(g.D - 1);
    int exact_hyps = 0;
    long long exact_entries = 0, with_int = 0, neg = 0, pos = 0;
    for (int d = 0; d < g.D; d++) {
        const float num = (float)d * range;          // k2_scan.hpp, hypothesis()
        const float quo = num / denom;
        const float Dd = g.dmin + quo;
        bool all = true;
        for (int s = 0; s < g.S; s++) {
            float off = (float)(s_hat - s) * Dd;     // core.hpp:542,550
            off = off * g.slope;                     // core.hpp:551
            const RowExactEntry e = row_exact_entry(off, g.U, C, s * pitch);
            int bad = -1;
            const bool same = reproduces(e, off, g.U, C, s * pitch, &bad);
            g_entries++;
            if (e.exact && !same) {
                if (g_failures++ < 20)
                    printf("FAIL %s: d=%d s=%d off=%.9g (0x%08x) U=%d is flagged exact, pixel u=%d differs\n", g.name, d, s, off, bits(off),
                           g.U, bad);
            }
            if (e.exact) {
                exact_entries++;
                g_exact++;
                with_int += e.t == 0.0f;
                neg += off < 0.0f;
                pos += off > 0.0f;
            }
            all = all && e.exact;
        }
        exact_hyps += all;
        if (all && print_which)
            printf("exact-hypothesis %s d %d D %.9g\n", g.name, d, Dd);
    }
    printf("grid %s U %d S %d D %d dmin %.9g dmax %.9g slope %.9g s_hat %d : exact hypotheses %d of %d, exact entries %lld (t == 0: %lld, off < 0: %lld, off > 0: %lld)\n",
           g.name, g.U, g.S, g.D, g.dmin, g.dmax, g.slope, s_hat, exact_hyps, g.D, exact_entries, with_int, neg, pos);
    if (g.want_exact >= 0 && exact_hyps != g.want_exact) {
        printf("FAIL %s: %d row-exact hypotheses, expected %d\n", g.name, exact_hyps, g.want_exact);
        g_failures++;
    }
    return exact_hyps;
}

int main()
{
    const float s14 = ldexpf(1.0f, -14), s16 = ldexpf(1.0f, -16);
    const Grid fixed[] = {
        // the bench configurations at their own U and S, and the shares the design rests on
        {"c3", 1920, 101, 256, -2.0f, 5.96875f, 1.0f, -1, 256},
        {"c2", 512, 33, 128, -1.0f, 2.96875f, 1.0f, -1, 128},
        {"c1", 540, 9, 64, -2.0f, 5.875f, 1.0f, -1, 64},
        {"skysat_lr", 960, 100, 120, -1.0f, 4.0f, 1.0f, -1, 2},
        {"minus1_1_D7", 320, 101, 7, -1.0f, 1.0f, 1.0f, -1, 3},
        // the GPU test's grids (tests/test_gpu_scalar_taps.py)
        {"gpu_D17", 320, 101, 17, -0.5f, 0.5f, 1.0f, -1, 17},
        {"gpu_D18", 320, 101, 18, -0.5f, 0.5f, 1.0f, -1, 2},
        {"gpu_U330", 330, 101, 17, -0.5f, 0.5f, 1.0f, -1, 17},
        {"gpu_D17_slope_half", 320, 101, 17, -0.5f, 0.5f, 0.5f, -1, 17},
        {"gpu_D17_s_hat_30", 320, 101, 17, -0.5f, 0.5f, 1.0f, 30, 17},
        {"gpu_D17_S99", 320, 99, 17, -0.5f, 0.5f, 1.0f, -1, 17},
        {"gpu_D7_s_hat_30", 320, 101, 7, -1.0f, 1.0f, 1.0f, 30, 3},
        {"gpu_D7_S99", 320, 99, 7, -1.0f, 1.0f, 1.0f, -1, 3},
        // slopes and an off-centre s_hat on dyadic and non-dyadic grids
        {"c3_slope_half", 1920, 101, 256, -2.0f, 5.96875f, 0.5f, -1, 256},
        {"c3_slope_03", 1920, 101, 256, -2.0f, 5.96875f, 0.3f, -1, -1},
        {"c3_s_hat_30", 1920, 101, 256, -2.0f, 5.96875f, 1.0f, 30, 256},
        {"skysat_slope_half", 960, 100, 120, -1.0f, 4.0f, 0.5f, -1, -1},
        {"skysat_s_hat_7", 960, 100, 120, -1.0f, 4.0f, 1.0f, 7, -1},
        {"D7_slope_03", 320, 101, 7, -1.0f, 1.0f, 0.3f, 30, -1},
        // integers only: every t is 0
        {"integers", 640, 33, 9, -4.0f, 4.0f, 1.0f, -1, 9},
    };
    for (const Grid& g : fixed)
        run_grid(g, g.D <= 7);

    // steps 2^-14 and 2^-16 around -1 .. : exactness is lost as the row grows
    const int widths[] = {256, 320, 2048, 4096};
    int prev14 = 1 << 30, prev16 = 1 << 30;
    for (int U : widths) {
        char n14[32], n16[32];
        snprintf(n14, sizeof n14, "step_2^-14_U%d", U);
        snprintf(n16, sizeof n16, "step_2^-16_U%d", U);
        const Grid g14 = {n14, U, 101, 33, -1.0f, -1.0f + 32.0f * s14, 1.0f, -1, -1};
        const Grid g16 = {n16, U, 101, 33, -1.0f, -1.0f + 32.0f * s16, 1.0f, 40, -1};
        const int e14 = run_grid(g14, false), e16 = run_grid(g16, false);
        if (e14 > prev14 || e16 > prev16 || e16 > e14) {
            printf("FAIL: exact hypotheses must not grow with U or with a finer step (%d, %d at U=%d)\n", e14, e16, U);
            g_failures++;
        }
        prev14 = e14, prev16 = e16;
    }
    if (prev14 >= 33) {
        printf("FAIL: step 2^-14 at U=4096 cannot be exact in every hypothesis\n");
        g_failures++;
    }

    // -1..1, D = 7: exactly the hypotheses with D_d in {-1, 0, 1} (d = 0, 3, 6), read back from the printed lines by the
    // Python side too
    if (g_exact * 20 < g_entries) {   // the comparison must be exercised, not only the refusal
        printf("FAIL: under 5 %% of the entries are exact\n");
        g_failures++;
    }
    if (g_failures) {
        printf("%lld failures\n", g_failures);
        return 1;
    }
    printf("row-exact tests ok: %lld entries, %lld exact, %lld pixel comparisons\n", g_entries, g_exact, g_pixels);
    return 0;
}
