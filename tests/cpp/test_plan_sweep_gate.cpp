// Host test of the sweep gate's pure decisions (rslf_plan_sweep_gate.hpp) and of the one predicate K4 and K11 share
// (k11_f2c_peak_rule.hpp).  Stand-alone: built by tests/test_sweep_gate_cpu.py with g++ -fsanitize=address,undefined
// -ffp-contract=off.  No HIP.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "rslf_plan_sweep_gate.hpp"

using namespace rslf;
using namespace rslf::plan;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

static void ratios()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    CHECK(sweep_gate_ratio_ok(0.0f) && !sweep_gate_on(0.0f));
    CHECK(sweep_gate_ratio_ok(-0.0f) && !sweep_gate_on(-0.0f));
    CHECK(sweep_gate_ratio_ok(1.0f) && sweep_gate_on(1.0f));
    CHECK(sweep_gate_ratio_ok(0.7f) && sweep_gate_on(0.7f));
    CHECK(sweep_gate_ratio_ok(std::numeric_limits<float>::denorm_min()) && sweep_gate_on(std::numeric_limits<float>::denorm_min()));
    CHECK(!sweep_gate_ratio_ok(nextafterf(1.0f, 2.0f)) && !sweep_gate_on(nextafterf(1.0f, 2.0f)));
    CHECK(!sweep_gate_ratio_ok(-0.1f) && !sweep_gate_on(-0.1f));
    CHECK(!sweep_gate_ratio_ok(nan) && !sweep_gate_on(nan));
    CHECK(!sweep_gate_ratio_ok(inf) && !sweep_gate_ratio_ok(-inf));
    CHECK(sweep_gate_counter_bytes(0.0f) == 0 && sweep_gate_counter_bytes(0.5f) == 8 && sweep_gate_counter_bytes(1.0f) == 8);
    CHECK(sweep_gate_counter_bytes(nan) == 0 && sweep_gate_counter_bytes(2.0f) == 0);
}

static void planes_and_window()
{
    for (int m = 0; m < 16; m++)
        CHECK(sweep_gate_planes_ok(m & 1, m & 2, m & 4, m & 8) == (m == 15));
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // the order of the refusals: the ratio first, then the window, then the mode, then the planes
    CHECK(sweep_gate_args(nan, false, true, false, false, false, false, false, false) == kSweepGateBadRatio);
    CHECK(sweep_gate_args(1.5f, true, false, true, true, true, true, true, true) == kSweepGateBadRatio);
    CHECK(sweep_gate_args(-1.0f, true, false, true, true, true, true, true, true) == kSweepGateBadRatio);
    CHECK(sweep_gate_args(0.7f, false, false, true, true, true, true, true, true) == kSweepGateWindow);   // no sweep open
    CHECK(sweep_gate_args(0.7f, true, true, true, true, true, true, true, true) == kSweepGateWindow);     // a visit has scanned
    CHECK(sweep_gate_args(0.7f, true, false, false, true, true, true, true, true) == kSweepGateWindow);   // past the first visit
    CHECK(sweep_gate_args(0.0f, false, false, true, false, false, false, false, false) == kSweepGateWindow);
    CHECK(sweep_gate_args(0.7f, true, false, true, false, true, true, true, true) == kSweepGateNoPeaks);
    for (int m = 0; m < 15; m++)
        CHECK(sweep_gate_args(0.7f, true, false, true, true, m & 1, m & 2, m & 4, m & 8) == kSweepGateNullPlane);
    CHECK(sweep_gate_args(0.7f, true, false, true, true, true, true, true, true) == kSweepGateOk);
    CHECK(sweep_gate_args(1.0f, true, false, true, true, true, true, true, true) == kSweepGateOk);
    // 0 inside the window switches the gate off whatever the peaks mode
    CHECK(sweep_gate_args(0.0f, true, false, true, false, false, false, false, false) == kSweepGateOk);
    CHECK(sweep_gate_args(0.0f, true, false, true, true, true, false, true, true) == kSweepGateOk);
    // the entries: no window to miss
    CHECK(sweep_gate_entry_args(0.0f, false, false, false, false, false) == kSweepGateOk);
    CHECK(sweep_gate_entry_args(0.7f, false, false, false, false, false) == kSweepGateNoPeaks);
    CHECK(sweep_gate_entry_args(0.7f, true, true, true, false, true) == kSweepGateNullPlane);
    CHECK(sweep_gate_entry_args(0.7f, true, true, true, true, true) == kSweepGateOk);
    CHECK(sweep_gate_entry_args(nan, true, true, true, true, true) == kSweepGateBadRatio);
}

static void predicate()
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // the sweep's statement IS the pyramid's
    const int32_t idx[] = {-1, 0, 3}, run[] = {-1, 0, 5};
    const float sc[] = {0.0f, 0.25f, 1.0f, nan}, rs[] = {0.0f, 0.2f, 0.25f, 1.0f, nan}, rr[] = {0.4f, 0.7f, 0.8f, 1.0f};
    for (int32_t i : idx)
        for (int32_t j : run)
            for (float s : sc)
                for (float t : rs)
                    for (float r : rr) {
                        const bool want = i >= 0 && j >= 0 && t > r * s;
                        CHECK(f2c_peak_ambiguous(i, j, s, t, r) == want);
                        CHECK(sweep_source_withheld(true, i, j, s, t, r) == want);
                        CHECK(!sweep_source_withheld(false, i, j, s, t, r));
                    }
    // r = 1 withholds nothing: a runner-up as high as its winner is not above it
    CHECK(!sweep_source_withheld(true, 2, 4, 0.5f, 0.5f, 1.0f));
    CHECK(sweep_source_withheld(true, 2, 4, 0.5f, 0.5f, nextafterf(1.0f, 0.0f)));
    // a NaN on either side compares false
    CHECK(!sweep_source_withheld(true, 2, 4, nan, 0.5f, 0.7f) && !sweep_source_withheld(true, 2, 4, 0.5f, nan, 0.7f));
    // no winner or no runner-up: never ambiguous
    CHECK(!sweep_source_withheld(true, -1, 4, 0.1f, 0.9f, 0.5f) && !sweep_source_withheld(true, 2, -1, 0.1f, 0.9f, 0.5f));
    // one binary32 multiply: 0.7f * 0.3f rounds to a float; a runner-up at exactly that float is not above the bound, its
    // successor is -- a bound kept in double (0.7f * 0.3f exactly) would call the first ambiguous or the second not
    const float bound = 0.7f * 0.3f;
    CHECK(!f2c_peak_ambiguous(0, 1, 0.3f, bound, 0.7f));
    CHECK(f2c_peak_ambiguous(0, 1, 0.3f, nextafterf(bound, 1.0f), 0.7f));
}

// One scanline by hand: the count of a visit is "passes gate 1 and fails gate 2", whatever else the pixel is
static void counting()
{
    struct Px { bool gate1; int32_t idx, runner; float score, runner_score; };
    const std::vector<Px> row = {{true, 3, 5, 1.0f, 0.9f},    // ambiguous at 0.7: withheld
                                 {false, 3, 5, 1.0f, 0.9f},   // ambiguous, but no source anyway: not counted
                                 {true, 3, -1, 1.0f, 0.0f},   // flat band, no runner-up
                                 {true, 3, 5, 1.0f, 0.7f},    // 0.7 > 0.7f * 1 is false
                                 {true, -1, -1, 0.0f, 0.0f},  // never scanned or painted
                                 {true, 2, 6, 0.5f, 0.4f}};   // 0.4 > 0.35
    int n07 = 0, n1 = 0;
    for (const Px& p : row) {
        n07 += sweep_source_withheld(p.gate1, p.idx, p.runner, p.score, p.runner_score, 0.7f);
        n1 += sweep_source_withheld(p.gate1, p.idx, p.runner, p.score, p.runner_score, 1.0f);
    }
    CHECK(n07 == 2 && n1 == 0);
}

int main()
{
    ratios();
    planes_and_window();
    predicate();
    counting();
    printf("sweep gate plan tests ok\n");
    return 0;
}
