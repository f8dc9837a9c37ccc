// Host test of the pure decisions of a kept fine-to-coarse run's validity by cross-view consistency
// (rslf_plan_f2c_consistency.hpp) and of the gate itself (consistency_gate, k12_consistency_rule.hpp).  Stand-alone: built by
// tests/test_f2c_consistency_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off and run directly.  No HIP.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "rslf_plan_f2c_consistency.hpp"
#include "rslf_plan_f2c_peaks.hpp"

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

// every (seen, agree, min_agree) up to 20 against the rule as the issue words it
static void the_gate()
{
    for (int seen = 0; seen <= 20; seen++)
        for (int agree = 0; agree <= 20; agree++)
            for (int m = 0; m <= 20; m++) {
                bool want;
                if (seen < m)
                    want = agree >= seen;   // fewer than m views can see it: all of them must agree
                else
                    want = agree >= m;      // at least m of the views that can see it agree
                CHECK(consistency_gate(seen, agree, m) == want);
                if (seen == 0)
                    CHECK(consistency_gate(seen, agree, m));   // nobody can see it: kept
                if (agree >= m)
                    CHECK(consistency_gate(seen, agree, m));   // never stricter than agree >= min_agree
                if (agree <= seen && seen >= m)
                    CHECK(consistency_gate(seen, agree, m) == (agree >= m));
            }
    // the three pixels of the hand-made scanline (tests/test_f2c_consistency_cpu.py)
    CHECK(!consistency_gate(2, 0, 2));   // contradicted by both neighbours
    CHECK(consistency_gate(0, 0, 2));    // its line leaves the field in both
    CHECK(consistency_gate(1, 1, 2));    // seen by one view, which agrees
    CHECK(!consistency_gate(1, 0, 2));
}

// consistency_gate_visit counts what consistency_visit counts
static void the_visit()
{
    const float d = 0.5f, tol = 0.125f;
    const float others[] = {0.5f, 0.625f, 0.6251f, 0.375f, 0.3749f, 3.0f, -1.0f, kInf, kNan};
    for (int in_field = 0; in_field < 2; in_field++)
        for (int ok_t = 0; ok_t < 2; ok_t++)
            for (float dt : others) {
                const bool ok = ok_t && consistency_finite(dt);
                ConsistencyAcc a = consistency_start(d);
                consistency_visit(&a, in_field != 0, d, dt, ok, tol);
                int32_t seen = 0, agree = 0;
                consistency_gate_visit(&seen, &agree, in_field != 0, d, dt, ok, tol);
                CHECK(seen == a.seen && agree == a.agree);
            }
}

static void arguments()
{
    CHECK(f2c_consistency_mask_args(3, 2, 5, 0.25f, 1, false) == kConsistencyOk);
    CHECK(f2c_consistency_mask_args(1, 1, 1, 0.0f, 7, false) == kConsistencyOk);
    CHECK(f2c_consistency_mask_args(0, 2, 5, 0.25f, 1, false) == kConsistencyBadShape);
    CHECK(f2c_consistency_mask_args(3, -1, 5, 0.25f, 1, false) == kConsistencyBadShape);
    CHECK(f2c_consistency_mask_args(3, 2, 0, 0.25f, 1, false) == kConsistencyBadShape);
    CHECK(f2c_consistency_mask_args(3, 2, 5, -0.25f, 1, false) == kConsistencyBadTol);
    CHECK(f2c_consistency_mask_args(3, 2, 5, kNan, 1, false) == kConsistencyBadTol);
    CHECK(f2c_consistency_mask_args(3, 2, 5, kInf, 1, false) == kConsistencyBadTol);
    CHECK(f2c_consistency_mask_args(3, 2, 5, 0.25f, 0, false) == kConsistencyBadMinAgree);   // K12 takes 0; the gate asks for 1
    CHECK(f2c_consistency_mask_args(3, 2, 5, 0.25f, -3, false) == kConsistencyBadMinAgree);
    CHECK(f2c_consistency_mask_args(3, 2, 5, 0.25f, 1, true) == kConsistencyAlias);
    // the order: shape, tol, min_agree, alias
    CHECK(f2c_consistency_mask_args(0, 2, 5, kNan, 0, true) == kConsistencyBadShape);
    CHECK(f2c_consistency_mask_args(3, 2, 5, kNan, 0, true) == kConsistencyBadTol);
    CHECK(f2c_consistency_mask_args(3, 2, 5, 0.25f, 0, true) == kConsistencyBadMinAgree);

    CHECK(f2c_consistency_args(0.25f, 2) == kF2cConsistencyOk);
    CHECK(f2c_consistency_args(0.0f, 1) == kF2cConsistencyOk);
    CHECK(f2c_consistency_args(0.25f, -1) == kF2cConsistencyBadMinAgree);
    CHECK(f2c_consistency_args(kNan, -1) == kF2cConsistencyBadMinAgree);
    CHECK(f2c_consistency_args(-0.5f, 2) == kF2cConsistencyBadTol);
    CHECK(f2c_consistency_args(kNan, 2) == kF2cConsistencyBadTol);
    CHECK(f2c_consistency_args(kInf, 2) == kF2cConsistencyBadTol);
    CHECK(f2c_consistency_args(-kInf, 2) == kF2cConsistencyBadTol);
    // off: tol is not looked at
    CHECK(f2c_consistency_args(kNan, 0) == kF2cConsistencyOk);
    CHECK(f2c_consistency_args(-1.0f, 0) == kF2cConsistencyOk);
}

static void applies_and_bytes()
{
    const F2cValidity rules[] = {kValidAll, kValidLineConf, kValidEdgeConf, kValidDispConf};
    for (F2cValidity r : rules)
        for (int m = -1; m <= 3; m++) {
            CHECK(f2c_consistency_applies(m, r) == (m > 0 && r != kValidAll));
            // beside f2c_unique_applies: the same levels
            CHECK(f2c_consistency_applies(m, r) == f2c_unique_applies(m > 0 ? 0.5f : 0.0f, r));
        }
    CHECK(f2c_consistency_level_bytes(false, 5, LevelDims{44, 64}) == 0);
    CHECK(f2c_consistency_level_bytes(true, 5, LevelDims{44, 64}) == (size_t)5 * 44 * 64 * 8);
    CHECK(f2c_consistency_level_bytes(true, 0, LevelDims{44, 64}) == 0);
    CHECK(f2c_consistency_level_bytes(true, 5, LevelDims{0, 64}) == 0);
    CHECK(f2c_consistency_level_bytes(true, 101, LevelDims{1080, 1920}) == (size_t)101 * 1080 * 1920 * 8);   // past 2^31 cells * bytes
    // one launch: 4 + 1 in, 1 out, 4 per count plane -- less than K12 writing one count plane and no validity reads it back
    CHECK(f2c_consistency_bytes(5, 44, 64, false, false) == (size_t)5 * 44 * 64 * 6);
    CHECK(f2c_consistency_bytes(5, 44, 64, true, false) == (size_t)5 * 44 * 64 * 10);
    CHECK(f2c_consistency_bytes(5, 44, 64, true, true) == (size_t)5 * 44 * 64 * 14);
    CHECK(f2c_consistency_bytes(101, 1080, 1920, true, true) == (size_t)101 * 1080 * 1920 * 14);
    CHECK(f2c_consistency_bytes(5, 44, 64, false, false) + (size_t)5 * 44 * 64 * 3 == consistency_bytes(5, 44, 64, true, 1, false, false));
    // the gate launch shares K12's grid and its limits
    CHECK(consistency_grid(5, 44, 64) == 48u * 5u);
    CHECK(consistency_grid(5, 44, kConsistencyMaxU + 1) == 0u);
}

int main()
{
    the_gate();
    the_visit();
    arguments();
    applies_and_bytes();
    printf("f2c consistency plan tests ok\n");
    return 0;
}
