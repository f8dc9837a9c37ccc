// The host-side decisions of a kept fine-to-coarse run's validity by cross-view consistency (rslf_f2c_consistency_mask,
// rslf_f2c_run_host_cs; rslf_consistency.hip, rslf_f2c.hip, rslf_f2c_keep.hip, k13_f2c_consistency.hpp): the argument checks,
// where the gate applies and what it takes on the device.  It continues rslf_plan_consistency.hpp, whose grid, segments and
// limits the gate launch shares.  Host-only, pure functions, g++ compiles it; tested by tests/cpp/test_plan_f2c_consistency.cpp.
// The rule itself, consistency_gate, is in k12_consistency_rule.hpp, shared with the kernel.
#pragma once

#include "rslf_plan.hpp"
#include "rslf_plan_consistency.hpp"

namespace rslf {
namespace plan {

// What rslf_f2c_consistency_mask refuses, in the order it looks (rslf_view_consistency's refusals; a gate asks for at least
// one agreeing view, and its validity output is required, so "no output" cannot occur):
//   shape      S, V, U >= 1
//   tol        finite and >= 0
//   min_agree  >= 1
//   alias      valid_out, agree, seen: none of them an input plane
inline ConsistencyArg f2c_consistency_mask_args(int S, int V, int U, float tol, int min_agree, bool aliased)
{
    if (S < 1 || V < 1 || U < 1)
        return kConsistencyBadShape;
    if (!(tol >= 0.0f) || !consistency_finite(tol))
        return kConsistencyBadTol;
    if (min_agree < 1)
        return kConsistencyBadMinAgree;
    if (aliased)
        return kConsistencyAlias;
    return kConsistencyOk;
}

// What rslf_f2c_run_host_cs refuses of its three trailing arguments before anything is queued.  min_agree = 0 is "off", and
// then tol and radius are not looked at; a negative min_agree is none; with the gate on, tol is finite and >= 0.  (Any radius
// is one: <= 0 asks every view.)
enum F2cConsistencyArg { kF2cConsistencyOk = 0, kF2cConsistencyBadMinAgree = 1, kF2cConsistencyBadTol = 2 };
inline F2cConsistencyArg f2c_consistency_args(float tol, int min_agree)
{
    if (min_agree < 0)
        return kF2cConsistencyBadMinAgree;
    if (min_agree > 0 && (!(tol >= 0.0f) || !consistency_finite(tol)))
        return kF2cConsistencyBadTol;
    return kF2cConsistencyOk;
}

// The gate touches a level's validity iff it is on and the level was not accepted whole (accept_all_last_scale: kValidAll
// stays everything), as f2c_unique_applies.
inline bool f2c_consistency_applies(int min_agree, F2cValidity rule) { return min_agree > 0 && rule != kValidAll; }

// Device bytes a gated run keeps beyond f2c_kept_bytes / f2c_peaks_bytes (which keep their values): per gated level the gate's
// agree and seen planes, int32 [S][V_p][U_p].  The second validity plane takes the first one's place, which is freed with the
// level's other temporaries.  A level accepted whole is not gated and holds none.
inline size_t f2c_consistency_level_bytes(bool gated, int S, LevelDims d)
{
    if (!gated || S < 1 || d.V < 1 || d.U < 1)
        return 0;
    return (size_t)S * (size_t)d.V * (size_t)d.U * 2 * sizeof(int);
}

// The algorithmic bytes of one gate launch: every cell's disparity and validity byte read once, the gated byte written once,
// the count planes asked for written once.
inline size_t f2c_consistency_bytes(int S, int V, int U, bool agree, bool seen)
{
    const size_t cells = (size_t)S * (size_t)V * (size_t)U;
    return cells * (4 + 1 + 1 + (agree ? 4 : 0) + (seen ? 4 : 0));
}

}  // namespace plan
}  // namespace rslf
