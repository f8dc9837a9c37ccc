// The host-side decisions of the 2-D sweep's gate by peak ratio (rslf_sweep_propagation_ratio; rslf_sweep.hip,
// k4_propagate.hpp): which ratios are ratios, which planes the gate reads, when the setter may be called and what it takes on
// the device.  The predicate itself is k11_f2c_peak_rule.hpp's f2c_peak_ambiguous, the one a kept pyramid's validity uses:
// K4 and K11 include that one statement, and sweep_source_withheld below only names it for the sweep.  Host-only apart from
// that header; pure functions, g++ compiles it alone; tested by tests/cpp/test_plan_sweep_gate.cpp.
#pragma once

#include <stddef.h>

#include "k11_f2c_peak_rule.hpp"

namespace rslf {
namespace plan {

// 0 is "off"; a ratio is in (0, 1].  A NaN, a negative value and a value above 1 are refused.
inline bool sweep_gate_ratio_ok(float ratio) { return ratio >= 0.0f && ratio <= 1.0f; }   // (false for a NaN)
inline bool sweep_gate_on(float ratio) { return ratio > 0.0f && ratio <= 1.0f; }

// The gate reads all four planes of the peaks mode at the visited view: a NULL among them leaves the predicate undefined.
inline bool sweep_gate_planes_ok(bool idx, bool score, bool runner_idx, bool runner_score)
{
    return idx && score && runner_idx && runner_score;
}

// What rslf_sweep_propagation_ratio refuses, in the order it looks: the first fault, kSweepGateOk for none.
//   ratio     0 or in (0, 1]
//   window    between rslf_sweep_begin (and rslf_sweep_peaks) and the first visit's scan
//   peaks     a ratio above 0 needs the peaks mode ...
//   planes    ... with all four planes
// A ratio of 0 inside the window is always accepted: it switches the gate off, whatever the peaks mode.
enum SweepGateArg { kSweepGateOk = 0, kSweepGateBadRatio = 1, kSweepGateWindow = 2, kSweepGateNoPeaks = 3, kSweepGateNullPlane = 4 };
inline SweepGateArg sweep_gate_args(float ratio, bool open, bool scanned, bool first, bool peaks_on, bool idx, bool score,
                                    bool runner_idx, bool runner_score)
{
    if (!sweep_gate_ratio_ok(ratio))
        return kSweepGateBadRatio;
    if (!open || scanned || !first)
        return kSweepGateWindow;
    if (ratio == 0.0f)
        return kSweepGateOk;
    if (!peaks_on)
        return kSweepGateNoPeaks;
    if (!sweep_gate_planes_ok(idx, score, runner_idx, runner_score))
        return kSweepGateNullPlane;
    return kSweepGateOk;
}

// What the *_pr entries refuse before they queue anything: the ratio, and a ratio above 0 without the four planes.
inline SweepGateArg sweep_gate_entry_args(float ratio, bool have_peaks, bool idx, bool score, bool runner_idx, bool runner_score)
{
    return sweep_gate_args(ratio, true, false, true, have_peaks, idx, score, runner_idx, runner_score);
}

// The gate's only buffer: the sweep's count of withheld sources, one 8-byte counter, sized when the ratio is set.  0 when off.
inline size_t sweep_gate_counter_bytes(float ratio) { return sweep_gate_on(ratio) ? 8 : 0; }

// A pixel that passed the gate of core.hpp:1097-1103 is withheld iff its peaks are ambiguous at the ratio.  r = 1 withholds
// nothing: a runner-up never scores above its winner.  A NaN score compares false.
inline bool sweep_source_withheld(bool passes_gate, int32_t idx, int32_t runner_idx, float score, float runner_score, float ratio)
{
    return passes_gate && f2c_peak_ambiguous(idx, runner_idx, score, runner_score, ratio);
}

}  // namespace plan
}  // namespace rslf
