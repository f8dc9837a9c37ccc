// The host-side decisions of a kept fine-to-coarse run's peak planes and of its validity by uniqueness (rslf_f2c_run_host_pk;
// rslf_f2c.hip, rslf_f2c_keep.hip, rslf_f2c_peaks.hip): the argument checks and what the planes take on the device.  Host-only
// like rslf_plan.hpp, which it continues; pure functions, tested by tests/cpp/test_plan_f2c_peaks.cpp.
#pragma once

#include "rslf_plan.hpp"
#include "rslf_plan_peaks.hpp"

namespace rslf {
namespace plan {

// What rslf_f2c_run_host_pk refuses, in the order it looks: the first argument at fault, kF2cPeaksOk for none.
//   peaks        0 or 1
//   ratio        0 (off) or in (0, 1]; a NaN is no ratio
//   ratio != 0   needs the peak planes
//   dim_d        with peaks, at most what rslf_sweep_peaks takes (kPeakMaxDimD)
enum F2cPeaksArg { kF2cPeaksOk = 0, kF2cPeaksBadFlag = 1, kF2cPeaksBadRatio = 2, kF2cPeaksRatioAlone = 3, kF2cPeaksBadDimD = 4 };
inline bool f2c_uniqueness_ok(float ratio) { return ratio >= 0.0f && ratio <= 1.0f; }   // (false for a NaN)
inline F2cPeaksArg f2c_peaks_args(int peaks, float ratio, int dim_d)
{
    if (peaks != 0 && peaks != 1)
        return kF2cPeaksBadFlag;
    if (!f2c_uniqueness_ok(ratio))
        return kF2cPeaksBadRatio;
    if (ratio != 0.0f && !peaks)
        return kF2cPeaksRatioAlone;
    if (peaks && dim_d > kPeakMaxDimD)
        return kF2cPeaksBadDimD;
    return kF2cPeaksOk;
}

// The uniqueness predicate touches a level's validity iff the ratio is on and the level was not accepted whole
// (accept_all_last_scale: kValidAll stays everything).
inline bool f2c_unique_applies(float ratio, F2cValidity rule) { return ratio > 0.0f && rule != kValidAll; }

// Device bytes of the peak planes of a kept run, beside f2c_kept_level_bytes / f2c_kept_bytes (which keep their values): per
// level idx, score, runner_idx, runner_score [S][V_p][U_p], 4 bytes each; for the run those of every level plus the fused
// four and the fused_level bytes at the finest size.  0 when the run holds none.
inline size_t f2c_peaks_level_bytes(bool peaks, int S, LevelDims d)
{
    if (!peaks || S < 1 || d.V < 1 || d.U < 1)
        return 0;
    return (size_t)S * (size_t)d.V * (size_t)d.U * 4 * sizeof(float);
}
inline size_t f2c_peaks_bytes(bool peaks, int S, const std::vector<LevelDims>& dims)
{
    if (!peaks || dims.empty() || S < 1)
        return 0;
    size_t total = (size_t)S * (size_t)dims[0].V * (size_t)dims[0].U * (4 * sizeof(float) + 1);
    for (const LevelDims& d : dims)
        total += f2c_peaks_level_bytes(true, S, d);
    return total;
}

// k11_fuse_peaks: lanes along u of the finest plane, a scanline of a view per (y, z) of the grid
constexpr int kFusePeaksBlock = 256;
inline bool f2c_fuse_peaks_grid_ok(int S, int V0, int U0) { return S >= 1 && V0 >= 1 && U0 >= 1 && S <= 65535 && V0 <= 65535; }

}  // namespace plan
}  // namespace rslf
