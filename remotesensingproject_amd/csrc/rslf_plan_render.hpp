// The host-side decisions of the BATCHED renderers (rslf_render_fit_many, rslf_render_planes_each and the host-pointer
// forms; rslf_render.hip, k6_render.hpp): how many workgroups a batch of planes gets, how large its scratch is, how
// many launches a fit costs, when a batch may use 16-byte loads.  Host-only like rslf_plan.hpp, which it continues (that
// header is near the length limit of a library source); pure functions, tested by tests/cpp/test_plan_render_batch.cpp.
#pragma once

#include "rslf_plan.hpp"

namespace rslf {
namespace plan {

constexpr int kRenderMaxPlanes = 65535;        // a plane is blockIdx.y of every batched launch
constexpr long long kFitMaxPixels = 1ll << 30; // per plane: the select counts in 32 bits
constexpr int kFitBatchMaxGroups = 4096;       // workgroups of one fit launch over a batch, unless the planes alone are more
constexpr size_t kSelectStateBytes = (2 * (size_t)kRadixBins + 4) * sizeof(uint32_t);   // k6_render.hpp: SelectState
constexpr size_t kFitPartialBytes = 2 * sizeof(double) + 2 * sizeof(float);             // k6_render.hpp: FitPartial

// The double sums of a plane are added in an order fixed by the plane's size alone: fit_blocks(n) partial sums ("sum
// blocks"), then their fixed-order reduction.  A batch only decides how many WORKGROUPS share a plane's sum blocks: each
// takes every groups-th block.  So plane k of a batch gets the bits of the single call, whatever the batch's size.
// One plane: fit_blocks(n) workgroups, one per sum block (the single call).  Many planes: the launch stays near
// kFitBatchMaxGroups workgroups in all -- 65535 planes of a few pixels get one each, not 1024.
inline int fit_batch_groups(int n_planes, long long n)
{
    const long long share = std::max<long long>(1, kFitBatchMaxGroups / std::max(1, n_planes));
    return (int)std::min<long long>(fit_blocks(n), share);
}
// ... and the bound the above keeps: groups * n_planes <= fit_batch_max_groups(n_planes)
inline long long fit_batch_max_groups(int n_planes)
{
    return std::max<long long>(kFitBatchMaxGroups, n_planes);
}

// Scratch of a fit over n_planes planes of n pixels.  State slot: one select state per plane, then (16-byte aligned) one
// result per plane -- two floats for the order statistics, a FitPartial otherwise.  Slab slot: the sum blocks' partials.
inline size_t fit_result_offset(int n_planes)
{
    return ((size_t)n_planes * kSelectStateBytes + 15) / 16 * 16;
}
inline size_t fit_state_bytes(int n_planes)
{
    return fit_result_offset(n_planes) + (size_t)n_planes * kFitPartialBytes;
}
inline size_t fit_slab_bytes(int n_planes, long long n)
{
    return (size_t)n_planes * (size_t)fit_blocks(n) * kFitPartialBytes;
}

// Launches of one fit, for any number of planes.  mode: RSLF_FIT_* (1 = QUANTILE: init, then count + narrow per digit;
// MINMAX and MEANSTD: partial sums + reduction).  Then one copy to the host and one wait.
constexpr int fit_launches(int mode)
{
    return mode == 1 ? 1 + 2 * kRadixPasses : 2;
}

// 16-byte loads in a fit over a batch: render_vec4_ok, where the plane stride counts only if a second plane exists.
inline bool fit_vec4_ok(int cols, long long row_stride, long long plane_stride, int n_planes, const void* planes, const void* valid)
{
    return render_vec4_ok(cols, row_stride, n_planes > 1 ? plane_stride : 0, planes, valid, nullptr);
}

// The table a per-plane render reads: the colour table's 256 x 3 bytes, then one (a, b) pair of floats per plane.
constexpr size_t kRenderTableBytes = 256 * 3;
inline size_t render_table_bytes(int n_planes)
{
    return kRenderTableBytes + (size_t)n_planes * 2 * sizeof(float);
}

// Elements from the first to one past the last element of a stack of strided planes (what a host-pointer form copies).
inline size_t planes_extent(int n_planes, size_t plane_stride, int rows, int cols, size_t row_stride)
{
    return (size_t)(n_planes - 1) * plane_stride + (size_t)(rows - 1) * row_stride + (size_t)cols;
}

}  // namespace plan
}  // namespace rslf
