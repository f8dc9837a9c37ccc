// The host-side decisions of the cross-view consistency check (rslf_view_consistency; rslf_consistency.hip,
// k12_consistency.hpp): which arguments are arguments, how large a volume one launch's grid takes, which views a radius
// leaves, and the bytes the step has to move.  Host-only like rslf_plan.hpp, which it continues; pure functions, g++ compiles
// it alone; tested by tests/cpp/test_plan_consistency.cpp.  The per-pixel rule itself is k12_consistency_rule.hpp, shared
// with the kernel.
#pragma once

#include <limits.h>
#include <stddef.h>

#include "k12_consistency_rule.hpp"

namespace rslf {
namespace plan {

constexpr int kConsistencyBlock = 256;   // threads of a workgroup = columns of a segment of a (view, scanline) row
constexpr int kConsistencyBatch = 8;     // views whose target pixels a thread has in flight together
// A column u plus a rounded offset below 1e9 in magnitude must stay an int: U is at most 2^30.
constexpr int kConsistencyMaxU = 1 << 30;

// What rslf_view_consistency refuses, in the order it looks: the first fault, kConsistencyOk for none.
//   shape      S, V, U >= 1
//   tol        finite and >= 0
//   min_agree  >= 0
//   outputs    at least one of the six planes
//   alias      no output plane is an input plane (a thread reads the OTHER views' rows while their workgroups write)
enum ConsistencyArg { kConsistencyOk = 0, kConsistencyBadShape, kConsistencyBadTol, kConsistencyBadMinAgree, kConsistencyNoOutput,
                      kConsistencyAlias };
inline ConsistencyArg consistency_args(int S, int V, int U, float tol, int min_agree, bool any_output, bool aliased)
{
    if (S < 1 || V < 1 || U < 1)
        return kConsistencyBadShape;
    if (!(tol >= 0.0f) || !consistency_finite(tol))
        return kConsistencyBadTol;
    if (min_agree < 0)
        return kConsistencyBadMinAgree;
    if (!any_output)
        return kConsistencyNoOutput;
    if (aliased)
        return kConsistencyAlias;
    return kConsistencyOk;
}

inline int consistency_segments(int U) { return (int)(((long long)U + kConsistencyBlock - 1) / kConsistencyBlock); }

// The grid of one launch: one workgroup per segment of a (view, scanline) row, a scanline's S * segments workgroups in a
// row, the scanlines dealt to the 8 XCDs in turn (xcd_logical_block_rows) -- so the launch has 8 * ceil(V / 8) scanlines'
// worth and the surplus ones return at once.  0: past what a grid holds (or U past kConsistencyMaxU).
inline unsigned consistency_grid(int S, int V, int U)
{
    if (S < 1 || V < 1 || U < 1 || U > kConsistencyMaxU)
        return 0u;
    const long long row_blocks = (long long)S * consistency_segments(U);
    const long long rows = ((long long)V + 7) / 8 * 8;
    if (row_blocks > (long long)INT_MAX)
        return 0u;
    const long long blocks = rows * row_blocks;
    return blocks <= (long long)INT_MAX ? (unsigned)blocks : 0u;
}

// The views a pixel of view s asks (the rule's window), and how many rows of a scanline a workgroup of view s touches.
inline int consistency_window_rows(int s, int S, int radius)
{
    int t0, t1;
    consistency_window(s, S, radius, &t0, &t1);
    return t1 - t0 + 1;
}

// The algorithmic bytes: every cell's disparity and validity byte read once, every plane asked for written once.
inline size_t consistency_out_bytes_per_cell(int n_count_planes, bool fused, bool valid_out)
{
    return (size_t)n_count_planes * 4 + (fused ? 4 : 0) + (valid_out ? 1 : 0);
}
inline size_t consistency_bytes(int S, int V, int U, bool have_valid, int n_count_planes, bool fused, bool valid_out)
{
    const size_t cells = (size_t)S * (size_t)V * (size_t)U;
    return cells * (4 + (have_valid ? 1 : 0) + consistency_out_bytes_per_cell(n_count_planes, fused, valid_out));
}

// The host form stages both inputs and all six planes in the context's shared buffers: bytes of the output stage per cell.
constexpr size_t kConsistencyStageOutBytes = 4 * 4 + 4 + 1;

}  // namespace plan
}  // namespace rslf
