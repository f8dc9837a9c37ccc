// The host-side decisions of the view warp (rslf_view_warp; rslf_warp.hip, k14_view_warp.hpp): which arguments are arguments,
// how much LDS a row's z-buffer takes and how wide a row may be, the grid of a launch and its limit, the source views a target
// asks and the order they rank in, and the bytes the step has to move.  Host-only like rslf_plan.hpp, which it continues; pure
// functions, g++ compiles it alone; tested by tests/cpp/test_plan_warp.cpp.  The per-pixel rule itself is k14_warp_rule.hpp,
// shared with the kernel.
#pragma once

#include <limits.h>
#include <stddef.h>

#include "k14_warp_rule.hpp"

namespace rslf {
namespace plan {

constexpr int kWarpBlock = 256;   // threads of a workgroup: one (target, scanline) row, walked in strides of 256 columns
constexpr int kWarpBatch = 4;     // column strides whose loads a thread has in flight before the first test
// The targets of one launch: their positions and exclusions travel in the kernel's arguments (2 KiB of the 4 KiB a launch
// has), so a call needs no scratch and no copy that outlives it; a call with more targets is several launches.
constexpr int kWarpLaunchTargets = 256;
// The width cap.  The z-buffer is one 64-bit key per column, the candidate counts -- only when asked for -- one dword more:
// 8 or 12 bytes per column of the 160 KiB of LDS a gfx950 CU has.  8192 columns (>= kEpiLinesMaxU, 8000) are 64 KiB of keys:
// two workgroups still share a CU at the cap (one with the counts, 96 KiB), and at the widths the project's fields have
// (1920 columns: 15 or 22.5 KiB) LDS allows ten or seven, so the eight waves a SIMD holds bound the occupancy, not the LDS.
// A cap at the LDS's end (13000 columns with counts) would leave one workgroup of four waves per CU with nothing to hide its
// loads behind.
constexpr int kWarpMaxU = 8192;
constexpr size_t kWarpLdsBudget = (size_t)160 << 10;

// What rslf_view_warp refuses, in the order it looks: the first fault, kWarpOk for none.
//   shape       S, V, U >= 1
//   targets     T >= 1
//   nearer      != 0
//   outputs     at least one of the nine planes
//   alias       no output plane is an input plane
//   volume      colour or err without a volume, or with one whose V, S, U differ
enum WarpArg { kWarpOk = 0, kWarpBadShape, kWarpBadTargets, kWarpBadNearer, kWarpNoOutput, kWarpAlias, kWarpNoVolume, kWarpVolumeShape };
inline WarpArg warp_args(int S, int V, int U, int T, int nearer, bool any_output, bool aliased, bool needs_volume, bool have_volume,
                         int vol_V, int vol_S, int vol_U)
{
    if (S < 1 || V < 1 || U < 1)
        return kWarpBadShape;
    if (T < 1)
        return kWarpBadTargets;
    if (nearer == 0)
        return kWarpBadNearer;
    if (!any_output)
        return kWarpNoOutput;
    if (aliased)
        return kWarpAlias;
    if (needs_volume && !have_volume)
        return kWarpNoVolume;
    if (needs_volume && (vol_V != V || vol_S != S || vol_U != U))
        return kWarpVolumeShape;
    return kWarpOk;
}

// One target: finite and within 65536; with err also integral and in [0, S).
enum WarpTarget { kWarpTargetOk = 0, kWarpTargetRange, kWarpTargetNotAView };
inline WarpTarget warp_target_arg(float t, int S, bool err)
{
    if (!warp_target_ok(t))
        return kWarpTargetRange;
    if (err && !warp_target_integral(t, S))
        return kWarpTargetNotAView;
    return kWarpTargetOk;
}

// Dynamic LDS of a workgroup: keys [U] of 8 bytes, then -- with the counts -- [U] dwords.
inline size_t warp_lds_bytes(int U, bool count) { return (size_t)U * (count ? 12 : 8); }

// What one launch cannot hold, RSLF_ERR_UNSUPPORTED: a row wider than the z-buffer, more views than a key's 16 bits count,
// more rows than a grid.
enum WarpLimit { kWarpFits = 0, kWarpTooWide, kWarpTooManyViews, kWarpGridLimit };

// The grid of a call's T targets: one workgroup per (target, scanline), a scanline's T workgroups in a row, the scanlines
// dealt to the 8 XCDs in turn (xcd_logical_block_rows) -- 8 * ceil(V / 8) scanlines' worth, the surplus ones return at once.
// 0: T * 8 * ceil(V / 8) is not below 2^31.
inline unsigned warp_grid(int V, int T)
{
    if (V < 1 || T < 1)
        return 0u;
    const long long blocks = (((long long)V + 7) / 8 * 8) * (long long)T;
    return blocks <= (long long)INT_MAX ? (unsigned)blocks : 0u;
}
inline WarpLimit warp_limits(int S, int V, int U, int T)
{
    if (U > kWarpMaxU)
        return kWarpTooWide;
    if (S > kWarpMaxViews)
        return kWarpTooManyViews;
    if (!warp_grid(V, T))
        return kWarpGridLimit;
    return kWarpFits;
}
// A call's launches: targets [first, first + n) each, n <= kWarpLaunchTargets.
inline int warp_launches(int T) { return (T + kWarpLaunchTargets - 1) / kWarpLaunchTargets; }
inline int warp_launch_targets(int T, int launch)
{
    const int left = T - launch * kWarpLaunchTargets;
    return left < kWarpLaunchTargets ? left : kWarpLaunchTargets;
}

// The source window of a target: the views [*s0, *s1] within the radius (every view for radius <= 0); false: none.
inline bool warp_window(float t, int S, int radius, int* s0, int* s1)
{
    int first = -1, last = -1;
    for (int s = 0; s < S; s++)
        if (warp_in_window(s, t, radius)) {
            first = first < 0 ? s : first;
            last = s;
        }
    *s0 = first, *s1 = last;
    return first >= 0;
}

// The rank order: order[k] is the view of rank k -- by (distance to t, s) -- for all S views.
inline void warp_rank_order(float t, int S, int* order)
{
    WarpWalk w = warp_walk_start(t, S);
    int s = 0, k = 0;
    while (warp_walk_next(&w, t, S, &s))
        order[k++] = s;
}

// The algorithmic bytes: per scanline the window's source rows -- disparity and validity byte -- read ONCE for all the targets
// of the call (they share an L2), one slab row gathered per hit for colour and one more read for err, every plane asked for
// written once.
struct WarpPlanes {
    bool hit, depth, src_view, src_col, count, colour, err, rows;
};
inline size_t warp_out_bytes_per_cell(const WarpPlanes& p, int C)
{
    return (p.hit ? 1 : 0) + (size_t)4 * ((p.depth ? 1 : 0) + (p.src_view ? 1 : 0) + (p.src_col ? 1 : 0) + (p.count ? 1 : 0) + (p.err ? 1 : 0)) +
           (p.colour ? (size_t)4 * C : 0);
}
inline size_t warp_bytes(int S_window, int V, int U, int T, int C, bool have_valid, const WarpPlanes& p)
{
    const size_t row = (size_t)V * (size_t)U;
    const size_t in = (size_t)S_window * row * (4 + (have_valid ? 1 : 0));
    const size_t vol = (p.colour || p.err ? (size_t)T * row * 4 * C : 0) + (p.err ? (size_t)T * row * 4 * C : 0);
    return in + vol + (size_t)T * row * warp_out_bytes_per_cell(p, C) + (p.rows ? (size_t)T * V * 12 : 0);
}

}  // namespace plan
}  // namespace rslf
