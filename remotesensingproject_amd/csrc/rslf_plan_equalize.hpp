// The pure decisions of the per-view equalisation (K19: rslf_equalize.hip, k19_equalize.hpp): what the entries refuse of a
// shape, how a row of pixels splits into peeled ends and groups of four pixels, which lane owns which floats and what
// channel each of them has, the tile of a workgroup, the capped grids of the two kernels and the walk of the statistics
// kernel over the rows of one view.  No HIP; g++ compiles it alone; every function is constexpr, so the kernels run the
// same ones; tested by tests/cpp/test_plan_equalize.cpp.  The per-sample rule itself is k19_equalize_rule.hpp.
//
// Everything here counts PIXELS (C floats each).  A lane owns four consecutive pixels of a row's body: 4 C floats that start
// at a multiple of 16 bytes, C loads of 16 bytes -- one at C = 1, three at C = 3 -- and float j of the lane's 4 C has channel
// j % C, a compile-time fact of its register.
#pragma once

#include <limits.h>
#include <stddef.h>

#include "k19_equalize_rule.hpp"

namespace rslf {
namespace plan {

constexpr int kEqBlock = 256;                     // threads of a workgroup
constexpr int kEqLane = 4;                        // consecutive pixels a lane owns
constexpr int kEqTile = kEqBlock * kEqLane;       // pixels of a tile
constexpr unsigned kEqGridCap = 2048;             // memory-bound kernels: 256 CUs x 8 workgroups, the work beyond strided over

// What the entries refuse of a field's shape, in the order they look.
enum EqualizeArg { kEqOk = 0, kEqBadShape, kEqTooLarge };
constexpr EqualizeArg equalize_shape(int V, int S, int U, int C)
{
    if (V < 1 || S < 1 || U < 1 || (C != 1 && C != 3))
        return kEqBadShape;
    // a view's V * U samples are counted exactly (k19_equalize_rule.hpp); a row's U * C floats and the V * S rows are ints
    if ((long long)V * U > kEqMaxSamples || (long long)U > (INT_MAX - 64) / 3 || (long long)V * S > (long long)INT_MAX)
        return kEqTooLarge;
    return kEqOk;
}

// How the pixels [0, U) of a row split: `head` pixels handled one by one, then `body` pixels in groups of four whose first
// float is 16-byte aligned, then `tail` pixels one by one.
struct EqualizeRow {
    int head, body, tail;
};
// The volume form: rows start at multiples of 256 bytes and are `pitch` pixels long (a multiple of 64), pad included: all body.
constexpr EqualizeRow equalize_row_volume(int pitch) { return EqualizeRow{0, pitch, 0}; }
// The dense form: the row starts `row_first` pixels (row * U) after the base; pixel p's first float is float
// (row_first + p) * C of the level, 16-byte aligned exactly when row_first + p is a multiple of 4 (C is 1 or 3) and the base
// is.  A base that is not: the whole row is peeled.
constexpr EqualizeRow equalize_row_dense(long long row_first, int U, bool base_aligned)
{
    if (!base_aligned)
        return EqualizeRow{U, 0, 0};
    const int lead = (int)((4 - row_first % 4) % 4);
    const int head = lead < U ? lead : U;
    const int body = (U - head) / kEqLane * kEqLane;
    return EqualizeRow{head, body, U - head - body};
}
constexpr int equalize_peeled(const EqualizeRow& r) { return r.head + r.tail; }
// The k-th peeled pixel of a row, k in [0, head + tail).
constexpr int equalize_peeled_pixel(const EqualizeRow& r, int k) { return k < r.head ? k : r.body + k; }

// Tiles of a row: its body in runs of kEqTile pixels; a row without a body still has tile 0, which also does the peel.  A
// launch gives every row equalize_tiles_per_row(pitch) or, in the dense form, (U) of them -- no row's body is longer -- and a
// tile at or beyond the end of its row's body (other than tile 0) has nothing to do.
constexpr int equalize_tiles_per_row(int body) { return body < 1 ? 1 : (body + kEqTile - 1) / kEqTile; }
constexpr bool equalize_tile_works(const EqualizeRow& r, int t) { return t == 0 || t * kEqTile < r.body; }
// The joint statistic adds three channels' sums as uint64: 3 * V * U * 65535^2 must stay below 2^64, a tighter cap than
// kEqMaxSamples (1431699457 samples per view).  A joint field beyond it is refused like a field beyond kEqMaxSamples.
constexpr bool equalize_joint_fits(int V, int U) { return (long long)V * U <= kEqMaxSamplesJoint; }
// The first pixel of lane `tid`'s group in tile t, and whether the group lies inside the body (all four pixels do then).
constexpr int equalize_lane_first(const EqualizeRow& r, int t, int tid) { return r.head + t * kEqTile + kEqLane * tid; }
constexpr bool equalize_lane_works(const EqualizeRow& r, int p0) { return p0 < r.head + r.body; }
// Float j of a lane's group (j in [0, 4 C)): its pixel within the group and its channel.
constexpr int equalize_float_pixel(int j, int C) { return j / C; }
constexpr int equalize_float_channel(int j, int C) { return j % C; }

// The apply kernel: one workgroup per (row, tile), capped and strided.
constexpr unsigned equalize_apply_grid(long long tiles) { return tiles < 1 ? 0u : (tiles < (long long)kEqGridCap ? (unsigned)tiles : kEqGridCap); }

// The statistics kernel: a workgroup walks rows of ONE view at a time, so that its totals go out as one atomic add per
// total and view.  A view's work is V * tiles_per_row items (item i: v = i / tiles_per_row, t = i % tiles_per_row; the row
// is v * S + s); `per_view` workgroups share it, workgroup w taking the items w, w + per_view, ...; the grid is `groups`
// such teams, team g doing the views g, g + groups, ...  groups * per_view <= kEqGridCap.
struct EqualizeStatsGrid {
    int per_view, groups;
};
constexpr EqualizeStatsGrid equalize_stats_grid(int V, int S, int tiles_per_row)
{
    const long long items = (long long)V * tiles_per_row;
    const long long room = (long long)kEqGridCap / S;   // workgroups a view can have when every view has a team
    const int per_view = room < 1 ? 1 : (int)(items < room ? items : room);
    const int groups = S < (int)kEqGridCap / per_view ? S : (int)kEqGridCap / per_view;
    return EqualizeStatsGrid{per_view, groups};
}
constexpr unsigned equalize_stats_blocks(const EqualizeStatsGrid& g) { return (unsigned)g.per_view * (unsigned)g.groups; }
constexpr int equalize_stats_team(const EqualizeStatsGrid& g, unsigned block) { return (int)(block / (unsigned)g.per_view); }
constexpr int equalize_stats_member(const EqualizeStatsGrid& g, unsigned block) { return (int)(block % (unsigned)g.per_view); }

}  // namespace plan
}  // namespace rslf
