// The host-side decisions of the level dilation's two streaming kernels (K18, k18_level_dilate.hpp; rslf_dilate.hip): the
// grids of k18_dilate_ranges and k18_undilate_many and which rows take 16-byte stores.  It continues rslf_plan_dilate.hpp:
// host-only, pure functions, g++ compiles it alone; tested by tests/cpp/test_plan_level_dilate.cpp.  The per-column rule
// and the span a store group covers are k18_ranges_rule.hpp's, shared with the kernel.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "k18_ranges_rule.hpp"
#include "rslf_plan_dilate.hpp"

namespace rslf {
namespace plan {

constexpr int kUndilateMany4 = 8;   // planes of 4-byte elements one k18_undilate_many launch serves ...
constexpr int kUndilateMany1 = 2;   // ... and of 1-byte elements
constexpr unsigned kRangesRowCap = 8192;   // grid.y of k18_dilate_ranges: the rows beyond are strided over

// k18_dilate_ranges: grid.x over a row's store groups, kDilateBlock of them per workgroup, one group of four floats per
// lane.  A row may start up to three floats past a 16-byte boundary, so it has at most (U' + 3 + 3) / 4 groups.
inline unsigned ranges_grid_x(int U_dilated)
{
    if (U_dilated < 1)
        return 0u;
    const long long groups = ranges_groups(3, U_dilated);
    return (unsigned)((groups + kDilateBlock - 1) / kDilateBlock);
}
inline unsigned ranges_grid_y(size_t rows) { return rows < 1 ? 0u : (rows < kRangesRowCap ? (unsigned)rows : kRangesRowCap); }
// The rows take 16-byte stores only when both output planes start on a 16-byte boundary: then row r starts
// (r * U') % 4 floats past one in both.
inline bool ranges_vector_stores(const void* out_min, const void* out_max)
{
    return (((uintptr_t)out_min | (uintptr_t)out_max) & 15u) == 0;
}
inline int ranges_row_offset(size_t row, int U_dilated, bool vector_stores)
{
    return vector_stores ? (int)((row * (size_t)U_dilated) & 3u) : 0;
}

// k18_undilate_many: x over the source-grid columns, y over the rows (capped, strided over), z over the planes.
inline unsigned undilate_many_grid_z(int n4, int n1) { return (unsigned)(n4 + n1); }
inline bool undilate_many_counts_ok(int n4, int n1) { return n4 >= 0 && n1 >= 0 && n4 <= kUndilateMany4 && n1 <= kUndilateMany1 && n4 + n1 >= 1; }

}  // namespace plan
}  // namespace rslf
