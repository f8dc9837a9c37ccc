// The host-side decisions of the 2-D sweep's sub-grid mode (rslf_sweep_subgrid; rslf_sweep.hip, rslf_subgrid.hip,
// k9_subgrid.hpp): which form of the refinement a visit queues, the list form's fixed grid, the planes' sizes.  Host-only like
// rslf_plan.hpp, which it continues (that header is at the length limit of a library source); pure functions, tested by
// tests/cpp/test_plan_sweep_subgrid.cpp.
#pragma once

#include "rslf_plan.hpp"

namespace rslf {
namespace plan {

// The sub-grid mode of a 2-D sweep (rslf_sweep_subgrid): which form of the refinement a visit queues after its scan.  The
// list form runs iff the visit's scan took the packed list the previous apply pass left -- never the first visit, never
// when that pass listed nothing ("force_packed" = 0, a plane of more than INT32_MAX pixels) -- and the "subgrid_list" hook
// is on.  Every other visit of a sweep in the mode takes the dense form; a sweep out of the mode takes none.
enum SubgridForm { kSubgridNone = 0, kSubgridDense = 1, kSubgridList = 2 };
inline SubgridForm sweep_subgrid_form(bool mode_on, bool first, bool listed, int subgrid_list, long long plane_pixels)
{
    if (!mode_on)
        return kSubgridNone;
    if (first || !listed || subgrid_list == 0 || plane_pixels > 2147483647ll)
        return kSubgridDense;
    return kSubgridList;
}

// Workgroups (256 lanes) of the list form's fixed grid: the list's length is on the device, so the grid covers what one
// pass over the device takes -- four workgroups per compute unit -- and strides; never more than the plane has entries for.
inline unsigned subgrid_list_blocks(int V, int U, int num_cus)
{
    if (V < 1 || U < 1)
        return 1;
    const long long need = ((long long)V * U + 255) / 256;
    const long long cap = 4ll * (num_cus > 0 ? num_cus : 256);
    return (unsigned)(need < cap ? need : cap);
}

// Bytes of each of a sweep's two planes [V][U] in the sub-grid mode (arg max: int32, score: float); 0 when off.  With line
// confidence on, the scan writes K7's arg-max plane and the refinement reads that one: one plane for both.
inline size_t sweep_subgrid_plane_bytes(bool mode_on, int V, int U)
{
    if (!mode_on || V < 1 || U < 1)
        return 0;
    return (size_t)V * (size_t)U * 4;
}

}  // namespace plan
}  // namespace rslf
