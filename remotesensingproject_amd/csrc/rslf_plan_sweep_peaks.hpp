// The host-side decisions of the 2-D sweep's peaks mode (rslf_sweep_peaks; rslf_sweep.hip, rslf_sweep_peaks.hip,
// k10_sweep_peaks.hpp): which form of the peaks step a visit queues, the list form's fixed grid, the sizes of the step's own
// buffers.  Host-only like rslf_plan.hpp, which it continues; pure functions, tested by tests/cpp/test_plan_sweep_peaks.cpp.
#pragma once

#include "rslf_plan_peaks.hpp"

namespace rslf {
namespace plan {

// The peaks mode of a 2-D sweep (rslf_sweep_peaks): which form of the step a visit queues after its scan (and after the
// sub-grid refinement, which still needs the visit's list).  The list form runs iff the visit's scan took the packed list
// the previous apply pass left -- never the first visit, never when that pass listed nothing ("force_packed" = 0, a plane of
// more than INT32_MAX pixels) -- and the "peaks_list" hook is on.  Every other visit of a sweep in the mode takes the dense
// form (score rows window by window, then k8_score_peaks); a sweep out of the mode takes none.
enum PeaksForm { kPeaksNone = 0, kPeaksDense = 1, kPeaksList = 2 };
inline PeaksForm sweep_peaks_form(bool mode_on, bool first, bool listed, int peaks_list, long long plane_pixels)
{
    if (!mode_on)
        return kPeaksNone;
    if (first || !listed || peaks_list == 0 || plane_pixels > 2147483647ll)
        return kPeaksDense;
    return kPeaksList;
}

// k10_peaks_list: a wave per list entry, kPeaksListWaves waves a workgroup.  The list's length is on the device, so the
// grid is fixed -- what one pass over the device takes, eight workgroups per compute unit -- and its waves stride over the
// entries; never more waves than the plane has pixels for.
constexpr int kPeaksListWaves = 4;
inline unsigned peaks_list_blocks(int V, int U, int num_cus)
{
    if (V < 1 || U < 1)
        return 1;
    const long long need = ((long long)V * U + kPeaksListWaves - 1) / kPeaksListWaves;
    const long long cap = 8ll * (num_cus > 0 ? num_cus : 256);
    return (unsigned)(need < cap ? need : cap);
}
// Rounds of 64 hypotheses a wave walks per entry (d = 64 r + lane)
inline int peaks_list_rounds(int dim_d) { return dim_d < 1 ? 0 : (dim_d + 63) / 64; }

// The dense form's own buffers, sized when the mode is set and grow-only -- the sweep's pixel lists (Scratch::list, count,
// the packed length) belong to the scans and stay untouched: a pixel list [V][U] ints, its per-scanline counts [V] ints
// followed by one 8-byte total, the mask plane [V][U] bytes ("this visit's idx >= 0").  0 when off.
inline size_t sweep_peaks_list_bytes(bool mode_on, int V, int U)
{
    return !mode_on || V < 1 || U < 1 ? 0 : (size_t)V * (size_t)U * sizeof(int);
}
inline size_t sweep_peaks_count_offset_total(int V) { return ((size_t)(V < 0 ? 0 : V) * sizeof(int) + 7) & ~(size_t)7; }
inline size_t sweep_peaks_count_bytes(bool mode_on, int V, int U)
{
    return !mode_on || V < 1 || U < 1 ? 0 : sweep_peaks_count_offset_total(V) + 8;
}
inline size_t sweep_peaks_mask_bytes(bool mode_on, int V, int U) { return !mode_on || V < 1 || U < 1 ? 0 : (size_t)V * (size_t)U; }

// Scanlines per window pass of the dense form and the staging bytes a pass of it takes: rslf_depth_epi_peaks' own
// (peaks_window_rows; at least one scanline), never more than the plane has.
inline int sweep_peaks_pass_rows(int V, int U, int dim_d, size_t budget_bytes)
{
    const int rows = peaks_window_rows(U, dim_d, budget_bytes);
    return rows < V ? (rows < 1 ? 1 : rows) : (V < 1 ? 1 : V);
}
inline size_t sweep_peaks_staging_bytes(int V, int U, int dim_d, size_t budget_bytes)
{
    if (V < 1 || U < 1 || dim_d < 1)
        return 0;
    return peaks_staging_bytes(sweep_peaks_pass_rows(V, U, dim_d, budget_bytes), U, dim_d, false);
}

}  // namespace plan
}  // namespace rslf
