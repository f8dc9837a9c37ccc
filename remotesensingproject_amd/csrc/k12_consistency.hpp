// K12: cross-view consistency of a sweep's disparity planes (rslf_view_consistency).  Not in the reference: its classes judge
// a pixel inside its own view only (C_e, C_d, C_l); this asks whether the views agree.  The per-pixel rule is
// k12_consistency_rule.hpp, the one statement the host tests compile too; this file is how the device walks it.
//
// One thread per target pixel, one workgroup per 256-column segment of a (view, scanline) row.  A thread's other views are
// visited in batches of kConsistencyBatch: every load of a batch -- the neighbour's disparity and validity byte -- is issued
// UNCONDITIONALLY at a column clamped into the row, before the first test (k4_propagate.hpp records what a load under `if`
// costs with this compiler: a basic block, and a wait, of its own).  The tests then run in ascending view order, which is what
// defines the fused value bit for bit.
//
// Traffic: a workgroup gathers from the rows of ONE scanline in every view of its window -- S * U * 5 bytes per scanline
// (0.97 MB at 1920 x 101), far below an XCD's 4 MiB L2 and above the LDS.  The grid is therefore ordered by scanline: a
// scanline's S * segments workgroups are consecutive logical blocks, and the scanlines are dealt to the XCDs in turn
// (xcd_logical_block_rows, the scan kernels' remap), so the workgroups that share rows share an L2 at about the same time.
// `order` keeps the two orders it was measured against (profiles/r19_consistency.md).  Placement only affects speed.
#pragma once

#include "k12_consistency_rule.hpp"
#include "rslf_device.hpp"
#include "rslf_plan_consistency.hpp"

namespace rslf {

enum ConsistencyOrder {
    kConsistencyOrderXcdRows = 0,   // scanline-major, scanlines dealt to the XCDs in turn (the one kept)
    kConsistencyOrderRows = 1,      // scanline-major, blocks as dispatched: a scanline's workgroups spread over all XCDs
    kConsistencyOrderPlanes = 2,    // the planes' own order [S][V][segments]
};

struct ConsistencyArgs {
    const float* depth;      // [S][V][U]
    const uint8_t* valid;    // [S][V][U], nullable
    int S, V, U, nseg;
    float slope, tol;
    int radius, min_agree;
    int order;
    int32_t* seen;           // [S][V][U] each, nullable
    int32_t* agree;
    int32_t* above;
    int32_t* below;
    float* fused;
    uint8_t* valid_out;
};

__device__ __forceinline__ void consistency_store(const ConsistencyArgs& a, long long o, const ConsistencyResult& r)
{
    if (a.seen)
        a.seen[o] = r.seen;
    if (a.agree)
        a.agree[o] = r.agree;
    if (a.above)
        a.above[o] = r.above;
    if (a.below)
        a.below[o] = r.below;
    if (a.fused)
        a.fused[o] = r.fused;
    if (a.valid_out)
        a.valid_out[o] = r.valid;
}

// HAS_VALID = false: a.valid is NULL and never read (a test of the pointer beside each load would put the load in a basic
// block of its own, and a wait with it).
template <bool HAS_VALID>
__global__ __launch_bounds__(plan::kConsistencyBlock) void k12_view_consistency(ConsistencyArgs a)
{
    constexpr int B = plan::kConsistencyBatch;
    const int row_blocks = a.S * a.nseg;
    int s, v, seg;
    if (a.order == kConsistencyOrderPlanes) {
        const int lb = (int)blockIdx.x;
        if (lb >= a.V * row_blocks)
            return;
        s = lb / (a.V * a.nseg);
        const int r = lb - s * (a.V * a.nseg);
        v = r / a.nseg;
        seg = r - v * a.nseg;
    } else {
        const int lb = a.order == kConsistencyOrderXcdRows ? xcd_logical_block_rows((int)blockIdx.x, row_blocks) : (int)blockIdx.x;
        v = lb / row_blocks;
        if (v >= a.V)
            return;   // the surplus blocks of a launch rounded up to eight scanlines
        const int r = lb - v * row_blocks;
        s = r / a.nseg;
        seg = r - s * a.nseg;
    }
    const int u = seg * plan::kConsistencyBlock + (int)threadIdx.x;
    const bool inside = u < a.U;
    const int uc = inside ? u : a.U - 1;
    const long long plane = (long long)a.V * a.U;
    const long long row = (long long)v * a.U;
    const long long o = (long long)s * plane + row + uc;
    const float d = a.depth[o];
    const uint8_t vb = HAS_VALID ? a.valid[o] : (uint8_t)255;
    const bool ok = inside && consistency_ok(d, vb);
    // a segment without an ok pixel (an invalid region, a band a mask left out) asks nobody: workgroup-uniform, and no
    // barrier follows
    if (!__syncthreads_or(ok ? 1 : 0)) {
        if (inside)
            consistency_store(a, o, consistency_nothing());
        return;
    }
    ConsistencyAcc acc = consistency_start(d);
    int t0, t1;
    consistency_window(s, a.S, a.radius, &t0, &t1);   // workgroup-uniform: with a radius, 2 * radius + 1 rows at the most
    for (int tb = t0; tb <= t1; tb += B) {
        bool live[B];
        float dt[B];
        uint8_t vt[B];
#pragma unroll
        for (int j = 0; j < B; j++) {
            const int t = tb + j;
            int x = uc;
            const bool in_field = consistency_column(consistency_offset(d, s, t, a.slope), u, a.U, &x);
            live[j] = ok & (t <= t1) & (t != s) & in_field;
            // (a lane without a target in view t reads its own column: the line its neighbours read)
            const long long q = (long long)(t <= t1 ? t : t1) * plane + row + (live[j] ? x : uc);
            dt[j] = a.depth[q];
            vt[j] = HAS_VALID ? a.valid[q] : (uint8_t)255;
        }
#pragma unroll
        for (int j = 0; j < B; j++)
            consistency_visit(&acc, live[j], d, dt[j], consistency_ok(dt[j], vt[j]), a.tol);
    }
    if (inside)
        consistency_store(a, o, ok ? consistency_finish(acc, a.min_agree) : consistency_nothing());
}

}  // namespace rslf
