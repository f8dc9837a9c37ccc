// K13: the gate form of the cross-view consistency check (rslf_f2c_consistency_mask) -- what a kept fine-to-coarse run puts on
// a level's validity between the level's sweep and the next level's ranges.  Not in the reference.  The per-pixel tests are
// K12's (k12_consistency_rule.hpp: ok, the column rule, tol, radius), the decision is consistency_gate, stated there once.
//
// The walk is k12_view_consistency's: one thread per pixel, one workgroup per 256-column segment of a (view, scanline) row, the
// grid ordered by scanline over the XCDs, the other views visited in batches of kConsistencyBatch with the sixteen loads of a
// batch issued unconditionally ahead of the first test, and the workgroup-uniform exit for a segment without an ok pixel.
// What differs:
//   * two counters per thread, seen and agree: no sum, no above, no below;
//   * the validity plane is required, and the gated byte goes to a SECOND plane -- a thread reads the other views' rows while
//     their workgroups write, so the output may not be the input;
//   * the agree / seen planes are optional;
//   * the pixels made invalid are counted: one ballot per wave, the four wave counts summed through LDS, and one 64-bit vector
//     atomic per workgroup that dropped something.
#pragma once

#include "k12_consistency.hpp"

namespace rslf {

struct F2cConsistencyArgs {
    const float* depth;      // [S][V][U]
    const uint8_t* valid;    // [S][V][U], required: the level's validity as the rule and the uniqueness ratio left it
    int S, V, U, nseg;
    float slope, tol;
    int radius, min_agree;
    int order;
    uint8_t* valid_out;      // [S][V][U], not `valid`
    int32_t* agree;          // [S][V][U] each, nullable
    int32_t* seen;
    unsigned long long* dropped;   // nullable: += the pixels this launch made invalid
};

__device__ __forceinline__ void f2c_consistency_store(const F2cConsistencyArgs& a, long long o, uint8_t byte, int32_t seen, int32_t agree)
{
    a.valid_out[o] = byte;
    if (a.agree)
        a.agree[o] = agree;
    if (a.seen)
        a.seen[o] = seen;
}

__global__ __launch_bounds__(plan::kConsistencyBlock) void k13_f2c_consistency_gate(F2cConsistencyArgs a)
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
    const uint8_t vb = a.valid[o];
    const bool ok = inside && consistency_ok(d, vb);
    // a segment without an ok pixel keeps its bytes (a non-zero byte on a non-finite disparity asks nobody and stays):
    // workgroup-uniform, before the counting barrier below
    if (!__syncthreads_or(ok ? 1 : 0)) {
        if (inside)
            f2c_consistency_store(a, o, vb, 0, 0);
        return;
    }
    int32_t seen = 0, agree = 0;
    int t0, t1;
    consistency_window(s, a.S, a.radius, &t0, &t1);   // workgroup-uniform
    // (one batch at a time: left to itself hipcc unrolls the batch loop of this kernel as well -- 256 VGPRs, one wave per
    // SIMD; rolled it takes 50)
#pragma unroll 1
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
            const long long q = (long long)(t <= t1 ? t : t1) * plane + row + (live[j] ? x : uc);
            dt[j] = a.depth[q];
            vt[j] = a.valid[q];
        }
#pragma unroll
        for (int j = 0; j < B; j++)
            consistency_gate_visit(&seen, &agree, live[j], d, dt[j], consistency_ok(dt[j], vt[j]), a.tol);
    }
    const bool drop = ok && !consistency_gate(seen, agree, a.min_agree);   // (ok: vb != 0)
    if (inside)
        f2c_consistency_store(a, o, drop ? (uint8_t)0 : vb, ok ? seen : 0, ok ? agree : 0);
    // every thread of the workgroup is here (the exit above is workgroup-uniform)
    __shared__ int s_n[plan::kConsistencyBlock / 64];
    const unsigned long long b = __ballot(drop);
    if ((threadIdx.x & 63) == 0)
        s_n[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0 && a.dropped) {
        int n = 0;
#pragma unroll
        for (int w = 0; w < plan::kConsistencyBlock / 64; w++)
            n += s_n[w];
        if (n)
            atomicAdd(a.dropped, (unsigned long long)n);
    }
}

}  // namespace rslf
