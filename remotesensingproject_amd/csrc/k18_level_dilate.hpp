// K18: what a fine-to-coarse level needs around a sweep that runs in a frame dilated along u (the level dilation,
// rslf_f2c.hip): the level's per-pixel ranges into the dilated frame, and the sweep's result planes back out of it.  The
// rule is k18_ranges_rule.hpp; the grids are rslf_plan_level_dilate.hpp's.  Both kernels stream: no LDS, no scratch.
//
// k18_dilate_ranges: the planes dmin, dmax [rows][U] become [rows][U'], both in one launch.  The kernel reads 2 * U floats
// of a row and writes 2 * U' = 2 * (f (U - 1) + 1): memory-bound, the stores f times the loads, so the stores are the ones
// made wide.  The planes are dense, so row r starts (r * U') % 4 floats past a 16-byte boundary; a lane owns the store group
// g of its row -- the four columns [4 g - a, 4 g - a + 4) with a that offset -- which makes every whole group one aligned
// 16-byte store and a wave's groups one 1 KiB run.  The groups cut by a row's two ends go out one float at a time, and so
// does everything when an output plane does not itself start on a 16-byte boundary (vec == 0).  The loads are one float each: a
// lane's four columns read at most 4 / f + 2 neighbouring floats, which the wave shares through the L1.  grid.y is capped
// and strides over the rows.
//
// k18_undilate_many: out[r][u] = in[r][u * f] for up to eight planes of 4-byte elements and two of 1-byte elements in one
// launch, the pointers in the kernel's arguments, blockIdx.z the plane.  A level's sweep leaves seven planes to bring
// back; k16_undilate_u would take a launch each.  The loads have stride f by their nature; the stores are a wave's 256
// (or 64) consecutive bytes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k18_ranges_rule.hpp"
#include "rslf_plan_level_dilate.hpp"

namespace rslf {

__global__ __launch_bounds__(plan::kDilateBlock) void k18_dilate_ranges(const float* __restrict__ dmin, const float* __restrict__ dmax,
                                                                         size_t rows, int U, int U_dilated, int f, int vec,
                                                                         float* __restrict__ out_min, float* __restrict__ out_max)
{
    const long long g = (long long)blockIdx.x * plan::kDilateBlock + threadIdx.x;
    for (size_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const int a = vec ? (int)((r * (size_t)U_dilated) & 3u) : 0;
        const RangesSpan s = ranges_span(g, a, U_dilated);
        if (s.count == 0)
            continue;
        const float* __restrict__ lo = dmin + r * (size_t)U;
        const float* __restrict__ hi = dmax + r * (size_t)U;
        float* __restrict__ olo = out_min + r * (size_t)U_dilated + s.first;
        float* __restrict__ ohi = out_max + r * (size_t)U_dilated + s.first;
        int i, p;
        ranges_source(s.first, f, &i, &p);   // every column of the span is at most f * (U - 1): i <= U - 1, and i + 1 <= U - 1 where p > 0
        float vlo[4], vhi[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            vlo[k] = vhi[k] = 0.0f;
            if (k < s.count) {
                vlo[k] = p == 0 ? lo[i] : ranges_min(lo[i], lo[i + 1]);
                vhi[k] = p == 0 ? hi[i] : ranges_max(hi[i], hi[i + 1]);
                if (++p == f) {
                    p = 0;
                    ++i;
                }
            }
        }
        if (vec && s.count == 4) {
            *reinterpret_cast<float4*>(olo) = make_float4(vlo[0], vlo[1], vlo[2], vlo[3]);
            *reinterpret_cast<float4*>(ohi) = make_float4(vhi[0], vhi[1], vhi[2], vhi[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < s.count) {
                    olo[k] = vlo[k];
                    ohi[k] = vhi[k];
                }
        }
    }
}

struct UndilateManyArgs {
    const void* in[plan::kUndilateMany4 + plan::kUndilateMany1];   // the 4-byte planes first, then the 1-byte ones
    void* out[plan::kUndilateMany4 + plan::kUndilateMany1];
    int n4, n1;
    size_t rows;
    int U_dilated, U, f;
};

__global__ __launch_bounds__(plan::kDilateBlock) void k18_undilate_many(const UndilateManyArgs a)
{
    const int u = (int)(blockIdx.x * plan::kDilateBlock + threadIdx.x);
    if (u >= a.U)
        return;
    const int plane = (int)blockIdx.z;   // (uniform: the pointers are read from the arguments once per wave)
    const size_t col = (size_t)u * a.f;
    if (plane < a.n4) {
        const uint32_t* __restrict__ in = static_cast<const uint32_t*>(a.in[plane]);
        uint32_t* __restrict__ out = static_cast<uint32_t*>(a.out[plane]);
        for (size_t r = blockIdx.y; r < a.rows; r += gridDim.y)
            out[r * (size_t)a.U + u] = in[r * (size_t)a.U_dilated + col];
    } else {
        const uint8_t* __restrict__ in = static_cast<const uint8_t*>(a.in[plane]);
        uint8_t* __restrict__ out = static_cast<uint8_t*>(a.out[plane]);
        for (size_t r = blockIdx.y; r < a.rows; r += gridDim.y)
            out[r * (size_t)a.U + u] = in[r * (size_t)a.U_dilated + col];
    }
}

}  // namespace rslf
