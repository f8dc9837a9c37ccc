// K16: the dilation of a volume along u by an integer factor (rslf_volume_dilate_u), and the way back for result planes
// (rslf_planes_undilate_u).  The rule is k16_dilate_rule.hpp; tile, stage and grid are rslf_plan_dilate.hpp's.
//
// k16_dilate_u<TAPS, C>: the source slab [V][S][pitch][C] becomes [V][S][pitch'][C].  The kernel moves (1 + f) times the
// source's bytes and does TAPS multiply-adds per sample: memory-bound.  A row is taken as its pitch' * C flattened floats,
// pad included; a workgroup owns a tile of 1024 of them and each lane writes four consecutive ones with one 16-byte store
// (rows start at multiples of 256 bytes, so every store is aligned and a wave's stores are one 1 KiB run).  The source
// floats the tile reads -- its columns divided by f, plus the taps' halo, clamped to the row -- are staged in LDS with
// 16-byte loads, so each source byte crosses the memory system once per tile and the TAPS reads per sample are LDS reads.
// The weight rows travel in the kernel's arguments and are copied to LDS once per workgroup: a lane's phase picks its row.
// Floats at and beyond U' * C are written as zeros: the scan kernels rely on the zero pad.  The grid is capped
// (plan::kDilateGridCap) and strides over the tiles.
#pragma once

#include <hip/hip_runtime.h>

#include "k16_dilate_rule.hpp"
#include "rslf_plan_dilate.hpp"

namespace rslf {

struct DilateArgs {
    const float* src;
    float* dst;
    long long tiles;           // rows * tiles_per_row
    int tiles_per_row;
    int row_in, row_out;       // floats of a source row (pitch * C) and of an output row (pitch' * C): multiples of 64
    int U, U_out, f;
    float lo, hi;              // the source volume's min and max
    DilateWeights wt;
};

template <int TAPS, int C>
__global__ __launch_bounds__(plan::kDilateBlock) void k16_dilate_u(const DilateArgs a)
{
    __shared__ __attribute__((aligned(16))) float seg[plan::kDilateStage];
    __shared__ float wsh[kDilateMaxFactor * kDilateMaxTaps];
    const int tid = (int)threadIdx.x;
    if (tid < kDilateMaxFactor * kDilateMaxTaps)
        wsh[tid] = a.wt.w[tid / kDilateMaxTaps][tid % kDilateMaxTaps];
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long row = tile / a.tiles_per_row;
        const int t = (int)(tile - row * a.tiles_per_row);
        const float* __restrict__ src = a.src + row * a.row_in;
        float* __restrict__ dst = a.dst + row * a.row_out;
        const int e0 = t * plan::kDilateTile;
        // the source segment of the tile: at most plan::kDilateStage floats (test_plan_dilate.cpp)
        const DilateStage stage = dilate_stage(e0, plan::kDilateTile, a.U, a.U_out, C, a.f, TAPS, a.row_in);
        const int first = stage.first;
        for (int k = 4 * tid; k < stage.count; k += 4 * plan::kDilateBlock)
            *reinterpret_cast<float4*>(&seg[k]) = *reinterpret_cast<const float4*>(&src[first + k]);
        __syncthreads();   // (also orders wsh before its first read)
        const int e = e0 + 4 * tid;
        if (e < a.row_out) {   // row_out is a multiple of 4: the lane's four floats are inside the row or all outside
            int j = e / C, c = e - j * C;
            int i = j / a.f, p = j - i * a.f;
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float v = 0.0f;   // the pad
                if (j < a.U_out) {
                    if (p == 0)
                        v = seg[i * C + c - first];
                    else
                        v = dilate_range(dilate_sum<TAPS>(seg, C, c - first, i, a.U, &wsh[p * kDilateMaxTaps]), a.lo, a.hi);
                }
                o[k] = v;
                if (++c == C) {
                    c = 0;
                    ++j;
                    if (++p == a.f) {
                        p = 0;
                        ++i;
                    }
                }
            }
            *reinterpret_cast<float4*>(&dst[e]) = make_float4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();   // the next tile's stage overwrites seg
    }
}

// out[r][u] = in[r][u * f]: a result plane of the dilated frame on the source grid.  Planes of 1-byte or 4-byte elements.
template <typename E>
__global__ __launch_bounds__(plan::kDilateBlock) void k16_undilate_u(const E* __restrict__ in, E* __restrict__ out, size_t rows, int U_dilated,
                                                                      int U, int f)
{
    const int u = (int)(blockIdx.x * plan::kDilateBlock + threadIdx.x);
    if (u >= U)
        return;
    for (size_t r = blockIdx.y; r < rows; r += gridDim.y)
        out[r * (size_t)U + u] = in[r * (size_t)U_dilated + (size_t)u * f];
}

}  // namespace rslf
