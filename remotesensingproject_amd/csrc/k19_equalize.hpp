// K19: the per-view equalisation (rslf_volume_view_stats, rslf_view_stats_dense, rslf_volume_equalize_views,
// rslf_volume_apply_view_gains, rslf_equalize_views_dense).  The rule is k19_equalize_rule.hpp; rows, lanes, tiles and grids
// are rslf_plan_equalize.hpp's.  Both kernels touch every float once and compute next to nothing: memory-bound.
//
// Two forms share each body:
//   volume form (pitch > 0): a filled slab [V][S][pitch][C], rows start at multiples of 256 bytes, so a row is all body;
//     the pixels at and beyond U are the pad: never counted, written as zeros;
//   dense form (pitch == 0): [V][S][U][C], only 4-byte aligned: up to three pixels at each end of a row are peeled and done
//     one by one by tile 0 of the row (plan::equalize_row_dense).
// A lane owns four consecutive pixels of the body, 4 C floats as C loads of 16 bytes, so the channel of a float is a
// compile-time fact of its register (plan::equalize_float_channel).
//
// k19_view_stats<C>: per view s and channel c the integers (n, s1, s2) of the rule.  A workgroup walks rows of ONE view at a
// time (plan::equalize_stats_grid); a lane accumulates in 64-bit integers (q^2 < 2^32: two samples already overflow 32 bits);
// the sums are reduced across the wave by shuffles, across the workgroup through LDS, and the workgroup adds its totals
// to the zeroed [S][C][3] buffer with one 64-bit integer atomic add per total.  Integer adds commute: the same bits on
// every run.  No floating-point atomic anywhere.
//
// k19_equalize_apply<C, INTEGER>: y = eq_apply(x, a[s][c], b[s][c], hi), 16-byte loads and stores; a lane reads its floats
// before it writes them and no other lane touches them, so the dense form may run in place.  With `partial` set every
// workgroup leaves the minimum and maximum of the floats it wrote below U there, as K0's rows do, for k0_minmax_final.
#pragma once

#include <hip/hip_runtime.h>

#include "k19_equalize_rule.hpp"
#include "rslf_plan_equalize.hpp"

namespace rslf {

struct EqualizeStatsArgs {
    const float* src;
    unsigned long long* stats;   // [S][C][3], zeroed before the launch
    int V, S, U;
    int row_px;                  // pixels from a row to the next: the pitch, or U
    int pitch;                   // the volume form's pitch; 0: the dense form
    int base_aligned;            // dense form: src is 16-byte aligned
    int tiles_per_row;
    int per_view, groups;        // plan::EqualizeStatsGrid
    float hi, k;                 // the cap and eq_quant_scale(hi)
};

struct EqualizeApplyArgs {
    const float* src;
    float* dst;                  // the dense form: may be src
    const float* a_b;            // [S][C][2]
    float* partial;              // [2 * gridDim.x] (min, max) per workgroup, or NULL
    long long tiles;             // rows * tiles_per_row
    int tiles_per_row;
    int S, U;
    int row_px, pitch, base_aligned;   // as above; base_aligned: src and dst both
    float hi;
};

// The 4 C floats of a lane's group, as C loads / stores of 16 bytes.
template <int C>
__device__ inline void eq_load_group(const float* p, float (&f)[plan::kEqLane * C])
{
#pragma unroll
    for (int i = 0; i < C; i++) {
        const float4 x = reinterpret_cast<const float4*>(p)[i];
        f[4 * i] = x.x, f[4 * i + 1] = x.y, f[4 * i + 2] = x.z, f[4 * i + 3] = x.w;
    }
}
template <int C>
__device__ inline void eq_store_group(float* p, const float (&f)[plan::kEqLane * C])
{
#pragma unroll
    for (int i = 0; i < C; i++)
        reinterpret_cast<float4*>(p)[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
}

template <int C>
__global__ __launch_bounds__(plan::kEqBlock) void k19_view_stats(const EqualizeStatsArgs a)
{
    constexpr int kTotals = C * kEqStats;
    __shared__ unsigned long long red[plan::kEqBlock / 64][kTotals];
    const int tid = (int)threadIdx.x;
    const int U = a.U;
    const plan::EqualizeStatsGrid g = {a.per_view, a.groups};
    const int member = plan::equalize_stats_member(g, blockIdx.x);
    const long long items = (long long)a.V * a.tiles_per_row;
    for (int s = plan::equalize_stats_team(g, blockIdx.x); s < a.S; s += a.groups) {   // (the same for the whole workgroup)
        uint64_t acc[C][kEqStats];
#pragma unroll
        for (int c = 0; c < C; c++)
            acc[c][0] = acc[c][1] = acc[c][2] = 0;
        for (long long i = member; i < items; i += a.per_view) {
            const int v = (int)(i / a.tiles_per_row), t = (int)(i - (long long)v * a.tiles_per_row);
            const long long row = (long long)v * a.S + s;
            const plan::EqualizeRow r = a.pitch ? plan::equalize_row_volume(a.pitch) : plan::equalize_row_dense(row * U, U, a.base_aligned != 0);
            if (!plan::equalize_tile_works(r, t))
                continue;
            const float* __restrict__ src = a.src + row * a.row_px * C;
            const int p0 = plan::equalize_lane_first(r, t, tid);
            if (plan::equalize_lane_works(r, p0) && p0 < U) {   // (p0 >= U: a group of the volume form's pad)
                float f[plan::kEqLane * C];
                eq_load_group<C>(&src[(long long)p0 * C], f);
#pragma unroll
                for (int j = 0; j < plan::kEqLane * C; j++) {
                    const int c = plan::equalize_float_channel(j, C);
                    if (p0 + plan::equalize_float_pixel(j, C) < U)
                        eq_count(f[j], a.hi, a.k, &acc[c][0], &acc[c][1], &acc[c][2]);
                }
            }
            if (t == 0) {   // the row's peeled ends, one pixel at a time (dense form)
                for (int k = tid; k < plan::equalize_peeled(r); k += plan::kEqBlock) {
                    const int p = plan::equalize_peeled_pixel(r, k);
#pragma unroll
                    for (int c = 0; c < C; c++)
                        eq_count(src[(long long)p * C + c], a.hi, a.k, &acc[c][0], &acc[c][1], &acc[c][2]);
                }
            }
        }
        // the wave, then the workgroup, then one atomic add per total
#pragma unroll
        for (int c = 0; c < C; c++) {
#pragma unroll
            for (int i = 0; i < kEqStats; i++) {
                unsigned long long x = acc[c][i];
                for (int o = 32; o > 0; o >>= 1)
                    x += __shfl_xor(x, o);
                if ((tid & 63) == 0)
                    red[tid >> 6][c * kEqStats + i] = x;
            }
        }
        __syncthreads();
        if (tid < kTotals) {
            unsigned long long x = red[0][tid];
            for (int w = 1; w < plan::kEqBlock / 64; w++)
                x += red[w][tid];
            if (x)
                atomicAdd(&a.stats[(long long)s * kTotals + tid], x);
        }
        __syncthreads();   // (the next view's totals go through the same LDS)
    }
}

struct EqualizeRange {
    float mn, mx;
    __device__ void take(float x)
    {
        mn = (x != x) ? -INFINITY : fminf(mn, x);   // (as K0: a NaN sends the scan to the generic kernel)
        mx = fmaxf(mx, x);
    }
};

template <int C, bool INTEGER>
__global__ __launch_bounds__(plan::kEqBlock) void k19_equalize_apply(const EqualizeApplyArgs a)
{
    __shared__ float smn[plan::kEqBlock / 64], smx[plan::kEqBlock / 64];
    const int tid = (int)threadIdx.x;
    const int U = a.U;
    EqualizeRange range = {INFINITY, -INFINITY};
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long row = tile / a.tiles_per_row;
        const int t = (int)(tile - row * a.tiles_per_row);
        const plan::EqualizeRow r = a.pitch ? plan::equalize_row_volume(a.pitch) : plan::equalize_row_dense(row * U, U, a.base_aligned != 0);
        if (!plan::equalize_tile_works(r, t))   // (the same for the whole workgroup)
            continue;
        const int s = (int)(row % a.S);
        float ca[C], cb[C];
#pragma unroll
        for (int c = 0; c < C; c++) {
            ca[c] = a.a_b[((long long)s * C + c) * 2];
            cb[c] = a.a_b[((long long)s * C + c) * 2 + 1];
        }
        const float* src = a.src + row * a.row_px * C;   // (no __restrict__: the dense form may run in place)
        float* dst = a.dst + row * a.row_px * C;
        const int p0 = plan::equalize_lane_first(r, t, tid);
        if (plan::equalize_lane_works(r, p0)) {
            float f[plan::kEqLane * C];
            if (p0 < U) {
                eq_load_group<C>(&src[(long long)p0 * C], f);
#pragma unroll
                for (int j = 0; j < plan::kEqLane * C; j++) {
                    const int c = plan::equalize_float_channel(j, C);
                    if (p0 + plan::equalize_float_pixel(j, C) < U) {
                        f[j] = eq_apply<INTEGER>(f[j], ca[c], cb[c], a.hi);
                        range.take(f[j]);
                    } else {
                        f[j] = 0.0f;   // the pad
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < plan::kEqLane * C; j++)
                    f[j] = 0.0f;
            }
            eq_store_group<C>(&dst[(long long)p0 * C], f);
        }
        if (t == 0) {   // the row's peeled ends, one pixel at a time (dense form)
            for (int k = tid; k < plan::equalize_peeled(r); k += plan::kEqBlock) {
                const int p = plan::equalize_peeled_pixel(r, k);
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const float y = eq_apply<INTEGER>(src[(long long)p * C + c], ca[c], cb[c], a.hi);
                    range.take(y);
                    dst[(long long)p * C + c] = y;
                }
            }
        }
    }
    if (!a.partial)   // (the same for the whole grid)
        return;
    for (int o = 32; o > 0; o >>= 1) {
        range.mn = fminf(range.mn, __shfl_xor(range.mn, o));
        range.mx = fmaxf(range.mx, __shfl_xor(range.mx, o));
    }
    if ((tid & 63) == 0) {
        smn[tid >> 6] = range.mn;
        smx[tid >> 6] = range.mx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < plan::kEqBlock / 64; i++) {
            range.mn = fminf(range.mn, smn[i]);
            range.mx = fmaxf(range.mx, smx[i]);
        }
        a.partial[2 * blockIdx.x] = range.mn;
        a.partial[2 * blockIdx.x + 1] = range.mx;
    }
}

}  // namespace rslf
