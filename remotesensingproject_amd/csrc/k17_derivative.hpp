// K17: the derivative channels (rslf_volume_derivative_channels, rslf_derivative_channels_dense).  The rule is
// k17_derivative_rule.hpp; rows, tiles, stage and grid are rslf_plan_derivative.hpp's.
//
// k17_derivative_channels<INTEGER>: a one-channel field x[V][S][row_in] becomes (x, fu, fv)[V][S][3 * row_in].  The kernel
// reads the source once from memory (the rows v - 1 and v + 1 are other workgroups' rows and mostly come from the caches)
// and writes three times as much: memory-bound.  Two forms share the body:
//   volume form (pitch > 0): rows are `pitch` columns long, pad included, and start at multiples of 256 bytes, so a row is
//     all body; the floats at and beyond 3 * U of every output row are written as zeros: the scan kernels rely on them;
//   raw form (pitch == 0): rows are U columns, dense, only 4-byte aligned: up to three columns at each end of a row are
//     peeled and done one by one by tile 0 of the row (plan::derivative_row_raw).
// A lane owns four consecutive columns of the body: one 16-byte load, and their twelve floats leave as three consecutive
// 16-byte stores (a wave's stores are one 3 KiB run).  The u - 1 and u + 1 neighbours inside the group are the lane's own
// registers; the column before the group and the column after come from an LDS stage of the row tile, with a halo of one
// column at each end, clamped to the row (two stages taken in turn, so a tile costs one barrier).  The rows v - 1 and
// v + 1 (clamped) are read from memory, S * row_in floats away, in the same breath as the row itself: as 16 bytes where
// that distance keeps the alignment, else as four floats.  The grid is capped (plan::kDerivGridCap) and strides over the
// tiles.  With `partial` set, every workgroup leaves the minimum and maximum of the floats it wrote below 3 * U there, as
// K0's rows do, for k0_minmax_final.
#pragma once

#include <hip/hip_runtime.h>

#include "k17_derivative_rule.hpp"
#include "rslf_plan_derivative.hpp"

namespace rslf {

struct DerivativeArgs {
    const float* src;
    float* dst;
    float* partial;            // [2 * gridDim.x] (min, max) per workgroup, or NULL
    long long tiles;           // rows * tiles_per_row
    int tiles_per_row;
    int V, S, U;
    int row_in;                // floats from a source row to the next: the pitch, or U; the output's is three times that
    int pitch;                 // the volume form's pitch; 0: the raw form
    int bases_aligned;         // raw form: src and dst are 16-byte aligned
    int v_aligned;             // S * row_in is a multiple of 4: the rows v - 1 and v + 1 are aligned as the row itself is
    float h, hi;               // derivative_half_weight(weight), the cap
};

struct DerivativeRange {
    float mn, mx;
    __device__ void take(float x)
    {
        mn = (x != x) ? -INFINITY : fminf(mn, x);   // (as K0: a NaN sends the scan to the generic kernel)
        mx = fmaxf(mx, x);
    }
};

template <bool INTEGER>
__global__ __launch_bounds__(plan::kDerivBlock) void k17_derivative_channels(const DerivativeArgs a)
{
    __shared__ __attribute__((aligned(16))) float stage[2][plan::kDerivStage];   // two, in turn: one barrier per tile
    __shared__ float smn[plan::kDerivBlock / 64], smx[plan::kDerivBlock / 64];
    const int tid = (int)threadIdx.x;
    const int U = a.U;
    DerivativeRange range = {INFINITY, -INFINITY};
    int turn = 0;
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long row = tile / a.tiles_per_row;
        const int t = (int)(tile - row * a.tiles_per_row);
        const plan::DerivativeRow r = a.pitch ? plan::derivative_row_volume(a.pitch) : plan::derivative_row_raw(row * U, U, a.bases_aligned != 0);
        if (!plan::derivative_tile_works(r, t))   // (the same for the whole workgroup)
            continue;
        const int v = (int)(row / a.S), s = (int)(row - (long long)v * a.S);
        const float* __restrict__ src = a.src + row * a.row_in;
        const float* __restrict__ below = a.src + ((long long)derivative_left(v) * a.S + s) * a.row_in;       // row v - 1, clamped
        const float* __restrict__ above = a.src + ((long long)derivative_right(v, a.V) * a.S + s) * a.row_in;  // row v + 1, clamped
        float* __restrict__ dst = a.dst + row * a.row_in * kDerivativeChannels;
        const int c0 = plan::derivative_tile_first(r, t);
        const int end = plan::derivative_stage_end(r, c0);   // one past the tile's last body column
        const int u0 = c0 + plan::kDerivLane * tid;
        const bool mine = u0 < end;                            // the group lies inside the body, all four columns
        // the tile before this one read the other stage; the tile before that read this one, and every lane has passed
        // the barrier that followed it
        float* const seg = stage[turn];
        turn ^= 1;
        float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f), dn = x, up = x;
        if (mine) {   // the three loads leave together; the rows v - 1 and v + 1 are not needed before the barrier
            x = *reinterpret_cast<const float4*>(&src[u0]);
            if (a.v_aligned) {
                dn = *reinterpret_cast<const float4*>(&below[u0]);
                up = *reinterpret_cast<const float4*>(&above[u0]);
            } else {
                dn = make_float4(below[u0], below[u0 + 1], below[u0 + 2], below[u0 + 3]);
                up = make_float4(above[u0], above[u0 + 1], above[u0 + 2], above[u0 + 3]);
            }
            *reinterpret_cast<float4*>(&seg[plan::derivative_stage_index(u0, c0)]) = x;
        }
        if (tid == 0)
            seg[plan::derivative_stage_index(c0 - 1, c0)] = src[derivative_left(c0)];
        if (tid == plan::kDerivBlock - 1)
            seg[plan::derivative_stage_index(end, c0)] = src[end < U ? end : U - 1];
        __syncthreads();
        if (mine) {
            const float own[4] = {x.x, x.y, x.z, x.w};
            const float vdn[4] = {dn.x, dn.y, dn.z, dn.w};
            const float vup[4] = {up.x, up.y, up.z, up.w};
            // the column before the group and the column after; read only where the rule asks for them
            const float before = u0 < U ? seg[plan::derivative_stage_index(derivative_left(u0), c0)] : 0.0f;
            const float after = u0 + plan::kDerivLane < U ? seg[plan::derivative_stage_index(u0 + plan::kDerivLane, c0)] : 0.0f;
            float o[plan::kDerivLane * kDerivativeChannels];
#pragma unroll
            for (int k = 0; k < plan::kDerivLane; k++) {
                const int u = u0 + k;
                float c = 0.0f, fu = 0.0f, fv = 0.0f;   // the pad
                if (u < U) {
                    const float left = k > 0 ? own[k > 0 ? k - 1 : 0] : before;
                    const float right = u + 1 < U ? (k < plan::kDerivLane - 1 ? own[k < plan::kDerivLane - 1 ? k + 1 : k] : after) : own[k];
                    c = own[k];
                    fu = derivative_feature<INTEGER>(right, left, a.h, a.hi);
                    fv = derivative_feature<INTEGER>(vup[k], vdn[k], a.h, a.hi);
                    range.take(c);
                    range.take(fu);
                    range.take(fv);
                }
                o[3 * k] = c, o[3 * k + 1] = fu, o[3 * k + 2] = fv;
            }
            float4* out = reinterpret_cast<float4*>(&dst[(long long)kDerivativeChannels * u0]);
            out[0] = make_float4(o[0], o[1], o[2], o[3]);
            out[1] = make_float4(o[4], o[5], o[6], o[7]);
            out[2] = make_float4(o[8], o[9], o[10], o[11]);
        }
        if (t == 0) {   // the row's peeled ends, one column at a time (raw form)
            for (int k = tid; k < plan::derivative_peeled(r); k += plan::kDerivBlock) {
                const int u = plan::derivative_peeled_column(r, k);
                const float c = src[u];
                const float fu = derivative_feature<INTEGER>(src[derivative_right(u, U)], src[derivative_left(u)], a.h, a.hi);
                const float fv = derivative_feature<INTEGER>(above[u], below[u], a.h, a.hi);
                range.take(c);
                range.take(fu);
                range.take(fv);
                float* out = &dst[(long long)kDerivativeChannels * u];
                out[0] = c, out[1] = fu, out[2] = fv;
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
        for (int i = 1; i < plan::kDerivBlock / 64; i++) {
            range.mn = fminf(range.mn, smn[i]);
            range.mx = fmaxf(range.mx, smx[i]);
        }
        a.partial[2 * blockIdx.x] = range.mn;
        a.partial[2 * blockIdx.x + 1] = range.mx;
    }
}

}  // namespace rslf
