// K14: the view warp (rslf_view_warp).  Not in the reference: what a view position t looks like given the disparity planes of
// every other view -- a scatter with an occlusion order, where K12 (k12_consistency.hpp) is a gather along a pixel's own line.
// The per-pixel rule is k14_warp_rule.hpp, the one statement the host tests compile too; this file is how the device walks it.
//
// One workgroup of 256 threads per (target, scanline).  Its z-buffer is one 64-bit key per column in dynamic LDS (and, only in
// the COUNT instantiation, one dword per column of candidate counts).  The workgroup clears it, then walks the source views of
// its window in rank order (warp_walk_*: the loop counter is the rank the key carries), each row in strides of 256 columns,
// kWarpBatch strides at a time: the loads of a batch -- disparity and validity byte, coalesced -- are issued UNCONDITIONALLY at a
// column clamped into the row, before the first test (k4_propagate.hpp and profiles/r19_consistency.md record what a load under
// `if` costs with this compiler: a basic block, and a wait, of its own).  Each candidate ends in one atomicMax on its column's
// key.  Where the disparity is locally constant consecutive lanes hit consecutive columns, and a wave's 64-bit LDS atomics
// fall on distinct banks.  After ONE barrier a second pass decodes each winner -- view and z out of the key, the source column
// recomputed (warp_source_column) -- and writes the planes, four columns per thread where the alignment allows; it gathers
// the colour from the slab, forms err against the slab's own row (v, t) and reduces a row's sums through wave shuffles and
// 48 bytes of LDS: a row has one owner, so there is no global atomic.
//
// Grid: ordered by scanline, the scanlines dealt to the XCDs in turn (xcd_logical_block_rows), the T targets of a scanline
// adjacent: the S source rows of a scanline (S * U * 5 bytes, 0.97 MB at 1920 x 101) come from HBM once and serve all the
// targets from one L2.  Placement only affects speed.
//
// Every index into LDS and every conversion to int sits behind consistency_column's guards (warp_candidate,
// warp_source_column): no input value -- NaN, +-inf, 1e30, a huge slope -- reaches an address.
#pragma once

#include "k14_warp_rule.hpp"
#include "rslf_device.hpp"
#include "rslf_plan_warp.hpp"

namespace rslf {

struct WarpArgs {
    const float* depth;     // [S][V][U]
    const uint8_t* valid;   // [S][V][U], nullable
    int S, V, U;
    float slope;
    int radius, nearer;
    int T;                  // the targets of THIS launch
    int k_first;            // ... whose planes start at target k_first of the call's
    int vec;                // 16-byte stores: U is a multiple of four and every plane asked for is 16-byte aligned
    VolView vol;            // base NULL: no volume
    uint8_t* hit;           // [T][V][U] each, nullable
    float* out_depth;
    int32_t* src_view;
    int32_t* src_col;
    int32_t* count;         // (non-NULL exactly in the COUNT instantiations)
    float* colour;          // [T][V][U][C]
    float* err;
    double* row_err;        // [T][V]
    int32_t* row_hits;
    float target[plan::kWarpLaunchTargets];
    int32_t exclude[plan::kWarpLaunchTargets];
};

// What the second pass knows of one target column.
struct WarpPixel {
    int hit;   // 0 / 1
    int32_t s, u;
    float d, err;
    int32_t count;
};

template <typename T4, typename T>
__device__ __forceinline__ void warp_store4(T* plane, long long o, const T (&x)[4], int n, bool vec)
{
    if (!plane)
        return;
    if (vec) {
        T4 q;
        q.x = x[0], q.y = x[1], q.z = x[2], q.w = x[3];
        *reinterpret_cast<T4*>(plane + o) = q;
    } else {
        for (int j = 0; j < n; j++)
            plane[o + j] = x[j];
    }
}

// HAS_VALID = false: a.valid is NULL and never read; COUNT = false: no count array in LDS, a.count NULL.
template <bool HAS_VALID, bool COUNT>
__global__ __launch_bounds__(plan::kWarpBlock) void k14_view_warp(WarpArgs a)
{
    constexpr int B = plan::kWarpBatch, W = plan::kWarpBlock;
    extern __shared__ unsigned long long s_warp_keys[];   // [U] keys | COUNT: [U] dwords
    uint32_t* const s_count = reinterpret_cast<uint32_t*>(s_warp_keys + a.U);
    __shared__ double s_row_err[W / kWave];
    __shared__ int s_row_hits[W / kWave];
    const int lb = xcd_logical_block_rows((int)blockIdx.x, a.T);
    const int v = lb / a.T;
    if (v >= a.V)
        return;   // the surplus blocks of a launch rounded up to eight scanlines
    const int k = lb - v * a.T;
    const int tid = (int)threadIdx.x;
    const float t = a.target[k];
    const int exclude = a.exclude[k];
    const int U = a.U;
    const long long plane = (long long)a.V * U, row = (long long)v * U;

    for (int u = tid; u < U; u += W) {
        s_warp_keys[u] = 0ull;
        if (COUNT)
            s_count[u] = 0u;
    }
    __syncthreads();

    WarpWalk walk = warp_walk_start(t, a.S);   // workgroup-uniform
    int s = 0, rank = 0;
    while (warp_walk_next(&walk, t, a.S, &s)) {
        const int r = rank++;
        if (!warp_in_window(s, t, a.radius))
            break;   // the walk leaves t: every later view is farther
        if (s == exclude)
            continue;
        const float* const drow = a.depth + (long long)s * plane + row;
        const uint8_t* const vrow = HAS_VALID ? a.valid + (long long)s * plane + row : nullptr;
        for (int u0 = 0; u0 < U; u0 += W * B) {
            float d[B];
            uint8_t vb[B];
#pragma unroll
            for (int j = 0; j < B; j++) {
                const int u = u0 + j * W + tid;
                const int uc = u < U ? u : U - 1;
                d[j] = drow[uc];
                vb[j] = HAS_VALID ? vrow[uc] : (uint8_t)255;
            }
#pragma unroll
            for (int j = 0; j < B; j++) {
                const int u = u0 + j * W + tid;
                int x = 0;
                if (u < U && warp_candidate(d[j], vb[j], s, u, U, t, exclude, a.radius, a.slope, &x)) {   // x in [0, U)
                    atomicMax(&s_warp_keys[x], warp_key(warp_z(d[j], a.nearer), r, s));
                    if (COUNT)
                        atomicAdd(&s_count[x], 1u);
                }
            }
        }
    }
    __syncthreads();

    const bool want_vol = a.vol.base != nullptr && (a.colour || a.err || a.row_err);
    const int C = a.vol.C;
    int tv = (int)t;   // |t| <= 65536; the slab's own row, read only for err (t is then a view)
    tv = tv < 0 ? 0 : tv >= a.S ? a.S - 1 : tv;
    const bool want_err = a.vol.base != nullptr && (a.err || a.row_err);
    const float* const lrow = want_err ? a.vol.row(v, tv) : nullptr;
    const long long out_row = ((long long)(a.k_first + k) * a.V + v) * U;
    double esum = 0.0;
    int nhit = 0;
    for (int q = tid; 4 * q < U; q += W) {
        const int n = U - 4 * q < 4 ? U - 4 * q : 4;
        uint8_t hit[4];
        float dd[4], ee[4];
        int32_t ss[4], uu[4], cc[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int x = 4 * q + j;
            const unsigned long long key = j < n ? s_warp_keys[x] : 0ull;
            hit[j] = key ? 255 : 0;
            ss[j] = uu[j] = -1;
            dd[j] = ee[j] = 0.0f;
            cc[j] = COUNT && j < n ? (int32_t)s_count[x] : 0;
            if (key) {
                int sv = warp_key_view(key);
                sv = sv < a.S ? sv : a.S - 1;
                const int su = warp_source_column(key, x, U, t, a.nearer, a.slope);
                ss[j] = sv, uu[j] = su;
                dd[j] = a.depth[(long long)sv * plane + row + su];   // the winner's stored disparity, its own bits
                nhit++;
                if (want_vol) {
                    const float* const src = a.vol.row(v, sv) + (long long)su * C;
                    if (a.colour) {
                        float* const dst = a.colour + (out_row + x) * C;
                        for (int c = 0; c < C; c++)
                            dst[c] = src[c];
                    }
                    if (want_err) {
                        ee[j] = warp_residual(src, lrow + (long long)x * C, C);
                        esum += (double)ee[j];
                    }
                }
            } else if (j < n && a.colour && want_vol) {
                float* const dst = a.colour + (out_row + x) * C;
                for (int c = 0; c < C; c++)
                    dst[c] = 0.0f;
            }
        }
        const long long o = out_row + 4 * q;
        const bool vec = a.vec != 0;
        if (a.hit) {
            if (vec)
                *reinterpret_cast<uint32_t*>(a.hit + o) = (uint32_t)hit[0] | (uint32_t)hit[1] << 8 | (uint32_t)hit[2] << 16 | (uint32_t)hit[3] << 24;
            else
                for (int j = 0; j < n; j++)
                    a.hit[o + j] = hit[j];
        }
        warp_store4<float4>(a.out_depth, o, dd, n, vec);
        warp_store4<int4>(a.src_view, o, ss, n, vec);
        warp_store4<int4>(a.src_col, o, uu, n, vec);
        if (COUNT)
            warp_store4<int4>(a.count, o, cc, n, vec);
        warp_store4<float4>(a.err, o, ee, n, vec);
    }
    if (a.row_err || a.row_hits) {   // workgroup-uniform
        for (int o = kWave / 2; o > 0; o >>= 1) {
            esum += __shfl_xor(esum, o);
            nhit += __shfl_xor(nhit, o);
        }
        if ((tid & (kWave - 1)) == 0) {
            s_row_err[tid / kWave] = esum;
            s_row_hits[tid / kWave] = nhit;
        }
        __syncthreads();
        if (tid == 0) {
            const long long o = (long long)(a.k_first + k) * a.V + v;
            if (a.row_err)
                a.row_err[o] = (s_row_err[0] + s_row_err[1]) + (s_row_err[2] + s_row_err[3]);
            if (a.row_hits)
                a.row_hits[o] = (s_row_hits[0] + s_row_hits[1]) + (s_row_hits[2] + s_row_hits[3]);
        }
    }
}

}  // namespace rslf
