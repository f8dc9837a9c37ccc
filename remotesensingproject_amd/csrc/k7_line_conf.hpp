// K7: the line confidence C_l of the 2-D sweep.
//
// rslf::compute_2D_depth_epi under -D_USE_LINE_CONFIDENCE_SCORE (include/rslf_depth_computation_core.hpp:1032-1081):
// for the visited view s_hat and every scanline v,
//   I[s][u]  = (s_hat - s) * depth[v][u] + u                       :1054-1058   (no slope_factor here, as written)
//   E[s][u]  = max(Interpolation1DLinear(C_e[s][v][.], I[s][u]), 0) :1059-1071   (include/rslf_interpolation.hpp:155-193)
//   C_l[v][u] = sum_s E[s][u] K[v][s][u] / sum_s K[v][s][u]         :1074-1076, written under the edge mask only (:1079)
// K[v] is the K(r - rbar) column the scan leaves for the pixels it scanned and accepted (core.hpp:647-651); the buffer
// lives for the whole sweep (core.hpp:975-979), so a masked pixel that this visit did not scan reads what an earlier
// visit left there (zeros before any did).
//
// Work mapping: one workgroup per 256 columns of one scanline, lane = pixel, a sequential loop over s -- the two sums are
// the reference's float sums with s ascending, and nothing crosses lanes, so the bits do not depend on the launch shape.
// A pixel the visit scanned and accepted (arg-max index >= 0) first re-runs its winning hypothesis with the generic
// arithmetic (scan_generic_body: the same bits as every scan variant, what k2_kernel_column does) into its column of K.
// The kernel is bound by memory: per masked pixel the S floats of its column ([V][S][U]: coalesced along u) and two C_e
// taps per view -- neighbouring floats of one plane row wherever neighbouring pixels carry similar disparities.  The loads
// of kLineConfBatch views are issued together, unconditionally and with clamped addresses, before the first is used.
#pragma once

#include "k2_scan.hpp"

namespace rslf {

constexpr int kLineConfBatch = 8;   // views whose column value and two taps a pixel has in flight together

struct LineConfArgs {
    int V, S, U, s_hat;
    const float* Ce_svu;       // [S][V][U] edge confidence as it stands (earlier scans have zeroed rejected pixels)
    float* K_vsu;              // [V][S][U] persistent kernel columns (not restrict: the rescan writes what the sums read)
    const float* depth_vu;     // [V][U] the FILTERED disparities of the visit (core.hpp:892)
    const uint8_t* mask_vu;    // [V][U] edge mask of the visited view after the scan's rejections
    float* Cl_vu;              // [V][U] out, written where the mask is set
};

// `idx_vu` (nullable): the visit's arg-max plane; with it `a` holds the scan's arguments (volume, ranges, constants).
template <int C>
__global__ __launch_bounds__(256) void k7_line_confidence(LineConfArgs q, ScanArgs a, const int32_t* __restrict__ idx_vu)
{
    const int v = blockIdx.y;
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= q.U)
        return;
    const long long o = (long long)v * q.U + u;
    float* Kcol = q.K_vsu + (long long)v * q.S * q.U + u;   // element s at Kcol[s * U]
    if (idx_vu) {
        const int d = idx_vu[o];
        if (d >= 0) {   // core.hpp:647-651: scanned and accepted now
            Best<C> best;
            best.init();
            scan_generic_body<C>(a, v, u, d, d + 1, best, Kcol, (long long)q.U);
        }
    }
    if (!q.mask_vu[o])   // core.hpp:1079
        return;
    const int Um1 = q.U - 1;
    const long long plane = (long long)q.V * q.U;
    const float* ce_v = q.Ce_svu + (long long)v * q.U;
    // core.hpp:1058: `S * row + U` is one MatExpr, gemm(S, row, 1, U, 1), which accumulates float data in double and
    // rounds once: I = (float)((double)(s_hat - s) * (double)depth + (double)u)
    const double dd = (double)q.depth_vu[o];
    const double ud = (double)u;
    float A = 0.0f, B = 0.0f;
    constexpr int N = kLineConfBatch;
    for (int s0 = 0; s0 < q.S; s0 += N) {
        float k[N], e0[N], e1[N], t[N];
        bool valid[N];
#pragma unroll
        for (int j = 0; j < N; j++) {
            const int s = min(s0 + j, q.S - 1);
            k[j] = Kcol[(long long)s * q.U];
            double x = (double)(q.s_hat - s) * dd;
            x = x + ud;
            const float I = (float)x;
            const bool ok = fabsf(I) < 2.0e9f;   // false for NaN: no conversion of a value an int cannot hold
            const float fl = floorf(I);
            const int i0 = ok ? (int)fl : -1;            // interp.hpp:179-181
            const int i1 = ok ? (int)ceilf(I) : -1;
            t[j] = I - fl;
            valid[j] = ok && !(i0 < 0 || i1 > Um1);      // interp.hpp:182
            const float* row = ce_v + (long long)s * plane;
            e0[j] = row[min(max(i0, 0), Um1)];
            e1[j] = row[min(max(i1, 0), Um1)];
        }
#pragma unroll
        for (int j = 0; j < N; j++) {
            if (s0 + j >= q.S)
                break;
            const float m0 = (1.0f - t[j]) * e0[j];
            const float m1 = t[j] * e1[j];
            float E = m0 + m1;                            // interp.hpp:184
            E = valid[j] ? E : NAN;                       // interp.hpp:189
            E = (E > 0.0f) ? E : 0.0f;                    // cv::max(E, 0), NaN -> 0   core.hpp:1071
            const float pr = E * k[j];                    // core.hpp:1074
            A = A + pr;                                   // core.hpp:1075
            B = B + k[j];                                 // core.hpp:1076
        }
    }
    q.Cl_vu[o] = (B != 0.0f) ? (A / B) : 0.0f;            // OpenCV 3.x divide: /0 -> 0   core.hpp:1079
}

}  // namespace rslf
